// What the units of the C ABI glue share (ginsim_api.hip, api_series.hip, api_mc.hip, api_traj.hip): the context, the two macros every
// entry point reports its failures with, and the context's scratch regions.  Internal: nothing but those four files includes it.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "ginsim.h"
#include "comm.hpp"
#include "launch.hpp"

struct ginsim_ctx {
    int device;
    hipStream_t stream;
    hipEvent_t ev0, ev1;
    std::vector<hipEvent_t> pool;   // lazily created, indexed by slot
    void* ws[4] = {nullptr, nullptr, nullptr, nullptr};   // grow-only scratch regions, one per Scratch slot (below)
    size_t ws_bytes[4] = {0, 0, 0, 0};
    double* series_host = nullptr;                        // pinned host memory the finishing launches of the series analyses (Allan,
    size_t series_host_doubles = 0;                       // overlapping Allan, PSD, CSD, cascade) write their results into
    int max_grid_y = 65535;                               // the device's maxGridSize[1]: the series analyses have the series (CSD: the pairs) there
    ginsim::Comm* comm = nullptr;                         // RCCL communicator of this rank (ginsim_comm_init), or nullptr
    double* comm_recv = nullptr;                          // device [8 slots][nranks][28]: the gathered records
    ginsim_stats* comm_host = nullptr;                    // pinned host copy of the same
    hipEvent_t comm_ev[8] = {};
    bool comm_pending[8] = {};
    ginsim_stats* stat_slots = nullptr;                   // pinned host records of ginsim_end_stats_begin/_finish
    hipEvent_t stat_ev[8] = {};
    bool stat_pending[8] = {};
    unsigned long long* selftest = nullptr;               // device [3]: the results of ginsim_pattern_check / ginsim_digest (kept: a
                                                          // hipMalloc + hipFree per call would flush stale translations, csrc/placed.hip)
};

// The context's scratch regions.  Every user of a slot launches on the context's one stream and has read what it needs of the
// region, in stream order, before the next user's launch writes it; two calls share a slot unless one holds its region while it
// makes the other.
enum Scratch {
    WS_STATS = 0,    // the end-point statistics: a call may reduce what a WS_TRAJ call (ginsim_end_stats_from_traj) still holds
    WS_SERIES = 1,   // the five series analyses: records and level buffers, dead once the call's finishing launch has run
    WS_TRAJ = 2,     // the readers of kept trajectories (process statistics, curves, keys, quantiles, covariance) and the XCC probe:
                     // each synchronises before it returns
    WS_MC = 3,       // what a Monte-Carlo, filter or PSD-vibration launch uses besides its parameter block (converted truth, carries,
                     // stamps, transform buffers): dead when that launch ends
};

// grow-only scratch owned by the context: avoids a hipMalloc/hipFree pair (~100 us each) per call (ginsim_api.hip; hidden: the
// glue's own, and its mangled name would read like an export of the C ABI)
__attribute__((visibility("hidden"))) hipError_t scratch(ginsim_ctx* c, Scratch slot, size_t bytes, void** out);

#define HIP_TRY(expr)                                                                         \
    do {                                                                                      \
        hipError_t e_ = (expr);                                                               \
        if (e_ != hipSuccess) {                                                               \
            ginsim::set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
            if (e_ == hipErrorOutOfMemory) { (void)hipGetLastError(); return GINSIM_ERR_NOMEM; } \
            return GINSIM_ERR_HIP;                                                            \
        }                                                                                     \
    } while (0)

#define REQUIRE(cond, ...)                    \
    do {                                      \
        if (!(cond)) {                        \
            ginsim::set_error(__VA_ARGS__);   \
            return GINSIM_ERR_ARG;            \
        }                                     \
    } while (0)

// RAII device allocation for the host-buffer entry points
struct DevBuf {
    void* p = nullptr;
    ~DevBuf() { if (p) (void)hipFree(p); }
    hipError_t alloc(size_t bytes) { return hipMalloc(&p, bytes ? bytes : 8); }
    template <class T> T* as() const { return reinterpret_cast<T*>(p); }
};
