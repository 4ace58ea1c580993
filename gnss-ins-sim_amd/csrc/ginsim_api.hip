// C ABI of libginsim.so (declared in include/ginsim.h): context handling, argument validation, error
// reporting and the host-buffer convenience entry points.  No kernels here.
#include <hip/hip_runtime.h>
#include <chrono>

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "ginsim.h"
#include "ginsim_oallan.h"
#include "ginsim_psd.h"
#include "ginsim_lpsd.h"
#include "ginsim_csd.h"
#include "ginsim_loose_all.h"
#include "ginsim_loose_all_cons.h"
#include "allan.hpp"
#include "oallan.hpp"
#include "psd.hpp"
#include "lpsd.hpp"
#include "csd.hpp"
#include "comm.hpp"
#include "launch.hpp"
#include "placed.hpp"

namespace ginsim {

static thread_local std::string g_err;

void set_error(const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_err = buf;
}

}  // namespace ginsim

using namespace ginsim;

struct ginsim_ctx {
    int device;
    hipStream_t stream;
    hipEvent_t ev0, ev1;
    std::vector<hipEvent_t> pool;   // lazily created, indexed by slot
    void* ws[4] = {nullptr, nullptr, nullptr, nullptr};   // grow-only scratch regions (stats / allan)
    size_t ws_bytes[4] = {0, 0, 0, 0};
    double* allan_host = nullptr;                         // pinned host memory the Allan kernels write their sums into
    size_t allan_host_doubles = 0;
    int max_grid_y = 65535;                               // the device's maxGridSize[1]: the Allan kernels have the series there
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

// grow-only scratch owned by the context: avoids a hipMalloc/hipFree pair (~100 us each) per call
static hipError_t scratch(ginsim_ctx* c, int slot, size_t bytes, void** out) {
    if (c->ws_bytes[slot] < bytes) {
        if (c->ws[slot]) {
            hipError_t e = hipStreamSynchronize(c->stream);
            if (e != hipSuccess) return e;
            e = hipFree(c->ws[slot]);
            if (e != hipSuccess) return e;
            c->ws[slot] = nullptr;
            c->ws_bytes[slot] = 0;
        }
        const size_t want = bytes + bytes / 4 + 4096;
        hipError_t e = hipMalloc(&c->ws[slot], want);
        if (e != hipSuccess) return e;
        c->ws_bytes[slot] = want;
    }
    *out = c->ws[slot];
    return hipSuccess;
}

#define HIP_TRY(expr)                                                                         \
    do {                                                                                      \
        hipError_t e_ = (expr);                                                               \
        if (e_ != hipSuccess) {                                                               \
            set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
            if (e_ == hipErrorOutOfMemory) { (void)hipGetLastError(); return GINSIM_ERR_NOMEM; } \
            return GINSIM_ERR_HIP;                                                            \
        }                                                                                     \
    } while (0)

#define REQUIRE(cond, ...)            \
    do {                              \
        if (!(cond)) {                \
            set_error(__VA_ARGS__);   \
            return GINSIM_ERR_ARG;    \
        }                             \
    } while (0)

// RAII device allocation for the host-buffer entry points
struct DevBuf {
    void* p = nullptr;
    ~DevBuf() { if (p) (void)hipFree(p); }
    hipError_t alloc(size_t bytes) { return hipMalloc(&p, bytes ? bytes : 8); }
    template <class T> T* as() const { return reinterpret_cast<T*>(p); }
};

// The selected runs of a device-resident series as [nsel][n][ncomp] doubles on the host: the body of the three ginsim_gather_*
// entry points.  launch(ids, out): the gather kernel of the series' layout and precision, on device copies.
template <class Launch>
static int gather_run(const char* who, ginsim_ctx* c, const void* series, int32_t ncomp, int64_t n, int64_t runs, const int64_t* run_ids,
                      int32_t nsel, double* host_out, Launch launch) {
    REQUIRE(c && series && run_ids && host_out, "%s: NULL argument", who);
    REQUIRE(ncomp >= 1 && n >= 1 && runs >= 1 && nsel >= 1, "%s: bad sizes", who);
    for (int i = 0; i < nsel; ++i)
        REQUIRE(run_ids[i] >= 0 && run_ids[i] < runs, "%s: run id %lld out of range", who, (long long)run_ids[i]);
    HIP_TRY(hipSetDevice(c->device));
    DevBuf ids, out;
    const size_t out_bytes = sizeof(double) * (size_t)nsel * n * ncomp;
    HIP_TRY(ids.alloc(sizeof(int64_t) * nsel));
    HIP_TRY(out.alloc(out_bytes));
    HIP_TRY(hipMemcpyAsync(ids.p, run_ids, sizeof(int64_t) * nsel, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(launch(ids.as<int64_t>(), out.as<double>()));
    HIP_TRY(hipMemcpyAsync(host_out, out.p, out_bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return GINSIM_OK;
}

// One launch over kept trajectories at requested samples (curve_entry, keys_entry, cov_entry below), on checked input; v.samples
// is still on the host.  Scratch: [body bytes: the family's records, then its slice records and shifts]
// [m sample indices].  launch(view with the samples on the device, scratch); out_bytes from the front of the scratch to the host.
template <class Launch>
static int traj_run(ginsim_ctx* c, TrajView v, size_t body, double* host_out, size_t out_bytes, Launch launch) {
    HIP_TRY(hipSetDevice(c->device));
    void* ws = nullptr;
    HIP_TRY(scratch(c, 2, body + sizeof(int64_t) * (size_t)v.m, &ws));
    if (v.samples) {
        int64_t* d_samples = reinterpret_cast<int64_t*>(reinterpret_cast<char*>(ws) + body);
        HIP_TRY(hipMemcpyAsync(d_samples, v.samples, sizeof(int64_t) * (size_t)v.m, hipMemcpyHostToDevice, c->stream));
        v.samples = d_samples;
    }
    HIP_TRY(launch(v, ws));
    if (out_bytes) HIP_TRY(hipMemcpyAsync(host_out, ws, out_bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return GINSIM_OK;
}

// What one Allan call runs: the averaging factors of allan.py:29-43, the decade levels, and for every level the kernel form that
// takes it.  Host arithmetic only; ginsim_allan launches from it and ginsim_allan_plan reports it, so the two cannot differ.
struct AllanStep { int k; int mode; };     // mode 0: allan_level_kernel, 1: wave-pair LDS-DMA kernel, 2: levels k and k+1 fused
struct AllanPlan {
    std::vector<int64_t> mult;             // the averaging factors; empty = the series is shorter than 9 s
    int levels = 0;
    std::vector<AllanLevel> lvs;
    AllanFold fold;
    int64_t records = 0;
    std::vector<AllanStep> steps;
    std::vector<int32_t> mode, chunks_per_block, nparts;       // per level, as ginsim_allan_level reports them
};

// The averaging factors exactly as allan.py:29-43 (none: the series is shorter than 9 s); returns the number of decades.
static int allan_factors(int64_t n, double fs, std::vector<int64_t>& mult, int64_t* mmax_out) {
    const double ts = 1.0 / fs;
    const int64_t mmax = *mmax_out = (int64_t)floor((double)n / 9.0);
    if ((double)mmax * ts < 1.0) return 0;
    const int decades = (int)ceil(log10((double)mmax));
    double scale = 0.1;
    for (int i = 0; i < decades; ++i) {
        scale *= 10;
        for (int j = 1; j < 10; ++j) {
            const int64_t m = (int64_t)(j * scale);
            if (m > mmax) break;
            mult.push_back(m);
        }
    }
    return decades;
}

static int allan_plan(const double* x, int64_t n, int32_t nseries, int64_t series_stride, double fs, AllanPlan& P) {
    REQUIRE(n >= 1 && nseries >= 1 && series_stride >= n && fs > 0, "allan: bad sizes");
    int64_t mmax = 0;
    const int decades = allan_factors(n, fs, P.mult, &mmax);
    if ((double)mmax * (1.0 / fs) < 1.0) return GINSIM_OK;
    const int levels = P.levels = decades;
    // levels of more than one chunk: per-wavefront / per-workgroup partial sums; ONE launch at the end folds them and runs
    // the levels of at most one chunk (the last three or four).  Where the level's rows are 16-byte aligned the
    // LDS-DMA wave-pair kernel takes the level, otherwise the register-staged one.
    std::vector<AllanLevel>& lvs = P.lvs;
    lvs.resize(levels);
    AllanFold& fold = P.fold;
    fold.nlevels = 0;
    fold.fused_level = -1;
    fold.pad = 0;
    for (int j = 0; j < 9; ++j) fold.fused_nb[j] = 0;
    int64_t& records = P.records;
    std::vector<AllanStep>& steps = P.steps;
    P.mode.assign(levels, 4);
    P.chunks_per_block.assign(levels, 1);
    P.nparts.assign(levels, 1);
    {
        int64_t n_in = n, stride_in = series_stride, pow10 = 1;
        for (int k = 0; k < levels; ++k) {
            AllanLevel& lv = lvs[k];
            lv.n_in = n_in;
            lv.n_out = (k + 1 < levels) ? n_in / 10 : 0;
            lv.in_stride = stride_in;
            lv.out_stride = lv.n_out;
            for (int j = 1; j <= 9; ++j) lv.nb[j - 1] = (j * pow10 <= mmax) ? n / (j * pow10) : 0;
            lv.nchunks = allan_chunks(n_in);
            lv.chunks_per_block = allan_chunks_per_block((int64_t)lv.nchunks * nseries);
            stride_in = lv.n_out;
            n_in = lv.n_out;
            pow10 *= 10;
        }
        int k = 0;
        if (levels >= 2 && lvs[0].n_in > allan_chunk_entries() && allan_fuse_applies(x, lvs[0], lvs[1])) {
            // levels 0 and 1 in one launch: the entries of level 1 never leave the chip (round 5; csrc/allan.hip)
            const int parts = allan_fuse_parts(lvs[0]);
            fold.nparts[0] = parts;
            fold.offset[0] = records;
            records += (int64_t)parts * nseries;
            fold.nparts[1] = parts;
            fold.offset[1] = records;
            records += (int64_t)parts * nseries * (allan_fuse_record() / 9);
            fold.fused_level = 1;
            for (int j = 0; j < 9; ++j) fold.fused_nb[j] = lvs[1].nb[j];
            steps.push_back(AllanStep{0, 2});
            P.mode[0] = 2;
            P.mode[1] = 3;
            P.chunks_per_block[0] = allan_fuse_chunks();
            P.nparts[0] = P.nparts[1] = parts;
            k = 2;
        }
        while (k < levels && lvs[k].n_in > allan_chunk_entries()) {
            REQUIRE(k < 8, "allan: series too long");
            AllanLevel& lv = lvs[k];
            // intermediate levels live in this call's scratch region, whose rows start 256-byte aligned
            const bool dma = allan_dma_applies(k == 0 ? x : reinterpret_cast<const double*>(uintptr_t(256)), lv);
            int parts;
            if (dma) {      // four workgroups per CU: ~1024 in flight; up to 8 chunks each so that the first, exposed load is amortised
                // a level that fits ONE round of resident workgroups (1024) with at most 16 chunks each runs as one (a second,
                // partly filled round costs a whole workgroup time: 144 000 entries x 192 series 62 -> 51 us); longer levels
                // in runs of 8 chunks
                static const int cap = [] { const char* e = getenv("GINSIM_ALLAN_CPB"); return e && atoi(e) > 0 ? atoi(e) : 8; }();
                const int64_t total = (int64_t)lv.nchunks * nseries;
                const int64_t max_parts = nseries <= 1024 ? 1024 / nseries : 1;         // workgroups per series in one round
                const int64_t fit = (lv.nchunks + max_parts - 1) / max_parts;
                const bool single = fit <= 16;
                const int64_t per = single ? fit : total / 4096;
                const int64_t lim = single ? 16 : cap;
                lv.chunks_per_block = (int32_t)(per < 1 ? 1 : (per > lim ? lim : per));
                parts = allan_pair_parts(lv);
            } else {
                parts = allan_parts(lv);
            }
            fold.nparts[k] = parts;
            fold.offset[k] = records;
            records += (int64_t)parts * nseries;
            steps.push_back(AllanStep{k, dma ? 1 : 0});
            P.mode[k] = dma ? 1 : 0;
            P.chunks_per_block[k] = lv.chunks_per_block;
            P.nparts[k] = parts;
            ++k;
        }
        fold.nlevels = k;
    }
    REQUIRE(levels - fold.nlevels <= 4, "allan: internal level plan");
    return GINSIM_OK;
}

// What one overlapping-Allan call runs: the same factors, the first `tile` of them in the tile form (2m <= H, ascending m), the
// others in the stream form, and the scratch it takes.  ginsim_oallan launches from it and ginsim_oallan_plan reports it.
struct OallanPlan {
    OallanFactors F;
    int tile = 0;
    int64_t theta_stride = 0;
    size_t b_records = 0, b_theta = 0, b_sums = 0;
};

static int oallan_plan(int64_t n, int32_t nseries, int64_t series_stride, double fs, OallanPlan& P) {
    REQUIRE(n >= 1 && nseries >= 1 && series_stride >= n && fs > 0 && std::isfinite(fs), "oallan: bad sizes");
    OallanFactors& F = P.F;
    memset(&F, 0, sizeof(F));
    std::vector<int64_t> mult;
    int64_t mmax = 0;
    allan_factors(n, fs, mult, &mmax);
    if (mult.empty()) return GINSIM_OK;
    REQUIRE((int)mult.size() <= kOallanMaxFactors && n < ((int64_t)1 << 31), "oallan: series too long");
    const char* e = getenv("GINSIM_OALLAN_TILE");           // read per call: 0 sends every factor through the stream form
    const bool tiles = !(e && e[0] == '0' && e[1] == 0);
    const int64_t C = oallan_tile_payload(), H = oallan_tile_halo(), W = oallan_stream_item();
    F.count = (int32_t)mult.size();
    int64_t records = 0;
    for (int i = 0; i < F.count; ++i) {
        const int64_t m = mult[i], terms = n - 2 * m + 1;   // n / m >= 9: terms > 0
        const bool tile = tiles && 2 * m <= H && i == P.tile && P.tile < kOallanTileFactors;
        if (tile) ++P.tile;
        const int64_t per = tile ? C : W;
        F.m[i] = (int32_t)m;
        F.nparts[i] = (int32_t)((terms + per - 1) / per);
        F.offset[i] = (int32_t)records;
        records += F.nparts[i];
    }
    F.records = (int32_t)records;
    const auto pad = [](size_t b) { return (b + 255) & ~(size_t)255; };
    P.b_records = pad(sizeof(double) * (size_t)records * (size_t)nseries);
    if (F.count > P.tile) {
        P.theta_stride = (n + 2) & ~(int64_t)1;             // theta[0 .. n], rows 16-byte aligned
        P.b_theta = pad(sizeof(double) * (size_t)P.theta_stride * (size_t)nseries);
        P.b_sums = pad(sizeof(double) * (size_t)(n / oallan_scan_chunk() + 1) * (size_t)nseries);
    }
    return GINSIM_OK;
}

// What one Welch call runs (psd.hpp): the refusals that ginsim_psd_welch and ginsim_psd_plan share, in the order
// include/ginsim_psd.h states and under the caller's prefix -- the arguments first (the call checks its window and detrend between
// the two), then the series against one segment, then the shape against what a launch and the geometry can state (psd.hpp keeps
// nparts in 64 bits until here).
static int psd_check(const char* who, int64_t n, int32_t nseries, int64_t series_stride, double fs, int32_t nperseg, int32_t step) {
    REQUIRE(n >= 1 && nseries >= 1 && series_stride >= n && fs > 0 && std::isfinite(fs), "%s: bad sizes", who);
    REQUIRE(nperseg >= (1 << kPsdMinLog2) && nperseg <= (1 << kPsdMaxLog2) && (nperseg & (nperseg - 1)) == 0,
            "%s: nperseg %d is not a power of two in [%d, %d]", who, (int)nperseg, 1 << kPsdMinLog2, 1 << kPsdMaxLog2);
    REQUIRE(step >= 1 && step <= nperseg, "%s: step %d outside [1, %d]", who, (int)step, (int)nperseg);
    return GINSIM_OK;
}

static int psd_plan(const char* who, int64_t n, int32_t nseries, int32_t nperseg, int32_t step, PsdShape& S) {
    if (n < nperseg) {
        set_error("%s: a series of n = %lld samples is shorter than one segment of nperseg = %d", who, (long long)n, (int)nperseg);
        return GINSIM_ERR_RANGE;
    }
    // a local: the caller's shape, and behind it ginsim_psd_plan's *g, stays as it was when the call is refused
    PsdShape s = psd_plan_shape(n, nperseg, step);
    if (s.nparts > kPsdMaxParts) {
        set_error("%s: %lld segments in parts of %d are %lld parts per series, more than the %lld a call can have: analyse the series in pieces",
                  who, (long long)s.segments, (int)s.segs_per_part, (long long)s.nparts, (long long)kPsdMaxParts);
        return GINSIM_ERR_RANGE;
    }
    if (!psd_record_bytes(s, nseries)) {
        set_error("%s: the records of %lld parts per series and %d series, %d sums each, pass 2^63 bytes: split the batch or the series",
                  who, (long long)s.nparts, (int)nseries, (int)s.nbins);
        return GINSIM_ERR_RANGE;
    }
    S = s;
    return GINSIM_OK;
}

// What one cascade call runs (lpsd.hpp) and the scratch it takes: the refusals that ginsim_lpsd and ginsim_lpsd_plan share behind
// psd_check and psd_plan of level 0, in the order include/ginsim_lpsd.h states.  S0 is level 0's checked shape (its records hold
// every other level's: fewer parts of the same size).
struct LpsdPlan {
    LpsdLevels lv;
    size_t b_level[2] = {0, 0}, b_records = 0, b_out = 0;
    size_t bytes() const { return b_level[0] + b_level[1] + b_records + b_out; }
};

static int lpsd_plan(const char* who, int64_t n, int32_t nseries, int32_t nperseg, int32_t step, int32_t min_segments,
                     const PsdShape& S0, LpsdPlan& P) {
    REQUIRE(min_segments >= 1, "%s: min_segments %d must be at least 1", who, (int)min_segments);
    if (S0.segments < min_segments) {
        set_error("%s: %lld segments at level 0 are fewer than min_segments = %d", who, (long long)S0.segments, (int)min_segments);
        return GINSIM_ERR_RANGE;
    }
    LpsdPlan p;
    p.lv = lpsd_plan_levels(n, nperseg, step, min_segments);
    p.lv.S[0] = S0;
    if (p.lv.levels > 1 && decimate2_tiles(p.lv.n[1]) > kDecMaxTiles) {
        set_error("%s: level 1 of %lld samples is %lld tiles of %d, more than the %lld a launch can have: analyse the series in pieces",
                  who, (long long)p.lv.n[1], (long long)decimate2_tiles(p.lv.n[1]), kDecTile, (long long)kDecMaxTiles);
        return GINSIM_ERR_RANGE;
    }
    p.b_records = S0.record_bytes;
    p.b_out = (sizeof(double) * (size_t)nseries * (size_t)S0.nbins + 255) & ~(size_t)255;
    for (int j = 1; j <= 2 && j < p.lv.levels; ++j) {
        // nseries n_j doubles, compared by division and never formed past 64 bits; a quarter of the range each leaves the sum exact
        if (p.lv.n[j] > (INT64_MAX / 4 - 255) / (int64_t)sizeof(double) / nseries) {
            set_error("%s: the level buffers of %d series and %lld samples at level %d pass 2^63 bytes: split the batch or the series",
                      who, (int)nseries, (long long)p.lv.n[j], j);
            return GINSIM_ERR_RANGE;
        }
        p.b_level[j - 1] = (sizeof(double) * (size_t)nseries * (size_t)p.lv.n[j] + 255) & ~(size_t)255;
    }
    if (p.b_records > (size_t)INT64_MAX / 4 || p.b_out > (size_t)INT64_MAX / 8) {
        set_error("%s: the scratch of %d series passes 2^63 bytes: split the batch or the series", who, (int)nseries);
        return GINSIM_ERR_RANGE;
    }
    P = p;
    return GINSIM_OK;
}

extern "C" {

int ginsim_abi_version(void) { return GINSIM_ABI_VERSION; }

const char* ginsim_last_error(void) { return g_err.c_str(); }

int ginsim_device_count(int* count) {
    REQUIRE(count, "device_count: NULL output");
    int n = 0;
    const hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) {
        *count = 0;
        set_error("hipGetDeviceCount: %s", hipGetErrorString(e));
        return GINSIM_ERR_NODEV;
    }
    *count = n;
    return GINSIM_OK;
}

int ginsim_create(int device, ginsim_ctx** out) {
    REQUIRE(out, "create: NULL output");
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n < 1) {
        set_error("no HIP device visible (the engine has no CPU fallback)");
        return GINSIM_ERR_NODEV;
    }
    REQUIRE(device >= 0 && device < n, "create: device %d out of range [0,%d)", device, n);
    HIP_TRY(hipSetDevice(device));
    ginsim_ctx* c = new ginsim_ctx();
    c->device = device;
    HIP_TRY(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    HIP_TRY(hipEventCreate(&c->ev0));
    HIP_TRY(hipEventCreate(&c->ev1));
    HIP_TRY(hipDeviceGetAttribute(&c->max_grid_y, hipDeviceAttributeMaxGridDimY, device));
    ginsim::placed_context_created(device);
    *out = c;
    return GINSIM_OK;
}

int ginsim_destroy(ginsim_ctx* c) {
    if (!c) return GINSIM_OK;
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    (void)hipEventDestroy(c->ev0);
    (void)hipEventDestroy(c->ev1);
    for (hipEvent_t e : c->pool)
        if (e) (void)hipEventDestroy(e);
    for (void* w : c->ws)
        if (w) (void)hipFree(w);
    for (hipEvent_t e : c->stat_ev)
        if (e) (void)hipEventDestroy(e);
    if (c->stat_slots) (void)hipHostFree(c->stat_slots);
    if (c->allan_host) (void)hipHostFree(c->allan_host);
    if (c->selftest) (void)hipFree(c->selftest);
    if (c->comm) ginsim::comm_destroy(c->comm);
    if (c->comm_recv) (void)hipFree(c->comm_recv);
    if (c->comm_host) (void)hipHostFree(c->comm_host);
    for (hipEvent_t e : c->comm_ev)
        if (e) (void)hipEventDestroy(e);
    ginsim::vib_psd_drop_plans(c->stream);            // this stream's hipFFT plans of the PSD vibration (it is idle now)
    (void)hipStreamDestroy(c->stream);
    ginsim::placed_free_owner(c->device, c);          // regions this context carved and never freed go back to the free list
    ginsim::placed_context_destroyed(c->device);      // the device's last context gives its placed arena back
    delete c;
    return GINSIM_OK;
}

int ginsim_device_name(ginsim_ctx* c, char* buf, size_t cap) {
    REQUIRE(c && buf && cap > 0, "device_name: bad arguments");
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, c->device));
    snprintf(buf, cap, "%s (%s, %d CUs)", prop.name, prop.gcnArchName, prop.multiProcessorCount);
    return GINSIM_OK;
}

int ginsim_malloc(ginsim_ctx* c, size_t bytes, void** dptr) {
    REQUIRE(c && dptr, "malloc: bad arguments");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipMalloc(dptr, bytes ? bytes : 8));
    return GINSIM_OK;
}

// ---- ABI 7: placed device memory (csrc/placed.hip)
int ginsim_placed_configure(ginsim_ctx* c, const ginsim_placed_options* o) {
    REQUIRE(c && o, "placed_configure: bad arguments");
    return ginsim::placed_configure(c->device, *o);
}

int ginsim_placed_reserve(ginsim_ctx* c, size_t bytes) {
    REQUIRE(c, "placed_reserve: NULL context");
    return ginsim::placed_reserve(c->device, c->stream, bytes);
}

int ginsim_malloc_placed(ginsim_ctx* c, size_t bytes, void** dptr) {
    REQUIRE(c && dptr, "malloc_placed: bad arguments");
    return ginsim::placed_malloc(c->device, c->stream, bytes, c, dptr);
}

int ginsim_placed_release(ginsim_ctx* c) {
    REQUIRE(c, "placed_release: NULL context");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return ginsim::placed_release(c->device, false);
}

int ginsim_placed_info_get(ginsim_ctx* c, ginsim_placed_info* out) {
    REQUIRE(c && out, "placed_info_get: bad arguments");
    ginsim::placed_info(c->device, out);
    return GINSIM_OK;
}

int ginsim_mem_info(ginsim_ctx* c, size_t* free_bytes, size_t* total_bytes) {
    REQUIRE(c && free_bytes && total_bytes, "mem_info: bad arguments");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipMemGetInfo(free_bytes, total_bytes));
    return GINSIM_OK;
}

int ginsim_host_alloc(ginsim_ctx* c, size_t bytes, void** hptr) {
    REQUIRE(c && hptr, "host_alloc: bad arguments");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipHostMalloc(hptr, bytes ? bytes : 8, hipHostMallocDefault));
    return GINSIM_OK;
}

int ginsim_host_free(ginsim_ctx* c, void* hptr) {
    // c may be NULL: page-locked arrays handed to a caller can outlive the context that allocated them (hipHostFree needs
    // no stream); with a live context its stream is drained first so that no copy still targets the pages
    if (!hptr) return GINSIM_OK;
    if (c) {
        HIP_TRY(hipSetDevice(c->device));
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    HIP_TRY(hipHostFree(hptr));
    return GINSIM_OK;
}

int ginsim_free(ginsim_ctx* c, void* dptr) {
    REQUIRE(c, "free: NULL context");
    if (!dptr) return GINSIM_OK;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (ginsim::placed_owns(c->device, dptr)) return ginsim::placed_free(c->device, dptr);     // back to the arena's free list
    HIP_TRY(hipFree(dptr));
    return GINSIM_OK;
}

int ginsim_memcpy_h2d(ginsim_ctx* c, void* dst, const void* src, size_t bytes) {
    REQUIRE(c && (bytes == 0 || (dst && src)), "memcpy_h2d: bad arguments");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return GINSIM_OK;
}

int ginsim_memcpy_d2h(ginsim_ctx* c, void* dst, const void* src, size_t bytes) {
    REQUIRE(c && (bytes == 0 || (dst && src)), "memcpy_d2h: bad arguments");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return GINSIM_OK;
}

int ginsim_memset(ginsim_ctx* c, void* dptr, int value, size_t bytes) {
    REQUIRE(c && (bytes == 0 || dptr), "memset: bad arguments");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipMemsetAsync(dptr, value, bytes, c->stream));
    return GINSIM_OK;
}

int ginsim_sync(ginsim_ctx* c) {
    REQUIRE(c, "sync: NULL context");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return GINSIM_OK;
}

int ginsim_timer_begin(ginsim_ctx* c) {
    REQUIRE(c, "timer_begin: NULL context");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipEventRecord(c->ev0, c->stream));
    return GINSIM_OK;
}

int ginsim_timer_end(ginsim_ctx* c, float* ms) {
    REQUIRE(c && ms, "timer_end: bad arguments");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipEventRecord(c->ev1, c->stream));
    HIP_TRY(hipEventSynchronize(c->ev1));
    HIP_TRY(hipEventElapsedTime(ms, c->ev0, c->ev1));
    return GINSIM_OK;
}

int ginsim_event_record(ginsim_ctx* c, int32_t slot) {
    REQUIRE(c && slot >= 0 && slot < GINSIM_MAX_EVENTS, "event_record: slot out of range");
    HIP_TRY(hipSetDevice(c->device));
    if ((size_t)slot >= c->pool.size()) c->pool.resize(slot + 1, nullptr);
    if (!c->pool[slot]) HIP_TRY(hipEventCreate(&c->pool[slot]));
    HIP_TRY(hipEventRecord(c->pool[slot], c->stream));
    return GINSIM_OK;
}

int ginsim_event_elapsed(ginsim_ctx* c, int32_t a, int32_t b, float* ms) {
    REQUIRE(c && ms && a >= 0 && b >= 0 && (size_t)a < c->pool.size() && (size_t)b < c->pool.size() && c->pool[a] &&
                c->pool[b], "event_elapsed: slots were not recorded");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipEventSynchronize(c->pool[b]));
    HIP_TRY(hipEventElapsedTime(ms, c->pool[a], c->pool[b]));
    return GINSIM_OK;
}

static int check_sensor(const ginsim_sensor_model& m, const char* what) {
    for (int i = 0; i < 3; ++i) {
        const double v[4] = {m.bias[i], m.gm_a[i], m.gm_b[i], m.white[i]};
        for (double x : v) REQUIRE(x == x && x - x == 0.0, "mc_run: %s model has a non-finite coefficient", what);
    }
    return GINSIM_OK;
}

// The checks that the parameter blocks of several entry points share.  who: the prefix of the messages.
static int check_sizes(const char* who, const ginsim_mc_params* m) {
    REQUIRE(m->n >= 1 && m->runs >= 1, "%s: n=%lld runs=%lld must be >= 1", who, (long long)m->n, (long long)m->runs);
    REQUIRE(m->n <= 0xFFFFFFFFll, "%s: n exceeds the 32-bit sample counter of the RNG", who);
    REQUIRE(m->runs <= (int64_t)0x7FFFFFFF * 64, "%s: too many runs for one launch", who);
    return GINSIM_OK;
}

// Where the samples of the inclinometer and the filter kernel come from: the given series, or the truth and the two sensor models.
// gps_in / gps_ref: the fixes of that source are there (true where the kernel takes none).
static int check_sensor_source(const char* who, const ginsim_mc_params* m, bool gps_in, bool gps_ref) {
    if (m->given_sensors) {
        REQUIRE(m->in_accel && m->in_gyro, "%s: given_sensors needs in_accel and in_gyro", who);
        REQUIRE(gps_in, "%s: given_sensors needs in_gps", who);
        return GINSIM_OK;
    }
    REQUIRE(m->ref_gyro && m->ref_accel, "%s: ref_accel/ref_gyro missing", who);
    REQUIRE(gps_ref, "%s: ref_gps missing", who);
    const int rc = check_sensor(m->accel, "accel");
    return rc ? rc : check_sensor(m->gyro, "gyro");
}

// the vibration terms of the kernels without the 'psd' form; noun: "inclinometer" / "filter"
static int check_vibration_no_psd(const char* who, const ginsim_mc_params* m, const char* noun) {
    for (const ginsim_vibration* v : {&m->vib_accel, &m->vib_gyro}) {
        if (v->type == GINSIM_VIB_NONE) continue;
        REQUIRE(v->type == GINSIM_VIB_RANDOM || v->type == GINSIM_VIB_SINUSOIDAL,
                "%s: the %s kernel takes the 'random' and 'sinusoidal' vibration only", who, noun);
        REQUIRE(!m->given_sensors, "%s: a vibration term cannot be added to given sensors", who);
        REQUIRE(std::isfinite(v->amp[0]) && std::isfinite(v->amp[1]) && std::isfinite(v->amp[2]) && std::isfinite(v->omega_dt),
                "%s: vibration amplitudes / frequency must be finite", who);
    }
    return GINSIM_OK;
}

static int check_mc_params(const ginsim_mc_params* p) {
    REQUIRE(p, "mc_run: NULL argument");
    int rc = check_sizes("mc_run", p);
    if (rc) return rc;
    REQUIRE(p->fs > 0.0, "mc_run: fs must be positive");
    REQUIRE(p->ref_frame == 0 || p->ref_frame == 1, "mc_run: ref_frame must be 0 or 1");
    REQUIRE(p->proc_plain_sums == 0 || p->proc_plain_sums == 1, "mc_run: proc_plain_sums must be 0 or 1");
    REQUIRE(p->algo_mask >= 0 && p->algo_mask <= 3, "mc_run: algo_mask must be a combination of GINSIM_ALGO_*");
    REQUIRE(p->algo_mask != 0 || (!p->given_sensors && (p->out_accel || p->out_gyro || p->out_odo)),
            "mc_run: algo_mask 0 (sensors only) needs sensor outputs");
    REQUIRE(p->algo_mask == 0 || (p->n_ini >= 1 && p->ini), "mc_run: initial-state table missing");
    REQUIRE(p->block_threads == 0 || p->block_threads == 64 || p->block_threads == 128 || p->block_threads == 256,
            "mc_run: block_threads must be 0, 64, 128 or 256");
    const bool odo = (p->algo_mask & GINSIM_ALGO_ODO) != 0, fre = (p->algo_mask & GINSIM_ALGO_FREE) != 0;
    if (p->given_sensors) {
        REQUIRE(p->in_gyro, "mc_run: given_sensors needs in_gyro");
        REQUIRE(!fre || p->in_accel, "mc_run: given_sensors free integration needs in_accel");
        REQUIRE(!odo || p->in_odo, "mc_run: given_sensors odometer integration needs in_odo");
    } else {
        REQUIRE(p->ref_gyro && p->ref_accel, "mc_run: ref_accel/ref_gyro missing");
        REQUIRE((!odo && !p->out_odo) || p->ref_odo, "mc_run: ref_odo missing");
        rc = check_sensor(p->accel, "accel");
        if (rc) return rc;
        rc = check_sensor(p->gyro, "gyro");
        if (rc) return rc;
    }
    for (const ginsim_vibration* v : {&p->vib_accel, &p->vib_gyro}) {
        REQUIRE(v->type == GINSIM_VIB_NONE || v->type == GINSIM_VIB_RANDOM || v->type == GINSIM_VIB_SINUSOIDAL || v->type == GINSIM_VIB_PSD,
                "mc_run: vibration type must be 0 (none), 1 (random), 2 (sinusoidal) or 3 (psd)");
        if (v->type == GINSIM_VIB_NONE) continue;
        REQUIRE(!p->given_sensors, "mc_run: a vibration term cannot be added to given sensors");
        if (v->type == GINSIM_VIB_PSD) {
            REQUIRE(v->series && v->period >= 2 && v->period <= 16384, "mc_run: a psd vibration needs its series (ginsim_vib_psd_series) and their period (2 .. 16384)");
            REQUIRE(p->precision == 0, "mc_run: the psd vibration runs on the fp64 kernels only");
            REQUIRE(p->sensor_layout == 0, "mc_run: the psd vibration runs on the lane-per-run kernels only (sensor_layout 0)");
        }
        REQUIRE(std::isfinite(v->amp[0]) && std::isfinite(v->amp[1]) && std::isfinite(v->amp[2]) && std::isfinite(v->omega_dt),
                "mc_run: vibration amplitudes / frequency must be finite");
    }
    REQUIRE(p->precision == 0 || p->precision == 1, "mc_run: precision must be 0 (fp64) or 1 (fp32)");
    REQUIRE(p->sensor_layout == 0 || p->sensor_layout == 1, "mc_run: sensor_layout must be 0 ([axis][sample][run]) or 1 ([run][axis][sample])");
    REQUIRE(p->sensor_layout == 0 || series_path_applies(*p),
            "mc_run: sensor_layout 1 is written by the time-parallel series kernels only (sensors only, fp64, <= 1024 runs, >= 2048 samples)");
    if (p->out_proc[0] || p->out_proc[1]) {
        REQUIRE(!p->given_sensors && p->precision == 0, "mc_run: online process statistics need generate mode and fp64");
        REQUIRE((p->algo_mask == GINSIM_ALGO_FREE && p->out_proc[0] && !p->out_proc[1]) ||
                (p->algo_mask == GINSIM_ALGO_ODO && p->out_proc[1] && !p->out_proc[0]),
                "mc_run: online process statistics take ONE algorithm per launch (out_proc of that algorithm only)");
        REQUIRE(p->ref_nav, "mc_run: online process statistics need ref_nav");
        REQUIRE(p->proc_first >= 0 && p->proc_first < p->n, "mc_run: proc_first out of range");
        REQUIRE(!p->proc_pos_ned || p->ref_frame == 0, "mc_run: NED position errors exist in ref_frame 0 only");
    }
    REQUIRE(!(p->out_end_ned[0] || p->out_end_ned[1]) || (p->ref_frame == 0 && p->precision == 0 && !p->given_sensors),
            "mc_run: out_end_ned needs ref_frame 0, fp64, generate mode");
    if (p->precision == 1) {
        REQUIRE(p->algo_mask != 0, "mc_run: the fp32 kernel needs an algorithm");
        REQUIRE(!(p->out_proc[0] || p->out_proc[1] || p->out_end_ned[0] || p->out_end_ned[1] || p->wave_trace),
                "mc_run: the fp32 kernel has no online process statistics, NED record or wave trace");
        REQUIRE(p->block_threads == 0 || p->block_threads == 256, "mc_run: the fp32 kernel takes block_threads 0 or 256 (256 = the plain kernel)");
    }
    return GINSIM_OK;
}

int ginsim_mc_variant(const ginsim_mc_params* p, int32_t* variant) {
    REQUIRE(p && variant, "mc_variant: NULL argument");
    *variant = p->precision == 1 ? mc_variant_f32(*p) : (series_path_applies(*p) ? 2 : mc_variant(*p));
    return GINSIM_OK;
}

int ginsim_mc_kernel_name(const ginsim_mc_params* p, char* buf, size_t cap) {
    REQUIRE(p && buf && cap > 0, "mc_kernel_name: bad arguments");
    const int rc = check_mc_params(p);
    if (rc) return rc;
    buf[0] = 0;
    if (p->precision == 1) (void)launch_mc_f32(*p, nullptr, nullptr, buf, cap);
    else if (series_path_applies(*p))       // the dominant one of series_kernel<0>, series_scan_kernel, series_kernel<1 | 2>
        snprintf(buf, cap, "ginsim::series_kernel<%d>", series_pass_b(*p));
    else (void)launch_mc(*p, nullptr, buf, cap, nullptr);
    REQUIRE(buf[0], "mc_kernel_name: no kernel serves these parameters");
    return GINSIM_OK;
}

int ginsim_mc_run(ginsim_ctx* c, const ginsim_mc_params* p) {
    REQUIRE(c, "mc_run: NULL argument");
    const int rc0 = check_mc_params(p);
    if (rc0) return rc0;
    HIP_TRY(hipSetDevice(c->device));
    if (p->precision == 1) {
        void* truth32 = nullptr;       // the wave-specialised fp32 kernel reads its truth as floats (converted by a pre-launch)
        const size_t tb = mc_f32_truth_bytes(*p);
        if (tb) HIP_TRY(scratch(c, 3, tb, &truth32));
        HIP_TRY(launch_mc_f32(*p, reinterpret_cast<float*>(truth32), c->stream, nullptr, 0));
    } else if (series_path_applies(*p)) {       // sensors only, few runs, long series: parallel along time
        int32_t L = 0;
        const int64_t nchunks = series_chunks(*p, &L);
        void* carry = nullptr;
        HIP_TRY(scratch(c, 3, sizeof(double) * 6 * (size_t)nchunks * (size_t)p->runs, &carry));
        HIP_TRY(launch_series(*p, reinterpret_cast<double*>(carry), c->stream));
    } else {
        void* about = nullptr;          // the launch-wide shift of the online process statistics (mc_kernel.hip, Proc): nine doubles
        if (p->out_proc[0] || p->out_proc[1]) HIP_TRY(scratch(c, 3, 9 * sizeof(double), &about));
        HIP_TRY(launch_mc(*p, c->stream, nullptr, 0, reinterpret_cast<double*>(about)));
    }
    return GINSIM_OK;
}

static int check_incl_params(const ginsim_mc_params* m, const ginsim_incl_params* p) {
    REQUIRE(m && p, "incl_run: NULL argument");
    int rc = check_sizes("incl_run", m);
    if (rc) return rc;
    REQUIRE(p->algo_mask >= 1 && p->algo_mask <= 3, "incl_run: algo_mask must be a combination of GINSIM_INCL_*");
    REQUIRE(p->n_list >= 0 && p->n_list <= m->runs, "incl_run: n_list must lie in 0 .. runs");
    REQUIRE(!(p->algo_mask & GINSIM_INCL_MAHONY) || p->bias_in, "incl_run: the Mahony filter needs bias_in");
    REQUIRE(std::isfinite(p->dt) && p->dt > 0.0, "incl_run: dt must be positive");
    REQUIRE(m->block_threads == 0 || m->block_threads == 64 || m->block_threads == 128 || m->block_threads == 256,
            "incl_run: block_threads must be 0, 64, 128 or 256");
    REQUIRE(m->precision == 0, "incl_run: the inclinometer kernel is fp64 only");
    rc = check_sensor_source("incl_run", m, true, true);
    if (rc) return rc;
    rc = check_vibration_no_psd("incl_run", m, "inclinometer");
    if (rc) return rc;
    const bool stats = p->out_end[0] || p->out_end[1] || p->out_proc[0] || p->out_proc[1];
    REQUIRE(!stats || m->ref_nav, "incl_run: statistics need ref_nav");
    REQUIRE(!stats || m->proc_first >= 0, "incl_run: proc_first must be >= 0");
    REQUIRE(!(p->out_quat[0] || p->out_euler[0] || p->out_wb || p->out_ab || p->out_end[0] || p->out_proc[0]) ||
            (p->algo_mask & GINSIM_INCL_MAHONY), "incl_run: Mahony outputs without the Mahony bit");
    REQUIRE(!(p->out_quat[1] || p->out_euler[1] || p->out_end[1] || p->out_proc[1]) || (p->algo_mask & GINSIM_INCL_TILT),
            "incl_run: tilt outputs without the tilt bit");
    return GINSIM_OK;
}

int ginsim_incl_variant(const ginsim_mc_params* mc, const ginsim_incl_params* p, int32_t* variant) {
    REQUIRE(variant, "incl_variant: NULL argument");
    const int rc = check_incl_params(mc, p);
    if (rc) return rc;
    *variant = incl_variant(*mc);
    return GINSIM_OK;
}

int ginsim_incl_kernel_name(const ginsim_mc_params* mc, const ginsim_incl_params* p, char* buf, size_t cap) {
    REQUIRE(buf && cap > 0, "incl_kernel_name: bad arguments");
    const int rc = check_incl_params(mc, p);
    if (rc) return rc;
    buf[0] = 0;
    (void)launch_incl(*mc, *p, nullptr, buf, cap);
    return GINSIM_OK;
}

int ginsim_incl_run(ginsim_ctx* c, const ginsim_mc_params* mc, const ginsim_incl_params* p) {
    REQUIRE(c, "incl_run: NULL argument");
    const int rc = check_incl_params(mc, p);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(launch_incl(*mc, *p, c->stream, nullptr, 0));
    return GINSIM_OK;
}

static int check_loose_params(const ginsim_mc_params* m, const ginsim_loose_params* p) {
    REQUIRE(m && p, "loose_run: NULL argument");
    int rc = check_sizes("loose_run", m);
    if (rc) return rc;
    REQUIRE(std::isfinite(m->fs) && m->fs > 0.0, "loose_run: fs must be positive");
    REQUIRE(m->ref_frame == 0 || m->ref_frame == 1, "loose_run: ref_frame must be 0 or 1");
    REQUIRE(m->precision == 0, "loose_run: the filter kernel is fp64 only");
    REQUIRE(m->n_ini >= 1 && m->ini, "loose_run: initial-state table missing");
    REQUIRE(m->block_threads == 0 || m->block_threads == 64, "loose_run: block_threads must be 0 or 64 (one wavefront per workgroup)");
    REQUIRE(p->n_list >= 0 && p->n_list <= m->runs, "loose_run: n_list must lie in 0 .. runs");
    REQUIRE(p->m >= 0 && p->m <= m->n, "loose_run: m=%lld fixes for n=%lld samples", (long long)p->m, (long long)m->n);
    REQUIRE(p->m == 0 || p->gps_stamp, "loose_run: gps_stamp missing");
    for (int64_t k = 0; k < p->m; ++k) {
        const long long s = (long long)p->gps_stamp[k];
        REQUIRE(s >= 0 && s < (long long)m->n, "loose_run: the stamp of fix %lld (%lld) is outside [0, %lld)", (long long)k, s, (long long)m->n);
        REQUIRE(k == 0 || s > (long long)p->gps_stamp[k - 1], "loose_run: the stamps are not strictly increasing at fix %lld", (long long)k);
    }
    rc = check_sensor_source("loose_run", m, p->m == 0 || p->in_gps, p->m == 0 || p->ref_gps);
    if (rc) return rc;
    if (!m->given_sensors)
        for (int k = 0; k < 6; ++k) REQUIRE(std::isfinite(p->gps_sigma[k]), "loose_run: gps_sigma must be finite");
    rc = check_vibration_no_psd("loose_run", m, "filter");
    if (rc) return rc;
    for (int k = 0; k < 6; ++k) REQUIRE(std::isfinite(p->r_diag[k]) && p->r_diag[k] > 0.0, "loose_run: r_diag must be positive");
    for (int k = 0; k < 5; ++k) REQUIRE(std::isfinite(p->p0[k]) && p->p0[k] > 0.0, "loose_run: p0 must be positive");
    for (int k = 0; k < 3; ++k) {
        REQUIRE(std::isfinite(p->q_v[k]) && p->q_v[k] >= 0.0 && std::isfinite(p->q_psi[k]) && p->q_psi[k] >= 0.0 &&
                std::isfinite(p->q_bg[k]) && p->q_bg[k] >= 0.0 && std::isfinite(p->q_ba[k]) && p->q_ba[k] >= 0.0,
                "loose_run: the process noise must be finite and not negative");
        REQUIRE(std::isfinite(p->decay_g[k]) && std::isfinite(p->decay_a[k]), "loose_run: decay_g / decay_a must be finite");
    }
    REQUIRE(!p->out_proc || m->ref_nav, "loose_run: out_proc needs ref_nav");
    REQUIRE(!p->out_proc || (m->proc_first >= 0 && m->proc_first < m->n), "loose_run: proc_first out of range");
    REQUIRE(!m->proc_pos_ned || m->ref_frame == 0, "loose_run: NED position errors exist in ref_frame 0 only");
    REQUIRE(!p->out_end_ned || m->ref_frame == 0, "loose_run: out_end_ned needs ref_frame 0");
    REQUIRE(p->aid_mask >= 0 && p->aid_mask <= 7, "loose_run: aid_mask=%d must lie in 0 .. 7", (int)p->aid_mask);
    if (p->aid_mask != 0) {
        REQUIRE(p->aid_every >= 1, "loose_run: aid_every must be >= 1");
        REQUIRE((p->aid_mask & 6) == 0 || (std::isfinite(p->r_nhc) && p->r_nhc > 0.0), "loose_run: r_nhc must be positive");
        if (p->aid_mask & 1) {
            REQUIRE(std::isfinite(p->r_odo) && p->r_odo > 0.0, "loose_run: r_odo must be positive");
            REQUIRE(std::isfinite(p->odo_scale_f) && p->odo_scale_f > 0.0, "loose_run: odo_scale_f must be positive");
            if (m->given_sensors) {
                REQUIRE(m->in_odo, "loose_run: odometer aiding with given_sensors needs in_odo");
            } else {
                REQUIRE(m->ref_odo, "loose_run: odometer aiding needs ref_odo");
                REQUIRE(std::isfinite(m->odo_scale) && std::isfinite(m->odo_stdv), "loose_run: odo_scale / odo_stdv must be finite");
            }
        }
    }
    return GINSIM_OK;
}

int ginsim_loose_variant(const ginsim_mc_params* mc, const ginsim_loose_params* p, int32_t* variant) {
    REQUIRE(variant, "loose_variant: NULL argument");
    const int rc = check_loose_params(mc, p);
    if (rc) return rc;
    *variant = loose_variant(*mc);
    return GINSIM_OK;
}

// the checkpoint block of a launch whose other two blocks passed check_loose_params
static int check_loose_cons(const ginsim_mc_params* m, const ginsim_loose_params* p, const ginsim_loose_cons_params* q) {
    REQUIRE(q, "loose_cons_run: NULL argument");
    REQUIRE(q->cons_m >= 0, "loose_cons_run: cons_m=%lld must be >= 0", (long long)q->cons_m);
    if (q->cons_m == 0) return GINSIM_OK;
    REQUIRE(q->cons_m <= m->n, "loose_cons_run: cons_m=%lld checkpoints for n=%lld samples", (long long)q->cons_m, (long long)m->n);
    REQUIRE(q->cons_sample && q->out_cons && q->cons_work, "loose_cons_run: cons_sample, out_cons or cons_work missing");
    REQUIRE(m->ref_nav, "loose_cons_run: checkpoints need ref_nav");
    REQUIRE(!p->out_proc, "loose_cons_run: online process statistics (out_proc) and checkpoints in one launch are refused");
    for (int64_t k = 0; k < q->cons_m; ++k) {
        const long long s = (long long)q->cons_sample[k];
        REQUIRE(s >= 0 && s < (long long)m->n, "loose_cons_run: checkpoint %lld (%lld) is outside [0, %lld)", (long long)k, s, (long long)m->n);
        REQUIRE(k == 0 || s > (long long)q->cons_sample[k - 1], "loose_cons_run: the checkpoints are not strictly increasing at %lld", (long long)k);
    }
    return GINSIM_OK;
}

// the magnetometer block of a launch whose other two blocks passed check_loose_params
static int check_loose_mag(const ginsim_mc_params* m, const ginsim_loose_mag_params* g) {
    REQUIRE(g, "loose_mag_run: NULL argument");
    REQUIRE(g->mag_every >= 0, "loose_mag_run: mag_every=%lld must be >= 0", (long long)g->mag_every);
    if (g->mag_every == 0) return GINSIM_OK;
    if (m->given_sensors) {
        REQUIRE(g->in_mag, "loose_mag_run: the magnetometer block with given_sensors needs in_mag");
    } else {
        REQUIRE(g->ref_mag, "loose_mag_run: the magnetometer block needs ref_mag");
        for (int k = 0; k < 9; ++k) REQUIRE(std::isfinite(g->mag_si[k]), "loose_mag_run: mag_si must be finite");
        for (int k = 0; k < 3; ++k)
            REQUIRE(std::isfinite(g->mag_hi[k]) && std::isfinite(g->mag_std[k]), "loose_mag_run: mag_hi / mag_std must be finite");
    }
    for (int k = 0; k < 9; ++k) REQUIRE(std::isfinite(g->cal_si[k]), "loose_mag_run: cal_si must be finite");
    for (int k = 0; k < 3; ++k) {
        REQUIRE(std::isfinite(g->mag_n[k]) && std::isfinite(g->cal_hi[k]), "loose_mag_run: mag_n / cal_hi must be finite");
        REQUIRE(std::isfinite(g->r_mag[k]) && g->r_mag[k] > 0.0, "loose_mag_run: r_mag must be positive");
    }
    REQUIRE(g->mag_n[0] != 0.0 || g->mag_n[1] != 0.0 || g->mag_n[2] != 0.0, "loose_mag_run: mag_n must not be the zero vector");
    return GINSIM_OK;
}

// the scale-factor block of a launch whose other two blocks passed check_loose_params (fp32 among what that refuses)
static int check_loose_scale(const ginsim_loose_params* p, const ginsim_loose_scale_params* q) {
    REQUIRE(q, "loose_scale_run: NULL argument");
    REQUIRE((p->aid_mask & 1) != 0, "loose_scale_run: aid_mask=%d has no bit 0: a scale-factor state without the odometer is refused", (int)p->aid_mask);
    REQUIRE(std::isfinite(q->scale0) && q->scale0 > 0.0, "loose_scale_run: scale0 must be positive");
    REQUIRE(std::isfinite(q->p0_scale) && q->p0_scale >= 0.0, "loose_scale_run: p0_scale must be finite and not negative");
    REQUIRE(std::isfinite(q->q_k) && q->q_k >= 0.0, "loose_scale_run: q_k must be finite and not negative");
    return GINSIM_OK;
}

// the standstill block of a launch whose other two blocks passed check_loose_params (fp32 among what that refuses)
static int check_loose_still(const ginsim_mc_params* m, const ginsim_loose_still_params* q) {
    REQUIRE(q, "loose_still_run: NULL argument");
    REQUIRE(q->still_mask >= 0 && q->still_mask <= 3, "loose_still_run: still_mask=%d must lie in 0 .. 3", (int)q->still_mask);
    if (q->still_mask == 0) return GINSIM_OK;
    REQUIRE(m->precision == 0, "loose_still_run: the standstill block is fp64 only");
    REQUIRE(q->still_every >= 1, "loose_still_run: still_every=%lld must be >= 1", (long long)q->still_every);
    REQUIRE((q->still_mask & 1) == 0 || (std::isfinite(q->r_zupt) && q->r_zupt > 0.0), "loose_still_run: r_zupt must be positive");
    for (int k = 0; k < 3; ++k)
        REQUIRE((q->still_mask & 2) == 0 || (std::isfinite(q->r_zaru[k]) && q->r_zaru[k] > 0.0), "loose_still_run: r_zaru must be positive");
    REQUIRE(q->still_flags, "loose_still_run: still_flags missing");
    return GINSIM_OK;
}

// The family of a launch of the filter, in one order: the combined family (two or three of the magnetometer, scale-factor and
// standstill blocks), checkpoints, magnetometer, scale-factor state, standstill, aiding, plain.  Before them all: checkpoints through
// ginsim_loose_all_cons.h, whatever blocks are left.
static hipError_t launch_loose(const LooseLaunch& L) {
    if (L.b->n_list <= 0 && !L.name) return hipSuccess;
    if (L.all_cons) return launch_loose_all_cons(L);
    if (L.all) return launch_loose_all(L);
    if (L.cons) return launch_loose_cons(L);
    if (L.mag) return launch_loose_mag(L);
    if (L.scale) return launch_loose_scale(L);
    if (L.still) return launch_loose_still(L);
    return L.b->aid_mask != 0 ? launch_loose_aided(L) : launch_loose_plain(L);
}

// What every entry point of the loose family does with its blocks: L.mc, L.b and, for the entry points of family `who`, that
// family's block (the others are NULL).  The one place that orders the checks: the base blocks, then the family's own; a
// degenerate block (cons_m == 0, mag_every == 0, still_mask == 0) is then no block.  L.name != NULL (c is not read): the kernel's name.  Otherwise
// the stamps, the visibility flags (padded to 8 bytes) and the checkpoint samples are copied next to each other into the context's
// scratch and the family is launched.
// LOOSE_ALL (ginsim_loose_all.h): any of the magnetometer, scale-factor and standstill blocks, each NULL or checked as its own family
// checks it, in that order; with two or three left after the degenerate ones the launch is the combined family's, with one or none
// the launch that block's own entry point makes.
// LOOSE_ALL_CONS (ginsim_loose_all_cons.h): LOOSE_ALL's blocks and checks, then the checkpoint block as LOOSE_CONS checks it, then
// the truth of the scale factor (L.scale_truth, a device pointer); with cons_m == 0 it is LOOSE_ALL, otherwise the launch is
// loose_all_cons_kernel whatever blocks are left.
enum LooseFamily { LOOSE_PLAIN, LOOSE_CONS, LOOSE_MAG, LOOSE_SCALE, LOOSE_STILL, LOOSE_ALL, LOOSE_ALL_CONS };

static int loose_entry(LooseFamily who, ginsim_ctx* c, LooseLaunch L) {
    int rc = check_loose_params(L.mc, L.b);
    if (rc) return rc;
    rc = who == LOOSE_CONS ? check_loose_cons(L.mc, L.b, L.cons) : who == LOOSE_MAG ? check_loose_mag(L.mc, L.mag)
       : who == LOOSE_SCALE ? check_loose_scale(L.b, L.scale) : who == LOOSE_STILL ? check_loose_still(L.mc, L.still) : GINSIM_OK;
    if (rc) return rc;
    if (who == LOOSE_ALL || who == LOOSE_ALL_CONS) {
        if (L.mag && (rc = check_loose_mag(L.mc, L.mag))) return rc;
        if (L.scale && (rc = check_loose_scale(L.b, L.scale))) return rc;
        if (L.still && (rc = check_loose_still(L.mc, L.still))) return rc;
    }
    if (who == LOOSE_ALL_CONS) {
        if ((rc = check_loose_cons(L.mc, L.b, L.cons))) return rc;
        REQUIRE(!L.scale_truth || L.scale, "loose_all_cons_run: scale_truth without a scale block");
    }
    if (L.cons && L.cons->cons_m == 0) L.cons = nullptr;
    if (L.mag && L.mag->mag_every == 0) L.mag = nullptr;
    if (L.still && L.still->still_mask == 0) L.still = nullptr;
    L.all_cons = who == LOOSE_ALL_CONS && L.cons != nullptr;
    L.all = (who == LOOSE_ALL || who == LOOSE_ALL_CONS) && (L.mag != nullptr) + (L.scale != nullptr) + (L.still != nullptr) >= 2;
    if (L.name) {
        L.name[0] = 0;
        (void)launch_loose(L);
        return GINSIM_OK;
    }
    HIP_TRY(hipSetDevice(c->device));
    const ginsim_loose_params* p = L.b;
    const size_t sb = sizeof(int64_t) * (size_t)p->m, vb = (sizeof(int32_t) * (size_t)p->m + 7) / 8 * 8;
    const size_t cb = L.cons ? sizeof(int64_t) * (size_t)L.cons->cons_m : 0;
    if (sb + cb > 0) {
        void* ws = nullptr;
        HIP_TRY(scratch(c, 3, sb + vb + cb, &ws));
        if (p->m > 0) {
            int64_t* d_stamp = reinterpret_cast<int64_t*>(ws);
            HIP_TRY(hipMemcpyAsync(d_stamp, p->gps_stamp, sb, hipMemcpyHostToDevice, c->stream));
            L.stamp = d_stamp;
            if (p->gps_visible) {
                int32_t* d_vis = reinterpret_cast<int32_t*>(reinterpret_cast<char*>(ws) + sb);
                HIP_TRY(hipMemcpyAsync(d_vis, p->gps_visible, sizeof(int32_t) * (size_t)p->m, hipMemcpyHostToDevice, c->stream));
                L.visible = d_vis;
            }
        }
        if (cb > 0) {
            int64_t* d_cons = reinterpret_cast<int64_t*>(reinterpret_cast<char*>(ws) + sb + vb);
            HIP_TRY(hipMemcpyAsync(d_cons, L.cons->cons_sample, cb, hipMemcpyHostToDevice, c->stream));
            L.samples = d_cons;
        }
    }
    L.stream = c->stream;
    HIP_TRY(launch_loose(L));
    return GINSIM_OK;
}

int ginsim_loose_kernel_name(const ginsim_mc_params* mc, const ginsim_loose_params* p, char* buf, size_t cap) {
    REQUIRE(buf && cap > 0, "loose_kernel_name: bad arguments");
    return loose_entry(LOOSE_PLAIN, nullptr, LooseLaunch{mc, p, nullptr, nullptr, nullptr, nullptr, buf, cap});
}

int ginsim_loose_run(ginsim_ctx* c, const ginsim_mc_params* mc, const ginsim_loose_params* p) {
    REQUIRE(c, "loose_run: NULL argument");
    return loose_entry(LOOSE_PLAIN, c, LooseLaunch{mc, p});
}

int ginsim_loose_cons_kernel_name(const ginsim_mc_params* mc, const ginsim_loose_params* p, const ginsim_loose_cons_params* cons,
                                  char* buf, size_t cap) {
    REQUIRE(buf && cap > 0, "loose_cons_kernel_name: bad arguments");
    return loose_entry(LOOSE_CONS, nullptr, LooseLaunch{mc, p, cons, nullptr, nullptr, nullptr, buf, cap});
}

int ginsim_loose_cons_run(ginsim_ctx* c, const ginsim_mc_params* mc, const ginsim_loose_params* p, const ginsim_loose_cons_params* cons) {
    REQUIRE(c, "loose_cons_run: NULL argument");
    return loose_entry(LOOSE_CONS, c, LooseLaunch{mc, p, cons});
}

int ginsim_loose_mag_kernel_name(const ginsim_mc_params* mc, const ginsim_loose_params* p, const ginsim_loose_mag_params* mag,
                                 char* buf, size_t cap) {
    REQUIRE(buf && cap > 0, "loose_mag_kernel_name: bad arguments");
    return loose_entry(LOOSE_MAG, nullptr, LooseLaunch{mc, p, nullptr, mag, nullptr, nullptr, buf, cap});
}

int ginsim_loose_mag_run(ginsim_ctx* c, const ginsim_mc_params* mc, const ginsim_loose_params* p, const ginsim_loose_mag_params* mag) {
    REQUIRE(c, "loose_mag_run: NULL argument");
    return loose_entry(LOOSE_MAG, c, LooseLaunch{mc, p, nullptr, mag});
}

int ginsim_loose_scale_kernel_name(const ginsim_mc_params* mc, const ginsim_loose_params* p, const ginsim_loose_scale_params* scale,
                                   char* buf, size_t cap) {
    REQUIRE(buf && cap > 0, "loose_scale_kernel_name: bad arguments");
    return loose_entry(LOOSE_SCALE, nullptr, LooseLaunch{mc, p, nullptr, nullptr, scale, nullptr, buf, cap});
}

int ginsim_loose_scale_run(ginsim_ctx* c, const ginsim_mc_params* mc, const ginsim_loose_params* p, const ginsim_loose_scale_params* scale) {
    REQUIRE(c, "loose_scale_run: NULL argument");
    return loose_entry(LOOSE_SCALE, c, LooseLaunch{mc, p, nullptr, nullptr, scale});
}

int ginsim_loose_still_kernel_name(const ginsim_mc_params* mc, const ginsim_loose_params* p, const ginsim_loose_still_params* still,
                                   char* buf, size_t cap) {
    REQUIRE(buf && cap > 0, "loose_still_kernel_name: bad arguments");
    return loose_entry(LOOSE_STILL, nullptr, LooseLaunch{mc, p, nullptr, nullptr, nullptr, still, buf, cap});
}

int ginsim_loose_still_run(ginsim_ctx* c, const ginsim_mc_params* mc, const ginsim_loose_params* p, const ginsim_loose_still_params* still) {
    REQUIRE(c, "loose_still_run: NULL argument");
    return loose_entry(LOOSE_STILL, c, LooseLaunch{mc, p, nullptr, nullptr, nullptr, still});
}

int ginsim_loose_all_kernel_name(const ginsim_mc_params* mc, const ginsim_loose_params* p, const ginsim_loose_mag_params* mag,
                                 const ginsim_loose_scale_params* scale, const ginsim_loose_still_params* still, char* buf, size_t cap) {
    REQUIRE(buf && cap > 0, "loose_all_kernel_name: bad arguments");
    return loose_entry(LOOSE_ALL, nullptr, LooseLaunch{mc, p, nullptr, mag, scale, still, buf, cap});
}

int ginsim_loose_all_run(ginsim_ctx* c, const ginsim_mc_params* mc, const ginsim_loose_params* p, const ginsim_loose_mag_params* mag,
                         const ginsim_loose_scale_params* scale, const ginsim_loose_still_params* still) {
    REQUIRE(c, "loose_all_run: NULL argument");
    return loose_entry(LOOSE_ALL, c, LooseLaunch{mc, p, nullptr, mag, scale, still});
}

int ginsim_loose_all_cons_kernel_name(const ginsim_mc_params* mc, const ginsim_loose_params* p, const ginsim_loose_mag_params* mag,
                                      const ginsim_loose_scale_params* scale, const ginsim_loose_still_params* still,
                                      const ginsim_loose_cons_params* cons, const double* scale_truth, char* buf, size_t cap) {
    REQUIRE(buf && cap > 0, "loose_all_cons_kernel_name: bad arguments");
    LooseLaunch L{mc, p, cons, mag, scale, still, buf, cap};
    L.scale_truth = scale_truth;
    return loose_entry(LOOSE_ALL_CONS, nullptr, L);
}

int ginsim_loose_all_cons_run(ginsim_ctx* c, const ginsim_mc_params* mc, const ginsim_loose_params* p, const ginsim_loose_mag_params* mag,
                              const ginsim_loose_scale_params* scale, const ginsim_loose_still_params* still,
                              const ginsim_loose_cons_params* cons, const double* scale_truth) {
    REQUIRE(c, "loose_all_cons_run: NULL argument");
    LooseLaunch L{mc, p, cons, mag, scale, still};
    L.scale_truth = scale_truth;
    return loose_entry(LOOSE_ALL_CONS, c, L);
}

int ginsim_aux_sensors(ginsim_ctx* c, const ginsim_aux_params* p) {
    REQUIRE(c && p, "aux_sensors: NULL argument");
    REQUIRE(p->runs >= 1 && p->n >= 0 && p->m >= 0, "aux_sensors: bad sizes");
    REQUIRE(!p->out_gps || p->ref_gps, "aux_sensors: ref_gps missing");
    REQUIRE(!p->out_mag || p->ref_mag, "aux_sensors: ref_mag missing");
    REQUIRE(p->n <= 0xFFFFFFFFll && p->m <= 0xFFFFFFFFll, "aux_sensors: sample index exceeds the RNG counter");
    REQUIRE((double)p->n * (double)p->runs < 5.0e11 && (double)p->m * (double)p->runs < 5.0e11, "aux_sensors: too many elements");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(launch_aux(*p, c->stream));
    return GINSIM_OK;
}

int ginsim_magcal_run(ginsim_ctx* c, const ginsim_magcal_params* p) {
    REQUIRE(c && p, "magcal_run: NULL argument");
    REQUIRE(p->runs >= 1, "magcal_run: runs=%lld must be >= 1", (long long)p->runs);
    REQUIRE(p->n >= 1 && p->n <= 0xFFFFFFFFll, "magcal_run: n must lie in 1 .. the 32-bit sample counter of the RNG");
    REQUIRE(p->runs <= (int64_t)0x7FFFFFFF * 64, "magcal_run: too many runs for one launch");
    REQUIRE(p->in_mag || p->ref_mag, "magcal_run: neither ref_mag (generated form) nor in_mag (given form)");
    REQUIRE(p->out_si && p->out_hi, "magcal_run: out_si / out_hi missing");
    for (int a = 0; a < 3; ++a) {
        const long long s0 = (long long)p->seg[2 * a], s1 = (long long)p->seg[2 * a + 1];
        REQUIRE(s0 >= 0 && s1 <= (long long)p->n, "magcal_run: range %c [%lld, %lld) is outside [0, %lld]", "xyz"[a], s0, s1, (long long)p->n);
        REQUIRE(s0 < s1, "magcal_run: range %c [%lld, %lld) is empty", "xyz"[a], s0, s1);
    }
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(launch_magcal(*p, c->stream));
    return GINSIM_OK;
}

int ginsim_end_stats(ginsim_ctx* c, const double* end_err, int64_t runs, ginsim_stats* host_out) {
    REQUIRE(c && end_err && host_out && runs >= 1, "end_stats: bad arguments");
    HIP_TRY(hipSetDevice(c->device));
    void* ws = nullptr;
    HIP_TRY(scratch(c, 0, stats_scratch_bytes(runs), &ws));
    HIP_TRY(launch_end_stats(end_err, runs, ws, c->stream));
    const char* res = reinterpret_cast<char*>(ws) + stats_scratch_bytes(runs) - sizeof(ginsim_stats);
    HIP_TRY(hipMemcpyAsync(host_out, res, sizeof(ginsim_stats), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return GINSIM_OK;
}

int ginsim_end_stats_begin(ginsim_ctx* c, const double* end_err, int64_t runs, int32_t slot) {
    REQUIRE(c && end_err && runs >= 1 && slot >= 0 && slot < 8, "end_stats_begin: bad arguments");
    REQUIRE(!c->stat_pending[slot], "end_stats_begin: slot %d is still pending (call ginsim_end_stats_finish first)", slot);
    HIP_TRY(hipSetDevice(c->device));
    if (!c->stat_slots) HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&c->stat_slots), 8 * sizeof(ginsim_stats), hipHostMallocDefault));
    if (!c->stat_ev[slot]) HIP_TRY(hipEventCreateWithFlags(&c->stat_ev[slot], hipEventDisableTiming));
    void* ws = nullptr;
    HIP_TRY(scratch(c, 0, stats_scratch_bytes(runs), &ws));
    HIP_TRY(launch_end_stats(end_err, runs, ws, c->stream));
    const char* res = reinterpret_cast<char*>(ws) + stats_scratch_bytes(runs) - sizeof(ginsim_stats);
    HIP_TRY(hipMemcpyAsync(&c->stat_slots[slot], res, sizeof(ginsim_stats), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipEventRecord(c->stat_ev[slot], c->stream));
    c->stat_pending[slot] = true;
    return GINSIM_OK;
}

int ginsim_end_stats_finish(ginsim_ctx* c, int32_t slot, ginsim_stats* host_out) {
    REQUIRE(c && host_out && slot >= 0 && slot < 8, "end_stats_finish: bad arguments");
    REQUIRE(c->stat_pending[slot], "end_stats_finish: nothing was begun in slot %d", slot);
    HIP_TRY(hipEventSynchronize(c->stat_ev[slot]));
    *host_out = c->stat_slots[slot];
    c->stat_pending[slot] = false;
    return GINSIM_OK;
}

// ---- multi-GPU exchange behind the ABI (RCCL on the context's stream; csrc/comm.cpp)
int ginsim_comm_unique_id(unsigned char* id) {
    REQUIRE(id, "comm_unique_id: NULL output");
    const char* err = comm_unique_id(id);
    if (err) { set_error("comm_unique_id: %s", err); return GINSIM_ERR_HIP; }
    return GINSIM_OK;
}

int ginsim_comm_init(ginsim_ctx* c, int32_t nranks, int32_t rank, const unsigned char* id) {
    REQUIRE(c && id && nranks >= 1 && rank >= 0 && rank < nranks, "comm_init: bad arguments");
    REQUIRE(!c->comm, "comm_init: this context already has a communicator");
    HIP_TRY(hipSetDevice(c->device));
    // the buffers first: a failure here must not leave a communicator behind (the other ranks would already be inside the
    // collective ncclCommInitRank, and a retry on this context would be refused)
    const size_t bytes = sizeof(ginsim_stats) * 8 * (size_t)nranks;
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&c->comm_recv), bytes);
    if (e == hipSuccess) e = hipHostMalloc(reinterpret_cast<void**>(&c->comm_host), bytes, hipHostMallocDefault);
    const char* err = e == hipSuccess ? comm_create(nranks, rank, id, &c->comm) : nullptr;
    if (e != hipSuccess || err) {
        if (c->comm_recv) { (void)hipFree(c->comm_recv); c->comm_recv = nullptr; }
        if (c->comm_host) { (void)hipHostFree(c->comm_host); c->comm_host = nullptr; }
        c->comm = nullptr;
        if (err) set_error("comm_init: %s", err);
        else set_error("comm_init: %s", hipGetErrorString(e));
        return GINSIM_ERR_HIP;
    }
    return GINSIM_OK;
}

int ginsim_comm_probe(void) {
    const char* err = comm_probe();
    if (err) { set_error("comm_probe: %s", err); return GINSIM_ERR_HIP; }
    return GINSIM_OK;
}

// where the FIRST workgroup of a launch on this context's stream lands: the accelerator complex die (XCD) of an MI300 / MI355X
__global__ void first_xcc_kernel(uint32_t* out) {
    if (threadIdx.x == 0) out[0] = __builtin_amdgcn_s_getreg((31 << 11) | 20) & 0xf;      // HW_REG_XCC_ID, bits 3:0
}

int ginsim_stream_first_xcc(ginsim_ctx* c, int32_t* xcc) {
    REQUIRE(c && xcc, "stream_first_xcc: NULL argument");
    HIP_TRY(hipSetDevice(c->device));
    void* ws = nullptr;
    HIP_TRY(scratch(c, 2, 64, &ws));
    hipLaunchKernelGGL(first_xcc_kernel, dim3(1), dim3(64), 0, c->stream, reinterpret_cast<uint32_t*>(ws));
    HIP_TRY(hipGetLastError());
    uint32_t v = 0;
    HIP_TRY(hipMemcpyAsync(&v, ws, sizeof v, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    *xcc = (int32_t)v;
    return GINSIM_OK;
}

int ginsim_vib_psd_series(ginsim_ctx* c, const double* amp, int64_t period, int64_t runs, uint64_t run_offset, uint64_t seed,
                          int32_t sensor, int32_t halve_per_run, double* out) {
    REQUIRE(c && amp && out, "vib_psd_series: NULL argument");
    REQUIRE(period >= 2 && period <= 16384 && period % 2 == 0, "vib_psd_series: period %lld must be even, 2 .. 16384 (time_series_from_psd.py:36-43)",
            (long long)period);
    REQUIRE(runs >= 1 && runs <= (int64_t)0x7FFFFFFF * 64, "vib_psd_series: runs=%lld out of range", (long long)runs);
    REQUIRE(sensor == 0 || sensor == 1, "vib_psd_series: sensor must be 0 (accelerometer) or 1 (gyroscope)");
    REQUIRE(halve_per_run == 0 || halve_per_run == 1, "vib_psd_series: halve_per_run must be 0 or 1");
    for (int64_t k = 0; k < 3 * (period / 2 + 1); ++k)
        REQUIRE(std::isfinite(amp[k]) && amp[k] >= 0.0, "vib_psd_series: amplitude %lld is negative or not finite", (long long)k);
    HIP_TRY(hipSetDevice(c->device));
    void* ws = nullptr;
    HIP_TRY(scratch(c, 3, vib_psd_scratch_bytes(period, runs), &ws));
    return launch_vib_psd(c->device, c->stream, amp, period, runs, run_offset, seed, sensor, halve_per_run, ws, out);
}

int ginsim_comm_query(ginsim_ctx* c, int32_t* nranks, int32_t* rank, int32_t* device) {
    REQUIRE(c && nranks && rank && device, "comm_query: bad arguments");
    REQUIRE(c->comm, "comm_query: no communicator (ginsim_comm_init)");
    int n = -1, r = -1, d = -1;
    const char* err = comm_query(c->comm, &n, &r, &d);
    if (err) { set_error("comm_query: %s", err); return GINSIM_ERR_HIP; }
    *nranks = n; *rank = r; *device = d;
    return GINSIM_OK;
}

int ginsim_comm_destroy(ginsim_ctx* c) {
    REQUIRE(c, "comm_destroy: NULL context");
    if (!c->comm) return GINSIM_OK;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    comm_destroy(c->comm);
    c->comm = nullptr;
    if (c->comm_recv) { (void)hipFree(c->comm_recv); c->comm_recv = nullptr; }
    if (c->comm_host) { (void)hipHostFree(c->comm_host); c->comm_host = nullptr; }
    for (bool& p : c->comm_pending) p = false;
    return GINSIM_OK;
}

int ginsim_end_stats_all_begin(ginsim_ctx* c, const double* end_err, int64_t runs, int32_t slot) {
    REQUIRE(c && runs >= 0 && (runs == 0 || end_err) && slot >= 0 && slot < 8, "end_stats_all_begin: bad arguments");
    REQUIRE(c->comm && c->comm_recv && c->comm_host, "end_stats_all_begin: no communicator (ginsim_comm_init)");
    REQUIRE(!c->comm_pending[slot], "end_stats_all_begin: slot %d is still pending (call ginsim_end_stats_all_finish first)", slot);
    HIP_TRY(hipSetDevice(c->device));
    if (!c->comm_ev[slot]) HIP_TRY(hipEventCreateWithFlags(&c->comm_ev[slot], hipEventDisableTiming));
    const int nranks = comm_nranks(c->comm);
    void* ws = nullptr;
    const size_t wb = stats_scratch_bytes(runs > 0 ? runs : 1);
    HIP_TRY(scratch(c, 0, wb, &ws));
    double* rec = reinterpret_cast<double*>(reinterpret_cast<char*>(ws) + wb - sizeof(ginsim_stats));
    if (runs > 0) HIP_TRY(launch_end_stats(end_err, runs, ws, c->stream));
    else HIP_TRY(hipMemsetAsync(rec, 0, sizeof(ginsim_stats), c->stream));      // a rank without runs: the empty record
    double* recv = c->comm_recv + (size_t)slot * nranks * (sizeof(ginsim_stats) / sizeof(double));
    const char* err = comm_allgather_f64(c->comm, rec, recv, sizeof(ginsim_stats) / sizeof(double), c->stream);
    if (err) { set_error("end_stats_all_begin: %s", err); return GINSIM_ERR_HIP; }
    HIP_TRY(hipMemcpyAsync(c->comm_host + (size_t)slot * nranks, recv, sizeof(ginsim_stats) * nranks, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipEventRecord(c->comm_ev[slot], c->stream));
    c->comm_pending[slot] = true;
    return GINSIM_OK;
}

int ginsim_end_stats_all_finish(ginsim_ctx* c, int32_t slot, ginsim_stats* merged) {
    REQUIRE(c && merged && slot >= 0 && slot < 8, "end_stats_all_finish: bad arguments");
    REQUIRE(c->comm && c->comm_pending[slot], "end_stats_all_finish: nothing was begun in slot %d", slot);
    HIP_TRY(hipEventSynchronize(c->comm_ev[slot]));
    c->comm_pending[slot] = false;
    const int nranks = comm_nranks(c->comm);
    std::vector<ginsim_stats> parts;
    for (int r = 0; r < nranks; ++r) {
        const ginsim_stats& p = c->comm_host[(size_t)slot * nranks + r];
        if (p.count > 0) parts.push_back(p);
    }
    memset(merged, 0, sizeof(*merged));
    if (!parts.empty()) stats_merge_host(parts.data(), (int)parts.size(), merged);     // fixed order: rank 0 .. nranks-1
    return GINSIM_OK;
}

// The per-run statistics of kept trajectories (stats.hip's process kernel) in the context's scratch.  proc_out: the records of the
// samples >= first_sample, [runs][3][9], to the host.  end_out (proc_out NULL): a one-sample window at n - 1, whose "mean" plane
// [9][runs] IS the end-point error, reduced by ginsim_end_stats.
static int traj_stats_run(ginsim_ctx* c, const TrajView& v, int64_t first_sample, int32_t pos_ned, double* proc_out, ginsim_stats* end_out) {
    HIP_TRY(hipSetDevice(c->device));
    void* ws = nullptr;
    const size_t bytes = sizeof(double) * 27 * (size_t)v.runs;
    HIP_TRY(scratch(c, 2, bytes, &ws));
    double* rec = reinterpret_cast<double*>(ws);
    HIP_TRY(launch_process_stats(v, proc_out ? first_sample : v.n - 1, pos_ned, proc_out ? 1 : 0, rec, c->stream));
    if (!proc_out) return ginsim_end_stats(c, rec + (size_t)9 * v.runs, v.runs, end_out);
    HIP_TRY(hipMemcpyAsync(proc_out, ws, bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return GINSIM_OK;
}

int ginsim_process_stats(ginsim_ctx* c, const double* traj, const double* ref, int64_t n, int64_t runs, int64_t first_sample,
                         int32_t pos_ned, double* host_out) {
    REQUIRE(c && traj && ref && host_out, "process_stats: NULL argument");
    REQUIRE(n >= 1 && runs >= 1 && first_sample >= 0 && first_sample < n, "process_stats: bad sizes");
    return traj_stats_run(c, TrajView{traj, 0, ref, n, runs, nullptr, 0, {nullptr, 0, 0}}, first_sample, pos_ned, host_out, nullptr);
}

int ginsim_end_stats_from_traj(ginsim_ctx* c, const double* traj, const double* ref, int64_t n, int64_t runs, int32_t pos_ned,
                               ginsim_stats* host_out) {
    REQUIRE(c && traj && ref && host_out && n >= 1 && runs >= 1, "end_stats_from_traj: bad arguments");
    return traj_stats_run(c, TrajView{traj, 0, ref, n, runs, nullptr, 0, {nullptr, 0, 0}}, 0, pos_ned, nullptr, host_out);
}

int ginsim_process_stats_f32(ginsim_ctx* c, const float* traj, const double* ref, int64_t n, int64_t runs, int64_t first_sample,
                             int32_t pos_ned, const double* origin, int32_t n_ini, uint64_t ini_first, double* host_out) {
    REQUIRE(c && traj && ref && origin && host_out, "process_stats_f32: NULL argument");
    REQUIRE(n >= 1 && runs >= 1 && first_sample >= 0 && first_sample < n && n_ini >= 1, "process_stats_f32: bad sizes");
    return traj_stats_run(c, TrajView{traj, 1, ref, n, runs, nullptr, 0, {origin, n_ini, ini_first}}, first_sample, pos_ned, host_out, nullptr);
}

int ginsim_end_stats_from_traj_f32(ginsim_ctx* c, const float* traj, const double* ref, int64_t n, int64_t runs, int32_t pos_ned,
                                   const double* origin, int32_t n_ini, uint64_t ini_first, ginsim_stats* host_out) {
    REQUIRE(c && traj && ref && origin && host_out && n >= 1 && runs >= 1 && n_ini >= 1, "end_stats_from_traj_f32: bad arguments");
    return traj_stats_run(c, TrajView{traj, 1, ref, n, runs, nullptr, 0, {origin, n_ini, ini_first}}, 0, pos_ned, nullptr, host_out);
}

// ---- across-run statistics of kept trajectories at requested samples: error-growth curves (csrc/error_curve.hip), quantile keys
// (csrc/error_quantile.hip) and error covariance (csrc/error_cov.hip).  The entry points describe their input as a TrajView whose
// samples are still on the HOST; the checks below and traj_run (above) are the one path of the three families.
static int check_curve_args(const char* who, const void* c, const TrajView& v, const void* host_out) {
    const int64_t n = v.n, m = v.m;
    REQUIRE(c && v.traj && v.ref && host_out, "%s: NULL argument", who);
    REQUIRE(n >= 1 && v.runs >= 1, "%s: n=%lld runs=%lld must be >= 1", who, (long long)n, (long long)v.runs);
    REQUIRE(m >= 1, "%s: m=%lld samples (at least one is needed)", who, (long long)m);
    REQUIRE(v.samples || m == n, "%s: samples == NULL means every sample, so m must be n (m=%lld, n=%lld)", who, (long long)m, (long long)n);
    REQUIRE(m <= 0x7FFFFFFFll, "%s: too many samples for one call", who);
    if (v.samples)
        for (int64_t i = 0; i < m; ++i)
            REQUIRE(v.samples[i] >= 0 && v.samples[i] < n, "%s: sample %lld (entry %lld) is outside [0, %lld)", who, (long long)v.samples[i],
                    (long long)i, (long long)n);
    return GINSIM_OK;
}

static int check_which(const char* who, int32_t which) {
    REQUIRE(which == 0 || which == 1, "%s: which=%d is neither 0 (position) nor 1 (velocity)", who, (int)which);
    return GINSIM_OK;
}

static int check_origin(const char* who, const TrajView& v) {
    REQUIRE(!v.f32 || (v.org.table && v.org.n_ini >= 1), "%s: the origin table of the displacement series is missing", who);
    return GINSIM_OK;
}

static int curve_entry(const char* who, ginsim_ctx* c, const TrajView& v, int32_t pos_ned, double* host_out) {
    int rc = check_curve_args(who, c, v, host_out);
    if (!rc) rc = check_origin(who, v);
    if (rc) return rc;
    return traj_run(c, v, error_curve_scratch_bytes(v), host_out, sizeof(double) * 36 * (size_t)v.m,
                    [&](const TrajView& d, void* ws) { return launch_error_curve(d, pos_ned, ws, c->stream); });
}

int ginsim_error_curve(ginsim_ctx* c, const double* traj, const double* ref, int64_t n, int64_t runs, const int64_t* samples, int64_t m,
                       int32_t pos_ned, double* host_out) {
    return curve_entry("error_curve", c, TrajView{traj, 0, ref, n, runs, samples, m, {nullptr, 0, 0}}, pos_ned, host_out);
}

int ginsim_error_curve_f32(ginsim_ctx* c, const float* traj, const double* ref, int64_t n, int64_t runs, const int64_t* samples,
                           int64_t m, int32_t pos_ned, const double* origin, int32_t n_ini, uint64_t ini_first, double* host_out) {
    return curve_entry("error_curve_f32", c, TrajView{traj, 1, ref, n, runs, samples, m, {origin, n_ini, ini_first}}, pos_ned, host_out);
}

int ginsim_curve_merge(const double* parts, int32_t nparts, int64_t m, double* out) {
    REQUIRE(parts && out && nparts >= 1 && m >= 1, "curve_merge: bad arguments");
    curve_merge_host(parts, nparts, m, out);
    return GINSIM_OK;
}

// the keys of every (sample, run) go to the caller's device rows: no records in the scratch, nothing to copy back
static int keys_entry(const char* who, ginsim_ctx* c, const TrajView& v, int32_t which, int32_t pos_ned, double* keys, int64_t row_stride,
                      int64_t col0) {
    int rc = check_curve_args(who, c, v, keys);
    if (!rc) rc = check_which(who, which);
    if (rc) return rc;
    REQUIRE(col0 >= 0, "%s: col0=%lld is negative", who, (long long)col0);
    REQUIRE(row_stride >= col0 + v.runs, "%s: row_stride=%lld is shorter than col0 + runs = %lld + %lld", who, (long long)row_stride,
            (long long)col0, (long long)v.runs);
    rc = check_origin(who, v);
    if (rc) return rc;
    return traj_run(c, v, 0, nullptr, 0, [&](const TrajView& d, void*) {
        return launch_radial_keys(d, which, pos_ned, keys, row_stride, col0, c->stream);
    });
}

int ginsim_radial_keys(ginsim_ctx* c, const double* traj, const double* ref, int64_t n, int64_t runs, const int64_t* samples, int64_t m,
                       int32_t which, int32_t pos_ned, double* keys, int64_t row_stride, int64_t col0) {
    return keys_entry("radial_keys", c, TrajView{traj, 0, ref, n, runs, samples, m, {nullptr, 0, 0}}, which, pos_ned, keys, row_stride, col0);
}

int ginsim_radial_keys_f32(ginsim_ctx* c, const float* traj, const double* ref, int64_t n, int64_t runs, const int64_t* samples,
                           int64_t m, int32_t which, int32_t pos_ned, const double* origin, int32_t n_ini, uint64_t ini_first,
                           double* keys, int64_t row_stride, int64_t col0) {
    return keys_entry("radial_keys_f32", c, TrajView{traj, 1, ref, n, runs, samples, m, {origin, n_ini, ini_first}}, which, pos_ned, keys,
                      row_stride, col0);
}

// the order statistics of key rows (csrc/error_quantile.hip, the select)
int ginsim_quantile_rows(ginsim_ctx* c, const double* keys, int64_t rows, int64_t len, int64_t row_stride, const double* probs,
                         int32_t q, double* host_out, double* host_count) {
    REQUIRE(c && keys && probs && host_out && host_count, "quantile_rows: NULL argument");
    REQUIRE(rows >= 1 && len >= 1, "quantile_rows: rows=%lld len=%lld must be >= 1", (long long)rows, (long long)len);
    REQUIRE(rows <= 0x7FFFFFFFll && len <= 0x7FFFFFFFll, "quantile_rows: too many rows or keys for one call");
    REQUIRE(row_stride >= len, "quantile_rows: row_stride=%lld is shorter than len=%lld", (long long)row_stride, (long long)len);
    REQUIRE(q >= 1 && q <= GINSIM_QUANTILE_MAX_PROBS, "quantile_rows: q=%d probabilities (1..%d at once)", (int)q,
            GINSIM_QUANTILE_MAX_PROBS);
    for (int i = 0; i < q; ++i)
        REQUIRE(std::isfinite(probs[i]) && probs[i] > 0.0 && probs[i] <= 1.0, "quantile_rows: probability %g (entry %d) is not in (0, 1]",
                probs[i], i);
    HIP_TRY(hipSetDevice(c->device));
    // scratch: [q probabilities][rows x q results][rows counts]
    const size_t res = sizeof(double) * (size_t)rows * ((size_t)q + 1);
    void* ws = nullptr;
    HIP_TRY(scratch(c, 2, sizeof(double) * (size_t)q + res, &ws));
    double* d_probs = reinterpret_cast<double*>(ws);
    double* d_out = d_probs + q;
    double* d_count = d_out + (size_t)rows * q;
    HIP_TRY(hipMemcpyAsync(d_probs, probs, sizeof(double) * (size_t)q, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(launch_quantile_rows(keys, rows, len, row_stride, d_probs, q, d_out, d_count, c->stream));
    HIP_TRY(hipMemcpyAsync(host_out, d_out, sizeof(double) * (size_t)rows * q, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(host_count, d_count, sizeof(double) * (size_t)rows, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return GINSIM_OK;
}

static int cov_entry(const char* who, ginsim_ctx* c, const TrajView& v, int32_t which, int32_t pos_ned, double* host_out) {
    int rc = check_curve_args(who, c, v, host_out);
    if (!rc) rc = check_which(who, which);
    if (!rc) rc = check_origin(who, v);
    if (rc) return rc;
    return traj_run(c, v, error_cov_scratch_bytes(v), host_out, sizeof(double) * GINSIM_COV_RECORD * (size_t)v.m,
                    [&](const TrajView& d, void* ws) { return launch_error_cov(d, which, pos_ned, ws, c->stream); });
}

int ginsim_error_cov(ginsim_ctx* c, const double* traj, const double* ref, int64_t n, int64_t runs, const int64_t* samples, int64_t m,
                     int32_t which, int32_t pos_ned, double* host_out) {
    return cov_entry("error_cov", c, TrajView{traj, 0, ref, n, runs, samples, m, {nullptr, 0, 0}}, which, pos_ned, host_out);
}

int ginsim_error_cov_f32(ginsim_ctx* c, const float* traj, const double* ref, int64_t n, int64_t runs, const int64_t* samples,
                         int64_t m, int32_t which, int32_t pos_ned, const double* origin, int32_t n_ini, uint64_t ini_first,
                         double* host_out) {
    return cov_entry("error_cov_f32", c, TrajView{traj, 1, ref, n, runs, samples, m, {origin, n_ini, ini_first}}, which, pos_ned, host_out);
}

int ginsim_cov_merge(const double* parts, int32_t nparts, int64_t m, double* out) {
    REQUIRE(parts && out, "cov_merge: NULL argument");
    REQUIRE(nparts >= 1 && m >= 1, "cov_merge: nparts=%d m=%lld must be >= 1", (int)nparts, (long long)m);
    cov_merge_host(parts, nparts, m, out);
    return GINSIM_OK;
}

int ginsim_stats_merge(const ginsim_stats* parts, int32_t nparts, ginsim_stats* out) {
    REQUIRE(parts && out && nparts >= 1, "stats_merge: bad arguments");
    stats_merge_host(parts, nparts, out);
    return GINSIM_OK;
}

int ginsim_gather_runs(ginsim_ctx* c, const double* series, int32_t ncomp, int64_t n, int64_t runs,
                       const int64_t* run_ids, int32_t nsel, double* host_out) {
    return gather_run("gather_runs", c, series, ncomp, n, runs, run_ids, nsel, host_out, [&](const int64_t* ids, double* out) {
        return launch_gather_runs(series, ncomp, n, runs, ids, nsel, out, c->stream);
    });
}

int ginsim_gather_series(ginsim_ctx* c, const double* series, int32_t ncomp, int64_t n, int64_t runs, const int64_t* run_ids,
                         int32_t nsel, double* host_out) {
    return gather_run("gather_series", c, series, ncomp, n, runs, run_ids, nsel, host_out, [&](const int64_t* ids, double* out) {
        return launch_gather_series(series, ncomp, n, ids, nsel, out, c->stream);
    });
}

int ginsim_gather_runs_f32(ginsim_ctx* c, const float* series, int32_t ncomp, int64_t n, int64_t runs,
                           const int64_t* run_ids, int32_t nsel, double* host_out) {
    return gather_run("gather_runs_f32", c, series, ncomp, n, runs, run_ids, nsel, host_out, [&](const int64_t* ids, double* out) {
        return launch_gather_runs_f32(series, ncomp, n, runs, ids, nsel, out, c->stream);
    });
}

int ginsim_free_integration(ginsim_ctx* c, int32_t algo, int32_t ref_frame, double fs, int32_t earth_rot,
                            const double* gyro, const double* accel, const double* odo, int64_t R, int64_t n,
                            const double* ini, int32_t n_ini, int32_t ini_has_g, uint64_t ini_first, double* att,
                            double* pos, double* vel) {
    REQUIRE(c && gyro && ini && att && pos && vel, "free_integration: NULL argument");
    REQUIRE(algo == GINSIM_ALGO_FREE || algo == GINSIM_ALGO_ODO, "free_integration: algo must be one GINSIM_ALGO_* bit");
    REQUIRE(algo != GINSIM_ALGO_FREE || accel, "free_integration: accel missing");
    REQUIRE(algo != GINSIM_ALGO_ODO || odo, "free_integration: odo missing");
    REQUIRE(R >= 1 && n >= 1 && n_ini >= 1, "free_integration: bad sizes");
    HIP_TRY(hipSetDevice(c->device));
    const size_t plane = (size_t)R * n;
    DevBuf d_aos, d_gyro, d_accel, d_odo, d_ini, d_traj;
    HIP_TRY(d_aos.alloc(sizeof(double) * plane * 3));
    HIP_TRY(d_gyro.alloc(sizeof(double) * plane * 3));
    HIP_TRY(d_accel.alloc(sizeof(double) * plane * 3));
    HIP_TRY(d_odo.alloc(sizeof(double) * plane));
    HIP_TRY(d_ini.alloc(sizeof(double) * 10 * n_ini));
    HIP_TRY(d_traj.alloc(sizeof(double) * plane * 9));
    HIP_TRY(hipMemcpyAsync(d_ini.p, ini, sizeof(double) * 10 * n_ini, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(d_aos.p, gyro, sizeof(double) * plane * 3, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(launch_aos_to_soa(d_aos.as<double>(), d_gyro.as<double>(), R, n, 3, c->stream));
    if (algo == GINSIM_ALGO_FREE) {
        HIP_TRY(hipMemcpyAsync(d_aos.p, accel, sizeof(double) * plane * 3, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(launch_aos_to_soa(d_aos.as<double>(), d_accel.as<double>(), R, n, 3, c->stream));
    } else {
        HIP_TRY(hipMemcpyAsync(d_aos.p, odo, sizeof(double) * plane, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(launch_aos_to_soa(d_aos.as<double>(), d_odo.as<double>(), R, n, 1, c->stream));
    }
    ginsim_mc_params p;
    memset(&p, 0, sizeof(p));
    p.n = n; p.runs = R; p.fs = fs; p.ref_frame = ref_frame; p.algo_mask = algo; p.earth_rot = earth_rot;
    p.n_ini = n_ini; p.ini_first = ini_first; p.ini_has_g = ini_has_g; p.given_sensors = 1;
    p.ini = d_ini.as<double>();
    p.in_gyro = d_gyro.as<double>(); p.in_accel = d_accel.as<double>(); p.in_odo = d_odo.as<double>();
    p.out_traj[algo == GINSIM_ALGO_FREE ? 0 : 1] = d_traj.as<double>();
    const int rc = ginsim_mc_run(c, &p);
    if (rc) return rc;
    // [9][n][R] -> three host arrays [R][n][3]
    std::vector<int64_t> all(R);
    for (int64_t i = 0; i < R; ++i) all[i] = i;
    DevBuf d_ids, d_out;
    HIP_TRY(d_ids.alloc(sizeof(int64_t) * R));
    HIP_TRY(d_out.alloc(sizeof(double) * plane * 3));
    HIP_TRY(hipMemcpyAsync(d_ids.p, all.data(), sizeof(int64_t) * R, hipMemcpyHostToDevice, c->stream));
    double* host[3] = {att, pos, vel};
    for (int k = 0; k < 3; ++k) {
        HIP_TRY(launch_gather_runs(d_traj.as<double>() + (size_t)3 * k * plane, 3, n, R, d_ids.as<int64_t>(), (int)R,
                                   d_out.as<double>(), c->stream));
        HIP_TRY(hipMemcpyAsync(host[k], d_out.p, sizeof(double) * plane * 3, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    return GINSIM_OK;
}

int ginsim_allan_plan(const double* x, int64_t n, int32_t nseries, int64_t series_stride, double fs, int32_t* ntau, int32_t* nlevels,
                      ginsim_allan_level* levels, int32_t cap) {
    REQUIRE(ntau && nlevels && (levels || cap == 0) && cap >= 0, "allan_plan: bad arguments");
    AllanPlan P;
    const int rc = allan_plan(x, n, nseries, series_stride, fs, P);
    if (rc) return rc;
    *ntau = (int32_t)P.mult.size();
    *nlevels = P.levels;
    if (P.levels > cap) { set_error("allan_plan: %d levels but capacity %d", P.levels, cap); return GINSIM_ERR_RANGE; }
    for (int k = 0; k < P.levels; ++k) {
        levels[k].n_in = P.lvs[k].n_in;
        levels[k].in_stride = P.lvs[k].in_stride;
        levels[k].mode = P.mode[k];
        levels[k].chunks_per_block = P.chunks_per_block[k];
        levels[k].nparts = P.nparts[k];
        levels[k].reserved = 0;
    }
    return GINSIM_OK;
}

int ginsim_allan(ginsim_ctx* c, const double* x, int64_t n, int32_t nseries, int64_t series_stride, double fs, double* tau,
                 double* avar, int32_t* ntau, int32_t cap) {
    REQUIRE(c && x && tau && avar && ntau, "allan: NULL argument");
    *ntau = 0;
    AllanPlan P;
    const int rc = allan_plan(x, n, nseries, series_stride, fs, P);
    if (rc) return rc;
    const std::vector<int64_t>& mult = P.mult;
    const int nt = (int)mult.size();
    if (nt == 0) return GINSIM_OK;
    // the three chunked kernels put the series on the grid's y dimension; the finishing launch has them on x
    if (!P.steps.empty() && nseries > c->max_grid_y) {
        set_error("allan: %d series on the grid's y dimension but the device takes %d: split the batch into calls of at most %d series",
                  (int)nseries, c->max_grid_y, c->max_grid_y);
        return GINSIM_ERR_RANGE;
    }
    if (nt > cap) { set_error("allan: %d averaging factors but capacity %d", nt, cap); return GINSIM_ERR_RANGE; }
    HIP_TRY(hipSetDevice(c->device));
    const double ts = 1.0 / fs;
    const int levels = P.levels;
    const int64_t n1 = n / 10;
    const std::vector<AllanLevel>& lvs = P.lvs;
    const AllanFold& fold = P.fold;
    const int64_t records = P.records;
    const std::vector<AllanStep>& steps = P.steps;
    struct Region { void* p; double* d() const { return reinterpret_cast<double*>(p); } } ping, pong, partial;
    const size_t b_ping = sizeof(double) * (size_t)nseries * (n1 + 1), b_pong = sizeof(double) * (size_t)nseries * (n1 / 10 + 1);
    const size_t b_part = sizeof(double) * 9 * (size_t)(records + 1), b_sums = 0;
    void* region = nullptr;
    HIP_TRY(scratch(c, 1, b_ping + b_pong + b_part + b_sums + 1024, &region));
    ping.p = region;
    pong.p = reinterpret_cast<char*>(region) + ((b_ping + 255) & ~(size_t)255);
    partial.p = reinterpret_cast<char*>(pong.p) + ((b_pong + 255) & ~(size_t)255);
    const double* in = x;
    int flip = 0;
    for (const AllanStep& st : steps) {
        // level k+1 (<= n/10 entries per series) goes to ping, k+2 to pong, ...
        const int k = st.k;
        if (st.mode == 2) {             // level k+1 -> ping (its last workgroup per series only), level k+2 -> pong
            HIP_TRY(launch_allan_fused(in, ping.d(), pong.d(), partial.d() + 9 * fold.offset[k], partial.d() + 9 * fold.offset[k + 1],
                                       lvs[k], lvs[k + 1], nseries, c->stream));
            in = pong.d();
            flip = 2;
            continue;
        }
        double* out = (flip++ % 2 == 0) ? ping.d() : pong.d();
        if (st.mode == 1)
            HIP_TRY(launch_allan_pair(in, out, partial.d() + 9 * fold.offset[k], lvs[k], nseries, c->stream));
        else
            HIP_TRY(launch_allan_level(in, out, partial.d() + 9 * fold.offset[k], lvs[k], nseries, c->stream));
        in = out;
    }
    AllanTail t;
    t.first = fold.nlevels;
    t.nlevels = levels - fold.nlevels;
    t.in_stride = t.nlevels > 0 ? lvs[t.first].in_stride : 0;
    t.nseries = nseries;
    for (int l = 0; l < t.nlevels; ++l) {
        t.n_in[l] = lvs[t.first + l].n_in;
        for (int j = 0; j < 9; ++j) t.nb[l][j] = lvs[t.first + l].nb[j];
    }
    // the sums go straight into pinned host memory (83 KB for 192 series x 6 levels): no copy, one synchronisation
    const size_t nsums = (size_t)9 * nseries * levels;
    if (c->allan_host_doubles < nsums) {
        if (c->allan_host) { HIP_TRY(hipStreamSynchronize(c->stream)); HIP_TRY(hipHostFree(c->allan_host)); c->allan_host = nullptr; c->allan_host_doubles = 0; }
        HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&c->allan_host), sizeof(double) * (nsums + nsums / 4 + 64), hipHostMallocDefault));
        c->allan_host_doubles = nsums + nsums / 4 + 64;
    }
    HIP_TRY(launch_allan_finish(in, partial.d(), c->allan_host, t, fold, nseries, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    const double* h = c->allan_host;
    for (int i = 0; i < nt; ++i) {
        const int64_t m = mult[i];
        int k = 0;
        int64_t p = 1;
        while (m / p >= 10) { p *= 10; ++k; }
        const int j = (int)(m / p);
        const int64_t nb = n / m;
        tau[i] = (double)m * ts;
        for (int s = 0; s < nseries; ++s) {
            const double sum = h[((size_t)k * nseries + s) * 9 + (j - 1)];
            avar[(size_t)s * cap + i] = 0.5 / (double)(nb - 1) * sum / ((double)m * (double)m);
        }
    }
    *ntau = nt;
    return GINSIM_OK;
}

// ---- overlapping Allan variance (include/ginsim_oallan.h, csrc/oallan.hip)
int ginsim_oallan_plan(const double* x, int64_t n, int32_t nseries, int64_t series_stride, double fs, int32_t* ntau,
                       ginsim_oallan_factor* f, int32_t cap, ginsim_oallan_geometry* g) {
    (void)x;
    REQUIRE(ntau && g && (f || cap == 0) && cap >= 0, "oallan_plan: bad arguments");
    OallanPlan P;
    const int rc = oallan_plan(n, nseries, series_stride, fs, P);
    if (rc) return rc;
    const int nt = P.F.count;
    *ntau = nt;
    g->tile_payload = oallan_tile_payload();
    g->tile_halo = oallan_tile_halo();
    g->scratch_bytes = (int64_t)(P.b_records + P.b_theta + P.b_sums);
    g->tile_factors = P.tile;
    g->stream_factors = nt - P.tile;
    if (nt > cap) { set_error("oallan_plan: %d averaging factors but capacity %d", nt, cap); return GINSIM_ERR_RANGE; }
    for (int i = 0; i < nt; ++i) {
        f[i].m = P.F.m[i];
        f[i].terms = n - 2 * (int64_t)P.F.m[i] + 1;
        f[i].form = i < P.tile ? 0 : 1;
        f[i].nparts = P.F.nparts[i];
    }
    return GINSIM_OK;
}

int ginsim_oallan(ginsim_ctx* c, const double* x, int64_t n, int32_t nseries, int64_t series_stride, double fs, double* tau,
                  double* oavar, int32_t* ntau, int32_t cap) {
    REQUIRE(c && x && tau && oavar && ntau, "oallan: NULL argument");
    *ntau = 0;
    OallanPlan P;
    const int rc = oallan_plan(n, nseries, series_stride, fs, P);
    if (rc) return rc;
    const OallanFactors& F = P.F;
    const int nt = F.count;
    if (nt == 0) return GINSIM_OK;
    // the tile, chunk-sum, apply and stream launches have the series on the grid's y dimension (the scan of the chunk sums and
    // the finishing launch on x)
    if (nseries > c->max_grid_y) {
        set_error("oallan: %d series on the grid's y dimension but the device takes %d: split the batch into calls of at most %d series",
                  (int)nseries, c->max_grid_y, c->max_grid_y);
        return GINSIM_ERR_RANGE;
    }
    if (nt > cap) { set_error("oallan: %d averaging factors but capacity %d", nt, cap); return GINSIM_ERR_RANGE; }
    HIP_TRY(hipSetDevice(c->device));
    void* region = nullptr;
    HIP_TRY(scratch(c, 1, P.b_records + P.b_theta + P.b_sums, &region));
    double* records = reinterpret_cast<double*>(region);
    double* theta = reinterpret_cast<double*>(reinterpret_cast<char*>(region) + P.b_records);
    double* sums = reinterpret_cast<double*>(reinterpret_cast<char*>(region) + P.b_records + P.b_theta);
    if (P.tile > 0) HIP_TRY(launch_oallan_tile(x, n, series_stride, nseries, F, 0, P.tile, records, c->stream));
    if (nt > P.tile) {
        HIP_TRY(launch_oallan_theta(x, n, series_stride, nseries, sums, theta, P.theta_stride, c->stream));
        HIP_TRY(launch_oallan_stream(theta, n, P.theta_stride, nseries, F, P.tile, nt - P.tile, records, c->stream));
    }
    // tau and the variances go straight into the pinned host memory ginsim_allan's sums go to: no copy, one synchronisation
    const size_t nout = (size_t)nt * ((size_t)nseries + 1);
    if (c->allan_host_doubles < nout) {
        if (c->allan_host) { HIP_TRY(hipStreamSynchronize(c->stream)); HIP_TRY(hipHostFree(c->allan_host)); c->allan_host = nullptr; c->allan_host_doubles = 0; }
        HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&c->allan_host), sizeof(double) * (nout + nout / 4 + 64), hipHostMallocDefault));
        c->allan_host_doubles = nout + nout / 4 + 64;
    }
    HIP_TRY(launch_oallan_finish(records, n, nseries, 1.0 / fs, F, c->allan_host, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    const double* h = c->allan_host;
    for (int i = 0; i < nt; ++i) tau[i] = h[i];
    for (int s = 0; s < nseries; ++s)
        for (int i = 0; i < nt; ++i) oavar[(size_t)s * cap + i] = h[(size_t)nt * (s + 1) + i];
    *ntau = nt;
    return GINSIM_OK;
}

// ---- Welch power spectral density (include/ginsim_psd.h, csrc/psd.hip)
int ginsim_psd_plan(int64_t n, int32_t nseries, int64_t series_stride, double fs, int32_t nperseg, int32_t step,
                    ginsim_psd_geometry* g) {
    REQUIRE(g, "psd_plan: NULL argument");
    int rc = psd_check("psd_plan", n, nseries, series_stride, fs, nperseg, step);
    if (rc) return rc;
    PsdShape S;
    rc = psd_plan("psd_plan", n, nseries, nperseg, step, S);
    if (rc) return rc;
    g->segments = S.segments;
    g->scratch_bytes = (int64_t)S.record_bytes;
    g->segs_per_part = S.segs_per_part;
    g->nparts = (int32_t)S.nparts;
    g->lds_bytes = psd_lds_bytes(nperseg);
    g->threads = psd_threads(nperseg);
    return GINSIM_OK;
}

int ginsim_psd_welch(ginsim_ctx* c, const double* x, int64_t n, int32_t nseries, int64_t series_stride, double fs, int32_t nperseg,
                     int32_t step, int32_t window, int32_t detrend, double* freq, double* psd, int32_t* nfreq, int32_t cap) {
    REQUIRE(c && x && freq && psd && nfreq, "psd: NULL argument");
    *nfreq = 0;
    int rc = psd_check("psd", n, nseries, series_stride, fs, nperseg, step);
    if (rc) return rc;
    REQUIRE((window == GINSIM_PSD_BOXCAR || window == GINSIM_PSD_HANN) && (detrend == 0 || detrend == 1),
            "psd: window %d (0 boxcar, 1 hann) or detrend %d (0, 1) out of range", (int)window, (int)detrend);
    PsdShape S;
    rc = psd_plan("psd", n, nseries, nperseg, step, S);
    if (rc) return rc;
    // both launches have the series on the grid's y dimension
    if (nseries > c->max_grid_y) {
        set_error("psd: %d series on the grid's y dimension but the device takes %d: split the batch into calls of at most %d series",
                  (int)nseries, c->max_grid_y, c->max_grid_y);
        return GINSIM_ERR_RANGE;
    }
    const int nb = S.nbins;
    *nfreq = nb;
    if (nb > cap) { set_error("psd: %d frequencies but capacity %d", nb, (int)cap); return GINSIM_ERR_RANGE; }
    HIP_TRY(hipSetDevice(c->device));
    void* region = nullptr;
    HIP_TRY(scratch(c, 1, S.record_bytes, &region));
    double* records = reinterpret_cast<double*>(region);
    HIP_TRY(launch_psd_parts(x, series_stride, nseries, step, window, detrend, S, records, c->stream));
    // the densities go straight into the pinned host memory the Allan results go to: no copy, one synchronisation
    const size_t nout = (size_t)nb * (size_t)nseries;
    if (c->allan_host_doubles < nout) {
        if (c->allan_host) { HIP_TRY(hipStreamSynchronize(c->stream)); HIP_TRY(hipHostFree(c->allan_host)); c->allan_host = nullptr; c->allan_host_doubles = 0; }
        HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&c->allan_host), sizeof(double) * (nout + nout / 4 + 64), hipHostMallocDefault));
        c->allan_host_doubles = nout + nout / 4 + 64;
    }
    const double U = window == GINSIM_PSD_HANN ? 0.375 * (double)nperseg : (double)nperseg;
    HIP_TRY(launch_psd_finish(records, nseries, S, 1.0 / ((double)S.segments * fs * U), c->allan_host, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    const double* h = c->allan_host;
    for (int k = 0; k < nb; ++k) freq[k] = (double)k * fs / (double)nperseg;
    for (int s = 0; s < nseries; ++s) memcpy(psd + (size_t)s * cap, h + (size_t)s * nb, sizeof(double) * nb);
    return GINSIM_OK;
}

// ---- Welch cross-spectral density between pairs of series (include/ginsim_csd.h, csrc/csd.hip)
// The refusals that ginsim_csd_welch and ginsim_csd_plan share, in the order include/ginsim_csd.h states and under the caller's
// prefix: the sizes, the pair count, the segment length and step (the call checks window, detrend and the pair table after this).
static int csd_check(const char* who, int64_t n, int32_t nseries, int64_t series_stride, double fs, int32_t npairs, int32_t nperseg,
                     int32_t step) {
    REQUIRE(n >= 1 && nseries >= 1 && series_stride >= n && fs > 0 && std::isfinite(fs), "%s: bad sizes", who);
    REQUIRE(npairs >= 1, "%s: npairs %d: a call needs at least one pair", who, (int)npairs);
    REQUIRE(nperseg != (1 << kPsdMaxLog2),
            "%s: nperseg %d is not taken: a workgroup keeps four sums per bin in registers and at %d the PSD kernel, with one, already "
            "holds 254 of 256; the largest segment is %d", who, (int)nperseg, (int)nperseg, 1 << kCsdMaxLog2);
    REQUIRE(nperseg >= (1 << kCsdMinLog2) && nperseg <= (1 << kCsdMaxLog2) && (nperseg & (nperseg - 1)) == 0,
            "%s: nperseg %d is not a power of two in [%d, %d]", who, (int)nperseg, 1 << kCsdMinLog2, 1 << kCsdMaxLog2);
    REQUIRE(step >= 1 && step <= nperseg, "%s: step %d outside [1, %d]", who, (int)step, (int)nperseg);
    return GINSIM_OK;
}

// the shape (psd.hpp's partition of one series) and the scratch of a call: records, then the pair table
static int csd_plan(const char* who, int64_t n, int32_t npairs, int32_t nperseg, int32_t step, PsdShape& S, size_t& table_bytes) {
    if (n < nperseg) {
        set_error("%s: a series of n = %lld samples is shorter than one segment of nperseg = %d", who, (long long)n, (int)nperseg);
        return GINSIM_ERR_RANGE;
    }
    PsdShape s = psd_plan_shape(n, nperseg, step);     // a local: a refused plan leaves the caller's as it was
    if (s.nparts > kPsdMaxParts) {
        set_error("%s: %lld segments in parts of %d are %lld parts per pair, more than the %lld a call can have: analyse the series in pieces",
                  who, (long long)s.segments, (int)s.segs_per_part, (long long)s.nparts, (long long)kPsdMaxParts);
        return GINSIM_ERR_RANGE;
    }
    size_t tb = 0;
    if (!csd_scratch_bytes(s, npairs, tb)) {
        set_error("%s: the records of %lld parts per pair and %d pairs, %d sums each, pass 2^63 bytes: split the table or the series",
                  who, (long long)s.nparts, (int)npairs, kCsdPlanes * (int)s.nbins);
        return GINSIM_ERR_RANGE;
    }
    S = s;
    table_bytes = tb;
    return GINSIM_OK;
}

int ginsim_csd_plan(int64_t n, int32_t nseries, int64_t series_stride, double fs, int32_t npairs, int32_t nperseg, int32_t step,
                    ginsim_csd_geometry* g) {
    REQUIRE(g, "csd_plan: NULL argument");
    int rc = csd_check("csd_plan", n, nseries, series_stride, fs, npairs, nperseg, step);
    if (rc) return rc;
    PsdShape S;
    size_t tb = 0;
    rc = csd_plan("csd_plan", n, npairs, nperseg, step, S, tb);
    if (rc) return rc;
    g->segments = S.segments;
    g->scratch_bytes = (int64_t)(S.record_bytes + tb);
    g->segs_per_part = S.segs_per_part;
    g->nparts = (int32_t)S.nparts;
    g->lds_bytes = csd_lds_bytes(nperseg);
    g->threads = csd_threads(nperseg);
    return GINSIM_OK;
}

int ginsim_csd_welch(ginsim_ctx* c, const double* x, int64_t n, int32_t nseries, int64_t series_stride, double fs,
                     const int32_t* pairs, int32_t npairs, int32_t nperseg, int32_t step, int32_t window, int32_t detrend,
                     double* freq, double* pxx, double* pyy, double* pxy_re, double* pxy_im, int32_t* nfreq, int32_t cap) {
    REQUIRE(c && x && pairs && freq && pxx && pyy && pxy_re && pxy_im && nfreq, "csd: NULL argument");
    *nfreq = 0;
    int rc = csd_check("csd", n, nseries, series_stride, fs, npairs, nperseg, step);
    if (rc) return rc;
    REQUIRE((window == GINSIM_PSD_BOXCAR || window == GINSIM_PSD_HANN) && (detrend == 0 || detrend == 1),
            "csd: window %d (0 boxcar, 1 hann) or detrend %d (0, 1) out of range", (int)window, (int)detrend);
    for (int32_t p = 0; p < npairs; ++p)
        REQUIRE(pairs[2 * p] >= 0 && pairs[2 * p] < nseries && pairs[2 * p + 1] >= 0 && pairs[2 * p + 1] < nseries,
                "csd: pair %d is (%d, %d) but the series are 0 .. %d", (int)p, (int)pairs[2 * p], (int)pairs[2 * p + 1], (int)nseries - 1);
    PsdShape S;
    size_t tb = 0;
    rc = csd_plan("csd", n, npairs, nperseg, step, S, tb);
    if (rc) return rc;
    // both launches have the pairs on the grid's y dimension
    if (npairs > c->max_grid_y) {
        set_error("csd: %d pairs on the grid's y dimension but the device takes %d: split the table into calls of at most %d pairs",
                  (int)npairs, c->max_grid_y, c->max_grid_y);
        return GINSIM_ERR_RANGE;
    }
    const int nb = S.nbins;
    *nfreq = nb;
    if (nb > cap) { set_error("csd: %d frequencies but capacity %d", nb, (int)cap); return GINSIM_ERR_RANGE; }
    HIP_TRY(hipSetDevice(c->device));
    void* region = nullptr;
    HIP_TRY(scratch(c, 1, S.record_bytes + tb, &region));
    double* records = reinterpret_cast<double*>(region);
    int32_t* d_pairs = reinterpret_cast<int32_t*>(reinterpret_cast<char*>(region) + S.record_bytes);
    // the table once per call; the copy has read the caller's (pageable) array when it returns
    HIP_TRY(hipMemcpyAsync(d_pairs, pairs, sizeof(int32_t) * 2 * (size_t)npairs, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(launch_csd_parts(x, series_stride, d_pairs, npairs, step, window, detrend, S, records, c->stream));
    // the four planes go straight into the pinned host memory the Allan and PSD results go to: no copy, one synchronisation
    const size_t plane = (size_t)nb * (size_t)npairs, nout = kCsdPlanes * plane;
    if (c->allan_host_doubles < nout) {
        if (c->allan_host) { HIP_TRY(hipStreamSynchronize(c->stream)); HIP_TRY(hipHostFree(c->allan_host)); c->allan_host = nullptr; c->allan_host_doubles = 0; }
        HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&c->allan_host), sizeof(double) * (nout + nout / 4 + 64), hipHostMallocDefault));
        c->allan_host_doubles = nout + nout / 4 + 64;
    }
    const double U = window == GINSIM_PSD_HANN ? 0.375 * (double)nperseg : (double)nperseg;
    HIP_TRY(launch_csd_finish(records, npairs, S, 1.0 / ((double)S.segments * fs * U), c->allan_host, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    const double* h = c->allan_host;
    double* const outs[kCsdPlanes] = {pxx, pyy, pxy_re, pxy_im};
    for (int k = 0; k < nb; ++k) freq[k] = (double)k * fs / (double)nperseg;
    for (int q = 0; q < kCsdPlanes; ++q)
        for (int p = 0; p < npairs; ++p) memcpy(outs[q] + (size_t)p * cap, h + q * plane + (size_t)p * nb, sizeof(double) * nb);
    return GINSIM_OK;
}

// ---- multi-resolution PSD: Welch's estimate on a decimating octave cascade (include/ginsim_lpsd.h, csrc/lpsd.hip)
int ginsim_decimate2(ginsim_ctx* c, const double* x, int64_t n, int32_t nseries, int64_t series_stride, double* y, int64_t y_stride,
                     int64_t* n_out) {
    REQUIRE(c && x && y && n_out, "decimate2: NULL argument");
    *n_out = 0;
    REQUIRE(nseries >= 1 && n >= kHalfbandTaps && series_stride >= n,
            "decimate2: bad sizes (n = %lld must be at least %d, series_stride at least n)", (long long)n, kHalfbandTaps);
    const int64_t no = decimate2_outputs(n);
    *n_out = no;
    if (y_stride < no) { set_error("decimate2: y_stride %lld is below the %lld outputs of a series", (long long)y_stride, (long long)no); return GINSIM_ERR_RANGE; }
    // the ranges x[0 .. (nseries-1) series_stride + n) and y[0 .. (nseries-1) y_stride + n_out), in bytes; a product past 64 bits
    // cannot be an allocation
    const __int128 xb = ((__int128)(nseries - 1) * series_stride + n) * 8, yb = ((__int128)(nseries - 1) * y_stride + no) * 8;
    const __int128 xa = (__int128)(uintptr_t)x, ya = (__int128)(uintptr_t)y;
    if (xa < ya + yb && ya < xa + xb) { set_error("decimate2: the ranges of x and y overlap"); return GINSIM_ERR_RANGE; }
    if (decimate2_tiles(no) > kDecMaxTiles) {
        set_error("decimate2: %lld outputs are %lld tiles of %d, more than the %lld a launch can have", (long long)no,
                  (long long)decimate2_tiles(no), kDecTile, (long long)kDecMaxTiles);
        return GINSIM_ERR_RANGE;
    }
    if (nseries > c->max_grid_y) {
        set_error("decimate2: %d series on the grid's y dimension but the device takes %d: split the batch into calls of at most %d series",
                  (int)nseries, c->max_grid_y, c->max_grid_y);
        return GINSIM_ERR_RANGE;
    }
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(launch_decimate2(x, n, series_stride, nseries, y, y_stride, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return GINSIM_OK;
}

int ginsim_lpsd_plan(int64_t n, int32_t nseries, int64_t series_stride, double fs, int32_t nperseg, int32_t step,
                     int32_t min_segments, ginsim_lpsd_geometry* g) {
    REQUIRE(g, "lpsd_plan: NULL argument");
    int rc = psd_check("lpsd_plan", n, nseries, series_stride, fs, nperseg, step);
    if (rc) return rc;
    PsdShape S0;
    rc = psd_plan("lpsd_plan", n, nseries, nperseg, step, S0);
    if (rc) return rc;
    LpsdPlan P;
    rc = lpsd_plan("lpsd_plan", n, nseries, nperseg, step, min_segments, S0, P);
    if (rc) return rc;
    memset(g, 0, sizeof(*g));
    g->scratch_bytes = (int64_t)P.bytes();
    g->levels = P.lv.levels;
    g->nbins = P.lv.nbins;
    for (int j = 0; j < P.lv.levels; ++j) {
        g->level[j].n = P.lv.n[j];
        g->level[j].segments = P.lv.S[j].segments;
        g->level[j].first_bin = P.lv.first_bin[j];
        g->level[j].bins = P.lv.bins[j];
        g->level[j].nparts = (int32_t)P.lv.S[j].nparts;
    }
    return GINSIM_OK;
}

int ginsim_lpsd(ginsim_ctx* c, const double* x, int64_t n, int32_t nseries, int64_t series_stride, double fs, int32_t nperseg,
                int32_t step, int32_t window, int32_t detrend, int32_t min_segments, double* freq, double* psd, int32_t* level,
                int32_t* nbins, int32_t cap) {
    REQUIRE(c && x && freq && psd && level && nbins, "lpsd: NULL argument");
    *nbins = 0;
    int rc = psd_check("lpsd", n, nseries, series_stride, fs, nperseg, step);
    if (rc) return rc;
    REQUIRE((window == GINSIM_PSD_BOXCAR || window == GINSIM_PSD_HANN) && (detrend == 0 || detrend == 1),
            "lpsd: window %d (0 boxcar, 1 hann) or detrend %d (0, 1) out of range", (int)window, (int)detrend);
    PsdShape S0;
    rc = psd_plan("lpsd", n, nseries, nperseg, step, S0);
    if (rc) return rc;
    // every launch has the series on the grid's y dimension
    if (nseries > c->max_grid_y) {
        set_error("lpsd: %d series on the grid's y dimension but the device takes %d: split the batch into calls of at most %d series",
                  (int)nseries, c->max_grid_y, c->max_grid_y);
        return GINSIM_ERR_RANGE;
    }
    LpsdPlan P;
    rc = lpsd_plan("lpsd", n, nseries, nperseg, step, min_segments, S0, P);
    if (rc) return rc;
    const LpsdLevels& lv = P.lv;
    const int nb = lv.nbins, full = S0.nbins;
    *nbins = nb;
    if (nb > cap) { set_error("lpsd: %d bins but capacity %d", nb, (int)cap); return GINSIM_ERR_RANGE; }
    HIP_TRY(hipSetDevice(c->device));
    void* region = nullptr;
    HIP_TRY(scratch(c, 1, P.bytes(), &region));
    char* base = reinterpret_cast<char*>(region);
    double* buf[2] = {reinterpret_cast<double*>(base), reinterpret_cast<double*>(base + P.b_level[0])};
    double* records = reinterpret_cast<double*>(base + P.b_level[0] + P.b_level[1]);
    double* dens = reinterpret_cast<double*>(base + P.b_level[0] + P.b_level[1] + P.b_records);
    // the reported bins go to the pinned host memory the Allan results go to, [nseries][nb]: one synchronisation at the end
    const size_t nout = (size_t)nb * (size_t)nseries;
    if (c->allan_host_doubles < nout) {
        if (c->allan_host) { HIP_TRY(hipStreamSynchronize(c->stream)); HIP_TRY(hipHostFree(c->allan_host)); c->allan_host = nullptr; c->allan_host_doubles = 0; }
        HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&c->allan_host), sizeof(double) * (nout + nout / 4 + 64), hipHostMallocDefault));
        c->allan_host_doubles = nout + nout / 4 + 64;
    }
    const double U = window == GINSIM_PSD_HANN ? 0.375 * (double)nperseg : (double)nperseg;
    const double* xj = x;                   // level j's series and their stride: the caller's, then the level buffers in turn
    int64_t stride_j = series_stride;
    double fs_j = fs;
    int col = nb;                           // level 0 is the last block of columns of the output
    for (int j = 0; j < lv.levels; ++j) {
        const PsdShape& S = lv.S[j];
        HIP_TRY(launch_psd_parts(xj, stride_j, nseries, step, window, detrend, S, records, c->stream));
        HIP_TRY(launch_psd_finish(records, nseries, S, 1.0 / ((double)S.segments * fs_j * U), dens, c->stream));
        col -= lv.bins[j];
        HIP_TRY(launch_lpsd_report(dens, nseries, full, lv.first_bin[j], lv.bins[j], c->allan_host + col, nb, c->stream));
        for (int k = 0; k < lv.bins[j]; ++k) {
            freq[col + k] = (double)(lv.first_bin[j] + k) * fs_j / (double)nperseg;
            level[col + k] = j;
        }
        if (j + 1 < lv.levels) {
            double* out = buf[j & 1];       // level j + 1: odd levels in the first buffer, even ones in the second
            HIP_TRY(launch_decimate2(xj, lv.n[j], stride_j, nseries, out, lv.n[j + 1], c->stream));
            xj = out;
            stride_j = lv.n[j + 1];
            fs_j *= 0.5;
        }
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    const double* h = c->allan_host;
    for (int s = 0; s < nseries; ++s) memcpy(psd + (size_t)s * cap, h + (size_t)s * nb, sizeof(double) * nb);
    return GINSIM_OK;
}

int ginsim_rng_normals(ginsim_ctx* c, uint64_t seed, uint64_t run, uint32_t stream, int64_t count, double* host_z0,
                       double* host_z1, uint32_t* host_words) {
    REQUIRE(c && host_z0 && host_z1 && count >= 1, "rng_normals: bad arguments");
    HIP_TRY(hipSetDevice(c->device));
    DevBuf z0, z1, w;
    HIP_TRY(z0.alloc(sizeof(double) * count));
    HIP_TRY(z1.alloc(sizeof(double) * count));
    HIP_TRY(w.alloc(sizeof(uint32_t) * 4 * count));
    HIP_TRY(launch_rng_probe(seed, run, stream, count, z0.as<double>(), z1.as<double>(),
                             host_words ? w.as<uint32_t>() : nullptr, c->stream));
    HIP_TRY(hipMemcpyAsync(host_z0, z0.p, sizeof(double) * count, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(host_z1, z1.p, sizeof(double) * count, hipMemcpyDeviceToHost, c->stream));
    if (host_words)
        HIP_TRY(hipMemcpyAsync(host_words, w.p, sizeof(uint32_t) * 4 * count, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return GINSIM_OK;
}

int ginsim_runs_to_series(ginsim_ctx* c, const double* series, int32_t ncomp, int64_t n, int64_t runs, double* out) {
    REQUIRE(c && series && out && series != out, "runs_to_series: bad pointers");
    REQUIRE(ncomp >= 1 && ncomp <= 65535 && n >= 1 && runs >= 1 && (runs + 63) / 64 <= 65535, "runs_to_series: bad sizes");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(launch_runs_to_series(series, out, ncomp, n, runs, c->stream));
    return GINSIM_OK;
}

int ginsim_normal_transform(ginsim_ctx* c, const uint32_t* host_words, int64_t count, double* host_z0, double* host_z1) {
    REQUIRE(c && host_words && host_z0 && host_z1 && count >= 1, "normal_transform: bad arguments");
    HIP_TRY(hipSetDevice(c->device));
    DevBuf z0, z1, w;
    HIP_TRY(z0.alloc(sizeof(double) * count));
    HIP_TRY(z1.alloc(sizeof(double) * count));
    HIP_TRY(w.alloc(sizeof(uint32_t) * 4 * count));
    HIP_TRY(hipMemcpyAsync(w.p, host_words, sizeof(uint32_t) * 4 * count, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(launch_normal_transform(w.as<uint32_t>(), count, z0.as<double>(), z1.as<double>(), c->stream));
    HIP_TRY(hipMemcpyAsync(host_z0, z0.p, sizeof(double) * count, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(host_z1, z1.p, sizeof(double) * count, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return GINSIM_OK;
}

// ---- ABI 9: memory self-test (csrc/selftest.hip)
static int selftest_args(ginsim_ctx* c, const void* dptr, size_t bytes, const char* what) {
    REQUIRE(c && (bytes == 0 || dptr), "%s: bad arguments", what);
    REQUIRE(bytes % 8 == 0 && ((uintptr_t)dptr & 7) == 0, "%s: the region must be whole, aligned 64-bit words", what);
    REQUIRE(bytes / 8 < ((uint64_t)1 << 40), "%s: more than 2^40 words", what);
    HIP_TRY(hipSetDevice(c->device));
    if (!c->selftest) HIP_TRY(hipMalloc(&c->selftest, 4 * sizeof(unsigned long long)));
    return GINSIM_OK;
}

int ginsim_pattern_fill(ginsim_ctx* c, void* dptr, size_t bytes, uint32_t tag) {
    const int rc = selftest_args(c, dptr, bytes, "pattern_fill");
    if (rc) return rc;
    if (bytes) HIP_TRY(launch_pattern_fill(dptr, bytes / 8, tag, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return GINSIM_OK;
}

int ginsim_pattern_check(ginsim_ctx* c, const void* dptr, size_t bytes, uint32_t tag, int64_t* bad, int64_t* first_bad_offset,
                         uint64_t* found) {
    REQUIRE(bad && first_bad_offset && found, "pattern_check: NULL output");
    const int rc = selftest_args(c, dptr, bytes, "pattern_check");
    if (rc) return rc;
    *bad = 0; *first_bad_offset = -1; *found = 0;
    if (!bytes) return GINSIM_OK;
    unsigned long long h[3] = {0, 0, 0};
    HIP_TRY(launch_pattern_check(dptr, bytes / 8, tag, c->selftest, c->stream));
    HIP_TRY(hipMemcpyAsync(h, c->selftest, sizeof(h), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    *bad = (int64_t)h[0];
    if (h[0]) { *first_bad_offset = (int64_t)(h[1] * 8); *found = h[2]; }
    return GINSIM_OK;
}

int ginsim_digest(ginsim_ctx* c, const void* dptr, size_t bytes, uint64_t* out) {
    REQUIRE(out, "digest: NULL output");
    const int rc = selftest_args(c, dptr, bytes, "digest");
    if (rc) return rc;
    *out = 0;
    if (!bytes) return GINSIM_OK;
    unsigned long long h = 0;
    HIP_TRY(launch_digest(dptr, bytes / 8, c->selftest, c->stream));
    HIP_TRY(hipMemcpyAsync(&h, c->selftest, sizeof(h), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    *out = (uint64_t)h;
    return GINSIM_OK;
}

}  // extern "C"
