// The core of the C ABI of libginsim.so (declared in include/ginsim.h): error reporting, the context and its scratch, memory,
// the placed arena, timers, the RCCL exchange, the RNG probes and the memory self-test.  The entry points of the series analyses
// are in api_series.hip, those of the Monte-Carlo, inclinometer and filter launches in api_mc.hip, the readers of kept trajectories
// and the gathers in api_traj.hip; api_common.hpp is what the four share.  No kernels here.
#include <cstdarg>
#include <string>

#include "api_common.hpp"
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

hipError_t scratch(ginsim_ctx* c, Scratch slot, size_t bytes, void** out) {
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
    if (c->series_host) (void)hipHostFree(c->series_host);
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
int ginsim_stream_first_xcc(ginsim_ctx* c, int32_t* xcc) {
    REQUIRE(c && xcc, "stream_first_xcc: NULL argument");
    HIP_TRY(hipSetDevice(c->device));
    void* ws = nullptr;
    HIP_TRY(scratch(c, WS_TRAJ, 64, &ws));
    HIP_TRY(launch_first_xcc(reinterpret_cast<uint32_t*>(ws), c->stream));
    uint32_t v = 0;
    HIP_TRY(hipMemcpyAsync(&v, ws, sizeof v, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    *xcc = (int32_t)v;
    return GINSIM_OK;
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
    HIP_TRY(scratch(c, WS_STATS, wb, &ws));
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
