// C ABI glue of what reads kept series and trajectories (include/ginsim.h): the end-point and process statistics, the across-run
// curves, quantile keys and covariance with their host merges, and the gathers.  No kernels here.
#include "api_common.hpp"

using namespace ginsim;

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
    HIP_TRY(scratch(c, WS_TRAJ, body + sizeof(int64_t) * (size_t)v.m, &ws));
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

extern "C" {

int ginsim_end_stats(ginsim_ctx* c, const double* end_err, int64_t runs, ginsim_stats* host_out) {
    REQUIRE(c && end_err && host_out && runs >= 1, "end_stats: bad arguments");
    HIP_TRY(hipSetDevice(c->device));
    void* ws = nullptr;
    HIP_TRY(scratch(c, WS_STATS, stats_scratch_bytes(runs), &ws));
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
    HIP_TRY(scratch(c, WS_STATS, stats_scratch_bytes(runs), &ws));
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

// The per-run statistics of kept trajectories (stats.hip's process kernel) in the context's scratch.  proc_out: the records of the
// samples >= first_sample, [runs][3][9], to the host.  end_out (proc_out NULL): a one-sample window at n - 1, whose "mean" plane
// [9][runs] IS the end-point error, reduced by ginsim_end_stats.
static int traj_stats_run(ginsim_ctx* c, const TrajView& v, int64_t first_sample, int32_t pos_ned, double* proc_out, ginsim_stats* end_out) {
    HIP_TRY(hipSetDevice(c->device));
    void* ws = nullptr;
    const size_t bytes = sizeof(double) * 27 * (size_t)v.runs;
    HIP_TRY(scratch(c, WS_TRAJ, bytes, &ws));
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
    HIP_TRY(scratch(c, WS_TRAJ, sizeof(double) * (size_t)q + res, &ws));
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

int ginsim_runs_to_series(ginsim_ctx* c, const double* series, int32_t ncomp, int64_t n, int64_t runs, double* out) {
    REQUIRE(c && series && out && series != out, "runs_to_series: bad pointers");
    REQUIRE(ncomp >= 1 && ncomp <= 65535 && n >= 1 && runs >= 1 && (runs + 63) / 64 <= 65535, "runs_to_series: bad sizes");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(launch_runs_to_series(series, out, ncomp, n, runs, c->stream));
    return GINSIM_OK;
}

}  // extern "C"
