// C ABI glue of the series analyses (include/ginsim.h's Allan variance, ginsim_oallan.h, ginsim_psd.h, ginsim_csd.h, ginsim_lpsd.h):
// what a call runs is planned on the host, and the entry points launch from the plan that the *_plan entry points report.  What the
// five families share -- the pinned result buffer, the grid's y limit, the window check, Welch's normalisation -- is stated once,
// below the plans.  No kernels here.
#include <string>

#include "api_common.hpp"
#include "ginsim_oallan.h"
#include "ginsim_psd.h"
#include "ginsim_lpsd.h"
#include "ginsim_csd.h"
#include "allan.hpp"
#include "oallan.hpp"
#include "psd.hpp"
#include "lpsd.hpp"
#include "csd.hpp"

using namespace ginsim;

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

// ---- what the entry points of the five families share
// The pinned host memory that the finishing launches write their results into (no copy, one synchronisation per call), grown to at
// least `doubles`.  The stream is drained before the old buffer goes: a launch of an earlier call may still write it.
static int result_buffer(ginsim_ctx* c, size_t doubles, double** out) {
    if (c->series_host_doubles < doubles) {
        if (c->series_host) { HIP_TRY(hipStreamSynchronize(c->stream)); HIP_TRY(hipHostFree(c->series_host)); c->series_host = nullptr; c->series_host_doubles = 0; }
        HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&c->series_host), sizeof(double) * (doubles + doubles / 4 + 64), hipHostMallocDefault));
        c->series_host_doubles = doubles + doubles / 4 + 64;
    }
    *out = c->series_host;
    return GINSIM_OK;
}

// `count` of `what` on the grid's y dimension ("series" of a "batch", "pairs" of a "table") against what the device takes there
static int check_grid_y(const char* who, const ginsim_ctx* c, int32_t count, const char* what, const char* whole) {
    if (count <= c->max_grid_y) return GINSIM_OK;
    set_error("%s: %d %s on the grid's y dimension but the device takes %d: split the %s into calls of at most %d %s", who, (int)count,
              what, c->max_grid_y, whole, c->max_grid_y, what);
    return GINSIM_ERR_RANGE;
}

static int check_window(const char* who, int32_t window, int32_t detrend) {
    REQUIRE((window == GINSIM_PSD_BOXCAR || window == GINSIM_PSD_HANN) && (detrend == 0 || detrend == 1),
            "%s: window %d (0 boxcar, 1 hann) or detrend %d (0, 1) out of range", who, (int)window, (int)detrend);
    return GINSIM_OK;
}

// Welch's density scale, 1 / (segments fs U); U, the sum of the squared window: nperseg (boxcar) or 3/8 of it (Hann)
static double welch_scale(int32_t window, int32_t nperseg, int64_t segments, double fs) {
    const double U = window == GINSIM_PSD_HANN ? 0.375 * (double)nperseg : (double)nperseg;
    return 1.0 / ((double)segments * fs * U);
}

extern "C" {

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
    if (!P.steps.empty())
        if (const int e = check_grid_y("allan", c, nseries, "series", "batch")) return e;
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
    HIP_TRY(scratch(c, WS_SERIES, b_ping + b_pong + b_part + b_sums + 1024, &region));
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
    double* h = nullptr;
    if (const int e = result_buffer(c, (size_t)9 * nseries * levels, &h)) return e;
    HIP_TRY(launch_allan_finish(in, partial.d(), h, t, fold, nseries, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
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
    if (const int e = check_grid_y("oallan", c, nseries, "series", "batch")) return e;
    if (nt > cap) { set_error("oallan: %d averaging factors but capacity %d", nt, cap); return GINSIM_ERR_RANGE; }
    HIP_TRY(hipSetDevice(c->device));
    void* region = nullptr;
    HIP_TRY(scratch(c, WS_SERIES, P.b_records + P.b_theta + P.b_sums, &region));
    double* records = reinterpret_cast<double*>(region);
    double* theta = reinterpret_cast<double*>(reinterpret_cast<char*>(region) + P.b_records);
    double* sums = reinterpret_cast<double*>(reinterpret_cast<char*>(region) + P.b_records + P.b_theta);
    if (P.tile > 0) HIP_TRY(launch_oallan_tile(x, n, series_stride, nseries, F, 0, P.tile, records, c->stream));
    if (nt > P.tile) {
        HIP_TRY(launch_oallan_theta(x, n, series_stride, nseries, sums, theta, P.theta_stride, c->stream));
        HIP_TRY(launch_oallan_stream(theta, n, P.theta_stride, nseries, F, P.tile, nt - P.tile, records, c->stream));
    }
    // tau and the variances go straight into pinned host memory: no copy, one synchronisation
    double* h = nullptr;
    if (const int e = result_buffer(c, (size_t)nt * ((size_t)nseries + 1), &h)) return e;
    HIP_TRY(launch_oallan_finish(records, n, nseries, 1.0 / fs, F, h, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
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
    rc = check_window("psd", window, detrend);
    if (rc) return rc;
    PsdShape S;
    rc = psd_plan("psd", n, nseries, nperseg, step, S);
    if (rc) return rc;
    // both launches have the series on the grid's y dimension
    rc = check_grid_y("psd", c, nseries, "series", "batch");
    if (rc) return rc;
    const int nb = S.nbins;
    *nfreq = nb;
    if (nb > cap) { set_error("psd: %d frequencies but capacity %d", nb, (int)cap); return GINSIM_ERR_RANGE; }
    HIP_TRY(hipSetDevice(c->device));
    void* region = nullptr;
    HIP_TRY(scratch(c, WS_SERIES, S.record_bytes, &region));
    double* records = reinterpret_cast<double*>(region);
    HIP_TRY(launch_psd_parts(x, series_stride, nseries, step, window, detrend, S, records, c->stream));
    // the densities go straight into pinned host memory: no copy, one synchronisation
    double* h = nullptr;
    rc = result_buffer(c, (size_t)nb * (size_t)nseries, &h);
    if (rc) return rc;
    HIP_TRY(launch_psd_finish(records, nseries, S, welch_scale(window, nperseg, S.segments, fs), h, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
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
    rc = check_window("csd", window, detrend);
    if (rc) return rc;
    for (int32_t p = 0; p < npairs; ++p)
        REQUIRE(pairs[2 * p] >= 0 && pairs[2 * p] < nseries && pairs[2 * p + 1] >= 0 && pairs[2 * p + 1] < nseries,
                "csd: pair %d is (%d, %d) but the series are 0 .. %d", (int)p, (int)pairs[2 * p], (int)pairs[2 * p + 1], (int)nseries - 1);
    PsdShape S;
    size_t tb = 0;
    rc = csd_plan("csd", n, npairs, nperseg, step, S, tb);
    if (rc) return rc;
    // both launches have the pairs on the grid's y dimension
    rc = check_grid_y("csd", c, npairs, "pairs", "table");
    if (rc) return rc;
    const int nb = S.nbins;
    *nfreq = nb;
    if (nb > cap) { set_error("csd: %d frequencies but capacity %d", nb, (int)cap); return GINSIM_ERR_RANGE; }
    HIP_TRY(hipSetDevice(c->device));
    void* region = nullptr;
    HIP_TRY(scratch(c, WS_SERIES, S.record_bytes + tb, &region));
    double* records = reinterpret_cast<double*>(region);
    int32_t* d_pairs = reinterpret_cast<int32_t*>(reinterpret_cast<char*>(region) + S.record_bytes);
    // the table once per call; the copy has read the caller's (pageable) array when it returns
    HIP_TRY(hipMemcpyAsync(d_pairs, pairs, sizeof(int32_t) * 2 * (size_t)npairs, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(launch_csd_parts(x, series_stride, d_pairs, npairs, step, window, detrend, S, records, c->stream));
    // the four planes go straight into pinned host memory: no copy, one synchronisation
    const size_t plane = (size_t)nb * (size_t)npairs;
    double* h = nullptr;
    rc = result_buffer(c, kCsdPlanes * plane, &h);
    if (rc) return rc;
    HIP_TRY(launch_csd_finish(records, npairs, S, welch_scale(window, nperseg, S.segments, fs), h, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
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
    if (const int e = check_grid_y("decimate2", c, nseries, "series", "batch")) return e;
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
    rc = check_window("lpsd", window, detrend);
    if (rc) return rc;
    PsdShape S0;
    rc = psd_plan("lpsd", n, nseries, nperseg, step, S0);
    if (rc) return rc;
    // every launch has the series on the grid's y dimension
    rc = check_grid_y("lpsd", c, nseries, "series", "batch");
    if (rc) return rc;
    LpsdPlan P;
    rc = lpsd_plan("lpsd", n, nseries, nperseg, step, min_segments, S0, P);
    if (rc) return rc;
    const LpsdLevels& lv = P.lv;
    const int nb = lv.nbins, full = S0.nbins;
    *nbins = nb;
    if (nb > cap) { set_error("lpsd: %d bins but capacity %d", nb, (int)cap); return GINSIM_ERR_RANGE; }
    HIP_TRY(hipSetDevice(c->device));
    void* region = nullptr;
    HIP_TRY(scratch(c, WS_SERIES, P.bytes(), &region));
    char* base = reinterpret_cast<char*>(region);
    double* buf[2] = {reinterpret_cast<double*>(base), reinterpret_cast<double*>(base + P.b_level[0])};
    double* records = reinterpret_cast<double*>(base + P.b_level[0] + P.b_level[1]);
    double* dens = reinterpret_cast<double*>(base + P.b_level[0] + P.b_level[1] + P.b_records);
    // the reported bins go to pinned host memory, [nseries][nb]: one synchronisation at the end
    double* h = nullptr;
    rc = result_buffer(c, (size_t)nb * (size_t)nseries, &h);
    if (rc) return rc;
    const double* xj = x;                   // level j's series and their stride: the caller's, then the level buffers in turn
    int64_t stride_j = series_stride;
    double fs_j = fs;
    int col = nb;                           // level 0 is the last block of columns of the output
    for (int j = 0; j < lv.levels; ++j) {
        const PsdShape& S = lv.S[j];
        HIP_TRY(launch_psd_parts(xj, stride_j, nseries, step, window, detrend, S, records, c->stream));
        HIP_TRY(launch_psd_finish(records, nseries, S, welch_scale(window, nperseg, S.segments, fs_j), dens, c->stream));
        col -= lv.bins[j];
        HIP_TRY(launch_lpsd_report(dens, nseries, full, lv.first_bin[j], lv.bins[j], h + col, nb, c->stream));
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
    for (int s = 0; s < nseries; ++s) memcpy(psd + (size_t)s * cap, h + (size_t)s * nb, sizeof(double) * nb);
    return GINSIM_OK;
}

}  // extern "C"
