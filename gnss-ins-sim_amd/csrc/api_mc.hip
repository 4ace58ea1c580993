// C ABI glue of the launches that synthesise sensors and run algorithms on them (include/ginsim.h, ginsim_loose_all.h,
// ginsim_loose_all_cons.h): the checks and entry points of the Monte-Carlo, inclinometer and InsLoose families, the auxiliary
// sensors, MagCal, the PSD vibration series and the given-data mechanisation.  No kernels here.
#include "api_common.hpp"
#include "ginsim_loose_all.h"
#include "ginsim_loose_all_cons.h"

using namespace ginsim;

extern "C" {

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
        if (tb) HIP_TRY(scratch(c, WS_MC, tb, &truth32));
        HIP_TRY(launch_mc_f32(*p, reinterpret_cast<float*>(truth32), c->stream, nullptr, 0));
    } else if (series_path_applies(*p)) {       // sensors only, few runs, long series: parallel along time
        int32_t L = 0;
        const int64_t nchunks = series_chunks(*p, &L);
        void* carry = nullptr;
        HIP_TRY(scratch(c, WS_MC, sizeof(double) * 6 * (size_t)nchunks * (size_t)p->runs, &carry));
        HIP_TRY(launch_series(*p, reinterpret_cast<double*>(carry), c->stream));
    } else {
        void* about = nullptr;          // the launch-wide shift of the online process statistics (mc_kernel.hip, Proc): nine doubles
        if (p->out_proc[0] || p->out_proc[1]) HIP_TRY(scratch(c, WS_MC, 9 * sizeof(double), &about));
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
        HIP_TRY(scratch(c, WS_MC, sb + vb + cb, &ws));
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
    HIP_TRY(scratch(c, WS_MC, vib_psd_scratch_bytes(period, runs), &ws));
    return launch_vib_psd(c->device, c->stream, amp, period, runs, run_offset, seed, sensor, halve_per_run, ws, out);
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

}  // extern "C"
