/*
 * ginsim.h -- C ABI of the MI355X-native Monte-Carlo strapdown-INS engine (libginsim.so).
 *
 * This is the drop-in boundary for ONE hot path of Aceinna/gnss-ins-sim:
 *     pathgen.path_gen  ->  acc_gen / gyro_gen / bias_drift  ->  FreeIntegration.run  ->  end-point stats
 * Style mirrors the reference's own FFI precedent (demo_algorithms/mag_calibrate.py:44,78-86 and
 * demo_algorithms/aceinna_ins.py:172-237): extern "C" functions, POD structs by pointer, caller-owned
 * row-major double buffers, explicit sizes.  Unlike the precedent every function returns an int status
 * (0 = ok, <0 = error) and never aborts; ginsim_last_error() returns the thread-local message.
 *
 * All reference citations are relative to the reference repository root.
 */
#ifndef GINSIM_H
#define GINSIM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GINSIM_ABI_VERSION 9

/* status codes */
#define GINSIM_OK          0
#define GINSIM_ERR_ARG    -1   /* bad argument (Python wrapper raises ValueError, like the reference) */
#define GINSIM_ERR_HIP    -2   /* HIP runtime error (message holds hipGetErrorString) */
#define GINSIM_ERR_NODEV  -3   /* no usable GPU */
#define GINSIM_ERR_RANGE  -4   /* output capacity too small */
#define GINSIM_ERR_NOMEM  -5   /* ABI 7: the device is out of memory (hipErrorOutOfMemory): the one failure a caller may retry after
                                * giving memory back; every other HIP failure stays GINSIM_ERR_HIP */
#define GINSIM_ERR_PLACED -6   /* ABI 7: ginsim_malloc_placed / _reserve: this device has no usable placed arena (no virtual-memory
                                * management, fewer than two classes of physical memory found, arena limit reached): allocate with
                                * ginsim_malloc instead */

typedef struct ginsim_ctx ginsim_ctx;   /* one context per device; re-entrant per context */

/* ---- context / plumbing -------------------------------------------------------------------- */
int         ginsim_abi_version(void);
const char* ginsim_last_error(void);
int  ginsim_device_count(int* count);
int  ginsim_create(int device, ginsim_ctx** out);
/* ABI 8: the XCD (accelerator complex die, 0 .. 7 on an MI355X) on which the FIRST workgroup of a launch on this context's stream
 * lands.  The dispatcher deals the workgroups of a launch to the XCDs in turn, starting at a die that belongs to the stream's
 * hardware queue (measured: the same for every launch of a stream, consecutive for streams made one after the other).  Two launches
 * that are to run side by side without costing each other a round of workgroups must fit TOGETHER into whole rounds on every die:
 * the drop-in Sim runs the few runs it keeps as ONE workgroup next to the statistics launch over all the others (1023 workgroups on
 * 8 x 64 slots: one die has a slot to spare) and picks the pair of contexts that puts that workgroup on that die. */
int  ginsim_stream_first_xcc(ginsim_ctx* ctx, int32_t* xcc);
int  ginsim_destroy(ginsim_ctx* ctx);
int  ginsim_device_name(ginsim_ctx* ctx, char* buf, size_t cap);
int  ginsim_mem_info(ginsim_ctx* ctx, size_t* free_bytes, size_t* total_bytes);   /* ABI 6: hipMemGetInfo of the context's device */
int  ginsim_malloc(ginsim_ctx* ctx, size_t bytes, void** dptr);
int  ginsim_free(ginsim_ctx* ctx, void* dptr);   /* regions of ginsim_malloc and of ginsim_malloc_placed alike */

/* ---- ABI 7: placed device memory -------------------------------------------------------------------------------------------
 * The 288 GB of an MI355X are three 96 GB classes of physical memory (the top level of the physical address; below it every HBM
 * stack and channel is interleaved).  A launch that streams SEVERAL output planes at once -- the 15 planes [component][sample][run]
 * the fused kernel writes where the reference keeps R x (n,3) arrays per series (ins_sim.py:490-506, ins_algo_manager.py:77-95) --
 * writes 5.7-5.9 TB/s when all of them lie in one class, 6.4-6.5 TB/s across two and 6.8-7.0 TB/s across three
 * (profiles/r06_placed_memory.json), and hipMalloc gives a process its first tens of GB from one class.  hipMalloc does not say
 * where a region lies, but the virtual-memory API lets the library build a range from physical chunks it has looked at: a
 * placed arena (one per device, shared by the contexts of a process) is a reserved virtual range whose 512 MiB stripes are
 * hipMemCreate'd chunks dealt to the range so that consecutive stripes cycle through the classes.  A chunk's class is found by
 * TIMING a fill that streams into it and into a reference chunk of each class at once (two streams in one class conflict: the pair
 * takes 1.3-1.9 x the time of a pair in different classes).  Chunks are created until every class has its share of the request
 * (or the budget is spent: then two classes, or GINSIM_ERR_PLACED), the rest is given back to the driver.  Every region carved
 * from the arena larger than a stripe spans the classes, whatever its planes' sizes; regions are handed out by a first-fit free
 * list and the arena grows by whole stripes.  ginsim_destroy returns what its context carved and never freed; the device's last
 * context gives the arena's memory back.  The reference has no counterpart (its arrays are NumPy's). */
typedef struct {
    int64_t stripe_bytes;       /* 0: 512 MiB.  A power of two >= 64 MiB (below 512 MiB a chunk no longer lies in ONE class) */
    int64_t budget_bytes;       /* 0: 200 GiB.  Most physical memory one search may hold while it looks for the classes */
    int64_t limit_bytes;        /* 0: a third of the device memory.  The arena never maps more than this */
    double  search_seconds;     /* 0: 3 s.  A search settles for the classes it has after this long; after a third of it for two
                                 * classes in balance (none gives more than three fifths of the stripes) */
} ginsim_placed_options;

typedef struct {
    int32_t available;          /* 1: the arena exists and spans at least two classes */
    int32_t classes;            /* classes of physical memory found so far (3 on MI355X) */
    int32_t searches;           /* chunk searches so far (one per growth) */
    int32_t failed;             /* 1: a search ended with fewer than two classes: placed requests now return GINSIM_ERR_PLACED */
    int64_t stripe_bytes;
    int64_t mapped_bytes;       /* stripes mapped into the arena */
    int64_t used_bytes;         /* handed out */
    int64_t limit_bytes;
    int64_t stripes_of_class[3];
    int64_t chunks_created;     /* over all searches */
    int64_t chunks_ambiguous;   /* chunks no class claimed clearly (given back) */
    int64_t probes;             /* timed fills */
    int64_t peak_held_bytes;    /* most physical memory a search held at once */
    double  search_seconds;     /* all searches together */
    double  last_search_seconds;
    double  anchor_ms;          /* time of a conflict-free pair fill of two stripes (calibrated on single streams) */
    char    stripe_classes[256];/* class letter of the first 255 stripes, in address order ("ABCBCA...") */
} ginsim_placed_info;

int  ginsim_placed_configure(ginsim_ctx* ctx, const ginsim_placed_options* options);   /* before the device's arena exists */
int  ginsim_placed_reserve(ginsim_ctx* ctx, size_t bytes);   /* grow the arena so that `bytes` more can be carved from it: ONE search
                                                               * for the regions of a job instead of one per region */
int  ginsim_malloc_placed(ginsim_ctx* ctx, size_t bytes, void** dptr);
int  ginsim_placed_release(ginsim_ctx* ctx);                  /* give the arena's memory back if nothing is carved from it */
int  ginsim_placed_info_get(ginsim_ctx* ctx, ginsim_placed_info* out);
int  ginsim_memcpy_h2d(ginsim_ctx* ctx, void* dst, const void* src, size_t bytes);
int  ginsim_memcpy_d2h(ginsim_ctx* ctx, void* dst, const void* src, size_t bytes);
int  ginsim_memset(ginsim_ctx* ctx, void* dptr, int value, size_t bytes);
/* Page-locked host memory for callers of the host-buffer entry points (ginsim_free_integration, ginsim_memcpy_*): copies from
 * and to such buffers run at the link rate instead of through the driver's staging of pageable memory.  The reference has
 * no counterpart (its arrays are plain NumPy); the Python layer wraps it as ginsim.pinned_empty(). */
int  ginsim_host_alloc(ginsim_ctx* ctx, size_t bytes, void** hptr);
int  ginsim_host_free(ginsim_ctx* ctx /* may be NULL: the pages may outlive the context */, void* hptr);
int  ginsim_sync(ginsim_ctx* ctx);
/* HIP-event timer on the context's stream (the stream every kernel of this context is launched on). */
int  ginsim_timer_begin(ginsim_ctx* ctx);
int  ginsim_timer_end(ginsim_ctx* ctx, float* elapsed_ms);
/* Event pool for timing many launches without synchronising in between: record event `slot` on the
 * context's stream; elapsed(a,b) synchronises on b and returns the time between the two records. */
#define GINSIM_MAX_EVENTS 8192
int  ginsim_event_record(ginsim_ctx* ctx, int32_t slot);
int  ginsim_event_elapsed(ginsim_ctx* ctx, int32_t slot_a, int32_t slot_b, float* elapsed_ms);

/* ---- truth: pathgen.path_gen (gnss_ins_sim/pathgen/pathgen.py:26-329, osr == 1) ------------- */
typedef struct {
    double  ini_pva[9];     /* lat, lon [rad], alt [m], body vel [m/s], yaw pitch roll [rad]  (ins_sim.py:597-610) */
    double  mobility[3];    /* max accel, max angular accel [rad/s^2], max angular rate [rad/s] (ins_sim.py:25) */
    double  fs;             /* IMU / simulation rate [Hz] */
    double  fs_gps;         /* GPS rate [Hz] (used when enable_gps) */
    int32_t ref_frame;      /* 0 NED/LLA, 1 virtual inertial frame */
    int32_t enable_gps;
    int32_t n_seg;          /* rows of motion_def */
    int32_t enable_mag;     /* emit the true magnetic field in the body frame (pathgen.py:273-279) */
    double  geo_mag_n[3];   /* geomagnetic field at the initial position in the N frame [uT] (pathgen.py:164-168; the WMM
                             * evaluation itself is outside the hot path).  ref_frame 1 drops the declination (:169-171). */
} ginsim_pathgen_params;

/* Upper bound of the IMU sample count: sum of ceil(duration*fs) (pathgen.py:116-127). */
int ginsim_pathgen_capacity(const ginsim_pathgen_params* p, const double* motion_def /*[n_seg][9]*/, int64_t* cap);
/* Host buffers, row-major: imu [cap][7] = idx,acc3,gyro3; nav [cap][10] = idx,pos3,velNED3,euler3;
 * gps [cap][8] = idx,pos3,vel3,visibility (may be NULL); odo [cap][5] = idx,dist,vel_b3 (may be NULL).
 * motion_def is not modified (the reference overwrites column 7, pathgen.py:122). */
int ginsim_pathgen(const ginsim_pathgen_params* p, const double* motion_def, int64_t cap,
                   double* imu, double* nav, double* gps, double* odo, double* mag /*[cap][4] = idx,mag3 or NULL*/,
                   int64_t* n_out, int64_t* m_out);

/* ---- ABI 6: the leaves of the path under their own entry points (host code, for hosted plugins and tools that call the
 * reference functions of the same names one state at a time; ginsim_pathgen and the kernels run the same code inline) ---- */
/* pathgen.calc_true_sensor_output (pathgen.py:331-411): c_nb [3][3] row-major (body -> nav, as the reference passes it); g is
 * used in ref_frame 1 only.  Outputs: acc, gyro (body frame), vel_dot_n, pos_dot_n (lat/lon/alt rates in ref_frame 0). */
int ginsim_calc_true_sensor_output(const double* pos_n, const double* vel_b, const double* att, const double* c_nb,
                                   const double* vel_dot_b, const double* att_dot, int32_t ref_frame, double g,
                                   double* acc, double* gyro, double* vel_dot_n, double* pos_dot_n);
/* pathgen.parse_motion_def (pathgen.py:413-439): seg[0] = command type 1..5, seg[1..3] attitude, seg[4..6] velocity command. */
int ginsim_parse_motion_def(const double* seg, const double* att, const double* vel, double* att_com, double* vel_com);
/* attitude.euler_update_zyx (attitude.py:679-721): x = [yaw, pitch, roll], w body rate, one step of dt. */
int ginsim_euler_update_zyx(const double* x, const double* w, double dt, double* y);

/* ---- Monte-Carlo fused kernel: noise injection + mechanisation + end-point error ------------- */
#define GINSIM_ALGO_FREE 1   /* demo_algorithms/free_integration.py:63-174      */
#define GINSIM_ALGO_ODO  2   /* demo_algorithms/free_integration_odo.py:63-160  */

typedef struct {            /* one 3-axis sensor: pathgen.acc_gen / gyro_gen / bias_drift (pathgen.py:441-594) */
    double  bias[3];        /* err['b'] */
    double  gm_a[3];        /* 1 - 1/(fs*tau)                        (pathgen.py:583); 0 when tau is inf */
    double  gm_b[3];        /* drift*sqrt(1-exp(-2/(fs*tau)))        (pathgen.py:586); drift when tau is inf */
    double  white[3];       /* rw / sqrt(dt)                         (pathgen.py:496, 558) */
    int32_t white_drift[3]; /* 1: tau is inf -> drift[j] = gm_b*N[j] (pathgen.py:593) */
    int32_t reserved;
} ginsim_sensor_model;

/* ABI 5.  The vibration term of one 3-axis sensor (pathgen.py:476-492 accel, :538-556 gyro; Sim.__parse_env, ins_sim.py:642-701,
 * turns the env strings into these numbers).  meas = truth + bias + drift + white + VIB, added last as the reference does:
 *   type 1 'random'      vib[j][k] = amp[k] N[j][k]                     (:485-488, :547-550; three more normals per sample)
 *   type 2 'sinusoidal'  vib[j][k] = amp[k] sin(omega_dt j + phase[k])  omega_dt = 2 pi freq dt; phase = 0 for the accelerometer
 *                        (:489-492), one uniform draw per run and axis times 2 pi for the gyroscope (:551-555)
 *   type 3 'psd' (ABI 8) vib[j][k] = series[k][j mod period][run]       (:479-484, :541-546: time_series_from_psd.py:16-63, a
 *                        random-phase inverse FFT of `period` <= 16384 points per run and axis, tiled to n); the series are made
 *                        on the device by ginsim_vib_psd_series BEFORE the launch and read by it
 * Vibration launches run on the general-sensor-model lane-per-run kernels (ginsim_mc_variant 0; fp64 and fp32 -- the fp32 term
 * is defined operation by operation, csrc/mc_kernel_f32.hip add_vibration) or, sensors only for few runs, on the time-parallel
 * series kernels (variant 2); given sensors refuse it.  Type 3 runs on the fp64 lane-per-run kernels only. */
#define GINSIM_VIB_NONE       0
#define GINSIM_VIB_RANDOM     1
#define GINSIM_VIB_SINUSOIDAL 2
#define GINSIM_VIB_PSD        3
typedef struct {
    int32_t type;           /* GINSIM_VIB_* */
    int32_t random_phase;   /* sinusoidal: 1 = a uniform phase per run and axis (gyro_gen), 0 = phase 0 (acc_gen) */
    double  amp[3];         /* vib_def['x'/'y'/'z']: 1 sigma (random) or peak (sinusoidal), m/s^2 or rad/s */
    double  omega_dt;       /* sinusoidal: ((2.0 * pi) * freq) * dt, rounded as the reference's left-to-right product */
    /* ---- ABI 8: type 3 ---- */
    const double* series;   /* device [3][period][runs], run fastest: what ginsim_vib_psd_series wrote for THESE runs */
    int64_t period;         /* N of time_series_from_psd.py:36-43: n (n + 1 when n is odd), at most 16384 */
} ginsim_vibration;

/* ABI 8.  The vibration series of one 3-axis sensor from a single-sided power spectral density, for `runs` Monte-Carlo runs at once
 * (pathgen.py:479-484 / :541-546 call time_series_from_psd.time_series_from_psd(sxx, freq, fs, n) per run and axis):
 *   x = real(ifft(X)),  X[k] = a[k] exp(i pi z[k]) for k = 0 .. period/2,  Hermitian above  (time_series_from_psd.py:51-57)
 * amp (HOST, [3][period / 2 + 1]) = a = sqrt(sxx' period fs), sxx' the PSD interpolated to the period's frequency grid with its
 * interior bins halved (:44-50) -- leaf arithmetic of O(period), left to the caller (ginsim.psd_amplitudes in the Python layer).
 * z[k] (time_series_from_psd.py:52, np.random.randn(L)) are the normals the 'random' vibration of the same sensor would draw at
 * SAMPLE k (streams 10 / 11 accel, 12 / 13 gyro of run run_offset + r): x, y, z of bin k.  One batched complex-to-real FFT
 * (hipFFT, loaded at run time) per block of runs, then a transposition into out (DEVICE, [3][period][runs], run fastest), scaled
 * by 1 / period.  sensor: 0 accelerometer, 1 gyroscope.
 * halve_per_run = 1 reproduces what the reference does when the PSD is GIVEN on the period's own grid (freq.shape[0] ==
 * period / 2 + 1): it then halves the caller's array in place at every call (:49 without the copy np.interp makes), so run r of a
 * Sim.run() sees interior bins scaled by 0.5^(r + 1); amp is then a of the array as given (nothing halved). */
int ginsim_vib_psd_series(ginsim_ctx* ctx, const double* amp, int64_t period, int64_t runs, uint64_t run_offset, uint64_t seed,
                          int32_t sensor, int32_t halve_per_run, double* out);

typedef struct {
    int64_t  n;             /* IMU samples per run */
    int64_t  runs;          /* Monte-Carlo runs on this device */
    uint64_t run_offset;    /* global id of this device's first run (enters the RNG counter) */
    uint64_t seed;          /* Philox key */
    double   fs;
    int32_t  ref_frame;     /* 0 NED/LLA (free_integration.py:117-172), 1 virtual inertial (:83-116) */
    int32_t  algo_mask;     /* GINSIM_ALGO_* bits; both algorithms see the same sensor realisation; 0 = sensors only */
    int32_t  earth_rot;     /* FreeIntegration(earth_rot=...) (free_integration.py:19, 150-152) */
    int32_t  n_ini;         /* columns of the initial-state table (free_integration.py:42-61) */
    uint64_t ini_first;     /* value of FreeIntegration.run_times before this batch (free_integration.py:69, 85-87) */
    int32_t  ini_has_g;     /* 10th element = externally supplied gravity (free_integration.py:59-61) */
    int32_t  given_sensors; /* 1: read gyro/accel[/odo] from in_* instead of generating them */
    ginsim_sensor_model accel, gyro;
    double   odo_scale, odo_stdv;          /* pathgen.odo_gen (pathgen.py:627-641) */
    double   ref_end[9];    /* truth att(3) pos(3) vel(3) at the last sample, for the end-point error */
    /* device pointers */
    const double* ini;        /* [n_ini][10] */
    const double* ref_accel;  /* [n][3] truth specific force (pathgen imu cols 1-3) */
    const double* ref_gyro;   /* [n][3] truth angular rate   (pathgen imu cols 4-6) */
    const double* ref_odo;    /* [n]    truth forward speed  (pathgen odo col 2), NULL if unused */
    const double* in_accel;   /* given_sensors: [3][n][runs] */
    const double* in_gyro;    /* given_sensors: [3][n][runs] */
    const double* in_odo;     /* given_sensors: [n][runs], NULL if unused */
    double* out_accel;        /* [3][n][runs] or NULL  (dmgr.accel, ins_sim.py:491-493) */
    double* out_gyro;         /* [3][n][runs] or NULL  (dmgr.gyro,  ins_sim.py:494-496) */
    double* out_odo;          /* [n][runs]    or NULL  (dmgr.odo,   ins_sim.py:504-506) */
    double* out_traj[2];      /* per algorithm bit: [9][n][runs] = att3,pos3,vel3 or NULL */
    double* out_end[2];       /* per algorithm bit: [9][runs] end-point error (att wrapped to [-pi,pi]) or NULL */
    /* tuning / telemetry (0 / NULL = defaults) */
    uint64_t* wave_trace;     /* device [n_waves][4] or NULL: HW_ID, XCC_ID, s_memtime at wave start and end */
    int32_t   block_threads;  /* workgroup size: 0 (default), 64, 128 or 256 */
    int32_t   end_pos_ned;    /* ref_frame 0: report the end-point position error in local NED metres (extra_opt='ned',
                               * ins_data_manager.py:474-488, 542-552) instead of [rad, rad, m] */
    int32_t   precision;      /* 0: fp64 (default).  1: fp32 kernel -- out_accel/out_gyro/out_odo/out_traj point to FLOAT
                               * buffers of the same [component][sample][run] shape; the position planes of out_traj hold
                               * the displacement from the run's initial position (ECEF-based for ref_frame 1, LLA for 0);
                               * out_end stays double; in_* (given_sensors) stay double and are rounded to float as read.
                               * The fp32 kernel consumes the SAME normals as the fp64 one (they are single-precision numbers)
                               * and every operation of it is one defined IEEE operation: oracle/c/ginsim_oracle.c
                               * (oracle_mc_run_f32) reproduces its series to the bit. */
    int32_t   proc_pos_ned;   /* process statistics of the position error in local NED metres (ref_frame 0 only) */
    /* ---- statistics WITHOUT trajectories (ABI 2): what Sim.results() needs when the series are not materialised ---- */
    const double* ref_nav;    /* [n][9] truth att3, pos3, vel3 of every sample; needed when out_proc is set */
    int64_t   proc_first;     /* first sample of the process-error window (err_stats_start, ins_data_manager.py:771-781) */
    double*   out_proc[2];    /* per algorithm bit: [3][9][runs] = max|e|, mean, std(ddof=0) of the error over samples
                               * >= proc_first, accumulated online in the fused kernel (InsDataMgr.__process_error_stats,
                               * ins_data_manager.py:761-795, on array_error :519-553), or NULL.  ONE algorithm bit per launch,
                               * generate mode, fp64. */
    double*   out_end_ned[2]; /* per algorithm bit: [9][runs] end-point error with the position error in local NED metres
                               * (extra_opt='ned', ins_data_manager.py:542-552) next to out_end, or NULL (ref_frame 0 only) */
    /* ---- ABI 4 ---- */
    int32_t   sensor_layout;  /* layout of out_accel / out_gyro / out_odo.  0 (default): [axis][sample][run], run fastest -- what
                               * the lane-per-run kernels write.  1: SERIES-major [run][axis][sample] ([run][sample] for the
                               * odometer) -- every series contiguous, the input layout of ginsim_allan (series_stride = n) and of
                               * the reference's own per-run arrays dmgr.accel.data[i] (ins_sim.py:491-496).  Only sensors-only
                               * launches (algo_mask 0) take it; with <= 1024 runs and >= 2048 samples they run on the
                               * time-parallel series kernels (ginsim_mc_variant reports 2), otherwise layout 1 is refused.
                               * PERFORMANCE CLIFF: with layout 0 and 2..1024 runs a sensors-only launch takes the lane-per-run
                               * kernel, whose time loop is ONE sequential chain over n per lane -- for long series (config 5:
                               * 1 440 000 samples) seconds instead of a millisecond.  A caller that wants few long series
                               * sets sensor_layout = 1 (or asks ginsim_mc_variant first: 2 = time-parallel). */
    int32_t   proc_plain_sums; /* online process statistics, the variants whose sums are shifted per LAUNCH (ref_frame 0 free integration; see
                               * csrc/mc_kernel.hip, Proc): 0 (default) = the sums are kept about the error of the first run's initial
                               * state against the truth at sample 0, so an error that is nearly constant over the window keeps its true
                               * std (np.std, ins_data_manager.py:761-795).  1 = the caller states that every run starts ON the truth
                               * (that error is zero): the sums are taken as they are -- what nine zero shifts give, nine
                               * double-precision subtractions per step fewer (BASELINE config 3: 2.3 %).  Stating it of runs that
                               * start off the truth brings back the rounding floor of ~1.5e-8 |mean| on the std.  (Was reserved4,
                               * which had to be 0.) */
    /* ---- ABI 5: vibration, Sim(env={'acc': ..., 'gyro': ...}) -> the vib term of pathgen.acc_gen / gyro_gen ---- */
    ginsim_vibration vib_accel, vib_gyro;
} ginsim_mc_params;

int ginsim_mc_run(ginsim_ctx* ctx, const ginsim_mc_params* p);

/* Which kernel ginsim_mc_run would launch for these parameters (telemetry for profiles; results are bit-identical between
 * 0 and 1): 0 = one wavefront per 64 runs does noise + mechanisation (mc_kernel / mc_kernel_f32), 1 = wave-specialised
 * producer/consumer workgroups (mc_kernel_split / mc_kernel_f32_split), chosen for batches of <= 1024 wavefronts and,
 * for one algorithm in ref_frame 1 (two producer groups: three wavefronts per SIMD), at every size; 2 (ABI 4) = the
 * time-parallel series kernels (sensors only, <= 1024 runs, >= 2048 samples, sensor_layout 1 or one run): a lane is a
 * SAMPLE, the Gauss-Markov recurrence a weighted scan -- same normals, sums associated differently (an ulp of the terms). */
int ginsim_mc_variant(const ginsim_mc_params* p, int32_t* variant);
/* ABI 3: the NAME of that kernel as rocprofv3 reports it, without arguments (e.g. "ginsim::mc_kernel_split<1, 1, false, 2,
 * true>"), written by the same dispatch code that launches it -- profiles and bench.py attribute to what really runs. */
int ginsim_mc_kernel_name(const ginsim_mc_params* p, char* buf, size_t cap);

/* ---- inclinometers: demo_algorithms/inclinometer_mahony.py::MahonyFilter (:50-151) and inclinometer_acc.py::TiltAcc (:37-56)
 *      over a batch of Monte-Carlo runs, one lane per run (csrc/inclinometer.hip).  Added without a change of
 *      GINSIM_ABI_VERSION: nothing existing moved.
 *      The sensors come from the ginsim_mc_params given next to these parameters, read exactly as ginsim_mc_run reads them:
 *      n, runs, run_offset, seed, accel, gyro, ref_accel, ref_gyro, vib_accel, vib_gyro (types 1 and 2; 'psd' is refused) in
 *      generate mode -- run r then sees bit for bit the accelerometer and gyroscope samples of run r of a ginsim_mc_run with the
 *      same seed --, or given_sensors with in_accel / in_gyro ([3][n][runs]).  ref_nav ([n][9], attitude in columns 0-2) and
 *      proc_first serve the statistics; block_threads the workgroup size (0 = 256).  Every other field is ignored.
 *      The Mahony filter of a run starts from bias_in (its gyro_bias) with q = (1, 0, 0, 0), err_int = 0 and ini = 0, as the
 *      reference's MahonyFilter after reset() does when the previous run's final state is that bias; q and err_int are rebuilt at
 *      the first sample with a non-zero accelerometer.  Chaining runs (run r starts from run r-1's final bias) is the caller's. */
#define GINSIM_INCL_MAHONY 1
#define GINSIM_INCL_TILT   2
typedef struct {
    int32_t  algo_mask;       /* GINSIM_INCL_* bits; both filters see the same sensor realisation */
    int32_t  reserved;        /* 0 */
    double   dt;              /* MahonyFilter.dt (1 / fs of the plugin's input) */
    double   kp_high, kp_low, ki_high, ki_low, innovation_limit;   /* MahonyFilter.kp_acc_high ... innovationLimit */
    const int64_t* run_list;  /* device [n_list] or NULL: lane i integrates run run_list[i] (ids < runs); NULL: runs 0 .. n_list-1 */
    int64_t  n_list;          /* lanes of the launch */
    const double* bias_in;    /* device [3][runs]: the Mahony filter's gyro_bias at the start of each run (needed with MAHONY) */
    double*  bias_out;        /* device [3][runs] or NULL: its gyro_bias at the end of each launched run */
    double*  out_quat[2];     /* per algorithm bit (0 Mahony, 1 tilt): [4][n][runs] att_quat, or NULL */
    double*  out_euler[2];    /* per algorithm bit: [3][n][runs] att_euler = quat2euler zyx of att_quat, or NULL */
    double*  out_wb;          /* Mahony: [3][n][runs] gyro_bias after each sample ('wb'), or NULL */
    double*  out_ab;          /* Mahony: [3][n][runs] the limited innovation acc_err ('ab'), or NULL */
    double*  out_end[2];      /* per algorithm bit: [3][runs] att_euler error at the last sample, wrapped to [-pi, pi], or NULL */
    double*  out_proc[2];     /* per algorithm bit: [3][3][runs] max|e|, mean, std (ddof 0) of the att_euler error over samples
                               * >= proc_first, or NULL */
} ginsim_incl_params;

int ginsim_incl_run(ginsim_ctx* ctx, const ginsim_mc_params* mc, const ginsim_incl_params* p);
/* 0: generated sensors, 1: given sensors */
int ginsim_incl_variant(const ginsim_mc_params* mc, const ginsim_incl_params* p, int32_t* variant);
/* the NAME of the kernel ginsim_incl_run launches, as rocprofv3 reports it (e.g. "ginsim::incl_kernel<3, false, false>") */
int ginsim_incl_kernel_name(const ginsim_mc_params* mc, const ginsim_incl_params* p, char* buf, size_t cap);

/* ---- loosely coupled GPS/INS Kalman filter: the interface demo_algorithms/ins_loose.py::InsLoose declares (input fs, gyro,
 *      accel, time, gps_time, gps; output pos, vel, att_euler, wb, ab; its prediction and correction are `pass`) filled in as a
 *      15-state closed-loop error-state filter over a batch of Monte-Carlo runs, one lane per run (csrc/ins_loose.hip).  Added
 *      without a change of GINSIM_ABI_VERSION: nothing existing moved.
 *      The IMU samples come from the ginsim_mc_params given next to these parameters, read exactly as ginsim_incl_run reads them
 *      (generate mode with vibration types 1 and 2, 'psd' refused; or given_sensors with in_accel / in_gyro); the initial states
 *      (ini, n_ini, ini_first, ini_has_g), ref_frame, earth_rot, fs, ref_end, end_pos_ned, ref_nav, proc_first and block_threads
 *      as ginsim_mc_run reads them.  The mechanisation is ginsim_mc_run's free integration on accel - ab and gyro - wb: a
 *      launch without a usable fix IS free integration.
 *      GPS fix k of run r is regenerated in the lane (ref_gps given: what ginsim_aux_sensors writes for the same seed, run_offset
 *      and gps_sigma, bit for bit, never stored) or read from in_gps (given_sensors).  It is applied at IMU sample gps_stamp[k]
 *      to the state that sample's row reports, before the row is stored, when gps_visible[k] != 0.
 *      Error state x = estimate - truth: dr (NED metres in ref_frame 0, the virtual-inertial axes in ref_frame 1), dv, psi (a
 *      small rotation in the navigation frame: C_est = (I - [psi x]) C, C = body -> navigation), dbg, dba.  Per IMU sample
 *      P <- Phi P Phi^T + Qd with Phi = I + F dt; the blocks of F are (r,v) = I, (v,psi) = [f^n x], (v,ba) = -C, (psi,bg) = C,
 *      (bg,bg) = -1/tau_g, (ba,ba) = -1/tau_a (Earth and transport rate neglected in F only).  A fix is six sequential scalar
 *      updates with z = ins - gps, H = [I6 0]; the state is fed back at once and zeroed. */
typedef struct {
    int64_t  m;               /* GPS fixes (0: none) */
    const int64_t* gps_stamp; /* HOST [m]: the IMU sample index of each fix (gps_time fs), strictly increasing, in [0, n) */
    const int32_t* gps_visible; /* HOST [m]: gps_visibility; a fix with 0 is skipped.  NULL: all visible */
    const double* ref_gps;    /* device [m][6]: generated form (truth pos3, vel3 of every fix), or NULL */
    double   gps_sigma[6];    /* generated form: as ginsim_aux_params.gps_sigma (position sigma in rad, rad, m for ref_frame 0) */
    const double* in_gps;     /* device [6][m][runs]: given form (with given_sensors) */
    double   r_diag[6];       /* measurement variances: position (m^2, NED metres in ref_frame 0) and velocity */
    double   p0[5];           /* initial 1 sigma of dr, dv, psi, dbg, dba (P0 is diagonal); all > 0 */
    double   q_v[3], q_psi[3];/* Qd of one IMU sample on dv and psi per BODY axis (rotated by C in the kernel): (vrw^2 | arw^2) dt */
    double   q_bg[3], q_ba[3];/* Qd of one IMU sample on the bias states: 2 sigma^2 / tau dt (0: a constant) */
    double   decay_g[3], decay_a[3]; /* 1 - dt / tau of the bias states (1: a random walk) */
    const int64_t* run_list;  /* device [n_list] or NULL: lane i filters run run_list[i] (ids < runs); NULL: runs 0 .. n_list-1 */
    int64_t  n_list;          /* lanes of the launch */
    double*  out_traj;        /* [9][n][runs] = att3, pos3, vel3 (the layout ginsim_process_stats / ginsim_error_curve read), or NULL */
    double*  out_wb;          /* [3][n][runs] estimated gyro bias at every sample, or NULL */
    double*  out_ab;          /* [3][n][runs] estimated accelerometer bias at every sample, or NULL */
    double*  out_end;         /* [9][runs] end-point error as ginsim_mc_params.out_end (attitude wrapped, end_pos_ned honoured), or NULL */
    double*  out_proc;        /* [3][9][runs] max|e|, mean, std (ddof 0) of the error over samples >= proc_first (needs ref_nav), or NULL */
    double*  out_bias_end;    /* [6][runs] wb3, ab3 at the last sample, or NULL */
    double*  out_pdiag_end;   /* [15][runs] diagonal of P at the last sample, or NULL */
    double*  out_end_ned;     /* [9][runs] a second end-point record with the position error in local NED metres, as
                               * ginsim_mc_params.out_end_ned (ref_frame 0 only), or NULL */
    /* Odometer and non-holonomic aiding (csrc/ins_loose_aided.hip), appended without a change of
     * GINSIM_ABI_VERSION: a zeroed tail is the filter as it was.  With D = C_est^T (navigation -> body) of the reported attitude, v
     * the reported navigation-frame velocity and v_b = D v, bit i of aid_mask selects the scalar measurement
     *   i = 0       z = v_b[0] - odo_j / odo_scale_f, variance r_odo      (the odometer)
     *   i = 1, 2    z = v_b[i] - 0,                   variance r_nhc      (no sideways, no vertical body velocity)
     * with the row h_i = [0, D[i,:], -(D [v x])[i,:], 0, 0].  One block runs the selected rows in ascending order from x = 0
     * (D, v and the rows from the state before the first one) and ends with the feedback of a GPS fix.  It runs at every IMU
     * sample j > 0 with j % aid_every == 0 on the state that sample's row reports, after a fix of the same sample, before the row
     * is stored.  odo_j is what ginsim_mc_run writes to out_odo for the same seed and run (the mc block's ref_odo, odo_scale,
     * odo_stdv; never stored), or in_odo[j runs + r] with given_sensors.  aid_mask != 0 launches loose_aided_kernel. */
    int32_t  aid_mask;        /* 0 .. 7; 0: no aiding (aid_every, odo_scale_f, r_odo, r_nhc are not read) */
    int64_t  aid_every;       /* >= 1: a block every aid_every IMU samples (n or more: never) */
    double   odo_scale_f;     /* the odometer scale factor the FILTER assumes (bit 0); finite, > 0 */
    double   r_odo;           /* variance of the scaled odometer sample, (m/s)^2 (bit 0); finite, > 0 */
    double   r_nhc;           /* variance of the two constraint rows, (m/s)^2 (bits 1, 2); finite, > 0 */
} ginsim_loose_params;

int ginsim_loose_run(ginsim_ctx* ctx, const ginsim_mc_params* mc, const ginsim_loose_params* p);
/* 0: generated sensors and fixes, 1: given */
int ginsim_loose_variant(const ginsim_mc_params* mc, const ginsim_loose_params* p, int32_t* variant);
/* the NAME of the kernel ginsim_loose_run launches, as rocprofv3 reports it (e.g. "ginsim::loose_kernel<1, false, false, false>") */
int ginsim_loose_kernel_name(const ginsim_mc_params* mc, const ginsim_loose_params* p, char* buf, size_t cap);

/* ---- consistency checkpoints of the filter (csrc/ins_loose_cons.hip): its predicted covariance and its actual
 *      error, reduced ACROSS the runs of a launch at chosen samples, inside the launch, where P lives.  Added without a change of
 *      GINSIM_ABI_VERSION and as a block of its own: ginsim_loose_params and ginsim_loose_run are exactly what they were.
 *      At IMU sample cons_sample[c], on the state that sample's row reports (after a fix and an aiding block of the same sample,
 *      before the row is stored), every lane forms the error state e = estimate - truth in the filter's own coordinates against
 *      row cons_sample[c] of the mc block's ref_nav (dr: NED metres through the truth's Rm + h and (Rn + h) cos(lat) in
 *      ref_frame 0, the plain difference in ref_frame 1; dv; psi: the antisymmetric part of I - C_est C^T), and the launch sums
 *      over its runs into out_cons[c][GINSIM_CONS_RECORD]:
 *        [0]       the number of runs included
 *        [1..15]   P_kk of the 15 states
 *        [16..24]  e_k^2 of the 9 navigation states (dr, dv, psi)
 *        [25..33]  e_k^2 / P_kk of the same
 *        [34..36]  e_b^T P_bb^-1 e_b of the position, velocity and attitude block (3 each for a consistent filter)
 *        [37..42]  reserved, written as 0
 *      A run with a non-finite value among these, a P_kk <= 0 or a 3x3 block that is not positive definite is left out of every
 *      sum and of the count.  The sums are taken in a fixed order (the lanes of a wavefront by a butterfly, the wavefronts
 *      ascending, no atomics): the record is a function of the inputs and the run list, bit for bit from launch to launch. */
#define GINSIM_CONS_RECORD 43
typedef struct {
    const int64_t* cons_sample; /* HOST [cons_m]: IMU sample indices, strictly increasing, in [0, n) */
    int64_t  cons_m;          /* checkpoints; 0: none -- the call is ginsim_loose_run (the pointers are not read) */
    double*  out_cons;        /* device [cons_m][GINSIM_CONS_RECORD] */
    double*  cons_work;       /* device [(n_list + 63) / 64][cons_m][GINSIM_CONS_RECORD]: the wavefronts' partial sums */
} ginsim_loose_cons_params;

/* ginsim_loose_run with checkpoints: launches loose_cons_kernel, then the kernel that adds the wavefronts' partial sums.  Refused:
 * cons_m < 0; cons_m > 0 with cons_sample, out_cons, cons_work or the mc block's ref_nav NULL, with samples outside [0, n) or
 * not strictly increasing, or together with p->out_proc (online process statistics and checkpoints in one launch). */
int ginsim_loose_cons_run(ginsim_ctx* ctx, const ginsim_mc_params* mc, const ginsim_loose_params* p, const ginsim_loose_cons_params* cons);
/* the NAME of the kernel it launches (e.g. "ginsim::loose_cons_kernel<1, false, false, false>" = RF, GIVEN, VIB, AID) */
int ginsim_loose_cons_kernel_name(const ginsim_mc_params* mc, const ginsim_loose_params* p, const ginsim_loose_cons_params* cons,
                                  char* buf, size_t cap);

/* ---- magnetometer aiding of the filter (csrc/ins_loose_mag.hip): a three-row heading block on psi.  Added without
 *      a change of GINSIM_ABI_VERSION and as a block of its own: ginsim_loose_params and ginsim_loose_run are exactly what they were.
 *      With D = C_est^T (navigation -> body) of the reported attitude, m_n = mag_n and the calibrated sample
 *      m_cal = cal_si . mag_j - cal_hi, to first order D_est m_n = m_b - D [m_n x] psi, so body axis i = 0, 1, 2 gives
 *        z_i = D[i,:] . m_n - m_cal[i],   h_i = [0, 0, m_n x D[i,:], 0, 0],   variance r_mag[i].
 *      One block runs the three rows in ascending order from x = 0 (D, z and the rows from the state before the first one) and
 *      ends with the feedback of a GPS fix.  It runs at every IMU sample j > 0 with j % mag_every == 0 on the state that sample's
 *      row reports: after a fix and after an odometer / non-holonomic block of the same sample, before the row is stored.
 *      mag_j is what ginsim_aux_sensors writes to out_mag for the same seed and run (ref_mag, mag_si, mag_hi, mag_std; never
 *      stored), or in_mag[(c n + j) runs + r] with given_sensors.  aid_mask of the loose block may be 0 or not. */
typedef struct {
    int64_t  mag_every;      /* 0: none -- the call is ginsim_loose_run (nothing else is read); >= 1: a block every mag_every samples (n or more: never) */
    const double* ref_mag;   /* device [n][3]: generated form */
    double   mag_si[9], mag_hi[3], mag_std[3];   /* generation, as ginsim_aux_params */
    const double* in_mag;    /* device [3][n][runs]: given form (with given_sensors) */
    double   mag_n[3];       /* the field the FILTER assumes in the navigation frame, uT */
    double   cal_si[9];      /* row major: m_cal = cal_si . mag - cal_hi */
    double   cal_hi[3];
    double   r_mag[3];       /* variances of the calibrated sample per body axis, uT^2; finite, > 0 */
} ginsim_loose_mag_params;

/* ginsim_loose_run with the magnetometer block: launches loose_mag_kernel.  Everything ginsim_loose_run refuses is refused, and:
 * mag_every < 0; with mag_every > 0 a missing ref_mag (generated form) or in_mag (given form), a non-finite mag_si, mag_hi,
 * mag_std, mag_n, cal_si or cal_hi, an r_mag that is not positive and finite, |mag_n| = 0. */
int ginsim_loose_mag_run(ginsim_ctx* ctx, const ginsim_mc_params* mc, const ginsim_loose_params* p, const ginsim_loose_mag_params* mag);
/* the NAME of the kernel it launches (e.g. "ginsim::loose_mag_kernel<1, false, false, false>" = RF, GIVEN, VIB, PS) */
int ginsim_loose_mag_kernel_name(const ginsim_mc_params* mc, const ginsim_loose_params* p, const ginsim_loose_mag_params* mag,
                                 char* buf, size_t cap);

/* ---- the odometer's scale factor as a 16th state of the filter (csrc/ins_loose_scale.hip).  Added without a
 *      change of GINSIM_ABI_VERSION and as a block of its own: ginsim_loose_params and ginsim_loose_run are exactly what they were.
 *      State 15 is dk = k_est - k, k the true scale of odo_j = k v_b[0] + stdv z.  k_est starts at scale0 with
 *      P[15][15] = p0_scale^2 and no correlation; Phi is the identity on it and P[15][15] += q_k per IMU sample.  The odometer
 *      row becomes z0 = v_b[0] - odo_j / k_est with the seventh entry h[15] = v_b[0] / k_est (v_b of the state before the first
 *      row) and the variance r_odo as it is; the constraint rows and the GPS rows have no entry on state 15.  Every block that ran a
 *      row (a fix, an aiding block) ends with k_est -= x[15] next to the feedback of the other states.  odo_scale_f is checked as
 *      ginsim_loose_run checks it and not read. */
typedef struct {
    double   scale0;          /* k_est at sample 0; finite, > 0 */
    double   p0_scale;        /* initial 1 sigma of dk; finite, >= 0 (0 with q_k = 0: k_est stays scale0, the 15-state filter) */
    double   q_k;             /* added to P[15][15] per IMU sample (odo_scale_q^2 dt); finite, >= 0 */
    double*  out_scale;       /* [n][runs] k_est of every stored row, or NULL */
    double*  out_scale_end;   /* [2][runs] k_est and P[15][15] at the last sample, or NULL */
    double*  out_pcross_end;  /* [15][runs] P[k][15], k = 0 .. 14, at the last sample, or NULL */
} ginsim_loose_scale_params;

/* ginsim_loose_run with the scale-factor state: launches loose_scale_kernel.  Everything ginsim_loose_run refuses is refused (fp32
 * among it), and: an aid_mask without bit 0 (a scale state without the odometer), scale0 that is not positive and finite,
 * p0_scale or q_k negative or not finite.  out_pdiag_end stays [15][runs]: the 16th diagonal entry is out_scale_end[1]. */
int ginsim_loose_scale_run(ginsim_ctx* ctx, const ginsim_mc_params* mc, const ginsim_loose_params* p, const ginsim_loose_scale_params* scale);
/* the NAME of the kernel it launches (e.g. "ginsim::loose_scale_kernel<1, false, false, false>" = RF, GIVEN, VIB, PS) */
int ginsim_loose_scale_kernel_name(const ginsim_mc_params* mc, const ginsim_loose_params* p, const ginsim_loose_scale_params* scale,
                                   char* buf, size_t cap);

/* ---- standstill aiding of the filter (csrc/ins_loose_still.hip): what the filter may assume while the vehicle
 *      stands still.  Added without a change of GINSIM_ABI_VERSION and as a block of its own: ginsim_loose_params and
 *      ginsim_loose_run are exactly what they were.  With x = estimate - truth every row observes one state, H = e_I:
 *        bit 0, the zero-velocity update, I = 3, 4, 5:     z_i = vel_i (the mechanised velocity, the coordinates of dv), R = r_zupt
 *        bit 1, the zero-angular-rate update, I = 9, 10, 11: z_i = bg_est_i + w_rest_i - gyro_i, R = r_zaru[i]; gyro is the RAW
 *               sample j - 1 (the last one the lane integrated), w_rest the rate the mechanisation assumes of a body at rest:
 *               C_est^T (W cos lat, 0, -W sin lat) in ref_frame 0 with earth_rot, zero otherwise.  The dependence of w_rest on
 *               psi (about 7e-5 psi) is neglected in H, as earth rate is neglected in F.
 *      One block runs the selected rows in ascending state order from x = 0 (every z from the state before the first row) and
 *      ends with the feedback of a GPS fix.  It runs at every IMU sample j > 0 with j % still_every == 0 and still_flags[j] != 0
 *      on the state that sample's row reports: after a fix and after an odometer / non-holonomic block of the same sample, before
 *      the row is stored.  aid_mask of the loose block may be 0 or not. */
typedef struct {
    int32_t  still_mask;     /* 0: none -- the call is ginsim_loose_run (nothing else is read); bit 0 ZUPT, bit 1 ZARU */
    int32_t  reserved;
    int64_t  still_every;    /* >= 1: a block is possible every still_every samples (n or more: never) */
    const int32_t* still_flags;  /* device [n]: the standstill signal per IMU sample, the same for every run */
    double   r_zupt;         /* (m/s)^2; finite, > 0 with bit 0 */
    double   r_zaru[3];      /* (rad/s)^2 per body axis; finite, > 0 with bit 1 */
} ginsim_loose_still_params;

/* ginsim_loose_run with the standstill block: launches loose_still_kernel.  Everything ginsim_loose_run refuses is refused (fp32
 * among it), and: a still_mask outside 0 .. 3; with still_mask != 0 still_every < 1, an r_zupt / r_zaru that is not positive and
 * finite where its bit is set, still_flags NULL. */
int ginsim_loose_still_run(ginsim_ctx* ctx, const ginsim_mc_params* mc, const ginsim_loose_params* p, const ginsim_loose_still_params* still);
/* the NAME of the kernel it launches (e.g. "ginsim::loose_still_kernel<1, false, false, false>" = RF, GIVEN, VIB, PS) */
int ginsim_loose_still_kernel_name(const ginsim_mc_params* mc, const ginsim_loose_params* p, const ginsim_loose_still_params* still,
                                   char* buf, size_t cap);

/* ---- auxiliary sensors of a Monte-Carlo batch: pathgen.gps_gen (pathgen.py:596-625) and pathgen.mag_gen (:643-661).
 *      FreeIntegration does not consume them, so they are generated only when they are to be kept. */
typedef struct {
    int64_t  n;             /* IMU samples (magnetometer rate) */
    int64_t  m;             /* GPS samples */
    int64_t  runs;
    uint64_t run_offset;
    uint64_t seed;
    double   gps_sigma[6];  /* position sigma (already in rad,rad,m for ref_frame 0: pathgen.py:616-619) and velocity sigma */
    double   mag_si[9];     /* soft-iron matrix, row major */
    double   mag_hi[3];     /* hard iron [uT] */
    double   mag_std[3];    /* noise sigma [uT] */
    const double* ref_gps;  /* device [m][6] or NULL */
    const double* ref_mag;  /* device [n][3] or NULL */
    double*  out_gps;       /* device [6][m][runs] or NULL */
    double*  out_mag;       /* device [3][n][runs] or NULL */
} ginsim_aux_params;

int ginsim_aux_sensors(ginsim_ctx* ctx, const ginsim_aux_params* p);

/* ---- soft / hard-iron magnetometer calibration: demo_algorithms/mag_calibrate.py::MagCal (:63-88) and the library it calls
 *      (mag_calibrate_src/src/MagCalibration.c) over a batch of Monte-Carlo runs, one lane per run (csrc/magcal.hip).  Added
 *      without a change of GINSIM_ABI_VERSION: nothing existing moved.
 *      Per run, from the three row ranges seg = [x0,xf) [y0,yf) [z0,zf) of its (n, 3) magnetometer series (the rotations about
 *      x, y and z): the normal of each range (3x3 normal equations) -> orthMtx; the relative sensitivities from the (max - min) of
 *      the rotated columns -> soft_iron = sens . orthMtx; a sphere fit over the scaled rows of all three ranges (4x4 normal
 *      equations) -> hard_iron = [centre, radius]; mag_cal = the scaled rows minus the centre.
 *      The series is either GENERATED inside the kernel (ref_mag given: sample j of run r is what ginsim_aux_sensors writes for
 *      the same seed, run_offset and mag_si / mag_hi / mag_std, bit for bit, and is never stored) or GIVEN (in_mag).
 *      Arithmetic is IEEE throughout: a degenerate range gives the non-finite values the divisions give, no error. */
typedef struct {
    int64_t  n;             /* samples of the magnetometer series */
    int64_t  runs;
    uint64_t run_offset;
    uint64_t seed;
    double   mag_si[9];     /* generated form: soft-iron matrix, row major; hard iron [uT]; noise sigma [uT] */
    double   mag_hi[3];
    double   mag_std[3];
    const double* ref_mag;  /* device [n][3]: generated form, or NULL */
    const double* in_mag;   /* device [3][n][runs]: given form (takes precedence), or NULL */
    int64_t  seg[6];        /* x0, xf, y0, yf, z0, zf: 0 <= start < end <= n */
    double*  out_si;        /* device [9][runs]: soft_iron, row major */
    double*  out_hi;        /* device [4][runs]: hard_iron x, y, z, radius */
    double*  out_cal;       /* device [3][(xf-x0)+(yf-y0)+(zf-z0)][runs]: mag_cal, the three ranges stacked, or NULL */
} ginsim_magcal_params;

int ginsim_magcal_run(ginsim_ctx* ctx, const ginsim_magcal_params* p);

/* ---- end-point statistics: InsDataMgr.__end_point_error_stats / __array_stats
 *      (gnss_ins_sim/sim/ins_data_manager.py:717-759, 797-808) ------------------------------------ */
typedef struct {
    double count;
    double mean[9];
    double m2[9];           /* sum of squared deviations from mean; std(ddof=0) = sqrt(m2/count) */
    double maxabs[9];
} ginsim_stats;             /* 28 doubles; mergeable across devices (Chan et al.) */

int ginsim_end_stats(ginsim_ctx* ctx, const double* end_err /*device [9][runs]*/, int64_t runs, ginsim_stats* host_out);

/* The same reduction without blocking the host: _begin enqueues the reduction and the copy of the record into pinned
 * host slot `slot` (0..7) on the context's stream; _finish waits for that slot only and returns the record.  A caller
 * can enqueue the next ginsim_mc_run between the two, so the host-side merge / multi-GPU exchange of batch k overlaps
 * the integration of batch k+1. */
int ginsim_end_stats_begin(ginsim_ctx* ctx, const double* end_err, int64_t runs, int32_t slot);
int ginsim_end_stats_finish(ginsim_ctx* ctx, int32_t slot, ginsim_stats* host_out);

/* ---- multi-GPU: Monte-Carlo runs shard over ranks by global run id (run_offset), one process and one context per GPU; the
 *      ONE exchange of the path is every rank's statistics record to every rank.  ABI 3 puts it behind the
 *      boundary: an RCCL all-gather enqueued on the context's stream right behind the on-device reduction (librccl is
 *      resolved at run time on first use; single-GPU callers never load it).  The reference has no counterpart
 *      (gnss_ins_sim/sim/ins_sim.py:490 is a serial loop).
 *      Bootstrap: rank 0 calls ginsim_comm_unique_id and hands the 128 bytes to the other ranks through whatever launcher the
 *      caller uses (an environment variable, a file, torch.distributed's store ...); every rank then calls ginsim_comm_init. */
#define GINSIM_COMM_ID_BYTES 128
/* ABI 4: can librccl be reached from this process (dlopen + dlsym, nothing else)?  Every rank calls it and the verdicts are
 * reduced BEFORE anyone enters the collective ginsim_comm_init: a rank that failed alone would leave the others waiting there. */
int ginsim_comm_probe(void);
/* rank 0 only (it starts RCCL's bootstrap listener for this id) */
int ginsim_comm_unique_id(unsigned char* id /*[GINSIM_COMM_ID_BYTES]*/);
/* Collective over the nranks ranks (ncclCommInitRank): returns an error on every rank or on none once all have entered; a rank
 * that never enters (it failed earlier) leaves the others blocked inside RCCL -- hence ginsim_comm_probe.  On failure the
 * context is left without a communicator and may retry. */
int ginsim_comm_init(ginsim_ctx* ctx, int32_t nranks, int32_t rank, const unsigned char* id);
int ginsim_comm_destroy(ginsim_ctx* ctx);
/* ABI 7: what the communicator ITSELF answers (ncclCommCount, ncclCommUserRank, ncclCommCuDevice) -- evidence that RCCL saw the
 * ranks the caller meant, for the benchmark line (`rccl_ranks`); -1 where the loaded librccl lacks a query. */
int ginsim_comm_query(ginsim_ctx* ctx, int32_t* nranks, int32_t* rank, int32_t* device);
/* ginsim_end_stats_begin / _finish over ALL ranks: reduction of this rank's end errors (runs may be 0: an empty record) ->
 * all-gather of the 28-double records -> copy into pinned slot `slot` (0..7), all on the context's stream; _finish waits for
 * that slot only and returns the Chan merge of the non-empty records in rank order (the same on every rank). */
int ginsim_end_stats_all_begin(ginsim_ctx* ctx, const double* end_err, int64_t runs, int32_t slot);
int ginsim_end_stats_all_finish(ginsim_ctx* ctx, int32_t slot, ginsim_stats* merged);

/* Process-error statistics of every run: InsDataMgr.__process_error_stats (ins_data_manager.py:761-795) over
 * array_error (:519-553): e[j] = traj[j] - ref[j] for samples j >= first_sample, attitude wrapped to [-pi,pi];
 * pos_ned != 0 (ref_frame 0, extra_opt='ned'): LLA error -> metres in the local NED frame of the reference (:542-552).
 * traj: device [9][n][runs]; ref: device [n][9] (att3,pos3,vel3 truth).  host_out [runs][3][9] = max|e|, mean, std(ddof=0). */
int ginsim_process_stats(ginsim_ctx* ctx, const double* traj, const double* ref, int64_t n, int64_t runs,
                         int64_t first_sample, int32_t pos_ned, double* host_out);
/* End-point statistics recomputed from kept trajectories (e.g. with pos_ned after the run): last-sample error of
 * every run on the device, then the same reduction as ginsim_end_stats. */
int ginsim_end_stats_from_traj(ginsim_ctx* ctx, const double* traj, const double* ref, int64_t n, int64_t runs,
                               int32_t pos_ned, ginsim_stats* host_out);
/* ABI 4: the same two statistics over the FLOAT trajectories of the fp32 kernel (precision 1), whose position planes hold the
 * displacement from the run's initial position: origin = device [n_ini][3], the initial positions (ECEF metres for ref_frame
 * 1, LLA for ref_frame 0) of the initial-state table the launch used, ini_first as in ginsim_mc_params.  The position of a sample
 * is formed as origin + displacement in fp64 and everything after it is the fp64 arithmetic of the calls above. */
int ginsim_process_stats_f32(ginsim_ctx* ctx, const float* traj, const double* ref, int64_t n, int64_t runs, int64_t first_sample,
                             int32_t pos_ned, const double* origin, int32_t n_ini, uint64_t ini_first, double* host_out);
int ginsim_end_stats_from_traj_f32(ginsim_ctx* ctx, const float* traj, const double* ref, int64_t n, int64_t runs, int32_t pos_ned,
                                   const double* origin, int32_t n_ini, uint64_t ini_first, ginsim_stats* host_out);
int ginsim_stats_merge(const ginsim_stats* parts, int32_t nparts, ginsim_stats* out);

/* ---- error-growth curves: the ACROSS-RUN statistics of the error at every requested sample (csrc/error_curve.hip).  At sample
 *      j this is __end_point_error_stats + __array_stats (ins_data_manager.py:717-759, 797-808) applied to the series cut after j,
 *      with the error expression of ginsim_process_stats (attitude wrapped, pos_ned as there).  Added without a change of
 *      GINSIM_ABI_VERSION: nothing existing moved.
 *      traj: device [9][n][runs]; ref: device [n][9]; samples: HOST int64[m] sample indices in [0, n), in any order, repeats
 *      allowed, or NULL = every sample (m must then be n).  host_out: [m][9] records of GINSIM_CURVE_RECORD doubles
 *      (count, mean, M2, max|e|): std(ddof=0) = sqrt(M2 / count).  The order of the sums depends on n, runs, m and on whether
 *      traj is 16-byte aligned (hipMalloc'ed and placed regions are; an aligned traj with an even run count of at least 128 is
 *      read two runs per lane, anything else one): the same (n, runs, m, alignment of traj) gives the same bits at every call,
 *      another alignment the same numbers to rounding. */
#define GINSIM_CURVE_RECORD 4
int ginsim_error_curve(ginsim_ctx* ctx, const double* traj, const double* ref, int64_t n, int64_t runs, const int64_t* samples,
                       int64_t m, int32_t pos_ned, double* host_out);
/* the same over the FLOAT trajectories of the fp32 kernel; origin, n_ini, ini_first as ginsim_process_stats_f32 takes them */
int ginsim_error_curve_f32(ginsim_ctx* ctx, const float* traj, const double* ref, int64_t n, int64_t runs, const int64_t* samples,
                           int64_t m, int32_t pos_ned, const double* origin, int32_t n_ini, uint64_t ini_first, double* host_out);
/* Host only: the curves of nparts sets of runs (parts: [nparts][m][9] records; a set without runs is all zeros) folded record by
 * record with the Chan merge of ginsim_stats_merge, in the order given. */
int ginsim_curve_merge(const double* parts, int32_t nparts, int64_t m, double* out);

/* ---- error quantiles across the runs (csrc/error_quantile.hip): the radius that holds a given share of the runs (CEP50, CEP95 /
 *      R95) and the same quantiles of the vertical and the 3-D error.  Moments do not give them: the radial error is not Gaussian.
 *      Added without a change of GINSIM_ABI_VERSION: nothing existing moved.
 *      ginsim_radial_keys reads kept planes as ginsim_error_curve does (traj: device [9][n][runs]; ref: device [n][9]; samples:
 *      HOST int64[m] in [0, n), any order, repeats allowed, or NULL = every sample, m must then be n) and forms, for which = 0 the
 *      position error (components 3..5; pos_ned != 0: in local NED metres, what ref_frame 0 needs for a radius to mean anything)
 *      or for which = 1 the velocity error (components 6..8; pos_ned is not looked at), with the error expression of
 *      ginsim_error_curve.  Per (sample s, run r) it writes three non-negative keys, k = 0 horizontal sqrt(e0^2 + e1^2), k = 1
 *      vertical |e2|, k = 2 3-D sqrt(e0^2 + e1^2 + e2^2), to the DEVICE array keys[(k * m + s) * row_stride + col0 + r]:
 *      row_stride >= col0 + runs, so that blocks of runs (or devices) fill one row of row_stride keys per (k, s), each at its col0.
 *      ginsim_quantile_rows: exact order statistics of each of `rows` rows of `len` doubles, row_stride (>= len) apart on the
 *      device, for q (1..GINSIM_QUANTILE_MAX_PROBS) probabilities in (0, 1] at once.  Keys that are not finite are left out;
 *      host_count[row] = N, the keys included.  host_out[row][i] is the k-th smallest included key, k = min(max(ceil(probs[i] * N),
 *      1), N) with probs[i] * N one fp64 product -- nearest rank, np.quantile(method='inverted_cdf') --, one of the keys bit for
 *      bit (no interpolation; -0.0 orders before +0.0), NaN when N = 0.  The same row gives the same bits at every call. */
#define GINSIM_QUANTILE_MAX_PROBS 8
int ginsim_radial_keys(ginsim_ctx* ctx, const double* traj, const double* ref, int64_t n, int64_t runs, const int64_t* samples,
                       int64_t m, int32_t which, int32_t pos_ned, double* keys, int64_t row_stride, int64_t col0);
/* the same over the FLOAT trajectories of the fp32 kernel; origin, n_ini, ini_first as ginsim_error_curve_f32 takes them */
int ginsim_radial_keys_f32(ginsim_ctx* ctx, const float* traj, const double* ref, int64_t n, int64_t runs, const int64_t* samples,
                           int64_t m, int32_t which, int32_t pos_ned, const double* origin, int32_t n_ini, uint64_t ini_first,
                           double* keys, int64_t row_stride, int64_t col0);
int ginsim_quantile_rows(ginsim_ctx* ctx, const double* keys, int64_t rows, int64_t len, int64_t row_stride, const double* probs,
                         int32_t q, double* host_out, double* host_count);

/* ---- error covariance across the runs (csrc/error_cov.hip): the mean vector and the 3x3 covariance of the position or velocity
 *      error at every requested sample -- which way the error points (along / cross track, the error ellipse), what neither the
 *      per-component moments of ginsim_error_curve nor the radii of ginsim_quantile_rows tell.  Added without a change of
 *      GINSIM_ABI_VERSION: nothing existing moved.
 *      traj, ref, n, runs, samples, m as ginsim_radial_keys takes them; which = 0 the position error (components 3..5; pos_ned != 0:
 *      in local NED metres), which = 1 the velocity error (components 6..8; pos_ned is not looked at), with the error expression of
 *      ginsim_error_curve; only those three planes are read.  host_out: [m] records of GINSIM_COV_RECORD doubles: count, mean[3],
 *      C[6] = sum (e_a - mean_a)(e_b - mean_b) over the runs in the order 00, 01, 02, 11, 12, 22; covariance (ddof 0) = C / count.
 *      A run with ANY of its three components not finite at a sample is left out of that sample's record (unlike
 *      ginsim_error_curve, which lets it poison the record): count is the number of runs that entered.  count = 0: mean and C are
 *      NaN; count = 1: the run's error and C exactly 0.  The same (n, runs, m) gives the same bits at every call. */
#define GINSIM_COV_RECORD 10
int ginsim_error_cov(ginsim_ctx* ctx, const double* traj, const double* ref, int64_t n, int64_t runs, const int64_t* samples,
                     int64_t m, int32_t which, int32_t pos_ned, double* host_out);
/* the same over the FLOAT trajectories of the fp32 kernel; origin, n_ini, ini_first as ginsim_error_curve_f32 takes them */
int ginsim_error_cov_f32(ginsim_ctx* ctx, const float* traj, const double* ref, int64_t n, int64_t runs, const int64_t* samples,
                         int64_t m, int32_t which, int32_t pos_ned, const double* origin, int32_t n_ini, uint64_t ini_first,
                         double* host_out);
/* Host only: the records of nparts sets of runs (parts: [nparts][m] records; a set without runs is all zeros, or any record of
 * count 0) folded record by record with C = C_a + C_b + dd^T n_a n_b / n, d = mean_b - mean_a, in the order given; a result
 * without runs is count 0 with NaN mean and C. */
int ginsim_cov_merge(const double* parts, int32_t nparts, int64_t m, double* out);

/* ---- data access: pull selected runs out of a [ncomp][n][runs] device series into host [nsel][n][ncomp] */
int ginsim_gather_runs(ginsim_ctx* ctx, const double* series, int32_t ncomp, int64_t n, int64_t runs,
                       const int64_t* run_ids /*host*/, int32_t nsel, double* host_out);
/* same for a SERIES-major sensor buffer (sensor_layout 1): series [runs][ncomp][n] -> host [nsel][n][ncomp] */
int ginsim_gather_series(ginsim_ctx* ctx, const double* series, int32_t ncomp, int64_t n, int64_t runs,
                         const int64_t* run_ids /*host*/, int32_t nsel, double* host_out);
/* same for a float series written by the fp32 kernel (values widened to double on the way out) */
int ginsim_gather_runs_f32(ginsim_ctx* ctx, const float* series, int32_t ncomp, int64_t n, int64_t runs,
                           const int64_t* run_ids /*host*/, int32_t nsel, double* host_out);

/* ---- given-data mechanisation with host buffers: the plugin's .run(set_of_input) boundary
 *      (free_integration.py:63-174 / free_integration_odo.py:63-160).  gyro/accel [R][n][3], odo [R][n],
 *      ini [n_ini][10]; outputs att/pos/vel [R][n][3].  algo is ONE GINSIM_ALGO_* bit. */
int ginsim_free_integration(ginsim_ctx* ctx, int32_t algo, int32_t ref_frame, double fs, int32_t earth_rot,
                            const double* gyro, const double* accel, const double* odo, int64_t R, int64_t n,
                            const double* ini, int32_t n_ini, int32_t ini_has_g, uint64_t ini_first,
                            double* att, double* pos, double* vel);

/* ---- Allan variance: allan.allan_var (gnss_ins_sim/allan/allan.py:18-59) for a batch of series, as the Allan
 *      plugin applies it to each sensor axis (demo_algorithms/allan_analysis.py:33-49).
 *      x: device pointer, series s occupies x[s*series_stride .. +n).  Outputs (host): tau[cap] and
 *      avar[nseries][cap] (Allan VARIANCE; the plugin reports its square root); *ntau = number of averaging
 *      factors (0 when the series is shorter than 9 s, allan.py:30-31). */
int ginsim_allan(ginsim_ctx* ctx, const double* x, int64_t n, int32_t nseries, int64_t series_stride, double fs,
                 double* tau, double* avar, int32_t* ntau, int32_t cap);

/* Which kernel form ginsim_allan runs at every decade level of such a call, from the planning code the call itself launches
 * from.  Host arithmetic only: no context, no device, nothing launched, x never followed (only its value modulo 16 counts).
 * Level k holds n / 10^k entries per series.  mode: 0 register-staged allan_level_kernel, 1 wave-pair LDS-DMA allan_pair_kernel,
 * 2 allan_fused_kernel as its first level, 3 as its second, 4 allan_tail_kernel (levels of at most one 2520-entry chunk).
 * chunks_per_block and nparts: chunks a wavefront (mode 0) or workgroup (1, 2, 3) folds, and partial records per series.
 * *ntau as ginsim_allan reports it, *nlevels = levels of the call (0 when ntau is 0); GINSIM_ERR_RANGE when cap is smaller.
 * A call whose chunked levels (modes 0-3) have more series than the device's maxGridSize[1] is refused by ginsim_allan with
 * GINSIM_ERR_RANGE before any launch: split the batch.  Added without a change of GINSIM_ABI_VERSION: nothing existing moved. */
typedef struct {
    int64_t n_in, in_stride;
    int32_t mode, chunks_per_block, nparts, reserved;
} ginsim_allan_level;
int ginsim_allan_plan(const double* x, int64_t n, int32_t nseries, int64_t series_stride, double fs, int32_t* ntau,
                      int32_t* nlevels, ginsim_allan_level* levels /*[cap]*/, int32_t cap);

/* Device-to-device re-layout of a Monte-Carlo series [ncomp][n][runs] (run fastest, what ginsim_mc_run writes) into
 * per-run contiguous series [runs][ncomp][n] -- the input layout of ginsim_allan, so that the Allan plugin
 * (demo_algorithms/allan_analysis.py:33-49) works on the generated sensors without a host round trip. */
int ginsim_runs_to_series(ginsim_ctx* ctx, const double* series, int32_t ncomp, int64_t n, int64_t runs, double* out);

/* ---- RNG self-test hook: first `count` normal pairs of (seed, run, stream) computed ON DEVICE.  Stream s at sample j is
 *      half (s & 1) of the Philox4x32-7 block with counter (j, s >> 1, run_lo, run_hi) and key = seed; each of its two words
 *      gives one normal by a piecewise-cubic inversion of the tail probability that is defined operation by operation in
 *      IEEE single precision on a committed coefficient table (csrc/fastmath.hpp normal_icdf; spelled out in
 *      oracle/philox.py, which reproduces the device's normals to the bit).  |z| <= 6.23.  The normals are single-precision
 *      numbers returned as doubles.  host_words, if given, receives the raw block with counter (j, stream, run_lo, run_hi). ---- */
int ginsim_rng_normals(ginsim_ctx* ctx, uint64_t seed, uint64_t run, uint32_t stream, int64_t count,
                       double* host_z0, double* host_z1, uint32_t* host_words /*[count][4] or NULL*/);

/* Test hook: the device's normal transform applied to caller-chosen Philox words (z0 from w[i][0], z1 from w[i][1]; w[i][2..3]
 * unused), so that corner cases no seed will produce in a test (smallest / largest magnitude, every segment edge of the
 * coefficient table) can be pinned against the oracle. */
int ginsim_normal_transform(ginsim_ctx* ctx, const uint32_t* host_words /*[count][4]*/, int64_t count, double* host_z0,
                            double* host_z1);

/* ---- ABI 9: memory self-test.  Word i (64-bit, counted from dptr) of a pattern is ((uint64_t)tag << 40) | i: unique per
 *      (tag, offset), so that a word found in the wrong place names its cause -- another region's tag: an alias; 0: a zero
 *      fill; a repeated byte: a memset.  Written and read by kernels on the context's stream (oracle/pattern.py spells out
 *      the same formulas); bytes % 8 == 0, dptr 8-byte aligned, bytes / 8 < 2^40.  Each call synchronises the stream. ---- */
int ginsim_pattern_fill(ginsim_ctx* ctx, void* dptr, size_t bytes, uint32_t tag);
/* bad: the number of words that differ from the pattern; first_bad_offset: the byte offset of the lowest (-1: none); found:
 * the word read there (0 when none). */
int ginsim_pattern_check(ginsim_ctx* ctx, const void* dptr, size_t bytes, uint32_t tag, int64_t* bad, int64_t* first_bad_offset,
                         uint64_t* found);
/* Order-independent 64-bit digest: sum over i of splitmix64(w_i ^ (i * 0x9E3779B97F4A7C15)) mod 2^64, with the standard
 * splitmix64 finaliser (add 0x9E3779B97F4A7C15, then the two xor-shift-multiplies and a final xor-shift). */
int ginsim_digest(ginsim_ctx* ctx, const void* dptr, size_t bytes, uint64_t* out);

#ifdef __cplusplus
}
#endif
#endif /* GINSIM_H */
