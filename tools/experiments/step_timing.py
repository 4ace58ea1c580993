"""Where the consumer wavefront of mc_kernel_split spends a step (DESIGN_EXPERIMENTS E9).

    python gnss-ins-sim_amd/build.py --tag timing -DGINSIM_STEP_TIMING
    GINSIM_LIB=gnss-ins-sim_amd/lib/libginsim_timing.so python tools/experiments/step_timing.py [--stats-only]

A C2-shaped launch with an experiment library whose consumer wave 0 of every workgroup sums s_memtime deltas from the top of a step to
the finished sensor sums and over the whole step (ginsim_step_timing reads the table); prints the per-step means as one JSON line."""
import ctypes as C, json, os, sys
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "gnss-ins-sim_amd"))
import numpy as np
import ginsim
from ginsim import workloads
keep = '--stats-only' not in sys.argv
ctx = ginsim.Context(0)
ini, truth, _ = workloads.truth_from_profile('turn_90deg', 100.0, 1)
n = 1000
truth = {k: (v[:n] if hasattr(v, 'shape') and v.shape and v.shape[0] >= n else v) for k, v in truth.items()}
acc, gyr = workloads.imu_grade('mid-accuracy')
R = 65536
job = ginsim.MonteCarloJob(ctx, 100.0, 1, truth, acc, gyr, ini, runs=R, seed=1, keep_sensors=keep, keep_traj=keep)
name = job.kernel_name()
for _ in range(20):
    job.launch()
ctx.sync()
G = R // 256
buf = (C.c_ulonglong * (2 * G))()
f = ginsim.lib.ginsim_step_timing
f.restype = C.c_int
rc = f(buf, G)
t = np.array(buf[:], dtype=np.float64).reshape(G, 2)
steps = job.n - 1 + (1 if keep else 0)
out = {'lib': os.environ.get('GINSIM_LIB'), 'kernel': name, 'keep': keep, 'rows': rc, 'n': job.n, 'steps_timed_per_wave': steps,
       'input_cycles_per_step_mean': float(t[:, 0].mean() / steps), 'step_cycles_per_step_mean': float(t[:, 1].mean() / steps),
       'input_cycles_per_step_min_max': [float(t[:, 0].min() / steps), float(t[:, 0].max() / steps)],
       'step_cycles_per_step_min_max': [float(t[:, 1].min() / steps), float(t[:, 1].max() / steps)],
       'input_share_of_step': float(t[:, 0].sum() / t[:, 1].sum())}
print(json.dumps(out))
job.release()
