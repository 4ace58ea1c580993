#!/usr/bin/env python3
"""Regenerate the committed evidence under profiles/ from ONE raw evidence run (gpurun_out/round_<tag>/, made by
tools/gpu_round.sh <tag>).  Every output carries the sha256 of the libginsim.so that ran and the tag of the raw run.

    python tools/summarize_prof.py <tag> [--traffic]

--traffic also (re)writes profiles/pmc_traffic.json, the file bench.py falls back to when it cannot run rocprofv3 itself; it
is only honoured by bench.py when its `libginsim_sha256` equals the hash of the library being benchmarked.
"""
import csv
import glob
import json
import os
import shutil
import sqlite3
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
tag = sys.argv[1]
SRC = os.path.join(REPO, 'gpurun_out', 'round_' + tag)
DST = os.path.join(REPO, 'profiles')
sha = open(os.path.join(SRC, 'lib_sha256.txt')).read().strip()
os.makedirs(DST, exist_ok=True)
stamp = '# raw run: gpurun_out/round_%s ; libginsim.so sha256[:16] = %s' % (tag, sha)


def db(name):
    hits = sorted(glob.glob(os.path.join(SRC, name, '**', '*.db'), recursive=True))
    return sqlite3.connect(hits[0]) if hits else None


# --- bench line + parity margins + test log tail
for f, out in (('bench.json', tag + '_bench_n1.json'), ('parity_margins.json', tag + '_parity_margins.json')):
    if os.path.exists(os.path.join(SRC, f)):
        shutil.copy(os.path.join(SRC, f), os.path.join(DST, out))
bench = json.load(open(os.path.join(SRC, 'bench.json')))
assert bench['config']['libginsim_sha256'] == sha, 'bench.json was produced by another library build'
with open(os.path.join(DST, tag + '_gpu_tests.txt'), 'w') as f:
    f.write(stamp + '\n')
    f.write(open(os.path.join(SRC, 'pytest_gpu.log')).read()[-600:])
    f.write(open(os.path.join(SRC, 'smoke.log')).read()[-200:])

# --- kernel trace of the default bench command
con = db('prof_trace')
# one row per kernel AND launch size: the same kernel serves several configurations (C2 headline, C4's share, ...)
rows = list(con.execute("select name, count(*), sum(end-start), avg(end-start), min(end-start), max(end-start), "
                        "max(vgpr_count), max(sgpr_count), max(lds_size), grid_x, max(workgroup_x) "
                        "from kernels group by name, grid_x order by sum(end-start) desc"))
total = sum(r[2] for r in rows)
with open(os.path.join(DST, tag + '_kernel_trace_stats.csv'), 'w', newline='') as f:
    w = csv.writer(f)
    w.writerow([stamp])
    w.writerow(['# rocprofv3 --kernel-trace --stats -- python bench.py --full --cpu-baseline-seconds 0 --pmc off   (200 timed + 30 warm-up steps, all legs)'])
    w.writerow(['kernel', 'calls', 'total_ns', 'avg_ns', 'min_ns', 'max_ns', 'percent', 'vgpr', 'sgpr', 'lds_bytes', 'grid_x', 'workgroup_x'])
    for r in rows:
        w.writerow([r[0], r[1], int(r[2]), int(r[3]), int(r[4]), int(r[5]), '%.2f' % (100.0 * r[2] / total)] + list(r[6:]))
k = bench['roofline']['kernel']
tr = [(r[1], r[3] / 1e6, r[9]) for r in rows if r[0].startswith('void ' + k + '(')]
tr.sort(reverse=True)       # the headline configuration is the one with the most launches (pre-warm + warm-up + timed steps)
agree = {'raw_run': 'gpurun_out/round_' + tag, 'libginsim_sha256': sha, 'kernel': k,
         'hip_events_ms_unprofiled_bench': bench['roofline']['kernel_ms_avg']}
if tr:
    # the TIMED launches are the last `steps` of that grid size; the same command's own HIP-event average (it ran under the
    # profiler: prof_trace.json) is the number the trace must agree with -- the un-profiled bench.json runs a few % faster
    durs = [r[0] / 1e6 for r in con.execute("select end - start from kernels where name like ? and grid_x = ? order by start",
                                            ('void ' + k + '(%', tr[0][2]))]
    steps = bench['steps']
    agree.update({'trace_launches': len(durs), 'trace_ms_avg_all': sum(durs) / len(durs)})
    try:
        prof_line = [l for l in open(os.path.join(SRC, 'prof_trace.json')).read().splitlines() if l.startswith('{')][-1]
        prof = json.loads(prof_line)
        agree['hip_events_ms_same_profiled_command'] = prof['roofline']['kernel_ms_avg']
        # round 6: the profiled command says WHICH launches of the trace its timed region was (the same kernel also runs in the
        # repeated region, with the other placement and inside the Sim legs)
        win = prof['roofline'].get('timed_launches')
        timed = durs[win['first']:win['first'] + win['count']] if win else durs[-steps:]
        agree.update({'trace_ms_avg_timed_steps': sum(timed) / len(timed), 'timed_launches': win})
    except (OSError, IndexError, ValueError, KeyError):
        agree['trace_ms_avg_timed_steps'] = sum(durs[-steps:]) / len(durs[-steps:])
with open(os.path.join(DST, tag + '_headline_kernel_agreement.json'), 'w') as f:
    json.dump(agree, f, indent=1)
print(json.dumps(agree))

con = db('prof_allan')
if con:
    rows = list(con.execute("select name, grid_x, grid_y, count(*), avg(end-start), min(end-start), max(end-start), max(vgpr_count), max(lds_size) "
                            "from kernels where name like '%allan%' group by name, grid_x, grid_y order by avg(end-start) desc"))
    with open(os.path.join(DST, tag + '_allan_kernel_trace.csv'), 'w', newline='') as f:
        w = csv.writer(f)
        w.writerow([stamp])
        w.writerow(['# rocprofv3 --kernel-trace --stats -- python tools/bench_allan.py  (192 series x 1 440 000 samples, 11 calls)'])
        w.writerow(['kernel', 'grid_x', 'grid_y', 'calls', 'avg_ns', 'min_ns', 'max_ns', 'vgpr', 'lds_bytes'])
        for r in rows:
            w.writerow([r[0], r[1], r[2], r[3], int(r[4]), int(r[5]), int(r[6]), r[7], r[8]])

# --- PMC passes
pmc = {}
for d in sorted(os.listdir(SRC)):
    if d.startswith('prof_pmc'):
        con = db(d)
        if con:
            for kn, c, n, avg, mn, mx in con.execute("select kernel_name, counter_name, count(*), avg(value), min(value), max(value) "
                                                     "from counters_collection group by kernel_name, counter_name"):
                pmc.setdefault(kn, {})[c] = (n, avg, mn, mx)
with open(os.path.join(DST, tag + '_pmc_counters.csv'), 'w', newline='') as f:
    w = csv.writer(f)
    w.writerow([stamp])
    w.writerow(['# rocprofv3 --pmc <one group per pass> --kernel-trace -- python bench.py --pmc-child (the C2 workload: headline, given-sensors and '
                'fp32 launch; since round 4 also a C3-shaped launch cut to 8192 samples with and without the online statistics, config 5\'s '
                'sensor generation and Allan calls); values are per dispatch (avg/min/max over dispatches)'])
    w.writerow(['kernel', 'counter', 'dispatches', 'avg', 'min', 'max'])
    for kn in sorted(pmc):
        for c in sorted(pmc[kn]):
            w.writerow([kn, c] + ['%.6g' % v if isinstance(v, float) else v for v in pmc[kn][c]])

traffic = {}
for kn, c in pmc.items():
    if 'mc_kernel' in kn and 'FETCH_SIZE' in c and 'WRITE_SIZE' in c:
        # MI355X_MICROARCH.md (HBM): rocprofv3 reports FETCH_SIZE/WRITE_SIZE in KiB; on gfx950 FETCH_SIZE reads half of the
        # bytes of a coalesced stream -> doubled.  WRITE_SIZE matches the known byte count of these kernels exactly.
        fetch_b, write_b = 2.0 * c['FETCH_SIZE'][1] * 1024, c['WRITE_SIZE'][1] * 1024
        name = kn[len('void '):] if kn.startswith('void ') else kn
        name = name[:name.index('(')]
        traffic[name] = {'hbm_bytes_per_launch': fetch_b + write_b, 'fetch_bytes_corrected': fetch_b, 'write_bytes': write_b,
                         'dispatches': c['WRITE_SIZE'][0]}
summary = {'raw_run': 'gpurun_out/round_' + tag, 'libginsim_sha256': sha, 'kernels': traffic}
with open(os.path.join(DST, tag + '_pmc_traffic.json'), 'w') as f:
    json.dump(summary, f, indent=1)
if '--traffic' in sys.argv:
    with open(os.path.join(DST, 'pmc_traffic.json'), 'w') as f:
        json.dump(summary, f, indent=1)
print(json.dumps(summary, indent=1))
# --- round 4: the compute-bound launches (C3) and the multi-kernel Allan call
XCDS, SIMDS = 8, 1024
extra = {}
for kn, c in pmc.items():
    name = kn[len('void '):kn.index('(')] if kn.startswith('void ') else kn[:kn.index('(')] if '(' in kn else kn
    if 'mc_kernel<0, 1, false' in kn and 'SQ_ACTIVE_INST_VALU' in c and 'GRBM_GUI_ACTIVE' in c and 'SQ_WAVES' in c:
        steps = 8191.0                  # bench.PMC_CUT_SAMPLES - 1
        cyc = c['GRBM_GUI_ACTIVE'][1] / XCDS
        extra[name] = {'valu_busy': 4.0 * c['SQ_ACTIVE_INST_VALU'][1] / (SIMDS * cyc),
                       'valu_per_step_and_64_runs': c['SQ_INSTS_VALU'][1] / c['SQ_WAVES'][1] / steps,
                       'salu_per_step_and_64_runs': c['SQ_INSTS_SALU'][1] / c['SQ_WAVES'][1] / steps if 'SQ_INSTS_SALU' in c else None,
                       'lds_bank_conflict_over_active': (c['SQ_LDS_BANK_CONFLICT'][1] / c['SQ_LDS_IDX_ACTIVE'][1]) if 'SQ_LDS_IDX_ACTIVE' in c else None,
                       'wait_inst_any_over_wave_cycles': (c['SQ_WAIT_INST_ANY'][1] / c['SQ_WAVE_CYCLES'][1]) if 'SQ_WAVE_CYCLES' in c and 'SQ_WAIT_INST_ANY' in c else None}
allan = {k: c for k, c in pmc.items() if 'ginsim::allan_' in k}
if allan and all('WRITE_SIZE' in c and 'FETCH_SIZE' in c for c in allan.values()):
    calls = [c['WRITE_SIZE'][0] for k, c in allan.items() if 'allan_tail_kernel' in k]
    if calls:
        w_b = sum(c['WRITE_SIZE'][0] * c['WRITE_SIZE'][1] for c in allan.values()) * 1024.0 / calls[0]
        f_b = sum(c['FETCH_SIZE'][0] * c['FETCH_SIZE'][1] for c in allan.values()) * 2048.0 / calls[0]
        extra['ginsim_allan (192 x 1 440 000, per call)'] = {'hbm_bytes': w_b + f_b, 'write_bytes': w_b, 'fetch_bytes_corrected': f_b,
                                                            'over_algorithmic': (w_b + f_b) / (8.0 * 192 * 1440000), 'calls': calls[0]}
with open(os.path.join(DST, tag + '_compute_bound_and_allan.json'), 'w') as f:
    json.dump({'raw_run': 'gpurun_out/round_' + tag, 'libginsim_sha256': sha, 'kernels': extra}, f, indent=1)
print(json.dumps(extra, indent=1))

valu = {}
for kn, c in pmc.items():
    if ('mc_kernel_split<' in kn or 'mc_kernel_f32_split<' in kn) and 'SQ_INSTS_VALU' in c and 'SQ_WAVES' in c:
        steps = 1000.0
        args_ = kn[kn.index('<') + 1:kn.index('>')].split(', ')
        prod = int(args_[3])                                # wavefronts per 64 runs = 1 consumer + PROD producers
        groups = c['SQ_WAVES'][1] / (1.0 + prod)
        name = kn[len('void '):kn.index('(')] if kn.startswith('void ') else kn[:kn.index('(')]
        valu[name] = {'valu_per_step_and_64_runs': c['SQ_INSTS_VALU'][1] / groups / steps,
                      'salu_per_step_and_64_runs': c['SQ_INSTS_SALU'][1] / groups / steps if 'SQ_INSTS_SALU' in c else None}
        print('%s: VALU per step and 64 runs = %.1f' % (name, valu[name]['valu_per_step_and_64_runs']))
with open(os.path.join(DST, tag + '_valu_per_step.json'), 'w') as f:
    json.dump({'raw_run': 'gpurun_out/round_' + tag, 'libginsim_sha256': sha, 'kernels': valu}, f, indent=1)

# --- round 5: per-unit utilisation of the dominant Allan kernel (levels 0 + 1 fused), VERDICT r04 item 1
units = {}
dur = {}
for d in sorted(os.listdir(SRC)):
    if d.startswith('prof_pmc'):
        con = db(d)
        if con:
            for kn, n, avg in con.execute("select name, count(*), avg(end - start) from kernels where name like '%allan%' group by name"):
                dur.setdefault(kn, []).append(avg)
for kn, c in pmc.items():
    if 'ginsim::allan_' not in kn or not dur.get(kn):
        continue
    t = sum(dur[kn]) / len(dur[kn]) * 1e-9                      # seconds per dispatch, averaged over the counter passes
    name = kn[len('void '):kn.index('(')] if kn.startswith('void ') else kn[:kn.index('(')] if '(' in kn else kn
    u = {'dispatch_us_under_the_counter_passes': t * 1e6}
    if 'FETCH_SIZE' in c and 'WRITE_SIZE' in c:
        u['hbm_bytes'] = (2.0 * c['FETCH_SIZE'][1] + c['WRITE_SIZE'][1]) * 1024
        u['hbm_frac_of_8TBps'] = u['hbm_bytes'] / t / 8e12
    if 'SQ_ACTIVE_INST_VALU' in c:
        u['valu_busy_frac_of_1024_simds_at_2.4GHz'] = 4.0 * c['SQ_ACTIVE_INST_VALU'][1] / (SIMDS * 2.4e9 * t)
    if 'SQ_LDS_IDX_ACTIVE' in c:
        u['lds_active_frac_of_256_cus_at_2.4GHz'] = c['SQ_LDS_IDX_ACTIVE'][1] / (256 * 2.4e9 * t)
        if 'SQ_LDS_BANK_CONFLICT' in c:
            u['lds_bank_conflict_over_active'] = c['SQ_LDS_BANK_CONFLICT'][1] / c['SQ_LDS_IDX_ACTIVE'][1]
    if 'SQ_WAVE_CYCLES' in c:
        for k in ('SQ_WAIT_INST_ANY', 'SQ_ACTIVE_INST_ANY', 'SQ_WAIT_ANY'):
            if k in c:
                u[k.lower() + '_over_wave_cycles'] = c[k][1] / c['SQ_WAVE_CYCLES'][1]
    units[name] = u
if units:
    with open(os.path.join(DST, tag + '_allan_units.json'), 'w') as f:
        json.dump({'raw_run': 'gpurun_out/round_' + tag, 'libginsim_sha256': sha,
                   'what': 'per-unit utilisation of the Allan kernels of config 5 (192 x 1 440 000): HBM bytes from FETCH_SIZE x 2 + WRITE_SIZE, '
                           'VALU-busy SIMD cycles (4 x SQ_ACTIVE_INST_VALU), LDS-array cycles (SQ_LDS_IDX_ACTIVE) and the wave-cycle split, each '
                           'against the dispatch time under the counter passes', 'kernels': units}, f, indent=1)
    print(json.dumps(units, indent=1))
