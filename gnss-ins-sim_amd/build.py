#!/usr/bin/env python3
"""Build libginsim.so (HIP kernels + C ABI) for gfx950, in-tree.

    python gnss-ins-sim_amd/build.py [--force] [--verbose]

hipcc cross-compiles without a GPU.  Objects go to gnss-ins-sim_amd/build/, the library to
gnss-ins-sim_amd/lib/libginsim.so (git-ignored, but shipped to the GPU box by gpurun).
"""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
CSRC = os.path.join(HERE, 'csrc')
OBJ = os.path.join(HERE, 'build')
LIB = os.path.join(HERE, 'lib', 'libginsim.so')
ARCH = 'gfx950'
HIPCC = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')

COMMON = ['-O3', '-std=c++17', '-fPIC', '-I' + os.path.join(REPO, 'include'), '-I' + CSRC, '-Wall',
          '-Wno-unused-function']
# The fp64 kernel flags: mc_kernel.hip's, shared by the four files split off from it (series, aux_sensors, rng_probe, layout) so
# that their kernels compile to the ISA they had inside it.
# machine-LICM hoists ~35 fp64 polynomial constants (SGPR pairs) out of the time loop and then spills them
# to VGPR lanes; without it they are re-materialised with s_mov next to their use (SGPR spills 192 -> 71)
# -ffp-contract=on: fused multiply-adds only where one source expression spells a*b+c, decided in the front
# end, so the plain and the wave-specialised kernels (same inlined functions) give identical bits
MC_FLAGS = ['--offload-arch=' + ARCH, '-mllvm', '-disable-machine-licm', '-ffp-contract=on']
# (source, extra flags)
SOURCES = [
    ('mc_kernel.hip', MC_FLAGS),
    ('series.hip', MC_FLAGS),
    ('aux_sensors.hip', MC_FLAGS),
    ('rng_probe.hip', MC_FLAGS),
    ('layout.hip', MC_FLAGS),
    # the fp32 kernel is DEFINED operation by operation (the float oracle repeats it to the bit): no contraction at all,
    # fused multiply-adds only where the source spells __builtin_fmaf
    # no SLP vectorisation either: it packed the consumer's float arithmetic into v_pk_*_f32 pairs (a 4-cycle-class
    # instruction) and paid for the pairing with v_mov: 53 packed + 38 moves of 152 VALU on the common path;
    # scalar, the same step is 169 plain VALU and the launch 15 % faster (nothing kept 0.685 -> 0.584 ms), 132 -> 120 VGPRs
    ('mc_kernel_f32.hip', ['--offload-arch=' + ARCH, '-mllvm', '-disable-machine-licm', '-ffp-contract=off', '-fno-slp-vectorize']),
    # the sensor synthesis must give mc_kernel.hip's bits (same -ffp-contract=on); the filter code switches contraction off itself
    ('inclinometer.hip', ['--offload-arch=' + ARCH, '-ffp-contract=on']),
    # the magnetometer synthesis must give aux_mag_kernel's bits (mag_synth.hpp, same -ffp-contract=on as aux_sensors.hip)
    ('magcal.hip', ['--offload-arch=' + ARCH, '-ffp-contract=on']),
    # sensors as mc_kernel.hip's, fixes as aux_sensors.hip's (gps_synth.hpp): the same -ffp-contract=on; machine-LICM off as for
    # mc_kernel.hip: 0 bytes of scratch in every instantiation (the file's header has the whole account; tests/test_ins_loose_oracle.py
    # reads the report)
    ('ins_loose.hip', MC_FLAGS),
    # the same lane with the odometer / non-holonomic aiding block (ins_loose.hpp): the same flags, its own resource report
    # (tests/test_ins_loose_aided_oracle.py reads it)
    ('ins_loose_aided.hip', MC_FLAGS),
    # the same lane once more with consistency checkpoints (ins_loose.hpp, CONS): the same flags, its own resource report
    # (tests/test_ins_loose_cons_oracle.py reads it)
    ('ins_loose_cons.hip', MC_FLAGS),
    # the same lane with the magnetometer block (ins_loose.hpp, MAG): the same flags -- the magnetometer synthesis must give
    # aux_mag_kernel's bits (mag_synth.hpp, -ffp-contract=on) -- and its own resource report (tests/test_ins_loose_mag_oracle.py reads it)
    ('ins_loose_mag.hip', MC_FLAGS),
    # the aided lane with 16 states, the odometer's scale factor the last (ins_loose.hpp, NS): the same flags, its own resource
    # report (tests/test_ins_loose_scale_oracle.py reads it)
    ('ins_loose_scale.hip', MC_FLAGS),
    # the aided lane with the standstill block, ZUPT and ZARU (ins_loose.hpp, STILL): the same flags, its own resource report
    # (tests/test_ins_loose_still_oracle.py reads it)
    ('ins_loose_still.hip', MC_FLAGS),
    # the aided lane with the magnetometer block, the standstill block and (ins_loose_all16.hip) the 16th state together
    # (ins_loose.hpp, Tail::ALL), twelve instantiations per file: the same flags, their own resource reports
    # (tests/test_ins_loose_all_oracle.py reads them)
    ('ins_loose_all.hip', MC_FLAGS),
    ('ins_loose_all16.hip', MC_FLAGS),
    # the combined lane once more with consistency checkpoints (ins_loose.hpp, CONS with Tail::ALL), six instantiations per file:
    # the same flags, their own resource reports (tests/test_ins_loose_all_cons_oracle.py reads them)
    ('ins_loose_all_cons.hip', MC_FLAGS),
    ('ins_loose_all_cons16.hip', MC_FLAGS),
    ('stats.hip', ['--offload-arch=' + ARCH]),
    ('error_curve.hip', ['--offload-arch=' + ARCH]),
    # error_curve.hip's flags: the keys are formed from the shared error expression (traj_error.hpp, quantity_error) and their sums
    # are spelt as fused multiply-adds, so no flag decides their bits (tests/test_error_quantiles_oracle.py reads the resource
    # report: no scratch)
    ('error_quantile.hip', ['--offload-arch=' + ARCH]),
    # the same error expression (traj_error.hpp); machine-LICM off as for mc_kernel.hip: hoisted out of the run loop, the constants of the
    # geodetic conversion (NED form) spill 16 SGPRs (tests/test_error_covariance_oracle.py reads the resource report: no scratch,
    # no spills)
    ('error_cov.hip', ['--offload-arch=' + ARCH, '-mllvm', '-disable-machine-licm']),
    ('allan.hip', ['--offload-arch=' + ARCH]),
    ('oallan.hip', ['--offload-arch=' + ARCH]),
    # one instantiation per segment length, 8 .. 8192 (tests/test_psd_oracle.py reads the resource report: no scratch)
    ('psd.hip', ['--offload-arch=' + ARCH]),
    # the half-band decimation of the octave cascade; its sums are spelt as fused multiply-adds, so no flag decides their bits
    # (tests/test_lpsd_oracle.py reads the resource report: no scratch)
    ('lpsd.hip', ['--offload-arch=' + ARCH]),
    # one instantiation per segment length, 8 .. 4096, four accumulators per bin in registers (tests/test_csd_oracle.py reads the
    # resource report: no scratch)
    ('csd.hip', ['--offload-arch=' + ARCH]),
    ('placed.hip', ['--offload-arch=' + ARCH]),
    ('vib_psd.hip', ['--offload-arch=' + ARCH]),
    ('selftest.hip', ['--offload-arch=' + ARCH]),
    # the C ABI glue, host code only: the core and its three areas (api_common.hpp is what they share)
    ('ginsim_api.hip', ['--offload-arch=' + ARCH]),
    ('api_series.hip', ['--offload-arch=' + ARCH]),
    ('api_mc.hip', ['--offload-arch=' + ARCH]),
    ('api_traj.hip', ['--offload-arch=' + ARCH]),
    # host-only truth generator; no fused multiply-adds (see the file header)
    ('pathgen.cpp', ['-x', 'c++', '-ffp-contract=off']),
    # RCCL behind the C ABI (host code; librccl is dlopen()ed at run time, nothing is linked)
    ('comm.cpp', ['-x', 'hip', '--offload-arch=' + ARCH]),
]


def newer(a, b):
    return not os.path.exists(b) or os.path.getmtime(a) > os.path.getmtime(b)


def build(force=False, verbose=False, tag=None, defines=(), xflags=()):
    """tag / defines: an experiment build (A/B timing) -> lib/libginsim_<tag>.so from build/<tag>/ objects compiled with
    -D<define>; loaded with GINSIM_LIB=<path>.  The product build has neither."""
    global OBJ, LIB
    if tag:
        OBJ = os.path.join(HERE, 'build', tag)
        LIB = os.path.join(HERE, 'lib', 'libginsim_%s.so' % tag)
    os.makedirs(OBJ, exist_ok=True)
    os.makedirs(os.path.dirname(LIB), exist_ok=True)
    # every header there is, private and public, found by pattern: a new one needs no line here to rebuild what includes it
    deps = [os.path.join(d, f) for d, ends in ((CSRC, ('.hpp', '.h', '.inc')), (os.path.join(REPO, 'include'), ('.h',)))
            for f in sorted(os.listdir(d)) if f.endswith(ends)]
    deps.append(os.path.abspath(__file__))
    objs = []
    for src, extra in SOURCES:
        s = os.path.join(CSRC, src)
        if not os.path.exists(s):
            continue
        o = os.path.join(OBJ, src.rsplit('.', 1)[0] + '.o')
        objs.append(o)
        if force or newer(s, o) or any(newer(d, o) for d in deps):
            cmd = [HIPCC] + COMMON + extra + ['-D' + d for d in defines] + (list(xflags) if src.startswith('mc_kernel') else []) + ['-c', s, '-o', o]
            if src.endswith('.hip'):
                # per-kernel registers / scratch / occupancy as the compiler reports them -> build/<name>.resources.txt
                # (tests/test_host_cpu.py holds the hot kernels to two wavefronts per SIMD and no AGPR spills)
                cmd.insert(1, '-Rpass-analysis=kernel-resource-usage')
            if verbose:
                print(' '.join(cmd))
            p = subprocess.run(cmd, stderr=subprocess.PIPE, universal_newlines=True)
            if p.returncode != 0:       # show the compiler's own message, not a parse error of its remarks
                sys.stderr.write('\n'.join(l for l in p.stderr.splitlines() if 'remark:' not in l) + '\n')
                raise subprocess.CalledProcessError(p.returncode, cmd)
            if src.endswith('.hip'):
                remarks = [l for l in p.stderr.splitlines() if 'kernel-resource-usage' in l and 'remark:' in l]
                with open(o[:-2] + '.resources.txt', 'w') as f:
                    f.write('\n'.join(l.split('remark:', 1)[1].replace('[-Rpass-analysis=kernel-resource-usage]', '').strip()
                                      for l in remarks) + '\n')
                other = [l for l in p.stderr.splitlines() if 'kernel-resource-usage' not in l and not l.startswith(' ')]
                other = [l for l in other if l.strip() and not l.lstrip().startswith('|')]
                if p.returncode != 0 or verbose:
                    sys.stderr.write(p.stderr if p.returncode != 0 else '\n'.join(other) + '\n')
            elif p.stderr:
                sys.stderr.write(p.stderr)
            if p.returncode != 0:
                raise subprocess.CalledProcessError(p.returncode, cmd)
    if force or any(newer(o, LIB) for o in objs):
        # no undefined symbols: a launcher that launch.hpp declares and nothing defines fails here, not when the library is loaded
        cmd = [HIPCC, '-shared', '-fPIC', '-Wl,-z,defs', '--offload-arch=' + ARCH, '-o', LIB] + objs + ['-ldl']
        if verbose:
            print(' '.join(cmd))
        subprocess.check_call(cmd)
    return LIB


if __name__ == '__main__':
    _tag = sys.argv[sys.argv.index('--tag') + 1] if '--tag' in sys.argv else None
    _defs = [a[2:] for a in sys.argv if a.startswith('-D')]
    _xf = ['-' + a[2:] for a in sys.argv if a.startswith('-X')]      # -X<flag>: extra compiler flag for the MC kernels (experiments)
    print(build(force='--force' in sys.argv, verbose='--verbose' in sys.argv or '-v' in sys.argv, tag=_tag, defines=_defs, xflags=_xf))
