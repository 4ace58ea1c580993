"""Child process of test_gpu_allan_edges.py (section f): GINSIM_ALLAN_DMA and GINSIM_ALLAN_CPW are read once per process, so the
forced register-staged form needs a fresh one.  Runs the cases of allan_cases.FORCED under the environment it was started with,
asserts the plan of every call (mode 0 at every chunked level, the chunks per wavefront and records per series of the setting
named on the command line) and prints the variances as one JSON line."""
import json
import sys

import allan_cases as ac


def main(setting):
    import ginsim
    ctx = ginsim.Context(0)
    out = {}
    for n, (plan, parts3, parts0) in ac.FORCED.items():
        fs = ac.fs_of(n)
        stride, _ = ac.placement(n, ac.ALIGNED)
        buf = ctx.upload(ac.pack(ac.rows(600, n, fs, ac.FORCED_S), stride))
        _, lv = ginsim.allan_plan(buf, n, ac.FORCED_S, stride, fs)
        assert tuple(l['mode'] for l in lv) == plan, (n, lv)
        chunked = [l for l in lv if l['mode'] != ac.T]
        assert chunked and all(l['mode'] == ac.L and l['chunks_per_block'] == (3 if setting == 'cpw3' else 1) for l in chunked), (n, lv)
        assert tuple(l['nparts'] for l in chunked) == (parts3 if setting == 'cpw3' else parts0), (n, lv)
        avar, _ = ginsim.allan_var(ctx, buf, n, ac.FORCED_S, stride, fs)
        buf.free()
        out[str(n)] = avar.tolist()
    ctx.close()
    print(json.dumps(out))


if __name__ == '__main__':
    main(sys.argv[1])
