"""Characterisation of Sim's Monte-Carlo driver (gnss_ins_sim/sim/ins_sim.py) on a host without a GPU.

libginsim.so loads without a device and ginsim.pathgen is host code, so Sim.run() runs to its end once the device classes
(ginsim.default_context / Context / MonteCarloJob / InclinometerJob / AuxSensorJob, multi.DeviceSet / JobSet / AuxJobSet) are
replaced by recorders.  The recorders log, in order, every job construction (class, name of its context, the arguments bound to the
REAL constructor's signature with its defaults applied -- an omitted argument and its default spelled out are the same record),
every launch() / run() / release(), every sync() and every first_xcc() question; afterwards the test logs what the data manager
and sim.mc hold and asks sim.mc for statistics over another window, which makes the jobs that are built on demand.

tests/golden/sim_driver_trace.json holds the logs of every case below, recorded from commit 384e0b4 (the driver as one 297-line
function) by this file run with GINSIM_RECORD_TRACE=1.  It is the definition of "the same behaviour" for any later shape of the
driver and is not regenerated from a changed driver.

The second half tests the driver's plan function directly, for the numbers a trace shows only indirectly.  Expected values are
written out from the formulas of commit 384e0b4 (ins_sim.py:466-474, 526-527, 631-632 there)."""
import inspect
import json
import os
import zlib

import numpy as np
import pytest

from conftest import GOLDEN, PKG

FIXTURE = os.path.join(GOLDEN, 'sim_driver_trace.json')
CSV = os.path.join(PKG, 'motion_profiles', 'turn_90deg.csv')
XCC = {'main': 0, 'ctx1': 5, 'ctx2': 2, 'ctx3': 6, 'ctx4': 1, 'ctx5': 4}     # first_xcc() by context name: both orders of the pair occur


def digest(v):
    """JSON-able form of an argument: arrays as shape + dtype + CRC of their bytes."""
    if isinstance(v, np.ndarray):
        return 'nd%s %s %08x' % (list(v.shape), v.dtype, zlib.crc32(np.ascontiguousarray(v).tobytes()))
    if isinstance(v, dict):
        return {str(k): digest(x) for k, x in sorted(v.items(), key=lambda t: str(t[0]))}
    if isinstance(v, (list, tuple)):
        return [digest(x) for x in v]
    if isinstance(v, (np.floating, np.integer, np.bool_)):
        return v.item()
    if v is None or isinstance(v, (bool, int, float, str)):
        return v
    return getattr(v, 'name', None) or type(v).__name__


class Recorder(object):
    """The stand-ins for one case; `log` is the trace."""

    def __init__(self, monkeypatch):
        import ginsim
        from ginsim import multi
        from gnss_ins_sim.sim import ins_sim
        rec, self.log, self.made, self.contexts = self, [], 0, 0
        real = {'MonteCarloJob': ginsim.MonteCarloJob, 'InclinometerJob': ginsim.InclinometerJob, 'AuxSensorJob': ginsim.AuxSensorJob,
                'JobSet': multi.JobSet, 'AuxJobSet': multi.AuxJobSet}
        inner = {'JobSet': 'MonteCarloJob', 'AuxJobSet': 'AuxSensorJob'}      # the sets forward **kw to these constructors

        def bound(cls, args, kw):
            sig = inspect.signature(real[cls].__init__)
            b = sig.bind(None, *args, **kw)
            b.apply_defaults()
            out = dict(b.arguments)
            out.pop('self')
            if cls in inner:
                out.update(out.pop('kw'))
                for p in list(inspect.signature(real[inner[cls]].__init__).parameters.values())[2:]:
                    if p.default is not p.empty:
                        out.setdefault(p.name, p.default)
            return out

        class Ctx(object):
            PLACED_MIN_JOB = 2 ** 30

            def __init__(self, device=0, name=None):
                if name is None:
                    rec.contexts += 1
                    name = 'ctx%d' % rec.contexts
                self.device, self.name, self.handle = int(device), name, 1000 + rec.contexts + (0 if name != 'main' else 500)

            def first_xcc(self):
                rec.log.append(['first_xcc', self.name])
                return XCC[self.name]

            def sync(self):
                rec.log.append(['sync', self.name])

        class DevSet(Ctx):
            def __init__(self, devices):
                self.devices = multi.parse_devices(devices)
                self.name = 'devset%s' % (self.devices,)

            def __len__(self):
                return len(self.devices)

        class Job(object):
            cls = 'MonteCarloJob'
            passes = 3

            def __init__(self, *args, **kw):
                a = self.args = bound(self.cls, args, kw)
                rec.made += 1
                self.serial, self.name = rec.made, 'job%d' % rec.made
                ctx = a.pop('ctx', None) or a.pop('devset', None)
                self.runs, self.n = int(a['runs']), int(a['truth']['ref_accel'].shape[0]) if 'truth' in a else 0
                self.precision, self.algos = a.get('precision', 'f64'), tuple(a.get('algos', ()))
                self.keep_traj, self.proc_ned, self.end_ned = bool(a.get('keep_traj', False)), bool(a.get('proc_ned', False)), a.get('end_ned')
                self.proc_first = a.get('proc_first')
                rec.log.append([self.cls, self.name, ctx.name, digest(a)])

            def _said(self, what):
                rec.log.append([what, self.name])
                return self

            launch = lambda self: self._said('launch') and None
            run = lambda self: self._said('run')
            release = lambda self: self._said('release') and None
            placement = lambda self: 'placement of ' + self.name

            def _fill(self, run_ids, comps, salt):        # a value per (job, series, run): exact in binary
                ids = np.asarray(run_ids, dtype=np.int64).reshape(-1)
                return np.ones((ids.size, self.n, comps)) * (self.serial + salt / 16.0 + ids[:, None, None] / 4096.0)

            def sensors(self, name, run_ids):
                x = self._fill(run_ids, 3, {'accel': 1, 'gyro': 2, 'odo': 3}[name])
                return x[:, :, 0] if name == 'odo' else x

            def trajectories(self, algo, run_ids, displacement=False):
                return tuple(self._fill(run_ids, 3, 4 + k + 3 * (algo == 'odo')) * 2.0 ** -8 for k in range(3))

            def series(self, name, run_ids):
                return self._fill(run_ids, 4 if name.startswith('quat_') else 3, 10 + sum(map(ord, name)) % 5)

            def initial_biases(self):
                return np.arange(3.0 * self.runs).reshape(self.runs, 3) / 1024.0 + self.serial

            def process_stats_online(self, algo):
                return np.zeros((self.runs, 3, 9)) + self.serial

            def process_stats(self, algo, first_sample=0, pos_ned=False):
                rec.log.append(['process_stats', self.name, algo, int(first_sample), bool(pos_ned)])
                return np.zeros((self.runs, 3, 9)) + self.serial

            def stats(self, algo, ned=False):
                return ginsim.StatsResult.zero()

            def stats_from_traj(self, algo, pos_ned=False):
                rec.log.append(['stats_from_traj', self.name, algo, bool(pos_ned)])
                return ginsim.StatsResult.zero()

        kinds = {c: type(c, (Job,), {'cls': c}) for c in real}
        monkeypatch.setattr(ginsim, 'default_context', lambda: Ctx(0, 'main'))
        monkeypatch.setattr(ginsim, 'Context', Ctx)
        for c in ('MonteCarloJob', 'InclinometerJob', 'AuxSensorJob'):
            monkeypatch.setattr(ginsim, c, kinds[c])
        for c in ('JobSet', 'AuxJobSet'):
            monkeypatch.setattr(multi, c, kinds[c])
        monkeypatch.setattr(multi, 'DeviceSet', DevSet)
        monkeypatch.setattr(ins_sim.Sim, '_SIBLINGS', {})
        monkeypatch.setenv('GPU_MAX_HW_QUEUES', '4')
        for k in ('GINSIM_DEVICES', 'GINSIM_PLACED', 'GNSS_INS_SIM_REFERENCE') + ins_sim.Sim._RANK_ENV:
            monkeypatch.delenv(k, raising=False)


# ------------------------------------------------------------------------------------------------ the cases
class Hosted(object):
    """A plugin outside the kernels: the reference's per-run loop calls it on host copies."""
    input, output = ['fs', 'gyro'], ['wb']

    def run(self, set_of_input):
        self.res = [np.full(3, float(np.asarray(set_of_input[1])[0, 0]))]

    def get_results(self):
        return self.res

    def reset(self):
        pass


class OnDevice(Hosted):
    """A plugin that takes the device-resident sensor series of all runs at once."""
    output = ['ab']

    def run_device(self, job, fs):
        self.seen = (job.name, fs)
        return [[np.full(3, float(k))] for k in range(job.runs)]


def _imu(**kw):
    from gnss_ins_sim.sim import imu_model
    kw.setdefault('gps', False)
    return imu_model.IMU(accuracy='mid-accuracy', axis=kw.pop('axis', 6), **kw)


def _free(ini=0.0, **kw):
    from demo_algorithms import free_integration
    return free_integration.FreeIntegration(np.zeros(9) + ini, **kw)


def _odo(ini=0.0):
    from demo_algorithms import free_integration_odo
    return free_integration_odo.FreeIntegration(np.zeros(9) + ini)


def _mahony():
    from demo_algorithms import inclinometer_device
    return inclinometer_device.MahonyFilter()


def _tilt():
    from demo_algorithms import inclinometer_device
    return inclinometer_device.TiltAcc()


ODO = dict(odo=True, odo_opt={'scale': 0.999, 'stdv': 0.1})
STATS = dict(keep_trajectories=False)
PER_RUN = 1000 * (48 + 72)          # bytes of one kept run of turn_90deg at 100 Hz, 6-axis IMU, one fused plugin (n = 1000)

# name -> (runs, IMU options, plugins, Sim options[, (rank, world) of a pretended process group])
CASES = {
    'kept_one_plugin': (8, {}, lambda: _free(), {}),
    'kept_free_and_odo_one_group': (8, ODO, lambda: [_free(), _odo()], {}),
    'kept_two_groups': (8, {}, lambda: [_free(), _free(1e-3)], {}),
    'kept_earth_rot_off': (4, {}, lambda: _free(earth_rot=False), {'ref_frame': 0}),
    'stats_online': (1000, ODO, lambda: [_free(), _odo()], dict(STATS, stats_start=2.0)),
    'stats_end_point_only': (1000, ODO, lambda: [_free(), _odo()], dict(STATS, stats_start=-1)),
    'stats_rf0_end_ned': (1000, {}, lambda: _free(), dict(STATS, ref_frame=0)),
    'ride_one_kind': (1000, {}, lambda: _free(), dict(STATS, keep_runs=2)),
    'ride_two_kinds_online': (700, ODO, lambda: [_free(), _odo()], dict(STATS, keep_runs=2, ref_frame=0)),
    'ride_two_kinds_end_point': (700, ODO, lambda: [_free(), _odo()], dict(STATS, keep_runs=2, stats_start=-1)),
    'ride_refused_by_budget': (1000, {}, lambda: _free(), dict(STATS, keep_runs=2, max_device_bytes=256 * PER_RUN - 1)),
    'keep_runs_300_small_launch': (1000, {}, lambda: _free(), dict(STATS, keep_runs=300)),
    'placed_false_keep_runs_2': (1000, {}, lambda: _free(), dict(STATS, keep_runs=2, placed=False)),
    'placed_true_keep_runs_2': (1000, {}, lambda: _free(), dict(STATS, keep_runs=2, placed=True)),
    'placed_false_f32_keep_runs_3': (600, {}, lambda: _free(), dict(STATS, keep_runs=3, placed=False, precision='f32', max_device_bytes=2 ** 20)),
    'placed_true_f32_keep_runs_3': (600, {}, lambda: _free(), dict(STATS, keep_runs=3, placed=True, precision='f32', max_device_bytes=2 ** 20)),
    'placed_false_kept': (8, {}, lambda: _free(), dict(placed=False)),
    'no_algorithm': (3, ODO, lambda: None, dict(placed=True, precision='f32')),
    'no_algorithm_stats_only': (3, {}, lambda: None, dict(STATS)),
    'gps_and_magnetometer': (4, dict(axis=9, gps=True), lambda: _free(), dict(geo_mag_n=[20.0, 1.0, 40.0])),
    'env_random_and_sinusoidal': (8, {}, lambda: _free(), dict(env={'acc': '[0.03 0.001 0.01]-random', 'gyro': '[6 5 4]d-0.5Hz-sinusoidal'})),
    'auto_keeps_at_the_budget': (8, {}, lambda: _free(), dict(keep_trajectories='auto', max_device_bytes=8 * PER_RUN)),
    'auto_drops_a_byte_below': (8, {}, lambda: _free(), dict(keep_trajectories='auto', max_device_bytes=8 * PER_RUN - 1)),
    'two_contexts_on_one_gpu': (9, dict(axis=9, gps=True), lambda: _free(), dict(devices=[0, 0], geo_mag_n=[20.0, 1.0, 40.0])),
    'two_contexts_stats_keep_runs': (1000, {}, lambda: _free(), dict(STATS, devices=[0, 0], keep_runs=2)),
    'two_contexts_no_algorithm': (3, {}, lambda: None, dict(devices=[0, 0])),
    'rank_1_of_4': (1000, {}, lambda: _free(), dict(STATS, keep_runs=2), (1, 4)),
    'rank_1_of_4_kept_no_algorithm': (10, {}, lambda: None, {}, (1, 4)),
    'rank_without_runs': (2, {}, lambda: _free(), dict(STATS, keep_runs=1), (3, 4)),
    'inclinometers_kept': (8, {}, lambda: [_mahony(), _tilt()], {}),
    'inclinometers_stats_keep_runs': (300, {}, lambda: [_mahony(), _tilt()], dict(STATS, keep_runs=2)),
    'inclinometers_stats_last_run_job': (300, {}, lambda: [_mahony(), _tilt()], dict(STATS, stats_start=-1)),
    'inclinometers_next_to_fused': (300, {}, lambda: [_mahony(), _tilt(), _free()], dict(STATS, keep_runs=2)),
    'two_mahony_one_tilt_kept': (5, {}, lambda: [_free(), _mahony(), _mahony(), _tilt()], dict(placed=False)),
    'tilt_alone_all_kept_by_keep_runs': (4, {}, lambda: _tilt(), dict(STATS, keep_runs=4)),
    'hosted_plugin': (3, {}, lambda: [_free(), Hosted()], {}),
    'hosted_run_device_plugin': (3, {}, lambda: [OnDevice(), Hosted()], {}),
    'second_run_continues_run_times': (4, {}, lambda: _free(), {}),
}

REFUSALS = {
    'no_imu': (1, None, lambda: _free(), {}),
    'odo_plugin_without_odometer': (1, {}, lambda: _odo(), {}),
    'hosted_needs_kept_series': (1, {}, lambda: Hosted(), dict(STATS)),
    'inclinometer_f32': (1, {}, lambda: _mahony(), dict(precision='f32')),
    'inclinometer_process_group': (4, {}, lambda: _mahony(), {}, (1, 4)),
    'inclinometer_devices': (4, {}, lambda: _tilt(), dict(devices=[0, 0])),
    'psd_f32': (1, {}, lambda: None, dict(precision='f32', env={'acc': np.array([[0.0, 1e-4, 1e-4, 1e-4], [40.0, 1e-4, 1e-4, 1e-4]])})),
    'devices_process_group': (4, {}, lambda: _free(), dict(devices=[0, 0]), (1, 4)),
    'nine_axis_without_field': (1, dict(axis=9), lambda: _free(), {}),
}


def _sim(case, monkeypatch):
    from gnss_ins_sim.sim import ins_sim
    runs, imu, algos, opts = case[:4]
    opts = dict({'ref_frame': 1, 'seed': 7}, **opts)
    if len(case) > 4:       # a stand-in for torch.distributed: this process is rank r of w
        r, w = case[4]
        monkeypatch.setattr(ins_sim.Sim, '_dist', staticmethod(lambda: (r, w, 'group', 'xdev')))
        monkeypatch.setattr(ins_sim.Sim, '_pick_seed', lambda self, group, dev: 1234567)
    sim = ins_sim.Sim([100.0, 10.0, 10.0], CSV, imu=None if imu is None else _imu(**imu), algorithm=algos(), **opts)
    return sim, runs


def _after_run(sim, rec, name):
    from gnss_ins_sim.sim.sim_data import McSeries, ChainSeries
    d, log = sim.dmgr, rec.log
    log.append(['available', sorted(d.available)])
    for nm in sorted(d.available):
        x = d.get_data_all(nm)._data
        kind = next((k for k, t in (('McSeries', McSeries), ('ChainSeries', ChainSeries), ('dict', dict), ('array', np.ndarray))
                     if isinstance(x, t)), type(x).__name__)
        row = ['series', nm, kind]
        if kind in ('McSeries', 'ChainSeries', 'dict'):
            keys = list(x.keys())
            row += [len(x)] + ([keys[0], keys[-1], digest(np.round(x[keys[0]], 6)), digest(np.round(x[keys[-1]], 6))] if keys else [])
        elif kind == 'array':
            row.append(list(x.shape))
        log.append(row)
    algos = sim.amgr.algo or []
    log.append(['sim', sim.kept, getattr(sim, 'passes', None), sim.placement, getattr(sim._side_ctx, 'name', None),
                [getattr(a, 'run_times', None) for a in algos], [digest(getattr(a, 'gyro_bias', None)) for a in algos],
                [getattr(a, 'seen', None) for a in algos]])
    mc = sim.mc
    if mc is None:
        return
    jobname = lambda j: None if j is None else getattr(j, 'name', None) or [type(j).__name__, j.block.name, j.rest.name]
    log.append(['mc', mc.kept_block, mc.devices, mc.exchange, mc.algo_names, mc.kinds, mc.fused_names, mc.first_run, mc.runs_local,
                mc.total_runs, [jobname(j) for j in mc.jobs], [jobname(j) for j in mc.kept]])
    # statistics over ANOTHER window than the one run() accumulated: the jobs that are built on demand
    log.append(['process_stats', sorted(mc.process_stats('att_euler', 50, ned=False)['max'].keys())[:3]])
    if mc.fused_names:
        log.append(['process_stats ned', len(mc.process_stats('pos', 50, ned=True)['std'])])
    if sim.precision == 'f32':
        for nm in mc.fused_names:
            log.append(['end_stats ned', nm, mc.end_stats(nm, ned=True).count])


def trace(name, monkeypatch):
    rec = Recorder(monkeypatch)
    if name in REFUSALS:
        sim, runs = _sim(REFUSALS[name], monkeypatch)
        with pytest.raises(Exception) as e:
            sim.run(runs)
        rec.log.append(['refused', type(e.value).__name__, str(e.value)])
    else:
        sim, runs = _sim(CASES[name], monkeypatch)
        sim.run(runs)
        if name == 'second_run_continues_run_times':
            sim.run(runs)
        _after_run(sim, rec, name)
    return json.loads(json.dumps(rec.log))


def test_fixture_lists_every_case(monkeypatch):
    """GINSIM_RECORD_TRACE=1: write the fixture (at the commit it characterises, once); otherwise only check it is complete."""
    if os.environ.get('GINSIM_RECORD_TRACE') == '1':
        out = {}
        for name in list(CASES) + list(REFUSALS):
            with monkeypatch.context() as m:
                out[name] = trace(name, m)
        with open(FIXTURE, 'w') as f:
            f.write('{\n' + ',\n'.join('%s: [\n%s\n]' % (json.dumps(k), ',\n'.join(json.dumps(r) for r in v)) for k, v in out.items()) + '\n}\n')
    with open(FIXTURE) as f:
        assert sorted(json.load(f)) == sorted(list(CASES) + list(REFUSALS))


@pytest.mark.parametrize('name', list(CASES) + list(REFUSALS))
def test_driver_builds_launches_and_publishes_as_recorded(name, monkeypatch):
    with open(FIXTURE) as f:
        want = json.load(f)[name]
    got = trace(name, monkeypatch)
    for k, (a, b) in enumerate(zip(got, want)):
        assert a == b, 'record %d of %s' % (k, name)
    assert len(got) == len(want)


# ------------------------------------------------------------------------------------------------ the plan, directly
def _plan(imu, algos, runs=1000, n=1000, gps_rows=0, rank=0, world=1, in_group=False, ndev=1, asked=None, **opts):
    """plan_monte_carlo for a Sim of `runs` runs over n samples at 100 Hz; no device, no recorder."""
    from gnss_ins_sim.sim import ins_sim
    sim = ins_sim.Sim([100.0, 10.0, 10.0], CSV, imu=_imu(**imu), algorithm=algos, **dict({'ref_frame': 1, 'seed': 7}, **opts))
    sim.sim_count = runs
    algos = sim.amgr.algo or []

    def place(work, distributed):
        if asked is not None:
            asked.append((work, distributed))
        return ndev > 1, ndev
    roles = ins_sim._plugin_roles(sim, [getattr(a, 'mc_algo', None) for a in algos])
    return ins_sim.plan_monte_carlo(sim, algos, roles, np.arange(n) / 100.0, gps_rows, rank, world, in_group, place)


def test_plan_bytes_per_sample_of_every_sensor_and_plugin():
    """48 (accel + gyro) + 8 (odometer) + 72 per fused plugin + 24 (magnetometer) + 48 x GPS rows / n + 104 per MahonyFilter
    + 56 per TiltAcc."""
    assert _plan({}, None).per_sample == 48
    assert _plan({}, _free()).per_sample == 120
    assert _plan(ODO, [_free(), _odo()]).per_sample == 200
    assert _plan(ODO, None).per_sample == 56
    assert _plan(dict(axis=9, gps=True), _free(), gps_rows=100, geo_mag_n=[20.0, 1.0, 40.0]).per_sample == 148.8
    assert _plan(dict(axis=9), None, gps_rows=100, geo_mag_n=[20.0, 1.0, 40.0]).per_sample == 72      # no GPS: its rows do not count
    assert _plan({}, [_mahony(), _tilt()]).per_sample == 208
    assert _plan({}, [_mahony(), _tilt(), _free()]).per_sample == 280
    assert _plan({}, [_tilt()]).per_sample == 104


@pytest.mark.parametrize('split, largest', [({}, 1000), (dict(world=4, rank=2, in_group=True), 250), (dict(ndev=2), 500),
                                            (dict(world=3, rank=2, in_group=True), 334)])
def test_plan_auto_keeps_when_the_largest_share_fits_exactly(split, largest):
    """'auto' is decided on rank 0's share (the largest), divided over the devices: kept at per_sample * n * largest bytes, not
    one byte below -- the same answer on every rank."""
    need = 120 * 1000 * largest
    assert _plan({}, _free(), keep_trajectories='auto', max_device_bytes=need, **split).keep is True
    assert _plan({}, _free(), keep_trajectories='auto', max_device_bytes=need - 1, **split).keep is False


def test_plan_shares_and_kept_counts():
    p = _plan({}, _free(), world=4, rank=1, in_group=True, keep_trajectories=False, keep_runs=2)
    assert (p.first, p.count, p.kcount, p.keep) == (250, 250, 2, False)
    p = _plan({}, _free(), runs=1002, world=4, rank=3, in_group=True)
    assert (p.first, p.count, p.kcount, p.keep) == (752, 250, 250, True)
    p = _plan({}, _free(), runs=2, world=4, rank=3, in_group=True, keep_trajectories=False, keep_runs=1)
    assert (p.first, p.count, p.kcount) == (2, 0, 0)
    assert _plan({}, _free(), keep_trajectories=False, keep_runs=5000).kcount == 1000


@pytest.mark.parametrize('precision, ndev, budget, want', [('f64', 1, 2 ** 36, 954368), ('f32', 1, 2 ** 36, 1908736), ('f64', 2, 2 ** 36, 1908736),
                                                           ('f32', 2, 2 ** 36, 3817472), ('f64', 1, 2 ** 20, 256), ('f32', 2, 2 ** 20, 512)])
def test_plan_block_runs(precision, ndev, budget, want):
    """Runs per block of a re-integration with trajectories kept: 9 components of 4 or 8 bytes per sample within the budget, in
    whole workgroups of 256 runs and at least one, on every device."""
    assert _plan({}, _free(), precision=precision, ndev=ndev, max_device_bytes=budget, keep_trajectories=False).block_runs == want


def test_plan_kept_runs_ride_only_where_the_block_fits_and_one_context_integrates(monkeypatch):
    from gnss_ins_sim.sim import ins_sim
    ride = lambda **kw: _plan({}, _free(), **dict(dict(keep_trajectories=False, keep_runs=2), **kw)).ride
    assert ride() is True
    assert ride(max_device_bytes=120 * 1000 * 256) is True              # the block of 256 runs with everything kept fits exactly
    assert ride(max_device_bytes=120 * 1000 * 256 - 1) is False
    assert ride(keep_runs=256) is True and ride(keep_runs=257) is False and ride(keep_runs=0) is False
    assert ride(runs=257) is True and ride(runs=256) is False           # there must be a rest
    assert ride(precision='f32') is False
    assert ride(ndev=2) is False
    assert ride(world=2, in_group=True) is False
    assert ride(keep_trajectories=True) is False
    monkeypatch.setattr(ins_sim, 'KEPT_BLOCK', 10 ** 9)                 # read from the module when the plan is made
    assert ride() is False


def test_plan_what_the_statistics_launches_accumulate():
    stats = lambda **kw: _plan({}, _free(), keep_trajectories=False, **kw)
    p = stats(stats_start=2.0)
    assert (p.online, p.end_ned, p.proc_first) == (True, False, 200)
    p = stats(stats_start=-1, ref_frame=0)
    assert (p.online, p.end_ned, p.proc_first) == (False, True, 0)
    p = stats(stats_start=1e9)                                          # beyond the end: the first sample, as the data manager does
    assert (p.online, p.proc_first) == (True, 0)
    p = stats(precision='f32', ref_frame=0)
    assert (p.online, p.end_ned) == (False, False)
    p = _plan({}, _free(), ref_frame=0, stats_start=2.0)                # everything kept: nothing is accumulated online
    assert (p.online, p.end_ned, p.proc_first) == (False, False, 0)
    assert _plan({}, [_mahony()], stats_start=2.0).proc_first == 200    # the inclinometer kernel always takes the window


def test_plan_launch_groups_and_roles():
    p = _plan(ODO, [_free(), Hosted(), _odo(), _free(1e-3), _tilt(), _free()])
    assert (p.fused, p.incl, p.hosted) == ([0, 2, 3, 5], [4], [1])
    assert [(g.kinds, g.idx, g.first, g.earth_rot) for g in p.groups] == [(['free', 'odo'], [0, 2], 0, True), (['free'], [3], 0, True),
                                                                          (['free'], [5], 0, True)]
    assert float(np.ravel(p.groups[1].ini)[0]) == 1e-3


def test_plan_asks_for_the_devices_between_the_two_chain_refusals():
    asked = []
    with pytest.raises(ValueError, match='does not cross torch.distributed ranks'):
        _plan({}, [_mahony()], world=2, in_group=True, asked=asked)
    assert asked == []
    with pytest.raises(ValueError, match='does not cross devices'):
        _plan({}, [_mahony()], ndev=2, asked=asked)
    assert asked == [(0, False)]                                        # an inclinometer chain is never spread automatically
    del asked[:]
    _plan({}, _free(), runs=70, n=500, asked=asked)
    assert asked == [(70 * 500, False)]
