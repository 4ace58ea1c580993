"""Placed arena integrity (csrc/placed.hip): every live region -- carved from the arena or hipMalloc'ed -- holds exactly its own
bytes through carves, frees, growths (searches), a second context's exit and a rebuild of the arena.

The arena works around three behaviours of the driver's virtual-memory API (the header of csrc/placed.hip): an address
unmapped and mapped to another chunk can keep translating to the old one, and a freed reservation's addresses come back with
their stale translations.  A miss in that protocol does not fail a launch; it silently writes one region's data into another.
So every region here is filled with a pattern unique to (tag, word offset) -- ginsim_pattern_fill, ABI 9 -- and after every
event ALL live regions are checked on the device (ginsim_pattern_check): a word that is wrong names where it came from.
The helpers themselves are held to the NumPy statement of both formulas (oracle/pattern.py), and a deliberate overlap of two
views shows that the check sees an alias.  Then the real Monte-Carlo kernels run on placed planes in the same churned arena,
and finally two threads use two contexts of the device at once."""
import ctypes as C
import gc
import threading

import numpy as np
import pytest

from conftest import ang_close
from oracle import pattern as pat

pytestmark = pytest.mark.gpu

MiB, G = 1 << 20, 1 << 30
STRIPE = 512 * MiB
# A bounded search, below the library's 200 GiB: this module forces a dozen searches.  Not much lower: the driver can hand out
# chunks of one class of physical memory for a long stretch, and the searches recorded in DESIGN 4.1 held 12-140 GiB before every
# class had its share.  A search that runs out of budget first refuses the request and turns placement off for the context.
BUDGET = 160 * G


@pytest.fixture(scope='module')
def ctx():
    """A context whose device starts with no arena, searches with a bounded budget, and gets the default options back."""
    import ginsim
    from ginsim import _lib
    c = ginsim.Context(0)
    gc.collect()                        # jobs of earlier modules in reference cycles hold arena regions until collected
    for other in [o for o in gc.get_objects() if isinstance(o, ginsim.Context) and o.handle]:
        other.sync()
        other.release_pool()            # contexts earlier modules left alive (Sim's default and sibling contexts) park hipMalloc'ed
                                        # regions in their pools: give them back, so that the searches here see the device's memory
    assert c.placed_info()['mapped_bytes'] == 0, _why(c)
    opts = _lib.PlacedOptions(stripe_bytes=STRIPE, budget_bytes=BUDGET, limit_bytes=0, search_seconds=0.0)
    assert ginsim.lib.ginsim_placed_configure(c.handle, C.byref(opts)) == 0, ginsim.lib.ginsim_last_error()
    yield c
    gc.collect()
    c.sync()
    c.release_pool()
    rc = ginsim.lib.ginsim_placed_configure(c.handle, C.byref(_lib.PlacedOptions()))
    msg = ginsim.lib.ginsim_last_error()
    c.close()
    assert rc == 0, msg


def _why(ctx):
    """What a failed placement assertion prints: the context's note (why the arena refused), the device's free memory, the arena."""
    info = ctx.placed_info()
    return 'note %r; device free %.1f GiB; arena %s' % (ctx.placed_note, ctx.mem_info()[0] / G, {k: info[k] for k in (
        'mapped_bytes', 'used_bytes', 'searches', 'failed', 'stripes_of_class', 'chunks_created', 'chunks_ambiguous', 'last_search_seconds')})


def _searches(ctx):
    return ctx.placed_info()['searches']


def _h2d(ctx, ptr, words):
    import ginsim
    words = np.ascontiguousarray(words, dtype=np.uint64)
    ginsim._lib.check(ginsim.lib.ginsim_memcpy_h2d(ctx.handle, ptr, words.ctypes.data, words.nbytes))


def _what(word, owners):
    """A found word, decoded: which tag / region and word it is, or the fill that left it."""
    word = int(word)
    if word == 0:
        return '0 (a zero fill)'
    b = word & 0xFF
    if word == int.from_bytes(bytes([b]) * 8, 'little'):
        return '%#x (a memset of byte %#x)' % (word, b)
    tag, i = pat.decode(word)
    return '%#x = word %d (byte +%#x) of tag %#x (%s)' % (word, i, 8 * i, tag, owners.get(tag, 'no live region'))


# ------------------------------------------------------------------------------------------------------------- a. the helpers
@pytest.mark.parametrize('nbytes', [8, 4096 + 8, 3 * MiB + 24, 64 * MiB])
def test_pattern_and_digest_match_the_numpy_statement(ctx, nbytes):
    """Every word of a fill equals the mirror, the fill stays inside its region, and both digests agree bit for bit."""
    guard = 4096
    buf = ctx.malloc(nbytes + guard)
    try:
        ctx.pattern_fill(buf, nbytes + guard, 0x5A5)
        ctx.pattern_fill(buf, nbytes, 0x1234)
        got = ctx.download(buf, (nbytes // 8,), dtype=np.uint64)
        want = pat.pattern(0x1234, nbytes // 8)
        np.testing.assert_array_equal(got, want)
        # the words behind the region still hold the fill before it: nothing was written past `nbytes`
        np.testing.assert_array_equal(ctx.download(buf.at(nbytes), (guard // 8,), dtype=np.uint64),
                                      pat.pattern(0x5A5, guard // 8, first=nbytes // 8))
        assert ctx.pattern_check(buf, nbytes, 0x1234) == (0, -1, 0)
        assert ctx.digest(buf, nbytes) == pat.digest(want)
        assert ctx.digest(buf, nbytes + guard) == pat.digest(np.concatenate([want, pat.pattern(0x5A5, guard // 8, nbytes // 8)]))
        # random words (every bit pattern, not only pattern words)
        rnd = np.random.default_rng(nbytes).integers(0, 2 ** 64, size=nbytes // 8, dtype=np.uint64)
        _h2d(ctx, buf.ptr, rnd)
        assert ctx.digest(buf, nbytes) == pat.digest(rnd)
        bad, first, found = ctx.pattern_check(buf, nbytes, 0x1234)
        mismatch = np.flatnonzero(rnd != want)
        assert bad == mismatch.size and first == 8 * mismatch[0] and found == int(rnd[mismatch[0]])
    finally:
        buf.free(pool=False)


def test_the_check_sees_an_alias(ctx):
    """Positive control: a second view overlapping the last N words of a region is filled with another tag.  The check of the
    first tag reports exactly those N words, at the overlap's offset, holding the other tag's first word; a memset is named as
    one.  (Nothing is aliased for real: two views of one carved region.)"""
    size, n_over = 8 * MiB, 1000
    r = ctx.malloc(size + 2 * MiB, placed=True)
    assert r.placed, ctx.placed_note
    try:
        ta, tb = 0xA11, 0xB22
        ctx.pattern_fill(r, size, ta)
        assert ctx.pattern_check(r, size, ta) == (0, -1, 0)
        view, view_bytes = r.at(size - 8 * n_over), 8 * n_over + MiB
        ctx.pattern_fill(view, view_bytes, tb)
        bad, first, found = ctx.pattern_check(r, size, ta)
        assert (bad, first) == (n_over, size - 8 * n_over), (bad, first)
        assert pat.decode(found) == (tb, 0), _what(found, {ta: 'first', tb: 'second'})
        assert ctx.pattern_check(view, view_bytes, tb) == (0, -1, 0)
        # a memset over one 4 KiB window in front of the overlap: named as a repeated byte, at its own offset
        import ginsim
        assert ginsim.lib.ginsim_memset(ctx.handle, r.at(64 * 1024), 0xA5, 4096) == 0
        bad, first, found = ctx.pattern_check(r, size, ta)
        assert (bad, first, found) == (n_over + 512, 64 * 1024, 0xA5A5A5A5A5A5A5A5), (bad, first, hex(found))
    finally:
        r.free()


# ------------------------------------------------------------------------------------------------------------- b. the churn
class _Region(object):
    def __init__(self, name, buf, nbytes):
        self.name, self.buf, self.nbytes, self.ptr = name, buf, int(nbytes), buf.ptr
        self.tag = None
        self.windows = []           # (byte offset, bytes, tag) written by host copies over the kernel's fill


class _Ledger(object):
    """Every live region with the tag of its last fill.  check() runs the device check on ALL of them."""

    def __init__(self, ctx):
        self.ctx, self.live, self.owners, self._tag = ctx, {}, {}, 0x100

    def fresh_tag(self, name):
        self._tag += 1
        self.owners[self._tag] = name
        return self._tag

    def carve(self, name, nbytes, placed=True, ctx=None):
        ctx = ctx or self.ctx
        buf = ctx.malloc(nbytes, placed=placed)
        assert buf.placed == placed, (name, _why(ctx))
        r = self.live[name] = _Region(name, buf, nbytes)
        r.ctx = ctx
        self.fill(r)
        return r

    def fill(self, r):
        r.tag, r.windows = self.fresh_tag(r.name), []
        r.ctx.pattern_fill(r.ptr, r.nbytes, r.tag)

    def host_window(self, r, off, nbytes):
        """Host copy of a fresh tag's pattern (word 0 at `off`) over part of the region; read back by a download at once."""
        tag = self.fresh_tag('%s window +%#x' % (r.name, off))
        words = pat.pattern(tag, nbytes // 8)
        _h2d(self.ctx, r.ptr + off, words)
        np.testing.assert_array_equal(self.ctx.download(r.ptr + off, words.shape, dtype=np.uint64), words)
        r.windows.append((off, nbytes, tag))

    def drop(self, name, pool=True):
        r = self.live.pop(name)
        r.buf.free(pool=pool)           # placed: back to the arena's free list whatever `pool` says
        return r

    def check(self, event):
        """After `event`: every live region holds its tag's pattern except its host windows, which hold theirs; the kernel-written
        head and tail also read back right through a download."""
        for r in self.live.values():
            where = '%s: region %r (%s, %#x, %d bytes, tag %#x)' % (event, r.name, 'placed' if r.buf.placed else 'plain', r.ptr, r.nbytes, r.tag)
            bad, first, found = self.ctx.pattern_check(r.ptr, r.nbytes, r.tag)
            want_bad = sum(nb // 8 for _, nb, _ in r.windows)
            want_first = min(off for off, _, _ in r.windows) if r.windows else -1
            assert (bad, first) == (want_bad, want_first), '%s: %d bad words (expected %d), the first at byte +%#x holds %s' % (
                where, bad, want_bad, first, _what(found, self.owners))
            for off, nb, tag in r.windows:
                bad, first, found = self.ctx.pattern_check(r.ptr + off, nb, tag)
                assert bad == 0, '%s: host window +%#x: %d bad words, the first at +%#x holds %s' % (where, off, bad, first, _what(found, self.owners))
            covered = [(off, off + nb) for off, nb, _ in r.windows]
            for off in sorted({0, max(0, (r.nbytes - 4096) // 8 * 8)}):
                nb = min(4096, r.nbytes - off)
                if any(a < off + nb and off < b for a, b in covered):
                    continue
                got = self.ctx.download(r.ptr + off, (nb // 8,), dtype=np.uint64)
                np.testing.assert_array_equal(got, pat.pattern(r.tag, nb // 8, first=off // 8), err_msg=where + ' download +%#x' % off)


def _force_growth(ledger, name, extra=0):
    """Carve a region larger than all the free space of the arena (and `extra` more: room another thread may free meanwhile):
    the arena must grow, which is a search."""
    ctx = ledger.ctx
    info = ctx.placed_info()
    s0 = info['searches']
    r = ledger.carve(name, info['mapped_bytes'] - info['used_bytes'] + extra + STRIPE + 8)
    assert ctx.placed_info()['searches'] >= s0 + 1, (s0, ctx.placed_info())
    return r


def test_live_regions_keep_their_bytes_through_growth_handback_and_rebuild(ctx):
    import ginsim
    ledger = _Ledger(ctx)
    sizes = {'sub': 37 * MiB + 8, 'one': STRIPE, 'one_half': 3 * STRIPE // 2, 'five': 5 * STRIPE + 3 * MiB + 40}
    for cycle in range(3):
        c = 'c%d ' % cycle
        # 1. regions of mixed sizes, filled by the kernel; windows written by host copies; two plain regions
        s0 = _searches(ctx)
        assert ctx.placed_reserve(sum(sizes.values())), ctx.placed_note
        for k, nb in sizes.items():
            ledger.carve(c + k, nb)
        assert _searches(ctx) >= s0 + (1 if cycle == 0 else 0)
        five, half = ledger.live[c + 'five'], ledger.live[c + 'one_half']
        for off, nb in ((0, 4096), (STRIPE - 4096, 8192), (3 * STRIPE + 40, 24 * 1024), (five.nbytes - 4096 - 8, 4096 + 8)):
            ledger.host_window(five, off, nb)
        ledger.host_window(half, STRIPE - 1024, 2048)
        ledger.carve(c + 'plain_a', 64 * MiB + 8, placed=False)
        ledger.carve(c + 'plain_b', 3 * MiB + 24, placed=False)
        ledger.check(c + 'carve')
        # 2. a middle region freed; a different size carved into its hole
        hole = ledger.drop(c + 'one').ptr
        r = ledger.carve(c + 'in_hole', 300 * MiB + 16)
        assert hole <= r.ptr < hole + STRIPE, (hex(hole), hex(r.ptr))
        ledger.check(c + 'carve into a hole')
        # 3. a growth while everything is live; nothing between it and the check touches hipMalloc / hipFree (a plain free
        # flushes the translations by itself and would hide a missing flush in the library)
        _force_growth(ledger, c + 'grown')
        ledger.check(c + 'growth')
        # 4. a plain region parked in the context's pool, taken back, filled again
        p = ledger.carve(c + 'pooled', 48 * MiB, placed=False)
        ptr = p.ptr
        ledger.drop(c + 'pooled')
        p = ledger.carve(c + 'pooled', 48 * MiB, placed=False)
        assert p.ptr == ptr
        ledger.check(c + 'pool round trip')
        # 5. a second context carves, fills and closes without freeing: its region returns to the free list
        other = ginsim.Context(0)
        try:
            o = ledger.carve(c + 'other', 200 * MiB + 8, ctx=other)       # filled on the other context's stream
            ledger.check(c + 'second context carved')
            other_ptr = o.ptr
            ledger.live.pop(c + 'other')
        finally:
            other.close()
        r = ledger.carve(c + 'after_other', 200 * MiB + 8)
        assert r.ptr == other_ptr, (hex(r.ptr), hex(other_ptr))
        ledger.check(c + 'second context closed')
        # 6. every placed region freed and the arena given back; plain regions stay live (and more are made while no arena
        # exists); then the arena is rebuilt -- freed reservation addresses come back here, stale translations included
        for name in [k for k, r in ledger.live.items() if r.buf.placed]:
            ledger.drop(name)
        ctx.release_pool()
        assert ctx.placed_info()['mapped_bytes'] == 0, ctx.placed_info()
        ledger.check(c + 'arena given back')
        ledger.carve(c + 'plain_no_arena', 96 * MiB + 8, placed=False)
        ledger.carve(c + 'plain_stripe', STRIPE, placed=False)
        ledger.check(c + 'plain regions without an arena')
        s0 = _searches(ctx)
        ledger.carve(c + 'rebuilt', 2 * STRIPE + 5 * MiB + 8)
        assert _searches(ctx) == s0 + 1 and ctx.placed_info()['mapped_bytes'] > 0
        ledger.check(c + 'rebuild')
    for name in list(ledger.live):
        ledger.drop(name, pool=False)
    assert ctx.placed_info()['used_bytes'] == 0


# ------------------------------------------------------------------------------------------------------------- c. real planes
def _blocks(R, width=88):
    """first / middle / last block (as test_gpu_full_size): ragged starts put wavefront and workgroup edges inside"""
    return [(0, width), (R // 2 - width // 2 - 5, width), (R - width, width)]


def _digests(job):
    """Digest of each plane group a launch wrote: exactly 3 n runs 8 bytes each, not the region's rounding."""
    ctx, per = job.ctx, 3 * job.n * job.runs * 8
    out = {}
    if job.keep_sensors:
        for k in ('accel', 'gyro'):
            out[k] = ctx.digest(job.buffer(k).ptr, per)
    if job.keep_traj:
        for a in job.algos:
            base = job.buffer('traj_' + a).ptr
            for q, part in enumerate(('att', 'pos', 'vel')):
                out['%s_%s' % (a, part)] = ctx.digest(base + q * per, per)
    return out


def _c2_job(ctx, placed, runs=65536):
    import ginsim
    from ginsim import workloads
    ini, truth, _ = workloads.truth_from_profile('turn_90deg', 100.0, 1)
    acc, gyr = workloads.imu_grade('mid-accuracy')
    return ginsim.MonteCarloJob(ctx, 100.0, 1, truth, acc, gyr, ini, runs=runs, seed=20261016, keep_sensors=True,
                                keep_traj=True, placed=placed)


def test_real_kernels_on_placed_planes_after_the_churn(ctx):
    import ginsim
    from ginsim import workloads
    from oracle import c_oracle
    fs, R = 100.0, 65536
    job = _c2_job(ctx, True).run()
    assert job.placement()['placed'] == ['imu', 'traj_free'], _why(ctx)
    assert 15 * job.n * R * 8 > 14 * STRIPE
    ini, truth, _ = workloads.truth_from_profile('turn_90deg', fs, 1)
    acc, gyr = workloads.imu_grade('mid-accuracy')
    dev_end = job.end_errors('free')
    for first, count in _blocks(R):          # the planes are [c][n][runs]: every sampled run touches every stripe of every plane
        ids = np.arange(first, first + count)
        end, traj, sens = c_oracle.mc_run(20261016, first, count, fs, 1, truth, acc, gyr, ini, keep=count)
        att, pos, vel = job.trajectories('free', ids)
        d_att = np.abs(np.mod(att - traj[:, :, 0:3] + np.pi, 2 * np.pi) - np.pi).max()
        d_pos = np.abs(pos - traj[:, :, 3:6]).max()
        d_vel = np.abs(vel - traj[:, :, 6:9]).max()
        d_acc = np.abs(job.sensors('accel', ids) - sens[:, :, 0:3]).max()
        d_gyr = np.abs(job.sensors('gyro', ids) - sens[:, :, 3:6]).max()
        assert d_att <= 1e-9 and d_vel <= 1e-9 and d_pos <= 2e-8, (first, d_att, d_pos, d_vel)
        assert d_acc <= 1e-12 and d_gyr <= 1e-14, (first, d_acc, d_gyr)
        assert ang_close(dev_end[ids, :3], end[:, :3], 1e-9)
        np.testing.assert_allclose(dev_end[ids, 3:6], end[:, 3:6], rtol=0, atol=2e-8)
        np.testing.assert_allclose(dev_end[ids, 6:9], end[:, 6:9], rtol=0, atol=1e-9)
    dig = _digests(job)
    assert len(dig) == 5 and len(set(dig.values())) == 5

    # a second live placed job: ref_frame 0, both algorithms
    R2, odo_err = 16384, {'scale': 0.999, 'stdv': 0.1}
    ini0, truth0, _ = workloads.truth_from_profile('turn_90deg', fs, 0)
    job2 = ginsim.MonteCarloJob(ctx, fs, 0, truth0, acc, gyr, ini0, runs=R2, algos=('free', 'odo'), odo_err=odo_err, seed=77,
                                keep_sensors=True, keep_traj=True, placed=True).run()
    assert job2.placement()['placed'] == ['imu', 'odo', 'traj_free', 'traj_odo'], _why(ctx)
    for algo in ('free', 'odo'):
        dev = job2.end_errors(algo)
        for first, count in _blocks(R2, width=40):
            ids = np.arange(first, first + count)
            end, _, sens = c_oracle.mc_run(77, first, count, fs, 0, truth0, acc, gyr, ini0, algo=algo, odo_err=odo_err, keep=count)
            assert ang_close(dev[ids, :3], end[:, :3], 1e-9), (algo, first)
            np.testing.assert_allclose(dev[ids, 3:5], end[:, 3:5], rtol=0, atol=1e-12)
            np.testing.assert_allclose(dev[ids, 5], end[:, 5], rtol=0, atol=1e-9 * max(1.0, np.abs(end[:, 5]).max()))
            np.testing.assert_allclose(dev[ids, 6:9], end[:, 6:9], rtol=0, atol=1e-9)
            if algo == 'free':
                assert np.abs(job2.sensors('accel', ids) - sens[:, :, 0:3]).max() <= 1e-12
                assert np.abs(job2.sensors('gyro', ids) - sens[:, :, 3:6]).max() <= 1e-14
    assert _digests(job) == dig, 'a second job changed the planes of the first'

    # free the second job; force a growth; a given-sensor job reads the first job's placed accel / gyro planes
    job2.release()
    assert _digests(job) == dig, 'freeing the second job changed the planes of the first'
    ledger = _Ledger(ctx)
    _force_growth(ledger, 'grown next to the planes')
    ledger.check('growth next to live planes')
    assert _digests(job) == dig, 'a growth changed the planes of the first job'
    rep = ginsim.MonteCarloJob(ctx, fs, 1, truth, None, None, ini, runs=R, keep_traj=True, placed=True,
                               given={'gyro': job.buffer('gyro'), 'accel': job.buffer('accel')}).run()
    assert rep.placement()['placed'] == ['traj_free'], _why(ctx)
    np.testing.assert_array_equal(rep.end_errors('free'), dev_end)
    assert _digests(job) == dig, 'the given-sensor job changed the planes it read'
    ledger.check('given-sensor job')
    rep.release()
    ledger.drop('grown next to the planes')

    # the same job on hipMalloc planes: the same bytes
    plain = _c2_job(ctx, False).run()
    assert plain.placement()['placed'] == []
    assert _digests(plain) == dig
    plain.release()
    job.release()
    ctx.release_pool()


# ------------------------------------------------------------------------------------------------------------- d. two threads
def test_two_contexts_on_two_threads(ctx):
    """Thread A runs one seeded placed job four times on this context; thread B, on a second context of the device, carves,
    forces a growth, fills, checks and frees at the same time.  A's planes must be the same bytes every time (and those of
    hipMalloc planes); B's regions must hold theirs."""
    import ginsim
    R = 16384
    plain = _c2_job(ctx, False, runs=R).run()
    want = _digests(plain)
    plain.release()
    ctx.release_pool()
    other = ginsim.Context(0)
    start = threading.Barrier(2, timeout=120)
    a_digests, errors = [], []

    def thread_a():
        try:
            start.wait()
            for _ in range(4):
                job = _c2_job(ctx, True, runs=R).run()
                assert job.placement()['placed'] == ['imu', 'traj_free'], _why(ctx)
                a_digests.append(_digests(job))
                job.release()
        except BaseException as e:      # reported by the main thread
            errors.append(('A', e))

    def thread_b():
        try:
            ledger = _Ledger(other)
            start.wait()
            for i in range(3):
                ledger.carve('b%d small' % i, 300 * MiB + 8)
                if i == 0:          # larger than anything thread A can free meanwhile (its job is under 2 GiB)
                    _force_growth(ledger, 'b%d grown' % i, extra=3 * G)
                else:
                    ledger.carve('b%d large' % i, 3 * STRIPE + 8)
                ledger.check('thread B round %d' % i)
                for name in list(ledger.live):
                    ledger.drop(name)
        except BaseException as e:
            errors.append(('B', e))

    threads = [threading.Thread(target=thread_a, name='A', daemon=True), threading.Thread(target=thread_b, name='B', daemon=True)]
    try:
        for t in threads:
            t.start()
        for t in threads:
            t.join(timeout=600)
        hung = [t.name for t in threads if t.is_alive()]
        if hung:
            pytest.fail('thread(s) %s still running after 600 s' % hung)
        if errors:
            who, e = errors[0]
            raise AssertionError('thread %s: %r' % (who, e)) from e
        assert len(a_digests) == 4 and all(d == want for d in a_digests), (want, a_digests)
    finally:
        if not any(t.is_alive() for t in threads):
            other.close()
