"""Hand-built (gyro, accel) records for the inclinometer plugins, from a seed (test infrastructure: the golden's maker
tests/golden/make_golden_inclinometer.py and the tests build the same records with this one function; the golden stores the
first sample of each so that a change of the generator cannot pass unnoticed).

    sphere_batches() -> list of batches; a batch is a dict
        name, fs (the rate handed to MahonyFilter.run: dt = 1 / fs), gains (iref.GAINS keys, or None for the defaults),
        accel, gyro (R, n, 3), groups {group name: run indices within the batch}

The attitudes the DCM of both callers of acc_mag_quat can take have zero yaw: with pitch t and roll p the diagonal is
(cos t, cos p, cos t cos p), cos t >= 0, so dcm2quat's `tr > 0` boundary is the curve (1 + cos t)(1 + cos p) = 1 -- roll between
90 and 120 degrees -- and the accelerometer of such an attitude is -9.8 (-sin t, sin p cos t, cos p cos t).
"""
import numpy as np

SEED = 20261016
G = 9.8
ILL_GROUPS = ('near_x_1e-06', 'near_x_1e-09')       # 1 - ax^2 cancels: the pseudo-magnetometer amplifies the last bit of ax


def _unit(v):
    return v / np.sqrt(np.sum(v * v, axis=-1))[..., None]


def _acc_of(pitch, roll):
    return -G * np.stack([-np.sin(pitch), np.sin(roll) * np.cos(pitch), np.cos(roll) * np.cos(pitch)], axis=-1)


def sphere_batches(seed=SEED):
    rng = np.random.RandomState(seed)
    out = []

    # ---- 1. constant accelerometer directions over the whole sphere, 100 Hz, default gains
    n = 30
    dirs, groups = [], {}

    def add(name, d):
        d = np.asarray(d, dtype=np.float64).reshape(-1, 3)
        first = sum(x.shape[0] for x in dirs)
        groups[name] = np.arange(first, first + d.shape[0])
        dirs.append(d)
    add('axes', G * np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], dtype=np.float64))
    add('sphere', G * _unit(rng.standard_normal((200, 3))))
    for d in (1e-3, 1e-6, 1e-9):
        phi = rng.uniform(0, 2 * np.pi, 4)
        v = [[s * np.cos(d), np.sin(d) * np.cos(p), np.sin(d) * np.sin(p)] for s in (1.0, -1.0) for p in phi]
        add('near_x_%g' % d, G * np.array(v))
    for d in (1e-3, 1e-6, 1e-9):
        roll = np.array([95.0, 105.0, 115.0, -100.0, -110.0, -118.0]) * np.pi / 180
        cp = 1.0 / (1.0 + np.cos(roll)) - 1.0
        pitch = np.arccos(cp) * np.array([1, -1, 1, -1, 1, -1])
        add('tr0_%g' % d, np.concatenate([_acc_of(pitch + d, roll), _acc_of(pitch - d, roll)]))
    accel = np.repeat(np.concatenate(dirs)[:, None, :], n, axis=1)
    gyro = 0.3 * rng.standard_normal(accel.shape)
    quiet = np.concatenate([groups[k] for k in groups if k.startswith(('near_x', 'tr0'))])
    gyro[quiet] *= 0.2                                        # mostly under the 0.2 rad/s of the gain switch
    out.append(dict(name='sphere', fs=100.0, gains=None, accel=accel, gyro=gyro, groups=groups))

    # ---- 2. rates that take cos(theta / 2) below zero (|w + b| dt / 2 past pi / 2), and w + b == 0 exactly
    n, R = 40, 12
    accel = np.repeat((G * _unit(rng.standard_normal((R, 3))))[:, None, :], n, axis=1)
    axis = _unit(rng.standard_normal((R, 1, 3)))
    half = rng.uniform(0.8, 2.6, (R, n))                      # theta / 2 per sample: both sides of pi / 2 in every record
    half[0:4] = np.array([1.2, 1.7, 3.0, 3.3])[:, None]       # constant ones: never / always / always / past pi again
    gyro = axis * (2.0 * half / 0.01)[..., None] + 0.3 * rng.standard_normal((R, n, 3))
    accel[R - 1], gyro[R - 1] = [0.0, 0.0, -G], 0.0           # level, no rate, zero bias: theta == 0
    out.append(dict(name='flip', fs=100.0, gains=None, accel=accel, gyro=gyro,
                    groups={'cneg': np.arange(R - 1), 'theta0': np.array([R - 1])}))

    # ---- 3. records that start with 1, 2 and all samples of zero accelerometer
    n = 30
    base = np.concatenate([G * _unit(rng.standard_normal((2, 3))), _acc_of(np.array([0.3]), np.array([2.5]))])
    accel = np.repeat(np.tile(base, (3, 1))[:, None, :], n, axis=1)
    for k, z in enumerate((1, 2, n)):
        accel[3 * k:3 * k + 3, :z] = 0.0
    gyro = 0.1 * rng.standard_normal(accel.shape)
    out.append(dict(name='zero_acc', fs=100.0, gains=None, accel=accel, gyro=gyro,
                    groups={'zero_1': np.arange(0, 3), 'zero_2': np.arange(3, 6), 'zero_all': np.arange(6, 9)}))

    # ---- 4. norms on both sides of the gain switch and of the innovation limit; other gains, 50 Hz
    n, R = 60, 16
    d0 = _unit(rng.standard_normal((R, 3)))
    perp = _unit(np.cross(d0, rng.standard_normal((R, 3))))
    ang = 0.004 * rng.standard_normal((R, n))
    ang[:, 20:40] += 0.3                                      # the direction jumps by 0.3 rad and back: innovation past the limit
    d = d0[:, None, :] * np.cos(ang)[..., None] + perp[:, None, :] * np.sin(ang)[..., None]
    accel = d * (G + rng.choice([-0.21, -0.19, 0.19, 0.21, 0.0], (R, n)))[..., None]
    gyro = _unit(rng.standard_normal((R, n, 3))) * rng.choice([0.19, 0.21, 0.05], (R, n))[..., None]
    gains = dict(kp_high=2.0, kp_low=0.05, ki_high=0.2, ki_low=0.004, innovation_limit=0.03)
    out.append(dict(name='gains', fs=50.0, gains=gains, accel=accel, gyro=gyro, groups={'switch': np.arange(R)}))
    return out


WRAP_VALUES = np.array([np.pi, -np.pi, 3 * np.pi, -3 * np.pi,
                        np.nextafter(np.pi, 0), np.nextafter(np.pi, 4), np.nextafter(-np.pi, 0), np.nextafter(-np.pi, -4),
                        np.nextafter(3 * np.pi, 0), np.nextafter(3 * np.pi, 10), np.nextafter(-3 * np.pi, 0), np.nextafter(-3 * np.pi, -10),
                        0.0, np.pi - 1e-9, -(np.pi - 1e-9)])
