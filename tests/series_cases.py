"""Inputs of the series checks (tests/test_series_config.py without a GPU, tests/series_gpu_worker.py with one): seeded and small."""
import numpy as np
import series_reference as R

PARITY_T = (16, 63, 64, 65, 257, 1000, 4099)
PARITY_N_SERIES = (1, 3, 65)
PHIS = (0., 0.5, 0.9, 0.98)
C_MARGIN = 1e-6      # the smallest |C(t)| a case may show where the stop is decided: the device's C(t) is within 1e-9 of the yardstick's
GAP = 1e-3           # the smallest relative gap between the best and the second-best n_eff where the chosen origin is compared
# (T, series) whose first seed fails a margin condition take the seed listed here instead; found once with the yardstick alone
SEED_REPLACED = {(63, 36): 109}      # seed 9: the two best of the 8 origins lie 1.3e-4 apart


def parity_series(T, k):
    """series k of the parity batches of length T: AR(1) with phi = PHIS[k % 4] from RandomState(1000 seed + T + int(100 phi)),
    seed = k // 4 unless replaced"""
    phi = PHIS[k % 4]
    seed = SEED_REPLACED.get((T, k), k // 4)
    return R.ar1(np.random.RandomState(1000 * seed + T + int(100 * phi)), T, phi)[0]


def parity_batch(T, n_series=65):
    return np.stack([parity_series(T, k) for k in range(n_series)])


def parity_origins(T, n_origin):
    return np.array([0], 'i8') if n_origin == 1 else (T // 8) * np.arange(8, dtype='i8')


def unequal_batch():
    """(series (5, 1000), lengths): what lies past a length is NaN and must never be read"""
    a = parity_batch(1000, 5)
    n = np.array([1000, 999, 513, 64, 17], 'i8')
    for k in range(5):
        a[k, n[k]:] = np.nan
    return a, n


def white_series(T=4096, seed=10):
    """stationary white noise whose first three correlations happen to sum below 0, so that g = 1 at origin 0 (seed 10: the smallest
    |C(t)| where a stop is decided is 2.3e-2 and the best origin leads by 1.6e-2)"""
    return np.random.RandomState(seed).normal(size=T)


def drift_series(T=2048, seed=5, phi=0.5):
    """a start-up drift of five sigma that decays over T / 8 on an AR(1) series of unit variance"""
    x = R.ar1(np.random.RandomState(seed), T, phi)[0]
    return x + 5. * np.exp(-np.arange(T) / (T / 8.))


# ---- the entry point's refusals: before any device call, so they are the same with and without a GPU ------------------------------
def refusal_cases(a):
    """(label, keyword arguments of statistical_inefficiency, fragment of the message); the worker of the GPU tests walks them too"""
    nan = a.copy(); nan[2, 63] = np.nan
    inf = a.copy(); inf[0, 0] = np.inf
    return [
        ('no series', dict(series=np.zeros((0, 64))), 'at least one series'),
        ('no origin', dict(series=a, origins=()), 'at least one origin'),
        ('a length of 0', dict(series=a, lengths=[64, 0, 64]), 'length[1] = 0'),
        ('a length above stride', dict(series=a, lengths=[64, 64, 65]), 'length[2] = 65'),
        ('a negative origin', dict(series=a, origins=(-1, 4)), 'negative'),
        ('origins that do not ascend', dict(series=a, origins=(0, 8, 8)), 'does not ascend'),
        ('mintime below 1', dict(series=a, mintime=0), 'mintime'),
        ('max_lag below 1', dict(series=a, max_lag=0), 'max_lag'),
        ('an entry that is not a number', dict(series=nan), 'series 2, entry 63 is not finite'),
        ('an entry that is infinite', dict(series=inf), 'series 0, entry 0 is not finite'),
    ]
