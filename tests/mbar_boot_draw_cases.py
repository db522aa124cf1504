"""Inputs shared by the tests of the device draw of the MBAR bootstrap counts (tests/test_mbar_boot_draw_config.py on the CPU,
tests/mbar_boot_draw_gpu_worker.py on the GPU): the shapes of the equality check and the calls the two new entry points refuse
(upside_hip_mbar_bootstrap_drawn, upside_hip_mbar_bootstrap_counts).  Every refusal returns before any device call, so they are the
same with and without a GPU."""
import ctypes as ct
import numpy as np
import mbar_bootstrap_cases as C

T = 8192               # UPK_MBAR_BOOT_DRAW_TILE: up to T samples a state is counted in LDS, above by global atomics
SEED = (1 << 40) + 3
DRAW_N_K = (0, 1, 2, 255, 256, 257, 1000, T - 1, T, T + 1, 2 * T + 3)
DRAW_BLOCKS = (None, 7, (1, 1, 2, 3, 256, 300, 64, T, T + 5, 2, 10 ** 6))


def shuffled_origins(n_k, seed=11):
    return np.random.RandomState(seed).permutation(C.grouped_origins(n_k)).astype('i4')


def ar1(n, phi, rng, burn=500):
    """(n,) an AR(1) series x_i = phi x_{i-1} + e_i, e standard normal, after `burn` steps"""
    e = rng.normal(size=n + burn)
    x = np.zeros(n + burn)
    for i in range(1, n + burn):
        x[i] = phi * x[i - 1] + e[i]
    return x[burn:]


# ---- mbar.bootstrap(draw='device'): everything upside_hip_mbar_bootstrap refuses apart from what concerns counts, and the blocks ------
def drawn_refusal_cases():
    """(good keyword arguments of mbar.bootstrap, [(label, keyword changes, fragment of the message)])"""
    good, cases = C.boot_refusal_cases()
    good = dict(good, draw='device', n_bootstrap=2, seed=5)
    del good['counts']
    kept = [c for c in cases if 'counts' not in c[1]]
    assert len(kept) == len(cases) - 2      # 'no replicate' and 'a replicate that does not add up' concern counts
    kept += [
        ('no replicate', dict(n_bootstrap=0), 'at least one replicate'),
        ('a negative number of replicates', dict(n_bootstrap=-3), 'n_replicate = -3'),
        ('a block of no sample', dict(block=0), 'block[0] = 0'),
        ('a negative block of one state', dict(block=np.array([1, -2, 1])), 'block[1] = -2'),
    ]
    return good, kept


_DRAWN_ORDER = ('n_sample', 'n_state', 'd', 'values', 'energy', 'beta', 'rows', 'n_k', 'periods', 'state_of_sample', 'n_replicate', 'seed', 'block',
                'counts_out', 'tol', 'max_iter', 'f0', 'n_column', 'log_numerator', 'f_boot', 'column_boot', 'n_iter', 'last_delta')


def raw_drawn(calc, good, **override):
    """upside_hip_mbar_bootstrap_drawn itself on the good call with some arguments replaced: (rc, message)"""
    v = np.ascontiguousarray(good['values'], 'f4'); N, d = v.shape
    n_k = np.ascontiguousarray(good['n_k'], 'i8'); K = len(n_k)
    beta = np.ascontiguousarray(good['beta'], 'f8'); rows = np.ascontiguousarray(good['rows'], 'f4'); per = np.ascontiguousarray(good['periods'], 'f8')
    sos = C.grouped_origins(n_k)
    f_boot = np.zeros((2, K)); cols = np.zeros((2, 2)); ln = np.zeros((2, N))
    a = dict(n_sample=N, n_state=K, d=d, values=v.ctypes.data, energy=None, beta=beta.ctypes.data, rows=rows.ctypes.data, n_k=n_k.ctypes.data,
             periods=per.ctypes.data, state_of_sample=sos.ctypes.data, n_replicate=2, seed=5, block=None, counts_out=None, tol=0., max_iter=3, f0=None,
             n_column=0, log_numerator=None, f_boot=f_boot.ctypes.data, column_boot=cols.ctypes.data, n_iter=None, last_delta=None)
    if override.pop('with_columns', False):
        a.update(n_column=2, log_numerator=ln.ctypes.data)
    a.update(override)
    vp, i32, i64, u64, f64 = ct.c_void_p, ct.c_int, ct.c_longlong, ct.c_ulonglong, ct.c_double
    calc.upside_hip_mbar_bootstrap_drawn.argtypes = [i64, i32, i32, vp, vp, vp, vp, vp, vp, vp, i32, u64, vp, vp, f64, i32, vp, i32, vp, vp, vp, vp, vp]
    calc.upside_hip_mbar_bootstrap_drawn.restype = i32
    calc.upside_hip_last_error.restype = ct.c_char_p
    rc = calc.upside_hip_mbar_bootstrap_drawn(*[a[k] for k in _DRAWN_ORDER])
    return rc, calc.upside_hip_last_error().decode()


RAW_DRAWN_REFUSALS = [
    ('state_of_sample missing', dict(state_of_sample=None), 'state_of_sample must be given'),
    ('n_replicate below 1', dict(n_replicate=0), 'at least one replicate'),
    ('n_column below 0', dict(n_column=-1), 'n_column = -1 is negative'),
    ('columns without log_numerator', dict(with_columns=True, log_numerator=None), 'log_numerator and column_boot must be given'),
    ('f_boot missing', dict(f_boot=None), 'f_boot must be given'),
    ('N x K at 2^62', dict(n_sample=1 << 61), '2^62'),
]

# ---- mbar.bootstrap_counts_device --------------------------------------------------------------------------------------------------
COUNTS_GOOD = dict(n_k=np.array([10, 0, 12, 8], 'i8'), n_bootstrap=3, seed=SEED, block=np.array([2, 1, 5, 100]), first=4)
COUNTS_REFUSALS = [
    ('no replicate', dict(n_bootstrap=0), 'at least one replicate'),
    ('a negative first replicate', dict(first=-1), 'first_replicate = -1'),
    ('a first replicate at 2^32', dict(first=1 << 32), 'first_replicate = 4294967296'),
    ('replicates that reach 2^32', dict(first=(1 << 32) - 2), 'a replicate index must stay below 2^32'),
    ('a block of no sample', dict(block=0), 'block[0] = 0'),
    ('a negative block of an empty state', dict(block=np.array([2, -1, 5, 100])), 'block[1] = -1'),
    ('a negative n_k', dict(n_k=np.array([10, -1, 12, 8], 'i8'), state_of_sample=np.zeros(29, 'i4')), 'n_k[1] = -1 is negative'),
    ('a state index above K - 1', dict(state_of_sample=np.where(np.arange(30) == 29, 4, np.repeat([0, 2, 3], [10, 12, 8]))), 'state_of_sample[29] = 4 is outside 0 .. 3'),
    ('an origin without samples', dict(state_of_sample=np.where(np.arange(30) == 3, 1, np.repeat([0, 2, 3], [10, 12, 8]))), 'names a state without samples'),
    ('origins that do not add up', dict(state_of_sample=np.repeat([0, 2, 3], [11, 11, 8])), 'names state 0 for 11 samples'),
]


def raw_counts(calc, **override):
    """upside_hip_mbar_bootstrap_counts itself on a good call with some arguments replaced: (rc, message)"""
    n_k = np.array([10, 0, 12, 8], 'i8'); out = np.zeros((3, 30), 'u2')
    a = dict(n_state=4, n_k=n_k.ctypes.data, n_sample=30, state_of_sample=None, n_replicate=3, first_replicate=0, seed=1, block=None, counts_out=out.ctypes.data)
    a.update(override)
    vp, i32, i64, u64 = ct.c_void_p, ct.c_int, ct.c_longlong, ct.c_ulonglong
    calc.upside_hip_mbar_bootstrap_counts.argtypes = [i32, vp, i64, vp, i64, i64, u64, vp, vp]
    calc.upside_hip_mbar_bootstrap_counts.restype = i32
    calc.upside_hip_last_error.restype = ct.c_char_p
    order = ('n_state', 'n_k', 'n_sample', 'state_of_sample', 'n_replicate', 'first_replicate', 'seed', 'block', 'counts_out')
    rc = calc.upside_hip_mbar_bootstrap_counts(*[a[k] for k in order])
    return rc, calc.upside_hip_last_error().decode()


_BIG = np.array([(1 << 26) + 1], 'i8')
RAW_COUNTS_REFUSALS = [
    ('no state', dict(n_state=0), 'at least one state'),
    ('no sample', dict(n_sample=0), 'at least one sample'),
    ('n_k missing', dict(n_k=None), 'n_k and counts_out must be given'),
    ('counts_out missing', dict(counts_out=None), 'n_k and counts_out must be given'),
    ('n_k below n_sample', dict(n_sample=31), 'add up to 30, n_sample is 31'),
    ('n_k above n_sample', dict(n_sample=29), 'add up to more than n_sample = 29'),
    ('a negative number of replicates', dict(n_replicate=-2), 'n_replicate = -2'),
    ('2^32 replicates', dict(n_replicate=1 << 32), 'a replicate index must stay below 2^32'),
    ('more than 2^26 samples', dict(n_state=1, n_k=_BIG.ctypes.data, n_sample=(1 << 26) + 1), 'at most 2^26 samples'),
]
