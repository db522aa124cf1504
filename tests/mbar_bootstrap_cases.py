"""Inputs shared by the tests of the MBAR bootstrap (tests/test_mbar_bootstrap_config.py on the CPU, tests/mbar_bootstrap_gpu_worker.py
on the GPU): the replicates of the fixed-iteration check, the count-range case, profile columns and the calls the entry point
refuses."""
import ctypes as ct
import numpy as np
import mbar_reference as M
from mbar_cases import small_case, refusal_cases

BOUND = 1e-9          # |gpu - f64| <= BOUND max(1, |f64|): the bound of tests/test_gpu_mbar.py, both sides fp64
TOL = 1e-10           # the tolerance of the convergence checks
N_BOOT = 100          # their replicates, counts from default_rng(BOOT_SEED)
BOOT_SEED = 5
SIGMA_RATIO = (0.65, 1.5)   # bootstrap over asymptotic sigma: 0.88 .. 1.24 measured on the yardstick, widened by 3 / sqrt(2 x 100)


def grouped_origins(n_k):
    return np.repeat(np.arange(len(n_k), dtype='i4'), np.asarray(n_k, 'i8'))


def fixed_counts(n_k, seed):
    """(5, N) uint16 for samples grouped by state: all ones; three seeded stratified draws; one degenerate replicate with each state's
    whole count on a single sample of the state"""
    n_k = np.asarray(n_k, 'i8')
    N = int(n_k.sum())
    rng = np.random.default_rng(seed)
    start = np.concatenate(([0], np.cumsum(n_k)))
    out = np.zeros((5, N), 'u2')
    out[0] = 1
    for k in range(len(n_k)):
        m = int(n_k[k])
        if not m:
            continue
        for b in (1, 2, 3):
            out[b, start[k]:start[k + 1]] = np.bincount(rng.integers(0, m, m), minlength=m)
        out[4, start[k] + rng.integers(0, m)] = m
    return out


def repeated(case, c):
    """the case with sample n physically repeated c[n] times (in place, so the samples stay grouped by state)"""
    c = np.asarray(c, 'i8')
    out = dict(case)
    if case['values'] is not None:
        out['values'] = np.repeat(case['values'], c, axis=0)
    if case['energy'] is not None:
        out['energy'] = np.repeat(case['energy'], c)
    return out


def count_range_case(seed=31):
    """K = 2 with n_k = [66000, 10] (d = 1): (case, counts (2, N)) -- replicate 0 all ones; replicate 1 holds 65535 on one sample of
    state 0 and 465 on another, ones on state 1"""
    rng = np.random.RandomState(seed)
    n_k = np.array([66000, 10], 'i8')
    v = np.concatenate((rng.normal(0.0, 0.5, 66000), rng.normal(0.8, 0.5, 10))).astype('f4')[:, None]
    rows = np.array([[0.0, 2.0, 0.0], [0.8, 2.0, 0.0]], 'f4')
    case = dict(values=v, energy=None, beta=np.full(2, 1.0), rows=rows, n_k=n_k, periods=np.zeros(1))
    counts = np.ones((2, 66010), 'u2')
    counts[1, :66000] = 0
    counts[1, 17] = 65535; counts[1, 40001] = 465
    return case, counts


def profile_columns(case, edges, cv=0, beta_t=None):
    """(columns (n_bin, N), bin (N,)): per bin of edges along CV `cv`, -u_target(n) inside the bin and -inf outside, for the unbiased
    target at beta_t (default the case's first beta)"""
    x = case['values'][:, cv].astype('f8')
    beta_t = float(case['beta'][0]) if beta_t is None else beta_t
    e = np.zeros(len(x)) if case['energy'] is None else np.asarray(case['energy'], 'f8')
    b = np.searchsorted(edges, x, 'right') - 1
    b[(x < edges[0]) | (x >= edges[-1])] = -1
    cols = np.full((len(edges) - 1, len(x)), -np.inf)
    for j in range(len(edges) - 1):
        cols[j, b == j] = -beta_t * e[b == j]
    return cols, b


def converged_start(case):
    """the full-sample solution the convergence checks start from: the yardstick converged to TOL"""
    return M.mbar(tol=TOL, max_iter=5000, **case)['f']


# ---- the entry point's refusals: before any device call, so they are the same with and without a GPU ------------------------------
def boot_refusal_cases():
    """(good keyword arguments of mbar.bootstrap, [(label, keyword changes, fragment of the message)])"""
    base, shared = refusal_cases()
    good = dict(base, f=None, counts=np.ones((2, 30), 'u2'), tol=0., max_iter=3)
    cases = []
    for label, change, fragment in shared:      # everything upside_hip_mbar refuses about the problem (it has no target)
        if 'target' in change:
            continue
        change = dict(change)
        if 'f0' in change:
            change['f'] = change.pop('f0')
        if 'n_k' in change:      # counts and origins that match the changed n_k where that is possible: the n_k are what is refused
            change['state_of_sample'] = np.repeat(np.arange(3), 10).astype('i4')
        cases.append((label, change, fragment))
    moved = np.ones((2, 30), 'u2'); moved[1, 0] = 2; moved[1, 10] = 0
    nan_col = np.zeros((2, 30)); nan_col[1, 29] = np.nan
    inf_col = np.full((2, 30), -np.inf); inf_col[0, 3] = np.inf
    cases += [
        ('no replicate', dict(counts=np.zeros((0, 30), 'u2')), 'at least one replicate'),
        ('a state index above K - 1', dict(state_of_sample=np.where(np.arange(30) == 29, 3, np.repeat(np.arange(3), 10))), 'state_of_sample[29] = 3 is outside 0 .. 2'),
        ('a negative state index', dict(state_of_sample=np.where(np.arange(30) == 4, -1, np.repeat(np.arange(3), 10))), 'state_of_sample[4] = -1'),
        ('an origin without samples', dict(n_k=np.array([15, 15, 0], 'i8'), state_of_sample=np.array([0] * 15 + [1] * 14 + [2])), 'names a state without samples'),
        ('origins that do not add up', dict(state_of_sample=np.array([0] * 11 + [1] * 9 + [2] * 10)), 'names state 0 for 11 samples'),
        ('a replicate that does not add up', dict(counts=moved), 'replicate 1: the counts of state 0 add up to 11'),
        ('a column entry is not a number', dict(log_numerators=nan_col), 'column 1, sample 29 is not a number'),
        ('a column entry is +inf', dict(log_numerators=inf_col), 'column 0, sample 3 is +inf'),
        ('a workspace below one replicate', dict(workspace_bytes=8 * 30 - 1), 'do not fit the workspace'),
        ('a workspace above the limit', dict(workspace_bytes=(512 << 20) + 1), 'at most'),
    ]
    return good, cases


def raw_call(calc, good, **override):
    """upside_hip_mbar_bootstrap itself on the good call with some arguments replaced (for what mbar.bootstrap cannot be told:
    NULL arrays, a negative n_column): (rc, message)"""
    v = np.ascontiguousarray(good['values'], 'f4'); N, d = v.shape
    n_k = np.ascontiguousarray(good['n_k'], 'i8'); K = len(n_k)
    beta = np.ascontiguousarray(good['beta'], 'f8'); rows = np.ascontiguousarray(good['rows'], 'f4'); per = np.ascontiguousarray(good['periods'], 'f8')
    sos = grouped_origins(n_k); counts = np.ascontiguousarray(good['counts'], 'u2')
    f_boot = np.zeros((len(counts), K)); cols = np.zeros((len(counts), 2)); ln = np.zeros((2, N))
    a = dict(n_sample=N, n_state=K, d=d, values=v.ctypes.data, energy=None, beta=beta.ctypes.data, rows=rows.ctypes.data, n_k=n_k.ctypes.data,
             periods=per.ctypes.data, state_of_sample=sos.ctypes.data, n_replicate=len(counts), counts=counts.ctypes.data, tol=0., max_iter=3, f0=None,
             n_column=0, log_numerator=None, f_boot=f_boot.ctypes.data, column_boot=cols.ctypes.data, n_iter=None, last_delta=None)
    if override.pop('with_columns', False):
        a.update(n_column=2, log_numerator=ln.ctypes.data)
    a.update(override)
    vp, i32, i64, f64 = ct.c_void_p, ct.c_int, ct.c_longlong, ct.c_double
    calc.upside_hip_mbar_bootstrap.argtypes = [i64, i32, i32, vp, vp, vp, vp, vp, vp, vp, i32, vp, f64, i32, vp, i32, vp, vp, vp, vp, vp]
    calc.upside_hip_mbar_bootstrap.restype = i32
    calc.upside_hip_last_error.restype = ct.c_char_p
    order = ('n_sample', 'n_state', 'd', 'values', 'energy', 'beta', 'rows', 'n_k', 'periods', 'state_of_sample', 'n_replicate', 'counts', 'tol',
             'max_iter', 'f0', 'n_column', 'log_numerator', 'f_boot', 'column_boot', 'n_iter', 'last_delta')
    rc = calc.upside_hip_mbar_bootstrap(*[a[k] for k in order])
    return rc, calc.upside_hip_last_error().decode()


RAW_REFUSALS = [
    ('counts missing', dict(counts=None), 'counts and state_of_sample must be given'),
    ('state_of_sample missing', dict(state_of_sample=None), 'counts and state_of_sample must be given'),
    ('n_replicate below 1', dict(n_replicate=0), 'at least one replicate'),
    ('n_column below 0', dict(n_column=-1), 'n_column = -1 is negative'),
    ('columns without log_numerator', dict(with_columns=True, log_numerator=None), 'log_numerator and column_boot must be given'),
    ('f_boot missing', dict(f_boot=None), 'f_boot must be given'),
    ('N x K at 2^62', dict(n_sample=1 << 61), '2^62'),
]
