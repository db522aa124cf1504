"""Inputs shared by the MBAR tests (tests/test_mbar_config.py on the CPU, tests/mbar_gpu_worker.py on the GPU): small seeded cases,
the stressed cases of the fixed-iteration check and the calls the entry point refuses."""
import numpy as np

STATE_TILE = 128      # UPK_MBAR_STATE_TILE of include/upside_hip_kernels.h (the worker checks it against the library)
FE_TILE = 4           # UPK_MBAR_FE_TILE
TWO_PI = 2. * np.pi


def small_case(seed=3, K=4, n=40, d=1):
    rng = np.random.RandomState(seed)
    centers = np.linspace(-1., 1., K)
    v = np.concatenate([rng.normal(c, 0.5, n) for c in centers]).astype('f4')[:, None]
    if d == 2:
        v = np.column_stack((v[:, 0], rng.normal(0., 1., len(v)))).astype('f4')
    rows = np.zeros((K, 3 * d), 'f4')
    rows[:, 0] = centers; rows[:, d:2 * d] = 2.0
    return dict(values=v, energy=None, beta=np.full(K, 1.0), rows=rows, n_k=np.full(K, n, 'i8'), periods=np.zeros(d))


# ---- the entry point's refusals: before any device call, so they are the same with and without a GPU ------------------------------
def refusal_cases():
    """(label, keyword changes to a good call, fragment of the message)"""
    good = small_case(K=3, n=10)
    bad_rows_k = good['rows'].copy(); bad_rows_k[1, 1] = -1.
    bad_rows_w = good['rows'].copy(); bad_rows_w[2, 2] = -0.5
    nan_rows = good['rows'].copy(); nan_rows[0, 0] = np.nan
    nan_v = good['values'].copy(); nan_v[7, 0] = np.inf
    nine = dict(values=np.zeros((30, 9), 'f4'), rows=np.zeros((3, 27), 'f4'), periods=np.zeros(9))
    return good, [
        ('d above 8', nine, 'at most 8'),
        ('no state has samples', dict(n_k=np.zeros(3, 'i8')), 'no state has samples'),
        ('counts do not add up', dict(n_k=np.array([10, 10, 9], 'i8')), 'add up'),
        ('counts exceed', dict(n_k=np.array([10, 10, 11], 'i8')), 'add up'),
        ('a negative count', dict(n_k=np.array([20, -1, 11], 'i8')), 'negative'),
        ('spring_const below 0', dict(rows=bad_rows_k), 'spring_const'),
        ('flat_width below 0', dict(rows=bad_rows_w), 'flat_width'),
        ('a row entry is not finite', dict(rows=nan_rows), 'not finite'),
        ('a value is not finite', dict(values=nan_v), 'not finite'),
        ('an energy is not finite', dict(energy=np.where(np.arange(30) == 3, np.nan, 0.)), 'energy[3]'),
        ('a beta is not finite', dict(beta=np.array([1., np.inf, 1.])), 'beta[1]'),
        ('a period is not finite', dict(periods=np.array([np.nan])), 'periods[0]'),
        ('a negative period', dict(periods=np.array([-1.])), 'negative'),
        ('f0 is not finite', dict(f0=np.array([0., np.nan, 0.])), 'f0[1]'),
        ('the target is not finite', dict(target=(np.inf, None)), 'target'),
        ('the target row is negative', dict(target=(1., np.array([0., -1., 0.], 'f4'))), 'target'),
        ('tol below 0', dict(tol=-1.), 'tol'),
        ('no iteration', dict(max_iter=0), 'max_iter'),
    ]


# ---- the fixed-iteration check ----------------------------------------------------------------------------------------------------
FIXED_N = (1, 255, 256, 257, 1000)
FIXED_K = (1, 2, FE_TILE - 1, FE_TILE, FE_TILE + 1, STATE_TILE - 1, STATE_TILE, STATE_TILE + 1)
FIXED_D = (0, 1, 2, 8)


def stressed_case(N, K, d, seed):
    """one case of the fixed-iteration check.  Counts are unequal (a seeded multinomial) and two states are given N_k = 0 (one for K = 3, none
    below; the draw leaves further states empty).  d = 0: energies and K different beta.  d > 0: CV 0 is periodic (2 pi) for d >= 2 with centres
    cycling through +3.0, -3.0, +1.0, -1.0 and samples wrapped into (-pi, pi], so they lie on both sides of the cut; the flat
    bottoms cycle through 0 (no sample inside), 0.3 (some) and 100 (all); with d = 2 an energy and unequal beta come on top; the
    last state (K >= 2) has spring_const 1e6 on its last CV: its reduced energies reach 1e5 and beyond."""
    rng = np.random.RandomState(seed)
    active = np.ones(K, bool)
    n_zero = 0 if K < 3 else (1 if K == 3 else 2)
    if n_zero:
        active[rng.choice(K, n_zero, replace=False)] = False
    p = rng.dirichlet(np.full(int(active.sum()), 0.7))
    n_k = np.zeros(K, 'i8'); n_k[active] = rng.multinomial(N, p)
    if d == 0:
        return dict(values=None, energy=rng.normal(-40., 6., N), beta=np.linspace(0.9, 1.7, K) if K > 1 else np.array([1.1]), rows=None,
                    n_k=n_k, periods=None)
    owner = rng.randint(0, K, N)
    centers = np.zeros((K, d)); spring = np.zeros((K, d)); flat = np.zeros((K, d))
    for c in range(d):
        if c == 0 and d >= 2:
            centers[:, c] = np.array([3.0, -3.0, 1.0, -1.0])[np.arange(K) % 4]
        else:
            centers[:, c] = 5. + 0.02 * np.arange(K) + 0.3 * c + rng.normal(0., 0.2, K)
        spring[:, c] = rng.uniform(1., 6., K)
        flat[:, c] = np.array([0., 0.3, 100.])[(np.arange(K) + c) % 3]
    if K >= 2:
        spring[K - 1, d - 1] = 1e6; flat[K - 1, d - 1] = 0.
    v = centers[owner] + rng.normal(0., 0.6, (N, d))
    periods = np.zeros(d)
    if d >= 2:
        periods[0] = TWO_PI
        v[:, 0] = v[:, 0] - TWO_PI * np.rint(v[:, 0] / TWO_PI)
    rows = np.concatenate((centers, spring, flat), axis=1).astype('f4')
    energy, beta = None, np.full(K, 1.25)
    if d == 2:
        energy = rng.normal(-20., 3., N); beta = np.linspace(1.0, 1.5, K) if K > 1 else np.array([1.2])
    return dict(values=v.astype('f4'), energy=energy, beta=beta, rows=rows, n_k=n_k, periods=periods)


def temperature_case(seed=21):
    """six temperatures, seeded energies, unequal counts"""
    rng = np.random.RandomState(seed)
    T = np.array([0.70, 0.76, 0.83, 0.90, 0.98, 1.07])
    n_k = np.array([300, 250, 260, 240, 200, 250], 'i8')
    energy = np.concatenate([rng.normal(-120. + 90. * (t - 0.7), 4.5, n) for t, n in zip(T, n_k)])
    return dict(values=None, energy=energy, beta=1. / T, rows=None, n_k=n_k, periods=None)
