"""Inputs shared by the tests of the MBAR Gram pass and the uncertainties (tests/test_mbar_uncertainty_config.py on the CPU,
tests/mbar_uncertainty_gpu_worker.py on the GPU): the stressed shapes and the calls upside_hip_mbar_gram refuses."""
import numpy as np
import mbar_cases as C
import mbar_reference as M

GRAM_TILE = 64            # UPK_MBAR_GRAM_TILE of include/upside_hip_kernels.h (the worker checks it against the library)
GRAM_GRANULE = 32         # UPK_MBAR_GRAM_GRANULE: rows of a slab come in multiples of it
LARGE_ENERGY = 3e5        # the largest reduced energy of the stiff state of gram_case

GRAM_N = (1, 255, 256, 257, 1000)
GRAM_D = (0, 1, 2, 8)
GRAM_EXTRA = (0, 1, 3)


def gram_columns(T=GRAM_TILE):
    return (1, 2, T - 1, T, T + 1, 2 * T + 1)


def gram_case(N, K, d, seed):
    """mbar_cases.stressed_case -- a periodic CV with windows on both sides of the cut (d >= 2), flat bottoms holding none, some and all
    samples, unequal counts with two empty states, the last state stiff -- with the stiff state's spring constant rescaled so that its
    largest reduced energy is LARGE_ENERGY = 3e5 instead of some 5e6.  Why: the entries of W are exp(f_k - u_k(n) - D_n), and where
    a sample sits in the stiff state (with N = 1 it always does) three terms of the size of u cancel.  Each carries half an ulp of
    its size from its own computation, whoever computes it: 3 x 2^-35 = 9e-11 at 3e5, twice that in G -- a fifth of the bound
    1e-9 sqrt(G_kk G_ll) of the check.  At 5e6 one ulp is 9e-10 and two float64 evaluations that differ in the order of a single
    sum are already a bound apart, so nothing could be told there.  The state still has reduced energies above 1e5 wherever a sample
    lies far enough from its centre (the worker asserts it over the shapes of every d > 0).  d = 0, a temperature ladder, has no
    rows and so no stiff state: its reduced energies stay near 1e2."""
    case = C.stressed_case(N, K, d, seed)
    if d and K >= 2:
        v = case['values']
        u = M.reduced_energy(v, case['energy'], case['beta'], case['rows'], case['periods'])[:, K - 1]
        rows = case['rows'].copy()
        rows[K - 1, d + d - 1] = np.float32(rows[K - 1, d + d - 1] * min(1., LARGE_ENERGY / max(float(u.max()), 1e-300)))
        case['rows'] = rows
    return case


def gram_refusal_cases():
    """(label, keyword changes to a good call of mbar.gram, fragment of the message)"""
    good = C.small_case(K=3, n=10)
    good['f'] = np.array([0., 0.1, -0.2])
    good['log_columns'] = np.log(np.full((2, 30), 1. / 30.))
    nan_col = good['log_columns'].copy(); nan_col[1, 29] = np.nan
    inf_col = good['log_columns'].copy(); inf_col[0, 4] = np.inf
    nan_v = good['values'].copy(); nan_v[7, 0] = np.inf
    return good, [
        ('f is not a number', dict(f=np.array([0., np.nan, 0.])), 'f[1] is not finite'),
        ('f is infinite', dict(f=np.array([0., 0., -np.inf])), 'f[2] is not finite'),
        ('a log-column entry is not a number', dict(log_columns=nan_col), 'column 1, sample 29 is not a number'),
        ('a log-column entry is +inf', dict(log_columns=inf_col), 'column 0, sample 4 is +inf'),
        ('more than 8192 columns', dict(log_columns=np.zeros((8190, 30))), 'at most 8192'),
        ('counts do not add up', dict(n_k=np.array([10, 10, 9], 'i8')), 'add up'),
        ('a value is not finite', dict(values=nan_v), 'not finite'),
        ('a negative period', dict(periods=np.array([-1.])), 'negative'),
    ]
