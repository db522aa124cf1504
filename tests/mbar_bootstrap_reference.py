"""Float64 numpy yardstick of the MBAR bootstrap (the statement of upside_hip_mbar_bootstrap in include/upside_engine_c.h), written
from the definitions on top of tests/mbar_reference.py: the whole N x K matrix of reduced energies at once, one replicate after the
other, every logsumexp as max + log(sum(exp(x - max))).  Nothing is shared with csrc/kernels_mbar_boot.hip.  Pinned by
tests/test_mbar_bootstrap_config.py.

    D_b(n)   = logsumexp_{l : N_l > 0} (ln N_l + f_{b,l} - u_l(n))
    f'_{b,k} = -logsumexp_{n : c_b(n) > 0} (ln c_b(n) - u_k(n) - D_b(n)),    f'_b = f'_b - f'_{b,0}
    column_boot[b][j] = -logsumexp_{n : c_b(n) > 0} (ln c_b(n) + log_numerator[j][n] - D_b(n))     (+inf where nothing contributes)
"""
import numpy as np
import mbar_reference as M


def iterate(u, n_k, f, c):
    """one iteration of one replicate with the counts c (N,): (f', D) with D the denominators of the f that went in"""
    c = np.asarray(c)
    D = M.denominators(u, n_k, f)
    keep = c > 0
    fn = -M.logsumexp(np.log(c[keep].astype('f8'))[:, None] - u[keep] - D[keep, None], axis=0)
    return fn - fn[0], D


def columns(u, n_k, f, c, log_numerator):
    """(J,) the columns of one replicate at f"""
    c = np.asarray(c)
    D = M.denominators(u, n_k, f)
    ln = np.asarray(log_numerator, 'f8').reshape(-1, len(u))
    out = np.full(len(ln), np.inf)
    for j in range(len(ln)):
        keep = (c > 0) & (ln[j] > -np.inf)
        if keep.any():
            out[j] = -M.logsumexp(np.log(c[keep].astype('f8')) + ln[j, keep] - D[keep], axis=0)
    return out


def solve(u, n_k, counts, tol, max_iter, f0=None, log_numerator=None):
    """dict(f_boot (B, K), n_iter (B,), last_delta (B,)[, columns (B, J)]) of the replicates counts (B, N), each from f0 (None = 0)"""
    counts = np.asarray(counts).reshape(-1, len(u))
    B, K = len(counts), u.shape[1]
    f_boot = np.zeros((B, K)); n_iter = np.zeros(B, 'i8'); last = np.full(B, np.inf)
    cols = None if log_numerator is None else np.zeros((B, len(np.asarray(log_numerator).reshape(-1, len(u)))))
    for b in range(B):
        f = np.zeros(K) if f0 is None else np.array(f0, 'f8')
        it, delta = 0, np.inf
        while it < max_iter:
            fn, _ = iterate(u, n_k, f, counts[b])
            delta = float(np.abs(fn - f).max())
            f = fn; it += 1
            if delta < tol:
                break
        f_boot[b] = f; n_iter[b] = it; last[b] = delta
        if cols is not None:
            cols[b] = columns(u, n_k, f, counts[b], log_numerator)
    out = dict(f_boot=f_boot, n_iter=n_iter, last_delta=last)
    if cols is not None:
        out['columns'] = cols
    return out


def pair_sigma(f_boot):
    """(K, K) the standard deviation (ddof = 1) over the replicates of f_i - f_j"""
    f = np.asarray(f_boot, 'f8')
    return (f[:, :, None] - f[:, None, :]).std(axis=0, ddof=1)
