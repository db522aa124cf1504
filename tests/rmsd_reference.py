"""Float64 numpy yardstick of the pairwise RMSD of frames (upside_hip_rmsd_matrix, _nearest, _count; csrc/kernels_rmsd.hip;
upside-md_amd/cluster.py): the definitions restated, for the tests of the device kernels.  Frame f of n atoms, float32 widened exactly:
    c_f = mean_i x_f,i      y_f,i = x_f,i - c_f      G_f = sum_i |y_f,i|^2
    M_ab[c][d] = sum_i y_a,i[c] y_b,i[d]             lambda_ab = the largest eigenvalue of Horn's 4 x 4 matrix of M_ab (eigvalsh)
    d2_ab = max(0, G_a + G_b - 2 lambda_ab) / n      d_ab = sqrt(d2_ab)
-- the best PROPER rotation (Horn 1987).  kabsch_d2 is the independent route (the SVD of M with the smallest singular value negated
for a reflection) that tests/test_rmsd_config.py pins the yardstick with.  kcenters and gromos restate the two clusterings of
cluster.py on a GIVEN distance matrix, with the same tie rules."""
import numpy as np


def centre(x):
    """(y (F, n, 3) float64, G (F,))"""
    x = np.asarray(x, 'f8')
    assert x.ndim == 3 and x.shape[2] == 3 and x.shape[1] >= 3
    y = x - x.mean(1, keepdims=True)
    return y, (y * y).sum((1, 2))


def horn_matrix(M):
    """Horn's symmetric 4 x 4 matrix of the 3 x 3 matrices M (..., 3, 3), M[c][d] = sum_i a_i[c] b_i[d]"""
    Sxx, Sxy, Sxz = M[..., 0, 0], M[..., 0, 1], M[..., 0, 2]
    Syx, Syy, Syz = M[..., 1, 0], M[..., 1, 1], M[..., 1, 2]
    Szx, Szy, Szz = M[..., 2, 0], M[..., 2, 1], M[..., 2, 2]
    K = np.empty(M.shape[:-2] + (4, 4))
    K[..., 0, 0] = Sxx + Syy + Szz; K[..., 0, 1] = Syz - Szy; K[..., 0, 2] = Szx - Sxz; K[..., 0, 3] = Sxy - Syx
    K[..., 1, 1] = Sxx - Syy - Szz; K[..., 1, 2] = Sxy + Syx; K[..., 1, 3] = Szx + Sxz
    K[..., 2, 2] = -Sxx + Syy - Szz; K[..., 2, 3] = Syz + Szy
    K[..., 3, 3] = -Sxx - Syy + Szz
    for i in range(4):
        for j in range(i):
            K[..., i, j] = K[..., j, i]
    return K


def correlation(ya, yb, rows=64):
    """M (nA, nB, 3, 3), in slabs of rows"""
    return np.concatenate([np.einsum('aic,bid->abcd', ya[r:r + rows], yb) for r in range(0, len(ya), rows)])


def d2_matrix(a, b=None):
    """(d2 (nA, nB), scale (nA, nB)): scale = (G_a + G_b) / n, what the bounds of the tests are relative to"""
    ya, Ga = centre(a)
    yb, Gb = (ya, Ga) if b is None else centre(b)
    assert ya.shape[1] == yb.shape[1]
    n = ya.shape[1]
    lam = np.linalg.eigvalsh(horn_matrix(correlation(ya, yb)))[..., -1]
    gsum = Ga[:, None] + Gb[None, :]
    return np.maximum(0., gsum - 2. * lam) / n, gsum / n


def rmsd_matrix(a, b=None):
    """d (nA, nB); b None: a against itself, the diagonal exactly 0 and the lower triangle the mirror of the upper"""
    d = np.sqrt(d2_matrix(a, b)[0])
    if b is None:
        d = np.triu(d, 1)
        d = d + d.T
    return d


def kabsch_d2(a, b):
    """d2 of ONE pair by the SVD route: G_a + G_b - 2 (s0 + s1 +- s2), the smallest singular value negated when det(U V^T) < 0"""
    ya, Ga = centre(np.asarray(a)[None]); yb, Gb = centre(np.asarray(b)[None])
    M = ya[0].T @ yb[0]
    u, s, vt = np.linalg.svd(M)
    if np.linalg.det(u @ vt) < 0:
        s = s * np.array([1., 1., -1.])
    return (Ga[0] + Gb[0] - 2. * s.sum()) / ya.shape[1]


def nearest(d2):
    """(index, d2 of the best, d2 of the second best or +inf) per row; the lowest column on ties"""
    d2 = np.asarray(d2)
    idx = np.argmin(d2, axis=1)
    s = np.sort(d2, axis=1)
    return idx.astype('i8'), s[:, 0], (s[:, 1] if d2.shape[1] > 1 else np.full(len(d2), np.inf))


def widest_gap_cutoff(d):
    """(cutoff, lower, upper): the midpoint of the widest gap between consecutive sorted entries of d in its middle three fifths"""
    s = np.sort(np.asarray(d, 'f8').reshape(-1))
    lo, hi = len(s) // 5, len(s) - len(s) // 5
    if hi - lo < 2:
        lo, hi = 0, len(s)
    if hi - lo < 2:
        return float(s[0]) + 1., float(s[0]), np.inf
    gaps = np.diff(s[lo:hi])
    k = int(np.argmax(gaps))
    return float(0.5 * (s[lo + k] + s[lo + k + 1])), float(s[lo + k]), float(s[lo + k + 1])


def kcenters(D, k=None, cutoff=None, first=0, gaps=None):
    """cluster.kcenters on the distance matrix D (F, F): (centers, assignment, dist); gaps (a list) receives for every round the lead
    of the farthest frame over the next one, relative to its distance"""
    D = np.asarray(D, 'f8'); F = len(D)
    centers = [int(first)]
    running = D[:, first].copy(); running[first] = 0.
    assignment = np.zeros(F, 'i8')
    while len(centers) < F and (k is None or len(centers) < k):
        far = int(np.argmax(running))
        if cutoff is not None and running[far] <= cutoff:
            break
        if running[far] == 0.:
            break
        if gaps is not None and F > 1:
            top = np.sort(running)[-2:]
            gaps.append(float((top[1] - top[0]) / top[1]))
        d = D[:, far].copy(); d[far] = 0.
        closer = d < running
        assignment[closer] = len(centers)
        running = np.where(closer, d, running)
        centers.append(far)
    return np.array(centers, 'i8'), assignment, running


def gromos(D, cutoff):
    """cluster.gromos on the distance matrix D (F, F): (centers, assignment, sizes), the largest cluster first (stable)"""
    D = np.asarray(D, 'f8'); F = len(D)
    within = D <= cutoff
    within[np.arange(F), np.arange(F)] = True
    live = np.ones(F, bool)
    found = np.full(F, -1, 'i8')
    centers, sizes = [], []
    while live.any():
        count = (within & live[None, :]).sum(1)
        cand = np.flatnonzero(live)
        c = int(cand[np.argmax(count[cand])])
        members = cand[within[c, cand]]
        found[members] = len(centers)
        centers.append(c); sizes.append(len(members))
        live[members] = False
    centers = np.array(centers, 'i8'); sizes = np.array(sizes, 'i8')
    order = np.argsort(-sizes, kind='stable')
    number = np.empty(len(order), 'i8'); number[order] = np.arange(len(order))
    return centers[order], number[found], sizes[order]
