"""float64 numpy restatement of the path collective variables path_s and path_z (Branduardi, Gervasio & Parrinello 2007) and of the
biases on them: the yardstick of tests/test_gpu_cv_path.py, pinned on the CPU by tests/test_cv_path_config.py.

    d_k = min over proper rigid motions of the mean squared deviation between the selection and frame k  (k = 1..K, Angstrom^2)
    w_k = exp(-lambda (d_k - d_min)),   path_s = sum k w_k / sum w_k,   path_z = d_min - ln(sum w_k) / lambda

The alignment is Horn's: the largest eigenvalue of the 4x4 quaternion matrix by numpy.linalg.eigh, its eigenvector the rotation.
Specs are the dicts of config.pack_collective_variables; besides the two path kinds an 'rg' is understood, so that a bias on a mixture
can be restated."""
import numpy as np

PATH_KINDS = ('path_s', 'path_z')


def horn(a, b):
    """a, b (n,3) centred.  Returns (largest eigenvalue = max over proper R of sum a_i . R b_i, R (3,3) with a ~ b R^T, the relative
    gap between the two largest eigenvalues)"""
    M = b.T @ a                                           # M[u][v] = sum b_u a_v
    (Sxx, Sxy, Sxz), (Syx, Syy, Syz), (Szx, Szy, Szz) = M
    N = np.array([[Sxx + Syy + Szz, Syz - Szy, Szx - Sxz, Sxy - Syx],
                  [Syz - Szy, Sxx - Syy - Szz, Sxy + Syx, Szx + Sxz],
                  [Szx - Sxz, Sxy + Syx, -Sxx + Syy - Szz, Syz + Szy],
                  [Sxy - Syx, Szx + Sxz, Syz + Szy, -Sxx - Syy + Szz]])
    ev, vec = np.linalg.eigh(N)
    w, x, y, z = vec[:, -1]
    R = np.array([[w * w + x * x - y * y - z * z, 2 * (x * y - w * z), 2 * (x * z + w * y)],
                  [2 * (x * y + w * z), w * w - x * x + y * y - z * z, 2 * (y * z - w * x)],
                  [2 * (x * z - w * y), 2 * (y * z + w * x), w * w - x * x - y * y + z * z]])
    return ev[-1], R, (ev[-1] - ev[-2]) / abs(ev[-1])


def msd(xs, frame):
    """(d, dd/dxs (n,3), gap): the minimum mean squared deviation of the selection's positions xs (n,3) from frame (n,3)"""
    n = len(xs)
    a = xs - xs.mean(0); b = frame - frame.mean(0)
    lam, R, gap = horn(a, b)
    d = ((a * a).sum() + (b * b).sum() - 2. * lam) / n
    return d, (2. / n) * (a - b @ R.T), gap


def path(spec, x):
    """dict(s, z, ds (n_atom,3), dz (n_atom,3), d (K,), p (K,), gap (K,)) of a path spec at positions x (n_atom,3)"""
    x = np.asarray(x, 'f8')
    atoms = np.asarray(spec['atoms']).reshape(-1)
    frames = np.asarray(spec['frames'], 'f8'); lam = float(spec['lambda'])
    K = len(frames)
    res = [msd(x[atoms], f) for f in frames]
    d = np.array([r[0] for r in res]); gap = np.array([r[2] for r in res])
    d_min = d.min()
    w = np.exp(-lam * (d - d_min))
    p = w / w.sum()
    k = np.arange(1, K + 1, dtype='f8')
    s = (k * w).sum() / w.sum()
    z = d_min - np.log(w.sum()) / lam
    ds = np.zeros_like(x); dz = np.zeros_like(x)
    for j in range(K):
        np.add.at(ds, atoms, -lam * p[j] * (k[j] - s) * res[j][1])
        np.add.at(dz, atoms, p[j] * res[j][1])
    return dict(s=s, z=z, ds=ds, dz=dz, d=d, p=p, gap=gap)


def value_and_gradient(spec, x):
    x = np.asarray(x, 'f8')
    if spec['kind'] == 'rg':
        atoms = np.asarray(spec['atoms']).reshape(-1)
        a = x[atoms] - x[atoms].mean(0)
        v = np.sqrt((a * a).sum() / len(atoms))
        g = np.zeros_like(x); np.add.at(g, atoms, a / (len(atoms) * v))
        return v, g
    r = path(spec, x)
    return (r['s'], r['ds']) if spec['kind'] == 'path_s' else (r['z'], r['dz'])


def evaluate(specs, x):
    return np.array([value_and_gradient(sp, x)[0] for sp in specs])


def conditioning(specs, x, p_min=1e-12):
    """the smallest relative eigenvalue gap over the frames with weight p_k >= p_min of the path specs at x"""
    worst = np.inf
    for sp in specs:
        if sp['kind'] in PATH_KINDS:
            r = path(sp, x)
            worst = min(worst, r['gap'][r['p'] >= p_min].min())
    return worst


def harmonic(d, k, w):
    u = max(0., abs(d) - w)
    return 0.5 * k * u * u, (k * u if d >= 0. else -k * u)


def restraint_energy_and_gradient(specs, x, centers=None):
    """sum_c 1/2 k u^2, u = max(0, |v - center| - flat_width), its gradient (n_atom,3) and the values; centers overrides the specs'"""
    e = 0.; g = np.zeros_like(np.asarray(x, 'f8')); vals = []
    for c, sp in enumerate(specs):
        v, dv = value_and_gradient(sp, x)
        cen = float(sp['center']) if centers is None else float(centers[c])
        ec, f = harmonic(v - cen, float(sp['spring_const']), float(sp.get('flat_width', 0.)))
        e += ec; g += f * dv; vals.append(v)
    return e, g, np.array(vals)


def steer_center(sp, t):
    c = float(sp['center']) + float(sp['rate']) * float(t)
    r = float(sp['rate'])
    return min(c, float(sp['center_end'])) if r > 0 else (max(c, float(sp['center_end'])) if r < 0 else c)


def steer_energy_and_gradient(specs, x, t):
    return restraint_energy_and_gradient(specs, x, [steer_center(sp, t) for sp in specs])


def steer_work(specs, series, t0=0):
    """the work of moving the centres over the recorded values series (n_round, n_cv): row i holds the values at the end of round
    t0 + i + 1, where the centre switches from c(t0 + i) to c(t0 + i + 1)"""
    w = 0.
    for i, row in enumerate(np.asarray(series, 'f8')):
        for c, sp in enumerate(specs):
            k, fw = float(sp['spring_const']), float(sp.get('flat_width', 0.))
            w += harmonic(row[c] - steer_center(sp, t0 + i + 1), k, fw)[0] - harmonic(row[c] - steer_center(sp, t0 + i), k, fw)[0]
    return w


def metad_energy_and_gradient(specs, x, centers, weights, sigma):
    """V = sum_h w_h exp(-sum_c (v_c - s_hc)^2 / (2 sigma_c^2)) and its gradient (n_atom,3), the values"""
    vg = [value_and_gradient(sp, x) for sp in specs]
    v = np.array([a[0] for a in vg])
    centers = np.asarray(centers, 'f8').reshape(-1, len(specs)); weights = np.asarray(weights, 'f8'); sigma = np.asarray(sigma, 'f8')
    diff = v[None] - centers
    gsn = weights * np.exp(-0.5 * (diff * diff / sigma ** 2).sum(1))
    dv = -(gsn[:, None] * diff / sigma ** 2).sum(0)
    return gsn.sum(), sum(dv[c] * vg[c][1] for c in range(len(specs))), v
