"""Seeded inputs of the metadynamics-analysis tests (tests/test_metad_config.py, tests/metad_gpu_worker.py): lists of hills, points
near them, grids over them, and the double-well toy whose known free energy the reweighting formula must recover."""
import numpy as np

HILL_COUNTS = (0, 1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1000)
POINT_COUNTS = (1, 255, 256, 257, 1000)
LIST_COUNTS = (1, 3, 65)
AXIS_SIZES = (1, 15, 16, 17, 63, 64, 65, 100)
SCALES = (0., 1., -2.5)
SIGMA = np.array([0.35, 0.2, 0.5, 0.27])
TWO_PI = 2. * np.pi


def periods_of(d, periodic):
    """dimension 0 periodic with 2 pi, or none"""
    per = np.zeros(d)
    if periodic:
        per[0] = TWO_PI
    return per


def hills(d, n, seed, periodic=False):
    """(centers (n, d) f4, weights (n,) f4 of both signs): centres in a box of a few sigma; with `periodic`, dimension 0 has the
    period 2 pi and its centres lie within 0.3 of +pi or -pi, so that nearest images cross the border"""
    rng = np.random.RandomState(seed)
    c = rng.uniform(-2., 2., size=(n, d)) * (4. * SIGMA[:d])
    if periodic:
        side = rng.randint(0, 2, size=n) * 2 - 1
        c[:, 0] = side * (np.pi - rng.uniform(0., 0.3, size=n))
    w = rng.uniform(0.05, 0.4, size=n) * np.where(rng.uniform(size=n) < 0.3, -1., 1.)
    return c.astype('f4'), w.astype('f4')


def points_near(centers, n, seed, d, periodic=False):
    """n points (n, d) f8, each within 8 sigma of some hill (within the box of the hills where there are none)"""
    rng = np.random.RandomState(seed)
    if len(centers):
        x = centers[rng.randint(0, len(centers), size=n)].astype('f8') + np.clip(2.5 * rng.standard_normal((n, d)), -8., 8.) * SIGMA[:d]
    else:
        x = rng.uniform(-2., 2., size=(n, d)) * (4. * SIGMA[:d])
    if periodic:      # some beyond the border, to be wrapped
        x[:, 0] = np.where(np.abs(x[:, 0]) > np.pi + 1., x[:, 0] - TWO_PI * np.rint(x[:, 0] / TWO_PI), x[:, 0])
    return x


def axes_over(d, sizes, periodic=False):
    """axes of the given sizes over the box of hills() (a single value sits at 0.1 sigma)"""
    out = []
    for k, n in enumerate(sizes):
        if periodic and k == 0:
            out.append(-np.pi + TWO_PI * np.arange(n) / n)
        else:
            out.append(np.linspace(-9., 9., n) * SIGMA[k] if n > 1 else np.array([0.1 * SIGMA[k]]))
    return out


def unequal_lists(d, n_list, seed, periodic=False, counts=HILL_COUNTS):
    """n_list lists of unequal lengths from `counts`, list 1 (where there is one) empty: (centers, weights, hill_start)"""
    ns = [counts[(5 * l + seed) % len(counts)] for l in range(n_list)]
    if n_list > 1:
        ns[1] = 0
    parts = [hills(d, n, 100 * seed + l, periodic) for l, n in enumerate(ns)]
    return (np.concatenate([p[0] for p in parts]).reshape(-1, d), np.concatenate([p[1] for p in parts]),
            np.concatenate(([0], np.cumsum(ns))).astype('i8'))


# ---- the toy: 32 walkers sharing one list on U = 4 (x^2 - 1)^2 ---------------------------------------------------------------------------
TOY = dict(n_walker=32, kT=1., dt=0.002, n_round=20000, pace=50, every=10, sigma=0.1, height=0.2, table=1201, table_range=3.,
           grid=np.linspace(-2.5, 2.5, 501), bins=np.linspace(-1.4, 1.4, 29), drop=0.2)


def toy_potential(x):
    return 4. * (x * x - 1.) ** 2


def toy_run(seed, kdT):
    """overdamped Euler steps of dt on U + V with n_walker walkers depositing into one list every `pace` rounds (slot k n_walker + s),
    frames every `every` rounds, recorded BEFORE the round's deposit as the engine does.  The force of the bias comes from a table
    of V on 1201 points over [-3, 3] (central differences, linear interpolation); the hill weights come from the exact sum over the
    hills of earlier rounds, height exp(-V / kdT) (plain: height), rounded to float32 as the node stores them.
    Returns (centers (H, 1) f4, weights (H,) f4, frames (N,) f8, rounds (N,) i8), frames in time order, walkers side by side."""
    T = TOY
    rng = np.random.RandomState(seed)
    S, dt, sg = T['n_walker'], T['dt'], T['sigma']
    tx = np.linspace(-T['table_range'], T['table_range'], T['table'])
    h = tx[1] - tx[0]
    tv = np.zeros_like(tx)
    slope = np.zeros_like(tx)
    x = np.where(np.arange(S) % 2 == 0, -1., 1.) + 0.05 * rng.standard_normal(S)
    n_dep = T['n_round'] // T['pace']
    centers = np.zeros(n_dep * S, 'f4'); weights = np.zeros(n_dep * S, 'f4')
    frames = []; rounds = []
    noise = np.sqrt(2. * T['kT'] * dt)
    n = 0
    for r in range(1, T['n_round'] + 1):
        xi = np.clip(x, tx[0], tx[-1])
        f = -16. * x * (x * x - 1.) - np.interp(xi, tx, slope)
        x = x + f * dt + noise * rng.standard_normal(S)
        if r % T['every'] == 0:
            frames.append(x.copy()); rounds.append(np.full(S, r, 'i8'))
        if r % T['pace'] == 0:
            c32 = x.astype('f4')
            c = c32.astype('f8')
            if kdT > 0 and n:
                dz = (c[:, None] - centers[:n].astype('f8')[None, :]) / sg
                v_at = np.exp(-0.5 * dz * dz) @ weights[:n].astype('f8')
                w32 = (T['height'] * np.exp(-v_at / kdT)).astype('f4')
            else:
                w32 = np.full(S, T['height'], 'f4')
            centers[n:n + S] = c32; weights[n:n + S] = w32
            n += S
            dz = (tx[:, None] - c[None, :]) / sg
            tv += np.exp(-0.5 * dz * dz) @ w32.astype('f8')
            slope = np.gradient(tv, h)
    return centers[:, None], weights, np.concatenate(frames), np.concatenate(rounds)


def toy_profiles(frames, rounds, log_w):
    """(F_reweighted, F_unweighted, F_exact) over the toy's bins, each -ln of a probability normalised over the bins; the first
    fifth of the run is dropped"""
    T = TOY
    keep = rounds > T['drop'] * T['n_round']
    x, lw = frames[keep], log_w[keep]
    out = []
    for wts in (np.exp(lw - lw.max()), np.ones(len(x))):
        hst = np.histogram(x, bins=T['bins'], weights=wts)[0]
        with np.errstate(divide='ignore'):
            out.append(-T['kT'] * np.log(hst / hst.sum()))
    fine = np.linspace(T['bins'][0], T['bins'][-1], 28 * 200 + 1)
    mid = 0.5 * (fine[1:] + fine[:-1])
    p = np.exp(-toy_potential(mid) / T['kT']).reshape(28, 200).mean(axis=1)
    out.append(-T['kT'] * np.log(p / p.sum()))
    return out
