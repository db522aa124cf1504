"""Float64 numpy yardstick of the torsional collective variables and of the periodic rule of the two biases:

    dihedral             phi = atan2((B x A) . G, (A . B) |G|),  F = r1 - r2, G = r2 - r3, H = r4 - r3, A = F x G, B = H x G
                         (Blondel & Karplus 1996; radians in (-pi, pi]; periodic, period 2 pi)
    dihedral_similarity  mean_i 1/2 (1 + cos(phi_i - phi0_i)) over quadruples, in [0, 1]; not periodic
    wrap(d)              d - 2 pi rint(d / 2 pi): the difference of two values of a periodic CV by its nearest image
    restraint            E = sum_c 1/2 k_c u_c^2, u_c = max(0, |d_c| - flat_width_c), d_c = v_c - center_c, wrapped for a dihedral
    hills                V = sum_h w_h exp(-sum_c d_hc^2 / (2 sigma_c^2)), d_hc = v_c - s_hc, wrapped in a dihedral's dimension

The value is the definition above; torsion_iupac restates it by another route (bond vectors b1, b2, b3) and
tests/test_cv_dihedral_config.py holds the two against each other, against known answers, and the gradient against central
differences of the value.  The four older kinds are passed on to tests/cv_reference.py and tests/cv_restraint_reference.py."""
import numpy as np
import cv_reference as R
import cv_restraint_reference as Y

TWO_PI = 2. * np.pi
G_MIN = 1e-6           # |G| below this (Angstrom): the torsion has no direction
SIN2_MIN = 1e-12       # |A|^2 not above SIN2_MIN |F|^2 |G|^2 (or B, H): three atoms collinear to within 1e-6 in the sine, or two coincident
PERIODIC = ('dihedral',)


def wrap(d):
    d = np.asarray(d, 'f8')
    return d - TWO_PI * np.rint(d / TWO_PI)


def circle_distance(a, b):
    return np.abs(wrap(np.asarray(a, 'f8') - np.asarray(b, 'f8')))


def _parts(x, quad):
    r1, r2, r3, r4 = (np.asarray(x, 'f8')[int(i)] for i in quad)
    f, g, h = r1 - r2, r2 - r3, r4 - r3
    return f, g, h, np.cross(f, g), np.cross(h, g)


def torsion(x, quad):
    f, g, h, a, b = _parts(x, quad)
    sn = float(np.dot(np.cross(b, a), g)); cs = float(np.dot(a, b) * np.sqrt(np.dot(g, g)))
    return float(np.arctan2(sn + 0., cs + 0.))      # (+ 0.: a negative zero becomes a positive one; atan2(0, 0) = 0)


def torsion_iupac(x, quad):
    """the same angle from the bond vectors: atan2(|b2| b1 . (b2 x b3), (b1 x b2) . (b2 x b3))"""
    r1, r2, r3, r4 = (np.asarray(x, 'f8')[int(i)] for i in quad)
    b1, b2, b3 = r2 - r1, r3 - r2, r4 - r3
    n1, n2 = np.cross(b1, b2), np.cross(b2, b3)
    return float(np.arctan2(np.linalg.norm(b2) * np.dot(b1, n2) + 0., np.dot(n1, n2) + 0.))


def has_direction(x, quad):
    f, g, h, a, b = _parts(x, quad)
    g2 = np.dot(g, g)
    # ("not above" the threshold: coincident end atoms, f = 0 or h = 0, make both sides 0 and have no direction either)
    return not (g2 < G_MIN * G_MIN or not np.dot(a, a) > SIN2_MIN * np.dot(f, f) * g2 or not np.dot(b, b) > SIN2_MIN * np.dot(h, h) * g2)


def torsion_gradient(x, quad):
    """dphi/dr of the four atoms, (4, 3); zeros where the torsion has no direction"""
    out = np.zeros((4, 3))
    if not has_direction(x, quad):
        return out
    f, g, h, a, b = _parts(x, quad)
    gm = np.sqrt(np.dot(g, g)); a2 = np.dot(a, a); b2 = np.dot(b, b)
    d1 = -gm / a2 * a
    d4 = gm / b2 * b
    mid = np.dot(f, g) / (a2 * gm) * a - np.dot(h, g) / (b2 * gm) * b
    out[0] = d1; out[1] = -d1 + mid; out[2] = -d4 - mid; out[3] = d4
    return out


def quads_and_refs(sp):
    q = np.asarray(sp['quads']).reshape(-1, 4)
    return q, np.broadcast_to(np.asarray(sp['ref'], 'f8'), (len(q),))


def value_and_gradient(sp, x):
    """v and dv/dx (n_atom, 3) of one CV spec (any of the six kinds) at positions x (n_atom, 3), float64"""
    x = np.asarray(x, 'f8')
    k = sp['kind']
    if k == 'dihedral':
        q = np.asarray(sp['atoms']).reshape(-1)
        g = np.zeros_like(x)
        np.add.at(g, q, torsion_gradient(x, q))
        return torsion(x, q), g
    if k == 'dihedral_similarity':
        quads, refs = quads_and_refs(sp)
        g = np.zeros_like(x)
        v = 0.
        for q, p0 in zip(quads, refs):
            phi = torsion(x, q)
            v += 0.5 * (1. + np.cos(phi - p0))
            np.add.at(g, q, (-0.5 * np.sin(phi - p0) / len(quads)) * torsion_gradient(x, q))
        return float(v / len(quads)), g
    return Y.value_and_gradient(sp, x)


def evaluate(specs, x):
    return np.array([value_and_gradient(sp, x)[0] if sp['kind'] in ('dihedral', 'dihedral_similarity') else R.evaluate([sp], x)[0] for sp in specs], 'f8')


def periods_of(specs):
    return np.array([TWO_PI if sp['kind'] in PERIODIC else 0. for sp in specs])


def numeric_value_gradient(sp, x, h):
    """central differences of the value (a dihedral's difference taken on the circle), float64"""
    x = np.array(x, 'f8')
    g = np.zeros_like(x)
    for i in sorted(set(np.asarray(sp['atoms'] if sp['kind'] == 'dihedral' else sp['quads']).reshape(-1).tolist())):
        for d in range(3):
            x0 = x[i, d]
            x[i, d] = x0 + h; vp = value_and_gradient(sp, x)[0]
            x[i, d] = x0 - h; vm = value_and_gradient(sp, x)[0]
            x[i, d] = x0
            g[i, d] = (wrap(vp - vm) if sp['kind'] in PERIODIC else vp - vm) / (2. * h)
    return g


# ---- the restraint with the periodic rule ------------------------------------------------------------------------------------------
def restraint_term(v, center, k, w, periodic):
    """(E, dE/dv) of one restrained CV"""
    d = float(v) - float(center)
    if periodic:
        d = float(wrap(d))
    u = max(0., abs(d) - float(w))
    return 0.5 * float(k) * u * u, float(k) * u * np.sign(d)


def restraint_energy_and_gradient(specs, x):
    """(E, dE/dx (n_atom, 3), v (n_cv,)) of specs with 'center', 'spring_const' and 'flat_width' (default 0), float64"""
    x = np.asarray(x, 'f8')
    e, grad, vs = 0., np.zeros_like(x), []
    for sp in specs:
        v, g = value_and_gradient(sp, x)
        ec, dv = restraint_term(v, sp['center'], sp['spring_const'], sp.get('flat_width', 0.), sp['kind'] in PERIODIC)
        e += ec; grad += dv * g; vs.append(v)
    return e, grad, np.array(vs)


# ---- the hill sum with the periodic rule -------------------------------------------------------------------------------------------
def bias(v, centers, weights, sigma, periods):
    """(V, dV/dv (d,)) at the point v (d,): hills centers (n, d), weights (n,), widths sigma (d,), periods (d,) (0 = not periodic)"""
    v = np.asarray(v, 'f8').reshape(-1)
    sigma = np.asarray(sigma, 'f8').reshape(-1)
    w = np.asarray(weights, 'f8').reshape(-1)
    c = np.asarray(centers, 'f8').reshape(len(w), len(v))
    diff = v[None, :] - c
    for k, p in enumerate(np.asarray(periods, 'f8').reshape(-1)):
        if p > 0.:
            diff[:, k] -= p * np.rint(diff[:, k] / p)
    g = w * np.exp(-0.5 * ((diff / sigma) ** 2).sum(1))
    return float(g.sum()), -(g[:, None] * diff / sigma ** 2).sum(0)


def metad_energy_and_gradient(specs, x, centers, weights, sigma):
    """(V, dV/dx (n_atom, 3), v (d,)) in float64"""
    x = np.asarray(x, 'f8')
    vg = [value_and_gradient(sp, x) for sp in specs]
    v = np.array([a for a, _ in vg])
    e, dv = bias(v, centers, weights, sigma, periods_of(specs))
    grad = np.zeros_like(x)
    for c, (_, g) in enumerate(vg):
        grad += dv[c] * g
    return e, grad, v
