"""Float64 numpy yardstick of the cv_restraint node: energy and gradient of a list of restrained collective variables.

    E = sum_c 1/2 k_c u_c^2,   u_c = max(0, |v_c - center_c| - flat_width_c),   dE/dv_c = k_c u_c sign(v_c - center_c)

The values v_c come from cv_reference; the gradients dv/dx are restated from the definitions (the rotation of the rmsd from
cv_reference.kabsch_rotation, an SVD route that shares nothing with the kernel's quaternion).  tests/test_cv_restraint_config.py
pins the gradient against central differences of the energy.  A spec is a dict of config.add_cv_restraint: the CV's own keys plus
'center', 'spring_const' and 'flat_width' (default 0)."""
import numpy as np
import cv_reference as R

V_MIN = 1e-6      # an rg, rmsd or distance below this has no direction: zero force (the energy is still counted)


def value_and_gradient(sp, x):
    """v and dv/dx (n_atom, 3) of one CV spec at positions x (n_atom, 3), float64"""
    x = np.asarray(x, 'f8')
    g = np.zeros_like(x)
    k = sp['kind']
    if k == 'rg':
        a = np.asarray(sp['atoms'])
        d = x[a] - x[a].mean(0)
        v = float(np.sqrt((d ** 2).sum(1).mean()))
        if v >= V_MIN:
            np.add.at(g, a, d / (len(a) * v))
    elif k == 'rmsd':
        idx = np.asarray(sp['atoms'])
        a = x[idx] - x[idx].mean(0)
        b = np.asarray(sp['ref'], 'f8'); b = b - b.mean(0)
        u = R.kabsch_rotation(a, b)
        d = a - b @ u.T
        v = float(np.sqrt((d ** 2).sum(1).mean()))
        if v >= V_MIN:
            np.add.at(g, idx, d / (len(idx) * v))
    elif k == 'contacts':
        pairs = np.asarray(sp['pairs']).reshape(-1, 2)
        beta, lam = float(sp.get('beta', 5.)), float(sp.get('lambda', 1.8))
        r0 = np.broadcast_to(np.asarray(sp['r0'], 'f8'), (len(pairs),))
        d = x[pairs[:, 0]] - x[pairs[:, 1]]
        r = np.sqrt((d ** 2).sum(1))
        arg = beta * (r - lam * r0)
        e = np.exp(-np.abs(arg))
        v = float((np.where(arg > 0, e, 1.) / (1. + e)).mean())
        qq = e / (1. + e) ** 2                      # q (1 - q)
        w = np.where(r > 0, -beta * qq / (np.where(r > 0, r, 1.) * len(pairs)), 0.)
        np.add.at(g, pairs[:, 0], w[:, None] * d)
        np.add.at(g, pairs[:, 1], -w[:, None] * d)
    elif k == 'distance':
        a, b = int(sp['pair'][0]), int(sp['pair'][1])
        d = x[a] - x[b]
        v = float(np.sqrt((d ** 2).sum()))
        if v >= V_MIN:
            g[a] += d / v; g[b] -= d / v
    else:
        raise ValueError('unknown kind %r' % (k,))
    return v, g


def energy_and_gradient(specs, x, values=None):
    """(E, dE/dx (n_atom,3), v (n_cv,)) in float64.  values (n_cv, 3) = [center, spring_const, flat_width] rows override the specs'."""
    x = np.asarray(x, 'f8')
    e, grad, vs = 0., np.zeros_like(x), []
    for c, sp in enumerate(specs):
        v, g = value_and_gradient(sp, x)
        cen, k, w = (sp['center'], sp['spring_const'], sp.get('flat_width', 0.)) if values is None else values[c]
        d = v - float(cen)
        u = max(0., abs(d) - float(w))
        e += 0.5 * float(k) * u * u
        grad += (float(k) * u * np.sign(d)) * g
        vs.append(v)
    return e, grad, np.array(vs)


def energy(specs, x):
    return energy_and_gradient(specs, x)[0]


def numeric_gradient(specs, x, h=1e-5):
    """central differences of energy(), float64"""
    x = np.array(x, 'f8')
    g = np.zeros_like(x)
    for i in range(x.shape[0]):
        for d in range(3):
            x0 = x[i, d]
            x[i, d] = x0 + h; ep = energy(specs, x)
            x[i, d] = x0 - h; em = energy(specs, x)
            x[i, d] = x0
            g[i, d] = (ep - em) / (2. * h)
    return g
