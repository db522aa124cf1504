"""Float64 numpy yardstick of the cv_metadynamics node: the bias of a list of Gaussian hills in the space of d collective variables,

    V(v) = sum_h w_h exp(-sum_c (v_c - s_hc)^2 / (2 sigma_c^2)),   dV/dv_c = sum_h -w_h (v_c - s_hc) / sigma_c^2 exp(...)

and its gradient dV/dx = sum_c dV/dv_c dv_c/dx.  The values v_c and the gradients dv_c/dx come from value_and_gradient of
tests/cv_restraint_reference.py (pinned there against central differences); V and dV/dv are restated here from the formulas.
tests/test_cv_metadynamics_config.py pins the whole gradient against central differences of energy().  A spec is a dict of
config.pack_collective_variables."""
import numpy as np
from cv_restraint_reference import value_and_gradient


def bias(v, centers, weights, sigma):
    """(V, dV/dv (d,)) at the point v (d,) for hills centers (n, d), weights (n,), widths sigma (d,); float64"""
    v = np.asarray(v, 'f8').reshape(-1)
    sigma = np.asarray(sigma, 'f8').reshape(-1)
    w = np.asarray(weights, 'f8').reshape(-1)
    c = np.asarray(centers, 'f8').reshape(len(w), len(v))
    diff = v[None, :] - c
    g = w * np.exp(-0.5 * ((diff / sigma) ** 2).sum(1))
    return float(g.sum()), -(g[:, None] * diff / sigma ** 2).sum(0)


def values(specs, x):
    return np.array([value_and_gradient(sp, x)[0] for sp in specs])


def energy_and_gradient(specs, x, centers, weights, sigma):
    """(V, dV/dx (n_atom, 3), v (d,)) in float64"""
    x = np.asarray(x, 'f8')
    vg = [value_and_gradient(sp, x) for sp in specs]
    v = np.array([a for a, _ in vg])
    e, dv = bias(v, centers, weights, sigma)
    grad = np.zeros_like(x)
    for c, (_, g) in enumerate(vg):
        grad += dv[c] * g
    return e, grad, v


def energy(specs, x, centers, weights, sigma):
    return bias(values(specs, x), centers, weights, sigma)[0]


def numeric_gradient(specs, x, centers, weights, sigma, h=1e-5):
    """central differences of energy(), float64"""
    x = np.array(x, 'f8')
    g = np.zeros_like(x)
    for i in range(x.shape[0]):
        for d in range(3):
            x0 = x[i, d]
            x[i, d] = x0 + h; ep = energy(specs, x, centers, weights, sigma)
            x[i, d] = x0 - h; em = energy(specs, x, centers, weights, sigma)
            x[i, d] = x0
            g[i, d] = (ep - em) / (2. * h)
    return g
