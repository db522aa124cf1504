"""Float64 numpy yardstick of the moving restraint on collective variables (node cv_steer):

    c_c(t) = center_c + rate_c t, stopped at center_end_c (min for rate > 0, max for rate < 0)      t: completed MD rounds
    d_c    = v_c - c_c(t), wrapped into [-pi, pi] for a dihedral (the centre itself stays on the unwrapped line)
    E      = sum_c 1/2 k_c u_c^2,  u_c = max(0, |d_c| - flat_width_c)
    W_n    = W_{n-1} + sum_c E_c(v_n, c(n)) - E_c(v_n, c(n-1))       the centre is switched at the end of round n, at fixed coordinates

Values and their gradients come from tests/cv_dihedral_reference.py (which passes the four older kinds on to tests/cv_reference.py
and tests/cv_restraint_reference.py); the response to d is that file's restraint_term.  The schedule and the work are written out
here on their own, step by step in Python floats, and tests/test_cv_steer_config.py holds config.steer_center and config.steer_work
against them and the derivative against central differences of the energy."""
import numpy as np
import cv_dihedral_reference as D

VALUES = ('center', 'rate', 'center_end', 'spring_const', 'flat_width')


def center_at(center, rate, center_end, t):
    """the centre of one CV after t rounds"""
    center, rate, center_end = float(center), float(rate), float(center_end)
    c = center + rate * float(t)
    if rate > 0.:
        return min(c, center_end)
    if rate < 0.:
        return max(c, center_end)
    return c


def centers(specs, t):
    return np.array([center_at(sp['center'], sp['rate'], sp['center_end'], t) for sp in specs], 'f8')


def term(sp, v, t):
    """(E, dE/dv) of one CV with value v at clock t"""
    return D.restraint_term(v, center_at(sp['center'], sp['rate'], sp['center_end'], t), sp['spring_const'], sp.get('flat_width', 0.), sp['kind'] in D.PERIODIC)


def energy_and_gradient(specs, x, t):
    """(E, dE/dx (n_atom, 3), v (n_cv,)) at clock t of specs with the keys VALUES (flat_width defaults to 0), float64"""
    x = np.asarray(x, 'f8')
    e, grad, vs = 0., np.zeros_like(x), []
    for sp in specs:
        v, g = D.value_and_gradient(sp, x)
        ec, dv = term(sp, v, t)
        e += ec; grad += dv * g; vs.append(v)
    return e, grad, np.array(vs)


def energy(specs, x, t):
    return energy_and_gradient(specs, x, t)[0]


def numeric_gradient(specs, x, t, h=1e-5):
    """central differences of the energy over the atoms the CVs touch, float64"""
    x = np.array(x, 'f8')
    g = np.zeros_like(x)
    touched = set()
    for sp in specs:
        for key in ('atoms', 'pairs', 'pair', 'quads'):
            if key in sp:
                touched.update(np.asarray(sp[key]).reshape(-1).tolist())
    for i in sorted(touched):
        for d in range(3):
            x0 = x[i, d]
            x[i, d] = x0 + h; ep = energy(specs, x, t)
            x[i, d] = x0 - h; em = energy(specs, x, t)
            x[i, d] = x0
            g[i, d] = (ep - em) / (2. * h)
    return g


def work(specs, values, t0=0):
    """the accumulated work after each round, (n_round,): values (n_round, n_cv) as seen at the end of rounds t0 + 1, t0 + 2, ..."""
    values = np.asarray(values, 'f8')
    out, w = [], 0.
    for n, row in enumerate(values):
        dw = 0.
        for sp, v in zip(specs, row):
            dw += term(sp, v, t0 + n + 1)[0] - term(sp, v, t0 + n)[0]
        w += dw
        out.append(w)
    return np.array(out, 'f8')


def work_scale(specs, values, t0=0):
    """sum_n sum_c |E_c(v_n, c(n))| + |E_c(v_n, c(n-1))|: what the rounding of the work's terms is measured against"""
    values = np.asarray(values, 'f8')
    return float(sum(abs(term(sp, v, t0 + n + 1)[0]) + abs(term(sp, v, t0 + n)[0]) for n, row in enumerate(values) for sp, v in zip(specs, row)))
