"""Float64 numpy yardstick of the collective variables (radius of gyration, RMSD after optimal superposition, fraction of native
contacts, distance): the four formulas restated from their definitions, for the tests of the device kernel.  The RMSD goes through
the SVD of the correlation matrix (Kabsch 1976, with the reflection fix), applies the rotation and measures the distance atom by
atom -- a route that shares nothing with the kernel's quaternion eigenvalue and has no cancellation near the reference.
tests/test_cv_config.py pins it on cases with known answers."""
import numpy as np


def rg(x):
    x = np.asarray(x, 'f8')
    return float(np.sqrt(((x - x.mean(0)) ** 2).sum(1).mean()))


def kabsch_rotation(a, b):
    """the proper rotation U (det +1) minimising sum |a_i - U b_i|^2 for centred a, b (n,3)"""
    h = b.T @ a                            # sum_i b_i a_i^T
    u, s, vt = np.linalg.svd(h)
    d = np.sign(np.linalg.det(vt.T @ u.T))
    if d == 0:
        d = 1.
    return vt.T @ np.diag([1., 1., d]) @ u.T


def rmsd(x, ref):
    """minimum over proper rigid motions of sqrt(mean |x_i - (U ref_i + t)|^2)"""
    a = np.asarray(x, 'f8'); b = np.asarray(ref, 'f8')
    assert a.shape == b.shape and a.ndim == 2 and a.shape[1] == 3
    a = a - a.mean(0); b = b - b.mean(0)
    u = kabsch_rotation(a, b)
    return float(np.sqrt(((a - b @ u.T) ** 2).sum(1).mean()))


def contacts(x, pairs, r0, beta, lam):
    """Q = mean over pairs of 1 / (1 + exp(beta (r_ij - lam r0_ij))), evaluated without overflow"""
    x = np.asarray(x, 'f8'); pairs = np.asarray(pairs).reshape(-1, 2)
    r = np.sqrt(((x[pairs[:, 0]] - x[pairs[:, 1]]) ** 2).sum(1))
    arg = float(beta) * (r - float(lam) * np.asarray(r0, 'f8'))
    e = np.exp(-np.abs(arg))
    return float((np.where(arg > 0, e, 1.) / (1. + e)).mean())


def distance(x, pair):
    x = np.asarray(x, 'f8')
    return float(np.sqrt(((x[pair[0]] - x[pair[1]]) ** 2).sum()))


def evaluate(specs, x):
    """the values of a list of CV specs (the dicts of config.add_collective_variables) at positions x (n_atom,3): float64 (n_cv,)"""
    out = []
    for sp in specs:
        k = sp['kind']
        if k == 'rg':
            out.append(rg(np.asarray(x, 'f8')[np.asarray(sp['atoms'])]))
        elif k == 'rmsd':
            out.append(rmsd(np.asarray(x, 'f8')[np.asarray(sp['atoms'])], sp['ref']))
        elif k == 'contacts':
            out.append(contacts(x, sp['pairs'], sp['r0'], sp.get('beta', 5.), sp.get('lambda', 1.8)))
        elif k == 'distance':
            out.append(distance(x, sp['pair']))
        else:
            raise ValueError('unknown kind %r' % (k,))
    return np.array(out, 'f8')


def evaluate_packed(p, x):
    """the same from the packed arrays of /input/collective_variables (config.pack_collective_variables)"""
    x = np.asarray(x, 'f8')
    out, i_ref, i_pair = [], 0, 0
    for c, k in enumerate(np.asarray(p['kind'])):
        a = np.asarray(p['atoms'])[p['atom_start'][c]:p['atom_start'][c + 1]]
        if k == 0:
            out.append(rg(x[a]))
        elif k == 1:
            out.append(rmsd(x[a], np.asarray(p['ref_pos'], 'f8')[i_ref:i_ref + len(a)])); i_ref += len(a)
        elif k == 2:
            m = len(a) // 2
            out.append(contacts(x, a.reshape(-1, 2), np.asarray(p['contact_r0'])[i_pair:i_pair + m], p['contact_beta'][c], p['contact_lambda'][c]))
            i_pair += m
        elif k == 3:
            out.append(distance(x, a))
        else:
            raise ValueError('unknown kind %r' % (k,))
    return np.array(out, 'f8')


def random_rotation(rng):
    """a proper rotation from a random unit quaternion"""
    q = rng.standard_normal(4); q /= np.linalg.norm(q)
    a, b, c, d = q
    return np.array([[a * a + b * b - c * c - d * d, 2 * (b * c - a * d), 2 * (b * d + a * c)],
                     [2 * (b * c + a * d), a * a - b * b + c * c - d * d, 2 * (c * d - a * b)],
                     [2 * (b * d - a * c), 2 * (c * d + a * b), a * a - b * b - c * c + d * d]])
