"""Yardstick of the TorusDBN backbone prior (torus_dbn -> fixed_hmm): a float64 numpy restatement of the nodes' formulas that
never calls the library, and a helper that copies a fixture and appends seeded parameters with config.add_torus_dbn.

    torus_dbn   e[r, s] = prior[restypes[r], s] + basin_param[s, 0] + cs(r) . M[:, s]
                cs = (cos phi, sin phi, cos psi, sin psi, cos(phi - psi), sin(phi - psi)), phi, psi = rama[id[r], 0:2]
                M[0:2, s] = -kappa_phi (cos mu_phi, sin mu_phi), M[2:4, s] = -kappa_psi (cos mu_psi, sin mu_psi),
                M[4:6, s] = +kappa_cor (cos, sin)(mu_phi - mu_psi);  basin_param[s] = (log norm, kappa_phi, mu_phi, kappa_psi, mu_psi, kappa_cor)
    fixed_hmm   Z = sum over the state paths of exp(-sum_r e[index[r], s_r] - sum_{r >= 1} E[s_{r-1}, s_r]); potential = -log Z,
                computed in the log domain (no offsets, no rescaling: every intermediate is a logsumexp);
                d potential / d e[index[r], s] = posterior marginal of state s at chain position r,
                d potential / d E[i, j] = expected number of i -> j transitions.
"""
import os
import shutil
import sys
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

RESTYPE_ORDER = ['ALA', 'ARG', 'ASN', 'ASP', 'CYS', 'GLN', 'GLU', 'GLY', 'HIS', 'ILE', 'LEU', 'LYS', 'MET', 'PHE', 'PRO', 'SER',
                 'THR', 'TRP', 'TYR', 'VAL', 'CPR']


def logsumexp(x, axis=None):
    x = np.asarray(x, 'f8')
    m = np.max(x, axis=axis, keepdims=True)
    out = m + np.log(np.sum(np.exp(x - m), axis=axis, keepdims=True))
    return out.reshape(()) if axis is None else np.squeeze(out, axis=axis)


# ---- torus_dbn ------------------------------------------------------------------------------------------------------------
def cs_to_emission(basin_param):
    bp = np.asarray(basin_param, 'f8')
    M = np.zeros((6, bp.shape[0]))
    for row, k, a in ((0, -bp[:, 1], bp[:, 2]), (2, -bp[:, 3], bp[:, 4]), (4, bp[:, 5], bp[:, 2] - bp[:, 4])):
        M[row] = k * np.cos(a); M[row + 1] = k * np.sin(a)
    return M


def cs_rows(rama, ids):
    rama = np.asarray(rama, 'f8')
    phi, psi = rama[ids, 0], rama[ids, 1]
    return np.stack((np.cos(phi), np.sin(phi), np.cos(psi), np.sin(psi), np.cos(phi - psi), np.sin(phi - psi)), axis=1)


def emission_energies(rama, ids, restypes, prior, basin_param):
    """[len(ids), n_state]"""
    prior = np.asarray(prior, 'f8'); bp = np.asarray(basin_param, 'f8')
    return prior[np.asarray(restypes)] + bp[:, 0][None, :] + cs_rows(rama, ids).dot(cs_to_emission(bp))


def emission_backward(rama, ids, basin_param, sens, n_rama=None):
    """d / d rama [n_rama, 2] from sens = d / d e [len(ids), n_state]; repeated ids add up"""
    cs = cs_rows(rama, ids)
    g = np.asarray(sens, 'f8').dot(cs_to_emission(basin_param).T)      # [n, 6]
    d = np.zeros((len(rama) if n_rama is None else n_rama, 2))
    np.add.at(d[:, 0], ids, -cs[:, 1] * g[:, 0] + cs[:, 0] * g[:, 1] - cs[:, 5] * g[:, 4] + cs[:, 4] * g[:, 5])
    np.add.at(d[:, 1], ids, -cs[:, 3] * g[:, 2] + cs[:, 2] * g[:, 3] + cs[:, 5] * g[:, 4] - cs[:, 4] * g[:, 5])
    return d


def prior_param_deriv(sens, restypes, n_restype):
    """[n_restype, n_state]: sum over the residues of a type of their sens rows"""
    sens = np.asarray(sens, 'f8')
    d = np.zeros((n_restype, sens.shape[1]))
    np.add.at(d, np.asarray(restypes), sens)
    return d


# ---- fixed_hmm ------------------------------------------------------------------------------------------------------------
def neg_log_z(energy, transition_energy, index=None):
    """-log Z by a log-domain forward pass; energy [n_row, n_state], the chain runs over the rows index (default: all, in order)"""
    e = np.asarray(energy, 'f8'); E = np.asarray(transition_energy, 'f8')
    if index is not None:
        e = e[np.asarray(index)]
    a = -e[0]
    for r in range(1, len(e)):
        a = logsumexp(a[:, None] - E, axis=0) - e[r]
    return -float(logsumexp(a))


def forward_backward(energy, transition_energy, index=None):
    """dict: pot (-log Z), marginals [n_chain, n_state] (row r = chain position r), sens [n_row, n_state] (the marginals at the
    rows index[r] of the argument), counts [n_state, n_state] (expected transitions)"""
    e_all = np.asarray(energy, 'f8'); E = np.asarray(transition_energy, 'f8')
    index = np.arange(len(e_all)) if index is None else np.asarray(index)
    e = e_all[index]
    n, ns = e.shape
    alpha = np.zeros((n, ns)); beta = np.zeros((n, ns))
    alpha[0] = -e[0]
    for r in range(1, n):
        alpha[r] = logsumexp(alpha[r - 1][:, None] - E, axis=0) - e[r]
    log_z = logsumexp(alpha[-1])
    for r in range(n - 1, 0, -1):
        beta[r - 1] = logsumexp(-E + (beta[r] - e[r])[None, :], axis=1)
    marginals = np.exp(alpha + beta - log_z)
    counts = np.zeros((ns, ns))
    for r in range(1, n):
        counts += np.exp(alpha[r - 1][:, None] - E + (beta[r] - e[r])[None, :] - log_z)
    sens = np.zeros_like(e_all)
    np.add.at(sens, index, marginals)
    return dict(pot=-float(log_z), marginals=marginals, sens=sens, counts=counts)


def energy_offset(transition_energy):
    """the reference's offset: the Boltzmann average of the transition energies (a gauge: -log Z does not depend on it)"""
    E = np.asarray(transition_energy, 'f8')
    w = np.exp(E.min() - E)
    return float((E * w).sum() / w.sum())


def brute_force(energy, transition_energy):
    """explicit enumeration of every state path: (-log Z, marginals, counts)"""
    import itertools
    e = np.asarray(energy, 'f8'); E = np.asarray(transition_energy, 'f8')
    n, ns = e.shape
    z = 0.; marg = np.zeros((n, ns)); counts = np.zeros((ns, ns))
    for path in itertools.product(range(ns), repeat=n):
        w = np.exp(-sum(e[r, s] for r, s in enumerate(path)) - sum(E[path[r - 1], path[r]] for r in range(1, n)))
        z += w
        for r, s in enumerate(path):
            marg[r, s] += w
        for r in range(1, n):
            counts[path[r - 1], path[r]] += w
    return -np.log(z), marg / z, counts / z


# ---- the whole prior ------------------------------------------------------------------------------------------------------
def prior_energy(rama, par, ids=None, restypes=None, index=None):
    ids = par['id'] if ids is None else ids
    restypes = par['restypes'] if restypes is None else restypes
    e = emission_energies(rama, ids, restypes, par['aa_basin_energy'], par['basin_param'])
    return neg_log_z(e, par['transition_energy'], index)


def prior_backward(rama, par, index=None):
    """dict: energy (the torus_dbn output), pot, sens (d pot / d energy), d_rama, d_prior, counts"""
    e = emission_energies(rama, par['id'], par['restypes'], par['aa_basin_energy'], par['basin_param'])
    fb = forward_backward(e, par['transition_energy'], index)
    return dict(energy=e, pot=fb['pot'], sens=fb['sens'], counts=fb['counts'],
                d_rama=emission_backward(rama, par['id'], par['basin_param'], fb['sens']),
                d_prior=prior_param_deriv(fb['sens'], par['restypes'], len(par['aa_basin_energy'])))


# ---- parameters for the tests (no TorusDBN library ships with the reference: a seeded generator) ----------------------------
def random_parameters(n_state, seed, transition_span=3., prior_span=1., kappa=4.):
    rs = np.random.RandomState(seed)
    bp = np.zeros((n_state, 6), 'f4')
    bp[:, 0] = rs.normal(size=n_state)
    bp[:, 1] = rs.uniform(0.3, kappa, size=n_state); bp[:, 2] = rs.uniform(-np.pi, np.pi, size=n_state)
    bp[:, 3] = rs.uniform(0.3, kappa, size=n_state); bp[:, 4] = rs.uniform(-np.pi, np.pi, size=n_state)
    bp[:, 5] = rs.uniform(-1., 1., size=n_state)
    return dict(basin_param=bp, aa_basin_energy=(prior_span * rs.normal(size=(len(RESTYPE_ORDER), n_state))).astype('f4'),
                transition_energy=rs.uniform(0., transition_span, size=(n_state, n_state)).astype('f4'), restype_order=list(RESTYPE_ORDER))


def append_hmm(fixture_path, out_path, n_state=55, seed=1, par=None, name='', **kw):
    """copy a configuration and append a seeded TorusDBN prior; returns the parameters with the id, restypes and index that
    were written and the two node names"""
    from __graft_entry__ import load_package
    pkg = load_package()
    shutil.copyfile(fixture_path, out_path)
    os.chmod(out_path, 0o644)
    par = dict(par) if par is not None else random_parameters(n_state, seed, **kw)
    names = pkg.config.add_torus_dbn(out_path, par['basin_param'], par['aa_basin_energy'], par['transition_energy'], par['restype_order'], name=name)
    with pkg.h5lite.open_file(out_path) as f:
        g = f.group('input/potential/' + names[0])
        par['id'] = g.read('id', 'i4'); par['restypes'] = g.read('restypes', 'i4')
        par['index'] = f.group('input/potential/' + names[1]).read('index', 'i4')
    par['names'] = names
    return par
