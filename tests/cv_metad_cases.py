"""Inputs shared by the cv_metadynamics tests (CPU and GPU) on trpcage20 (60 atoms): CV sets of 1 to 4 dimensions, widths and random
hills around a point.  Everything is drawn from fixed seeds; nothing here touches the engine."""
import numpy as np
import parity_util as P
import cv_restraint_cases as K

NAME = 'trpcage20_7A'


def specs_of(d):
    """d = 1: rg over all atoms; d = 2: rmsd over CA + native contacts; d = 3: rg over the first 3 atoms, a distance, contacts with
    one pair; d = 4: rg over CA, rmsd over the first half, a distance, native contacts"""
    native = K.coords(NAME)
    n_atom = len(native)
    ca = np.arange(1, n_atom, 3, dtype='i4')
    rng = np.random.default_rng(11)
    pairs, r0 = P.pkg.config.native_contacts(native, ca)
    rmsd_ca = {'name': 'rmsd_ca', 'kind': 'rmsd', 'atoms': ca, 'ref': K.noisy_reference(native[ca], rng)}
    q = {'name': 'q', 'kind': 'contacts', 'pairs': pairs, 'r0': r0, 'beta': 5., 'lambda': 1.0}
    if d == 1:
        return [{'name': 'rg', 'kind': 'rg', 'atoms': np.arange(n_atom, dtype='i4')}]
    if d == 2:
        return [rmsd_ca, q]
    if d == 3:
        return [{'name': 'rg_3', 'kind': 'rg', 'atoms': np.arange(3, dtype='i4')}, {'name': 'd', 'kind': 'distance', 'pair': (int(ca[0]), int(ca[-1]))},
                {'name': 'q_1', 'kind': 'contacts', 'pairs': pairs[:1], 'r0': r0[:1], 'beta': 5., 'lambda': 1.0}]
    if d == 4:
        half = np.arange(n_atom // 2, dtype='i4')
        return [{'name': 'rg_ca', 'kind': 'rg', 'atoms': ca}, {'name': 'rmsd_half', 'kind': 'rmsd', 'atoms': half, 'ref': K.noisy_reference(native[half], rng)},
                {'name': 'd', 'kind': 'distance', 'pair': (int(ca[1]), int(ca[-2]))}, q]
    raise ValueError(d)


def rounded_to_file(specs):
    """the specs with every number rounded to the float32 the file holds: the yardstick sees the same definition"""
    out = []
    for sp in specs:
        sp = dict(sp)
        for k in ('ref', 'r0'):
            if k in sp:
                sp[k] = np.asarray(sp[k], 'f4').astype('f8')
        for k in ('beta', 'lambda'):
            if k in sp:
                sp[k] = float(np.float32(sp[k]))
        out.append(sp)
    return out


def sigma_of(v):
    """widths of a tenth of the value (float32, as the file holds them)"""
    return np.maximum(0.1 * np.abs(np.asarray(v, 'f8')), 0.01).astype('f4')


def random_hills(v, sigma, n, seed):
    """n hills with centres within +-2 sigma of v and weights in [0.1, 1], float32"""
    rng = np.random.default_rng(seed)
    d = len(v)
    c = np.asarray(v, 'f8')[None, :] + rng.uniform(-2., 2., (n, d)) * np.asarray(sigma, 'f8')[None, :]
    return c.astype('f4'), rng.uniform(0.1, 1., n).astype('f4')
