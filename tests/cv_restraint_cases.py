"""Inputs shared by the cv_restraint tests (CPU and GPU): perturbed structures and restrained-CV spec lists built from a fixture's
golden coordinates.  Everything is drawn from fixed seeds; nothing here touches the engine."""
import os
import numpy as np
import parity_util as P
import cv_reference as R


def coords(name):
    return np.load(os.path.join(P.GOLD, name + '.coords.npy')).astype('f8').reshape(-1, 3)


def perturbed(name, seed=0, sigma=0.5):
    """golden coordinates + N(0, sigma), rounded to fp32 (what the device sees), as float64"""
    rng = np.random.default_rng(seed)
    x = coords(name)
    return (x + sigma * rng.standard_normal(x.shape)).astype('f4').astype('f8')


def noisy_reference(x_sel, rng, sigma=1.5):
    """an rmsd reference: a rotated copy of the selection plus N(0, sigma)"""
    return (x_sel - x_sel.mean(0)) @ R.random_rotation(rng).T + sigma * rng.standard_normal(x_sel.shape) + rng.standard_normal(3)


def force_specs(name, x):
    """one node's worth of CVs covering every kind and the lane-stride edges, each with k > 0; the centres are placed relative to
    the values at x so that some CVs sit inside their flat bottom (zero force, zero energy) and the others on either side of it"""
    rng = np.random.default_rng(7)
    native = coords(name)
    n_atom = len(x)
    ca = np.arange(1, n_atom, 3, dtype='i4')
    specs = [{'name': 'rg_all', 'kind': 'rg', 'atoms': np.arange(n_atom, dtype='i4')}]
    for n in (255, 256, 257):
        if n < n_atom:
            specs.append({'name': 'rg_%d' % n, 'kind': 'rg', 'atoms': np.arange(n, dtype='i4')})
    half = np.arange(n_atom // 2, dtype='i4')
    three = np.array([n_atom - 1, 0, n_atom // 2], 'i4')
    specs += [{'name': 'rmsd_ca', 'kind': 'rmsd', 'atoms': ca, 'ref': noisy_reference(native[ca], rng)},
              {'name': 'rmsd_half', 'kind': 'rmsd', 'atoms': half, 'ref': noisy_reference(native[half], rng)},
              {'name': 'rmsd_3', 'kind': 'rmsd', 'atoms': three, 'ref': noisy_reference(native[three], rng)}]
    pairs, r0 = P.pkg.config.native_contacts(native, ca)
    specs += [{'name': 'q_1', 'kind': 'contacts', 'pairs': pairs[:1], 'r0': r0[:1], 'beta': 5., 'lambda': 1.0},
              {'name': 'q_native', 'kind': 'contacts', 'pairs': pairs, 'r0': r0, 'beta': 5., 'lambda': 1.0},
              {'name': 'd_a', 'kind': 'distance', 'pair': (int(ca[0]), int(ca[-1]))},
              {'name': 'd_b', 'kind': 'distance', 'pair': (int(ca[len(ca) // 2]), int(ca[0]))}]
    v = R.evaluate(specs, x)
    # (offset of the centre from the value, flat width) as fractions of the value: outside below, outside above, inside, plain harmonic
    place = [(-0.10, 0.), (0.12, 0.04), (0.05, 0.08), (-0.07, 0.02), (0.09, 0.)]
    for c, sp in enumerate(specs):
        off, w = place[c % len(place)]
        sp['center'] = float(v[c] * (1. + off)); sp['flat_width'] = float(abs(v[c]) * w)
        sp['spring_const'] = float((5. + c) / max(v[c], 0.05) ** 2)      # energies of order k (off v)^2 / 2 ~ 0.05 whatever the CV's unit
    return specs


def inside_flat(specs, x):
    v = R.evaluate(specs, x)
    return np.array([abs(v[c] - sp['center']) < sp['flat_width'] for c, sp in enumerate(specs)])
