"""The inputs of the path-CV tests, shared by tests/test_cv_path_config.py (which asserts that they keep the yardstick well
conditioned) and tests/cv_path_gpu_worker.py: selections, seeded smooth noise, paths made by config.interpolate_path from the fixture
to the fixture plus noise, and the systems the values are taken at.  Every number that reaches the device is rounded to the float32
it is stored in, so the yardstick sees the same definition."""
import numpy as np
import parity_util as P
import cv_restraint_cases as K

cfg = P.pkg.config
TRP = 'trpcage20_7A'        # 60 atoms
GB1 = 'proteinG56_7A'       # 168 atoms
FRAME_COUNTS = (2, 3, 4, 5, 63, 64)      # every remainder over the four wavefronts, and the full lane count of the eigen-solve
SELECTIONS = ((TRP, 3), (TRP, 20), (TRP, 60), (GB1, 63), (GB1, 64), (GB1, 65), (GB1, 128), (GB1, 129), (GB1, 168))
LAMBDA_FACTORS = (1., 100.)              # path_lambda, and a hundred times it: one frame dominates, the far weights underflow
N_SYS = 16
END_NOISE = 4.0                          # Angstrom: the path's last frame is the fixture plus smooth noise of this amplitude
GAP_MIN = 1e-3                           # relative gap of Horn's two largest eigenvalues that keeps the yardstick well conditioned


def smooth_noise(n_atom, amplitude, rng):
    """(n_atom,3): three sine modes along the chain with seeded directions and phases, rms about amplitude / sqrt(2) per mode sum"""
    t = np.arange(n_atom)[:, None] / float(n_atom)
    out = np.zeros((n_atom, 3))
    for m in range(3):
        out += rng.standard_normal(3)[None] * np.sin(2. * np.pi * (m + 1) * t + rng.uniform(0., 2. * np.pi))
    return amplitude * out / np.sqrt(3.)


def selection(name, n):
    n_atom = len(K.coords(name))
    if 3 * n == n_atom:
        return np.arange(1, n_atom, 3, dtype='i4')      # the CA atoms
    return np.arange(n, dtype='i4')


def end_structure(name, seed=11):
    x0 = K.coords(name)
    return x0 + smooth_noise(len(x0), END_NOISE, np.random.default_rng(seed))


def frames(name, atoms, n_frame, seed=11):
    """(K,n,3) float64 of float32 values: from the fixture to the fixture plus smooth noise"""
    return cfg.interpolate_path(K.coords(name)[atoms], end_structure(name, seed)[atoms], n_frame).astype('f4').astype('f8')


def specs(name, n, n_frame, factor=1., seed=11):
    """[path_s, path_z] over `n` atoms of `name` and n_frame frames, lambda = factor x path_lambda as the float32 stored"""
    atoms = selection(name, n)
    fr = frames(name, atoms, n_frame, seed)
    lam = float(np.float32(factor * cfg.path_lambda(fr)))
    return cfg.path_specs('path', atoms, fr, lam)


def systems(name, n_sys=N_SYS, seed=5, top=3.0):
    """(n_sys, n_atom, 3) float32: the fixture plus smooth noise growing from 0 to `top` Angstrom (system 0 sits on the first frame)"""
    x0 = K.coords(name)
    rng = np.random.default_rng(seed)
    return np.array([x0 + smooth_noise(len(x0), a, rng) for a in np.linspace(0., top, n_sys)]).astype('f4')


def value_cases():
    for name, n in SELECTIONS:
        for n_frame in FRAME_COUNTS:
            for factor in LAMBDA_FACTORS:
                yield name, n, n_frame, factor


def rg2(x, atoms):
    a = np.asarray(x, 'f8')[atoms]
    return float(((a - a.mean(0)) ** 2).sum() / len(atoms))


def md_frames():
    """K = 8 frames over the CA atoms of trpcage: the path of the md and record checks"""
    atoms = selection(TRP, 20)
    return atoms, frames(TRP, atoms, 8)
