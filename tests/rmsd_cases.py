"""Inputs of the RMSD tests (tests/test_rmsd_config.py on the CPU, tests/rmsd_gpu_worker.py on the device): seeded random-walk chains
with bond length 3.8, rounded to float32, and the refusals of the entry points as one list that both sides walk."""
import ctypes as ct
import numpy as np

PARITY_N = (3, 4, 5, 63, 64, 65, 168)      # below, at and above the k-step of 4 and the LDS chunk of 16 atoms
PARITY_F = (1, 2, 15, 16, 17, 63, 64, 65, 130)      # below, at and above a 16-block and a 64-tile; three tiles with a ragged edge
PARITY_RECT = ((1, 130), (130, 1), (65, 17), (17, 65))
N_CENTRES = (17, 65)
BOUND = 1e-12       # |d2 - d2_ref| <= BOUND (G_a + G_b) / n
MARGIN = 1e-9       # what the exact comparisons need on the yardstick: a thousand times the bound
NOISE = 0.05
MAGIC = 0x75706b52  # UPK_RMSD_MAGIC


def chain(rng, n):
    step = rng.standard_normal((n, 3))
    step *= 3.8 / np.linalg.norm(step, axis=1, keepdims=True)
    return np.cumsum(step, axis=0)


def chains(seed, F, n):
    rng = np.random.RandomState(seed)
    return np.stack([chain(rng, n) for _ in range(F)]).astype('f4')


def parity_set(n):
    """130 independent chains of n atoms; the set of F frames is its first F"""
    return chains(7000 + n, 130, n)


def config_set(n):
    """the 43 frames of the CPU check of the yardstick: 40 chains, a duplicate of frame 0, the mirror image of frame 1 and frame 2
    with noise of 1e-3"""
    x = chains(9000 + n, 40, n)
    rng = np.random.RandomState(9500 + n)
    return np.concatenate([x, x[:1], x[1:2] * np.array([-1., 1., 1.], 'f4'), x[2:3] + (1e-3 * rng.standard_normal((1, n, 3))).astype('f4')]).astype('f4')


def index_lists(seed=11):
    """positions into the 130-frame set that permute and repeat frames: (ia (70,), ib (45,))"""
    rng = np.random.RandomState(seed)
    ia = np.concatenate([rng.permutation(130)[:60], rng.randint(0, 130, 10)]).astype('i4')
    ib = np.concatenate([rng.permutation(130)[:35], rng.randint(0, 130, 10)]).astype('i4')
    return ia, ib


def nearest_case(n, C):
    """(rows (130, n, 3), centres (C, n, 3)): independent chains as centres, row j = centre j % C plus noise of 0.05 per coordinate"""
    cen = chains(5000 + 10 * n + C, C, n)
    rng = np.random.RandomState(6000 + 10 * n + C)
    rows = (cen[np.arange(130) % C].astype('f8') + NOISE * rng.standard_normal((130, n, 3))).astype('f4')
    return rows, cen


def stress_set(n=37):
    """(frames (72, n, 3), notes): duplicates of frame 0 at positions 5, 33 and 66 (another block, another tile), the mirror image of
    frame 1 at 2, frame 3 plus noise of 1e-3 at 4, collinear atoms at 6 and 7 (two directions), planar frames at 8 and 9, frame 10 =
    frame 11 scaled by 100"""
    x = chains(4000 + n, 72, n).astype('f8')
    rng = np.random.RandomState(4100 + n)
    for p in (5, 33, 66):
        x[p] = x[0]
    x[2] = x[1] * np.array([-1., 1., 1.])
    x[4] = x[3] + 1e-3 * rng.standard_normal((n, 3))
    for p in (6, 7):
        u = rng.standard_normal(3); u /= np.linalg.norm(u)
        x[p] = 3.8 * np.arange(n)[:, None] * u[None, :] + rng.standard_normal(3)
    for p in (8, 9):
        x[p, :, 2] = 1.5
    x[10] = 100. * x[11]
    return x.astype('f4')


def cluster_case(n=30):
    """(frames (130, n, 3), label (130,)): 5 well-separated chains plus noise of 0.05, with 40, 30, 26, 20 and 14 members in a seeded
    order; cutoff 1.0 lies between the intra-cluster and the inter-cluster distances (asserted on the yardstick)"""
    cen = chains(3000 + n, 5, n)
    rng = np.random.RandomState(3100 + n)
    label = rng.permutation(np.repeat(np.arange(5), (40, 30, 26, 20, 14)))
    x = (cen[label].astype('f8') + NOISE * rng.standard_normal((130, n, 3))).astype('f4')
    return x, label


CLUSTER_CUTOFF = 1.0


class FramesStruct(ct.Structure):      # upk_rmsd_frames_t of include/upside_hip_kernels.h: what a handle points to
    _fields_ = [('magic', ct.c_int), ('n_atom', ct.c_int), ('n_pad', ct.c_int), ('n_frame', ct.c_longlong), ('y', ct.c_void_p), ('g', ct.c_void_p),
                ('create_ms', ct.c_double * 2)]


def described_set(n_atom, n_frame):
    """a frame set's description without device memory: enough for every refusal, which returns before any device call"""
    return FramesStruct(MAGIC, n_atom, (n_atom + 3) // 4 * 4, n_frame, None, None)


def refusal_cases(lib, A, A6, n_frame, with_huge_sets=None):
    """[(label, thunk returning the entry point's status, fragment of the message)] for the handle A (n_frame frames of 5 atoms) and A6
    (frames of 6 atoms); with_huge_sets: two described sets of 2^20 frames of 5 atoms, for nA x nB = 2^40 without index lists"""
    from numpy import zeros, arange
    F = n_frame
    out = zeros((F, F)); idx = zeros(F, 'i8'); dist = zeros(F); cnt = zeros(F, 'i8')
    pos = zeros((4, 5, 3), 'f4'); bad = zeros((9, 5, 3), 'f4'); bad[7, 2, 1] = np.nan
    h = ct.c_void_p()
    i_hi = arange(F).astype('i4'); i_hi[3] = F
    i_lo = arange(F).astype('i4'); i_lo[0] = -1
    big = zeros(1 << 20, 'i4')
    p = lambda a: None if a is None else a.ctypes.data
    M = lambda a, na, ia, b, nb, ib, o: (lambda: lib.upside_hip_rmsd_matrix(a, na, p(ia), b, nb, p(ib), p(o)))
    N = lambda a, na, ia, b, nb, ib, i, d: (lambda: lib.upside_hip_rmsd_nearest(a, na, p(ia), b, nb, p(ib), p(i), p(d)))
    C = lambda a, na, ia, b, nb, ib, c, o: (lambda: lib.upside_hip_rmsd_count(a, na, p(ia), b, nb, p(ib), c, p(o)))
    cases = [
        ('create: no place for the handle', lambda: lib.upside_hip_frames_create(5, 4, pos.ctypes.data, None), 'frames_create: frames'),
        ('create: pos NULL', lambda: lib.upside_hip_frames_create(5, 4, None, ct.byref(h)), 'frames_create: pos must be given'),
        ('create: n_atom = 2', lambda: lib.upside_hip_frames_create(2, 4, pos.ctypes.data, ct.byref(h)), 'n_atom = 2'),
        ('create: n_frame = 0', lambda: lib.upside_hip_frames_create(5, 0, pos.ctypes.data, ct.byref(h)), 'n_frame = 0'),
        ('create: 2^40 coordinates', lambda: lib.upside_hip_frames_create(1 << 20, 1 << 20, pos.ctypes.data, ct.byref(h)), 'is not below 2^40'),
        ('create: a coordinate that is not a number', lambda: lib.upside_hip_frames_create(5, 9, bad.ctypes.data, ct.byref(h)), 'frame 7, atom 2 is not finite'),
        ('matrix: A NULL', M(None, F, None, A, F, None, out), 'rmsd_matrix: A must be given'),
        ('matrix: B NULL', M(A, F, None, None, F, None, out), 'rmsd_matrix: B must be given'),
        ('matrix: out NULL', M(A, F, None, A, F, None, None), 'rmsd_matrix: out must be given'),
        ('nearest: A NULL', N(None, F, None, A, F, None, idx, dist), 'rmsd_nearest: A must be given'),
        ('nearest: index NULL', N(A, F, None, A, F, None, None, dist), 'rmsd_nearest: index must be given'),
        ('nearest: dist NULL', N(A, F, None, A, F, None, idx, None), 'rmsd_nearest: dist must be given'),
        ('count: B NULL', C(A, F, None, None, F, None, 1., cnt), 'rmsd_count: B must be given'),
        ('count: count NULL', C(A, F, None, A, F, None, 1., None), 'rmsd_count: count must be given'),
        ('matrix: different n_atom', M(A, F, None, A6, F, None, out), 'hold 5 atoms, those of B 6'),
        ('nearest: different n_atom', N(A6, F, None, A, F, None, idx, dist), 'hold 6 atoms, those of B 5'),
        ('matrix: ia above the set', M(A, F, i_hi, A, F, None, out), 'ia[3] = %d is outside the set of %d frames' % (F, F)),
        ('count: ib below 0', C(A, F, None, A, F, i_lo, 1., cnt), 'ib[0] = -1 is outside'),
        ('matrix: nA = 0', M(A, 0, None, A, F, None, out), 'nA = 0'),
        ('nearest: nB = -1', N(A, F, None, A, -1, None, idx, dist), 'nB = -1'),
        ('matrix: nA not the set without a list', M(A, F - 1, None, A, F, None, out), 'nA = %d without an index list' % (F - 1)),
        ('count: cutoff < 0', C(A, F, None, A, F, None, -0.5, cnt), 'cutoff = -0.5'),
        ('count: cutoff not a number', C(A, F, None, A, F, None, float('nan'), cnt), 'must be finite and not negative'),
        ('count: cutoff +inf', C(A, F, None, A, F, None, float('inf'), cnt), 'must be finite and not negative'),
        ('matrix: 2^40 entries through index lists', M(A, 1 << 20, big, A, 1 << 20, big, out), 'nA x nB = 1048576 x 1048576 is not below 2^40'),
    ]
    if with_huge_sets is not None:
        H1, H2 = with_huge_sets
        cases.append(('matrix: 2^40 entries of whole sets', M(H1, 1 << 20, None, H2, 1 << 20, None, out), 'is not below 2^40'))
    return cases
