"""CPU tests of the RMSD yardstick tests/rmsd_reference.py (float64 numpy, the statement of upside_hip_rmsd_matrix / _nearest / _count)
against an independent formula, of the host-side pieces of upside-md_amd/cluster.py and of the entry points' refusals, and of the
margins the GPU checks of tests/test_gpu_rmsd.py rest their exact comparisons on.  None of them needs a GPU."""
import ctypes as ct
import os
import numpy as np
import pytest
import parity_util as P
import cv_reference as V
import rmsd_reference as R
import rmsd_cases as C

pkg = P.pkg
cl = pkg.cluster


def test_yardstick_equals_the_kabsch_form():
    """d2 = G_a + G_b - 2 sum sigma with the smallest singular value negated for a reflection, within 1e-13 (G_a + G_b) / n, on 43
    frames (a duplicate, a mirror image and a 1e-3 perturbation among them) for n in {3, 4, 5, 63, 64, 65, 168}"""
    worst = 0.
    for n in C.PARITY_N:
        x = C.config_set(n)
        d2, scale = R.d2_matrix(x)
        ref = np.array([[R.kabsch_d2(x[a], x[b]) for b in range(len(x))] for a in range(len(x))])
        r = float((np.abs(d2 - np.maximum(0., ref)) / scale).max())
        print('n = %3d: largest |d2 - d2_kabsch| / ((G_a + G_b) / n) = %.3e (bound 1e-13)' % (n, r))
        worst = max(worst, r)
        assert r <= 1e-13
        assert d2[0, 40] <= 1e-13 * scale[0, 40]                      # the duplicate
        assert 0. < np.sqrt(d2[2, 42]) < 3e-3                         # the 1e-3 perturbation
        if n > 3:      # (three atoms lie in a plane: the mirror image of a planar frame is a rotation of it)
            assert np.sqrt(d2[1, 41]) > 1e-3 and abs(d2[1, 41] - R.kabsch_d2(x[1], x[41])) <= 1e-13 * scale[1, 41]      # the mirror image
    print('worst %.3e' % worst)


def test_rotated_and_translated_frames_coincide_and_the_cv_yardstick_agrees():
    rng = np.random.RandomState(5)
    for n in C.PARITY_N:
        x = C.chains(8000 + n, 6, n).astype('f8')
        moved = np.stack([f @ V.random_rotation(rng).T + 1e3 * rng.standard_normal(3) for f in x])
        d2, scale = R.d2_matrix(x, moved)
        print('n = %3d: largest d2 / ((G_a + G_b) / n) of a moved copy %.3e (bound 1e-12)' % (n, (np.diag(d2) / np.diag(scale)).max()))
        assert (np.diag(d2) <= C.BOUND * np.diag(scale)).all(), (n, np.diag(d2) / np.diag(scale))
        d = R.rmsd_matrix(x[:3], x[3:])
        for a in range(3):
            for b in range(3):
                assert abs(d[a, b] - V.rmsd(x[a], x[3 + b])) <= 1e-10 * max(1., d[a, b]), (n, a, b)
    sym = R.rmsd_matrix(C.config_set(5))
    assert (np.diag(sym) == 0.).all() and np.array_equal(sym, sym.T)


def test_cluster_value_errors_come_before_the_library():
    class NoLibrary:      # touching the library would raise AttributeError, not ValueError
        pass
    x = C.chains(1, 4, 5)
    bad = NoLibrary()
    for what, call in (
            ('pos not (F, n, 3)', lambda: cl.Frames(x[0], library=bad)),
            ('pos last axis not 3', lambda: cl.Frames(x[:, :, :2], library=bad)),
            ('no frame', lambda: cl.Frames(x[:0], library=bad)),
            ('two atoms', lambda: cl.Frames(x[:, :2], library=bad)),
            ('two atoms after atoms', lambda: cl.Frames(x, atoms=[0, 1], library=bad)),
            ('atoms outside', lambda: cl.Frames(x, atoms=[0, 1, 5], library=bad)),
            ('atoms below 0', lambda: cl.Frames(x, atoms=[-1, 1, 2], library=bad)),
            ('atoms empty', lambda: cl.Frames(x, atoms=[], library=bad)),
            ('atoms not whole numbers', lambda: cl.Frames(x, atoms=[0., 1.5, 2.], library=bad)),
            ('a coordinate not finite', lambda: cl.Frames(np.where(np.arange(60).reshape(4, 5, 3) == 31, np.nan, x), library=bad)),
            ('nearest without b', lambda: cl.nearest(x, None, library=bad)),
            ('count_within without b', lambda: cl.count_within(x, None, 1., library=bad)),
            ('cutoff negative', lambda: cl.count_within(x, x, -1., library=bad)),
            ('cutoff not a number', lambda: cl.count_within(x, x, np.nan, library=bad)),
            ('cutoff an array', lambda: cl.count_within(x, x, [1., 2.], library=bad)),
            ('kcenters without k and cutoff', lambda: cl.kcenters(x, library=bad)),
            ('kcenters k = 0', lambda: cl.kcenters(x, k=0, library=bad)),
            ('kcenters k = 1.5', lambda: cl.kcenters(x, k=1.5, library=bad)),
            ('kcenters cutoff negative', lambda: cl.kcenters(x, cutoff=-1., library=bad)),
            ('gromos cutoff negative', lambda: cl.gromos(x, -0.1, library=bad)),
            ('gromos cutoff inf', lambda: cl.gromos(x, np.inf, library=bad)),
            ('path_neighbour_table one frame', lambda: pkg.config.path_neighbour_table(x[:1])),
            ('path_neighbour_table two atoms', lambda: pkg.config.path_neighbour_table(x[:, :2])),
    ):
        with pytest.raises(ValueError):
            call()
        print('ValueError:', what)
    with pytest.raises(ValueError) as err:
        cl.Frames(np.where(np.arange(60).reshape(4, 5, 3) == 31, np.inf, x), library=bad)
    assert 'frame 2' in str(err.value)

    # those that need a Frames: an object that stands for a live set without a library behind it
    def stand_in(F, n):
        f = cl.Frames.__new__(cl.Frames)
        f._handle, f._lib, f.n_frame, f.n_atom = ct.c_void_p(1), bad, F, n
        return f
    a, b = stand_in(4, 5), stand_in(4, 6)
    closed = stand_in(4, 5); closed._handle = None
    for what, call in (
            ('different n_atom', lambda: cl.rmsd_matrix(a, b)),
            ('ia outside', lambda: cl.rmsd_matrix(a, ia=[0, 4])),
            ('ib below 0', lambda: cl.nearest(a, a, ib=[-1])),
            ('ia empty', lambda: cl.count_within(a, a, 1., ia=[])),
            ('ia not whole numbers', lambda: cl.rmsd_matrix(a, ia=[0.5, 1.])),
            ('ia two-dimensional', lambda: cl.rmsd_matrix(a, ia=[[0, 1]])),
            ('atoms with a Frames', lambda: cl.rmsd_matrix(a, atoms=[0, 1, 2])),
            ('a closed Frames', lambda: cl.rmsd_matrix(closed)),
            ('kcenters first outside', lambda: cl.kcenters(a, k=2, first=4)),
            ('matrix of 2^40 entries', lambda: cl.rmsd_matrix(a, ia=np.zeros(1 << 20, 'i4'), ib=np.zeros(1 << 20, 'i4'))),
    ):
        with pytest.raises(ValueError):
            call()
        print('ValueError:', what)
    for f in (a, b, closed):
        f._handle = None      # (nothing to free)


def test_the_entry_points_state_their_refusals():
    """the refusals of upside_hip_frames_create and upside_hip_rmsd_* return before any device call, so they are the same with and
    without a GPU; the frame sets are descriptions without device memory"""
    if not os.path.exists(pkg.PRODUCT_LIB):
        pytest.fail('libupside_hip.so not built (run __graft_entry__.build())')
    lib = cl._library(None)
    A, A6 = C.described_set(5, 20), C.described_set(6, 20)
    H1, H2 = C.described_set(5, 1 << 20), C.described_set(5, 1 << 20)
    cases = C.refusal_cases(lib, ct.byref(A), ct.byref(A6), 20, (ct.byref(H1), ct.byref(H2)))
    assert len(cases) >= 26
    for label, call, fragment in cases:
        rc = call()
        msg = lib.upside_hip_last_error().decode()
        print('%-48s %d %s' % (label, rc, msg))
        assert rc == 1 and fragment in msg, (label, rc, msg)
    dead = C.described_set(5, 20); dead.magic = 0
    out = np.zeros((20, 20))
    assert lib.upside_hip_rmsd_matrix(ct.byref(dead), 20, None, ct.byref(A), 20, None, out.ctypes.data) == 1
    assert 'A is not a live frame set' in lib.upside_hip_last_error().decode()
    lib.upside_hip_frames_free(None)
    # the Python layer turns a refusal of the library into RuntimeError with its message
    f = cl.Frames.__new__(cl.Frames)
    f._handle, f._lib, f.n_frame, f.n_atom = ct.cast(ct.pointer(dead), ct.c_void_p), lib, 20, 5
    with pytest.raises(RuntimeError) as err:
        cl.rmsd_matrix(f)
    assert 'not a live frame set' in str(err.value)
    f._handle = None


def test_clusterings_of_the_yardstick_on_a_hand_made_matrix():
    """six points on a line at 0, 1, 2, 10, 11, 20: distances |x_i - x_j|, with ties"""
    x = np.array([0., 1., 2., 10., 11., 20.])
    D = np.abs(x[:, None] - x[None, :])
    c, a, d = R.kcenters(D, k=3)
    # from 0 the farthest is 20; then 10 and 11 have running distances 10 and 9: 10 (index 3)
    assert c.tolist() == [0, 5, 3] and a.tolist() == [0, 0, 0, 2, 2, 1] and d.tolist() == [0., 1., 2., 0., 1., 0.]
    c, a, d = R.kcenters(D, cutoff=2.)
    assert c.tolist() == [0, 5, 3] and d.max() <= 2.
    c, a, d = R.kcenters(D, k=2, first=2)
    assert c.tolist() == [2, 5] and a.tolist() == [0, 0, 0, 0, 0, 1]      # 11 is 9 from both: the lower centre number stays
    c, a, d = R.kcenters(np.zeros((3, 3)), k=3)
    assert c.tolist() == [0] and a.tolist() == [0, 0, 0]                  # every frame coincides with the centre
    # equidistant from 1: points 0 and 2 (distance 1 each) -- the lowest index is the next centre
    c, a, d = R.kcenters(np.abs(x[:3, None] - x[None, :3]), k=2, first=1)
    assert c.tolist() == [1, 0]
    # gromos with cutoff 1: counts (itself included) 2, 3, 2, 2, 2, 1 -> centre 1 takes {0, 1, 2}; then 10 and 11 tie at 2: the lower
    c, a, s = R.gromos(D, 1.)
    assert c.tolist() == [1, 3, 5] and a.tolist() == [0, 0, 0, 1, 1, 2] and s.tolist() == [3, 2, 1]
    # cutoff 0: every point its own cluster, in index order
    c, a, s = R.gromos(D, 0.)
    assert c.tolist() == list(range(6)) and s.tolist() == [1] * 6
    # the largest cluster first although it is found second: 0 | 5, 6 | 20, 21, 22, 23 with cutoff 1 -> counts 1 | 2, 2 | 2, 3, 3, 2
    y = np.array([0., 5., 6., 20., 21., 22., 23.])
    c, a, s = R.gromos(np.abs(y[:, None] - y[None, :]), 1.)
    assert c.tolist() == [4, 1, 0, 6] and s.tolist() == [3, 2, 1, 1] and a.tolist() == [2, 1, 1, 0, 0, 0, 3]
    oc, oa, os_ = cl.order_clusters([0, 1, 4], [0, 1, 1, 2, 2, 2], [1, 2, 3])
    assert oc.tolist() == [4, 1, 0] and oa.tolist() == [2, 1, 1, 0, 0, 0] and os_.tolist() == [3, 2, 1]
    cut, lo, hi = R.widest_gap_cutoff([0., 1., 2., 3., 7., 8., 9., 10., 11., 30.])
    assert (cut, lo, hi) == (5., 3., 7.)      # (the gap 11 .. 30 lies outside the middle three fifths)


def test_the_gpu_cases_keep_their_margins():
    """what the exact comparisons of tests/test_gpu_rmsd.py rest on, on the yardstick alone, for every shape of the parity check: the
    best and the second-best d2 of every row differ by more than 1e-9 (G_a + G_b) / n, and so do the two d2 around the count cutoff;
    the clustering case keeps inter-cluster distances above ten times the intra-cluster ones, with the cutoff between them"""
    for n in C.PARITY_N:
        for nc in C.N_CENTRES:
            rows, cen = C.nearest_case(n, nc)
            d2, scale = R.d2_matrix(rows, cen)
            idx, best, second = R.nearest(d2)
            assert n < 63 or np.array_equal(idx, np.arange(130) % nc), (n, nc)      # (triangles of three atoms are all alike)
            assert ((second - best) > C.MARGIN * scale.max(1)).all(), (n, nc)
            for F in C.PARITY_F:
                cut, lo, hi = R.widest_gap_cutoff(np.sqrt(d2[:F]))
                assert hi * hi - lo * lo > C.MARGIN * scale[:F].max() and lo < cut < hi, (n, nc, F, lo, hi)
        # the rectangular shapes take the first nA frames of the parity set against its last nB
        d2, scale = R.d2_matrix(C.parity_set(n))
        for nA, nB in C.PARITY_RECT:
            ra, rb = d2[:nA, 130 - nB:], scale[:nA, 130 - nB:]
            idx, best, second = R.nearest(ra)
            assert ((second - best) > C.MARGIN * rb.max(1)).all(), (n, nA, nB)
            cut, lo, hi = R.widest_gap_cutoff(np.sqrt(ra))
            assert hi * hi - lo * lo > C.MARGIN * rb.max(), (n, nA, nB)
    x, label = C.cluster_case()
    D = R.rmsd_matrix(x)
    same = label[:, None] == label[None, :]
    intra, inter = D[same].max(), D[~same].min()
    print('clustering case: largest intra-cluster d %.4f, smallest inter-cluster d %.4f, cutoff %.2f' % (intra, inter, C.CLUSTER_CUTOFF))
    assert inter > 10. * intra and intra < C.CLUSTER_CUTOFF < inter
    gaps = []
    c, a, d = R.kcenters(D, k=5, gaps=gaps)
    assert len(set(label[c].tolist())) == 5 and np.array_equal(label[c][a], label)
    # the farthest frame of every round leads the next by a thousand times what the bound on d2 allows d to move, relative to d:
    # BOUND scale / (2 d^2) with d above the smallest inter-cluster distance
    need = 1e3 * C.BOUND * R.d2_matrix(x)[1].max() / (2. * inter * inter)
    print('kcenters: smallest lead of the farthest frame %.3e of its distance, needed %.3e' % (min(gaps), need))
    assert min(gaps) > need, gaps
    c, a, s = R.gromos(D, C.CLUSTER_CUTOFF)
    assert s.tolist() == [40, 30, 26, 20, 14] and np.array_equal(label[c][a], label)
