"""CPU tests of the path collective variables: the float64 yardstick tests/cv_path_reference.py is pinned here (its gradients against
central differences of its own values, closed forms, the conditioning of every input the GPU tests use), and so is the host side in
config.py: packing, the refusals, path_lambda, interpolate_path, path_specs, and the constants that earlier tests pin with ==."""
import os
import sys
import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import parity_util as P                # noqa: E402
import cv_restraint_cases as K         # noqa: E402
import cv_path_reference as R          # noqa: E402
import cv_path_cases as C              # noqa: E402

cfg = P.pkg.config

# |gradient - central difference| / largest |gradient| of the yardstick, h = 1e-5 Angstrom: measured 1.9e-7 (path_s) and 4.3e-8
# (path_z) as the largest over the cases below -- the truncation error of the difference, h^2 x the third derivative, which lambda
# enters cubed; asserted at ten times that
FD_BOUND = {'path_s': 1.9e-6, 'path_z': 4.3e-7}


def central_difference(spec, x, h=1e-5):
    fd = np.zeros_like(x)
    for i in range(len(x)):
        for d in range(3):
            xp = x.copy(); xp[i, d] += h
            xm = x.copy(); xm[i, d] -= h
            fd[i, d] = (R.value_and_gradient(spec, xp)[0] - R.value_and_gradient(spec, xm)[0]) / (2. * h)
    return fd


@pytest.mark.parametrize('n,n_frame,system', [(60, 8, 9), (20, 5, 15), (3, 4, 12)])
def test_yardstick_gradients_agree_with_central_differences(n, n_frame, system):
    specs = C.specs(C.TRP, n, n_frame)
    x = C.systems(C.TRP)[system].astype('f8')
    assert R.conditioning(specs, x) >= C.GAP_MIN
    for sp in specs:
        v, g = R.value_and_gradient(sp, x)
        fd = central_difference(sp, x)
        err = np.abs(fd - g).max() / np.abs(g).max()
        print('%s n %d K %d: value %.9g, |gradient - central difference| / largest |gradient| = %.3e (bound %.1e)' % (sp['kind'], n, n_frame, v, err, FD_BOUND[sp['kind']]))
        assert np.abs(g).max() > 0 and err <= FD_BOUND[sp['kind']]
        assert not g[np.setdiff1d(np.arange(len(x)), sp['atoms'])].any()


def test_two_identical_frames_give_the_midpoint():
    x = K.perturbed(C.TRP)
    atoms = np.arange(60)
    f = C.end_structure(C.TRP)
    lam = 0.7
    s_spec, z_spec = cfg.path_specs('twin', atoms, np.array([f, f]), lam)
    r = R.path(s_spec, x)
    d = R.msd(x[atoms], f)[0]
    print('s %.15g, z %.15g, d - ln 2 / lambda %.15g' % (r['s'], r['z'], d - np.log(2.) / lam))
    assert r['s'] == 1.5 and abs(r['z'] - (d - np.log(2.) / lam)) <= 1e-14 * d and d > 0.1
    assert abs(R.value_and_gradient(z_spec, x)[0] - r['z']) == 0.
    # the minimum MSD is the one a singular value decomposition gives
    assert abs(d - cfg._superpose(f, x)[1]) <= 1e-12 * d


def test_a_structure_on_frame_j_reports_j():
    atoms, fr = C.md_frames()
    x0 = K.coords(C.TRP)
    lam = cfg.path_lambda(fr)
    sp = cfg.path_specs('p', atoms, fr, 20. * lam)[0]      # well separated: a neighbour weighs exp(-46)
    rot = np.linalg.qr(np.random.default_rng(3).standard_normal((3, 3)))[0]
    rot *= np.sign(np.linalg.det(rot))
    for j in range(1, len(fr) + 1):
        x = x0.copy()
        x[atoms] = fr[j - 1] @ rot.T + np.array([1., -2., 3.])      # frame j, moved rigidly
        r = R.path(sp, x)
        print('on frame %d: s = %.12f, z = %.3e, d_j = %.3e' % (j, r['s'], r['z'], r['d'][j - 1]))
        assert abs(r['s'] - j) < 1e-6 and abs(r['d'][j - 1]) < 1e-10 and abs(r['z']) < 1e-6
        assert np.isfinite(r['ds']).all() and np.isfinite(r['dz']).all()


def test_path_lambda_and_interpolate_path():
    x0 = K.coords(C.TRP); b = C.end_structure(C.TRP)
    fr = cfg.interpolate_path(x0, b, 5)
    assert fr.shape == (5, 60, 3) and np.array_equal(fr[0], x0)
    moved, msd_end = cfg._superpose(b, x0)
    assert np.allclose(fr[-1], moved) and abs(R.msd(x0, b)[0] - msd_end) <= 1e-12 * msd_end
    assert np.allclose(fr[2], 0.5 * (x0 + moved))
    # equally spaced on a line: adjacent frames are (1/4)^2 of the whole apart, before the residual re-alignment (which can only lower it)
    adj = np.mean([R.msd(fr[k], fr[k + 1])[0] for k in range(4)])
    assert abs(cfg.path_lambda(fr) - 2.3 / adj) <= 1e-12 * 2.3 / adj and adj <= msd_end / 16. * (1. + 1e-12)
    for bad in (fr[:1], fr[:, :2], fr[0], np.array([x0, x0])):
        with pytest.raises(ValueError):
            cfg.path_lambda(bad)
    for a, bb, k in ((x0, b, 1), (x0, b, 65), (x0, b[:10], 4), (x0[:2], b[:2], 4)):
        with pytest.raises(ValueError):
            cfg.interpolate_path(a, bb, k)
    s_spec, z_spec = cfg.path_specs('fold', np.arange(60), fr)
    assert (s_spec['name'], s_spec['kind'], z_spec['name'], z_spec['kind']) == ('fold_s', 'path_s', 'fold_z', 'path_z')
    assert s_spec['lambda'] == z_spec['lambda'] == cfg.path_lambda(fr)


def test_pack_round_trip_and_datasets():
    atoms, fr = C.md_frames()
    specs = [{'name': 'rg', 'kind': 'rg', 'atoms': np.arange(60)}] + cfg.path_specs('p', atoms, fr, 3.5) + \
            [{'name': 'ref', 'kind': 'rmsd', 'atoms': np.arange(5), 'ref': K.coords(C.TRP)[:5]}, cfg.path_specs('q', np.arange(4), fr[:3, :4], 0.25)[1]]
    p = cfg.pack_collective_variables(specs, 60)
    assert p['kind'].tolist() == [0, 8, 9, 1, 9] and p['path_n_frame'].tolist() == [0, 8, 8, 0, 3] and p['path_n_frame'].dtype == np.int32
    assert p['path_lambda'].tolist() == [0., 3.5, 3.5, 0., 0.25] and p['path_lambda'].dtype == np.float32
    assert p['path_ref_pos'].shape == (2 * 8 * 20 + 3 * 4, 3) and p['path_ref_pos'].dtype == np.float32 and p['ref_pos'].shape == (5, 3)
    assert np.array_equal(p['path_ref_pos'][:160], fr.reshape(-1, 3).astype('f4')) and np.array_equal(p['path_ref_pos'][320:], fr[:3, :4].reshape(-1, 3).astype('f4'))
    back = cfg.unpack_collective_variables(p)
    assert [sp['kind'] for sp in back] == [sp['kind'] for sp in specs] and [sp['name'] for sp in back] == ['rg', 'p_s', 'p_z', 'ref', 'q_z']
    again = cfg.pack_collective_variables(back, 60)
    assert sorted(again) == sorted(p) and all(np.array_equal(again[k], p[k]) for k in p)
    assert cfg.cv_periods(p).tolist() == [0.] * 5 and cfg.cv_periods(specs).tolist() == [0.] * 5
    assert cfg._cv_datasets(p) == cfg.CV_DATASETS + cfg.CV_PATH_DATASETS
    # the path datasets are written only where a path kind exists
    old = cfg.pack_collective_variables([specs[0], specs[3]], 60)
    assert cfg._cv_datasets(old) == cfg.CV_DATASETS
    sim = cfg.pack_collective_variables([{'kind': 'dihedral_similarity', 'quads': [[0, 1, 2, 3]], 'ref': 0.5}, specs[1]], 60)
    assert cfg._cv_datasets(sim) == cfg.CV_DATASETS + ('dihedral_ref',) + cfg.CV_PATH_DATASETS


def test_written_groups_hold_the_path_datasets(tmp_path):
    import shutil
    atoms, fr = C.md_frames()
    specs = cfg.path_specs('p', atoms, fr, 3.5)
    path = str(tmp_path / 'cv.up')
    shutil.copyfile(P.fixture(C.TRP), path)
    p = cfg.add_collective_variables(path, specs)
    cfg.add_cv_restraint(path, [dict(specs[0], center=2., spring_const=3.)])
    cfg.add_cv_steer(path, [dict(specs[0], center=2., center_end=7., n_round=50, spring_const=3.)])
    cfg.add_cv_metadynamics(path, specs, [0.2, 0.1], 0.3, 2, 10)
    with P.pkg.h5lite.open_file(path) as f:
        for grp in ('input/collective_variables', 'input/potential/cv_restraint', 'input/potential/cv_steer', 'input/potential/cv_metadynamics'):
            g = f.group(grp)
            n_cv = len(g.read('kind'))
            assert g.read('path_n_frame').tolist() == [8] * n_cv and g.read('path_lambda').tolist() == [3.5] * n_cv
            assert g.read('path_ref_pos').shape == (n_cv * 160, 3) and g.read('kind').tolist() == [8, 9][:n_cv]
            assert 'dihedral_ref' not in g.keys()
            del g
    assert np.array_equal(p['path_ref_pos'][:160], fr.reshape(-1, 3).astype('f4'))
    # a definition without a path kind is written as it always was
    cfg.add_collective_variables(path, [{'kind': 'rg', 'atoms': np.arange(60)}])
    with P.pkg.h5lite.open_file(path) as f:
        assert sorted(f.group('input/collective_variables').keys()) == sorted(cfg.CV_DATASETS)
    assert cfg.metad_node_parameters(path, 'cv_metadynamics')['periods'].tolist() == [0., 0.]


def test_earlier_constants_keep_their_values():
    assert cfg.CV_KINDS == ('rg', 'rmsd', 'contacts', 'distance', 'dihedral', 'dihedral_similarity')
    assert cfg.CV_PERIOD == {'rg': 0., 'rmsd': 0., 'contacts': 0., 'distance': 0., 'dihedral': 2. * np.pi, 'dihedral_similarity': 0.}
    assert cfg.CV_DATASETS == ('kind', 'atom_start', 'atoms', 'ref_pos', 'contact_r0', 'contact_beta', 'contact_lambda', 'names')
    assert cfg.CV_PATH_KINDS == ('path_s', 'path_z') and cfg.CV_PATH_MAX_FRAMES == 64
    assert cfg.CV_KIND_CODE == {'rg': 0, 'rmsd': 1, 'contacts': 2, 'distance': 3, 'dihedral': 4, 'dihedral_similarity': 5, 'path_s': 8, 'path_z': 9}
    assert 6 not in cfg.CV_KIND_NAME and 7 not in cfg.CV_KIND_NAME and cfg.CV_KIND_NAME[8] == 'path_s' and cfg.CV_KIND_NAME[9] == 'path_z'
    header = open(os.path.join(P.ROOT, 'include', 'upside_hip_kernels.h')).read()
    assert 'UPK_CV_PATH_S = 8, UPK_CV_PATH_Z = 9' in header and '#define UPK_CV_PATH_MAX_FRAMES 64' in header


FR = np.zeros((4, 5, 3)) + np.arange(5)[None, :, None] * np.array([1., 0.5, 0.25]) + np.arange(4)[:, None, None] * 0.1
GOOD = {'kind': 'path_s', 'atoms': np.arange(5), 'frames': FR, 'lambda': 1.5}


@pytest.mark.parametrize('change,needle', [
    (dict(frames=FR[:1]), '1 frames; a path needs 2 to 64'),
    (dict(frames=np.zeros((65, 5, 3))), '65 frames; a path needs 2 to 64'),
    (dict(atoms=np.arange(2), frames=FR[:, :2]), 'at least 3 atoms'),
    (dict(frames=FR[:, :4]), 'frames must be (K, 5, 3)'),
    (dict(frames=FR[0]), 'frames must be (K, 5, 3)'),
    (dict(frames=np.where(np.arange(60).reshape(4, 5, 3) == 17, np.nan, FR)), 'frames are not finite'),
    (dict(frames=np.where(np.arange(60).reshape(4, 5, 3) == 59, np.inf, FR)), 'frames are not finite'),
    ({'lambda': 0.}, 'lambda must be one positive, finite number'),
    ({'lambda': -1.}, 'lambda must be one positive, finite number'),
    ({'lambda': np.nan}, 'lambda must be one positive, finite number'),
    ({'lambda': np.inf}, 'lambda must be one positive, finite number'),
    ({'lambda': 1e-60}, 'lambda must be one positive, finite number'),      # (0 as the float32 the engine holds)
    ({'lambda': [1., 2.]}, 'lambda must be one positive, finite number'),
    (dict(atoms=np.arange(56, 61)), 'out of range'),
    (dict(ref=FR[0]), "unexpected key 'ref'"),
    (dict(kind='path'), 'unknown kind'),
])
def test_config_refusals(change, needle):
    sp = dict(GOOD); sp.update(change)
    with pytest.raises(ValueError) as err:
        cfg.pack_collective_variables([{'kind': 'rg', 'atoms': [0, 1]}, sp], 60)
    print(err.value)
    assert needle in str(err.value) and 'collective variable 1' in str(err.value)


@pytest.mark.parametrize('missing', ['atoms', 'frames', 'lambda'])
def test_config_refuses_a_missing_key(missing):
    sp = dict((k, v) for k, v in dict(GOOD, kind='path_z').items() if k != missing)
    with pytest.raises(ValueError) as err:
        cfg.pack_collective_variables([sp], 60)
    assert '%r is missing' % missing in str(err.value) and '(path_z)' in str(err.value)


def test_inputs_of_the_gpu_tests_keep_the_yardstick_well_conditioned():
    """every value case of tests/cv_path_gpu_worker.py: on every system, every frame with weight p_k >= 1e-12 has a relative gap of
    at least 1e-3 between the two largest eigenvalues of Horn's matrix"""
    xs = dict((name, C.systems(name).astype('f8')) for name in (C.TRP, C.GB1))
    worst = np.inf
    for name, n, n_frame, factor in C.value_cases():
        specs = C.specs(name, n, n_frame, factor)
        gap = min(R.conditioning(specs[:1], x) for x in xs[name])
        worst = min(worst, gap)
        assert gap >= C.GAP_MIN, (name, n, n_frame, factor, gap)
    atoms, fr = C.md_frames()
    sp = cfg.path_specs('p', atoms, fr)
    gap = min(R.conditioning(sp[:1], x) for x in xs[C.TRP])
    worst = min(worst, gap)
    print('smallest relative eigenvalue gap over all cases and systems: %.3e (required %.0e)' % (worst, C.GAP_MIN))
    assert worst >= C.GAP_MIN
