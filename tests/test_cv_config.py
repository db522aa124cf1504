"""CPU tests of the collective variables' host side: config.add_collective_variables round-trips through h5lite and refuses bad
specs with messages, config.native_contacts builds a sane pair list, the float64 yardstick tests/cv_reference.py gives the known
answers it is trusted for, and libupside_hip.so exports the new entry points."""
import ctypes as ct
import os
import re
import shutil
import numpy as np
import pytest
import parity_util as P
import cv_reference as R

cfg = P.pkg.config
h5lite = P.pkg.h5lite


def coords(name='proteinG56_7A'):
    return np.load(os.path.join(P.GOLD, name + '.coords.npy')).astype('f8').reshape(-1, 3)


def example_specs(pos):
    ca = np.arange(1, len(pos), 3, dtype='i4')
    pairs, r0 = cfg.native_contacts(pos, ca, 8.0, 4)
    return [{'name': 'rg_ca', 'kind': 'rg', 'atoms': ca},
            {'kind': 'rmsd', 'atoms': ca, 'ref': pos[ca]},
            {'kind': 'contacts', 'pairs': pairs, 'r0': r0, 'beta': 5., 'lambda': 1.8},
            {'kind': 'distance', 'pair': (int(ca[0]), int(ca[-1]))},
            {'kind': 'rg', 'atoms': np.arange(len(pos))}]


def read_group(path):
    with h5lite.open_file(path) as f:
        return dict((k, f.read('input/collective_variables/' + k)) for k in
                    ('kind', 'atom_start', 'atoms', 'ref_pos', 'contact_r0', 'contact_beta', 'contact_lambda', 'names'))


def test_add_collective_variables_round_trips(tmp_path):
    path = str(tmp_path / 'g.up')
    shutil.copyfile(P.fixture('proteinG56_7A'), path)
    pos = cfg.read_pos(path).astype('f8')
    specs = example_specs(pos)
    packed = cfg.add_collective_variables(path, specs)
    got = read_group(path)
    n_ca = len(specs[0]['atoms']); n_pair = len(specs[2]['pairs'])
    assert got['kind'].tolist() == [0, 1, 2, 3, 0]
    assert got['atom_start'].tolist() == [0, n_ca, 2 * n_ca, 2 * n_ca + 2 * n_pair, 2 * n_ca + 2 * n_pair + 2, 2 * n_ca + 2 * n_pair + 2 + len(pos)]
    assert got['atoms'].dtype == np.int32 and got['ref_pos'].dtype == np.float32 and got['contact_r0'].dtype == np.float32
    assert got['ref_pos'].shape == (n_ca, 3) and got['contact_r0'].shape == (n_pair,)
    assert np.array_equal(got['atoms'][2 * n_ca:2 * n_ca + 2 * n_pair].reshape(-1, 2), specs[2]['pairs'])      # interleaved pairs
    assert [x.decode() for x in got['names']] == ['rg_ca', 'rmsd', 'contacts', 'distance', 'rg']
    assert got['contact_beta'][2] == 5. and abs(got['contact_lambda'][2] - 1.8) < 1e-6 and got['contact_beta'][0] == 0.
    for k in got:
        assert np.array_equal(got[k], packed[k]), k
    # the packed form and the specs mean the same thing to the yardstick
    x = pos + np.random.default_rng(1).standard_normal(pos.shape)
    assert np.allclose(R.evaluate_packed(got, x), R.evaluate(specs, x), rtol=0, atol=1e-5)
    # written again: replaced, not appended; an empty list is a valid (empty) group
    cfg.add_collective_variables(path, specs[:1])
    assert read_group(path)['kind'].tolist() == [0]
    cfg.add_collective_variables(path, [])
    got = read_group(path)
    assert got['kind'].shape == (0,) and got['atom_start'].tolist() == [0] and got['ref_pos'].shape == (0, 3)


@pytest.mark.parametrize('spec, message', [
    ({'kind': 'gyration', 'atoms': [1, 2, 3]}, 'unknown kind'),
    ({'atoms': [1, 2, 3]}, "'kind'"),
    ({'kind': 'rg', 'atoms': []}, 'empty selection'),
    ({'kind': 'rg', 'atoms': [0, 10 ** 6]}, 'out of range'),
    ({'kind': 'rg', 'atoms': [-1, 2]}, 'out of range'),
    ({'kind': 'rg', 'atoms': [0.5, 2.]}, 'integers'),
    ({'kind': 'rg'}, "'atoms' is missing"),
    ({'kind': 'rg', 'atoms': [1, 2], 'ref': np.zeros((2, 3))}, "unexpected key 'ref'"),
    ({'kind': 'rmsd', 'atoms': [1, 4], 'ref': np.zeros((2, 3))}, 'at least 3 atoms'),
    ({'kind': 'rmsd', 'atoms': [1, 4, 7], 'ref': np.zeros((4, 3))}, 'ref must be (3, 3)'),
    ({'kind': 'rmsd', 'atoms': [1, 4, 7], 'ref': np.full((3, 3), np.nan)}, 'not finite'),
    ({'kind': 'contacts', 'pairs': [1, 4, 7], 'r0': 5.}, 'pairs must be (m, 2)'),
    ({'kind': 'contacts', 'pairs': [[1, 4]], 'r0': [5., 6.]}, 'one entry per pair'),
    ({'kind': 'contacts', 'pairs': [[1, 4]], 'r0': 0.}, 'r0 must be positive'),
    ({'kind': 'contacts', 'pairs': [[1, 4]], 'r0': [-2.]}, 'r0 must be positive'),
    ({'kind': 'contacts', 'pairs': [[1, 4]], 'r0': 5., 'beta': np.inf}, 'finite'),
    ({'kind': 'distance', 'pair': (1, 2, 3)}, 'exactly 2 atoms'),
])
def test_bad_specs_are_refused_with_messages(tmp_path, spec, message):
    path = str(tmp_path / 'g.up')
    shutil.copyfile(P.fixture('trpcage20_7A'), path)
    good = {'kind': 'rg', 'atoms': [0, 1, 2]}
    with pytest.raises(ValueError) as err:
        cfg.add_collective_variables(path, [good, spec])
    assert message in str(err.value) and 'collective variable 1' in str(err.value), str(err.value)
    with h5lite.open_file(path) as f:      # nothing was written
        assert 'collective_variables' not in f.group('input')


def test_too_many_and_duplicate_names_are_refused():
    with pytest.raises(ValueError, match='exceed the limit of 64'):
        cfg.pack_collective_variables([{'kind': 'distance', 'pair': (0, 1)}] * 65, 10)
    p = cfg.pack_collective_variables([{'kind': 'distance', 'pair': (0, 1)}, {'kind': 'distance', 'pair': (0, 2)}], 10)
    assert [x.decode() for x in p['names']] == ['distance_0', 'distance_1']      # a repeated default name is numbered
    with pytest.raises(ValueError, match='distinct'):
        cfg.pack_collective_variables([{'name': 'a', 'kind': 'distance', 'pair': (0, 1)}, {'name': 'a', 'kind': 'distance', 'pair': (0, 2)}], 10)


def test_native_contacts_of_protein_g():
    pos = coords()
    ca = np.arange(1, len(pos), 3, dtype='i4')
    pairs, r0 = cfg.native_contacts(pos, ca, 8.0, 4)
    assert len(pairs) > len(ca) and pairs.shape == (len(r0), 2) and pairs.dtype == np.int32 and r0.dtype == np.float32
    assert np.isin(pairs, ca).all()
    assert (pairs[:, 0] < pairs[:, 1]).all()                                  # each pair once: no (j, i) beside (i, j)
    assert len(set(map(tuple, pairs.tolist()))) == len(pairs)
    assert ((pairs[:, 1] - pairs[:, 0]) // 3 >= 4).all()                      # sequence separation along the CA list
    d = np.sqrt(((pos[pairs[:, 0]] - pos[pairs[:, 1]]) ** 2).sum(1))
    assert np.allclose(d, r0, rtol=1e-6) and (r0 < 8.0).all() and (r0 > 0).all()
    # complete: every qualifying pair is there
    n = sum(1 for i in range(len(ca)) for j in range(i + 4, len(ca)) if np.linalg.norm(pos[ca[i]] - pos[ca[j]]) < 8.0)
    assert n == len(pairs)
    assert len(cfg.native_contacts(pos, ca, 8.0, 10)[0]) < len(pairs)
    with pytest.raises(ValueError):
        cfg.native_contacts(pos, [0, len(pos)], 8.0, 4)


def test_default_collective_variables_are_the_four_observables():
    pos = coords('trpcage20_7A')
    specs = cfg.default_collective_variables(pos)
    assert [s['kind'] for s in specs] == ['rg', 'rmsd', 'contacts', 'distance']
    v = R.evaluate(specs, pos)
    assert v[0] > 3. and v[1] < 1e-9 and v[2] > 0.99 and v[3] > 1.


# ---- the yardstick on cases with known answers ----------------------------------------------------------------
def test_yardstick_rmsd_of_a_rigid_motion_is_zero():
    rng = np.random.default_rng(7)
    pos = coords()
    for k in range(5):
        moved = pos @ R.random_rotation(rng).T + rng.standard_normal(3) * 50.
        r = R.rmsd(moved, pos)
        print('rigid motion %d: rmsd %.3e' % (k, r))
        assert r < 1e-9


def test_yardstick_rmsd_of_a_mirror_image_is_not_zero():
    pos = coords()
    mirrored = pos * np.array([1., 1., -1.])
    assert R.rmsd(mirrored, pos) > 1.0            # a chiral chain cannot be rotated onto its mirror image
    assert R.rmsd(mirrored, mirrored) < 1e-12
    # a known displacement: one atom of a 4-atom set moved by d changes the RMSD by at most d / 2 and by more than 0
    a = np.array([[0., 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]])
    b = a.copy(); b[3, 2] += 0.1
    assert 0. < R.rmsd(b, a) <= 0.05 + 1e-12


def test_yardstick_rg_of_known_point_sets():
    cube = np.array([[x, y, z] for x in (-1., 1.) for y in (-1., 1.) for z in (-1., 1.)])
    assert abs(R.rg(cube) - np.sqrt(3.)) < 1e-14
    assert abs(R.rg(cube * 2.5 + np.array([10., -3., 7.])) - 2.5 * np.sqrt(3.)) < 1e-13
    assert abs(R.rg(np.array([[0., 0, 0], [2., 0, 0]])) - 1.) < 1e-15


def test_yardstick_q_is_one_half_at_lambda_r0_and_exact_far_away():
    x = np.array([[0., 0, 0], [9., 0, 0], [0, 0, 1e3]])
    assert R.contacts(x, [[0, 1]], [5.], 5., 1.8) == 0.5
    assert R.contacts(x, [[0, 2]], [5.], 5., 1.8) == 0.              # 1e3 A apart: exactly 0, no overflow
    assert R.contacts(x, [[0, 1], [0, 2]], [5., 5.], 5., 1.8) == 0.25
    x[1, 0] = 1.
    assert abs(R.contacts(x, [[0, 1]], [5.], 5., 1.8) - 1. / (1. + np.exp(5. * (1. - 9.)))) < 1e-15
    assert R.distance(x, (0, 2)) == 1e3


# ---- the shared library --------------------------------------------------------------------------------------
CV_SYMBOLS = ['upside_hip_cv_define', 'upside_hip_cv_load', 'upside_hip_cv_count', 'upside_hip_cv_compute', 'upside_hip_cv_record',
              'upside_hip_cv_read', 'upk_cv_compute', 'upk_cv_record']


def test_cv_symbols_are_declared_and_exported():
    if not os.path.exists(P.pkg.PRODUCT_LIB):
        pytest.fail('libupside_hip.so not built (run __graft_entry__.build())')
    lib = ct.CDLL(P.pkg.PRODUCT_LIB)
    declared = ''
    for header in ('upside_engine_c.h', 'upside_hip_kernels.h'):
        txt = open(os.path.join(P.ROOT, 'include', header)).read()
        declared += re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    for n in CV_SYMBOLS:
        assert re.search(r'\b%s\s*\(' % n, declared), 'not declared: ' + n
        assert hasattr(lib, n), 'not exported: ' + n


def test_engine_binds_the_cv_calls():
    eng = P.pkg.engine
    assert eng.BatchEngine is eng.Ensemble
    for m in ('define_cvs', 'load_cvs', 'cvs', 'record_cvs', 'read_cvs'):
        assert callable(getattr(eng.BatchEngine, m)), m
