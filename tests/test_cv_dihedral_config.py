"""CPU tests of the torsional collective variables' host side: the float64 yardstick tests/cv_dihedral_reference.py gives the
answers it is trusted for (known torsions, its gradient against central differences of its own value, continuity of the wrapped
restraint and hill sum across the cut at +-pi), config packs, writes and refuses the two new kinds, a definition of the older
kinds is written exactly as before, and metadynamics_free_energy wraps periodic dimensions."""
import os
import shutil
import numpy as np
import pytest
import parity_util as P
import cv_reference as R
import cv_dihedral_reference as D

cfg = P.pkg.config
h5lite = P.pkg.h5lite
NAME = 'trpcage20_7A'
OLD_DATASETS = ('kind', 'atom_start', 'atoms', 'ref_pos', 'contact_r0', 'contact_beta', 'contact_lambda', 'names')


def coords(name=NAME):
    return np.load(os.path.join(P.GOLD, name + '.coords.npy')).astype('f8').reshape(-1, 3)


def four_atoms(phi):
    """r1 at angle 0 and r4 at angle phi around the axis r2 -> r3 = +z, seen from r2: F = (1,0,0), G = (0,0,-1)"""
    return np.array([[1., 0., 0.], [0., 0., 0.], [0., 0., 1.], [np.cos(phi), np.sin(phi), 1.]])


# ---- yardstick: known answers ------------------------------------------------------------------------------------------------------
def test_yardstick_known_torsions():
    q = (0, 1, 2, 3)
    # by hand for r4 = (0, 1, 1): A = F x G = (0, 1, 0), B = H x G = (-1, 0, 0), (B x A) . G = +1, A . B = 0: +90 degrees
    assert D.torsion(four_atoms(np.pi / 2), q) == pytest.approx(np.pi / 2, abs=1e-15)
    assert D.torsion(four_atoms(-np.pi / 2), q) == pytest.approx(-np.pi / 2, abs=1e-15)
    assert D.torsion(np.array([[1., 0, 0], [0, 0, 0], [0, 0, 1.], [1., 0, 1.]]), q) == 0.                 # cis, exactly planar
    assert D.torsion(np.array([[1., 0, 0], [0, 0, 0], [0, 0, 1.], [-1., 0, 1.]]), q) == np.pi              # trans: +pi, never -pi
    rng = np.random.default_rng(0)
    for _ in range(200):      # the definition against the bond-vector form, any geometry
        x = rng.standard_normal((4, 3)) * 3.
        assert abs(D.wrap(D.torsion(x, q) - D.torsion_iupac(x, q))) < 1e-12
    for phi in np.linspace(-3.1, 3.1, 41):
        assert D.torsion(four_atoms(phi), q) == pytest.approx(phi, abs=1e-14)
    # coincident atoms: atan2(0, 0) = 0, no direction
    x = np.zeros((4, 3))
    assert D.torsion(x, q) == 0. and not D.torsion_gradient(x, q).any()


def test_yardstick_similarity_known_answers():
    x = four_atoms(0.7)
    sp = lambda ref: {'kind': 'dihedral_similarity', 'quads': [(0, 1, 2, 3)], 'ref': ref}
    assert D.value_and_gradient(sp(0.7), x)[0] == pytest.approx(1., abs=1e-15)
    assert D.value_and_gradient(sp(0.7 + np.pi), x)[0] == pytest.approx(0., abs=1e-15)
    assert D.value_and_gradient(sp(0.7 + np.pi / 2), x)[0] == pytest.approx(0.5, abs=1e-15)
    # the mean over quadruples, each with its own reference
    x = coords()
    quads = np.array([(0, 1, 2, 3), (3, 4, 5, 6), (10, 30, 20, 5)])
    phis = np.array([D.torsion(x, q) for q in quads])
    refs = np.array([0.3, -2., 3.])
    v = D.value_and_gradient({'kind': 'dihedral_similarity', 'quads': quads, 'ref': refs}, x)[0]
    assert v == pytest.approx(np.mean(0.5 * (1. + np.cos(phis - refs))), abs=1e-15)


# ---- yardstick: gradient -----------------------------------------------------------------------------------------------------------
def test_yardstick_gradient_matches_central_differences():
    """step 1e-5 A on coordinates of order 10 A: the truncation error h^2 f''' / 6 and the rounding error eps / h are both ~1e-10 of a
    gradient of order 1 / A; agreement reached: 3e-9 relative at worst over these cases, asserted at 1e-7"""
    x = coords() + 0.3 * np.random.default_rng(2).standard_normal((60, 3))
    phi_q, _, psi_q, _ = cfg.backbone_dihedrals(P.fixture(NAME))
    rng = np.random.default_rng(3)
    rq = np.array([rng.choice(60, 4, replace=False) for _ in range(12)])
    specs = [{'kind': 'dihedral', 'atoms': phi_q[4]}, {'kind': 'dihedral', 'atoms': psi_q[9]}, {'kind': 'dihedral', 'atoms': (4, 5, 7, 8)},      # (an omega, near +-pi)
             {'kind': 'dihedral_similarity', 'quads': rq, 'ref': rng.uniform(-np.pi, np.pi, 12)},
             {'kind': 'dihedral_similarity', 'quads': np.concatenate((phi_q, psi_q)), 'ref': -0.9}]
    worst = 0.
    for sp in specs:
        g = D.value_and_gradient(sp, x)[1]
        n = D.numeric_value_gradient(sp, x, 1e-5)
        err = np.abs(g - n).max() / np.abs(g).max()
        worst = max(worst, err)
        print('%s: largest |analytic - central difference| / largest |gradient| = %.2e' % (sp['kind'], err))
        assert err < 1e-7
        assert np.abs(g.sum(0)).max() < 1e-12 * np.abs(g).max() * len(g)      # a torsion is invariant under translation
    print('worst %.2e' % worst)
    # no direction: collinear first three atoms give zero gradient and a finite value
    xc = np.array([[0., 0, 0], [1., 0, 0], [2., 0, 0], [2., 1., 0.5]])
    v, g = D.value_and_gradient({'kind': 'dihedral', 'atoms': (0, 1, 2, 3)}, xc)
    assert np.isfinite(v) and not g.any()
    xc[1] = xc[0]; xc[2] = (2., 0.3, 0.)      # ... and so do coincident first two atoms (F = 0: both sides of the collinearity test are 0)
    v, g = D.value_and_gradient({'kind': 'dihedral', 'atoms': (0, 1, 2, 3)}, xc)
    assert v == 0. and not g.any()


# ---- yardstick: wrapping -----------------------------------------------------------------------------------------------------------
def test_yardstick_wrap_and_continuity_across_the_cut():
    assert float(D.wrap(-3.0 - 3.0)) == pytest.approx(2. * np.pi - 6., abs=1e-15) and 0.283 < float(D.wrap(-6.)) < 0.284
    assert float(D.wrap(0.5)) == 0.5 and float(D.wrap(7.)) == pytest.approx(7. - 2. * np.pi)
    # a window centred at +3.0: the value walks through the cut at pi; energy and slope are continuous there
    eps = 1e-9
    for w in (0., 0.05):
        ea, da = D.restraint_term(np.pi - eps, 3.0, 10., w, True)
        eb, db = D.restraint_term(-np.pi + eps, 3.0, 10., w, True)
        assert abs(ea - eb) < 1e-7 and abs(da - db) < 1e-7 and da > 0.
        # ... while the plain difference would act from the wrong side of the cut
        assert D.restraint_term(-np.pi + eps, 3.0, 10., w, False)[0] > 100. * eb
    e, d = D.restraint_term(-3.0, 3.0, 10., 0., True)
    assert e == pytest.approx(0.5 * 10. * (2. * np.pi - 6.) ** 2) and d == pytest.approx(10. * (2. * np.pi - 6.))
    # centre any finite number: shifted by a period, nothing changes
    assert D.restraint_term(1., 3.0 + 4. * np.pi, 10., 0., True)[0] == pytest.approx(D.restraint_term(1., 3.0, 10., 0., True)[0])
    # hills on both sides of the cut, in a space (dihedral, not periodic)
    centers = np.array([[3.1, 1.], [-3.1, 1.2], [3.0, 0.8]]); weights = np.array([1., 0.5, 0.7]); sigma = np.array([0.2, 0.3])
    va, ga = D.bias([np.pi - eps, 1.], centers, weights, sigma, [D.TWO_PI, 0.])
    vb, gb = D.bias([-np.pi + eps, 1.], centers, weights, sigma, [D.TWO_PI, 0.])
    assert abs(va - vb) < 1e-7 and np.abs(ga - gb).max() < 1e-6
    direct = sum(w * np.exp(-0.5 * (((np.pi - eps - c[0] + np.pi) % D.TWO_PI - np.pi) / 0.2) ** 2 - 0.5 * ((1. - c[1]) / 0.3) ** 2) for c, w in zip(centers, weights))
    assert va == pytest.approx(direct, rel=1e-12)
    # periods of 0 everywhere: the plain sum of tests/cv_metad_reference.py
    import cv_metad_reference as M
    v0, g0 = D.bias([2.9, 1.], centers, weights, sigma, [0., 0.]); v1, g1 = M.bias([2.9, 1.], centers, weights, sigma)
    assert v0 == v1 and np.array_equal(g0, g1)


# ---- config: packing and round trip ------------------------------------------------------------------------------------------------
def new_specs():
    return [{'name': 'phi5', 'kind': 'dihedral', 'atoms': (14, 15, 16, 17)},
            {'kind': 'rg', 'atoms': np.arange(1, 60, 3)},
            {'kind': 'dihedral_similarity', 'quads': [(0, 1, 2, 3), (3, 4, 5, 6)], 'ref': [-1., 2.5]},
            {'name': 'hc', 'kind': 'dihedral_similarity', 'quads': np.array([(9, 7, 8, 6)]), 'ref': -0.995},
            {'kind': 'contacts', 'pairs': [(1, 13)], 'r0': 6.}]


def test_pack_and_round_trip_of_both_kinds(tmp_path):
    assert cfg.CV_KINDS == ('rg', 'rmsd', 'contacts', 'distance', 'dihedral', 'dihedral_similarity')
    p = cfg.pack_collective_variables(new_specs(), 60)
    assert p['kind'].tolist() == [4, 0, 5, 5, 2]
    assert p['atom_start'].tolist() == [0, 4, 24, 32, 36, 38]
    assert p['atoms'][:4].tolist() == [14, 15, 16, 17] and p['atoms'][24:36].tolist() == [0, 1, 2, 3, 3, 4, 5, 6, 9, 7, 8, 6]
    assert p['dihedral_ref'].dtype == np.float32 and np.array_equal(p['dihedral_ref'], np.array([-1., 2.5, -0.995], 'f4'))
    assert [x.decode() for x in p['names']] == ['phi5', 'rg', 'dihedral_similarity', 'hc', 'contacts']
    assert cfg.cv_periods(p).tolist() == [2. * np.pi, 0., 0., 0., 0.] and cfg.cv_periods(new_specs()).tolist() == cfg.cv_periods(p).tolist()
    assert cfg.CV_PERIOD == {'rg': 0., 'rmsd': 0., 'contacts': 0., 'distance': 0., 'dihedral': 2. * np.pi, 'dihedral_similarity': 0.}
    path = str(tmp_path / 't.up')
    shutil.copyfile(P.fixture(NAME), path)
    cfg.add_collective_variables(path, new_specs())
    with h5lite.open_file(path) as f:
        assert sorted(f.group('input/collective_variables').keys()) == sorted(OLD_DATASETS + ('dihedral_ref',))
        for k in OLD_DATASETS + ('dihedral_ref',):
            assert np.array_equal(f.read('input/collective_variables/' + k), p[k]), k
    rest = [dict(sp, center=0.5, spring_const=2.) for sp in new_specs()]
    cfg.add_cv_restraint(path, rest)
    cfg.add_cv_metadynamics(path, new_specs()[:3], sigma=[0.3, 0.5, 0.1], height=0.1, pace=5, capacity=10)
    with h5lite.open_file(path) as f:
        assert np.array_equal(f.read('input/potential/cv_restraint/dihedral_ref'), p['dihedral_ref'])
        assert np.array_equal(f.read('input/potential/cv_metadynamics/dihedral_ref'), np.array([-1., 2.5], 'f4'))


def test_old_kinds_are_written_exactly_as_before(tmp_path):
    """a spec of the four older kinds: the eight datasets and no other, holding these hand-written arrays (what
    pack_collective_variables gave before the torsional kinds existed)"""
    specs = [{'kind': 'rg', 'atoms': [1, 4, 7]}, {'kind': 'rmsd', 'atoms': [1, 4, 7], 'ref': [[0, 0, 0], [1, 0, 0], [0, 2, 0]]},
             {'kind': 'contacts', 'pairs': [(1, 13), (4, 16)], 'r0': [6., 7.], 'beta': 4., 'lambda': 1.5}, {'name': 'd', 'kind': 'distance', 'pair': (1, 58)}]
    want = dict(kind=np.array([0, 1, 2, 3], 'i4'), atom_start=np.array([0, 3, 6, 10, 12], 'i4'), atoms=np.array([1, 4, 7, 1, 4, 7, 1, 13, 4, 16, 1, 58], 'i4'),
                ref_pos=np.array([[0, 0, 0], [1, 0, 0], [0, 2, 0]], 'f4'), contact_r0=np.array([6., 7.], 'f4'), contact_beta=np.array([0, 0, 4., 0], 'f4'),
                contact_lambda=np.array([0, 0, 1.5, 0], 'f4'), names=np.asarray(['rg', 'rmsd', 'contacts', 'd'], 'S'))
    p = cfg.pack_collective_variables(specs, 60)
    assert sorted(p) == sorted(OLD_DATASETS + ('dihedral_ref',)) and p['dihedral_ref'].shape == (0,) and p['dihedral_ref'].dtype == np.float32
    for k, v in want.items():
        assert p[k].dtype == v.dtype and np.array_equal(p[k], v), k
    path = str(tmp_path / 't.up')
    shutil.copyfile(P.fixture(NAME), path)
    cfg.add_collective_variables(path, specs)
    cfg.add_cv_restraint(path, [dict(sp, center=1., spring_const=1.) for sp in specs])
    cfg.add_cv_metadynamics(path, specs, sigma=[1., 1., 0.1, 1.], height=0.1, pace=5, capacity=10)
    with h5lite.open_file(path) as f:
        assert sorted(f.group('input/collective_variables').keys()) == sorted(OLD_DATASETS)
        assert sorted(f.group('input/potential/cv_restraint').keys()) == sorted(OLD_DATASETS + cfg.CV_RESTRAINT_VALUES)
        assert sorted(f.group('input/potential/cv_metadynamics').keys()) == sorted(OLD_DATASETS + ('sigma',))
        for k, v in want.items():
            assert np.array_equal(f.read('input/collective_variables/' + k), v), k
    # the defaults stay the four folding observables
    assert [sp['kind'] for sp in cfg.default_collective_variables(coords())] == ['rg', 'rmsd', 'contacts', 'distance']


def test_backbone_dihedrals_and_helix_content():
    path = P.fixture(NAME)
    phi_q, phi_r, psi_q, psi_r = cfg.backbone_dihedrals(path)
    with h5lite.open_file(path) as f:
        ids = f.read('input/potential/rama_coord/id')
    assert ids.shape == (20, 5)
    assert phi_q.shape == (19, 4) and psi_q.shape == (19, 4) and phi_r.tolist() == list(range(1, 20)) and psi_r.tolist() == list(range(19))
    assert np.array_equal(phi_q, ids[1:, 0:4]) and np.array_equal(psi_q, ids[:19, 1:5])
    assert (ids[0, 0] == -1) and (ids[19, 4] == -1)
    sp = cfg.helix_content_spec(path)
    assert sp['kind'] == 'dihedral_similarity' and np.array_equal(sp['quads'], np.concatenate((phi_q, psi_q)))
    assert np.array_equal(sp['ref'], np.array([-0.995] * 19 + [-0.820] * 19))
    sp = cfg.helix_content_spec(path, residues=[0, 3, 4], phi0=-1., psi0=-0.8)
    assert np.array_equal(sp['quads'], np.concatenate((ids[[3, 4], 0:4], ids[[0, 3, 4], 1:5]))) and sp['ref'].tolist() == [-1.] * 2 + [-0.8] * 3
    cfg.pack_collective_variables([sp], 60)
    # an ideal helix scores 1: the angles of the fixture's own structure as references
    x = coords()
    own = dict(sp, ref=[D.torsion(x, q) for q in sp['quads']])
    assert D.value_and_gradient(own, x)[0] == pytest.approx(1., abs=1e-12)


def test_free_energy_wraps_periodic_dimensions():
    rng = np.random.default_rng(5)
    centers = np.column_stack((rng.uniform(-np.pi, np.pi, 40), rng.uniform(5., 9., 40))); weights = rng.uniform(0.1, 1., 40); sigma = np.array([0.25, 0.5])
    grid = np.column_stack((np.linspace(-np.pi, np.pi, 33), np.linspace(5., 9., 33)))
    plain = cfg.metadynamics_free_energy(centers, weights, sigma, grid)
    z = (grid[:, None, :] - centers[None]) / sigma
    assert np.array_equal(plain, -(weights * np.exp(-0.5 * (z * z).sum(2))).sum(1))                        # periods=None: today's arithmetic
    assert np.array_equal(cfg.metadynamics_free_energy(centers, weights, sigma, grid, periods=[0., 0.]), plain)
    got = cfg.metadynamics_free_energy(centers, weights, sigma, grid, periods=[2. * np.pi, 0.])
    want = np.array([-D.bias(g, centers, weights, sigma, [D.TWO_PI, 0.])[0] for g in grid])
    assert np.abs(got - want).max() <= 1e-14 * np.abs(want).max()
    # -pi and +pi are one point of a periodic dimension
    ends = cfg.metadynamics_free_energy(centers[:, :1], weights, sigma[:1], np.array([-np.pi, np.pi]), periods=[2. * np.pi])
    assert ends[0] == pytest.approx(ends[1], rel=1e-12)
    wt = cfg.metadynamics_free_energy(centers, weights, sigma, grid, kT=0.8, kdT=2., periods=cfg.cv_periods([{'kind': 'dihedral'}, {'kind': 'rg'}]))
    assert np.allclose(wt, (0.8 + 2.) / 2. * want, rtol=1e-13, atol=0)
    with pytest.raises(ValueError, match='periods'):
        cfg.metadynamics_free_energy(centers, weights, sigma, grid, periods=[2. * np.pi])


# ---- config: refusals --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('spec, message', [
    ({'kind': 'angle', 'atoms': [1, 2, 3]}, 'unknown kind'),
    ({'kind': 'dihedral', 'atoms': [1, 2, 3]}, 'exactly 4 atoms'),
    ({'kind': 'dihedral', 'atoms': [1, 2, 3, 4, 5]}, 'exactly 4 atoms'),
    ({'kind': 'dihedral', 'atoms': [1, 2, 3, 1]}, 'quadruple 0 repeats an atom'),
    ({'kind': 'dihedral', 'atoms': [1, 2, 3, 60]}, 'out of range'),
    ({'kind': 'dihedral'}, "'atoms' is missing"),
    ({'kind': 'dihedral', 'atoms': [1, 2, 3, 4], 'ref': 0.}, "unexpected key 'ref'"),
    ({'kind': 'dihedral_similarity', 'quads': [1, 2, 3, 4, 5, 6], 'ref': 0.}, 'quads must be (m, 4)'),
    ({'kind': 'dihedral_similarity', 'quads': [[1, 2, 3]], 'ref': 0.}, 'quads must be (m, 4)'),
    ({'kind': 'dihedral_similarity', 'quads': [[1, 2, 3, 4], [5, 6, 7, 6]], 'ref': 0.}, 'quadruple 1 repeats an atom'),
    ({'kind': 'dihedral_similarity', 'quads': [[1, 2, 3, 4]]}, "'ref' is missing"),
    ({'kind': 'dihedral_similarity', 'quads': [[1, 2, 3, 4]], 'ref': [0., 1.]}, 'one angle per quadruple'),
    ({'kind': 'dihedral_similarity', 'quads': [[1, 2, 3, 4]], 'ref': [np.nan]}, 'ref is not finite'),
    ({'kind': 'dihedral_similarity', 'quads': [[1, 2, 3, 4]], 'ref': np.inf}, 'ref is not finite'),
    ({'kind': 'dihedral_similarity', 'quads': np.zeros((0, 4), 'i4'), 'ref': []}, 'empty selection'),
])
def test_bad_specs_are_refused(spec, message):
    with pytest.raises(ValueError) as err:
        cfg.pack_collective_variables([{'kind': 'rg', 'atoms': [0, 1]}, spec], 60)
    assert message in str(err.value) and 'collective variable 1' in str(err.value)
