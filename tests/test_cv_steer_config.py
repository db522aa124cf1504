"""CPU tests of the moving restraint's host side (node cv_steer): the float64 yardstick tests/cv_steer_reference.py gives the answers
it is trusted for (its derivative against central differences of its own energy, a schedule and a work series computed by hand),
config.steer_center and config.steer_work agree with it, add_cv_steer writes, round-trips and refuses, jarzynski_free_energy is
safe for large work, and the library registers the node type and exports its entry points."""
import os
import shutil
import numpy as np
import pytest
import parity_util as P
import cv_restraint_cases as K
import cv_dihedral_reference as D
import cv_steer_reference as S

cfg = P.pkg.config
h5lite = P.pkg.h5lite
NAME = 'trpcage20_7A'
OLD_DATASETS = ('kind', 'atom_start', 'atoms', 'ref_pos', 'contact_r0', 'contact_beta', 'contact_lambda', 'names')


@pytest.fixture(scope='module')
def lib():
    if not os.path.exists(P.pkg.PRODUCT_LIB):
        pytest.fail('libupside_hip.so not built (run __graft_entry__.build())')
    return P.pkg.UpsideLibrary(P.pkg.PRODUCT_LIB)


def base_file(tmp_path, tag='t'):
    p = str(tmp_path / (tag + '.up'))
    shutil.copyfile(P.fixture(NAME), p)
    return p


def all_datasets(path):
    out = {}
    with h5lite.open_file(path) as t:
        def walk(g, prefix):
            for k in g.keys():
                if g.is_group(k):
                    walk(g.group(k), prefix + k + '/')
                else:
                    out[prefix + k] = g.read(k)
        walk(t, '/')
    return out


def every_kind(x):
    """the CVs of cv_restraint_cases.force_specs plus two dihedrals and a dihedral_similarity, each with a schedule: some moving up,
    some down, some at rest"""
    specs = K.force_specs(NAME, x)
    phi_q, phi_r, psi_q, psi_r = cfg.backbone_dihedrals(P.fixture(NAME))
    more = [{'name': 'phi5', 'kind': 'dihedral', 'atoms': phi_q[list(phi_r).index(5)]},
            {'name': 'psi12', 'kind': 'dihedral', 'atoms': psi_q[list(psi_r).index(12)]},
            dict(cfg.helix_content_spec(P.fixture(NAME)), name='helix')]
    v = D.evaluate(more, x)
    for sp, val, (off, k, w) in zip(more, v, ((0.4, 8., 0.), (-0.5, 6., 0.1), (0.1, 40., 0.02))):
        sp['center'] = float(val + off); sp['spring_const'] = k; sp['flat_width'] = w
    specs += more
    for c, sp in enumerate(specs):      # rate per round as a fraction of the flat-bottom-free offset: +, -, 0 in turn
        step = (0.01, -0.02, 0.)[c % 3] * max(abs(sp['center']), 0.1)
        sp['rate'] = float(step); sp['center_end'] = float(sp['center'] + 25 * step)
    return specs


# ---- yardstick ---------------------------------------------------------------------------------------------------------------------
def test_yardstick_derivative_matches_central_differences():
    """step 1e-5 A: truncation h^2 f''' / 6 and rounding eps E / h are both ~1e-10 of a gradient of order 1; agreement reached over the
    11 CVs of every kind at clocks 0, 7 and past the end: 3.9e-10 of the largest element at worst, asserted at 3e-7 (what the older
    yardsticks reach)"""
    x = K.perturbed(NAME)
    specs = every_kind(x)
    assert len(specs) == 11 and sorted(set(sp['kind'] for sp in specs)) == sorted(cfg.CV_KINDS)
    worst = 0.
    for t in (0, 7, 1000):
        e, g, v = S.energy_and_gradient(specs, x, t)
        n = S.numeric_gradient(specs, x, t)
        err = np.abs(g - n).max() / np.abs(g).max()
        worst = max(worst, err)
        print('clock %4d: energy %.6g, largest |analytic - central difference| / largest |gradient| = %.2e' % (t, e, err))
        assert e > 0. and err < 3e-7
    print('worst %.2e' % worst)
    # the energy moves with the clock, and stops moving at the end of the schedule
    assert S.energy(specs, x, 0) != S.energy(specs, x, 7) and S.energy(specs, x, 25) == S.energy(specs, x, 1000)
    # rate = 0 everywhere: the restraint of tests/cv_dihedral_reference.py, bit for bit
    still = [dict(sp, rate=0., center_end=sp['center']) for sp in specs]
    e0, g0, _ = S.energy_and_gradient(still, x, 123)
    e1, g1, _ = D.restraint_energy_and_gradient(still, x)
    assert e0 == e1 and np.array_equal(g0, g1)


def test_steer_center_clamps_on_both_signs_and_hits_the_end_exactly():
    # (center_end - center) / rate an integer: 0 -> 2 in 8 steps of 0.25; the end is reached at t = 8 and kept
    t = np.arange(12)
    up = cfg.steer_center(0., 0.25, 2., t)
    assert np.array_equal(up, np.minimum(0.25 * t, 2.)) and up[8] == 2. and up[7] == 1.75 and up[11] == 2.
    down = cfg.steer_center(1., -0.25, -1., t)
    assert np.array_equal(down, np.maximum(1. - 0.25 * t, -1.)) and down[8] == -1. and down[11] == -1.
    # ... and not an integer: 0 -> 1 in steps of 0.3 overshoots at t = 4 and is stopped at exactly 1
    part = cfg.steer_center(0., 0.3, 1., t)
    assert part[3] == 0.3 * 3 and part[4] == 1. and part[11] == 1.
    part = cfg.steer_center(0., -0.3, -1., t)
    assert part[3] == -(0.3 * 3) and part[4] == -1. and part[11] == -1.
    # float32 inputs whose quotient is no integer in binary (n_round = 7): the last step may fall short of or beyond the end by an ulp
    c0, ce = np.float32(3.3), np.float32(7.9)
    r = np.float32((float(ce) - float(c0)) / 7.)
    got = cfg.steer_center(c0, r, ce, np.array([6, 7, 8, 10 ** 6]))
    assert got[0] < float(ce) and got[2] == float(ce) and got[3] == float(ce) and abs(got[1] - float(ce)) <= 1e-6
    # rate 0: at rest whatever the clock; several CVs at once; against the yardstick's scalar schedule
    assert cfg.steer_center(1.5, 0., 1.5, 10 ** 9) == 1.5
    many = cfg.steer_center([0., 1., 5.], [0.25, -0.25, 0.], [2., -1., 5.], t)
    assert many.shape == (12, 3) and np.array_equal(many[:, 0], up) and np.array_equal(many[:, 1], down) and (many[:, 2] == 5.).all()
    rng = np.random.default_rng(0)
    for _ in range(200):
        c0, ce = rng.uniform(-5, 5, 2); n = rng.integers(1, 40); tt = int(rng.integers(0, 80))
        r = (ce - c0) / n
        assert float(cfg.steer_center(c0, r, ce, tt)) == S.center_at(c0, r, ce, tt)
    # a dihedral's centre winds on the unwrapped line: no folding in the schedule
    assert cfg.steer_center(3.0, 0.1, 10., 50) == 3.0 + 0.1 * 50


def test_steer_work_of_a_hand_computed_case():
    """one CV, k = 2, no flat bottom, centre 0 -> 2 at +1 per round, the value recorded as 1.0, 1.5, 1.5 at the ends of rounds 1-3:
    E(v, c) = (v - c)^2;  round 1: E(1, 1) - E(1, 0) = -1;  round 2: E(1.5, 2) - E(1.5, 1) = 0.25 - 0.25 = 0;  round 3: the centre
    rests at 2, nothing.  With flat_width 0.5, u = max(0, |d| - 0.5): round 1: 0 - 0.25;  round 2: 0 - 0 = 0."""
    w = cfg.steer_work([[1.0], [1.5], [1.5]], [0.], [1.], [2.], [2.], [0.])
    assert np.array_equal(w, [-1., -1., -1.])
    w = cfg.steer_work([1.0, 1.5, 1.5], [0.], [1.], [2.], [2.], [0.5])       # (n_round,) for one CV
    assert np.array_equal(w, [-0.25, -0.25, -0.25])
    w = cfg.steer_work([[1.0], [2.5], [1.5]], [0.], [1.], [2.], [2.], [0.])       # round 2: E(2.5, 2) - E(2.5, 1) = 0.25 - 2.25 = -2
    assert np.array_equal(w, [-1., -3., -3.])
    # t0: the same series recorded from clock 1 on sees the centre go 1 -> 2 -> 2
    w = cfg.steer_work([[1.0], [1.5]], [0.], [1.], [2.], [2.], [0.], t0=1)       # E(1, 2) - E(1, 1) = 1; then at rest
    assert np.array_equal(w, [1., 1.])
    # two CVs add; against the yardstick's step-by-step loop on a random series
    rng = np.random.default_rng(1)
    specs = [dict(kind='distance', center=5., rate=0.1, center_end=7., spring_const=3., flat_width=0.2),
             dict(kind='rg', center=9., rate=-0.05, center_end=8.5, spring_const=7., flat_width=0.)]
    v = np.column_stack((rng.uniform(4., 8., 30), rng.uniform(8., 10., 30)))
    got = cfg.steer_work(v, *[[sp[k] for sp in specs] for k in S.VALUES])
    want = S.work(specs, v)
    print('largest |steer_work - yardstick| / scale %.2e' % (np.abs(got - want).max() / S.work_scale(specs, v)))
    assert np.abs(got - want).max() <= 1e-14 * S.work_scale(specs, v)
    with pytest.raises(ValueError, match='values must be'):
        cfg.steer_work(np.zeros((3, 3)), *[[sp[k] for sp in specs] for k in S.VALUES])


def test_steer_work_across_the_cut():
    """a dihedral pulled from +3.0 upwards at 0.1 per round with k = 10: at the end of round 5 the centre goes 3.4 -> 3.5 on the
    unwrapped line while the value is -2.9, i.e. 2 pi - 2.9 = 3.383...: d goes -0.0168 -> -0.1168; unwrapped it would be -6.3 -> -6.4"""
    v = [[3.05], [3.1], [-3.1], [-3.0], [-2.9]]
    two_pi = 2. * np.pi
    w = cfg.steer_work(v, [3.0], [0.1], [4.0], [10.], [0.], periods=[two_pi])
    e = lambda val, c: 5. * (((val - c + np.pi) % two_pi) - np.pi) ** 2
    want = np.cumsum([e(val[0], 3.0 + 0.1 * (n + 1)) - e(val[0], 3.0 + 0.1 * n) for n, val in enumerate(v)])
    assert np.abs(w - want).max() < 1e-13
    last = e(-2.9, 3.5) - e(-2.9, 3.4)
    assert abs(last - 5. * (0.11681469 ** 2 - 0.01681469 ** 2)) < 1e-6
    plain = cfg.steer_work(v, [3.0], [0.1], [4.0], [10.], [0.])
    assert abs(plain[-1]) > 50. * abs(w[-1])      # without periods the plain difference of ~6.3 rad would be charged
    spec = [dict(kind='dihedral', center=3.0, rate=0.1, center_end=4.0, spring_const=10., flat_width=0.)]
    assert np.abs(w - S.work(spec, v)).max() < 1e-13
    assert np.array_equal(cfg.steer_work(v, [3.0], [0.1], [4.0], [10.], [0.], periods=[0.]), plain)


def test_jarzynski_free_energy():
    assert cfg.jarzynski_free_energy([3.25] * 7, 0.6) == pytest.approx(3.25, abs=1e-14)
    assert cfg.jarzynski_free_energy([-2.] * 3, 0.8) == pytest.approx(-2., abs=1e-14)
    kT = 0.6
    big = cfg.jarzynski_free_energy([1e4 * kT, 1e4 * kT], kT)      # exp(-1e4) underflows: only log-sum-exp survives
    assert np.isfinite(big) and big == pytest.approx(1e4 * kT, rel=1e-14)
    big = cfg.jarzynski_free_energy([-1e4 * kT, -1e4 * kT + 1.], kT)
    assert np.isfinite(big)
    w = np.array([0.1, 0.5, 0.9, 2.0])
    assert cfg.jarzynski_free_energy(w, kT) == pytest.approx(-kT * np.log(np.mean(np.exp(-w / kT))), rel=1e-13)
    assert cfg.jarzynski_free_energy(w, kT) <= w.mean()      # Jensen: Delta F <= <W>
    for bad in ([], [np.nan], [np.inf, 1.]):
        with pytest.raises(ValueError, match='work'):
            cfg.jarzynski_free_energy(bad, kT)
    with pytest.raises(ValueError, match='kT'):
        cfg.jarzynski_free_energy(w, 0.)


# ---- config: writing ---------------------------------------------------------------------------------------------------------------
def steer_specs():
    return [{'name': 'd', 'kind': 'distance', 'pair': (1, 58), 'center': 10., 'center_end': 18., 'n_round': 160, 'spring_const': 20.},
            {'name': 'phi5', 'kind': 'dihedral', 'atoms': (14, 15, 16, 17), 'center': 3.0, 'center_end': 9.0, 'rate': 0.05, 'spring_const': 5., 'flat_width': 0.1},
            {'kind': 'rg', 'atoms': np.arange(1, 60, 3), 'center': 7., 'center_end': 7., 'rate': 0., 'spring_const': 2.}]


def test_add_cv_steer_round_trips_and_leaves_the_rest_of_the_file_alone(tmp_path):
    assert cfg.CV_STEER_VALUES == ('center', 'rate', 'center_end', 'spring_const', 'flat_width') == S.VALUES
    p = base_file(tmp_path)
    before = all_datasets(p)
    packed = cfg.add_cv_steer(p, steer_specs())
    want = dict(center=[10., 3.0, 7.], rate=[0.05, 0.05, 0.], center_end=[18., 9.0, 7.], spring_const=[20., 5., 2.], flat_width=[0., 0.1, 0.])
    after = all_datasets(p)
    node = '/input/potential/cv_steer/'
    assert sorted(k for k in after if k not in before) == sorted(node + k for k in OLD_DATASETS + cfg.CV_STEER_VALUES)      # no dihedral_ref: no dihedral_similarity
    for k in before:      # everything else: byte for byte what it was
        assert after[k].dtype == before[k].dtype and after[k].shape == before[k].shape and after[k].tobytes() == before[k].tobytes(), k
    for k, v in want.items():
        assert after[node + k].dtype == np.float32 and np.array_equal(after[node + k], np.asarray(v, 'f4')), k
        assert np.array_equal(packed[k], after[node + k])
    bare = cfg.pack_collective_variables([dict((k, v) for k, v in sp.items() if k not in cfg.CV_STEER_VALUES + ('n_round',)) for sp in steer_specs()], 60)
    for k in OLD_DATASETS:
        assert np.array_equal(after[node + k], bare[k]), k
    with h5lite.open_file(p) as f:
        assert [a.decode() if isinstance(a, bytes) else str(a) for a in f.group('input/potential/cv_steer').get_attr('arguments')] == ['pos']
    # a second node under another name; a dihedral_similarity brings its dihedral_ref; writing again replaces
    sim = {'kind': 'dihedral_similarity', 'quads': [(0, 1, 2, 3), (3, 4, 5, 6)], 'ref': [-1., 2.5], 'center': 0.5, 'center_end': 0.9, 'n_round': 4, 'spring_const': 30.}
    cfg.add_cv_steer(p, [sim], name='cv_steer_helix')
    cfg.add_cv_steer(p, [sim], name='cv_steer_helix')
    d = all_datasets(p)
    assert np.array_equal(d['/input/potential/cv_steer_helix/dihedral_ref'], np.array([-1., 2.5], 'f4'))
    assert d['/input/potential/cv_steer_helix/rate'][0] == np.float32((0.9 - 0.5) / 4)
    assert all(d[k].tobytes() == after[k].tobytes() for k in after)
    # the pinned constants and the packed dict are what they were
    assert cfg.CV_KINDS == ('rg', 'rmsd', 'contacts', 'distance', 'dihedral', 'dihedral_similarity') and cfg.CV_DATASETS == OLD_DATASETS
    assert sorted(bare) == sorted(OLD_DATASETS + ('dihedral_ref',))


def test_files_without_the_node_are_written_as_before(tmp_path):
    """the writers of the other CV groups give the datasets they gave: the same keys, and no cv_steer anywhere"""
    specs = [{'kind': 'rg', 'atoms': [1, 4, 7]}, {'name': 'd', 'kind': 'distance', 'pair': (1, 58)}]
    p = base_file(tmp_path)
    cfg.add_collective_variables(p, specs)
    cfg.add_cv_restraint(p, [dict(sp, center=1., spring_const=1.) for sp in specs])
    cfg.add_cv_metadynamics(p, specs, sigma=[1., 1.], height=0.1, pace=5, capacity=10)
    d = all_datasets(p)
    assert not any('cv_steer' in k for k in d)
    with h5lite.open_file(p) as f:
        assert sorted(f.group('input/collective_variables').keys()) == sorted(OLD_DATASETS)
        assert sorted(f.group('input/potential/cv_restraint').keys()) == sorted(OLD_DATASETS + cfg.CV_RESTRAINT_VALUES)
        assert sorted(f.group('input/potential/cv_metadynamics').keys()) == sorted(OLD_DATASETS + ('sigma',))
    # two files written the same way are the same bytes, with and without this module's functions having run in between
    q = base_file(tmp_path, 'q')
    cfg.add_cv_steer(base_file(tmp_path, 'other'), steer_specs())
    cfg.add_collective_variables(q, specs)
    cfg.add_cv_restraint(q, [dict(sp, center=1., spring_const=1.) for sp in specs])
    cfg.add_cv_metadynamics(q, specs, sigma=[1., 1.], height=0.1, pace=5, capacity=10)
    assert open(p, 'rb').read() == open(q, 'rb').read()


GOOD = {'kind': 'distance', 'pair': (1, 58), 'center': 10., 'center_end': 18., 'rate': 0.05, 'spring_const': 20.}


@pytest.mark.parametrize('change, message', [
    (dict(center=None), "'center' is missing"),
    (dict(center_end=None), "'center_end' is missing"),
    (dict(spring_const=None), "'spring_const' is missing"),
    (dict(rate=None), "exactly one of 'rate' and 'n_round'"),
    (dict(n_round=10), "exactly one of 'rate' and 'n_round'"),
    (dict(rate=None, n_round=0), 'n_round must be positive'),
    (dict(rate=None, n_round=-3), 'n_round must be positive'),
    (dict(center=np.nan), 'center is not finite'),
    (dict(rate=np.inf), 'rate is not finite'),
    (dict(center_end=-np.inf), 'center_end is not finite'),
    (dict(spring_const=np.nan), 'spring_const is not finite'),
    (dict(flat_width=np.inf), 'flat_width is not finite'),
    (dict(spring_const=-1.), 'spring_const must not be negative'),
    (dict(flat_width=-0.1), 'flat_width must not be negative'),
    (dict(rate=-0.05), 'center_end lies behind center'),
    (dict(center_end=5.), 'center_end lies behind center'),
    (dict(rate=0.), 'rate is 0 but center_end differs from center'),
    (dict(center=[1., 2.]), 'center must be one number'),
    (dict(pair=(1, 60)), 'out of range'),
    (dict(kind='angle'), 'unknown kind'),
])
def test_add_cv_steer_refuses(tmp_path, change, message):
    p = base_file(tmp_path)
    before = open(p, 'rb').read()
    sp = dict(GOOD, **change)
    sp = dict((k, v) for k, v in sp.items() if v is not None)
    with pytest.raises(ValueError) as err:
        cfg.add_cv_steer(p, [dict(GOOD, name='fine'), sp])
    assert message in str(err.value) and 'collective variable 1' in str(err.value), str(err.value)
    assert open(p, 'rb').read() == before      # a refusal writes nothing


def test_add_cv_steer_refuses_an_empty_list_and_a_foreign_name(tmp_path):
    p = base_file(tmp_path)
    with pytest.raises(ValueError, match='no collective variables'):
        cfg.add_cv_steer(p, [])
    with pytest.raises(ValueError, match="must start with 'cv_steer'"):
        cfg.add_cv_steer(p, [GOOD], name='pull')
    with pytest.raises(ValueError, match='65 collective variables exceed the limit of 64'):
        cfg.add_cv_steer(p, [dict(GOOD, name='d%d' % i) for i in range(65)])
    cfg.add_cv_steer(p, [dict(GOOD, rate=0., center_end=10.)])      # rate 0 with center_end == center: a cv_restraint


# ---- the library ---------------------------------------------------------------------------------------------------------------------
def test_node_type_is_registered_and_the_entry_points_are_exported(lib):
    import ctypes as ct
    c = lib.calc
    c.upside_hip_node_type_registered.argtypes = [ct.c_char_p]
    assert c.upside_hip_node_type_registered(b'cv_steer') == 1
    assert c.upside_hip_node_type_registered(b'cv_restraint') == 1 and c.upside_hip_node_type_registered(b'cv_steering_wheel') == 0
    engine_h = open(os.path.join(P.ROOT, 'include', 'upside_engine_c.h')).read()
    for n in ('upside_hip_steer_info', 'upside_hip_steer_read', 'upside_hip_steer_write', 'upside_hip_steer_values'):
        assert n + '(' in engine_h and hasattr(c, n), n
    kernels_h = open(os.path.join(P.ROOT, 'include', 'upside_hip_kernels.h')).read()
    for n in ('upk_cv_steer', 'upk_cv_steer_advance'):
        assert n + '(' in kernels_h and hasattr(c, n), n
    E = P.pkg.engine.Ensemble
    assert callable(E.steer_state) and callable(E.set_steer_state) and callable(E.steer_values)


def test_files_differing_in_the_five_values_share_one_group(lib, tmp_path):
    import hamiltonian_files as H
    base = base_file(tmp_path, 'base')
    cfg.add_cv_steer(base, steer_specs())
    outs = []
    for i in range(3):
        o = str(tmp_path / ('s%d.up' % i))
        shutil.copyfile(base, o)
        for k in cfg.CV_STEER_VALUES:
            H.rewrite(o, 'cv_steer', k, lambda v, i=i: (v * (1. + 0.1 * i)).astype('f4'))
        outs.append(o)
    groups = lambda paths: list(P.pkg.engine.group_configurations(paths, library=lib))
    assert groups(outs) == [0, 0, 0]
    other = str(tmp_path / 'other.up')
    shutil.copyfile(outs[1], other)
    H.rewrite(other, 'cv_steer', 'atoms', lambda v: v[::-1].copy())
    assert groups([outs[0], other, outs[2]]) == [0, 1, 0]
