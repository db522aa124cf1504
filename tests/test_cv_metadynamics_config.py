"""CPU checks of the cv_metadynamics node's surroundings: the float64 yardstick tests/cv_metad_reference.py pinned against central
differences of its own energy, the configuration writers (config.add_cv_metadynamics, config.set_metadynamics_hills) with their
refusals, config.metadynamics_free_energy on a hand-computed case, and the C-ABI names.  No GPU."""
import ctypes as ct
import os
import shutil
import numpy as np
import pytest
import parity_util as P
import cv_restraint_cases as K
import cv_metad_reference as Y
import cv_metad_cases as M

cfg = P.pkg.config
NODE = 'cv_metadynamics'


# ---- the yardstick -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('d', [1, 2, 3])
def test_yardstick_gradient_matches_central_differences(d):
    """trpcage20, 7 random hills within +-2 sigma of the current values; bound 1e-6 of the largest element"""
    x = K.perturbed(M.NAME)
    specs = M.specs_of(d)
    v = Y.values(specs, x)
    sigma = M.sigma_of(v)
    centers, weights = M.random_hills(v, sigma, 7, 100 + d)
    e, g, v2 = Y.energy_and_gradient(specs, x, centers, weights, sigma)
    assert np.array_equal(v, v2) and e > 0. and g.any()
    num = Y.numeric_gradient(specs, x, centers, weights, sigma, 1e-5)
    err = np.abs(g - num).max() / np.abs(num).max()
    print('d = %d: V %.6f, max |analytic - numeric| / max |numeric| = %.3e' % (d, e, err))
    assert err <= 1e-6


def test_yardstick_bias_of_one_hill_by_hand():
    """one hill of weight 2 at the origin of a 2-d space, sigma (1, 2), at the point (1, 2): exponent -(1/2 + 1/2) = -1"""
    e, dv = Y.bias([1., 2.], [[0., 0.]], [2.], [1., 2.])
    assert abs(e - 2. * np.exp(-1.)) < 1e-15
    assert np.allclose(dv, [-2. * np.exp(-1.) * 1. / 1., -2. * np.exp(-1.) * 2. / 4.], rtol=1e-15, atol=0)
    assert Y.bias([1., 2.], np.zeros((0, 2)), [], [1., 2.])[0] == 0.


# ---- the writers -------------------------------------------------------------------------------------------------------------------
def base_file(tmp_path, tag='base'):
    p = str(tmp_path / (tag + '.up'))
    shutil.copyfile(P.fixture(M.NAME), p)
    return p


def test_add_cv_metadynamics_and_hills_round_trip(tmp_path):
    p = base_file(tmp_path)
    specs = M.specs_of(2)
    packed = cfg.add_cv_metadynamics(p, specs, [0.5, 0.05], 0.3, 4, 100, kdT=2.5, shared=True, name=NODE + '_a')
    ref = cfg.pack_collective_variables(specs, 60)
    node, args, attrs = read_node(p, NODE + '_a')
    assert args == ['pos']
    for k in ('kind', 'atom_start', 'atoms', 'ref_pos', 'contact_r0', 'contact_beta', 'contact_lambda'):
        assert np.array_equal(node[k], ref[k]) and np.array_equal(packed[k], ref[k]), k
    assert node['sigma'].dtype == np.float32 and np.array_equal(node['sigma'], np.array([0.5, 0.05], 'f4'))
    assert attrs == dict(height=0.3, kdT=2.5, pace=4, capacity=100, shared=1)
    # a second call under the same name replaces the node; the defaults are plain and unshared
    cfg.add_cv_metadynamics(p, M.specs_of(1), [0.7], 1., 1, 5, name=NODE + '_a')
    node, args, attrs = read_node(p, NODE + '_a')
    assert len(node['kind']) == 1 and attrs == dict(height=1., kdT=0., pace=1, capacity=5, shared=0)
    # hills: outside /input/potential, rewritten whole
    before = cfg_digest(p)
    c = np.array([[1.5], [2.5], [3.5]]); w = np.array([0.25, 0.5, 1.])
    cfg.set_metadynamics_hills(p, NODE + '_a', c, w)
    cfg.set_metadynamics_hills(p, NODE + '_a', c[:2, 0], w[:2])      # (n,) for d = 1
    hc, hw = read_hills(p, NODE + '_a')
    assert hc.dtype == np.float32 and hw.dtype == np.float32 and hc.shape == (2, 1) and np.array_equal(hc[:, 0], [1.5, 2.5]) and np.array_equal(hw, [0.25, 0.5])
    assert cfg_digest(p) == before      # /input/potential is untouched
    cfg.set_metadynamics_hills(p, NODE + '_a', np.zeros((0, 1)), [])
    assert read_hills(p, NODE + '_a')[1].shape == (0,)


def read_node(path, name):
    """(datasets, arguments, numeric attributes) of a potential node; every handle is released on return"""
    with P.pkg.h5lite.open_file(path) as t:
        g = t.group('input/potential/' + name)
        one = lambda a: np.asarray(g.get_attr(a)).ravel()[0]
        attrs = dict((a, float(one(a))) for a in ('height', 'kdT'))
        attrs.update((a, int(one(a))) for a in ('pace', 'capacity', 'shared'))
        return (dict((k, g.read(k)) for k in g.keys()), [x.decode() if isinstance(x, bytes) else x for x in np.asarray(g.get_attr('arguments')).ravel()], attrs)


def read_hills(path, name):
    with P.pkg.h5lite.open_file(path) as t:
        g = t.group('input/metadynamics/' + name)
        return g.read('hill_center'), g.read('hill_weight')


def cfg_digest(path):
    """the node names of /input/potential and the bytes of the metadynamics node's datasets"""
    with P.pkg.h5lite.open_file(path) as t:
        names = sorted(t.group('input/potential').keys())
    node = read_node(path, NODE + '_a')
    return names, sorted((k, np.asarray(v).tobytes()) for k, v in node[0].items()), node[1], node[2]


REFUSALS = [
    ('name', dict(name='metadynamics'), "must start with 'cv_metadynamics'"),
    ('no CVs', dict(specs=[]), 'no collective variables'),
    ('d = 5', dict(specs='five', sigma=[1.] * 5), 'limit of 4'),
    ('a spec that is no dict', dict(specs=['rg']), "a dict with a 'kind' is expected"),
    ('short sigma', dict(sigma=[1.]), 'sigma holds 1 entries'),
    ('sigma = 0', dict(sigma=[1., 0.]), 'sigma must be finite and positive'),
    ('sigma < 0', dict(sigma=[-1., 1.]), 'sigma must be finite and positive'),
    ('sigma not finite', dict(sigma=[np.inf, 1.]), 'sigma must be finite and positive'),
    ('height = 0', dict(height=0.), 'height must be finite and positive'),
    ('height not finite', dict(height=np.nan), 'height must be finite and positive'),
    ('kdT < 0', dict(kdT=-1.), 'kdT must be finite and not negative'),
    ('pace = 0', dict(pace=0), 'pace must be'),
    ('pace = 1.5', dict(pace=1.5), 'pace must be'),
    ('capacity = 0', dict(capacity=0), 'capacity must be'),
    ('capacity too large', dict(capacity=(1 << 24) + 1), 'capacity must be'),
    ('atom out of range', dict(specs=[{'kind': 'rg', 'atoms': [0, 60]}, {'kind': 'distance', 'pair': (0, 1)}]), 'out of range'),
]


@pytest.mark.parametrize('what,change,needle', REFUSALS, ids=[r[0] for r in REFUSALS])
def test_add_cv_metadynamics_refuses(tmp_path, what, change, needle):
    """every refusal of the writer, by its message; the file is left as it was"""
    p = base_file(tmp_path)
    before = open(p, 'rb').read()
    kw = dict(specs=M.specs_of(2), sigma=[0.5, 0.05], height=0.3, pace=2, capacity=10, kdT=0., name=NODE)
    kw.update(change)
    if kw['specs'] == 'five':
        kw['specs'] = M.specs_of(4) + M.specs_of(1)
    with pytest.raises(ValueError) as err:
        cfg.add_cv_metadynamics(p, kw.pop('specs'), kw.pop('sigma'), kw.pop('height'), kw.pop('pace'), kw.pop('capacity'), **kw)
    assert needle in str(err.value), str(err.value)
    assert open(p, 'rb').read() == before


def test_set_metadynamics_hills_refuses(tmp_path):
    p = base_file(tmp_path)
    cfg.add_cv_metadynamics(p, M.specs_of(2), [0.5, 0.05], 0.3, 2, 3)
    before = open(p, 'rb').read()
    for c, w, node, needle in ((np.zeros((2, 2)), [1., 1.], 'cv_metadynamics_x', 'has no node'),
                               (np.zeros((2, 3)), [1., 1.], NODE, 'centers must be (2 hills, 2 CVs)'),
                               (np.zeros((2, 2)), [1.], NODE, 'centers must be (1 hills, 2 CVs)'),
                               (np.zeros((4, 2)), [1.] * 4, NODE, '4 hills exceed the capacity of 3'),
                               (np.array([[0., np.nan]]), [1.], NODE, 'must be finite'),
                               (np.zeros((1, 2)), [np.inf], NODE, 'must be finite')):
        with pytest.raises(ValueError) as err:
            cfg.set_metadynamics_hills(p, node, c, w)
        assert needle in str(err.value), str(err.value)
    assert open(p, 'rb').read() == before


# ---- the free-energy estimate ------------------------------------------------------------------------------------------------------
def test_free_energy_of_two_hills_by_hand():
    """d = 1, sigma 2, hills of weight 1 at 0 and 3 at 4, read at 0, 2 and 4:
       V(0) = 1 + 3 exp(-2), V(2) = exp(-1/2) + 3 exp(-1/2), V(4) = exp(-2) + 3"""
    v = np.array([1. + 3. * np.exp(-2.), 4. * np.exp(-0.5), np.exp(-2.) + 3.])
    f = cfg.metadynamics_free_energy([[0.], [4.]], [1., 3.], [2.], [0., 2., 4.])
    assert f.dtype == np.float64 and np.allclose(f, -v, rtol=1e-15, atol=0)
    f = cfg.metadynamics_free_energy([0., 4.], [1., 3.], [2.], np.array([[0.], [2.], [4.]]), kT=0.8, kdT=2.4)
    assert np.allclose(f, -(0.8 + 2.4) / 2.4 * v, rtol=1e-15, atol=0)
    # d = 2: one hill, exponent -(1/2 + 1/2)
    f = cfg.metadynamics_free_energy([[0., 0.]], [2.], [1., 2.], [[1., 2.]])
    assert np.allclose(f, [-2. * np.exp(-1.)], rtol=1e-15, atol=0)
    assert np.array_equal(cfg.metadynamics_free_energy(np.zeros((0, 1)), [], [1.], [0., 1.]), [0., 0.])
    with pytest.raises(ValueError):
        cfg.metadynamics_free_energy([[0.]], [1.], [1.], [0.], kdT=1.)      # well-tempered needs kT
    with pytest.raises(ValueError):
        cfg.metadynamics_free_energy([[0.]], [1.], [1., 1.], [0.])


# ---- the library -------------------------------------------------------------------------------------------------------------------
def test_library_exports_the_metadynamics_entry_points_and_registers_the_node():
    if not os.path.exists(P.pkg.PRODUCT_LIB):
        pytest.fail('libupside_hip.so not built (run __graft_entry__.build())')
    lib = ct.CDLL(P.pkg.PRODUCT_LIB)      # (loading runs the registry's prefix-collision check of every built-in type)
    for n in ('upside_hip_metad_info', 'upside_hip_metad_read', 'upside_hip_metad_write', 'upside_hip_metad_values', 'upk_cv_metad', 'upk_cv_metad_deposit'):
        assert hasattr(lib, n), n
    lib.upside_hip_node_type_registered.argtypes = [ct.c_char_p]
    assert lib.upside_hip_node_type_registered(b'cv_metadynamics') == 1 and lib.upside_hip_node_type_registered(b'cv_restraint') == 1
