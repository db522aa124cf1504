"""CPU checks of the cv_restraint node's surroundings: the float64 yardstick tests/cv_restraint_reference.py pinned against central
differences of its own energy, the configuration writers (config.add_cv_restraint, config.write_umbrella_windows), the grouping
of window files into one engine (HDF5 only) and the C-ABI.  No GPU."""
import os
import shutil
import numpy as np
import pytest
import parity_util as P
import cv_reference as R
import cv_restraint_reference as Y
import cv_restraint_cases as K

cfg = P.pkg.config
VALUES = ('center', 'spring_const', 'flat_width')


@pytest.fixture(scope='module')
def lib():
    if not os.path.exists(P.pkg.PRODUCT_LIB):
        pytest.fail('libupside_hip.so not built (run __graft_entry__.build())')
    return P.pkg.UpsideLibrary(P.pkg.PRODUCT_LIB)


def read_node(path, name='cv_restraint'):
    with P.pkg.h5lite.open_file(path) as t:
        g = t.group('input/potential/' + name)
        return dict((k, g.read(k)) for k in g.keys()), [x.decode() if isinstance(x, bytes) else x for x in np.asarray(g.get_attr('arguments')).ravel()]


# ---- the yardstick -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['trpcage20_7A', 'syn300_10A'])
def test_yardstick_gradient_matches_central_differences(name):
    """every kind, all atoms and CA only, flat-bottom CVs inside and outside the flat region; bound 1e-6 of the largest element"""
    x = K.perturbed(name)
    specs = K.force_specs(name, x)
    inside = K.inside_flat(specs, x)
    assert inside.any() and (~inside).any()
    for c, sp in enumerate(specs):
        e, g, _ = Y.energy_and_gradient([sp], x)
        if inside[c]:
            assert e == 0. and not g.any(), sp['name']
        else:
            assert e > 0. and g.any(), sp['name']
    e, g, v = Y.energy_and_gradient(specs, x)
    assert np.allclose(v, R.evaluate(specs, x), rtol=0, atol=0)
    num = Y.numeric_gradient(specs, x, 1e-5)
    err = np.abs(g - num).max() / np.abs(num).max()
    print('%s: E %.6f, max |analytic - numeric| / max |numeric| = %.3e' % (name, e, err))
    assert err <= 1e-6
    for sp in specs:      # and each CV on its own (a wrong gradient of a small term would hide in the sum)
        if sp['name'] in ('rg_255', 'rg_257'):
            continue
        g1 = Y.energy_and_gradient([sp], x)[1]
        if not g1.any():
            continue
        touched = np.unique(np.nonzero(g1)[0])[:40]
        n1 = _numeric_rows([sp], x, touched)
        err1 = np.abs(g1[touched] - n1).max() / np.abs(n1).max()
        print('  %-10s %.3e' % (sp['name'], err1))
        assert err1 <= 1e-6, sp['name']


def _numeric_rows(specs, x, rows, h=1e-5):
    x = np.array(x, 'f8'); out = np.zeros((len(rows), 3))
    for j, i in enumerate(rows):
        for d in range(3):
            x0 = x[i, d]
            x[i, d] = x0 + h; ep = Y.energy(specs, x)
            x[i, d] = x0 - h; em = Y.energy(specs, x)
            x[i, d] = x0
            out[j, d] = (ep - em) / (2. * h)
    return out


def test_yardstick_small_values_give_zero_force_and_keep_the_energy():
    x = np.zeros((4, 3)); x[3] = (1., 2., 3.)
    for sp in ({'kind': 'rg', 'atoms': [0, 1, 2]}, {'kind': 'distance', 'pair': (0, 1)},
               {'kind': 'rmsd', 'atoms': [0, 1, 2], 'ref': np.zeros((3, 3))},
               {'kind': 'contacts', 'pairs': [(0, 1)], 'r0': 1., 'beta': 5., 'lambda': 1.}):
        sp = dict(sp, center=2., spring_const=3.)
        e, g, v = Y.energy_and_gradient([sp], x)
        assert not g.any() and np.isfinite(e) and e > 0., sp['kind']


# ---- the writers -------------------------------------------------------------------------------------------------------------------
def base_file(tmp_path, name='proteinG56_7A', tag='base'):
    p = str(tmp_path / (tag + '.up'))
    shutil.copyfile(P.fixture(name), p)
    return p


def small_specs(pos):
    ca = np.arange(1, len(pos), 3, dtype='i4')
    pairs, r0 = cfg.native_contacts(pos, ca)
    return [{'name': 'rmsd_ca', 'kind': 'rmsd', 'atoms': ca, 'ref': pos[ca], 'center': 2., 'spring_const': 5.},
            {'name': 'q', 'kind': 'contacts', 'pairs': pairs, 'r0': r0, 'beta': 5., 'lambda': 1.8, 'center': 0.5, 'spring_const': 200., 'flat_width': 0.05},
            {'name': 'rmsd_n', 'kind': 'rmsd', 'atoms': ca[:7], 'ref': pos[ca[:7]] + 1., 'center': 1., 'spring_const': 0.},
            {'name': 'rg', 'kind': 'rg', 'atoms': ca, 'center': 10., 'spring_const': 1., 'flat_width': 0.5},
            {'name': 'ee', 'kind': 'distance', 'pair': (int(ca[0]), int(ca[-1])), 'center': 12., 'spring_const': 0.3}]


def test_add_cv_restraint_round_trips(tmp_path):
    pos = K.coords('proteinG56_7A')
    p = base_file(tmp_path)
    specs = small_specs(pos)
    packed = cfg.add_cv_restraint(p, specs)
    d, args = read_node(p)
    assert args == ['pos']
    n_ca = len(pos) // 3
    n_pair = len(specs[1]['pairs'])
    assert d['kind'].dtype == np.int32 and list(d['kind']) == [1, 2, 1, 0, 3]
    assert d['atom_start'].dtype == np.int32 and list(d['atom_start']) == [0, n_ca, n_ca + 2 * n_pair, n_ca + 2 * n_pair + 7, 2 * n_ca + 2 * n_pair + 7, 2 * n_ca + 2 * n_pair + 9]
    assert d['atoms'].dtype == np.int32 and len(d['atoms']) == d['atom_start'][-1]
    assert d['ref_pos'].dtype == np.float32 and d['ref_pos'].shape == (n_ca + 7, 3)       # the two rmsd references back to back
    assert np.array_equal(d['ref_pos'][n_ca:], (pos[np.arange(1, 21, 3)] + 1.).astype('f4'))
    assert d['contact_r0'].dtype == np.float32 and d['contact_r0'].shape == (n_pair,)
    assert list(d['contact_beta']) == [0., 5., 0., 0., 0.] and np.allclose(d['contact_lambda'], [0., 1.8, 0., 0., 0.])
    assert [x.decode() for x in d['names']] == ['rmsd_ca', 'q', 'rmsd_n', 'rg', 'ee']
    for k, want in zip(VALUES, ([2., 0.5, 1., 10., 12.], [5., 200., 0., 1., 0.3], [0., 0.05, 0., 0.5, 0.])):
        assert d[k].dtype == np.float32 and np.array_equal(d[k], np.asarray(want, 'f4')), k
        assert np.array_equal(packed[k], d[k])
    # a second node coexists; writing a node again replaces it
    cfg.add_cv_restraint(p, specs[3:4], name='cv_restraint_rg')
    cfg.add_cv_restraint(p, specs[:2])
    assert len(read_node(p, 'cv_restraint_rg')[0]['kind']) == 1 and len(read_node(p)[0]['kind']) == 2


@pytest.mark.parametrize('change,message', [
    (lambda s: s[0].update(kind='angle'), 'unknown kind'),
    (lambda s: s[0].update(atoms=np.array([1, 4, 168], 'i4'), ref=np.zeros((3, 3))), 'atom 168 out of range'),
    (lambda s: s[0].update(atoms=np.array([1, 4], 'i4'), ref=np.zeros((2, 3))), 'an rmsd selection needs at least 3 atoms'),
    (lambda s: s[4].update(pair=(1, 4, 7)), 'pair must hold exactly 2 atoms'),
    (lambda s: s[1].update(pairs=np.arange(9).reshape(3, 3)), 'pairs must be (m, 2)'),
    (lambda s: s[0].pop('center'), "'center' is missing"),
    (lambda s: s[0].pop('spring_const'), "'spring_const' is missing"),
    (lambda s: s[0].update(spring_const=-1.), 'spring_const must not be negative'),
    (lambda s: s[0].update(spring_const=float('nan')), 'spring_const is not finite'),
    (lambda s: s[0].update(flat_width=-0.1), 'flat_width must not be negative'),
    (lambda s: s[0].update(flat_width=float('inf')), 'flat_width is not finite'),
    (lambda s: s[0].update(center=float('nan')), 'center is not finite'),
    (lambda s: s[0].update(center=[1., 2.]), 'center must be one number'),
])
def test_add_cv_restraint_refusals(tmp_path, change, message):
    p = base_file(tmp_path)
    specs = small_specs(K.coords('proteinG56_7A'))
    change(specs)
    before = open(p, 'rb').read()
    with pytest.raises(ValueError) as err:
        cfg.add_cv_restraint(p, specs)
    assert message in str(err.value), str(err.value)
    assert open(p, 'rb').read() == before      # a refusal writes nothing


def test_add_cv_restraint_refuses_too_many_an_empty_list_and_a_foreign_name(tmp_path):
    p = base_file(tmp_path)
    one = {'kind': 'distance', 'pair': (1, 4), 'center': 3., 'spring_const': 1.}
    with pytest.raises(ValueError, match='65 collective variables exceed the limit of 64'):
        cfg.add_cv_restraint(p, [dict(one, name='d%d' % i) for i in range(65)])
    with pytest.raises(ValueError, match='no collective variables'):
        cfg.add_cv_restraint(p, [])
    with pytest.raises(ValueError, match="must start with 'cv_restraint'"):
        cfg.add_cv_restraint(p, [one], name='umbrella')


def windows(tmp_path, n, base=None):
    pos = K.coords('proteinG56_7A')
    base = base or base_file(tmp_path)
    cfg.add_cv_restraint(base, small_specs(pos)[:2])
    outs = [str(tmp_path / ('w%d.up' % i)) for i in range(n)]
    i = np.arange(n)
    cfg.write_umbrella_windows(base, outs, 'cv_restraint', np.column_stack((1. + 0.5 * i, 0.2 + 0.1 * i)),
                               np.column_stack((5. + i, 100. + 20. * i)), np.column_stack((0.1 * i, 0.01 * i)))
    return base, outs


def all_datasets(path):
    out = {}
    with P.pkg.h5lite.open_file(path) as t:
        def walk(g, prefix):
            for k in g.keys():
                if g.is_group(k):
                    walk(g.group(k), prefix + k + '/')
                else:
                    out[prefix + k] = g.read(k)
        walk(t, '/')
    return out


def test_write_umbrella_windows_changes_only_the_three_datasets(tmp_path):
    base, outs = windows(tmp_path, 3)
    d0 = all_datasets(base)
    for i, p in enumerate(outs):
        d = all_datasets(p)
        assert sorted(d) == sorted(d0)
        changed = sorted(k for k in d0 if d[k].dtype != d0[k].dtype or d[k].shape != d0[k].shape or d[k].tobytes() != d0[k].tobytes())
        assert changed == sorted('/input/potential/cv_restraint/' + k for k in VALUES), (i, changed)
        g = read_node(p)[0]
        assert np.array_equal(g['center'], np.asarray([1. + 0.5 * i, 0.2 + 0.1 * i], 'f4')) and g['center'].dtype == np.float32
        assert np.array_equal(g['spring_const'], np.asarray([5. + i, 100. + 20. * i], 'f4'))
        assert np.array_equal(g['flat_width'], np.asarray([0.1 * i, 0.01 * i], 'f4'))
    keep = [str(tmp_path / 'k.up')]
    cfg.write_umbrella_windows(base, keep, 'cv_restraint', [[3., 0.4]])       # None keeps the base file's values
    assert np.array_equal(read_node(keep[0])[0]['spring_const'], read_node(base)[0]['spring_const'])
    with pytest.raises(ValueError, match='must be \\(2 windows, 2 CVs\\)'):
        cfg.write_umbrella_windows(base, outs[:2], 'cv_restraint', [1., 2., 3.])
    with pytest.raises(ValueError, match='spring_const must not be negative'):
        cfg.write_umbrella_windows(base, outs[:1], 'cv_restraint', [[1., 2.]], [[-1., 2.]])
    with pytest.raises(ValueError, match="has no node 'cv_restraint_x'"):
        cfg.write_umbrella_windows(base, outs[:1], 'cv_restraint_x', [[1., 2.]])


# ---- grouping (HDF5 only) ----------------------------------------------------------------------------------------------------------
def test_windows_share_one_group_and_a_changed_definition_does_not(lib, tmp_path):
    import hamiltonian_files as H
    base, outs = windows(tmp_path, 5)
    groups = lambda paths: list(P.pkg.engine.group_configurations(paths, library=lib))
    assert groups(outs) == [0] * 5
    for j, (name, fn) in enumerate((('atoms', lambda v: v[::-1].copy()), ('ref_pos', lambda v: v + 0.25))):
        other = str(tmp_path / ('other_%s.up' % name))
        shutil.copyfile(outs[1], other)
        H.rewrite(other, 'cv_restraint', name, fn)
        assert groups([outs[0], other, outs[2]]) == [0, 1, 0], name


# ---- ABI ---------------------------------------------------------------------------------------------------------------------------
def test_restraint_values_is_declared_exported_and_bound(lib):
    txt = open(os.path.join(P.ROOT, 'include', 'upside_engine_c.h')).read()
    n = 'upside_hip_cv_restraint_values'
    assert n + '(' in txt, n
    assert hasattr(lib.calc, n), n
    assert 'upk_cv_restraint(' in open(os.path.join(P.ROOT, 'include', 'upside_hip_kernels.h')).read()
    assert callable(P.pkg.engine.Ensemble.restraint_values)
    assert callable(cfg.add_cv_restraint) and callable(cfg.write_umbrella_windows)
