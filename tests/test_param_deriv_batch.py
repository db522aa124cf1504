"""GPU tests of the batched parameter derivatives (upside_hip_get_param_deriv_all / _param_deriv_accumulate / _param_deriv_read
and the Ensemble methods over them): every system's table equals the per-system get_param_deriv, the systems at the golden
structure equal the reference's -DPARAM_DERIV build, the tables are bit-reproducible and independent of the rest of the batch,
and the device accumulator equals the float64 host sum."""
import ctypes as ct
import re
import numpy as np
import pytest
import parity_util as P

pytestmark = pytest.mark.gpu
FIXTURES = ['trpcage20_7A', 'proteinG56_7A', 'syn150_10A', 'syn300_10A', 'syn300_7A', 'proteinG56_restraints']


@pytest.fixture(scope='module')
def hip():
    import torch
    assert torch.cuda.is_available(), 'these tests need a GPU'
    lib = P.pkg.default_library()     # raises when the HIP extension is missing: no fallback
    c = lib.calc
    P.pkg.engine.Ensemble._bind(c)
    c.upside_hip_get_param_deriv.argtypes = [ct.c_void_p, ct.c_char_p, ct.c_int, ct.c_int, ct.c_void_p]
    c.upside_hip_last_error.restype = ct.c_char_p
    return lib


def n_param_of(ens, node):
    """the size the batched calls expect, from the error message of a request of the wrong size"""
    c = ens.calc
    assert c.upside_hip_get_param_deriv_all(ens.engine, node.encode(), -1, None) == 1
    m = re.search(r'expected (\d+)', c.upside_hip_last_error().decode())
    assert m, c.upside_hip_last_error()
    return int(m.group(1))


def potential_nodes(path):
    with P.pkg.h5lite.open_file(path) as t:
        return sorted(t.group('input/potential').keys())


def per_system(ens, node, s, shape):
    out = np.zeros(shape, 'f4')
    assert ens.calc.upside_hip_get_param_deriv(ens.engine, node.encode(), int(s), int(np.prod(shape)), out.ctypes.data) == 0
    return out


def md_frames(lib, name, n, seed=7):
    """n structures along a short trajectory from the fixture's structure (one replica per frame)"""
    g = P.golden(name)
    ens = P.pkg.engine.Ensemble(P.fixture(name), n, library=lib)
    ens.set_pos(g['pos'])
    ens.init_md(0.8, seed)
    ens.run_rounds(4)
    x = ens.get_pos()
    ens.close()
    return x


@pytest.mark.parametrize('name', FIXTURES)
def test_all_systems_match_per_system_and_golden(hip, name):
    g = P.golden(name)
    structs = [g['pos']] + ([g['pos2']] if 'pos2' in g else [])
    structs += list(md_frames(hip, name, 5 - len(structs)))
    x = np.stack(structs).astype('f4')
    ens = P.pkg.engine.Ensemble(P.fixture(name), 5, library=hip)
    ens.set_pos(x)
    ens.energies()
    checked = 0
    for node in potential_nodes(P.fixture(name)):
        n = n_param_of(ens, node)
        if n == 0:
            assert ens.param_deriv(node, ()).shape == (5,)
            continue
        key = 'param_deriv/' + node
        shape = g[key].shape if key in g else (n,)
        assert int(np.prod(shape)) == n, node
        allv = ens.param_deriv(node, shape)
        assert allv.shape == (5,) + shape
        for s in range(5):
            ref = per_system(ens, node, s, shape)
            if not np.any(ref):
                assert not np.any(allv[s]), (node, s)
            else:
                assert P.rel_rms(ref, allv[s]) <= 1e-6, (node, s, P.rel_rms(ref, allv[s]))
        if key in g:    # the system at `pos` against the reference (tolerances of test_param_derivs_match_reference_golden)
            if not np.any(g[key]):
                assert not np.any(allv[0]), node
            else:
                tol = 5e-5 if node.startswith('placement') else 1e-5
                assert P.rel_rms(g[key], allv[0]) <= tol, (node, P.rel_rms(g[key], allv[0]))
        checked += 1
    assert checked >= 3
    ens.close()


def test_tables_are_deterministic_and_independent_of_the_batch(hip):
    name = 'proteinG56_7A'
    g = P.golden(name)
    x = np.stack([g['pos'], g['pos2'], g['pos'], g['pos2'], g['pos']]).astype('f4')
    ens = P.pkg.engine.Ensemble(P.fixture(name), 5, library=hip)
    ens.set_pos(x)
    ens.energies()
    singles = {}
    for tag in ('pos', 'pos2'):
        one = P.pkg.engine.Ensemble(P.fixture(name), 1, library=hip)
        one.set_pos(g[tag])
        one.energies()
        singles[tag] = one
    nodes = [k.split('/', 1)[1] for k in g if k.startswith('param_deriv/')]
    assert 'rotamer' in nodes and len(nodes) >= 9
    for node in nodes:
        shape = g['param_deriv/' + node].shape
        a = ens.param_deriv(node, shape)
        b = ens.param_deriv(node, shape)
        assert a.tobytes() == b.tobytes(), node                       # run to run
        assert a[0].tobytes() == a[2].tobytes() == a[4].tobytes(), node
        assert a[1].tobytes() == a[3].tobytes(), node                 # whatever else shares the batch
        assert singles['pos'].param_deriv(node, shape)[0].tobytes() == a[0].tobytes(), node
        assert singles['pos2'].param_deriv(node, shape)[0].tobytes() == a[1].tobytes(), node
    for one in singles.values():
        one.close()
    ens.close()


def test_accumulate_and_read(hip):
    name = 'proteinG56_7A'
    g = P.golden(name)
    S = 4
    ens = P.pkg.engine.Ensemble(P.fixture(name), S, library=hip)
    ens.set_pos(g['pos'])
    ens.init_md(0.8, 11)
    nodes = {k.split('/', 1)[1]: g[k].shape for k in g if k.startswith('param_deriv/')}
    rs = np.random.RandomState(5)
    host = {n: np.zeros(shp, 'f8') for n, shp in nodes.items()}
    for _ in range(3):
        ens.run_steps(6)
        ens.energies()
        w = rs.uniform(-1.5, 1.5, size=S).astype('f4')
        for node, shp in nodes.items():
            ens.param_deriv_accumulate(node, w)
            d = ens.param_deriv(node, shp).astype('f8')
            for s in range(S):             # the device's order: systems ascending
                host[node] += np.float64(w[s]) * d[s]
    for node, shp in nodes.items():
        total, n_frame = ens.param_deriv_read(node, shp, reset=False)
        assert n_frame == 3, node
        scale = max(np.abs(host[node]).max(), 1e-30)
        assert np.abs(total - host[node]).max() <= 1e-12 * scale, (node, np.abs(total - host[node]).max() / scale)
        total2, n2 = ens.param_deriv_read(node, shp, reset=True)
        assert n2 == 3 and np.array_equal(total, total2)
        total3, n3 = ens.param_deriv_read(node, shp)
        assert n3 == 0 and not np.any(total3), node
    # NULL weights = all ones
    node, shp = 'rotamer', nodes['rotamer']
    ens.param_deriv_accumulate(node)
    t_none, _ = ens.param_deriv_read(node, shp)
    ens.param_deriv_accumulate(node, np.ones(S, 'f4'))
    t_ones, n = ens.param_deriv_read(node, shp)
    assert n == 1 and np.array_equal(t_none, t_ones)
    d = ens.param_deriv(node, shp).astype('f8')
    ref = np.zeros(shp, 'f8')
    for s in range(S):
        ref += d[s]
    assert np.array_equal(t_none, ref)
    ens.close()


def test_errors(hip):
    name = 'trpcage20_7A'
    ens = P.pkg.engine.Ensemble(P.fixture(name), 2, library=hip)
    ens.set_pos(P.golden(name)['pos'])
    ens.energies()
    c, e = ens.calc, ens.engine
    shp = P.golden(name)['param_deriv/rotamer'].shape
    n = int(np.prod(shp))
    buf = np.zeros((2, n), 'f4'); dbl = np.zeros(n, 'f8'); nf = np.zeros(1, 'i8')
    for call in (lambda: c.upside_hip_get_param_deriv_all(e, b'rotamer', n - 1, buf.ctypes.data),
                 lambda: c.upside_hip_param_deriv_read(e, b'rotamer', n + 1, dbl.ctypes.data, nf.ctypes.data, 0)):
        assert call() == 1
        assert b'expected %d' % n in c.upside_hip_last_error()
    for call in (lambda: c.upside_hip_get_param_deriv_all(e, b'no_such_node', n, buf.ctypes.data),
                 lambda: c.upside_hip_param_deriv_accumulate(e, b'no_such_node', None),
                 lambda: c.upside_hip_param_deriv_read(e, b'no_such_node', n, dbl.ctypes.data, nf.ctypes.data, 0)):
        assert call() == 1
        assert b'not found' in c.upside_hip_last_error()
    for call in (lambda: c.upside_hip_get_param_deriv_all(e, b'rotamer', n, None),
                 lambda: c.upside_hip_param_deriv_read(e, b'rotamer', n, None, nf.ctypes.data, 0)):
        assert call() == 1
        assert b'NULL' in c.upside_hip_last_error()
    with pytest.raises(RuntimeError):
        ens.param_deriv('rotamer', (n + 1,))
    # a node without a derivative: n_param = 0, nothing to do
    assert c.upside_hip_get_param_deriv_all(e, b'protein_hbond', 0, None) == 0
    assert c.upside_hip_param_deriv_accumulate(e, b'protein_hbond', None) == 0
    assert c.upside_hip_param_deriv_read(e, b'protein_hbond', 0, None, nf.ctypes.data, 1) == 0 and nf[0] == 1
    assert c.upside_hip_get_param_deriv_all(e, b'protein_hbond', 1, buf.ctypes.data) == 1
    ens.close()


def test_batch_of_512_crosses_the_large_solve_path(hip):
    name = 'syn300_10A'
    g = P.golden(name)
    S = 512
    ens = P.pkg.engine.Ensemble(P.fixture(name), S, library=hip)
    rs = np.random.RandomState(2)
    x = g['pos'][None] + np.float32(0.05) * rs.normal(size=(S,) + g['pos'].shape).astype('f4')
    ens.set_pos(x)
    ens.energies()
    for node in ('rotamer', 'hbond_coverage'):
        shape = g['param_deriv/' + node].shape
        allv = ens.param_deriv(node, shape)
        for s in (0, 255, 511):
            ref = per_system(ens, node, s, shape)
            assert P.rel_rms(ref, allv[s]) <= 1e-6, (node, s, P.rel_rms(ref, allv[s]))
    ens.close()
