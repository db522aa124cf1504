"""GPU tests of Hamiltonian ladders in one engine (upside_hip_construct_files, per-system set_param, upside_hip_hamiltonian_swap
and upside_main over them): every system computes what an engine of its own file computes, identical files stay bit for bit
what upside_hip_construct computes, the device swap set reaches the verdicts of the host procedure, and upside_main matches
the unmodified reference executable."""
import os
import subprocess
import sys
import numpy as np
import pytest
import parity_util as P
import hamiltonian_files as H

pytestmark = pytest.mark.gpu
E = P.pkg.engine


@pytest.fixture(scope='module')
def lib():
    import torch
    assert torch.cuda.is_available(), 'these tests need a GPU'
    import ctypes as ct
    lib = P.pkg.default_library()
    E.Ensemble._bind(lib.calc)
    lib.calc.upside_hip_swap_between.argtypes = [ct.c_void_p, ct.c_int, ct.c_void_p, ct.c_int]
    lib.calc.upside_replica_decide_lboltz.argtypes = [ct.c_int, ct.c_void_p, ct.c_uint32, ct.c_uint64, ct.c_int, ct.c_void_p]
    return lib


def ladder(tmp_path, base, n, change, tag='w'):
    fs = []
    for i in range(n):
        f = H.copy_fixture(base, tmp_path / ('%s%d.up' % (tag, i)))
        change(f, i)
        fs.append(f)
    return fs


def test_per_system_values_match_separate_engines(lib, tmp_path):
    """eight windows varying every row of the table at once (AFM included).  Against an engine of 8 copies of window i
    (the same batch size and code path: bitwise) and against construct_deriv_engine on window i alone (1e-6 relative)"""
    fs = ladder(tmp_path, 'proteinG56_restraints', 8, H.vary_table)
    pos = P.golden('proteinG56_restraints')['pos'].astype('f4')
    big = E.Ensemble.from_files(fs, library=lib)
    big.set_pos(pos)
    e, d = big.energies_and_derivs()
    assert len(set(np.round(e, 3))) == 8             # the windows really differ
    for i, f in enumerate(fs):
        same = E.Ensemble(f, 8, library=lib)
        same.set_pos(pos)
        e8, d8 = same.energies_and_derivs()
        assert e8[i] == e[i], (i, e8[i], e[i])
        assert np.array_equal(d8[i], d[i]), i
        same.close()
        up = P.pkg.Upside(f)
        e1 = float(np.asarray(up.energy(pos)).ravel()[0]); d1 = up.deriv(pos)
        up.close()
        assert abs(e1 - e[i]) <= 1e-6 * max(1., abs(e1)), (i, e1, e[i])
        assert P.rel_rms(d1, d[i]) < 1e-6, i
    big.close()


def test_identical_files_are_bitwise_construct(lib):
    n = 4
    f = P.fixture('proteinG56_restraints')
    pos = P.golden('proteinG56_restraints')['pos'].astype('f4')
    a = E.Ensemble.from_files([f] * n, library=lib); b = E.Ensemble(f, n, library=lib)
    for x in (a, b):
        x.set_pos(pos)
    ea, da = a.energies_and_derivs(); eb, db = b.energies_and_derivs()
    assert np.array_equal(ea, eb) and np.array_equal(da, db)
    for x in (a, b):
        x.init_md([0.8, 0.85, 0.9, 0.95], 13)
        x.run_steps(30)
    assert np.array_equal(a.get_pos(), b.get_pos())
    assert np.array_equal(a.get_mom(), b.get_mom())
    a.close(); b.close()


@pytest.mark.parametrize('node,dataset', [('dist_spring', 'id'), ('rama_map_pot', 'rama_pot')])
def test_refusal_names_node_and_dataset(lib, tmp_path, node, dataset):
    base = H.copy_fixture('proteinG56_restraints', tmp_path / 'a.up')
    other = H.copy_fixture('proteinG56_restraints', tmp_path / 'b.up')
    H.rewrite(other, node, dataset, lambda v: v[::-1].copy() if dataset == 'id' else v * 1.01)
    with pytest.raises(RuntimeError) as err:
        E.Ensemble.from_files([base, other], library=lib)
    msg = str(err.value)
    assert node in msg and dataset in msg and 'b.up' in msg, msg


def test_set_param_system_equals_file_ladder(lib, tmp_path):
    n = 6
    scales = [1. - 0.04 * i for i in range(n)]
    fs = ladder(tmp_path, 'proteinG56_7A', n, lambda f, i: H.scale_hbond(f, scales[i]))
    pos = P.golden('proteinG56_7A')['pos'].astype('f4')
    files = E.Ensemble.from_files(fs, library=lib)
    files.set_pos(pos)
    ef, df = files.energies_and_derivs()
    base = float(files.get_param((1,), 'hbond_energy', system=0)[0])
    copies = E.Ensemble.from_files([P.fixture('proteinG56_7A')] * n, library=lib)
    copies.set_pos(pos)
    for i in range(n):
        copies.set_param([files.get_param((1,), 'hbond_energy', system=i)[0]], 'hbond_energy', system=i)
        assert copies.get_param((1,), 'hbond_energy', system=i)[0] == files.get_param((1,), 'hbond_energy', system=i)[0]
    ec, dc = copies.energies_and_derivs()
    assert np.array_equal(ec, ef) and np.array_equal(dc, df)
    assert len(set(ec.tolist())) == n
    # each system's parameter derivative is taken at its own values
    for node in ('hbond_energy', 'rotamer'):
        singles = []
        for i, f in enumerate(fs):
            one = E.Ensemble(f, 1, library=lib)
            one.set_pos(pos); one.energies()
            shape = _param_shape(one, node)
            singles.append(one.param_deriv(node, shape)[0])
            one.close()
        files.energies()
        got = files.param_deriv(node, shape)
        for i in range(n):
            assert P.rel_rms(singles[i], got[i]) < 1e-6, (node, i)
    # set_param afterwards: every system again
    copies.set_param([base], 'hbond_energy')
    e_all = copies.energies()
    assert np.all(e_all == e_all[0])
    assert copies.get_param((1,), 'hbond_energy', system=n - 1)[0] == np.float32(base)
    files.close(); copies.close()


def _param_shape(ens, node):
    import re
    c = ens.calc
    assert c.upside_hip_get_param_deriv_all(ens.engine, node.encode(), -1, None) == 1
    return (int(re.search(r'expected (\d+)', c.upside_hip_last_error().decode()).group(1)),)


def test_device_swap_matches_host_procedure(lib, tmp_path):
    """a 16-window hbond_energy ladder with a temperature ladder on top: upside_hip_hamiltonian_swap against
    upside_hip_swap_between + upside_replica_decide_lboltz on the same state, several rounds, both swap sets"""
    n = 16
    fs = ladder(tmp_path, 'proteinG56_7A', n, lambda f, i: H.scale_hbond(f, 1. - 0.01 * i))
    temps = np.linspace(0.80, 0.90, n).astype('f4')
    dev = E.Ensemble.from_files(fs, library=lib); host = E.Ensemble.from_files(fs, library=lib)
    c = lib.calc
    for x in (dev, host):
        x.set_pos(P.golden('proteinG56_7A')['pos'])
        x.init_md(temps, 17)
    sets = [np.array([[i, i + 1] for i in range(0, n, 2)]), np.array([[i, i + 1] for i in range(1, n - 1, 2)])]
    seen = set()
    for rnd in range(1, 7):
        dev.run_steps(6)
        host.set_pos(dev.get_pos())
        draw = 0
        for k, st in enumerate(sets):
            acc, nxt = dev.hamiltonian_swap(st, 101, rnd, draw0=draw, want_accepted=True)
            old = -(1. / temps) * host.energies()
            for a, b in st:
                assert c.upside_hip_swap_between(host.engine, int(a), host.engine, int(b)) == 0
            new = -(1. / temps) * host.energies()
            diff = np.array([(new[a] + new[b]) - (old[a] + old[b]) for a, b in st], 'f4')
            href = np.zeros(len(st) + 1, 'i4')
            assert c.upside_replica_decide_lboltz(len(st), diff.ctypes.data, 101, rnd, draw, href.ctypes.data) == 0
            for p, (a, b) in enumerate(st):
                if not href[p]:
                    assert c.upside_hip_swap_between(host.engine, int(a), host.engine, int(b)) == 0
            assert np.array_equal(acc, href[:-1].astype(bool)), (rnd, k, acc, href)
            assert nxt == href[-1]
            assert np.array_equal(dev.get_pos(), host.get_pos())
            seen.update(acc.tolist())
            draw = nxt
    assert seen == {True, False}, seen
    # draw0 < 0 continues from the device counter of the previous set
    p0 = dev.get_pos()
    acc0, nxt0 = dev.hamiltonian_swap(sets[0], 5, 99, draw0=0, want_accepted=True)
    dev.hamiltonian_swap(sets[1], 5, 99, draw0=-1)
    a_cont = dev.get_pos()
    dev.set_pos(p0)
    dev.hamiltonian_swap(sets[0], 5, 99, draw0=0)
    dev.hamiltonian_swap(sets[1], 5, 99, draw0=nxt0)
    assert np.array_equal(dev.get_pos(), a_cont)
    dev.close(); host.close()


def _read_output(path):
    with P.pkg.h5lite.open_file(path) as f:
        out = f.group('output')
        return {k: out.read(k) for k in out.keys()}


def _umbrella(f, i):
    H.rewrite(f, 'dist_spring', 'equil_dist', lambda v: v * (1. + 0.002 * i))
    H.scale_hbond(f, 1. - 0.015 * i)


def test_upside_main_ladder_matches_reference(lib, tmp_path):
    ref_exe = os.path.join(P.ROOT, 'oracle', '_ref', 'upside_7A')
    assert os.path.exists(ref_exe), 'reference executable not built (oracle/_ref)'
    n = 8
    temps = ','.join('%.3f' % t for t in np.linspace(0.80, 0.87, n))
    args = ['--duration', '0.27', '--frame-interval', '0.054', '--temperature', temps, '--seed', '3', '--replica-interval', '0.055',
            '--swap-set', ','.join('%d-%d' % (i, i + 1) for i in range(0, n, 2)), '--swap-set', ','.join('%d-%d' % (i, i + 1) for i in range(1, n - 1, 2))]

    def run(tag, extra=(), env=None, mc=False, ref=False):
        fs = ladder(tmp_path, 'proteinG56_7A', n, _umbrella, tag=tag)
        if mc:
            for f in fs:
                P.pkg.config.add_pivot_moves(f)
        if ref:
            subprocess.run([ref_exe] + args + list(extra) + fs, check=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=900,
                           env=dict(os.environ, OMP_NUM_THREADS='4'))
        else:
            old = os.environ.get('UPSIDE_HIP_HAMILTONIAN_BATCH')
            if env is not None:
                os.environ['UPSIDE_HIP_HAMILTONIAN_BATCH'] = env
            try:
                lib.in_process_upside(args + list(extra) + fs, verbose=False)
            finally:
                if env is not None:
                    if old is None:
                        del os.environ['UPSIDE_HIP_HAMILTONIAN_BATCH']
                    else:
                        os.environ['UPSIDE_HIP_HAMILTONIAN_BATCH'] = old
        return [_read_output(f) for f in fs]

    ref = run('r', ref=True)
    got = run('h')
    off = run('o', env='0')
    assert len(set(np.unique(np.concatenate([r['replica_index'].ravel() for r in ref])).tolist())) == n
    moved = False
    for s in range(n):
        assert np.array_equal(got[s]['replica_index'], ref[s]['replica_index']), s
        assert np.array_equal(got[s]['replica_cumulative_swaps'], ref[s]['replica_cumulative_swaps']), s
        assert np.array_equal(off[s]['replica_index'], got[s]['replica_index']), s
        assert abs(got[s]['potential'][0, 0] - ref[s]['potential'][0, 0]) < 1e-4 * max(1., abs(ref[s]['potential'][0, 0])), s
        assert P.rel_rms(ref[s]['pos'][1], got[s]['pos'][1]) < 1e-3, s
        moved |= bool(np.any(got[s]['replica_index'] != s))
    assert moved                                    # some swaps were accepted
    mc = ['--monte-carlo-interval', '0.027']
    ref_mc = run('rm', mc, mc=True, ref=True)
    got_mc = run('hm', mc, mc=True)
    for s in range(n):
        assert np.array_equal(got_mc[s]['replica_index'], ref_mc[s]['replica_index']), s


def test_ladder_md_under_graph_capture(lib, tmp_path):
    """an hbond_energy ladder (no AFM: graph replay is the default at this batch size) under the captured MD loop equals plain
    launches bit for bit, with a set_param_system between two run_steps calls"""
    fs = ladder(tmp_path, 'proteinG56_7A', 4, lambda f, i: H.scale_hbond(f, 1. - 0.03 * i))
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'hamiltonian_graph_worker.py')
    res = {}
    for g in ('1', '0'):
        out = str(tmp_path / ('graph%s.npz' % g))
        env = dict(os.environ, UPSIDE_HIP_GRAPH=g, PYTHONPATH=os.pathsep.join([os.path.dirname(worker), P.ROOT]))
        subprocess.run([sys.executable, worker, out] + fs, check=True, timeout=600, env=env)
        res[g] = np.load(out)
    for k in ('mid', 'pos', 'mom', 'energy'):
        assert np.array_equal(res['1'][k], res['0'][k]), k
    assert not np.array_equal(res['1']['mid'], res['1']['pos'])


def _add_cavity(path, ids, radius, spring_constant=5.):
    with P.pkg.h5lite.open_file(path, 'r+') as t:
        g = t.group('input/potential').create_group('cavity_radial')
        g.set_attr('arguments', ['pos'])
        g.write('id', np.asarray(ids, 'i4'))
        g.write('radius', np.full(len(ids), radius, 'f4'))
        g.write('spring_constant', np.full(len(ids), spring_constant, 'f4'))
    return path


def test_cavity_radial_ladder(lib, tmp_path):
    """cavity_radial (in no fixture) on copies of trpcage20_7A, the radius at the median distance of the atoms from the origin.
    Window 1 changes only spring_constant, window 2 only radius: each of the node's two arrays in turn is the one that makes the
    table full.  Per window bitwise against an engine of three copies of its file and within RTOL of the oracle on its file;
    three copies of window 0 keep the single shared row and are bitwise what construct computes; a differing id is refused."""
    name = 'trpcage20_7A'
    pos = P.golden(name)['pos'].astype('f4')
    dist = np.sqrt((pos.reshape(-1, 3).astype('f8') ** 2).sum(axis=1))
    n_atom, radius = len(dist), float(np.median(dist))
    assert (dist > radius).any() and (dist < radius).any()
    fs = [_add_cavity(H.copy_fixture(name, tmp_path / ('c%d.up' % i)), np.arange(n_atom), radius) for i in range(3)]
    H.rewrite(fs[1], 'cavity_radial', 'spring_constant', lambda v: v * 1.5)
    H.rewrite(fs[2], 'cavity_radial', 'radius', lambda v: v * 0.9)
    big = E.Ensemble.from_files(fs, library=lib)
    big.set_pos(pos)
    e, d = big.energies_and_derivs()
    big.close()
    assert len(set(e.tolist())) == 3                 # the windows really differ
    for i, f in enumerate(fs):
        same = E.Ensemble(f, 3, library=lib)
        same.set_pos(pos)
        e3, d3 = same.energies_and_derivs()
        same.close()
        assert e3[i] == e[i], (i, e3[i], e[i])
        assert np.array_equal(d3[i], d[i]), i
        orc = P.pkg.Upside(f, library=P.oracle_library())
        ref = dict(energy=np.float32(orc.energy(pos)), deriv=orc.deriv(pos))
        node_energy = float(orc.get_output('cavity_radial')[0, 0])
        orc.close()
        assert node_energy != 0., i
        bad = P.compare(ref, dict(energy=e[i], deriv=d[i]), rtol=P.RTOL, verbose=True)
        assert not bad, (i, bad)
    up = P.pkg.Upside(fs[0])
    up.energy(pos)
    assert float(up.get_output('cavity_radial')[0, 0]) != 0.
    up.close()
    a = E.Ensemble.from_files([fs[0]] * 3, library=lib); b = E.Ensemble(fs[0], 3, library=lib)
    for x in (a, b):
        x.set_pos(pos)
    ea, da = a.energies_and_derivs(); eb, db = b.energies_and_derivs()
    a.close(); b.close()
    assert np.array_equal(ea, eb) and np.array_equal(da, db)
    other = _add_cavity(H.copy_fixture(name, tmp_path / 'other_id.up'), np.arange(n_atom)[::-1], radius)
    with pytest.raises(RuntimeError) as err:
        E.Ensemble.from_files([fs[0], other], library=lib)
    msg = str(err.value)
    assert 'cavity_radial' in msg and 'id' in msg and 'other_id.up' in msg, msg
