"""set_param / get_param of the force-field nodes on the device (rotamer, the coverage graphs, environment_coverage, protein_hbond,
hbond_sc_radial, the fixed placements, nonlinear_coupling_environment and the linear couplings), the write step of parameter training.

An engine built from the OLD file, with its pair lists built at the old cut-off, takes the perturbed tables of set_param_cases.py
and must then be indistinguishable from an engine built from the file that holds them:
  - against a fresh device engine of the rewritten file: every result within 2e-6 relative RMS, energies within rtol 2e-6 / atol 1e-3
    (the bound test_alternate_code_paths_agree holds two code paths of one engine to);
  - against a fresh oracle engine of that file: P.compare at RTOL = 1e-5, the total energy within RTOL x sum |potential|, the five
    canonical pair lists bit for bit, the side-chain solve's sweep count equal and n_bad_solve 0;
  - get_param_deriv against the oracle at 1e-5 (5e-5 on the fixed placements: test_param_derivs_match_reference_golden's bounds).
The same under every switch that selects which device image of a table a pass reads, for every system of a batch, across a captured MD
graph, and for the energies an exchange attempt keeps.  No bound here comes from the code under test.

With UPSIDE_SET_PARAM_RECORD=<file> the largest deviation seen per comparison is written there (profiles/set_param_parity.txt)."""
import ctypes as ct
import os
import subprocess
import sys
import numpy as np
import pytest
import parity_util as P
import set_param_cases as C
import set_param_gpu_worker as W

pytestmark = pytest.mark.gpu
RTOL = P.RTOL
PATH_TOL = 2e-6
HERE = os.path.dirname(os.path.abspath(__file__))
RECORD = {}
NOT_ARRAYS = ('sweeps', 'n_bad')


def record(label, value):
    RECORD[label] = max(RECORD.get(label, 0.), float(value))


def record_flag(label, flag):
    RECORD[label] = min(RECORD.get(label, 1.), 1. if flag else 0.)


@pytest.fixture(scope='module')
def hip():
    import torch
    assert torch.cuda.is_available(), 'these tests need a GPU'
    lib = P.pkg.default_library()     # raises when the HIP extension is missing: no fallback
    P.pkg.engine.Ensemble._bind(lib.calc)
    W.bind(lib.calc)
    yield lib
    out = os.environ.get('UPSIDE_SET_PARAM_RECORD')
    if out:
        with open(out, 'w') as f:
            for k in sorted(RECORD):
                f.write('%-64s %.3e\n' % (k, RECORD[k]))


@pytest.fixture(scope='module')
def oracle():
    return P.oracle_library()


class Work(object):
    """the rewritten files and the worker runs of this module, made once"""

    def __init__(self, root):
        self.root, self.files, self.runs = root, {}, {}

    def built(self, case):
        if case not in self.files:
            path = str(self.root / (case + '.up'))
            old, new = C.build(case, path)
            self.files[case] = (path, old, new)
        return self.files[case]

    def run(self, mode, case, env_extra, *args):
        key = (mode, case, tuple(sorted(env_extra.items()))) + args
        if key not in self.runs:
            out = str(self.root / ('run%d.npz' % len(self.runs)))
            env = dict(os.environ, PYTHONPATH=os.pathsep.join([HERE, P.ROOT]))
            env.pop('UPSIDE_SET_PARAM_RECORD', None)
            env.update(env_extra)
            subprocess.run([sys.executable, os.path.join(HERE, 'set_param_gpu_worker.py'), mode, case, self.built(case)[0], out] + list(args),
                           check=True, timeout=300, env=env, cwd=HERE)
            self.runs[key] = dict(np.load(out))
        return self.runs[key]


@pytest.fixture(scope='module')
def work(tmp_path_factory):
    return Work(tmp_path_factory.mktemp('set_param'))


def is_scalar_key(k):
    return k == 'energy' or k.startswith('pot/')


def assert_same_engine(ref, act, label):
    """two device engines that must hold the same parameters: 2e-6 relative RMS, energies rtol 2e-6 / atol 1e-3, lists and sweeps equal"""
    assert sorted(ref) == sorted(act)
    for k in sorted(ref):
        if k.startswith('pairlist/') or k in NOT_ARRAYS:
            assert np.array_equal(ref[k], act[k]), (label, k)
        elif is_scalar_key(k):
            record(label + ' energies abs', abs(float(ref[k]) - float(act[k])))
            assert np.allclose(ref[k], act[k], rtol=PATH_TOL, atol=1e-3), (label, k, ref[k], act[k])
        else:
            e = P.rel_rms(ref[k], act[k])
            record(label + ' rel_rms', e)
            assert e <= PATH_TOL, (label, k, e)


def bit_equal(ref, act):
    return all(np.asarray(ref[k]).tobytes() == np.asarray(act[k]).tobytes() for k in ref)


def assert_matches_oracle(ref, act, fixture, label):
    keys = [k for k in sorted(ref) if k != 'energy' and not k.startswith('pairlist/') and k not in NOT_ARRAYS]
    for k in keys:
        record(label + ' rel_rms', abs(float(ref[k]) - float(act[k])) / max(1., abs(float(ref[k]))) if np.ndim(ref[k]) == 0 else P.rel_rms(ref[k], act[k]))
    bad = P.compare(ref, act, keys=keys, rtol=RTOL)
    assert not bad, (label, 'outside 1e-5 relative', bad)
    scale = sum(abs(float(ref['pot/' + k])) for k in C.potential_names(fixture))
    record(label + ' energy / sum|pot|', abs(float(ref['energy']) - float(act['energy'])) / scale)
    assert abs(float(ref['energy']) - float(act['energy'])) <= RTOL * scale, (label, ref['energy'], act['energy'])
    for node in C.PAIRLIST_NODES:
        po, ph = ref['pairlist/' + node], act['pairlist/' + node]
        assert po.shape == ph.shape and np.array_equal(po, ph), (label, node, po.shape, ph.shape)
    assert int(act['sweeps']) == int(ref['sweeps']), (label, act['sweeps'], ref['sweeps'])
    assert int(act['n_bad']) == 0 and int(ref['n_bad']) == 0, label


def assert_param_derivs(ref, act, label):
    assert sorted(ref) == sorted(act) and ref
    for k in sorted(ref):
        node = k.split('/', 1)[1]
        if not np.any(ref[k]):
            assert not np.any(act[k]), (label, k)      # environment_coverage: zeros
            continue
        e = P.rel_rms(ref[k], act[k])
        record(label + (' placements' if node.startswith('placement') else '') + ' rel_rms', e)
        assert e <= C.param_deriv_tol(node), (label, k, e)


# ---- (a) one node at a time -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', C.NODE_CASES)
def test_one_node_at_a_time(hip, oracle, work, case):
    fixture, nodes = C.fixture_of(case), C.nodes_of(case)
    path, old, new = work.built(case)
    pos, pos2 = C.positions(fixture)
    up = P.pkg.Upside(P.fixture(fixture))
    first = W.hip_snapshot(up, fixture, pos)           # the lists exist at the old cut-off
    W.set_tables(up, nodes, old, new)                  # get_param = the file's table, then = the new one, bit for bit
    fresh = P.pkg.Upside(path)
    orc = P.pkg.Upside(path, library=oracle)
    for tag, x in (('pos', pos), ('pos2', pos2)):      # pos2: through the cached lists
        act = W.hip_snapshot(up, fixture, x)
        assert_same_engine(W.hip_snapshot(fresh, fixture, x), act, '(a) set_param vs fresh device engine')
        assert_matches_oracle(W.oracle_snapshot(orc, fixture, x), act, fixture, '(a) set_param vs oracle')
    if any(n not in C.NO_PARAM_DERIV for n in nodes):      # (of the last evaluation: pos2)
        assert_param_derivs(W.param_derivs(orc, nodes, new), W.param_derivs(up, nodes, new), '(a) get_param_deriv vs oracle')
    # requests of the wrong size are refused and change nothing
    c = hip.calc
    for node in nodes:
        n = len(new[node])
        buf = np.zeros(n + 1, 'f4')
        assert c.set_param(n - 1, buf.ctypes.data, up.engine, node.encode()) == 1
        assert c.set_param(n + 1, buf.ctypes.data, up.engine, node.encode()) == 1
        assert c.get_param(n + 1, buf.ctypes.data, up.engine, node.encode()) == 1
        W.check_get_param(up, node, new[node])
    # the old tables back: the first evaluation again
    for node in nodes:
        up.set_param(old[node], node)
        W.check_get_param(up, node, old[node])
    back = W.hip_snapshot(up, fixture, pos)
    assert_same_engine(first, back, '(a) old tables set back vs first evaluation')
    record_flag('(a) old tables set back: bit-equal to the first evaluation (1 = every case)', bit_equal(first, back))
    up.close(); fresh.close(); orc.close()


# ---- (b) everything at once, (c) under every switch that selects a table image ------------------------------------------------------
def check_tables_run(res, oracle, work, case, label):
    fixture, nodes = C.fixture_of(case), C.nodes_of(case)
    path, old, new = work.built(case)
    orc = P.pkg.Upside(path, library=oracle)
    for tag, x in zip(('pos', 'pos2'), C.positions(fixture)):
        act = W.sub(res, 'set:%s:' % tag)
        assert_same_engine(W.sub(res, 'fresh:%s:' % tag), act, label + ' set_param vs fresh device engine')
        assert_matches_oracle(W.oracle_snapshot(orc, fixture, x), act, fixture, label + ' set_param vs oracle')
    act = dict((k, v) for k, v in W.sub(res, 'set:').items() if k.startswith('param_deriv/'))      # (of the last evaluation: pos2)
    assert_param_derivs(W.param_derivs(orc, nodes, new), act, label + ' get_param_deriv vs oracle')
    orc.close()


@pytest.mark.parametrize('case', ['every_proteinG56_7A', 'every_syn150_10A'])
def test_every_table_at_once(hip, oracle, work, case):
    check_tables_run(work.run('tables', case, {}), oracle, work, case, '(b)')


TABLE_IMAGES = [
    {'UPSIDE_HIP_IG_POLY': '0'},             # coverage passes on the spline-coefficient table, not its polynomial image
    {'UPSIDE_HIP_ROT_POLY': '0'},            # side-chain energy pass on the triangular table, not its polynomial image
    {'UPSIDE_HIP_PAIR2': '0'},               # scalar forms of the side-chain gradient and coverage passes
    {'UPSIDE_HIP_IG_UNSTAGED': '1'},         # coverage passes reading the raw table from global memory
    {'UPSIDE_HIP_ROT_UNSTAGED': '1'},        # side-chain passes with bead rows in global memory
    {'UPSIDE_HIP_ROTAMER_ATOMIC': '1'},      # pair matrices accumulated with atomics
    {'UPSIDE_HIP_BP_CLUSTER': '1', 'UPSIDE_HIP_BP_ENERGY_TABLE': '1'},      # one-workgroup solve taking exp(-E) of the pair matrices itself
]


@pytest.mark.parametrize('env_extra', TABLE_IMAGES, ids=lambda e: ','.join('%s=%s' % kv for kv in sorted(e.items())))
def test_every_table_image_follows(hip, oracle, work, env_extra):
    case = 'every_proteinG56_7A'
    base = work.run('tables', case, {})
    res = work.run('tables', case, env_extra)
    check_tables_run(res, oracle, work, case, '(c)')
    for tag in ('pos', 'pos2'):
        assert_same_engine(W.sub(base, 'set:%s:' % tag), W.sub(res, 'set:%s:' % tag), '(c) switch vs default run')


# Up to 16 systems the cached lists reach 1.5 (1 + 0.2 cutoff) past the cut-off: 4.2 A for environment_coverage (9 A) and 4.3 A for
# hbond_sc_radial (9.33 A).  The cut-offs of the cases grow by 1.0 A and 2.33 A, so a list that set_param forgot to rebuild would still
# hold every pair in range.  With the margin at 0.2 (1 + 0.2 cutoff) = 0.56 A it does not.
NARROW_MARGIN = {'UPSIDE_HIP_SKIN_SCALE': '0.2'}


@pytest.mark.parametrize('case', ['environment_coverage_grow', 'hbond_sc_radial', 'every_proteinG56_7A'])
def test_moved_cut_off_rebuilds_the_cached_lists(hip, oracle, work, case):
    check_tables_run(work.run('tables', case, NARROW_MARGIN), oracle, work, case, '(c) narrow list margin:')


# ---- (d) every system of a batch ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n_system', [3, 20])      # 20: past the 16 systems up to which the MD loop is a captured graph by default
def test_batch(hip, oracle, work, n_system):
    case = 'every_proteinG56_7A'
    fixture, nodes = C.fixture_of(case), C.nodes_of(case)
    path, old, new = work.built(case)
    pos, pos2 = C.positions(fixture)
    t = np.linspace(0., 1., n_system).astype('f4')
    x = np.ascontiguousarray(pos[None] + t[:, None, None] * (pos2 - pos)[None]).astype('f4')      # distinct coordinates
    ens = P.pkg.engine.Ensemble(P.fixture(fixture), n_system, library=hip)
    ens.set_pos(x)
    ens.energies()                                     # the lists exist at the old cut-off
    for node in nodes:
        assert ens.get_param(old[node].shape, node).tobytes() == old[node].tobytes(), node
        ens.set_param(new[node], node)
        assert ens.get_param(new[node].shape, node).tobytes() == new[node].tobytes(), node
    e, d = ens.energies_and_derivs()
    orc = P.pkg.Upside(path, library=oracle)
    deriv_nodes = [n for n in nodes if n not in C.NO_PARAM_DERIV]
    checked = range(n_system) if n_system <= 3 else (0, n_system // 2, n_system - 1)
    for s in range(n_system):
        ref = P.evaluate_all(orc, x[s])
        e1, e2 = P.rel_rms(ref['deriv'], d[s]), P.max_rel_to_scale(ref['deriv'], d[s])
        record('(d) forces of every system vs oracle rel_rms', e1)
        assert e1 <= RTOL and e2 <= 10 * RTOL, (s, e1, e2)
        scale = sum(abs(float(ref['pot/' + k])) for k in P.POTENTIAL_NODES)
        assert abs(float(ref['energy']) - float(e[s])) <= RTOL * scale, (s, ref['energy'], e[s])
        if s in checked:
            act = {}
            for node in deriv_nodes:
                out = np.zeros(new[node].shape, 'f4')
                assert ens.calc.upside_hip_get_param_deriv(ens.engine, node.encode(), s, out.size, out.ctypes.data) == 0
                act['param_deriv/' + node] = out
            assert_param_derivs(W.param_derivs(orc, nodes, new), act, '(d) upside_hip_get_param_deriv vs oracle')
    # one accumulate / read against the per-system tables (test_param_deriv_batch.py: the float64 host sum, systems ascending)
    w = np.random.RandomState(5).uniform(-1.5, 1.5, size=n_system).astype('f4')
    for node in deriv_nodes:
        shape = new[node].shape
        ens.param_deriv_accumulate(node, w)
        tab = ens.param_deriv(node, shape).astype('f8')
        host = np.zeros(shape, 'f8')
        for s in range(n_system):
            host += np.float64(w[s]) * tab[s]
        total, n_frame = ens.param_deriv_read(node, shape)
        assert n_frame == 1, node
        scale = max(np.abs(host).max(), 1e-30)
        record('(d) param_deriv_read vs float64 host sum, max / scale', np.abs(total - host).max() / scale)
        assert np.abs(total - host).max() <= 1e-12 * scale, (node, np.abs(total - host).max() / scale)
    orc.close(); ens.close()


# ---- (e) MD around a set_param ------------------------------------------------------------------------------------------------------
MD_CASE = 'md_proteinG56_7A'


def md_run(work, graph, readback):
    return work.run('md', MD_CASE, {'UPSIDE_HIP_GRAPH': graph}, '1' if readback else '0')


@pytest.mark.parametrize('readback', [False, True])
def test_md_graph_replay_equals_plain_launches(hip, work, readback):
    """run_steps, set_param with the steps still in flight, run_steps: the captured graph must not replay the old tables or cut-offs"""
    a, b = md_run(work, '1', readback), md_run(work, '0', readback)
    for k in (['mid'] if readback else []) + ['pos', 'mom', 'energy', 'force']:
        assert np.array_equal(a[k], b[k]), k
    record_flag('(e) UPSIDE_HIP_GRAPH=1 and 0 bit-equal (1 = yes)', True)
    if readback:
        assert not np.array_equal(a['mid'], a['pos'])


def test_md_set_param_waits_for_the_steps_in_flight(hip, work):
    """a get_pos() in front of the set_param (which waits for the stream) changes nothing, in either launch mode"""
    for graph in ('1', '0'):
        a, b = md_run(work, graph, False), md_run(work, graph, True)
        for k in ('pos', 'mom', 'energy', 'force'):
            assert np.array_equal(a[k], b[k]), (graph, k)
    record_flag('(e) with and without a read-back before set_param bit-equal (1 = yes)', True)


@pytest.mark.parametrize('env_extra', [{}, NARROW_MARGIN], ids=['default', 'narrow_list_margin'])
def test_md_final_state_matches_oracle(hip, oracle, work, env_extra):
    path = work.built(MD_CASE)[0]
    res = work.run('md', MD_CASE, dict(env_extra, UPSIDE_HIP_GRAPH='1'), '0')
    orc = P.pkg.Upside(path, library=oracle)
    for s in range(res['pos'].shape[0]):
        ref = P.evaluate_all(orc, res['pos'][s])
        e1, e2 = P.rel_rms(ref['deriv'], res['force'][s]), P.max_rel_to_scale(ref['deriv'], res['force'][s])
        record('(e) forces at the final coordinates vs oracle rel_rms', e1)
        assert e1 <= RTOL and e2 <= 10 * RTOL, (s, e1, e2)
        scale = sum(abs(float(ref['pot/' + k])) for k in P.POTENTIAL_NODES)
        assert abs(float(ref['energy']) - float(res['energy'][s])) <= RTOL * scale, s
        for node in C.PAIRLIST_NODES:
            assert np.array_equal(res['pairlist/%d/%s' % (s, node)], P.oracle_pairlist(orc, node)), (s, node)
    orc.close()


# ---- (f) exchange ---------------------------------------------------------------------------------------------------------------------
def test_replica_swap_next_rejects_energies_of_older_parameters(hip, work):
    """a later swap set may only reuse the energies of its own attempt: after a set_param they belong to another Hamiltonian"""
    case = 'rotamer'
    fixture = C.fixture_of(case)
    path, old, new = work.built(case)
    c = hip.calc
    for f in (c.upside_hip_replica_swap_from, c.upside_hip_replica_swap_next):
        f.argtypes = [ct.c_void_p, ct.c_int, ct.c_void_p, ct.c_uint32, ct.c_uint64, ct.c_int, ct.c_void_p]
    ens = P.pkg.engine.Ensemble(P.fixture(fixture), 4, library=hip)
    ens.set_pos(C.positions(fixture)[0])
    ens.init_md(np.array([0.7, 0.8, 0.9, 1.0], 'f4'), 5)
    e = ens.engine
    p0 = np.array([[0, 1], [2, 3]], 'i4'); p1 = np.array([[1, 2]], 'i4')
    acc = np.zeros(3, 'i4'); acc1 = np.zeros(2, 'i4')
    assert c.upside_hip_replica_swap_from(e, 2, p0.ctypes.data, 11, 1, 0, acc.ctypes.data) == 0
    assert c.upside_hip_replica_swap_next(e, 1, p1.ctypes.data, 11, 1, int(acc[-1]), acc1.ctypes.data) == 0      # same attempt: fine
    assert c.upside_hip_replica_swap_from(e, 2, p0.ctypes.data, 11, 2, 0, acc.ctypes.data) == 0
    ens.set_param(new['rotamer'], 'rotamer')
    assert c.upside_hip_replica_swap_next(e, 1, p1.ctypes.data, 11, 2, int(acc[-1]), acc1.ctypes.data) != 0      # new parameters in between
    assert c.upside_hip_replica_swap_from(e, 2, p0.ctypes.data, 11, 2, 0, acc.ctypes.data) == 0                  # a new attempt is fine
    assert c.upside_hip_replica_swap_next(e, 1, p1.ctypes.data, 11, 2, int(acc[-1]), acc1.ctypes.data) == 0
    ens.close()
