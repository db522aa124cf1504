"""Child process of tests/test_gpu_walked_lists.py: one check per invocation of the lists the pair passes walk (upside_hip_get_walked_lists,
upside_hip_get_backbone_list) against tests/walked_lists.py,

    python tests/walked_lists_gpu_worker.py CHECK WORKDIR [ARG ...]

under whatever UPSIDE_HIP_* environment the parent set (the switches are read once per process).  It prints every tally before it asserts
and ends with 'CHECK <name> PASSED'.  At most one engine is alive at a time.  References: for the oracle-listed graphs
P.oracle_pairlist at the device's current positions; for the radial graphs the yardstick on the device's source-node outputs.  Every
comparison is exact."""
import os
import sys
import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import parity_util as P                  # noqa: E402
import walked_lists as WL                # noqa: E402

pkg = P.pkg
Ensemble = pkg.engine.Ensemble
STATIC_FIXTURES = ['trpcage20_7A', 'proteinG56_7A', 'syn150_10A', 'syn300_10A', 'syn300_7A']
# Factors of the compressed / stretched structures of `static`, chosen on the CPU with the yardstick on the oracle's node outputs at
# cache_cutoff = cutoff + 1.5 (1 + 0.2 cutoff): pooled over these and the golden structures, the cached row lengths of the walked side-1
# lists and of the walked side-2 lists each fill every class of WL.cnt_classes, no row exceeds its capacity (512 words; syn300_10A at 0.8
# has rows of 491 by the yardstick and the device reports a neighbour-list overflow there, at 0.9 the rows stay well below) and the
# side-chain graph stays below its slot and adjacency capacities (12107 residue pairs of 28800, 160 neighbours of 256).
SCALED = {'syn300_10A': (0.9, 1.3), 'proteinG56_7A': (0.5, 2.0)}
RUNS = (1, 5, 6, 7, 12, 13, 30)          # multiples and non-multiples of the six captured steps
BACKBONE_RUNS = (1, 5, 6, 7, 12, 13, 16)  # 60 steps


def scaled(x, f):
    c = x.mean(0, keepdims=True)
    return ((x - c) * np.float32(f) + c).astype('f4')


def node_output(ens, name):
    """get_output through the C-ABI: system 0 of the engine"""
    c = ens.calc
    n = np.zeros(1, np.intc); w = np.zeros(1, np.intc)
    assert c.get_output_dims(n.ctypes.data, w.ctypes.data, ens.engine, name.encode()) == 0, name
    out = np.zeros((int(n[0]), int(w[0])), 'f4')
    assert c.get_output(out.size, out.ctypes.data, ens.engine, name.encode()) == 0, name
    return out


def records_of(ens, node, system):
    """the records of the sides the MD path keeps; a side it does not keep must refuse with status 2"""
    out = []
    for side in (1, 2):
        try:
            out.append(ens.walked_lists(node, system, side))
        except RuntimeError as err:
            if getattr(err, 'status', 0) == 2 and 'does not keep' in str(err):
                continue
            if side == 2 and 'one side only' in str(err):
                continue
            raise
    assert out, node
    return out


class Oracle(object):
    """the oracle's pair lists at given atom positions, every oracle-listed graph from one evaluation"""
    def __init__(self, fixture):
        self.orc = pkg.Upside(P.fixture(fixture), library=P.oracle_library())
        self.seen = {}

    def forget(self):
        self.seen = {}

    def edges(self, pos, node):
        key = pos.tobytes()
        if key not in self.seen:
            self.orc.deriv(pos)
            self.seen[key] = {n: P.oracle_pairlist(self.orc, n) for n in WL.ORACLE_GRAPHS}
        return self.seen[key][node]


def reference_edges(oracle, specs, ens_pos, node, recs):
    if node in WL.ORACLE_GRAPHS:
        return oracle.edges(ens_pos, node)
    # radial graphs: the yardstick on the device's own source-node outputs of this system
    r = recs[0]; sp = specs[node]
    p1, p2 = (r['src_rows'], r['src_other']) if r['side'] == 1 else (r['src_other'], r['src_rows'])
    return WL.edges_yardstick(p1, p2, sp['id1'], sp['id2'], r['cutoff'], sp['itype'], sp['symmetric'])


def check_system(ens, oracle, specs, nodes, system, pos, first_pass, tallies):
    """check_graph on every node and kept side of one system; returns {node: n_edge}"""
    for node in nodes:
        recs = records_of(ens, node, system)
        ref = reference_edges(oracle, specs, pos, node, recs)
        want_cut = WL.graph_cutoff(specs[node])
        for r in recs:
            assert r['cutoff'].tobytes() == np.float32(want_cut).tobytes(), (node, r['cutoff'], want_cut)
            src = None
            if system == 0:
                src = {nm: node_output(ens, nm) for nm in {r['source_rows'], r['source_other']}}
            t = WL.check_graph(r, ref, first_pass=first_pass, source_out=src)
            k = (node, r['side'])
            a = tallies.setdefault(k, dict(records=0, edges=0, cached=0, walked=0, cnt=[]))
            a['records'] += 1; a['edges'] += t['n_edge']; a['cached'] += t['n_cached']; a['walked'] += t['n_walked']
            a['cnt'].append(t['cnt'])


def print_tallies(tallies):
    for (node, side), a in sorted(tallies.items()):
        print('  %-26s side %d: %5d records, %9d edges, %9d walked, %9d cached' % (node, side, a['records'], a['edges'], a['walked'], a['cached']))


def static(work):
    tallies = {}
    by_side = {1: [], 2: []}
    for name in STATIC_FIXTURES:
        g = P.golden(name)
        cases = [('pos', g['pos']), ('pos2', g['pos2'])] + [('x%.2f' % f, scaled(g['pos'], f)) for f in SCALED.get(name, ())]
        specs = {n: WL.graph_spec(pkg.h5lite, P.fixture(name), n) for n in WL.ORACLE_GRAPHS}
        oracle = Oracle(name)
        for tag, x in cases:
            ens = Ensemble(P.fixture(name), 1)      # a fresh engine: the first pass builds, refines and orders every list
            ens.set_pos(x[None])
            ens.energies_and_derivs()
            t = {}
            check_system(ens, oracle, specs, WL.ORACLE_GRAPHS, 0, np.ascontiguousarray(x, 'f4'), True, t)
            ens.close()
            oracle.forget()
            print('%s %s' % (name, tag)); print_tallies(t)
            for (node, side), a in t.items():
                by_side[side] += a['cnt']
                b = tallies.setdefault((node, side), dict(records=0, edges=0, cached=0, walked=0, cnt=[]))
                for k in a:
                    b[k] += a[k]
    print('all structures'); print_tallies(tallies)
    ok = True
    for side in (1, 2):
        cls = WL.cnt_classes(np.concatenate(by_side[side]))
        print('cached row lengths of the walked side-%d lists: %r' % (side, cls))
        ok &= all(v > 0 for v in cls.values())
    for (node, side), a in sorted(tallies.items()):
        print('  %-26s side %d: %r' % (node, side, WL.cnt_classes(np.concatenate(a['cnt']))))
    assert ok, 'a class of cached row lengths is empty'
    assert {k[0] for k in tallies} == set(WL.ORACLE_GRAPHS)


def far_structure(x):
    """the structure turned a quarter about the z axis through its centroid: far more than any margin for all but the few atoms near the
    axis, and z (what the fields of the restraint fixture depend on) is kept"""
    c = x.mean(0, keepdims=True); d = x - c
    return np.ascontiguousarray(np.stack((-d[:, 1], d[:, 0], d[:, 2]), 1) + c, 'f4')


def md_script(work, fixture, size, nodes=None, runs=RUNS, backbone=False, record=None):
    import torch
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    S = {'ncu+8': n_cu + 8, '2ncu+8': 2 * n_cu + 8}.get(size) or int(size)
    nodes = list(WL.ORACLE_GRAPHS if nodes is None else nodes)
    g = P.golden(fixture)
    specs = {n: WL.graph_spec(pkg.h5lite, P.fixture(fixture), n) for n in nodes}
    oracle = Oracle(fixture)
    rng = np.random.RandomState(11)
    starts = [g['pos'], g.get('pos2', g['pos'])]
    pos0 = np.stack([starts[s % 2] for s in range(S)]).astype('f4') + (0.02 * rng.randn(S, g['pos'].shape[0], 3)).astype('f4')
    temps = np.linspace(0.5, 1.5, S).astype('f4')
    ens = Ensemble(P.fixture(fixture), S)
    ens.set_pos(pos0)
    ens.init_md(temps, 5)
    print('%s, %d systems (%d CUs), temperatures %.2f .. %.2f, switches %r' % (
        fixture, S, n_cu, temps[0], temps[-1], {k: v for k, v in os.environ.items() if k.startswith('UPSIDE_HIP_')}))
    flag_classes = {n: dict(none=0, some=0, all=0) for n in nodes}
    tallies = {}
    saved = dict(pos=[], pot=[])
    n_check = [0]

    def deriv_only():
        d = np.zeros((S, ens.n_atom, 3), 'f4')
        ens._check(ens.calc.upside_hip_compute(ens.engine, None, d.ctypes.data), 'compute')

    def checkpoint(what):
        ens.energies_and_derivs()
        pos = ens.get_pos()
        assert np.isfinite(pos).all(), 'positions are not finite after ' + what
        oracle.forget()
        first = n_check[0] == 0
        n_check[0] += 1
        line = []
        for node in nodes:
            fl = ens.rebuild_flags(node)
            n_fl = int((fl != 0).sum())
            flag_classes[node]['none' if n_fl == 0 else ('all' if n_fl == S else 'some')] += 1
            if S <= 24:
                systems = list(range(S))
            else:
                quiet = np.flatnonzero(fl == 0)
                systems = sorted({0, S - 1} | set(np.flatnonzero(fl).tolist()) | set(quiet[np.linspace(0, len(quiet) - 1, min(6, len(quiet))).astype(int)].tolist() if len(quiet) else ()))
            for s in systems:
                check_system(ens, oracle, specs, [node], s, pos[s], first, tallies)
            line.append('%s %d/%d' % (node, n_fl, len(systems)))
        if backbone:
            t = dict(listed=0, near=0)
            pot = np.zeros(S, 'f4')
            for s in range(S):
                b = ens.backbone_list('backbone_pairs', s)
                if s == 0:
                    assert b['centre'].tobytes() == np.ascontiguousarray(node_output(ens, 'affine_alignment')[b['id'], :3]).tobytes()
                r = WL.check_backbone(b, b['centre'])
                t['listed'] += r['n_listed']; t['near'] += r['n_near']; pot[s] = b['potential']
            saved['pos'].append(pos); saved['pot'].append(pot)
            line.append('backbone_pairs: %d listed, %d within the cutoff, cap %d skin %.2f' % (t['listed'], t['near'], b['cap'], b['skin']))
        print('after %-28s rebuilt/checked: %s' % (what, '; '.join(line)))

    checkpoint('the first pass')
    ops = [('one derivative-only pass', deriv_only),
           ('an energies-only call', lambda: ens.energies()),
           ('set_system_pos(%d, far)' % (S // 2), lambda: ens.set_system_pos(S // 2, far_structure(starts[1]))),
           ('swap_systems(0, %d)' % (S - 1), lambda: ens.swap_systems(0, S - 1)),
           ('set_temperature(reversed)', lambda: ens.set_temperature(temps[::-1])),
           ('one more derivative-only pass', deriv_only)]
    for i, k in enumerate(runs):
        ens.run_steps(k)
        checkpoint('run_steps(%d)' % k)
        if i < len(ops):
            ops[i][1]()
            checkpoint(ops[i][0])
    ens.close()
    print_tallies(tallies)
    for node in nodes:
        print('  %-26s check points with no / some / every system rebuilding: %r' % (node, flag_classes[node]))
    for node in nodes:
        assert all(v > 0 for v in flag_classes[node].values()), (node, flag_classes[node])
    if record:
        np.savez(record, pos=np.stack(saved['pos']), pot=np.stack(saved['pot']), fixture=fixture)
        print('recorded %d check points of %d systems in %s' % (len(saved['pos']), S, record))


def md(work, fixture, size):
    md_script(work, fixture, size)


def radial(work):
    md_script(work, 'proteinG56_restraints', 3, nodes=WL.RADIAL_GRAPHS)


def backbone(work, size, record):
    md_script(work, 'syn150_10A', size, nodes=[], runs=BACKBONE_RUNS, backbone=True, record=record)


def backbone_nolist(work, record):
    """with the cached list off: the positions another child recorded give the same bits of the backbone_pairs potential, system by system"""
    d = np.load(record)
    pos, pot = d['pos'], d['pot']
    S = pos.shape[1]
    ens = Ensemble(P.fixture(str(d['fixture'])), S)
    assert not ens.backbone_list('backbone_pairs', 0, must_have_list=False)['list_on'], 'the list is on: UPSIDE_HIP_BACKBONE_LIST=0 did not reach the engine'
    n_diff = 0; n_nonzero = 0
    for k in range(len(pos)):
        ens.set_pos(pos[k])
        ens.energies_and_derivs()
        got = np.array([ens.backbone_list('backbone_pairs', s, must_have_list=False)['potential'] for s in range(S)], 'f4')
        same = got.tobytes() == pot[k].tobytes()
        n_diff += not same
        print('check point %2d: potentials %.6f .. %.6f, same bits as with the list: %s' % (k, got.min(), got.max(), same))
        n_nonzero += int((got != 0.).sum())      # (a system without a steric contact has potential 0)
    ens.close()
    print('%d potentials of %d are not zero' % (n_nonzero, pot.size))
    assert n_diff == 0, '%d check points differ' % n_diff
    assert n_nonzero > 0, 'every potential is zero: nothing was compared'


def refusals(work):
    name = 'proteinG56_7A'
    g = P.golden(name); S = 3
    ens = Ensemble(P.fixture(name), S)
    ens.set_pos(np.stack([g['pos'], g['pos2'], g['pos']]).astype('f4'))
    ens.energies_and_derivs()
    e0, d0 = ens.energies_and_derivs()
    kept = {n: ens.walked_lists(n, 0, 1 if n != 'hbond_coverage' else 2)['md_sides'] for n in ('hbond_coverage', 'environment_coverage')}
    print('sides kept: %r' % kept)
    one_sided = [(n, 3 - k) for n, k in sorted(kept.items()) if k != 3]
    assert one_sided, 'no graph of this engine keeps one side only: the refusal of a side that is not kept cannot be shown'
    f = ens.calc.upside_hip_get_walked_lists
    info = np.zeros(20, 'i4'); cut = np.zeros(2, 'f4'); ints = np.zeros(4, 'i4'); floats = np.zeros(4, 'f4')

    def small_buffer():
        rc = f(ens.engine, b'rotamer', 0, 1, info.ctypes.data, cut.ctypes.data, None, 0, 4, ints.ctypes.data, 4, floats.ctypes.data)
        assert rc == 3 and info[14] > 4 and not ints.any(), rc
        raise RuntimeError(ens.calc.upside_hip_last_error().decode())
    cases = [('side %d of %s, which is not kept' % (sd, n), lambda n=n, sd=sd: ens.walked_lists(n, 1, sd), 'does not keep') for n, sd in one_sided]
    cases += [
             ('side 2 of a symmetric graph', lambda: ens.walked_lists('rotamer', 0, 2), 'one side only'),
             ('side 3', lambda: ens.walked_lists('protein_hbond', 0, 3), 'side must be'),
             ('a node without a graph', lambda: ens.walked_lists('backbone_pairs', 0, 1), 'no interaction graph'),
             ('an unknown node', lambda: ens.walked_lists('no_such_node', 0, 1), 'not found'),
             ('system -1', lambda: ens.walked_lists('rotamer', -1, 1), 'invalid system'),
             ('system S', lambda: ens.walked_lists('rotamer', S, 1), 'invalid system'),
             ('too small a buffer', small_buffer, 'buffer too small'),
             ('rebuild_flags of a node without a graph', lambda: ens.rebuild_flags('backbone_pairs'), 'no interaction graph'),
             ('the backbone accessor with the list off', lambda: ens.backbone_list('backbone_pairs', 0), 'keeps no cached'),
             ('the backbone accessor on another node', lambda: ens.backbone_list('rotamer', 0), 'not a backbone_pairs'),
             ('the backbone accessor, system S', lambda: ens.backbone_list('backbone_pairs', S), 'invalid system')]
    n_ok = 0
    for what, call, reason in cases:
        try:
            call()
            print('%-44s no error' % what)
        except RuntimeError as err:
            print('%-44s %s' % (what, err))
            n_ok += reason in str(err)
    assert n_ok == len(cases), '%d of %d' % (n_ok, len(cases))
    a = ens.walked_lists('rotamer', 1, 1); b = ens.walked_lists('rotamer', 1, 1)
    same_rec = all((a[k] is None and b[k] is None) or np.array_equal(a[k], b[k]) for k in a)
    e1, d1 = ens.energies_and_derivs()
    same = e1.tobytes() == e0.tobytes() and d1.tobytes() == d0.tobytes()
    print('two reads agree: %s; a compute afterwards returns the bits of the one before: %s' % (same_rec, same))
    assert same and same_rec
    ens.close()


CHECKS = dict(static=static, md=md, radial=radial, backbone=backbone, backbone_nolist=backbone_nolist, refusals=refusals)

if __name__ == '__main__':
    which, work = sys.argv[1], sys.argv[2]
    CHECKS[which](work, *sys.argv[3:])
    print('CHECK %s PASSED' % which)
