"""Device side of test_gpu_set_param.py.  Imported, it gives the helpers that take a snapshot of an engine (every result of
evaluate_all, the five canonical pair lists, the side-chain solve's sweep count and n_bad_solve) in one flat dict.  Run as a
program, it does the work of one case under whatever UPSIDE_HIP_* environment the parent set (the switches are read once per
process) and saves the snapshots:

  tables CASE NEW_FILE OUT         engine of the old file, lists built at the old cut-off, set_param of every table of the case, then
                                   the snapshot at pos and pos2 ('set:...'), the same of a fresh engine of NEW_FILE ('fresh:...') and the
                                   parameter derivatives of both after pos2 ('set:param_deriv/...')
  md CASE NEW_FILE OUT READBACK    four systems: run_steps(30), get_pos() only if READBACK is 1, set_param, run_steps(30); then pos, mom,
                                   the energies and forces of a force pass at the final coordinates and every system's pair lists"""
import ctypes as ct
import sys
import numpy as np
import parity_util as P
import set_param_cases as C


def bind(c):
    c.upside_hip_get_pairlist.restype = ct.c_int
    c.upside_hip_get_pairlist.argtypes = [ct.c_void_p, ct.c_char_p, ct.c_int, ct.c_int, ct.c_void_p, ct.c_void_p]
    c.upside_hip_rotamer_iterations.argtypes = [ct.c_void_p, ct.c_void_p]
    c.upside_hip_get_param_deriv.argtypes = [ct.c_void_p, ct.c_char_p, ct.c_int, ct.c_int, ct.c_void_p]
    c.upside_hip_last_error.restype = ct.c_char_p
    return c


def hip_pairlist(up, node, system=0, cap=400000):
    i1 = np.zeros(cap, 'i4'); i2 = np.zeros(cap, 'i4')
    n = up.calc.upside_hip_get_pairlist(ct.c_void_p(up.engine), node.encode(), int(system), cap, i1.ctypes.data, i2.ctypes.data)
    assert 0 <= n <= cap, (node, n)
    return np.column_stack((i1[:n], i2[:n]))


def hip_sweeps(up, n_system=1):
    it = np.zeros(n_system, 'i4')
    assert up.calc.upside_hip_rotamer_iterations(ct.c_void_p(up.engine), it.ctypes.data) == 0
    return it


def snapshot(up, fixture, pos, pairlist, sweeps):
    """flat dict of one evaluation: evaluate_all's keys, 'pairlist/<node>', 'sweeps', 'n_bad'"""
    ec, ep = C.extras(fixture)
    res = dict(P.evaluate_all(up, pos, ec, ep))
    for node in C.PAIRLIST_NODES:
        res['pairlist/' + node] = pairlist(up, node)
    res['sweeps'] = np.int64(sweeps(up))
    res['n_bad'] = np.int64(up.get_value_by_name((1,), 'rotamer', 'read n_bad_solve')[0])
    return res


def hip_snapshot(up, fixture, pos):
    return snapshot(up, fixture, pos, hip_pairlist, lambda u: int(hip_sweeps(u)[0]))


def oracle_snapshot(orc, fixture, pos):
    return snapshot(orc, fixture, pos, P.oracle_pairlist, lambda u: u.calc.oracle_rotamer_iterations(u.engine))


def param_derivs(up, nodes, tables):
    """get_param_deriv of the last force pass, flat, for the nodes that serve one"""
    return dict(('param_deriv/' + n, up.get_param_deriv(tables[n].shape, n)) for n in nodes if n not in C.NO_PARAM_DERIV)


def check_get_param(up, node, table):
    got = up.get_param(table.shape, node)
    assert got.tobytes() == table.tobytes(), 'get_param of %s is not the table, bit for bit, in file order' % node


def set_tables(up, nodes, old, new):
    for node in nodes:
        check_get_param(up, node, old[node])
        up.set_param(new[node], node)
        check_get_param(up, node, new[node])


def sub(d, prefix):
    return dict((k[len(prefix):], d[k]) for k in d if k.startswith(prefix))


def run_tables(case, new_file, out):
    fixture, nodes = C.fixture_of(case), C.nodes_of(case)
    old = dict((n, C.read_table(P.fixture(fixture), n)) for n in nodes)
    new = dict((n, C.read_table(new_file, n)) for n in nodes)
    pos, pos2 = C.positions(fixture)
    res = {}
    up = P.pkg.Upside(P.fixture(fixture)); bind(up.calc)
    up.deriv(pos)                      # the lists exist at the old cut-off
    set_tables(up, nodes, old, new)
    fresh = P.pkg.Upside(new_file)
    for tag, u in (('set', up), ('fresh', fresh)):
        for ptag, x in (('pos', pos), ('pos2', pos2)):
            for k, v in hip_snapshot(u, fixture, x).items():
                res['%s:%s:%s' % (tag, ptag, k)] = v
        for k, v in param_derivs(u, nodes, new).items():
            res['%s:%s' % (tag, k)] = v
    up.close(); fresh.close()
    np.savez(out, **res)


def run_md(case, new_file, out, readback):
    fixture, nodes = C.fixture_of(case), C.nodes_of(case)
    new = dict((n, C.read_table(new_file, n)) for n in nodes)
    S = 4
    ens = P.pkg.engine.Ensemble(P.fixture(fixture), S); bind(ens.calc)
    ens.set_pos(C.positions(fixture)[0])
    ens.init_md(np.linspace(0.8, 0.9, S), 5)
    ens.run_steps(30)
    res = {}
    if readback:
        res['mid'] = ens.get_pos()
    for n in nodes:                    # (the steps above may still be in flight)
        ens.set_param(new[n], n)
    ens.run_steps(30)
    res['pos'] = ens.get_pos(); res['mom'] = ens.get_mom()
    res['energy'], res['force'] = ens.energies_and_derivs()
    for s in range(S):
        for node in C.PAIRLIST_NODES:
            res['pairlist/%d/%s' % (s, node)] = hip_pairlist(ens, node, s)
    ens.close()
    np.savez(out, **res)


if __name__ == '__main__':
    if sys.argv[1] == 'tables':
        run_tables(*sys.argv[2:5])
    elif sys.argv[1] == 'md':
        run_md(sys.argv[2], sys.argv[3], sys.argv[4], sys.argv[5] == '1')
    else:
        raise SystemExit('unknown mode %r' % sys.argv[1])
