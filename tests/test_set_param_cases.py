"""The perturbed tables of set_param_cases.py, checked on the oracle alone (no GPU): every case loads, gives finite forces and a
converged side-chain solve, moves what it is meant to move, and -- for the interaction-graph nodes, whose set_param the oracle serves --
the oracle after its own set_param on an engine of the old file equals a fresh oracle engine of the rewritten file.  These are
conditions on the INPUTS of test_gpu_set_param.py: a case that did not move its node would let a set_param that does nothing pass."""
import numpy as np
import pytest
import parity_util as P
import set_param_cases as C

MAX_ITER = 1000      # the solve's sweep limit in every fixture (rotamer's max_iter attribute)


@pytest.fixture(scope='module')
def oracle():
    return P.oracle_library()


@pytest.mark.parametrize('case', sorted(C.CASES))
def test_case_is_loadable_and_not_vacuous(oracle, tmp_path, case):
    fixture = C.fixture_of(case)
    path = str(tmp_path / (case + '.up'))
    old, new = C.build(case, path)
    ec, ep = C.extras(fixture)
    pos, pos2 = C.positions(fixture)
    o_old = P.pkg.Upside(P.fixture(fixture), library=oracle)
    o_new = P.pkg.Upside(path, library=oracle)      # loads
    r_old = P.evaluate_all(o_old, pos, ec, ep)
    r_new = P.evaluate_all(o_new, pos, ec, ep)
    assert np.isfinite(r_new['deriv']).all() and np.isfinite(float(r_new['energy']))
    sweeps = o_new.calc.oracle_rotamer_iterations(o_new.engine)
    assert 0 < sweeps < MAX_ITER, sweeps
    assert int(o_new.get_value_by_name((1,), 'rotamer', 'read n_bad_solve')[0]) == 0
    for node in C.nodes_of(case):
        assert not np.array_equal(old[node], new[node]), node
        k = C.own_key(fixture, node)
        assert P.rel_rms(r_old[k], r_new[k]) > 1e-3, (node, P.rel_rms(r_old[k], r_new[k]))
    moved = P.rel_rms(r_old['deriv'], r_new['deriv'])
    assert moved > 1e-2, moved
    # the oracle agrees with itself: set_param on the engine of the old file, lists already built at the old cut-off
    settable = [n for n in C.nodes_of(case) if n in C.ORACLE_SETTABLE]
    if settable:
        for node in settable:
            assert np.array_equal(o_old.get_param(new[node].shape, node), old[node]), node
            o_old.set_param(new[node], node)
            assert np.array_equal(o_old.get_param(new[node].shape, node), new[node]), node
        if len(settable) == len(C.nodes_of(case)):
            for p in (pos, pos2):
                r_set = P.evaluate_all(o_old, p, ec, ep)
                r_fresh = P.evaluate_all(o_new, p, ec, ep)
                assert not P.compare(r_fresh, r_set, rtol=1e-7)
                for node in C.PAIRLIST_NODES:
                    assert np.array_equal(P.oracle_pairlist(o_old, node), P.oracle_pairlist(o_new, node)), node
                assert o_old.calc.oracle_rotamer_iterations(o_old.engine) == o_new.calc.oracle_rotamer_iterations(o_new.engine)
    o_old.close(); o_new.close()


def test_side_chain_table_keeps_its_symmetry(tmp_path):
    """the rules update_cutoffs checks: mirror entries exchange their angular halves and share the radial part"""
    _, new = C.build('rotamer', str(tmp_path / 'r.up'))
    shape = C.table_shape(P.fixture('trpcage20_7A'), 'rotamer')
    T = new['rotamer'].reshape(shape)
    na = (shape[2] - 2 * C._ROTAMER_KNOTS[shape[2]]) // 2
    M = T.transpose(1, 0, 2)
    assert np.array_equal(M[..., :na], T[..., na:2 * na]) and np.array_equal(M[..., na:2 * na], T[..., :na])
    assert np.array_equal(M[..., 2 * na:], T[..., 2 * na:])


@pytest.mark.parametrize('case', ['placement_fixed_point_vector_only', 'placement_fixed_point_vector_only_CB', 'placement_fixed_point_vector_scalar'])
def test_placement_directions_stay_unit_vectors(tmp_path, case):
    """the angular splines are not clamped: a direction longer than 1 is outside the domain of every engine"""
    old, new = C.build(case, str(tmp_path / 'p.up'))
    shape = C.table_shape(P.fixture(C.fixture_of(case)), case)
    for T in (old[case].reshape(shape), new[case].reshape(shape)):
        assert np.abs(np.sqrt((T[:, 3:6].astype('f8') ** 2).sum(axis=1)) - 1.).max() < 1e-6
    assert P.rel_rms(old[case].reshape(shape)[:, 3:6], new[case].reshape(shape)[:, 3:6]) > 1e-2      # ... and they do turn


def test_cut_offs_move_as_stated(oracle, tmp_path):
    """environment_coverage's pair count follows p[0] + 1 / p[1] up and down (308 -> 418 pairs on trpcage20_7A at +1.0 A), and
    hbond_sc_radial's potential follows its table (14.4 -> 33.0 on proteinG56_restraints)"""
    pos = C.positions('trpcage20_7A')[0]
    n = {}
    for case in ('environment_coverage_grow', 'environment_coverage_shrink'):
        path = str(tmp_path / (case + '.up'))
        C.build(case, path)
        o = P.pkg.Upside(path, library=oracle)
        o.deriv(pos)
        n[case] = len(P.oracle_pairlist(o, 'environment_coverage'))
        o.close()
    o = P.pkg.Upside(P.fixture('trpcage20_7A'), library=oracle)
    o.deriv(pos)
    n0 = len(P.oracle_pairlist(o, 'environment_coverage'))
    o.close()
    assert (n0, n['environment_coverage_grow']) == (308, 418)
    assert n['environment_coverage_shrink'] < n0
    fx = 'proteinG56_restraints'
    path = str(tmp_path / 'radial.up')
    C.build('hbond_sc_radial', path)
    pot = []
    for f in (P.fixture(fx), path):
        o = P.pkg.Upside(f, library=oracle)
        o.energy(C.positions(fx)[0])
        pot.append(float(o.get_output('hbond_sc_radial')[0, 0]))
        o.close()
    assert abs(pot[0] - 14.4) < 0.05 and abs(pot[1] - 33.0) < 0.05, pot
