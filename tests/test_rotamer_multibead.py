"""CPU tests: a side-chain library with two beads per rotamer state (tests/rotamer_multibead.py), and the oracle on it against golden
vectors of the compiled unmodified reference (tests/golden/multibead_proteinG56.golden.npz, tools/make_fixtures.py --multibead).

Tolerances follow parity_util.golden_tol: max(1e-5, 2 x the reference's own -O1-against-O3 spread on this configuration)
(tests/golden/reference_noise_floor.json, tools/noise_floor.py multibead_proteinG56: forces 5.9e-6, worst sensitivity 1.1e-5,
side-chain parameter derivative 5.2e-6); node outputs and per-node potentials 1e-5, named values as in tests/test_oracle_pinning.py."""
import numpy as np
import pytest
import parity_util as P
import rotamer_multibead as M


@pytest.fixture(scope='module')
def made(tmp_path_factory):
    return M.write_configuration(tmp_path_factory.mktemp('multibead'))


def test_library_has_states_with_two_beads(made):
    path, info, n_type = made
    count = M.beads_per_state(path)
    assert set(count.values()) == {1, 2} and n_type == 20 + len(M.TWO_BEADS)
    for n_rot in (1, 3, 6):                    # a 1-state, a 3-state and a 6-state residue type with two beads, and one-bead states beside them
        assert any(v == 2 for (r, _, _), v in count.items() if r == n_rot), n_rot
        assert any(v == 1 for (r, _, _), v in count.items() if r == n_rot), n_rot
    seq = P.pkg.config.PROTEIN_G
    two = sum(seq.count(a) for a in 'ATKE')
    assert two == 28 and info['n_bead'] == sum(count.values())
    with P.pkg.h5lite.open_file(path) as t, P.pkg.h5lite.open_file(P.fixture('proteinG56_7A')) as t0:
        assert info['n_bead'] > t0.group('input/potential/rotamer').shape('pair_interaction/id')[0]
        pos = t.group('input/potential/placement_fixed_point_vector_only').read('placement_data', 'f8')
        layer = t.group('input/potential/placement_fixed_point_vector_only').read('layer_index', 'i4')
    ids = sorted(count)                          # the second bead of a state sits 1 A from the first, along the stored direction
    pairs = [(layer[i], layer[i + 1]) for i in range(len(layer) - 1)
             if layer[i + 1] == layer[i] + 1 and np.allclose(pos[layer[i], 3:6], pos[layer[i + 1], 3:6]) and
             abs(np.linalg.norm(pos[layer[i + 1], :3] - pos[layer[i], :3]) - 1.) < 1e-6]
    assert len(pairs) >= sum(1 for v in count.values() if v == 2) and ids


def test_oracle_matches_reference_golden_on_two_beads_per_state(made):
    path, info, n_type = made
    g = dict(np.load(M.GOLDEN))
    up = P.pkg.Upside(path, library=P.oracle_library())
    assert np.array_equal(up.initial_pos, g['pos'])
    act = M.record(up, path, n_type)
    pairs = P.oracle_pairlist(up, 'rotamer')
    up.close()
    tol_d, tol_s, tol_p = (P.golden_tol(M.NAME, 'pos', k) for k in ('deriv', 'sens', 'param_deriv'))
    assert 1e-5 <= tol_d < 1.3e-5 and 1e-5 <= tol_s < 2.4e-5 and 1e-5 <= tol_p < 1.2e-5
    assert P.rel_rms(g['deriv'], act['deriv']) < tol_d, P.rel_rms(g['deriv'], act['deriv'])
    scale = sum(abs(float(act['pot/' + k])) for k in P.POTENTIAL_NODES)
    assert abs(float(act['energy']) - float(g['energy'])) < 1e-5 * scale
    n_checked = 0
    for k in sorted(g):
        if k.startswith('out/') and g[k].size:
            assert P.rel_rms(g[k], act[k]) < 1e-5, (k, P.rel_rms(g[k], act[k]))
        elif k.startswith('sens/') and g[k].size:
            assert P.rel_rms(g[k], act[k]) < tol_s, (k, P.rel_rms(g[k], act[k]))
        elif k.startswith('pot/'):
            assert abs(float(g[k]) - float(act[k])) < 1e-5 * max(1., abs(float(g[k]))), (k, g[k], act[k])
        else:
            continue
        n_checked += 1
    assert n_checked >= 2 * len(P.COORD_NODES) - 2 + len(P.POTENTIAL_NODES)
    m = g['rotamer/node_energy'] < 1e4
    assert int(act['rotamer/n_node']) == int(g['rotamer/n_node']) == 56
    assert np.abs(act['rotamer/node_energy'] - g['rotamer/node_energy'])[m].max() < 5e-4
    assert np.array_equal(act['rotamer/node_energy'][~m], g['rotamer/node_energy'][~m])
    assert np.abs(act['rotamer/rotamer_free_energy'] - g['rotamer/rotamer_free_energy']).max() < 2e-4
    assert np.abs(act['rotamer/rotamer_1body_energy'] - g['rotamer/rotamer_1body_energy']).max() < 2e-4
    assert np.array_equal(act['rotamer/count_edges_by_type'], g['rotamer/count_edges_by_type'])
    assert g['rotamer/count_edges_by_type'][20:].sum() > 0                    # bead pairs of the new types are in range
    assert P.rel_rms(g['param_deriv/rotamer'], act['param_deriv/rotamer']) < tol_p
    assert np.abs(g['param_deriv/rotamer'][20:]).max() > 0
    assert np.array_equal(pairs, g['pairlist/edges'][:, :2])
