"""GPU tests (run with -m gpu on an MI355X): a side-chain library with two beads per rotamer state (tests/rotamer_multibead.py) through the
product, against the oracle on the same configuration (tests/test_rotamer_multibead.py pins the oracle on it to the reference).

With two beads in a state, an entry of a pair matrix has up to four contributing bead pairs (accumulated with float atomics, energy form),
the 1-body energy of a state sums over its beads, and the gradient pass and the parameter derivative walk the bead list of every state:
code that the shipped one-bead libraries run with a single contribution per entry.  Each case runs in a worker process (the switches are
read once per process): the default selection, the large-batch selection with the layout launch, and the alternate pair, gradient and
solve passes."""
import os
import subprocess
import sys
import numpy as np
import pytest
import parity_util as P
import rotamer_multibead as M
import rotamer_forms_cases as C

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))

CASES = [
    ('default', {}),
    ('large_batch_layout1', dict(C.BASE, UPSIDE_HIP_BP_LAYOUT='1')),       # the layout launch in front of a solve that must fold itself
    ('sort_beads0', {'UPSIDE_HIP_ROT_SORT_BEADS': '0'}),                   # beads in the configuration's order: a state's two beads still adjacent, nodes not
    ('rot_unstaged', {'UPSIDE_HIP_ROT_UNSTAGED': '1'}),
    ('rot_poly0', {'UPSIDE_HIP_ROT_POLY': '0'}),
    ('pair2_0', {'UPSIDE_HIP_PAIR2': '0'}),
    ('cluster6', {'UPSIDE_HIP_BP_CLUSTER': '6'}),
]


@pytest.fixture(scope='module')
def setup(tmp_path_factory):
    """the configuration, the two structures, and the oracle's answers: computed once, shared, left unchanged"""
    tmp = tmp_path_factory.mktemp('multibead_gpu')
    path, info, n_type = M.write_configuration(tmp)
    g = dict(np.load(M.GOLDEN))
    pos = g['pos']
    pos2 = (pos + 0.05 * np.random.RandomState(112).normal(size=pos.shape)).astype('f4')
    posfile = str(tmp / 'pos.npz')
    np.savez(posfile, pos=np.stack([pos, pos2, pos]).astype('f4'))
    shp = (n_type, n_type, 62)
    orc = P.pkg.Upside(path, library=P.oracle_library())
    ref = M.record(orc, path, n_type)
    ref['rotamer/edge_energy'] = orc.get_value_by_name((56, 56, 6, 6), 'rotamer', 'edge_energy')
    pairs = P.oracle_pairlist(orc, 'rotamer')
    orc.close()
    orc = P.pkg.Upside(path, library=P.oracle_library())
    ref2 = dict(energy=np.float32(orc.energy(pos2)), deriv=orc.deriv(pos2))
    ref2['param_deriv'] = orc.get_param_deriv(shp, 'rotamer')
    pairs2 = P.oracle_pairlist(orc, 'rotamer')
    md = []
    for s in range(3):      # system s uses seed + s
        p = pos.copy(); m = np.zeros_like(p)
        orc.calc.oracle_run_md(orc.engine, p.ctypes.data, m.ctypes.data, 4, 0.009, 0.8, 12345 + s, 5.0, 1)
        md.append((p, m))
    orc.close()
    assert np.array_equal(pairs, g['pairlist/edges'][:, :2]) and P.rel_rms(ref['deriv'], ref2['deriv']) > 1e-3
    return dict(tmp=tmp, path=path, n_type=n_type, posfile=posfile, golden=g, ref=ref, ref2=ref2, pairs=pairs, pairs2=pairs2, md=md, runs={})


def run_case(setup, tag):
    if tag not in setup['runs']:
        out = str(setup['tmp'] / (tag + '.npz'))
        env = {k: v for k, v in os.environ.items() if not k.startswith('UPSIDE_HIP_')}
        env.update(dict(CASES)[tag])
        r = subprocess.run([sys.executable, os.path.join(HERE, 'rotamer_multibead_worker.py'), setup['path'], out, setup['posfile'],
                            str(setup['n_type'])], env=env, cwd=HERE, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=180)
        assert r.returncode == 0, (tag, r.stdout.decode()[-2000:])
        setup['runs'][tag] = dict(np.load(out))
    return setup['runs'][tag]


@pytest.mark.parametrize('tag', [t for t, _ in CASES])
def test_two_beads_per_state_match_oracle(setup, tag):
    """every node's output and sensitivities, energies, forces, the side-chain named values, the parameter derivative of every system and
    the pair list of the side-chain graph, one system and three"""
    r = run_case(setup, tag)
    ref, ref2, g = setup['ref'], setup['ref2'], setup['golden']
    one = {k[len('one/'):]: v for k, v in r.items() if k.startswith('one/')}
    for k in ('ens_form/', 'one_form/'):      # energy form, whatever else the case selects; the solve folds itself
        assert int(r[k + 'p_prob']) == 0 and int(r[k + 'select_prefold']) == 0, (tag, k)
    if tag == 'large_batch_layout1':
        assert int(r['ens_form/node_prob_in_solve']) == 0 and (r['ens_form/words'] == 0).all()      # the layout launch ran and laid every system out
    if tag == 'cluster6':
        assert int(r['ens_form/cluster']) == 1
    keys = ['energy', 'deriv'] + [k for k in ref if k.startswith(('out/', 'sens/', 'pot/'))]
    bad = P.compare(ref, one, keys=keys, rtol=P.RTOL, verbose=True)
    for s, rr in enumerate((ref, ref2, ref)):
        bad += [(s,) + b for b in P.compare(dict(energy=rr['energy'], deriv=rr['deriv']), dict(energy=r['ens_energy'][s], deriv=r['ens_force'][s]), rtol=P.RTOL, verbose=True)]
    assert not bad, (tag, bad)
    # named values, as test_rotamer_named_values holds them
    m = g['rotamer/node_energy'] < 1e4
    ne = one['rotamer/node_energy']
    assert np.abs(ne - g['rotamer/node_energy'])[m].max() < 5e-4 and np.array_equal(ne[~m], g['rotamer/node_energy'][~m])
    assert np.abs(ne - ref['rotamer/node_energy'])[m].max() < 2e-5
    fe = one['rotamer/rotamer_free_energy']
    assert np.abs(fe - g['rotamer/rotamer_free_energy']).max() < 2e-4 and np.abs(fe - ref['rotamer/rotamer_free_energy']).max() < 5e-5
    assert np.abs(one['rotamer/rotamer_1body_energy'] - g['rotamer/rotamer_1body_energy']).max() < 2e-4
    ee, eo = one['rotamer/edge_energy'], ref['rotamer/edge_energy']
    assert np.array_equal(ee != 0, eo != 0) and np.abs(ee - eo).max() < 2e-5 * max(1., np.abs(eo).max())
    assert int(one['n_bad'][0]) == 0 and np.array_equal(one['rotamer/count_edges_by_type'], ref['rotamer/count_edges_by_type'])
    assert abs(float(fe.sum()) - float(one['pot/rotamer'])) < 1e-3 * max(1., np.abs(fe).sum())
    # parameter derivative of every system
    pd = r['ens_param_deriv']
    errs = [P.rel_rms(ref['param_deriv/rotamer'], one['param_deriv/rotamer']), P.rel_rms(ref['param_deriv/rotamer'], pd[0]),
            P.rel_rms(ref2['param_deriv'], pd[1]), P.rel_rms(ref['param_deriv/rotamer'], pd[2])]
    print('param deriv rel_rms', errs)
    assert max(errs) < P.RTOL, (tag, errs)
    assert P.rel_rms(pd[0], pd[1]) > 1e-3 and np.abs(pd[0][20:]).max() > 0
    # pair lists, bit for bit
    assert np.array_equal(r['ens_pairs0'], setup['pairs']) and np.array_equal(r['ens_pairs2'], setup['pairs'])
    assert np.array_equal(r['ens_pairs1'], setup['pairs2'])


def test_md_of_two_beads_per_state_matches_oracle(setup):
    """4 rounds (12 steps) of 3 systems, at the tolerances of test_thermostat_and_integrator_match_oracle"""
    r = run_case(setup, 'default')
    for s, (p, m) in enumerate(setup['md']):
        ep, em = P.rel_rms(p, r['md_pos'][s]), P.rel_rms(m, r['md_mom'][s])
        print('system %d: pos rel_rms %.3e mom rel_rms %.3e' % (s, ep, em))
        assert ep < 1e-5 and em < 1e-3, (s, ep, em)
    assert not np.array_equal(r['md_pos'][0], r['md_pos'][1])


def test_repeated_evaluations_of_two_beads_per_state_agree(setup):
    """the several-beads form accumulates with float atomics in no fixed order: repeated evaluations of the same structures agree within
    2e-6 (whether they return the same bits is measured, profiles/rotamer_forms.txt, not required), and so do two systems with the same
    structure"""
    for tag in ('default', 'large_batch_layout1'):
        r = run_case(setup, tag)
        print('%s: %d distinct results in 11 evaluations, worst rel_rms to the first %.3e; systems 0 and 2 bit-equal: %s'
              % (tag, int(r['repeat_distinct']), float(r['repeat_worst']), np.array_equal(r['ens_force'][0], r['ens_force'][2])))
        assert float(r['repeat_worst']) < 2e-6
        assert P.rel_rms(r['ens_force'][0], r['ens_force'][2]) < 2e-6
