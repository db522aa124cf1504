"""Side-chain solve: the energy form of the pair matrices on the paths a large batch selects (the tests marked gpu need an MI355X; the
check of the fixtures runs on the oracle alone).

Every shipped side-chain library keeps its pair matrices as exp(-E); a library with several beads per state, UPSIDE_HIP_ROTAMER_ATOMIC=1,
UPSIDE_HIP_BP_ENERGY_TABLE=1 and every cluster solve keep E and leave the exp to the solve.  From 512 systems on the inbox layout and the
fold of the edges to 1-state partners run as a launch in front of the solve -- before the solve's exp pass.  tests/rotamer_forms_cases.py
has the cases; each runs in a worker process, since the switches are read once per process, and each worker reports through the
side-chain node's `solve_form` read-out which form and which fold it ran, so that a case that quietly took another path fails."""
import os
import subprocess
import sys
import numpy as np
import pytest
import parity_util as P
import rotamer_forms_cases as C

HERE = os.path.dirname(os.path.abspath(__file__))
SMALL = 'proteinG56_7A'
LARGE = 'trpcage20_7A'


def run_worker(tmp_path, name, tag, posfile, env_extra):
    out = str(tmp_path / (tag + '.npz'))
    env = {k: v for k, v in os.environ.items() if not k.startswith('UPSIDE_HIP_')}      # the cases name every switch they run under
    env.update(env_extra)
    r = subprocess.run([sys.executable, os.path.join(HERE, 'rotamer_forms_worker.py'), name, out, posfile], env=env, cwd=HERE,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=180)
    if r.returncode != 0:
        return 'worker of case %s failed (exit status %d): %s' % (tag, r.returncode, r.stdout.decode()[-1500:])      # (the tests of that case fail, the other cases still run)
    return dict(np.load(out))


def ran(r):
    assert not isinstance(r, str), r
    return r


def assert_fixture_can_tell(name, pos, min_folded):
    cls, folded = C.fold_condition(name, pos)
    assert all(cls.values()), (name, cls)
    assert folded >= min_folded, (name, folded)


def figures(ref, act, keys_force, keys_energy, what):
    """every figure printed before any is asserted"""
    rows = [(k, P.rel_rms(ref[k], act[k])) for k in keys_force]
    for k, err in rows:
        print('%-24s %-12s rel_rms %.3e' % (what, k, err))
    for k in keys_energy:
        print('%-24s %-12s max |dE| %.3e' % (what, k, float(np.abs(np.asarray(ref[k], 'f8') - act[k]).max())))
    return rows


def assert_same(ref, act, keys_force, keys_energy, what, rows):
    for k, err in rows:
        assert err < 2e-6, (what, k, err)
    for k in keys_energy:
        assert np.allclose(ref[k], act[k], rtol=2e-6, atol=1e-3), (what, k, ref[k], act[k])


def assert_form(res, prefix, want, n_system, what):
    got = {k[len(prefix):]: v for k, v in res.items() if k.startswith(prefix)}
    for k in ('p_prob', 'node_prob_in_solve', 'layout', 'cluster'):
        assert int(got[k]) == want[k], (what, prefix, k, got, want)
    words = got['words']
    assert words.shape == (n_system,) and (words == want['word']).all(), (what, prefix, words, want)
    # the solve takes the layout launch's fold over where the library selects it, for the systems that launch laid out
    prefold = int(got['select_prefold']) and want['compact'] and not want['cluster'] and bool((words == 0).all())
    assert int(prefold) == want['prefold'], (what, prefix, got, want)


@pytest.fixture(scope='module')
def small_runs(tmp_path_factory):
    """the default path and every case of rotamer_forms_cases.CASES on 3 systems of the 56-residue fixture: evaluated once, shared"""
    tmp = tmp_path_factory.mktemp('rotamer_forms')
    g = P.golden(SMALL)
    posfile = str(tmp / 'pos.npz')
    np.savez(posfile, pos=np.stack([g['pos'], g['pos2'], g['pos']]).astype('f4'))
    runs = {'default': run_worker(tmp, SMALL, 'default', posfile, {})}
    for tag, extra in C.CASES:
        runs[tag] = run_worker(tmp, SMALL, tag, posfile, dict(C.BASE, **extra))
    return runs


def test_fixtures_can_tell_a_wrong_fold():
    """on the oracle, at the golden structures: every slot class has an active slot and at least 10 multi-state nodes of the 56-residue fixture
    carry folded 1-state partners worth more than 1e-3 -- a fold that multiplied by anything but exp(-E) moves their probabilities at first
    order.  (The 20-residue fixture has 9 such nodes at its first structure: too few for the crossed cases, enough for the 512-system one,
    which asks for an active edge from a multi-state node to a 1-state partner.)"""
    for name, min_folded in ((SMALL, 10), (LARGE, 1)):
        g = P.golden(name)
        assert_fixture_can_tell(name, g['pos'], min_folded)
        assert_fixture_can_tell(name, g['pos2'], min_folded)


@pytest.mark.gpu
def test_control_matches_oracle(small_runs):
    """the large-batch selection in the probability form, forced at 3 systems, against the oracle: every node's output and sensitivities of the
    first structure, energy and forces of the second, and the 3-system engine"""
    g = P.golden(SMALL)
    orc = P.pkg.Upside(P.fixture(SMALL), library=P.oracle_library())
    ref = P.evaluate_all(orc, g['pos'])
    ref2 = dict(energy=np.float32(orc.energy(g['pos2'])), deriv=orc.deriv(g['pos2']))
    orc.close()
    for tag in ('control', 'layout1'):
        r = ran(small_runs[tag])
        bad = P.compare(ref, {k[len('one/'):]: v for k, v in r.items() if k.startswith('one/')}, rtol=P.RTOL)
        bad += P.compare(ref2, dict(energy=r['one_energy2'], deriv=r['one_force2']), rtol=P.RTOL)
        for s, rr in enumerate((ref, ref2, ref)):
            bad += P.compare(dict(energy=rr['energy'], deriv=rr['deriv']), dict(energy=r['ens_energy'][s], deriv=r['ens_force'][s]), rtol=P.RTOL)
        assert not bad, (tag, bad)


@pytest.mark.gpu
@pytest.mark.parametrize('tag', [t for t, _ in C.CASES])
def test_energy_form_on_large_batch_paths(small_runs, tag):
    """forces and energies of every case agree with the default path of the same process layout, and the case ran the form, the layout launch
    and the fold it names"""
    extra = dict(C.CASES)[tag]
    base, r = ran(small_runs['default']), ran(small_runs[tag])
    want = C.expected_form(extra, 3)
    keys = (('one/deriv', 'one_force2', 'ens_force'), ('one/energy', 'one_energy2', 'ens_energy'))
    rows = figures(base, r, keys[0], keys[1], tag)
    assert_form(r, 'ens_form/', want, 3, tag)
    assert_form(r, 'one_form/', want, 1, tag)
    assert_same(base, r, keys[0], keys[1], tag, rows)


@pytest.mark.gpu
def test_energy_form_at_512_systems(tmp_path):
    """the selection 512 systems get by default (layout launch and pre-fold allocated by the batch size, nothing forced) with the accumulating
    energy form: every system against the same engine in the probability form, three of them against the oracle"""
    g = P.golden(LARGE)
    S = 512
    rng = np.random.RandomState(512)
    pos = (g['pos'][None].astype('f8') + 0.05 * rng.standard_normal((S,) + g['pos'].shape)).astype('f4')
    posfile = str(tmp_path / 'pos.npz')
    np.savez(posfile, pos=pos)
    for s in (0, 255, 511):                      # the perturbed structures keep what the check needs: every slot class active, multi-state nodes with folded 1-state partners
        assert_fixture_can_tell(LARGE, pos[s], 1)
    prob = ran(run_worker(tmp_path, LARGE, 'prob', posfile, {}))
    atom = ran(run_worker(tmp_path, LARGE, 'atomic', posfile, C.ATOMIC))
    worst = max(P.rel_rms(prob['ens_force'][s], atom['ens_force'][s]) for s in range(S))
    print('512 systems: worst per-system force rel_rms %.3e, max |dE| %.3e' % (worst, float(np.abs(prob['ens_energy'].astype('f8') - atom['ens_energy']).max())))
    common = dict(node_prob_in_solve=0, layout=1, cluster=0, word=0, compact=True)
    assert_form(prob, 'ens_form/', dict(common, p_prob=1, prefold=1), S, 'probability form')
    assert_form(atom, 'ens_form/', dict(common, p_prob=0, prefold=0), S, 'energy form')
    orc = P.pkg.Upside(P.fixture(LARGE), library=P.oracle_library())
    for s in (0, 255, 511):
        ref = dict(energy=np.float32(orc.energy(pos[s])), deriv=orc.deriv(pos[s]))
        for what, r in (('probability form', prob), ('energy form', atom)):
            bad = P.compare(ref, dict(energy=r['ens_energy'][s], deriv=r['ens_force'][s]), rtol=P.RTOL)
            assert not bad, (what, s, bad)
    orc.close()
    assert worst < 2e-6
    assert np.allclose(prob['ens_energy'], atom['ens_energy'], rtol=2e-6, atol=1e-3)
