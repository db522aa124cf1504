"""GPU tests of the pair passes' gradient accumulators at the limits of their range and resolution (cases: accumulator_cases.py).

The partner side of every pair gradient is summed in 64-bit fixed point: the packed passes (hbond_coverage graphs, side-chain gradient;
pair2_device.h) in counts of 2^-22 through a 32-bit conversion that holds |v| < 512 and a wide path beyond it, the scalar passes
(UPSIDE_HIP_PAIR2=0, and every other pair graph; device_math.h: to_fixed32) in counts of 2^-32 for |v| < 2^31.  The shipped force
field stays an order of magnitude below 512, so these tests make it steeper by powers of two -- exact in fp32, so that the oracle and
all float arithmetic of the product scale exactly, the rounding of the fixed point stays absolute, and a case that passes at k = 1 can
fail at a larger k only through range -- and flatter, where the absolute rounding is what is left.

Chains A, B and C (environment coupling, hydrogen-bond energy, both) never reach a packed pass: its pair sensitivities are rotamer
marginals.  They passed before the wide path as they do with it.  Chain D (the hbond_coverage tables) does.  Without the wide path,
relative RMS error against the oracle at k = 2^8 / 2^12 / 2^16: forces 0.21 / 0.57 / 0.60 and sens/protein_hbond 0.43 / 0.95 / 0.997 on
trpcage20_7A, forces 0.45 and sens/protein_hbond 0.96 on proteinG56_7A at 2^12; with it 1.4e-6 .. 2.1e-6.  A table 2^28 times as steep
was evaluated without any error; it is refused now."""
import ctypes as ct
import os
import subprocess
import sys
import numpy as np
import pytest
import parity_util as P
import accumulator_cases as AC

pytestmark = pytest.mark.gpu
RTOL = P.RTOL
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope='module')
def hip():
    import torch
    assert torch.cuda.is_available(), 'these tests need a GPU'
    lib = P.pkg.default_library()     # raises when the HIP extension is missing: no fallback
    c = lib.calc
    c.upside_hip_get_pairlist.restype = ct.c_int
    c.upside_hip_get_pairlist.argtypes = [ct.c_void_p, ct.c_char_p, ct.c_int, ct.c_int, ct.c_void_p, ct.c_void_p]
    c.upside_hip_last_error.restype = ct.c_char_p
    P.pkg.engine.Ensemble._bind(c)
    return lib


def hip_pairlist(up, node, sys=0, cap=400000):
    i1 = np.zeros(cap, 'i4'); i2 = np.zeros(cap, 'i4')
    n = up.calc.upside_hip_get_pairlist(up.engine, node.encode(), sys, cap, i1.ctypes.data, i2.ctypes.data)
    assert 0 <= n <= cap
    return np.column_stack((i1[:n], i2[:n]))


class Evaluations(object):
    """oracle and product results of a case, computed once and shared by the tests (never modified)"""

    def __init__(self, directory):
        self.directory, self.done = str(directory), {}

    def __call__(self, name, which, chain, k):
        key = (name, which, 'A' if k == 1. else chain, float(k))      # (k = 1 is the shipped file on every chain)
        if key not in self.done:
            path = AC.write_case(self.directory, name, key[2], k)
            x = AC.positions(name, which)
            orc = P.pkg.Upside(path, library=P.oracle_library())
            ref = P.evaluate_all(orc, x)
            orc.close()
            assert all(np.isfinite(np.asarray(v)).all() for v in ref.values()), 'the oracle is not finite on %r' % (key,)
            up = P.pkg.Upside(path)
            act = P.evaluate_all(up, x)
            n_max = AC.longest_row(hip_pairlist(up, 'environment_coverage'))
            up.close()
            self.done[key] = dict(ref=ref, act=act, n_max=n_max, path=path)
        return self.done[key]


@pytest.fixture(scope='module')
def evaluated(hip, tmp_path_factory):
    return Evaluations(tmp_path_factory.mktemp('accumulator_cases'))


def compare_with_floor(ref, act, floor_key):
    """P.compare with the tolerance rule of P.golden_tol where the side-chain solve is ill-conditioned: max(1e-5, 2 x the reference's own
    build-to-build spread on exactly this case, tests/golden/reference_noise_floor.json) for the forces and for the sensitivities,
    1e-5 for everything else.  floor_key None: 1e-5 throughout."""
    if floor_key is None:
        return P.compare(ref, act, rtol=RTOL, verbose=True)
    tol_d, tol_s = P.golden_tol(floor_key, 'pos', 'deriv'), P.golden_tol(floor_key, 'pos', 'sens')
    print('%s: tolerance forces %.2e sensitivities %.2e' % (floor_key, tol_d, tol_s))
    sens = sorted(k for k in ref if k.startswith('sens/'))
    rest = sorted(k for k in ref if k != 'deriv' and not k.startswith('sens/'))
    return P.compare(ref, act, keys=['deriv'], rtol=tol_d, verbose=True) + P.compare(ref, act, keys=sens, rtol=tol_s, verbose=True) + \
        P.compare(ref, act, keys=rest, rtol=RTOL, verbose=True)


def floor_key_of(name, which, chain, k):
    """chain D reaches the side-chain solve (the coverage energies are its one-body terms), whose answer the reference itself reproduces
    only to 2e-5 .. 9e-5 between builds at these factors: those cases carry a measured floor.  Chains A, B and C do not: 1e-5."""
    return AC.chain_key(name, which, chain, k) if chain == 'D' and k > 1. else None


def case_id(v):
    return AC.klabel(v) if isinstance(v, float) else str(v)


@pytest.mark.parametrize('chain,k', AC.RANGE_CASES, ids=case_id)
@pytest.mark.parametrize('name,which', AC.STRUCTURES)
def test_range_matches_oracle(evaluated, name, which, chain, k):
    """every output, sensitivity, potential, the energy and the forces at force fields up to 2^16 times as steep: 1e-5 relative RMS
    and 10x that for the largest deviation, as at k = 1 (chain D: compare_with_floor)"""
    e = evaluated(name, which, chain, k)
    print('%s %s chain %s k = %s' % (name, which, chain, AC.klabel(k)))
    bad = compare_with_floor(e['ref'], e['act'], floor_key_of(name, which, chain, k))
    assert not bad, 'outside tolerance: %r' % (bad,)


@pytest.mark.parametrize('k', AC.K_RANGE, ids=case_id)
@pytest.mark.parametrize('name,which', AC.STRUCTURES)
def test_coupling_chain_is_linear(evaluated, name, which, k):
    """reference-free: the product's own sensitivities of the coupling chain at k, divided by k, are its own at k = 1 (2e-6, the bound
    the two accumulator forms hold between each other in test_alternate_code_paths_agree)"""
    one, big = evaluated(name, which, 'A', 1.)['act'], evaluated(name, which, 'A', k)['act']
    for key in AC.CHAIN_A_SENS:
        err = P.rel_rms(one[key], np.asarray(big[key], 'f8') / k)
        print('%-48s k = %-5s rel_rms %.3e' % (key, AC.klabel(k), err))
        assert err <= 2e-6, (key, AC.klabel(k), err)


@pytest.mark.parametrize('k', AC.K_SMALL, ids=case_id)
@pytest.mark.parametrize('chain', ['A', 'B', 'C'])
@pytest.mark.parametrize('name,which', AC.STRUCTURES)
def test_resolution_of_small_contributions(evaluated, name, which, chain, k):
    """force fields 2^-8 and 2^-16 times as steep: the forces (dominated by the unscaled terms) stay within 1e-5; the sensitivities of
    the coupling chain, now far below the float rounding of the unscaled ones, stay within the rounding of the conversion: half a count of
    2^-22 per contribution, at most n_max contributions per element (the longest row of the graph's pair list), plus the float error."""
    e = evaluated(name, which, chain, k)
    bad = P.compare(e['ref'], e['act'], keys=['deriv'], rtol=RTOL, verbose=True)
    assert not bad, bad
    if chain == 'B':
        return
    assert e['n_max'] > 0
    for key in AC.CHAIN_A_SENS:
        ref, act = np.asarray(e['ref'][key], 'f8'), np.asarray(e['act'][key], 'f8')
        bound = e['n_max'] * 2. ** -23 + RTOL * np.abs(ref).max()
        err = np.abs(act - ref).max()
        print('%-48s k = %-5s max abs err %.3e  bound %.3e  (n_max %d, max |ref| %.3e)' % (key, AC.klabel(k), err, bound, e['n_max'], np.abs(ref).max()))
        assert err <= bound, (key, err, bound)


FORMS = [
    {'UPSIDE_HIP_PAIR2': '0'},               # scalar (one partner per lane) forms of the side-chain gradient and coverage passes: 2^-32 counts
    {'UPSIDE_HIP_IG_UNSTAGED': '1'},         # coverage graphs through the kernels for systems too large for LDS
    {'UPSIDE_HIP_IG_POLY': '0'},             # coverage pair passes on the spline-coefficient table
    {'UPSIDE_HIP_IG_WGS': '4096'},           # several workgroups per system: their exact partial sums are merged in the global accumulators
]


@pytest.mark.parametrize('name,chain', [('trpcage20_7A', 'C'), ('proteinG56_7A', 'C'), ('proteinG56_7A', 'D')])
def test_every_form_of_the_passes(hip, tmp_path, name, chain):
    """the k = 2^12 cases in child processes under each switch that selects another form of the pair passes: each matches the oracle
    as the default form does, and the default form within 2e-6 (chain D, which the side-chain solve sees: within the measured floor)"""
    k = 2. ** 12
    path = AC.write_case(str(tmp_path), name, chain, k)
    tags = [w for n, w in AC.STRUCTURES if n == name]
    np.savez(str(tmp_path / 'structures.npz'), **dict((w, AC.positions(name, w)) for w in tags))
    orc = P.pkg.Upside(path, library=P.oracle_library())
    ref = dict((w, P.evaluate_all(orc, AC.positions(name, w))) for w in tags)
    orc.close()

    def run(env_extra, tag):
        out = str(tmp_path / (tag + '.npz'))
        env = dict(os.environ); env.update(env_extra)
        subprocess.run([sys.executable, os.path.join(HERE, 'accumulator_worker.py'), path, str(tmp_path / 'structures.npz'), out],
                       check=True, env=env, timeout=300, cwd=HERE)
        z = np.load(out)
        return dict((w, dict((key[len(w) + 1:], z[key]) for key in z.files if key.startswith(w + ':'))) for w in tags)

    base = run({}, 'default')
    for i, env_extra in enumerate([{}] + FORMS):
        alt = base if not env_extra else run(env_extra, 'form%d' % i)
        for w in tags:
            print('%s %s chain %s k = 2^12 %r' % (name, w, chain, env_extra))
            bad = compare_with_floor(ref[w], alt[w], floor_key_of(name, w, chain, k))
            assert not bad, (env_extra, w, bad)
            if floor_key_of(name, w, chain, k):     # (the forms round the coverage energies differently, and the solve amplifies that as it does between builds)
                bad = compare_with_floor(base[w], alt[w], floor_key_of(name, w, chain, k))
                assert not bad, (env_extra, w, 'against the default form', bad)
                continue
            for key in sorted(base[w]):
                if np.ndim(base[w][key]) == 0:
                    assert abs(float(base[w][key]) - float(alt[w][key])) <= 2e-6 * max(1., abs(float(base[w][key]))), (env_extra, w, key)
                else:
                    assert P.rel_rms(base[w][key], alt[w][key]) <= 2e-6, (env_extra, w, key, P.rel_rms(base[w][key], alt[w][key]))


def test_a_steep_neighbour_in_the_batch(hip, tmp_path):
    """three systems in one engine, the middle one 2^12 times as steep (chain B: the hydrogen-bond energy is the scaled value that
    may differ between the systems of an engine; the coupling's coefficients of chain A may not, from_files refuses such files).
    The middle system matches the oracle, and its neighbours are bit for bit what an engine of the shipped file alone computes."""
    name = 'proteinG56_7A'
    E = P.pkg.engine
    files = [AC.write_case(str(tmp_path), name, 'B', k) for k in (1., 2. ** 12)]
    x = AC.positions(name, 'initial_pos')
    ens = E.Ensemble.from_files([files[0], files[1], files[0]], library=hip)
    ens.set_pos(x)
    e, d = ens.energies_and_derivs()
    ens.close()
    orc = P.pkg.Upside(files[1], library=P.oracle_library())
    ref = P.evaluate_all(orc, x)
    orc.close()
    bad = P.compare(ref, dict(energy=e[1], deriv=d[1]), keys=['energy', 'deriv'], rtol=RTOL, verbose=True)
    assert not bad, bad
    one = E.Ensemble(files[0], 1, library=hip)
    one.set_pos(x)
    e1, d1 = one.energies_and_derivs()
    one.close()
    for s in (0, 2):
        assert e[s] == e1[0], (s, e[s], e1[0])
        assert np.array_equal(d[s], d1[0]), s


def test_contribution_beyond_the_wide_range_fails_loudly(hip, tmp_path):
    """a coverage table 2^28 times as steep puts single contributions past the 2^24 the wide path holds (the oracle's forces reach 1e9
    there and are finite): the call fails and names the pass; nothing is returned as if it were a gradient"""
    name = 'trpcage20_7A'
    path = AC.write_case(str(tmp_path), name, 'D', 2. ** 28)
    x = AC.positions(name, 'initial_pos')
    orc = P.pkg.Upside(path, library=P.oracle_library())
    ref = orc.deriv(x)
    orc.close()
    assert np.isfinite(ref).all() and np.abs(ref).max() > 2. ** 24
    up = P.pkg.Upside(path)
    with pytest.raises(RuntimeError):
        up.deriv(x)
    msg = hip.calc.upside_hip_last_error().decode()
    up.close()
    assert 'coverage' in msg and 'not valid' in msg, msg


@pytest.mark.parametrize('name,factor', AC.COMPRESSED)
def test_compressed_structures_match_oracle(hip, name, factor):
    """structures compressed to 0.8 and 0.7 of their size, at the shipped force field: the largest contributions the side-chain gradient
    pass sees through a configuration file.  Tolerance as P.golden_tol: max(1e-5, 2 x the reference's own build-to-build spread on
    exactly these coordinates, tests/golden/reference_noise_floor.json) for the forces and the sensitivities, 1e-5 for the rest."""
    x = AC.compressed_positions(name, factor)
    orc = P.pkg.Upside(P.fixture(name), library=P.oracle_library())
    ref = P.evaluate_all(orc, x)
    it = P.oracle_library().calc.oracle_rotamer_iterations(orc.engine)
    orc.close()
    assert 0 < it < AC.ROTAMER_ITERATION_CAP, it
    up = P.pkg.Upside(P.fixture(name))
    act = P.evaluate_all(up, x)
    up.close()
    print('%s: %d iterations' % (AC.noise_floor_key(name, factor), it))
    bad = compare_with_floor(ref, act, AC.noise_floor_key(name, factor))
    assert not bad, bad
