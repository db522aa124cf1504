"""Child process of tests/test_gpu_cv_metadynamics.py: one check of the cv_metadynamics node per invocation,

    python tests/cv_metad_gpu_worker.py CHECK WORKDIR

prints every figure it compares before it asserts and ends with 'CHECK <name> PASSED'.  The yardstick is
tests/cv_metad_reference.py (float64 numpy, pinned by tests/test_cv_metadynamics_config.py).  Where the bias must be seen alone, the
check runs on a copy of the fixture whose other potential groups are deleted: energy and derivative are then the node's own.
Everything runs on trpcage20 (60 atoms)."""
import os
import shutil
import subprocess
import sys
import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import parity_util as P                  # noqa: E402
import cv_restraint_cases as K           # noqa: E402
import cv_metad_reference as Y           # noqa: E402
import cv_metad_cases as M               # noqa: E402

pkg = P.pkg
cfg = pkg.config
E = pkg.engine
RTOL = P.RTOL
NODE = 'cv_metadynamics'
NAME = M.NAME
CLI_LIMIT = 240      # seconds for one upside_hip run; tests/test_gpu_cv_metadynamics.py gives the whole check 600
MD_SIGMA = (0.3, 0.05)      # rmsd over CA (Angstrom), Q: wider than the CVs move in two rounds, so consecutive hills overlap
HEIGHT = 0.3


def make(work, tag, specs, sigma, alone, height=HEIGHT, pace=2, capacity=5, kdT=0., shared=False):
    """a copy of the fixture with the node added; alone: nothing else under /input/potential"""
    p = os.path.join(work, '%s.up' % tag)
    shutil.copyfile(P.fixture(NAME), p)
    if alone:
        with pkg.h5lite.open_file(p, 'r+') as t:
            pot = t.group('input/potential')
            for k in pot.keys():
                pkg.h5lite.Node.delete(pot, k)
    cfg.add_cv_metadynamics(p, specs, sigma, height, pace, capacity, kdT=kdT, shared=shared, name=NODE)
    return p


def compare_deriv(ref, got, what):
    e1 = P.rel_rms(ref, got); e2 = P.max_rel_to_scale(ref, got)
    print('%-36s derivative: rel_rms %.3e (bound %.0e), largest element / scale %.3e (bound %.0e)' % (what, e1, RTOL, e2, 10 * RTOL))
    assert e1 <= RTOL and e2 <= 10 * RTOL, what


# ---- 1. energy and force against the yardstick --------------------------------------------------------------------------------------
def bias(work):
    x = K.perturbed(NAME)
    for d in (1, 2, 3, 4):
        specs = M.specs_of(d)
        stored = M.rounded_to_file(specs)
        v_ref = Y.values(stored, x)
        sigma = M.sigma_of(v_ref)
        ens = E.Ensemble(make(work, 'bias%d' % d, specs, sigma, True, capacity=1000), 1)
        assert ens.metad_info(NODE) == (d, 1000, 1)
        ens.define_cvs(specs)
        ens.set_pos(x.astype('f4'))
        assert ens.get_pos()[0].astype('f8').tobytes() == x.tobytes()
        for n in (0, 1, 255, 256, 257, 1000):
            centers, weights = M.random_hills(v_ref, sigma, n, 1000 * d + n)
            ens.set_metad_hills(NODE, centers, weights)
            e, g = ens.energies_and_derivs()
            e = e.astype('f8')
            e_ref, g_ref, _ = Y.energy_and_gradient(stored, x, centers, weights, sigma)
            if n == 0:
                print('d = %d, no hills: energy %r, largest |derivative| %r' % (d, float(e[0]), float(np.abs(g).max())))
                assert e[0] == 0. and not g.any()
                continue
            print('d = %d, %4d hills: energy gpu %.9g, f64 %.9g, relative difference %.3e (bound 1e-6)' % (d, n, e[0], e_ref, abs(e[0] - e_ref) / abs(e_ref)))
            assert abs(e[0] - e_ref) <= 1e-6 * abs(e_ref)
            compare_deriv(g_ref, g[0], 'd = %d, %4d hills' % (d, n))
        v = ens.metad_values(NODE)
        print('d = %d: largest relative difference of a CV value %.3e; the bits of cvs(): %s' % (d, np.abs(v[0] - v_ref).max() / np.abs(v_ref).max(), v.tobytes() == ens.cvs().tobytes()))
        assert v.shape == (1, d) and np.abs(v[0] - v_ref).max() <= RTOL * np.abs(v_ref).max() and v.tobytes() == ens.cvs().tobytes()
        ens.close()
    coincident(work)


def coincident(work):
    """two coincident atoms in a distance CV: finite output, zero force from that CV (alone: every component exactly 0; beside an
    rg: the force is the rg's)"""
    x = K.perturbed(NAME)
    x[4] = x[3]
    dist = {'name': 'd', 'kind': 'distance', 'pair': (3, 4)}
    rg = {'name': 'rg', 'kind': 'rg', 'atoms': np.arange(60, dtype='i4')}
    for tag, specs in (('co1', [dist]), ('co2', [dist, rg])):
        v = Y.values(specs, x)
        sigma = M.sigma_of(v)
        centers, weights = M.random_hills(v, sigma, 40, 5)
        ens = E.Ensemble(make(work, tag, specs, sigma, True, capacity=40), 1)
        ens.set_pos(x.astype('f4'))
        ens.set_metad_hills(NODE, centers, weights)
        e, g = ens.energies_and_derivs()
        e = e.astype('f8')
        e_ref, g_ref, v_ref = Y.energy_and_gradient(specs, x, centers, weights, sigma)
        print('coincident atoms, d = %d: values %s, energy gpu %.9g, f64 %.9g, largest |derivative| %r' % (len(specs), ens.metad_values(NODE)[0], e[0], e_ref, float(np.abs(g).max())))
        assert v_ref[0] == 0. and np.isfinite(e).all() and np.isfinite(g).all() and e_ref > 0. and abs(e[0] - e_ref) <= 1e-6 * e_ref
        if len(specs) == 1:
            assert not g.any()
        else:
            compare_deriv(g_ref, g[0], 'coincident atoms beside an rg')
        ens.close()


# ---- 2. deposition ------------------------------------------------------------------------------------------------------------------
def md_engine(work, tag, kdT=0., n_system=1, shared=False, pace=2, capacity=5):
    specs = M.specs_of(2)
    ens = E.Ensemble(make(work, tag, specs, MD_SIGMA, False, pace=pace, capacity=capacity, kdT=kdT, shared=shared), n_system)
    ens.set_pos(K.coords(NAME).astype('f4'))
    ens.init_md(0.8, 21)
    ens.define_cvs(specs)
    return ens


def deposit(work):
    h32 = np.float32(HEIGHT)
    sigma = np.asarray(MD_SIGMA, 'f4').astype('f8')
    for kdT in (0., 2.0):
        ens = md_engine(work, 'dep%g' % kdT, kdT)
        assert ens.metad_hills(NODE)[0].shape == (0, 2)
        prev_c = np.zeros((0, 2), 'f4'); prev_w = np.zeros(0, 'f4')
        for i in range(7):
            ens.run_rounds(2)
            cv = ens.cvs()[0]
            ens.energies()      # (a force pass outside MD deposits nothing)
            c, w, na = ens.metad_hills(NODE)
            print('kdT %g, call %d: cvs %s; %d hills, %d attempts; newest hill %s weight %r' % (kdT, i, cv, len(w), na, c[-1], float(w[-1])))
            assert len(w) == min(i + 1, 5) and na == i + 1
            assert c[:len(prev_w)].tobytes() == prev_c.tobytes() and w[:len(prev_w)].tobytes() == prev_w.tobytes(), 'an earlier hill changed'
            if i < 5:
                assert c[i].tobytes() == cv.tobytes(), 'the newest centre is not the bits of cvs()'
                if kdT == 0. or i == 0:
                    assert w[i] == h32
                else:
                    v_at = Y.bias(c[i].astype('f8'), c[:i], w[:i], sigma)[0]
                    want = float(h32) * np.exp(-v_at / kdT)
                    print('    V of the %d earlier hills at this centre %.9g: weight %.9g, f64 %.9g, relative difference %.3e (bound 1e-6)' % (i, v_at, w[i], want, abs(w[i] - want) / want))
                    assert abs(float(w[i]) - want) <= 1e-6 * want and w[i] < h32
            prev_c, prev_w = c, w
        assert len(prev_w) == 5 and na == 7
        ens.close()


# ---- 3. captured graph against plain launches ---------------------------------------------------------------------------------------
def graph_run(work, tag, with_node):
    if with_node:
        ens = md_engine(work, tag)
    else:
        ens = E.Ensemble(P.fixture(NAME), 1)
        ens.set_pos(K.coords(NAME).astype('f4'))
        ens.init_md(0.8, 21)
    ens.run_rounds(12)
    out = [ens.get_pos(), ens.get_mom()]
    if with_node:
        c, w, na = ens.metad_hills(NODE)
        assert len(w) == 5 and na == 6
        out += [c, w]
    ens.close()
    return out


def graph(work):
    """run under UPSIDE_HIP_GRAPH=1 and =0 by the parent, which compares the two files this leaves"""
    g = os.environ.get('UPSIDE_HIP_GRAPH', 'x')
    print('UPSIDE_HIP_GRAPH=%s' % g)
    a = graph_run(work, 'graph' + g, True); b = graph_run(work, 'graph' + g, True)
    assert all(np.isfinite(x).all() for x in a)
    same = all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    print('two runs of 12 rounds: positions, momenta and the 5 hills bit-identical: %s' % same)
    assert same
    f = graph_run(work, 'free' + g, False)
    np.savez(os.path.join(work, 'graph%s.npz' % g), pos=a[0], mom=a[1], centers=a[2], weights=a[3], free_pos=f[0], free_mom=f[1])


# ---- 4. determinism and batch independence ------------------------------------------------------------------------------------------
def batch(work):
    x0 = K.perturbed(NAME)
    specs = M.specs_of(2)
    v0 = Y.values(M.rounded_to_file(specs), x0)
    sigma = M.sigma_of(v0)
    path = make(work, 'batch', specs, sigma, True, capacity=300)
    c0, w0 = M.random_hills(v0, sigma, 300, 9)
    one = E.Ensemble(path, 1)
    one.set_pos(x0.astype('f4')); one.set_metad_hills(NODE, c0, w0)
    e1, d1 = one.energies_and_derivs()
    one.close()
    assert e1[0] > 0. and d1.any()
    rng = np.random.default_rng(3)
    for n_sys in (64, 600):
        x = (x0[None] + 0.3 * rng.standard_normal((n_sys,) + x0.shape)).astype('f4')
        same = (0, 7, n_sys - 1)
        runs = []
        for rep in range(2):
            ens = E.Ensemble(path, n_sys)
            assert ens.metad_info(NODE) == (2, 300, n_sys)
            for s in range(n_sys):
                if s in same:
                    x[s] = x0; ens.set_metad_hills(NODE, c0, w0, system=s)
                else:
                    ens.set_metad_hills(NODE, *M.random_hills(v0, sigma, 1 + s % 13, s), system=s)
            ens.set_pos(x)
            runs.append(ens.energies_and_derivs())
            if rep == 0:      # hills stay with the system index when coordinates are exchanged
                before = [ens.metad_hills(NODE, s) for s in (0, 1)]
                ens.swap_systems(0, 1)
                after = [ens.metad_hills(NODE, s) for s in (0, 1)]
                assert all(a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[2] == b[2] for a, b in zip(before, after))
                assert ens.get_pos()[1].tobytes() == x[0].tobytes()
            ens.close()
        assert runs[0][0].tobytes() == runs[1][0].tobytes() and runs[0][1].tobytes() == runs[1][1].tobytes(), 'two runs of %d systems differ' % n_sys
        e, d = runs[0]
        distinct = len(set(e.tolist()))
        print('%d systems: two runs bit-identical; %d distinct energies; systems 0, 7 and %d against a one-system engine: energies %s / %r' % (n_sys, distinct, n_sys - 1, e[list(same)], float(e1[0])))
        assert distinct >= n_sys - 4
        for s in same:
            assert e[s] == e1[0] and d[s].tobytes() == d1[0].tobytes(), 'system %d of %d differs from the one-system engine' % (s, n_sys)


# ---- 5. walkers on one list -----------------------------------------------------------------------------------------------------------
def walkers(work):
    S = 4
    ens = md_engine(work, 'walk', n_system=S, shared=True, pace=1, capacity=10)
    assert ens.metad_info(NODE) == (2, 10, 1)
    per_round = []
    for r in range(3):
        ens.run_rounds(1)
        per_round.append(ens.cvs())
    c, w, na = ens.metad_hills(NODE)
    print('3 rounds of 4 walkers on a list of 10 slots: %d hills visible, %d deposits attempted' % (len(w), na))
    assert len(w) == 8 and na == 3
    for s in range(S):
        cs, ws, nas = ens.metad_hills(NODE, system=s)
        assert cs.tobytes() == c.tobytes() and ws.tobytes() == w.tobytes() and nas == 3
    for k in range(2):
        for s in range(S):
            print('  slot %d: %s; cvs() of system %d after round %d: %s' % (k * S + s, c[k * S + s], s, k + 1, per_round[k][s]))
            assert c[k * S + s].tobytes() == per_round[k][s].tobytes() and w[k * S + s] == np.float32(HEIGHT)
    assert len(set(c[:, 0].tolist())) == 8      # (the walkers are at different places)
    pos = ens.get_pos()
    ens.close()
    # the bias alone: a shared list read by 4 systems against an unshared one-system engine holding the same 8 hills
    specs = M.specs_of(2)
    sh = E.Ensemble(make(work, 'walk_sh', specs, MD_SIGMA, True, pace=1, capacity=10, shared=True), S)
    sh.set_pos(pos); sh.set_metad_hills(NODE, c, w)
    e, d = sh.energies_and_derivs()
    sh.close()
    own = E.Ensemble(make(work, 'walk_own', specs, MD_SIGMA, True, pace=1, capacity=10), 1)
    own.set_metad_hills(NODE, c, w)
    for s in range(S):
        own.set_pos(pos[s])
        e1, d1 = own.energies_and_derivs()
        print('  system %d: bias %r on the shared list, %r in a one-system engine of its own' % (s, float(e[s]), float(e1[0])))
        assert e[s] == e1[0] and e[s] > 0. and d[s].tobytes() == d1[0].tobytes()
    own.close()


# ---- 6. reading and writing hills -----------------------------------------------------------------------------------------------------
def readback(work):
    print('UPSIDE_HIP_GRAPH=%s' % os.environ.get('UPSIDE_HIP_GRAPH'))
    ens = md_engine(work, 'rb', pace=1, capacity=8)
    v = ens.cvs()[0]
    c3, w3 = M.random_hills(v, MD_SIGMA, 3, 4)
    ens.set_metad_hills(NODE, c3, w3)
    c, w, na = ens.metad_hills(NODE)
    assert c.tobytes() == c3.tobytes() and w.tobytes() == w3.tobytes() and na == 3
    got = []
    for r in range(2):
        ens.run_rounds(1)
        got.append(ens.cvs()[0])
    c, w, na = ens.metad_hills(NODE)
    print('3 hills written, 2 rounds at pace 1: %d hills, %d attempts; slots 3 and 4: %s %s' % (len(w), na, c[3], c[4]))
    assert len(w) == 5 and na == 5 and c[:3].tobytes() == c3.tobytes() and w[:3].tobytes() == w3.tobytes()
    assert c[3].tobytes() == got[0].tobytes() and c[4].tobytes() == got[1].tobytes() and np.all(w[3:] == np.float32(HEIGHT))
    ens.run_rounds(10)      # (long enough for the rounds to be captured and replayed where graphs are on)
    e_before = ens.energies()
    c2, w2 = M.random_hills(ens.cvs()[0], MD_SIGMA, 6, 8)
    ens.set_metad_hills(NODE, c2, w2)
    e = ens.energies()
    fresh = md_engine(work, 'rb_fresh', pace=1, capacity=8)
    fresh.set_pos(ens.get_pos()); fresh.set_metad_hills(NODE, c2, w2)
    ef = fresh.energies()
    print('after 12 rounds, 6 new hills written: energy %r (before %r); a fresh engine with those hills at the same positions %r' % (float(e[0]), float(e_before[0]), float(ef[0])))
    assert np.array_equal(e, ef) and e[0] != e_before[0]
    ens.run_rounds(2)      # the replayed rounds go on from the written hills
    c, w, na = ens.metad_hills(NODE)
    assert len(w) == 8 and na == 8 and c[:6].tobytes() == c2.tobytes()
    ens.close(); fresh.close()


# ---- 7. upside_hip ----------------------------------------------------------------------------------------------------------------------
def run_cli(args):
    exe = os.path.join(P.ROOT, 'upside-md_amd', 'csrc', 'upside_hip')
    try:      # a limit well inside the parent's: the run is over (killed by subprocess.run) before the parent gives up on this process
        r = subprocess.run([exe] + args, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=CLI_LIMIT)
    except subprocess.TimeoutExpired as err:
        print((err.stdout or b'').decode()[-3000:])
        print('upside_hip did not finish in %d s' % CLI_LIMIT)
        sys.exit(124)      # a hang: the parent starts nothing more
    if r.returncode:
        print(r.stdout.decode()[-3000:])
        if r.returncode < 0 or r.returncode > 1:
            sys.exit(r.returncode if r.returncode > 0 else 128 - r.returncode)      # a signal: the parent starts nothing more
        raise AssertionError('upside_hip failed')


def read_output(path):
    with pkg.h5lite.open_file(path) as t:
        out = t.group('output')
        m = out.group('metadynamics/' + NODE)
        return out.read('potential'), out.read('pos', 'f4'), m.read('hill_center', 'f4'), m.read('hill_weight', 'f4'), m.read('n_attempt')


def cli(work):
    specs = M.specs_of(2)
    args = ['--duration', '0.162', '--frame-interval', '0.054', '--seed', '3', '--temperature', '0.8']      # 6 rounds of 3 x 0.009
    first = make(work, 'cli1', specs, MD_SIGMA, False, pace=2, capacity=10)
    run_cli(args + [first])
    pot, pos, c, w, na = read_output(first)
    print('first run: %d frames, %d hills, n_attempt %s, centres %s' % (len(pot), len(w), na.ravel().tolist(), c.tolist()))
    assert c.shape == (3, 2) and w.shape == (3,) and int(na.ravel()[0]) == 3 and np.all(w == np.float32(HEIGHT)) and float(pot.ravel()[0]) != 0.
    second = make(work, 'cli2', specs, MD_SIGMA, False, pace=2, capacity=10)
    cfg.set_metadynamics_hills(second, NODE, c, w)
    run_cli(args + [second])
    pot2, pos2, c2, w2, na2 = read_output(second)
    ens = E.Ensemble(second, 1)
    ens.set_pos(pos2[0, 0]); ens.set_metad_hills(NODE, c, w)
    want = float(ens.energies()[0])
    ens.set_metad_hills(NODE, c[:0], w[:0])
    without = float(ens.energies()[0])
    ens.close()
    print('second run: frame-0 potential %.9g; Ensemble + set_metad_hills at the initial structure %.9g (without the hills %.9g); %d hills at the end, n_attempt %s'
          % (pot2.ravel()[0], want, without, len(w2), na2.ravel().tolist()))
    assert abs(float(pot2.ravel()[0]) - want) <= 1e-6 * max(1., abs(want)) and abs(want - without) > 1e-4 * max(1., abs(want))
    assert c2.shape == (6, 2) and int(na2.ravel()[0]) == 6 and c2[:3].tobytes() == c.tobytes() and w2[:3].tobytes() == w.tobytes()


# ---- 8. refusals ------------------------------------------------------------------------------------------------------------------------
def refusals(work):
    import hamiltonian_files as H
    specs = M.specs_of(2)
    x = K.perturbed(NAME).astype('f4')
    good_path = make(work, 'good', specs, MD_SIGMA, True, capacity=6)
    hc, hw = M.random_hills(Y.values(specs, x.astype('f8')), MD_SIGMA, 6, 2)

    def good_energy():
        ens = E.Ensemble(good_path, 2)
        ens.set_pos(x)
        for s in range(2):
            ens.set_metad_hills(NODE, hc, hw, system=s)
        e = ens.energies()
        ens.close()
        return e
    e0 = good_energy()
    assert np.isfinite(e0).all() and e0[0] > 0.

    def tampered(tag, dataset=None, fn=None, attr=None, value=None, five=False):
        p = os.path.join(work, 'bad_%s.up' % tag)
        shutil.copyfile(good_path, p)
        if five:      # a node of 5 CVs, written past the checks of config.add_cv_metadynamics
            packed = cfg.pack_collective_variables(M.specs_of(4) + M.specs_of(1), 60)
            with pkg.h5lite.open_file(p, 'r+') as t:
                g = t.group('input/potential/' + NODE)
                for k in ('kind', 'atom_start', 'atoms', 'ref_pos', 'contact_r0', 'contact_beta', 'contact_lambda', 'names', 'sigma'):
                    g.delete(k)
                    g.write(k, packed[k] if k != 'sigma' else np.ones(5, 'f4'))
        if dataset:
            H.rewrite(p, NODE, dataset, fn)
        if attr:
            with pkg.h5lite.open_file(p, 'r+') as t:
                t.group('input/potential/' + NODE).set_attr(attr, value)
        return p

    cases = [
        ('sigma = 0', dict(dataset='sigma', fn=lambda v: v * np.array([1., 0.], 'f4')), ['sigma of CV 1 must be finite and positive']),
        ('sigma < 0', dict(dataset='sigma', fn=lambda v: -v), ['sigma of CV 0 must be finite and positive']),
        ('sigma not finite', dict(dataset='sigma', fn=lambda v: v * np.array([1., np.inf], 'f4')), ['sigma of CV 1 must be finite and positive']),
        ('short sigma', dict(dataset='sigma', fn=lambda v: v[:1].copy()), ['sigma holds 1 entries', '2 CVs']),
        ('d = 5', dict(five=True), ['5 CVs', 'limit of 4']),
        ('pace = 0', dict(attr='pace', value=0), ['pace must be at least 1']),
        ('capacity = 0', dict(attr='capacity', value=0), ['capacity must be between 1 and']),
        ('kdT < 0', dict(attr='kdT', value=-1.), ['kdT must be finite and not negative']),
        ('height = 0', dict(attr='height', value=0.), ['height must be finite and positive']),
        ('shared = 2', dict(attr='shared', value=2), ['shared must be 0 or 1']),
    ]
    for i, (what, how, needles) in enumerate(cases):
        path = tampered(str(i), **how)
        try:
            E.Ensemble(path, 2)
        except RuntimeError as err:
            print('%-28s refused: %s' % (what, err))
            for nd in needles:
                assert nd in str(err), (what, nd, str(err))
            assert NODE in str(err)
        else:
            raise AssertionError('%s: the node was constructed' % what)
        os.remove(path)
        assert np.array_equal(good_energy(), e0), what + ': the process no longer constructs a good engine'

    # hills refused by a live engine, which stays as it was
    own = E.Ensemble(good_path, 2); own.set_pos(x)
    shared_path = make(work, 'good_shared', specs, MD_SIGMA, True, capacity=6, shared=True)
    sh = E.Ensemble(shared_path, 4); sh.set_pos(x)
    for s in range(2):
        own.set_metad_hills(NODE, hc, hw, system=s)
    sh.set_metad_hills(NODE, hc[:4], hw[:4])
    e_sh = sh.energies()
    c7, w7 = M.random_hills(np.zeros(2), MD_SIGMA, 7, 1)
    bad_c = hc.copy(); bad_c[2, 1] = np.nan
    bad_w = hw.copy(); bad_w[5] = np.inf
    for what, ens, c, w, needle in (('n_hill > capacity', own, c7, w7, '7 hills exceed the capacity of 6'),
                                    ('a centre that is not finite', own, bad_c, hw, 'centre of hill 2 is not finite'),
                                    ('a weight that is not finite', own, hc, bad_w, 'weight of hill 5 is not finite'),
                                    ('shared, 6 hills for 4 systems', sh, hc, hw, '6 hills are no multiple of 4 systems')):
        try:
            ens.set_metad_hills(NODE, c, w, system=1)
        except RuntimeError as err:
            print('%-28s refused: %s' % (what, err))
            assert needle in str(err) and NODE in str(err), (what, str(err))
        else:
            raise AssertionError('%s: the hills were accepted' % what)
        assert np.array_equal(own.energies(), e0) and np.array_equal(sh.energies(), e_sh), what
    for bad in ('cv_restraint', 'cv_metadynamics_x'):
        try:
            own.metad_hills(bad)
        except RuntimeError as err:
            print('%-28s refused: %s' % ('node ' + bad, err))
        else:
            raise AssertionError('hills of a node that does not exist')
    own.close(); sh.close()

    # the files of one engine must agree on the node
    other = os.path.join(work, 'other_sigma.up')
    shutil.copyfile(good_path, other)
    H.rewrite(other, NODE, 'sigma', lambda v: (2. * v).astype('f4'))
    try:
        E.Ensemble.from_files([good_path, other])
    except RuntimeError as err:
        print('files differing in sigma refused: %s' % err)
        assert 'other_sigma.up' in str(err) and NODE in str(err) and 'sigma' in str(err)
    else:
        raise AssertionError('files differing in sigma were accepted')
    assert np.array_equal(good_energy(), e0)


CHECKS = dict(bias=bias, deposit=deposit, graph=graph, batch=batch, walkers=walkers, readback=readback, cli=cli, refusals=refusals)

if __name__ == '__main__':
    import torch
    assert torch.cuda.is_available(), 'these checks need a GPU'
    which, workdir = sys.argv[1], sys.argv[2]
    CHECKS[which](workdir)
    print('CHECK %s PASSED' % which)
