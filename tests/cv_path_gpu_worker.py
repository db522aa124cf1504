"""Child process of tests/test_gpu_cv_path.py: one check of the path collective variables (kinds path_s and path_z,
csrc/cv_path_device.h) per invocation,

    python tests/cv_path_gpu_worker.py CHECK WORKDIR

prints every figure it compares before it asserts and ends with 'CHECK <name> PASSED'.  The yardstick is tests/cv_path_reference.py
(float64 numpy, pinned by tests/test_cv_path_config.py, which also asserts that the inputs of tests/cv_path_cases.py keep it well
conditioned).  Fixtures: trpcage20_7A (60 atoms) and, for lane boundaries, proteinG56_7A (168 atoms).
Bounds: path_s within parity_util.RTOL x max(|s|, 1); path_z within RTOL x max(|z|, Rg^2 of the selection); a bias energy within 1e-6
relative; a derivative within RTOL as relative RMS and 10 x RTOL of its scale in the largest element; the accumulated work within
1e-12 x sum_n (|E(v_n, c(n))| + |E(v_n, c(n-1))|) of the yardstick's restatement from the recorded series (the bound of
tests/cv_steer_gpu_worker.py); equalities between engine runs are bitwise."""
import os
import shutil
import subprocess
import sys
import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import parity_util as P                  # noqa: E402
import cv_restraint_cases as K           # noqa: E402
import cv_path_reference as R            # noqa: E402
import cv_path_cases as C                # noqa: E402

pkg = P.pkg
cfg = pkg.config
E = pkg.engine
RTOL = P.RTOL
TRP = C.TRP
RESTRAINT = 'cv_restraint'
STEER = 'cv_steer'
METAD = 'cv_metadynamics'
STEER_VALUES = ('center', 'rate', 'center_end', 'spring_const', 'flat_width')
CLI_LIMIT = 240      # seconds for one upside_hip run


def r32(v):
    return float(np.float32(v))


def bare(specs):
    return [dict((k, v) for k, v in sp.items() if k not in STEER_VALUES) for sp in specs]


def stored(specs):
    """the bias values rounded to the float32 the file holds (frames and lambda are float32 values already: cv_path_cases)"""
    return [dict(sp, **dict((k, r32(sp[k])) for k in STEER_VALUES if k in sp)) for sp in specs]


def strip_potential(path):
    with pkg.h5lite.open_file(path, 'r+') as t:
        pot = t.group('input/potential')
        for k in pot.keys():
            pkg.h5lite.Node.delete(pot, k)


def node_file(work, tag, add, alone, name=TRP):
    p = os.path.join(work, '%s.up' % tag)
    shutil.copyfile(P.fixture(name), p)
    if alone:
        strip_potential(p)
    add(p)
    return p


def compare_deriv(ref, got, what):
    e1 = P.rel_rms(ref, got); e2 = P.max_rel_to_scale(ref, got)
    print('%-50s derivative: rel_rms %.3e (bound %.0e), largest element / scale %.3e (bound %.0e)' % (what, e1, RTOL, e2, 10 * RTOL))
    assert np.isfinite(got).all() and e1 <= RTOL and e2 <= 10 * RTOL, what


def compare_energy(ref, got, what):
    rel = abs(float(got) - ref) / abs(ref)
    print('%-50s energy gpu %.9g, f64 %.9g, relative difference %.3e (bound 1e-6)' % (what, got, ref, rel))
    assert ref > 0. and rel <= 1e-6, what


def value_ratios(gpu, x32, specs):
    """(|s gpu - f64| / bound, |z gpu - f64| / bound, the yardstick's (s, z)) over the systems: specs is [path_s, path_z] of one path"""
    atoms = np.asarray(specs[0]['atoms'])
    ref = []; bound = []
    for x in np.asarray(x32, 'f4').astype('f8'):
        r = R.path(specs[0], x)
        ref.append((r['s'], r['z']))
        bound.append((RTOL * max(abs(r['s']), 1.), RTOL * max(abs(r['z']), C.rg2(x, atoms))))
    ref = np.array(ref); bound = np.array(bound)
    assert np.isfinite(gpu).all()
    return np.abs(np.asarray(gpu, 'f8') - ref) / bound, ref


# ---- 1. values -------------------------------------------------------------------------------------------------------------------------
def values(work):
    worst = 0.
    engines = {}
    for name in (C.TRP, C.GB1):
        engines[name] = E.Ensemble(P.fixture(name), C.N_SYS)
        engines[name].set_pos(C.systems(name))
    print('%d systems per fixture: smooth noise growing from 0 to 3 A; columns: largest |gpu - f64| / bound of s and of z over the systems' % C.N_SYS)
    for name, n, n_frame, factor in C.value_cases():
        specs = C.specs(name, n, n_frame, factor)
        ens = engines[name]
        ens.define_cvs(specs)
        assert ens.cv_periods.tolist() == [0., 0.] and ens.cv_names == ['path_s', 'path_z']
        got = ens.cvs()
        ratio, ref = value_ratios(got, C.systems(name), specs)
        i = int(np.argmax(ratio.max(1)))
        print('%-13s n %3d K %2d lambda %10.4g: s %.3e, z %.3e   (system %2d: s gpu %.9g f64 %.9g, z gpu %.9g f64 %.9g)' %
              (name, n, n_frame, specs[0]['lambda'], ratio[:, 0].max(), ratio[:, 1].max(), i, got[i, 0], ref[i, 0], got[i, 1], ref[i, 1]))
        assert (got[:, 0] >= 1.) .all() and (got[:, 0] <= n_frame).all()
        assert ratio.max() <= 1., (name, n, n_frame, factor, ratio.max())
        worst = max(worst, ratio.max())
    print('largest ratio over all cases: %.3e' % worst)
    for ens in engines.values():
        ens.close()


# ---- 2. batch independence -------------------------------------------------------------------------------------------------------------
def batch(work):
    n_sys = 64
    same = (0, 7, n_sys - 1)
    x = C.systems(TRP, n_sys, seed=3)
    for s in same:
        x[s] = x[20]
    specs = C.specs(TRP, 60, 5) + [dict(sp, name=sp['name'] + '_ca') for sp in C.specs(TRP, 20, 64)]
    rest = [dict(sp, center=2.5 if sp['kind'] == 'path_s' else 0.3, spring_const=4.) for sp in specs]
    path = node_file(work, 'batch', lambda p: cfg.add_cv_restraint(p, rest), True)
    runs = []
    for rep in range(2):
        ens = E.Ensemble(path, n_sys)
        ens.define_cvs(specs)
        ens.set_pos(x)
        v = ens.cvs()
        e, d = ens.energies_and_derivs()
        runs.append((v, e, d))
        ens.close()
    (v, e, d), (v2, e2, d2) = runs
    print('two runs of 64 systems: values, energies and forces bit-identical: %s' % (v.tobytes() == v2.tobytes() and e.tobytes() == e2.tobytes() and d.tobytes() == d2.tobytes()))
    assert v.tobytes() == v2.tobytes() and e.tobytes() == e2.tobytes() and d.tobytes() == d2.tobytes()
    for s in same[1:]:
        ok = v[s].tobytes() == v[0].tobytes() and e[s].tobytes() == e[0].tobytes() and d[s].tobytes() == d[0].tobytes()
        print('system %2d against system 0 at the same positions: values, energy and forces bit-identical: %s' % (s, ok))
        assert ok
    assert np.isfinite(d).all() and np.abs(d[0]).max() > 0 and v[1].tobytes() != v[0].tobytes()
    # a smaller batch holds the same rows
    ens = E.Ensemble(path, 3)
    ens.define_cvs(specs); ens.set_pos(x[[20, 1, 2]])
    v3 = ens.cvs(); e3, d3 = ens.energies_and_derivs()
    ens.close()
    assert v3[0].tobytes() == v[0].tobytes() and v3[1].tobytes() == v[1].tobytes() and d3[0].tobytes() == d[0].tobytes() and d3[2].tobytes() == d[2].tobytes()
    print('the rows of a batch of 3 are the bits of the batch of 64')


# ---- 3. restraint ----------------------------------------------------------------------------------------------------------------------
def restraint_specs(name, n, n_frame, x, factor=1.):
    s_spec, z_spec = C.specs(name, n, n_frame, factor)
    n_atom = len(x)
    rg = {'name': 'rg', 'kind': 'rg', 'atoms': np.arange(n_atom, dtype='i4')}
    v = R.evaluate([s_spec, z_spec, rg], x)
    return [dict(s_spec, center=r32(v[0] + 0.7), spring_const=6., flat_width=0.),
            dict(z_spec, center=r32(0.5 * v[1]), spring_const=3., flat_width=r32(0.05 * v[1])),
            dict(rg, center=r32(v[2] - 0.8), spring_const=2., flat_width=0.)]


def restraint(work):
    for name, n, n_frame, system in ((TRP, 60, 5, 9), (TRP, 20, 64, 15), (C.GB1, 129, 63, 6), (C.GB1, 65, 3, 12)):
        x32 = C.systems(name)[system]
        x = x32.astype('f8')
        specs = restraint_specs(name, n, n_frame, x)
        for tag, sub in (('s, z and rg', specs), ('s alone', specs[:1]), ('z alone', specs[1:2]), ('rg alone', specs[2:])):
            what = '%s n %d K %d: %s' % (name, n, n_frame, tag)
            ens = E.Ensemble(node_file(work, 'restraint', lambda p: cfg.add_cv_restraint(p, sub), True, name), 2)
            ens.define_cvs(bare(sub))
            ens.set_pos(np.array([x32, C.systems(name)[3]]))
            e, d = ens.energies_and_derivs()
            e_ref, g_ref, v_ref = R.restraint_energy_and_gradient(stored(sub), x)
            compare_energy(e_ref, e.astype('f8')[0], what)
            compare_deriv(g_ref, d[0], what)
            vals = ens.restraint_values(RESTRAINT)
            assert vals.tobytes() == ens.cvs().tobytes(), 'restraint_values are not the bits of cvs()'
            ens.close()
        print('%s n %d K %d: restraint_values equal cvs() bitwise' % (name, n, n_frame))
    # a dominating frame (100 x lambda): most coefficients underflow to exactly 0 and their frames are skipped
    x32 = C.systems(TRP)[11]
    specs = restraint_specs(TRP, 60, 64, x32.astype('f8'), 100.)[:2]
    ens = E.Ensemble(node_file(work, 'restraint_sharp', lambda p: cfg.add_cv_restraint(p, specs), True), 1)
    ens.set_pos(x32)
    e, d = ens.energies_and_derivs()
    e_ref, g_ref, _ = R.restraint_energy_and_gradient(stored(specs), x32.astype('f8'))
    p = R.path(specs[0], x32.astype('f8'))['p']
    print('100 x lambda, K = 64: %d of 64 weights are exactly 0, the largest is %.6f' % (int((p == 0.).sum()), p.max()))
    assert (p == 0.).sum() >= 32
    compare_energy(e_ref, e.astype('f8')[0], 'a dominating frame')
    compare_deriv(g_ref, d[0], 'a dominating frame')
    ens.close()
    # a structure sitting exactly on a frame (moved rigidly): d_k = 0 there, finite energy and finite forces
    atoms, fr = C.md_frames()
    on = K.coords(TRP).copy()
    c, s = np.cos(0.7), np.sin(0.7)
    on[atoms] = fr[4] @ np.array([[c, -s, 0.], [s, c, 0.], [0., 0., 1.]]).T + np.array([3., 1., -2.])
    on32 = on.astype('f4')
    lam = r32(cfg.path_lambda(fr))
    specs = cfg.path_specs('p', atoms, fr, lam)
    specs = [dict(specs[0], center=3.5, spring_const=6.), dict(specs[1], center=1., spring_const=3.)]
    ens = E.Ensemble(node_file(work, 'restraint_on', lambda p: cfg.add_cv_restraint(p, specs), True), 1)
    ens.set_pos(on32)
    e, d = ens.energies_and_derivs()
    v = ens.restraint_values(RESTRAINT)[0]
    e_ref, g_ref, v_ref = R.restraint_energy_and_gradient(stored(specs), on32.astype('f8'))
    print('on frame 5: s gpu %.9g f64 %.9g, z gpu %.9g f64 %.9g; energy gpu %.9g f64 %.9g; largest |force| %.6g' % (v[0], v_ref[0], v[1], v_ref[1], e[0], e_ref, np.abs(d).max()))
    assert np.isfinite(e).all() and np.isfinite(d).all() and np.isfinite(v).all()
    assert abs(v[0] - v_ref[0]) <= RTOL * max(abs(v_ref[0]), 1.) and abs(v[1] - v_ref[1]) <= RTOL * max(abs(v_ref[1]), C.rg2(on32, atoms))
    compare_energy(e_ref, e.astype('f8')[0], 'on a frame')
    compare_deriv(g_ref, d[0], 'on a frame')
    ens.close()


# ---- 4. steering along s ---------------------------------------------------------------------------------------------------------------
def steer(work):
    atoms, fr = C.md_frames()
    lam = r32(cfg.path_lambda(fr))
    s_spec = cfg.path_specs('fold', atoms, fr, lam)[0]
    n_sys = 4
    x32 = C.systems(TRP)[[0, 5, 10, 15]]
    spec = dict(s_spec, center=1.5, center_end=r32(1.5 + 0.05 * 40), rate=r32(0.05), spring_const=8., flat_width=0.)
    st = stored([spec])
    ens = E.Ensemble(node_file(work, 'steer', lambda p: cfg.add_cv_steer(p, [spec]), False), n_sys)
    ens.define_cvs(bare([spec]))
    ens.set_pos(x32)
    alone = E.Ensemble(node_file(work, 'steer_alone', lambda p: cfg.add_cv_steer(p, [spec]), True), n_sys)
    alone.set_pos(x32)
    for t in (0, 7):
        alone.set_steer_state(STEER, clock=t)
        e, d = alone.energies_and_derivs()
        centre = alone.steer_state(STEER)['center']
        assert np.array_equal(centre[:, 0], np.full(n_sys, R.steer_center(st[0], t)))
        for s in range(n_sys):
            e_ref, g_ref, _ = R.steer_energy_and_gradient(st, x32[s].astype('f8'), t)
            compare_energy(e_ref, e.astype('f8')[s], 'clock %d, system %d (centre %.4f)' % (t, s, centre[s, 0]))
            compare_deriv(g_ref, d[s], 'clock %d, system %d' % (t, s))
        assert alone.steer_values(STEER).tobytes() == ens.cvs().tobytes()
    alone.close()
    # the work of 7 rounds of MD with the full potential, restated by the yardstick from the recorded series
    ens.init_md(0.8, 21)
    ens.record_cvs(1, 7)
    ens.run_rounds(7)
    series = ens.read_cvs()
    state = ens.steer_state(STEER)
    ens.close()
    assert series.shape == (7, n_sys, 1) and state['clock'].tolist() == [7] * n_sys
    k = st[0]['spring_const']
    for s in range(n_sys):
        want = R.steer_work(st, series[:, s, :])
        scale = sum(R.harmonic(float(v) - R.steer_center(st[0], i + 1), k, 0.)[0] + R.harmonic(float(v) - R.steer_center(st[0], i), k, 0.)[0] for i, v in enumerate(series[:, s, 0]))
        print('system %d: s over 7 rounds %s; work gpu %.15g, f64 %.15g, |difference| / scale %.3e (bound 1e-12)' %
              (s, np.round(series[:, s, 0], 4).tolist(), state['work'][s], want, abs(state['work'][s] - want) / scale))
        assert np.isfinite(state['work'][s]) and abs(state['work'][s] - want) <= 1e-12 * scale and state['work'][s] != 0.


# ---- 5. metadynamics in (s, z) ---------------------------------------------------------------------------------------------------------
def metad_file(work, tag, specs, sigma, alone, height=0.3, pace=2, capacity=5, kdT=0.):
    return node_file(work, tag, lambda p: cfg.add_cv_metadynamics(p, specs, sigma, height, pace, capacity, kdT=kdT), alone)


def metad(work):
    atoms, fr = C.md_frames()
    specs = cfg.path_specs('fold', atoms, fr, r32(cfg.path_lambda(fr)))
    x32 = C.systems(TRP)[9]
    x = x32.astype('f8')
    v_ref = R.evaluate(specs, x)
    sigma = np.array([0.3, 0.1 * v_ref[1]], 'f4')
    ens = E.Ensemble(metad_file(work, 'bias', specs, sigma, True, capacity=257), 1)
    ens.define_cvs(specs)
    ens.set_pos(x32)
    print('(s, z) = %s, sigma %s' % (np.round(v_ref, 5).tolist(), sigma.tolist()))
    for n in (1, 255, 256, 257):
        rng = np.random.default_rng(100 + n)
        centers = (v_ref[None] + rng.uniform(-2., 2., (n, 2)) * sigma.astype('f8')[None]).astype('f4')
        weights = rng.uniform(0.1, 1., n).astype('f4')
        ens.set_metad_hills(METAD, centers, weights)
        e, g = ens.energies_and_derivs()
        e_ref, g_ref, _ = R.metad_energy_and_gradient(specs, x, centers, weights, sigma)
        compare_energy(e_ref, e.astype('f8')[0], '%3d hills' % n)
        compare_deriv(g_ref, g[0], '%3d hills' % n)
    v = ens.metad_values(METAD)
    assert v.tobytes() == ens.cvs().tobytes() and abs(v[0, 0] - v_ref[0]) <= RTOL * max(abs(v_ref[0]), 1.)
    ens.close()
    # deposited centres are the bits of cvs()
    ens = md_engine(work, 'dep', specs, 0.)
    for i in range(3):
        ens.run_rounds(2)
        cv = ens.cvs()[0]
        c, w, na = ens.metad_hills(METAD)
        print('deposit %d: centre %s, cvs() %s' % (i, c[-1], cv))
        assert len(w) == 1 + i and na == 1 + i and c[-1].tobytes() == cv.tobytes(), 'the newest centre is not the bits of cvs()'
    ens.close()


MD_SIGMA = (0.3, 0.5)


def md_engine(work, tag, specs, kdT):
    ens = E.Ensemble(metad_file(work, tag, specs, MD_SIGMA, False, height=0.3, pace=2, capacity=5, kdT=kdT), 1)
    ens.set_pos(K.coords(TRP).astype('f4'))
    ens.init_md(0.8, 21)
    ens.define_cvs(specs)
    return ens


def graph(work):
    """run under UPSIDE_HIP_GRAPH=1 and =0 by the parent, which compares the two files this leaves"""
    g = os.environ.get('UPSIDE_HIP_GRAPH', 'x')
    print('UPSIDE_HIP_GRAPH=%s' % g)
    atoms, fr = C.md_frames()
    specs = cfg.path_specs('fold', atoms, fr, r32(cfg.path_lambda(fr)))
    runs = []
    for rep in range(2):
        ens = md_engine(work, 'graph' + g, specs, 2.0)
        ens.run_rounds(12)
        c, w, na = ens.metad_hills(METAD)
        assert len(w) == 5 and na == 6
        runs.append([ens.get_pos(), ens.get_mom(), c, w])
        ens.close()
    a, b = runs
    assert all(np.isfinite(v).all() for v in a)
    same = all(u.tobytes() == v.tobytes() for u, v in zip(a, b))
    print('two runs of 12 rounds: positions, momenta and the 5 hills bit-identical: %s' % same)
    print('hill centres (s, z): %s' % np.round(a[2], 4).tolist())
    assert same
    np.savez(os.path.join(work, 'graph%s.npz' % g), pos=a[0], mom=a[1], centers=a[2], weights=a[3])


# ---- 6. the restraint under MD ---------------------------------------------------------------------------------------------------------
MD_SPRING = 10.      # energy units per unit of s squared: a thermal spread of sqrt(T / k) = 0.28 in s at T = 0.8, against a margin of 2.5


def md(work):
    """8 systems with the full potential, K = 8; four restrained to s = 2 and four to s = 7 with spring_const MD_SPRING = 10"""
    atoms, fr = C.md_frames()
    s_spec = cfg.path_specs('fold', atoms, fr, r32(cfg.path_lambda(fr)))[0]
    base = node_file(work, 'mdbase', lambda p: cfg.add_cv_restraint(p, [dict(s_spec, center=2., spring_const=MD_SPRING)]), False)
    centers = np.array([2.] * 4 + [7.] * 4)
    fs = cfg.write_umbrella_windows(base, [os.path.join(work, 'md%d.up' % i) for i in range(8)], RESTRAINT, centers)
    ens = E.Ensemble.from_files(fs)
    ens.set_pos(P.golden(TRP)['pos'])
    ens.define_cvs([s_spec])
    start = ens.cvs()[:, 0]
    ens.init_md(0.8, 21)
    ens.run_rounds(200)
    v = ens.cvs()[:, 0].astype('f8')
    pos = ens.get_pos()
    ens.close()
    own = np.abs(v - centers); other = np.abs(v - centers[::-1])
    print('s at the start %.4f; spring_const %g, T = 0.8, 200 rounds' % (start[0], MD_SPRING))
    print('centres %s' % centers.tolist())
    print('s       %s' % np.round(v, 4).tolist())
    assert np.isfinite(pos).all() and np.isfinite(v).all()
    assert (own < other).all()


# ---- 7. recording, /output/cv and MBAR over a ladder in s ------------------------------------------------------------------------------
def record(work):
    atoms, fr = C.md_frames()
    specs = cfg.path_specs('fold', atoms, fr, r32(cfg.path_lambda(fr)))

    def engine():
        ens = E.Ensemble(P.fixture(TRP), 8)
        ens.set_pos(P.golden(TRP)['pos'])
        ens.init_md(np.linspace(0.7, 0.9, 8), 9)
        ens.define_cvs(specs)
        return ens
    a = engine()
    a.record_cvs(1, 20)
    a.run_rounds(20)
    series, n_stored, n_attempted = a.read_cvs(with_counts=True)
    pa = a.get_pos()
    a.close()
    assert series.shape == (20, 8, 2) and n_stored == 20 and n_attempted == 20
    b = engine()
    manual = []
    for k in range(20):
        b.run_rounds(1)
        manual.append(b.cvs())
    manual = np.array(manual)
    b.close()
    n_diff = int((manual.view('u4') != series.view('u4')).sum())
    print('recorded series against run_rounds(1) + cvs() x 20: %d of %d values differ in their bits' % (n_diff, series.size))
    assert manual.tobytes() == series.tobytes() and np.abs(series[-1] - series[0]).max() > 1e-3
    ratio, _ = value_ratios(series[-1], pa, specs)
    print('last sample against the yardstick: largest |gpu - f64| / bound %.3e' % ratio.max())
    assert ratio.max() <= 1.
    # upside_hip on a file with both kinds in /input/collective_variables
    exe = os.path.join(P.ROOT, 'upside-md_amd', 'csrc', 'upside_hip')
    path = os.path.join(work, 'cli.up')
    shutil.copyfile(P.fixture(TRP), path)
    cfg.add_collective_variables(path, specs)
    try:
        r = subprocess.run([exe, '--duration', '0.27', '--frame-interval', '0.054', '--seed', '3', '--temperature', '0.8', path],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=CLI_LIMIT)
    except subprocess.TimeoutExpired as err:
        print((err.stdout or b'').decode()[-3000:])
        print('upside_hip did not finish in %d s' % CLI_LIMIT)
        sys.exit(124)      # a hang: the parent starts nothing more
    if r.returncode:
        print(r.stdout.decode()[-3000:])
        if r.returncode < 0 or r.returncode > 1:
            sys.exit(r.returncode if r.returncode > 0 else 128 - r.returncode)      # a signal: the parent starts nothing more
        raise AssertionError('upside_hip failed')
    with pkg.h5lite.open_file(path) as f:
        pos = f.read('output/pos', 'f4'); cv = f.read('output/cv'); names = f.get_attr('cv_names', 'output')
    print('/output/pos %s, /output/cv %s %s, names %s' % (pos.shape, cv.shape, cv.dtype, list(names)))
    assert cv.dtype == np.float32 and cv.shape == (pos.shape[0], 1, 2) and pos.shape[0] >= 5 and list(names) == ['fold_s', 'fold_z']
    ratio, _ = value_ratios(cv[:, 0], pos[:, 0], specs)
    print('/output/cv against the yardstick on the stored frames: largest |gpu - f64| / bound %.3e' % ratio.max())
    assert ratio.max() <= 1. and np.abs(cv[-1] - cv[0]).max() > 1e-3
    # a 4-window ladder in s through umbrella_mbar
    base = node_file(work, 'ladder', lambda p: cfg.add_cv_restraint(p, [dict(specs[0], center=1.5, spring_const=MD_SPRING)]), False)
    centers = np.array([1.2, 1.6, 2.0, 2.4])
    fs = cfg.write_umbrella_windows(base, [os.path.join(work, 'w%d.up' % i) for i in range(4)], RESTRAINT, centers)
    ens = E.Ensemble.from_files(fs)
    ens.set_pos(P.golden(TRP)['pos'])
    ens.init_md(0.8, 21)
    ens.define_cvs(specs)
    ens.record_cvs(1, 100)
    ens.run_rounds(100)
    got = ens.umbrella_mbar(RESTRAINT, 0.8, tol=0., max_iter=50)
    ens.close()
    print('4 windows in s at %s, 100 rounds: f = %s, names %s' % (centers.tolist(), np.round(got['f'], 4).tolist(), got['names']))
    assert got['names'] == ['fold_s'] and got['periods'].tolist() == [0.] and len(got['f']) == 4 and np.isfinite(got['f']).all()
    assert np.ptp(got['f']) > 0.


# ---- 8. refusals -----------------------------------------------------------------------------------------------------------------------
def refusals(work):
    import hamiltonian_files as H
    atoms, fr = C.md_frames()
    n = len(atoms)
    good_specs = cfg.path_specs('fold', atoms, fr, 3.5)
    ens = E.Ensemble(P.fixture(TRP), 4)
    ens.set_pos(C.systems(TRP)[[1, 6, 11, 15]])
    ens.define_cvs(good_specs)
    good = ens.cvs()
    assert np.isfinite(good).all()

    def still_in_force(what):
        assert ens.n_cv == 2 and ens.cvs().tobytes() == good.tobytes(), what + ': the previous definition is no longer in force'

    def packed(kind=(8, 9), n_frame=(8, 8), lam=(3.5, 3.5), lists=None, frames=None, drop=()):
        lists = [atoms, atoms] if lists is None else lists
        rows = np.concatenate([fr[:k, :len(l)].reshape(-1, 3) for k, l in zip(n_frame, lists)]) if frames is None else frames
        p = dict(kind=np.asarray(kind, 'i4'), atom_start=np.concatenate(([0], np.cumsum([len(l) for l in lists]))).astype('i4'),
                 atoms=np.concatenate([np.asarray(l, 'i4') for l in lists]), ref_pos=np.zeros((0, 3), 'f4'), contact_r0=np.zeros(0, 'f4'),
                 contact_beta=np.zeros(len(kind), 'f4'), contact_lambda=np.zeros(len(kind), 'f4'), names=['c%d' % i for i in range(len(kind))],
                 path_n_frame=np.asarray(n_frame, 'i4'), path_lambda=np.asarray(lam, 'f4'), path_ref_pos=np.asarray(rows, 'f4'))
        for k in drop:
            del p[k]
        return p
    ens.define_cvs(packed())
    assert ens.cvs().tobytes() == good.tobytes(), 'the packed form of the good definition gives other values'
    nan_rows = fr.reshape(-1, 3).copy(); nan_rows[100, 1] = np.nan
    inf_rows = fr.reshape(-1, 3).copy(); inf_rows[-1, 2] = np.inf
    two = [atoms, atoms[:2]]
    cases = [
        ('K = 1', packed(n_frame=(8, 1)), ['1 frames; a path needs 2 to 64', 'collective variable 1 (path_z)']),
        ('K = 0', packed(n_frame=(0, 8)), ['0 frames; a path needs 2 to 64', 'collective variable 0 (path_s)']),
        ('K = 65', packed(n_frame=(8, 65), frames=np.zeros((8 * n + 65 * n, 3))), ['65 frames; a path needs 2 to 64', 'UPK_CV_PATH_MAX_FRAMES']),
        ('n = 2', packed(lists=two), ['a path selection needs at least 3 atoms', 'collective variable 1 (path_z)']),
        ('lambda = 0', packed(lam=(3.5, 0.)), ['path_lambda must be positive and finite', 'collective variable 1']),
        ('lambda < 0', packed(lam=(-1., 3.5)), ['path_lambda must be positive and finite', 'collective variable 0']),
        ('lambda nan', packed(lam=(np.nan, 3.5)), ['path_lambda must be positive and finite']),
        ('lambda inf', packed(lam=(3.5, np.inf)), ['path_lambda must be positive and finite']),
        ('frames nan', packed(frames=np.concatenate((nan_rows, fr.reshape(-1, 3)))), ['path_ref_pos is not finite', 'collective variable 0']),
        ('frames inf', packed(frames=np.concatenate((fr.reshape(-1, 3), inf_rows))), ['path_ref_pos is not finite', 'collective variable 1']),
        ('path arrays NULL', packed(drop=('path_n_frame', 'path_lambda', 'path_ref_pos')), ['path_n_frame, path_lambda and path_ref_pos must be given', 'upside_hip_cv_define3']),
        ('path_ref_pos NULL', packed(drop=('path_ref_pos',)), ['path_n_frame, path_lambda and path_ref_pos must be given']),
        ('path_lambda NULL', packed(drop=('path_lambda',)), ['path_n_frame, path_lambda and path_ref_pos must be given']),
        ('atom out of range', packed(lists=[atoms, np.array([0, 1, 60])]), ['out of range']),
        ('kind 7', packed(kind=(8, 7)), ['unknown kind 7', '4 dihedral, 5 dihedral_similarity', '8 path_s, 9 path_z']),
        ('kind 6', packed(kind=(6, 9)), ['unknown kind 6']),
        ('kind 10', packed(kind=(8, 10)), ['unknown kind 10']),
    ]
    for what, p, needles in cases:
        try:
            ens.define_cvs(p)
        except RuntimeError as err:
            print('%-24s refused: %s' % (what, err))
            for nd in needles:
                assert nd in str(err), (what, nd, str(err))
        else:
            raise AssertionError('%s: the definition was accepted' % what)
        still_in_force(what)
    # the older entry points carry no frames: a path kind is refused there
    c = ens.calc
    kind = np.array([8], 'i4'); start = np.array([0, n], 'i4'); at = np.asarray(atoms, 'i4'); z = np.zeros(1, 'f4')
    for what, rc in (('upside_hip_cv_define, kind 8', c.upside_hip_cv_define(ens.engine, 1, kind.ctypes.data, start.ctypes.data, at.ctypes.data, None, None, z.ctypes.data, z.ctypes.data)),
                     ('upside_hip_cv_define2, kind 8', c.upside_hip_cv_define2(ens.engine, 1, kind.ctypes.data, start.ctypes.data, at.ctypes.data, None, None, z.ctypes.data, z.ctypes.data, None))):
        msg = c.upside_hip_last_error().decode()
        print('%-30s refused: %s' % (what, msg))
        assert rc != 0 and 'path_n_frame, path_lambda and path_ref_pos must be given' in msg
        still_in_force(what)
    # the older entry point still serves the older kinds
    kind[0] = 0
    assert c.upside_hip_cv_define2(ens.engine, 1, kind.ctypes.data, start.ctypes.data, at.ctypes.data, None, None, z.ctypes.data, z.ctypes.data, None) == 0
    assert ens.n_cv == 1 and np.isfinite(ens.cvs()).all()
    ens.define_cvs(good_specs)
    still_in_force('the good definition again')

    # the HDF5 path
    def bad_file(tag, fix):
        bad = os.path.join(work, 'bad_%s.up' % tag)
        shutil.copyfile(P.fixture(TRP), bad)
        cfg.add_collective_variables(bad, good_specs)
        with pkg.h5lite.open_file(bad, 'r+') as f:
            fix(f)
        return bad

    def rewrite(f, name, value):
        f.delete('input/collective_variables/' + name)
        if value is not None:
            f.write('input/collective_variables/' + name, value)
    g = 'input/collective_variables/'
    file_cases = [
        ('short rows', lambda f: rewrite(f, 'path_ref_pos', np.zeros((2 * 8 * n - 1, 3), 'f4')), ['path_ref_pos holds 319 rows', '320']),
        ('long rows', lambda f: rewrite(f, 'path_ref_pos', np.zeros((2 * 8 * n + 20, 3), 'f4')), ['path_ref_pos holds 340 rows', '320']),
        ('absent rows', lambda f: rewrite(f, 'path_ref_pos', None), ['come together']),
        ('all three absent', lambda f: [rewrite(f, k, None) for k in cfg.CV_PATH_DATASETS], ['is a path kind', 'absent']),
        ('K = 1', lambda f: rewrite(f, 'path_n_frame', np.array([8, 1], 'i4')), ['1 frames; a path needs 2 to 64']),
        ('K = 65', lambda f: rewrite(f, 'path_n_frame', np.array([65, 8], 'i4')), ['65 frames; a path needs 2 to 64']),
        ('short path_lambda', lambda f: rewrite(f, 'path_lambda', np.array([3.5], 'f4')), ['must have n_cv entries']),
        ('lambda = 0', lambda f: rewrite(f, 'path_lambda', np.array([3.5, 0.], 'f4')), ['path_lambda must be positive and finite']),
        ('frames nan', lambda f: rewrite(f, 'path_ref_pos', np.concatenate((nan_rows, nan_rows)).astype('f4')), ['path_ref_pos is not finite']),
        ('n = 2', lambda f: (rewrite(f, 'atoms', np.concatenate((atoms, atoms[:2])).astype('i4')), rewrite(f, 'atom_start', np.array([0, n, n + 2], 'i4')),
                             rewrite(f, 'path_ref_pos', np.zeros((8 * n + 16, 3), 'f4'))), ['at least 3 atoms']),
    ]
    for tag, fix, needles in file_cases:
        bad = bad_file(tag.replace(' ', '_').replace('=', ''), fix)
        try:
            ens.load_cvs(bad)
        except RuntimeError as err:
            print('%-24s refused: %s' % ('load_cvs, ' + tag, err))
            for nd in needles:
                assert nd in str(err), (tag, nd, str(err))
            assert '/input/collective_variables' in str(err) or 'collective variable' in str(err)
        else:
            raise AssertionError('a group with %s was accepted' % tag)
        still_in_force('load_cvs ' + tag)
    # a file without the path datasets loads as it did; one with them loads too
    old = os.path.join(work, 'old.up'); new = os.path.join(work, 'new.up')
    for p in (old, new):
        shutil.copyfile(P.fixture(TRP), p)
    cfg.add_collective_variables(old, cfg.default_collective_variables(K.coords(TRP)))
    with pkg.h5lite.open_file(old) as f:
        assert not set(cfg.CV_PATH_DATASETS) & set(f.group('input/collective_variables').keys())
    cfg.add_collective_variables(new, good_specs)
    assert ens.load_cvs(old) == 4 and ens.cv_periods.tolist() == [0.] * 4
    assert ens.load_cvs(new) == 2 and ens.cvs().tobytes() == good.tobytes() and ens.cv_periods.tolist() == [0., 0.] and ens.cv_names == ['fold_s', 'fold_z']
    ens.close()
    # bias nodes: the same refusals name the node; a ladder whose files differ in a path dataset names file, node and dataset
    rest = [dict(sp, center=2.5 if sp['kind'] == 'path_s' else 0.5, spring_const=2.) for sp in good_specs]
    good_path = node_file(work, 'ladder0', lambda p: cfg.add_cv_restraint(p, rest), False)
    for ds, change in (('path_ref_pos', lambda v: v + 0.25), ('path_lambda', lambda v: v * 2.), ('path_n_frame', lambda v: v - 1)):
        other = os.path.join(work, 'other_%s.up' % ds)
        shutil.copyfile(good_path, other)
        H.rewrite(other, RESTRAINT, ds, change)
        try:
            E.Ensemble.from_files([good_path, other])
        except RuntimeError as err:
            print('a ladder differing in %s refused: %s' % (ds, err))
            assert 'other_%s.up' % ds in str(err) and RESTRAINT in str(err) and ds in str(err)
        else:
            raise AssertionError('a ladder differing in %s was accepted' % ds)
    short = os.path.join(work, 'short_rows.up')
    shutil.copyfile(good_path, short)
    H.rewrite(short, RESTRAINT, 'path_ref_pos', lambda v: v[:100])
    try:
        E.Ensemble(short, 2)
    except RuntimeError as err:
        print('a node with short path_ref_pos refused: %s' % err)
        assert 'path_ref_pos holds 100 rows' in str(err) and RESTRAINT in str(err)
    else:
        raise AssertionError('a node with short path_ref_pos was constructed')
    ens = E.Ensemble.from_files([good_path, good_path])      # the process is still usable
    ens.set_pos(K.coords(TRP).astype('f4'))
    e = ens.energies()
    ens.close()
    assert np.isfinite(e).all() and e[0] == e[1]


CHECKS = dict(values=values, batch=batch, restraint=restraint, steer=steer, metad=metad, graph=graph, md=md, record=record, refusals=refusals)

if __name__ == '__main__':
    import torch
    assert torch.cuda.is_available(), 'these checks need a GPU'
    which, workdir = sys.argv[1], sys.argv[2]
    CHECKS[which](workdir)
    print('CHECK %s PASSED' % which)
