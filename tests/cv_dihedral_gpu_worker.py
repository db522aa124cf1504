"""Child process of tests/test_gpu_cv_dihedral.py: one check of the torsional collective variables (kinds dihedral and
dihedral_similarity) and of the periodic rule of cv_restraint and cv_metadynamics per invocation,

    python tests/cv_dihedral_gpu_worker.py CHECK WORKDIR

prints every figure it compares before it asserts and ends with 'CHECK <name> PASSED'.  The yardstick is
tests/cv_dihedral_reference.py (float64 numpy, pinned by tests/test_cv_dihedral_config.py).  Everything runs on trpcage20 (60 atoms).
Bounds: a value within parity_util.RTOL x max(|value|, 1), a dihedral's difference taken on the circle; a bias energy within 1e-6
relative; a derivative within RTOL as relative RMS and 10 x RTOL of its scale in the largest element; equalities between engine
runs are bitwise."""
import os
import shutil
import subprocess
import sys
import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import parity_util as P                  # noqa: E402
import cv_restraint_cases as K           # noqa: E402
import cv_dihedral_reference as D        # noqa: E402

pkg = P.pkg
cfg = pkg.config
E = pkg.engine
RTOL = P.RTOL
NAME = 'trpcage20_7A'
N_ATOM = 60
RESTRAINT = 'cv_restraint'
METAD = 'cv_metadynamics'
VALUES = ('center', 'spring_const', 'flat_width')
CLI_LIMIT = 240      # seconds for one upside_hip run


# ---- inputs --------------------------------------------------------------------------------------------------------------------------
def backbone():
    return cfg.backbone_dihedrals(P.fixture(NAME))


def omega(r):
    """CA, C of residue r, N, CA of residue r + 1"""
    return (3 * r + 1, 3 * r + 2, 3 * r + 3, 3 * r + 4)


def random_quads(rng, m):
    return np.array([rng.choice(N_ATOM, 4, replace=False) for _ in range(m)], 'i4')


def place_fourth(x, quad, phi):
    """move atom quad[3] so that the torsion of quad is phi (before the rounding to float32 that follows)"""
    r1, r2, r3 = (x[int(i)] for i in quad[:3])
    u = (r3 - r2) / np.linalg.norm(r3 - r2)
    p = (r1 - r2) - np.dot(r1 - r2, u) * u; p /= np.linalg.norm(p)
    x[int(quad[3])] = r3 + 0.5 * u + 1.3 * (np.cos(phi) * p + np.sin(phi) * np.cross(u, p))


def stored(specs):
    """the specs with every number rounded to the float32 the file or the engine holds: the yardstick sees the same definition"""
    out = []
    for sp in specs:
        sp = dict(sp)
        for k in ('ref', 'r0'):
            if k in sp:
                sp[k] = np.asarray(sp[k], 'f4').astype('f8')
        for k in ('beta', 'lambda') + VALUES:
            if k in sp:
                sp[k] = float(np.float32(sp[k]))
        out.append(sp)
    return out


def bare(specs):
    return [dict((k, v) for k, v in sp.items() if k not in VALUES) for sp in specs]


def value_ratio(gpu, ref, specs):
    """|gpu - f64| / (RTOL max(|f64|, 1)) per entry, gpu and ref (..., n_cv); a dihedral's difference on the circle"""
    gpu = np.asarray(gpu, 'f8'); ref = np.asarray(ref, 'f8')
    per = np.array([sp['kind'] == 'dihedral' for sp in specs])
    diff = np.where(per, D.circle_distance(gpu, ref), np.abs(gpu - ref))
    return diff / (RTOL * np.maximum(np.abs(ref), 1.))


def check_values(gpu, x32, specs, what):
    ref = np.array([D.evaluate(stored(specs), x) for x in np.asarray(x32, 'f4').astype('f8')])
    assert np.isfinite(gpu).all(), (what, 'a value is not finite')
    ratio = value_ratio(gpu, ref, specs)
    for kind in sorted(set(sp['kind'] for sp in specs)):
        cols = [c for c, sp in enumerate(specs) if sp['kind'] == kind]
        r = ratio[:, cols]
        s, c = np.unravel_index(np.argmax(r), r.shape)
        print('%-26s %-20s largest |gpu - f64| / bound = %.3e  (system %d, %s: gpu %.9g, f64 %.9g)' %
              (what, kind, r.max(), s, specs[cols[c]].get('name', kind), gpu[s, cols[c]], ref[s, cols[c]]))
    assert ratio.max() <= 1., (what, 'largest ratio', ratio.max())
    return ref


def compare_deriv(ref, got, what):
    e1 = P.rel_rms(ref, got); e2 = P.max_rel_to_scale(ref, got)
    print('%-44s derivative: rel_rms %.3e (bound %.0e), largest element / scale %.3e (bound %.0e)' % (what, e1, RTOL, e2, 10 * RTOL))
    assert e1 <= RTOL and e2 <= 10 * RTOL, what


def strip_potential(path):
    with pkg.h5lite.open_file(path, 'r+') as t:
        pot = t.group('input/potential')
        for k in pot.keys():
            pkg.h5lite.Node.delete(pot, k)


def restraint_file(work, tag, specs, alone):
    p = os.path.join(work, '%s.up' % tag)
    shutil.copyfile(P.fixture(NAME), p)
    if alone:
        strip_potential(p)
    cfg.add_cv_restraint(p, specs)
    return p


def metad_file(work, tag, specs, sigma, alone, height=0.3, pace=2, capacity=5, kdT=0.):
    p = os.path.join(work, '%s.up' % tag)
    shutil.copyfile(P.fixture(NAME), p)
    if alone:
        strip_potential(p)
    cfg.add_cv_metadynamics(p, specs, sigma, height, pace, capacity, kdT=kdT)
    return p


# ---- 1. values -------------------------------------------------------------------------------------------------------------------------
CIS = (40, 41, 42, 43)
TRANS = (50, 51, 52, 53)


def value_specs():
    phi_q, phi_r, psi_q, psi_r = backbone()
    specs = [{'name': 'phi%d' % r, 'kind': 'dihedral', 'atoms': q} for q, r in zip(phi_q, phi_r)]
    specs += [{'name': 'psi%d' % r, 'kind': 'dihedral', 'atoms': q} for q, r in zip(psi_q, psi_r)]
    specs += [{'name': 'omega%d' % r, 'kind': 'dihedral', 'atoms': omega(r)} for r in (2, 9, 15)]
    rng = np.random.default_rng(41)
    for m in (1, 255, 256, 257, 600):      # one lane, one short of / exactly / one past a full stride of CV_BLOCK = 256 lanes, three strides
        specs.append({'name': 'sim%d' % m, 'kind': 'dihedral_similarity', 'quads': random_quads(rng, m), 'ref': rng.uniform(-np.pi, np.pi, m)})
    specs.append(cfg.helix_content_spec(P.fixture(NAME)))
    specs += [{'name': 'planar_cis', 'kind': 'dihedral', 'atoms': CIS}, {'name': 'planar_trans', 'kind': 'dihedral', 'atoms': TRANS}]
    assert len(specs) <= cfg.CV_MAX
    return specs, phi_r, psi_r


def values(work):
    specs, phi_r, psi_r = value_specs()
    pos0 = cfg.read_pos(P.fixture(NAME)).astype('f8')
    n_sys = 16
    rng = np.random.default_rng(13)
    x = np.repeat(pos0[None], n_sys, 0)
    x[:n_sys - 1] += np.linspace(0., 3., n_sys - 1)[:, None, None] * rng.standard_normal((n_sys - 1,) + pos0.shape)
    # the last system: four atoms exactly in a plane, r1 and r4 on the same side of the axis (cis) and on opposite sides (trans)
    x[n_sys - 1, list(CIS)] = np.array([[1., 0., 5.], [0., 0., 5.], [0., 1., 5.], [1., 1., 5.]]) + np.array([8., -4., 0.])
    x[n_sys - 1, list(TRANS)] = np.array([[1., 0., 5.], [0., 0., 5.], [0., 1., 5.], [-1., 1., 5.]]) + np.array([-16., 2., 0.])
    x = x.astype('f4')
    ens = E.Ensemble(P.fixture(NAME), n_sys)
    ens.define_cvs(specs)
    assert ens.n_cv == len(specs) and ens.cv_names == [sp['name'] for sp in specs]
    per = ens.cv_periods
    assert per.shape == (len(specs),) and all((p == 2. * np.pi) == (sp['kind'] == 'dihedral') for p, sp in zip(per, specs)) and set(per.tolist()) == {0., 2. * np.pi}
    ens.set_pos(x)
    gpu = ens.cvs()
    assert ens.get_pos().tobytes() == x.tobytes()
    print('%d CVs, %d systems' % (len(specs), n_sys))
    ref = check_values(gpu, x, specs, NAME)
    near = [c for c, sp in enumerate(specs) if sp['name'].startswith('omega')]
    print('omega torsions of the unperturbed structure: gpu %s, f64 %s' % (gpu[0, near], ref[0, near]))
    assert (np.abs(ref[0, near]) > 2.8).all(), 'the omega torsions are meant to lie beside +-pi'
    c_cis, c_trans = len(specs) - 2, len(specs) - 1
    print('exactly planar: cis gpu %r (f64 %r), trans gpu %r (f64 %r)' % (float(gpu[-1, c_cis]), ref[-1, c_cis], float(gpu[-1, c_trans]), ref[-1, c_trans]))
    assert gpu[-1, c_cis] == 0. and not np.signbit(gpu[-1, c_cis]) and gpu[-1, c_trans] == np.float32(np.pi) and ref[-1, c_cis] == 0. and ref[-1, c_trans] == np.pi
    sim = [c for c, sp in enumerate(specs) if sp['kind'] == 'dihedral_similarity']
    assert (gpu[:, sim] >= 0.).all() and (gpu[:, sim] <= 1.).all()
    # system 0 carries no noise: the phi / psi CVs are the angles of the rama_coord node (rows with a dummy angle have no CV)
    ens.energies()
    rama32 = np.zeros((20, 2), 'f4')      # (get_output of the reference's C interface: system 0's rows)
    assert ens.calc.get_output(rama32.size, rama32.ctypes.data, ens.engine, b'rama_coord') == 0
    rama = rama32.astype('f8')
    n_phi = len(phi_r)
    d_phi = D.circle_distance(gpu[0, :n_phi], rama[phi_r, 0]); d_psi = D.circle_distance(gpu[0, n_phi:n_phi + len(psi_r)], rama[psi_r, 1])
    bound_phi = RTOL * np.maximum(np.abs(rama[phi_r, 0]), 1.); bound_psi = RTOL * np.maximum(np.abs(rama[psi_r, 1]), 1.)
    print('against get_output(rama_coord) of system 0: largest |difference| / bound: phi %.3e, psi %.3e' % ((d_phi / bound_phi).max(), (d_psi / bound_psi).max()))
    assert rama.shape == (20, 2) and (d_phi <= bound_phi).all() and (d_psi <= bound_psi).all()
    ens.close()


# ---- 2. batch independence -------------------------------------------------------------------------------------------------------------
def batch(work):
    specs, _, _ = value_specs()
    pos0 = cfg.read_pos(P.fixture(NAME)).astype('f8')
    rng = np.random.default_rng(3)
    n_sys = 64
    x = (pos0[None] + rng.standard_normal((n_sys,) + pos0.shape)).astype('f4')
    for s in (0, 7, n_sys - 1):
        x[s] = (pos0 + 0.7 * np.random.default_rng(4).standard_normal(pos0.shape)).astype('f4')
    runs = []
    for rep in range(2):
        ens = E.Ensemble(P.fixture(NAME), n_sys)
        ens.define_cvs(specs); ens.set_pos(x)
        runs.append(ens.cvs())
        ens.close()
    assert runs[0].tobytes() == runs[1].tobytes(), 'two runs differ'
    for s in (7, n_sys - 1):
        assert runs[0][s].tobytes() == runs[0][0].tobytes(), 'system %d differs from system 0 at the same positions' % s
    assert all(runs[0][s].tobytes() != runs[0][0].tobytes() for s in range(n_sys) if s not in (0, 7, n_sys - 1))
    check_values(runs[0], x, specs, '%s x %d' % (NAME, n_sys))
    print('systems 0, 7 and %d of %d bit-identical, two runs bit-identical' % (n_sys - 1, n_sys))


# ---- 3. the restraint against the yardstick --------------------------------------------------------------------------------------------
def restraint_case():
    """positions and one node's worth of restrained CVs: two dihedrals outside their window (one with a flat bottom), one inside its
    flat bottom, one whose centre (+3.0) lies across the cut from its value (-3.0), a dihedral_similarity over 257 quadruples, the
    helix content and one older kind"""
    phi_q, phi_r, psi_q, psi_r = backbone()
    x = K.perturbed(NAME)
    cut = omega(9)
    place_fourth(x, cut, -3.0)
    x = x.astype('f4').astype('f8')
    rng = np.random.default_rng(17)
    ca = np.arange(1, N_ATOM, 3, dtype='i4')
    specs = [{'name': 'phi5', 'kind': 'dihedral', 'atoms': phi_q[list(phi_r).index(5)]},
             {'name': 'psi12_flat', 'kind': 'dihedral', 'atoms': psi_q[list(psi_r).index(12)]},
             {'name': 'phi15_inside', 'kind': 'dihedral', 'atoms': phi_q[list(phi_r).index(15)]},
             {'name': 'omega9_cut', 'kind': 'dihedral', 'atoms': cut},
             {'name': 'sim257', 'kind': 'dihedral_similarity', 'quads': random_quads(rng, 257), 'ref': rng.uniform(-np.pi, np.pi, 257)},
             cfg.helix_content_spec(P.fixture(NAME)),
             {'name': 'rg_ca', 'kind': 'rg', 'atoms': ca}]
    v = D.evaluate(specs, x)
    place = [(v[0] + 0.4, 8., 0.), (v[1] - 0.5, 6., 0.1), (v[2] + 0.05, 9., 0.2), (3.0, 6., 0.), (v[4] + 0.1, 40., 0.), (0.9, 30., 0.02), (0.9 * v[6], 1.5, 0.)]
    for sp, (c, k, w) in zip(specs, place):
        sp['center'] = float(c); sp['spring_const'] = float(k); sp['flat_width'] = float(w)
    return x, specs, v


def rows_of(specs):
    return np.concatenate([[np.float32(sp.get(k, 0.)) for sp in specs] for k in VALUES]).astype('f4')


def restraint(work):
    x, specs, v0 = restraint_case()
    st = stored(specs)
    print('values at the test positions: %s' % dict((sp['name'], round(float(a), 4)) for sp, a in zip(specs, v0)))
    assert abs(v0[3] + 3.0) < 1e-5, 'the torsion across the cut is meant to be -3.0'
    ens = E.Ensemble(restraint_file(work, 'res', specs, True), 1)
    ens.define_cvs(bare(specs))
    ens.set_pos(x.astype('f4'))
    assert ens.get_pos()[0].astype('f8').tobytes() == x.tobytes()
    e, d = ens.energies_and_derivs()
    e = e.astype('f8')
    e_ref, g_ref, v_ref = D.restraint_energy_and_gradient(st, x)
    vals = ens.restraint_values(RESTRAINT); cvs = ens.cvs()
    print('all %d CVs: energy gpu %.9g, f64 %.9g, relative difference %.3e (bound 1e-6)' % (len(specs), e[0], e_ref, abs(e[0] - e_ref) / abs(e_ref)))
    assert abs(e[0] - e_ref) <= 1e-6 * abs(e_ref)
    compare_deriv(g_ref, d[0], 'all CVs')
    print('largest |value - f64| / bound %.3e; restraint_values against cvs(): bitwise %s' % (value_ratio(vals[0], v_ref, specs).max(), vals.tobytes() == cvs.tobytes()))
    assert value_ratio(vals[0], v_ref, specs).max() <= 1. and vals.shape == (1, len(specs)) and vals.tobytes() == cvs.tobytes()
    full = rows_of(specs)
    n = len(specs)
    for c, sp in enumerate(st):      # each CV alone, through set_param: the others switched off by spring_const = 0
        row = full.copy(); row[n:2 * n] = 0.; row[n + c] = full[n + c]
        ens.set_param(row, RESTRAINT)
        e1, d1 = ens.energies_and_derivs()
        e1 = e1.astype('f8')
        er, gr, _ = D.restraint_energy_and_gradient([sp], x)
        if sp['name'].endswith('inside'):
            print('  %-14s inside its flat bottom: energy %r, largest |derivative| %r' % (sp['name'], float(e1[0]), float(np.abs(d1).max())))
            assert er == 0. and e1[0] == 0. and not d1.any()
            continue
        print('  %-14s energy gpu %.9g, f64 %.9g (%.1e)' % (sp['name'], e1[0], er, abs(e1[0] - er) / er))
        assert er > 0. and abs(e1[0] - er) <= 1e-6 * er, sp['name']
        compare_deriv(gr, d1[0], '  ' + sp['name'])
        if sp['name'] == 'omega9_cut':      # the nearest image of the centre: 2 pi - 6 away, not 6
            want = 0.5 * sp['spring_const'] * (2. * np.pi - 6.) ** 2
            print('  %-14s across the cut: 1/2 k (2 pi - 6)^2 = %.6g; the plain difference would give %.6g' % (sp['name'], want, 0.5 * sp['spring_const'] * 36.))
            assert abs(e1[0] - want) <= 1e-3 * want      # (the torsion was placed at -3.0 before its atoms were rounded to float32)
    ens.close()
    # no direction: three collinear atoms and two coincident ones give zero force and a finite energy
    xs = x.astype('f4')
    xs[[20, 21, 22]] = np.array([[1., 2., 3.], [2., 2., 3.], [4., 2., 3.]], 'f4')
    xs[31] = xs[30]
    small = [dict(sp, center=1., spring_const=3.) for sp in ({'name': 'collinear', 'kind': 'dihedral', 'atoms': (20, 21, 22, 25)}, {'name': 'coincident', 'kind': 'dihedral', 'atoms': (29, 30, 31, 32)},
                                                               {'name': 'sim', 'kind': 'dihedral_similarity', 'quads': [(25, 22, 21, 20), (30, 31, 29, 33)], 'ref': [0.4, -1.]})]
    ens = E.Ensemble(restraint_file(work, 'small', small, True), 1)
    ens.set_pos(xs)
    e, d = ens.energies_and_derivs()
    e = e.astype('f8')
    e_ref = D.restraint_energy_and_gradient(stored(small), xs.astype('f8'))[0]
    print('collinear and coincident atoms: values %s, energy gpu %.9g, f64 %.9g, largest |derivative| %r' % (ens.restraint_values(RESTRAINT)[0], e[0], e_ref, float(np.abs(d).max())))
    assert np.isfinite(e).all() and e_ref > 0. and abs(e[0] - e_ref) <= 1e-6 * e_ref and not d.any()
    ens.close()


# ---- 4. the restraint under MD ---------------------------------------------------------------------------------------------------------
def md(work):
    phi_q, phi_r, psi_q, psi_r = backbone()
    spec = {'name': 'psi10', 'kind': 'dihedral', 'atoms': psi_q[list(psi_r).index(10)], 'center': 0., 'spring_const': 50.}
    base = restraint_file(work, 'mdbase', [spec], False)
    centers = np.array([0.9 * np.pi] * 4 + [-0.1 * np.pi] * 4)
    fs = cfg.write_umbrella_windows(base, [os.path.join(work, 'md%d.up' % i) for i in range(8)], RESTRAINT, centers)
    ens = E.Ensemble.from_files(fs)
    ens.set_pos(P.golden(NAME)['pos'])
    ens.define_cvs(bare([spec]))
    start = ens.cvs()[:, 0]
    ens.init_md(0.8, 21)
    ens.run_rounds(200)
    v = ens.cvs()[:, 0].astype('f8')
    pos = ens.get_pos()
    ens.close()
    own = D.circle_distance(v, centers); other = D.circle_distance(v, centers[::-1])
    print('psi of residue 10 at the start %.4f; spring_const 50, T = 0.8, 200 rounds' % start[0])
    print('centres %s' % np.round(centers, 4).tolist())
    print('values  %s' % np.round(v, 4).tolist())
    print('distance on the circle to the own centre %s, to the other group\'s %s' % (np.round(own, 4).tolist(), np.round(other, 4).tolist()))
    assert np.isfinite(pos).all() and np.isfinite(v).all()
    assert (own < other).all()


# ---- 5. metadynamics -------------------------------------------------------------------------------------------------------------------
def hills_beside_the_cut(v, sigma, n, seed, periodic):
    """n hills with centres within +-2 sigma of v, folded into (-pi, pi] in the periodic dimensions, weights in [0.1, 1], float32"""
    rng = np.random.default_rng(seed)
    c = np.asarray(v, 'f8')[None, :] + rng.uniform(-2., 2., (n, len(v))) * np.asarray(sigma, 'f8')[None, :]
    for k in np.nonzero(periodic)[0]:
        c[:, k] = D.wrap(c[:, k])
    return c.astype('f4'), rng.uniform(0.1, 1., n).astype('f4')


def metad(work):
    phi_q, phi_r, psi_q, psi_r = backbone()
    phi = {'name': 'phi10', 'kind': 'dihedral', 'atoms': phi_q[list(phi_r).index(10)]}
    psi = {'name': 'psi10', 'kind': 'dihedral', 'atoms': psi_q[list(psi_r).index(10)]}
    rg = {'name': 'rg', 'kind': 'rg', 'atoms': np.arange(N_ATOM, dtype='i4')}
    x = K.perturbed(NAME)
    place_fourth(x, phi['atoms'], 3.1)        # phi just below +pi, psi just above -pi: hills within 2 sigma lie on both sides of the cut
    place_fourth(x, psi['atoms'], -3.12)
    x = x.astype('f4').astype('f8')
    for tag, specs in (('phipsi', [phi, psi]), ('phirg', [phi, rg])):
        v_ref = D.evaluate(specs, x)
        periodic = np.array([sp['kind'] == 'dihedral' for sp in specs])
        sigma = np.where(periodic, 0.2, 0.1 * np.abs(v_ref)).astype('f4')
        ens = E.Ensemble(metad_file(work, 'bias_' + tag, specs, sigma, True, capacity=257), 1)
        ens.define_cvs(specs)
        ens.set_pos(x.astype('f4'))
        print('%s: values %s, sigma %s' % (tag, np.round(v_ref, 5).tolist(), sigma.tolist()))
        for n in (1, 255, 256, 257):
            centers, weights = hills_beside_the_cut(v_ref, sigma, n, 100 + n, periodic)
            if n > 1:
                across = np.abs(centers[:, 0].astype('f8') - v_ref[0]) > np.pi
                assert across.any() and (~across).any(), 'the hills are meant to lie on both sides of the cut'
            ens.set_metad_hills(METAD, centers, weights)
            e, g = ens.energies_and_derivs()
            e = e.astype('f8')
            e_ref, g_ref, _ = D.metad_energy_and_gradient(specs, x, centers, weights, sigma)
            print('%s, %3d hills: energy gpu %.9g, f64 %.9g, relative difference %.3e (bound 1e-6)' % (tag, n, e[0], e_ref, abs(e[0] - e_ref) / abs(e_ref)))
            assert e_ref > 0. and abs(e[0] - e_ref) <= 1e-6 * abs(e_ref)
            compare_deriv(g_ref, g[0], '%s, %3d hills' % (tag, n))
        v = ens.metad_values(METAD)
        assert v.tobytes() == ens.cvs().tobytes() and value_ratio(v[0], v_ref, specs).max() <= 1.
        ens.close()
    deposit(work, [phi, psi])


MD_SIGMA = (0.35, 0.35)
HEIGHT = 0.3


def md_engine(work, tag, specs, kdT):
    ens = E.Ensemble(metad_file(work, tag, specs, MD_SIGMA, False, height=HEIGHT, pace=2, capacity=5, kdT=kdT), 1)
    ens.set_pos(K.coords(NAME).astype('f4'))
    ens.init_md(0.8, 21)
    ens.define_cvs(specs)
    return ens


def deposit(work, specs):
    """well-tempered deposition in (phi, psi): centres are the bits of cvs(), weights follow the yardstick's wrapped hill sum"""
    h32 = np.float32(HEIGHT); kdT = 2.0
    sigma = np.asarray(MD_SIGMA, 'f4').astype('f8')
    ens = md_engine(work, 'dep', specs, kdT)
    # two hills written beforehand, a period away from where the walker is: only a wrapped sum sees them at their full weight
    start = ens.cvs()[0]
    pre_c = (start[None, :].astype('f8') + np.array([[2. * np.pi - 0.1, 0.05], [0.1, 0.1 - 2. * np.pi]])).astype('f4'); pre_w = np.array([0.5, 0.4], 'f4')
    ens.set_metad_hills(METAD, pre_c, pre_w)
    for i in range(3):
        ens.run_rounds(2)
        cv = ens.cvs()[0]
        c, w, na = ens.metad_hills(METAD)
        assert len(w) == 3 + i and na == 3 + i and c[:2].tobytes() == pre_c.tobytes()      # (written hills count as attempts)
        assert c[-1].tobytes() == cv.tobytes(), 'the newest centre is not the bits of cvs()'
        v_at = D.bias(c[-1].astype('f8'), c[:-1], w[:-1], sigma, [D.TWO_PI, D.TWO_PI])[0]
        plain = D.bias(c[-1].astype('f8'), c[:-1], w[:-1], sigma, [0., 0.])[0]
        want = float(h32) * np.exp(-v_at / kdT)
        print('deposit %d at %s: V of the %d earlier hills %.9g (unwrapped it would be %.3g): weight %.9g, f64 %.9g, relative difference %.3e (bound 1e-6)'
              % (i, cv, len(w) - 1, v_at, plain, w[-1], want, abs(w[-1] - want) / want))
        assert abs(float(w[-1]) - want) <= 1e-6 * want and w[-1] < h32 and v_at > plain + 0.05
    ens.close()


def graph(work):
    """run under UPSIDE_HIP_GRAPH=1 and =0 by the parent, which compares the two files this leaves"""
    g = os.environ.get('UPSIDE_HIP_GRAPH', 'x')
    print('UPSIDE_HIP_GRAPH=%s' % g)
    phi_q, phi_r, psi_q, psi_r = backbone()
    specs = [{'name': 'phi10', 'kind': 'dihedral', 'atoms': phi_q[list(phi_r).index(10)]}, {'name': 'psi10', 'kind': 'dihedral', 'atoms': psi_q[list(psi_r).index(10)]}]
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
    assert same
    np.savez(os.path.join(work, 'graph%s.npz' % g), pos=a[0], mom=a[1], centers=a[2], weights=a[3])


# ---- 6. recording and /output/cv -------------------------------------------------------------------------------------------------------
def record_specs():
    phi_q, phi_r, psi_q, psi_r = backbone()
    return [{'name': 'phi10', 'kind': 'dihedral', 'atoms': phi_q[list(phi_r).index(10)]}, dict(cfg.helix_content_spec(P.fixture(NAME)), name='helix'),
            {'name': 'omega9', 'kind': 'dihedral', 'atoms': omega(9)}]


def record(work):
    specs = record_specs()

    def engine():
        ens = E.Ensemble(P.fixture(NAME), 8)
        ens.set_pos(P.golden(NAME)['pos'])
        ens.init_md(np.linspace(0.7, 0.9, 8), 9)
        ens.define_cvs(specs)
        return ens
    a = engine()
    a.record_cvs(1, 40)
    a.run_rounds(40)
    series, n_stored, n_attempted = a.read_cvs(with_counts=True)
    pa = a.get_pos()
    a.close()
    assert series.shape == (40, 8, len(specs)) and n_stored == 40 and n_attempted == 40
    b = engine()
    manual = []
    for k in range(40):
        b.run_rounds(1)
        manual.append(b.cvs())
    manual = np.array(manual)
    b.close()
    n_diff = int((manual.view('u4') != series.view('u4')).sum())
    print('recorded series against run_rounds(1) + cvs() x 40: %d of %d values differ in their bits' % (n_diff, series.size))
    assert manual.tobytes() == series.tobytes() and np.abs(series[-1] - series[0]).max() > 1e-3
    check_values(series[-1], pa, specs, 'last sample')
    # upside_hip on a file that defines a phi and a helix-content CV
    exe = os.path.join(P.ROOT, 'upside-md_amd', 'csrc', 'upside_hip')
    path = os.path.join(work, 'cli.up')
    shutil.copyfile(P.fixture(NAME), path)
    cfg.add_collective_variables(path, specs[:2])
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
    assert cv.dtype == np.float32 and cv.shape == (pos.shape[0], 1, 2) and pos.shape[0] >= 5 and list(names) == ['phi10', 'helix']
    check_values(cv[:, 0], pos[:, 0], specs[:2], '/output/cv')
    assert np.abs(cv[-1] - cv[0]).max() > 1e-3


# ---- 7. refusals -----------------------------------------------------------------------------------------------------------------------
def refusals(work):
    import ctypes as ct
    import hamiltonian_files as H
    ens = E.Ensemble(P.fixture(NAME), 4)
    pos0 = cfg.read_pos(P.fixture(NAME)).astype('f8')
    ens.set_pos((pos0[None] + 0.5 * np.random.default_rng(2).standard_normal((4,) + pos0.shape)).astype('f4'))
    specs = record_specs()
    ens.define_cvs(specs)
    good = ens.cvs()

    def packed(kind, lists, dref=None):
        start = np.concatenate(([0], np.cumsum([len(l) for l in lists]))).astype('i4')
        p = dict(kind=np.asarray(kind, 'i4'), atom_start=start, atoms=np.concatenate([np.asarray(l, 'i4') for l in lists]), ref_pos=np.zeros((0, 3), 'f4'),
                 contact_r0=np.zeros(0, 'f4'), contact_beta=np.zeros(len(kind), 'f4'), contact_lambda=np.zeros(len(kind), 'f4'), names=['c%d' % i for i in range(len(kind))])
        if dref is not None:
            p['dihedral_ref'] = np.asarray(dref, 'f4')
        return p

    def still_in_force(what):
        assert ens.n_cv == len(specs) and ens.cvs().tobytes() == good.tobytes(), what + ': the previous definition is no longer in force'

    cases = [
        ('dihedral of 3 atoms', packed([0, 4], [[0, 1], [1, 2, 3]], []), ['exactly 4 atoms', 'collective variable 1 (dihedral)']),
        ('dihedral of 8 atoms', packed([4], [[0, 1, 2, 3, 4, 5, 6, 7]], []), ['exactly 4 atoms']),
        ('similarity list of 6', packed([5], [[0, 1, 2, 3, 4, 5]], [0.]), ['multiple of 4', 'collective variable 0 (dihedral_similarity)']),
        ('dihedral repeats an atom', packed([4], [[0, 1, 2, 1]], []), ['quadruple 0 repeats an atom', '(dihedral)']),
        ('similarity repeats an atom', packed([0, 5], [[0, 1], [0, 1, 2, 3, 4, 5, 4, 7]], [0., 1.]), ['quadruple 1 repeats an atom', 'collective variable 1 (dihedral_similarity)']),
        ('dihedral_ref NULL', packed([5], [[0, 1, 2, 3]]), ['dihedral_ref must be given', 'collective variable 0 (dihedral_similarity)']),
        ('dihedral_ref not finite', packed([5, 5], [[0, 1, 2, 3], [4, 5, 6, 7]], [0.5, np.nan]), ['dihedral_ref is not finite', 'collective variable 1']),
        ('dihedral_ref infinite', packed([5], [[0, 1, 2, 3]], [np.inf]), ['dihedral_ref is not finite']),
        ('atom out of range', packed([4], [[0, 1, 2, N_ATOM]], []), ['out of range']),
        ('kind 7', packed([0, 7], [[0, 1], [1, 2]], []), ['unknown kind 7', '4 dihedral, 5 dihedral_similarity']),
        ('kind 6', packed([6], [[0, 1, 2, 3]], []), ['unknown kind 6']),
    ]
    for what, p, needles in cases:
        try:
            ens.define_cvs(p)
        except RuntimeError as err:
            print('%-28s refused: %s' % (what, err))
            for nd in needles:
                assert nd in str(err), (what, nd, str(err))
        else:
            raise AssertionError('%s: the definition was accepted' % what)
        still_in_force(what)
    # the old entry point carries no reference angles: a kind 5 is refused there, a kind 4 is served
    c = ens.calc
    kind = np.array([5], 'i4'); start = np.array([0, 4], 'i4'); atoms = np.array([0, 1, 2, 3], 'i4'); z = np.zeros(1, 'f4')
    rc = c.upside_hip_cv_define(ens.engine, 1, kind.ctypes.data, start.ctypes.data, atoms.ctypes.data, None, None, z.ctypes.data, z.ctypes.data)
    msg = c.upside_hip_last_error().decode()
    print('%-28s refused: %s' % ('upside_hip_cv_define, kind 5', msg))
    assert rc != 0 and 'dihedral_ref must be given' in msg
    still_in_force('the old entry point with kind 5')
    kind[0] = 4; atoms[:] = specs[0]['atoms']
    assert c.upside_hip_cv_define(ens.engine, 1, kind.ctypes.data, start.ctypes.data, atoms.ctypes.data, None, None, z.ctypes.data, z.ctypes.data) == 0
    assert ens.n_cv == 1 and ens.cvs().tobytes() == np.ascontiguousarray(good[:, :1]).tobytes()
    ens.define_cvs(specs)
    # the HDF5 path: dihedral_ref of the wrong length, and absent beside a dihedral_similarity
    for tag, fix, needle in (('short', lambda f: (f.delete('input/collective_variables/dihedral_ref'), f.write('input/collective_variables/dihedral_ref', np.zeros(3, 'f4'))), 'dihedral_ref holds 3 entries'),
                             ('absent', lambda f: f.delete('input/collective_variables/dihedral_ref'), 'dihedral_ref holds 0 entries')):
        bad = os.path.join(work, 'bad_%s.up' % tag)
        shutil.copyfile(P.fixture(NAME), bad)
        cfg.add_collective_variables(bad, specs)
        with pkg.h5lite.open_file(bad, 'r+') as f:
            fix(f)
        try:
            ens.load_cvs(bad)
        except RuntimeError as err:
            print('%-28s refused: %s' % ('load_cvs, dihedral_ref ' + tag, err))
            assert needle in str(err) and '38 quadruples' in str(err)
        else:
            raise AssertionError('a group with dihedral_ref %s was accepted' % tag)
        still_in_force('load_cvs ' + tag)
    # a file written before the kinds existed (no dihedral_ref) loads as it did; one with the kinds loads too
    old = os.path.join(work, 'old.up'); new = os.path.join(work, 'new.up')
    for p in (old, new):
        shutil.copyfile(P.fixture(NAME), p)
    cfg.add_collective_variables(old, cfg.default_collective_variables(pos0))
    with pkg.h5lite.open_file(old) as f:
        assert 'dihedral_ref' not in f.group('input/collective_variables').keys()
    cfg.add_collective_variables(new, specs)
    assert ens.load_cvs(old) == 4 and ens.cv_periods.tolist() == [0.] * 4
    assert ens.load_cvs(new) == len(specs) and ens.cvs().tobytes() == good.tobytes() and ens.cv_periods.tolist() == [2. * np.pi, 0., 2. * np.pi]
    ens.close()
    # bias nodes: the same refusals name the node; a ladder whose files differ in dihedral_ref names file, node and dataset
    rest = [dict(sp, center=0.5, spring_const=2.) for sp in specs]
    good_path = restraint_file(work, 'ladder0', rest, False)
    other = os.path.join(work, 'other_ref.up')
    shutil.copyfile(good_path, other)
    H.rewrite(other, RESTRAINT, 'dihedral_ref', lambda v: v + 0.25)
    try:
        E.Ensemble.from_files([good_path, other])
    except RuntimeError as err:
        print('a ladder differing in dihedral_ref refused: %s' % err)
        assert 'other_ref.up' in str(err) and RESTRAINT in str(err) and 'dihedral_ref' in str(err)
    else:
        raise AssertionError('a ladder differing in dihedral_ref was accepted')
    short = os.path.join(work, 'short_ref.up')
    shutil.copyfile(good_path, short)
    H.rewrite(short, RESTRAINT, 'dihedral_ref', lambda v: v[:5])
    try:
        E.Ensemble(short, 2)
    except RuntimeError as err:
        print('a node with a short dihedral_ref refused: %s' % err)
        assert 'dihedral_ref holds 5 entries' in str(err) and RESTRAINT in str(err)
    else:
        raise AssertionError('a node with a short dihedral_ref was constructed')
    ens = E.Ensemble.from_files([good_path, good_path])      # the process is still usable
    ens.set_pos(pos0.astype('f4'))
    e = ens.energies()
    ens.close()
    assert np.isfinite(e).all() and e[0] == e[1]


CHECKS = dict(values=values, batch=batch, restraint=restraint, md=md, metad=metad, graph=graph, record=record, refusals=refusals)

if __name__ == '__main__':
    import torch
    assert torch.cuda.is_available(), 'these checks need a GPU'
    which, workdir = sys.argv[1], sys.argv[2]
    CHECKS[which](workdir)
    print('CHECK %s PASSED' % which)
