"""Child process of tests/test_gpu_cv_steer.py: one check of the moving restraint on collective variables (node cv_steer) per
invocation,

    python tests/cv_steer_gpu_worker.py CHECK WORKDIR

prints every figure it compares before it asserts and ends with 'CHECK <name> PASSED'.  The yardstick is
tests/cv_steer_reference.py (float64 numpy, pinned by tests/test_cv_steer_config.py).  Everything runs on trpcage20 (60 atoms).
Bounds: an energy within 1e-6 relative; a derivative within parity_util.RTOL as relative RMS and 10 x RTOL of its scale in the
largest element; a centre within 1e-15 relative of config.steer_center; the accumulated work within 1e-12 x sum_n sum_c (|E_c(v_n,
c(n))| + |E_c(v_n, c(n-1))|) of config.steer_work of the recorded series -- both sides do a dozen IEEE fp64 operations per term on
the same fp32 inputs, 1.1e-16 each, and may differ in FMA contraction: three orders of margin, and four orders below what an fp32
accumulator or unrounded CV values would show; equalities between engine runs are bitwise."""
import os
import shutil
import subprocess
import sys
import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import parity_util as P                  # noqa: E402
import cv_restraint_cases as K           # noqa: E402
import cv_dihedral_reference as D        # noqa: E402
import cv_steer_reference as S           # noqa: E402

pkg = P.pkg
cfg = pkg.config
E = pkg.engine
RTOL = P.RTOL
NAME = 'trpcage20_7A'
N_ATOM = 60
NODE = 'cv_steer'
VALUES = S.VALUES
CLI_LIMIT = 240      # seconds for one upside_hip run


# ---- inputs --------------------------------------------------------------------------------------------------------------------------
def r32(v):
    return float(np.float32(v))


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
                sp[k] = r32(sp[k])
        out.append(sp)
    return out


def bare(specs):
    return [dict((k, v) for k, v in sp.items() if k not in VALUES) for sp in specs]


def rows_of(specs):
    return np.concatenate([[np.float32(sp.get(k, 0.)) for sp in specs] for k in VALUES]).astype('f4')


def columns(specs):
    """the five value arrays of a spec list as float64 of their float32 values, in the order of VALUES"""
    return [np.array([r32(sp.get(k, 0.)) for sp in specs], 'f8') for k in VALUES]


def compare_deriv(ref, got, what):
    e1 = P.rel_rms(ref, got); e2 = P.max_rel_to_scale(ref, got)
    print('%-44s derivative: rel_rms %.3e (bound %.0e), largest element / scale %.3e (bound %.0e)' % (what, e1, RTOL, e2, 10 * RTOL))
    assert e1 <= RTOL and e2 <= 10 * RTOL, what


def compare_energy(ref, got, what):
    rel = abs(float(got) - ref) / abs(ref)
    print('%-44s energy gpu %.9g, f64 %.9g, relative difference %.3e (bound 1e-6)' % (what, got, ref, rel))
    assert ref > 0. and rel <= 1e-6, what


def strip_potential(path):
    with pkg.h5lite.open_file(path, 'r+') as t:
        pot = t.group('input/potential')
        for k in pot.keys():
            pkg.h5lite.Node.delete(pot, k)


def steer_file(work, tag, specs, alone, name=NODE):
    p = os.path.join(work, '%s.up' % tag)
    shutil.copyfile(P.fixture(NAME), p)
    if alone:
        strip_potential(p)
    cfg.add_cv_steer(p, specs, name=name)
    return p


def place_fourth(x, quad, phi):
    """move atom quad[3] so that the torsion of quad is phi (before the rounding to float32 that follows)"""
    r1, r2, r3 = (x[int(i)] for i in quad[:3])
    u = (r3 - r2) / np.linalg.norm(r3 - r2)
    p = (r1 - r2) - np.dot(r1 - r2, u) * u; p /= np.linalg.norm(p)
    x[int(quad[3])] = r3 + 0.5 * u + 1.3 * (np.cos(phi) * p + np.sin(phi) * np.cross(u, p))


def every_kind(x):
    """11 CVs: the eight of cv_restraint_cases.force_specs (rg, three rmsd, two contacts, two distances; some inside their flat bottom)
    plus two dihedrals (one with a flat bottom) and the helix content, all at rest: rate 0, center_end = center"""
    specs = K.force_specs(NAME, x)
    phi_q, phi_r, psi_q, psi_r = cfg.backbone_dihedrals(P.fixture(NAME))
    more = [{'name': 'phi5', 'kind': 'dihedral', 'atoms': phi_q[list(phi_r).index(5)]},
            {'name': 'psi12_flat', 'kind': 'dihedral', 'atoms': psi_q[list(psi_r).index(12)]},
            dict(cfg.helix_content_spec(P.fixture(NAME)), name='helix')]
    for sp, val, (off, k, w) in zip(more, D.evaluate(more, x), ((0.4, 8., 0.), (-0.5, 6., 0.1), (0.1, 40., 0.02))):
        sp['center'] = float(val + off); sp['spring_const'] = k; sp['flat_width'] = w
    specs += more
    for sp in specs:
        sp['center'] = r32(sp['center']); sp['rate'] = 0.; sp['center_end'] = sp['center']
    assert len(specs) == 11 and sorted(set(sp['kind'] for sp in specs)) == sorted(cfg.CV_KINDS)
    return specs


N_PULL = 20      # rounds from center to center_end in the moving cases


def moving(specs, x):
    """the same CVs pulled over N_PULL rounds, alternately up and down, by 30 % of the distance between centre and value (at least 0.05)"""
    v = D.evaluate(specs, x)
    out = []
    for c, sp in enumerate(specs):
        sp = dict(sp)
        span = (1. if c % 2 == 0 else -1.) * max(0.3 * abs(v[c] - sp['center']), 0.05)
        sp['center_end'] = r32(sp['center'] + span)
        sp['rate'] = r32((sp['center_end'] - sp['center']) / N_PULL)
        out.append(sp)
    return out


# ---- 1. static: rate = 0 is a cv_restraint ---------------------------------------------------------------------------------------------
def static(work):
    x = K.perturbed(NAME)
    specs = every_kind(x)
    st = stored(specs)
    e_ref, g_ref, v_ref = S.energy_and_gradient(st, x, 0)
    ens = E.Ensemble(steer_file(work, 'static', specs, True), 1)
    ens.define_cvs(bare(specs))
    ens.set_pos(x.astype('f4'))
    e, d = ens.energies_and_derivs()
    print('%d CVs at rest: %s' % (len(specs), ', '.join(sp['name'] for sp in specs)))
    compare_energy(e_ref, e.astype('f8')[0], 'all CVs against the yardstick')
    compare_deriv(g_ref, d[0], 'all CVs against the yardstick')
    vals = ens.steer_values(NODE); cvs = ens.cvs()
    one = np.zeros(len(specs), 'f4')
    assert ens.calc.get_value_by_name(len(specs), one.ctypes.data, ens.engine, NODE.encode(), b'cv_value') == 0
    print('steer_values against cvs(): bitwise %s; get_value_by_name(cv_value) against system 0: bitwise %s' % (vals.tobytes() == cvs.tobytes(), one.tobytes() == vals[0].tobytes()))
    assert vals.shape == (1, len(specs)) and vals.tobytes() == cvs.tobytes() and one.tobytes() == vals[0].tobytes()
    assert np.abs(vals[0] - v_ref).max() <= 1e-4
    state = ens.steer_state(NODE)
    assert state['clock'].tolist() == [0] and state['work'].tolist() == [0.] and np.array_equal(state['center'][0], columns(specs)[0])
    assert np.array_equal(ens.get_param((5 * len(specs),), NODE), rows_of(specs))
    # at rest the clock does not matter
    ens.set_steer_state(NODE, clock=12345)
    e2, d2 = ens.energies_and_derivs()
    assert e2.tobytes() == e.tobytes() and d2.tobytes() == d.tobytes() and ens.steer_state(NODE)['clock'].tolist() == [12345]
    ens.close()
    # a cv_restraint node with the same rows
    rp = os.path.join(work, 'static_restraint.up')
    shutil.copyfile(P.fixture(NAME), rp); strip_potential(rp)
    cfg.add_cv_restraint(rp, [dict((k, v) for k, v in sp.items() if k not in ('rate', 'center_end')) for sp in specs])
    res = E.Ensemble(rp, 1)
    res.set_pos(x.astype('f4'))
    er, dr = res.energies_and_derivs()
    res.close()
    compare_energy(float(er[0]), e.astype('f8')[0], 'against a cv_restraint of the same rows')
    compare_deriv(dr[0], d[0], 'against a cv_restraint of the same rows')
    print('cv_steer at rest against cv_restraint: energy bit-identical %s, derivative bit-identical %s' % (er.tobytes() == e.tobytes(), dr.tobytes() == d.tobytes()))
    # a node of one CV (the hand-over through LDS is double-buffered by CV parity): an rmsd, whose rotation travels that way, and a dihedral
    for sp in (specs[1], specs[8]):
        ens = E.Ensemble(steer_file(work, 'one_' + sp['name'], [sp], True), 1)
        ens.set_pos(x.astype('f4'))
        e1, d1 = ens.energies_and_derivs()
        ens.close()
        er1, gr1, _ = S.energy_and_gradient(stored([sp]), x, 0)
        compare_energy(er1, e1.astype('f8')[0], 'n_cv = 1: ' + sp['name'])
        compare_deriv(gr1, d1[0], 'n_cv = 1: ' + sp['name'])


# ---- 2. moving: the centre follows the system's clock -----------------------------------------------------------------------------------
def moving_check(work):
    n_sys = 16
    x0 = K.perturbed(NAME)
    rng = np.random.default_rng(5)
    x = (x0[None] + 0.4 * rng.standard_normal((n_sys,) + x0.shape)).astype('f4')
    specs = moving(every_kind(x0), x0)
    st = stored(specs)
    cen, rate, end, _, _ = columns(specs)
    assert (rate > 0).sum() >= 4 and (rate < 0).sum() >= 4
    ens = E.Ensemble(steer_file(work, 'moving', specs, True), n_sys)
    ens.set_pos(x)
    for t in (0, 1, 7, N_PULL - 1, N_PULL, N_PULL + 10 ** 6):
        ens.set_steer_state(NODE, clock=t)
        e, d = ens.energies_and_derivs()
        state = ens.steer_state(NODE)
        want = cfg.steer_center(cen, rate, end, t)
        dev = np.abs(state['center'] - want[None]).max() / np.abs(want).max()
        print('clock %8d: largest |centre - steer_center| / |centre| %.3e (bound 1e-15); centres of system 0: %s' % (t, dev, np.round(state['center'][0], 5).tolist()))
        assert (np.abs(state['center'] - want[None]) <= 1e-15 * np.abs(want)[None]).all() and state['clock'].tolist() == [t] * n_sys
        assert np.array_equal(want, S.centers(st, t))
        if t >= N_PULL:
            assert (np.abs(want - end) <= 1e-6 * np.abs(end)).all() and (t == N_PULL or np.array_equal(want, end))
        for s in range(n_sys):
            e_ref, g_ref, _ = S.energy_and_gradient(st, x[s].astype('f8'), t)
            rel = abs(float(e[s]) - e_ref) / e_ref
            e1 = P.rel_rms(g_ref, d[s]); e2 = P.max_rel_to_scale(g_ref, d[s])
            if s in (0, n_sys - 1):
                print('   system %2d: energy gpu %.9g, f64 %.9g (%.1e, bound 1e-6); derivative rel_rms %.3e (bound %.0e), largest / scale %.3e (bound %.0e)' %
                      (s, e[s], e_ref, rel, e1, RTOL, e2, 10 * RTOL))
            assert rel <= 1e-6 and e1 <= RTOL and e2 <= 10 * RTOL, (t, s, rel, e1, e2)
    # every system its own clock
    clocks = np.arange(n_sys) * 3
    ens.set_steer_state(NODE, clock=clocks)
    e, _ = ens.energies_and_derivs()
    state = ens.steer_state(NODE)
    want = cfg.steer_center(cen, rate, end, clocks)
    assert want.shape == (n_sys, len(specs)) and (np.abs(state['center'] - want) <= 1e-15 * np.abs(want)).all() and state['clock'].tolist() == clocks.tolist()
    for s in (1, 5, n_sys - 1):
        e_ref = S.energy(st, x[s].astype('f8'), int(clocks[s]))
        assert abs(float(e[s]) - e_ref) <= 1e-6 * e_ref
    print('clocks %s: centres and energies per system within the bounds' % clocks.tolist())
    ens.close()
    # a dihedral whose centre has travelled from +3.0 past +pi to an unwrapped 3.5 while the value sits at -2.9: the nearest image
    quad = (28, 29, 30, 31)      # CA, C of residue 9, N, CA of residue 10
    xc = x0.copy()
    place_fourth(xc, quad, -2.9)
    xc = xc.astype('f4').astype('f8')
    cut = [{'name': 'omega9', 'kind': 'dihedral', 'atoms': quad, 'center': 3.0, 'rate': r32(0.1), 'center_end': 4.0, 'spring_const': 6., 'flat_width': 0.}]
    ens = E.Ensemble(steer_file(work, 'cut', cut, True), 1)
    ens.set_pos(xc.astype('f4'))
    ens.set_steer_state(NODE, clock=5)
    e, d = ens.energies_and_derivs()
    c = ens.steer_state(NODE)['center'][0, 0]
    v = float(ens.steer_values(NODE)[0, 0])
    ens.close()
    e_ref, g_ref, _ = S.energy_and_gradient(stored(cut), xc, 5)
    dd = float(D.wrap(v - c))
    print('across the cut: value %.6f, centre %.6f (unwrapped, beyond pi), wrapped difference %.6f; the plain difference would be %.4f' % (v, c, dd, v - c))
    compare_energy(e_ref, e.astype('f8')[0], 'across the cut')
    compare_deriv(g_ref, d[0], 'across the cut')
    assert c == 3.0 + r32(0.1) * 5 and c > np.pi and abs(v + 2.9) < 1e-5 and abs(dd + 0.11681) < 1e-4
    assert abs(float(e[0]) - 0.5 * 6. * dd * dd) <= 1e-5 * float(e[0])


# ---- 3. batch independence -------------------------------------------------------------------------------------------------------------
def batch(work):
    n_sys = 64
    x0 = K.perturbed(NAME)
    specs = moving(every_kind(x0), x0)
    rng = np.random.default_rng(3)
    x = (x0[None] + rng.standard_normal((n_sys,) + x0.shape)).astype('f4')
    same = (0, 7, n_sys - 1)
    for s in same:
        x[s] = (x0 + 0.7 * np.random.default_rng(4).standard_normal(x0.shape)).astype('f4')
    rows = np.repeat(rows_of(specs)[None], n_sys, 0)
    n = len(specs)
    clocks = np.full(n_sys, 7, 'i8')
    for s in range(n_sys):
        if s not in same:      # the others pull harder, from elsewhere, and are further along
            rows[s, 3 * n:4 * n] *= np.float32(1. + 0.01 * s); rows[s, :n] += np.float32(0.001 * s) * rows[s, n:2 * n]; clocks[s] = s % 25
            rows[s, 2 * n:3 * n] += np.float32(0.001 * s) * rows[s, n:2 * n]
    path = steer_file(work, 'batch', specs, True)
    runs = []
    for rep in range(2):
        ens = E.Ensemble(path, n_sys)
        for s in range(n_sys):
            ens.set_param(rows[s], NODE, system=s)
        ens.set_steer_state(NODE, clock=clocks)
        ens.set_pos(x)
        e, d = ens.energies_and_derivs()
        runs.append((e, d, ens.steer_state(NODE)['center'], ens.steer_values(NODE)))
        assert all(np.array_equal(ens.get_param((5 * n,), NODE, system=s), rows[s]) for s in (0, 1, n_sys - 1))
        ens.close()
    assert all(a.tobytes() == b.tobytes() for a, b in zip(*runs)), 'two runs differ'
    e, d, c, v = runs[0]
    for s in same[1:]:
        assert all(a[s].tobytes() == a[0].tobytes() for a in (e, d, c, v)), 'system %d differs from system 0 at the same positions, rows and clock' % s
    assert all(e[s] != e[0] for s in range(n_sys) if s not in same)
    st = stored(specs)
    compare_energy(S.energy(st, x[0].astype('f8'), 7), float(e[0]), 'system 0 of %d' % n_sys)
    print('systems 0, 7 and %d of %d bit-identical in energy, derivative, centres and values; two runs bit-identical' % (n_sys - 1, n_sys))


# ---- 4. the accumulated work ------------------------------------------------------------------------------------------------------------
def md_specs():
    phi_q, phi_r, psi_q, psi_r = cfg.backbone_dihedrals(P.fixture(NAME))
    ca = np.arange(1, N_ATOM, 3, dtype='i4')
    specs = [{'name': 'd_ee', 'kind': 'distance', 'pair': (int(ca[0]), int(ca[-1]))},
             {'name': 'rg_ca', 'kind': 'rg', 'atoms': ca},
             {'name': 'psi10', 'kind': 'dihedral', 'atoms': psi_q[list(psi_r).index(10)]}]
    v = D.evaluate(specs, np.asarray(P.golden(NAME)['pos'], 'f8').reshape(-1, 3))
    for sp, val, k in zip(specs, v, (5., 10., 8.)):
        sp['center'] = r32(val); sp['rate'] = 0.; sp['center_end'] = sp['center']; sp['spring_const'] = k; sp['flat_width'] = 0.
    return specs, v


def md_rows(specs, n_sys, n_round=30):
    """per system its own pulling speed: system s moves every centre by (s + 1) / n_sys of (+3 A, -1 A, +1.5 rad) over n_round rounds"""
    n = len(specs)
    rows = np.repeat(rows_of(specs)[None], n_sys, 0)
    for s in range(n_sys):
        span = np.array([3., -1., 1.5]) * (s + 1) / n_sys
        rows[s, 2 * n:3 * n] = (rows[s, :n].astype('f8') + span).astype('f4')
        rows[s, n:2 * n] = ((rows[s, 2 * n:3 * n].astype('f8') - rows[s, :n].astype('f8')) / n_round).astype('f4')
    return rows


def work_of(series, rows, specs, t0=0):
    """(config.steer_work's last entry, the bound's scale) per system from a recorded series (n_round, n_sys, n_cv)"""
    n = len(specs)
    per = cfg.cv_periods(bare(specs))
    want, scale = [], []
    for s in range(series.shape[1]):
        cols = [rows[s, a * n:(a + 1) * n].astype('f8') for a in range(5)]
        want.append(cfg.steer_work(series[:, s], *cols, periods=per, t0=t0)[-1])
        sp = [dict(b, **dict((k, float(cols[a][c])) for a, k in enumerate(VALUES))) for c, b in enumerate(bare(specs))]
        scale.append(S.work_scale(sp, series[:, s].astype('f8'), t0))
        assert abs(S.work(sp, series[:, s].astype('f8'), t0)[-1] - want[-1]) <= 1e-13 * scale[-1]      # (the two restatements agree)
    return np.array(want), np.array(scale)


def work(work_dir):
    n_sys, n_round = 8, 40
    specs, v0 = md_specs()
    rows = md_rows(specs, n_sys)
    ens = E.Ensemble(steer_file(work_dir, 'work', specs, False), n_sys)
    for s in range(n_sys):
        ens.set_param(rows[s], NODE, system=s)
    ens.define_cvs(bare(specs))
    results = []
    for rep in range(2):
        ens.set_steer_state(NODE, clock=0, work=0.)
        ens.set_pos(P.golden(NAME)['pos'])
        ens.init_md(0.8, 11)
        ens.record_cvs(1, n_round)
        ens.run_rounds(n_round)
        series = ens.read_cvs()
        state = ens.steer_state(NODE)
        results.append((state['work'].copy(), series.copy(), ens.get_pos()))
        if rep:
            break
        assert series.shape == (n_round, n_sys, len(specs))
        want, scale = work_of(series, rows, specs)
        ratio = np.abs(state['work'] - want) / (1e-12 * scale)
        print('values at the start %s; T = 0.8, %d rounds, every system its own rates' % (np.round(v0, 4).tolist(), n_round))
        for s in range(n_sys):
            print('system %d: work on the device %.15g, steer_work of the recorded series %.15g, |difference| / bound %.3e (bound: 1e-12 x %.6g)' %
                  (s, state['work'][s], want[s], ratio[s], scale[s]))
        print('largest |difference| / bound %.3e; clocks %s' % (ratio.max(), state['clock'].tolist()))
        assert ratio.max() <= 1.
        assert state['clock'].tolist() == [n_round] * n_sys
        assert (state['work'] != 0.).all() and len(set(state['work'].tolist())) == n_sys
        for s in range(n_sys):
            assert np.array_equal(state['center'][s], cfg.steer_center(rows[s, 0:3].astype('f8'), rows[s, 3:6].astype('f8'), rows[s, 6:9].astype('f8'), n_round))
        # an fp32 accumulator or unrounded values would miss the bound by orders: the size of one float32 rounding of the total
        print('for scale: one float32 rounding of the work is %.1e of the bound' % (np.abs(state['work']).max() * 6e-8 / (1e-12 * scale.max())))
    ens.close()
    same = results[0][0].tobytes() == results[1][0].tobytes()
    print('after set_steer_state(clock=0, work=0) and the same seed: work bitwise the same %s, series %s, positions %s' %
          (same, results[0][1].tobytes() == results[1][1].tobytes(), results[0][2].tobytes() == results[1][2].tobytes()))
    assert same


# ---- 5. pulling holds -------------------------------------------------------------------------------------------------------------------
def pull(work_dir):
    n_sys = 8
    specs, v0 = md_specs()
    spec = dict(specs[0], spring_const=20.)
    d0 = spec['center']
    ends = np.array([r32(d0 + 8.)] * 4 + [r32(d0 - 4.)] * 4)
    ens = E.Ensemble(steer_file(work_dir, 'pull', [spec], False), n_sys)
    for s in range(n_sys):
        ens.set_param(np.array([d0, (ends[s] - d0) / 150., ends[s], 20., 0.], 'f4'), NODE, system=s)
    ens.define_cvs(bare([spec]))
    ens.set_pos(P.golden(NAME)['pos'])
    ens.init_md(0.8, 21)
    ens.run_rounds(150)
    mid = ens.steer_state(NODE)
    ens.run_rounds(50)
    v = ens.cvs()[:, 0].astype('f8')
    pos = ens.get_pos()
    state = ens.steer_state(NODE)
    ens.close()
    print('end-to-end distance at the start %.4f; spring_const 20, T = 0.8, 150 rounds of pulling and 50 at the end' % d0)
    print('ends    %s' % np.round(ends, 4).tolist())
    print('values  %s' % np.round(v, 4).tolist())
    print('centres after 150 rounds %s, after 200 %s' % (np.round(mid['center'][:, 0], 4).tolist(), np.round(state['center'][:, 0], 4).tolist()))
    print('work    %s' % np.round(state['work'], 4).tolist())
    own = np.abs(v - ends); other = np.abs(v - ends[::-1])
    assert np.isfinite(pos).all() and np.isfinite(v).all() and np.isfinite(state['work']).all()
    assert (own < other).all()
    assert np.array_equal(state['center'][:, 0], ends) and state['clock'].tolist() == [200] * n_sys
    assert np.array_equal(mid['work'], state['work'])      # a centre at rest does no work


# ---- 6. captured graph ------------------------------------------------------------------------------------------------------------------
def graph(work_dir):
    """run under UPSIDE_HIP_GRAPH=1 and =0 by the parent, which compares the two files this leaves"""
    g = os.environ.get('UPSIDE_HIP_GRAPH', 'x')
    print('UPSIDE_HIP_GRAPH=%s' % g)
    n_sys = 4
    specs, _ = md_specs()
    rows = md_rows(specs, n_sys)
    path = steer_file(work_dir, 'graph' + g, specs, False)
    runs = []
    for rep in range(2):
        ens = E.Ensemble(path, n_sys)
        for s in range(n_sys):
            ens.set_param(rows[s], NODE, system=s)
        ens.define_cvs(bare(specs))
        ens.set_pos(P.golden(NAME)['pos'])
        ens.init_md(0.8, 21)
        ens.record_cvs(1, 12)
        ens.run_rounds(6)
        first = ens.steer_state(NODE)
        ens.set_steer_state(NODE, clock=[3, 3, 20, 40], work=1.5)      # between two replays: back in time, and past the end
        ens.run_rounds(6)
        state = ens.steer_state(NODE)
        series = ens.read_cvs()
        runs.append([ens.get_pos(), ens.get_mom(), state['work'], state['clock'], state['center'], series])
        ens.close()
        if rep == 0:
            assert first['clock'].tolist() == [6] * n_sys and state['clock'].tolist() == [9, 9, 26, 46]
            w0, s0 = work_of(series[:6], rows, specs)
            want = []
            for s, t0 in enumerate((3, 3, 20, 40)):
                w, sc = work_of(series[6:, s:s + 1], rows[s:s + 1], specs, t0=t0)
                want.append((1.5 + w[0], sc[0] + 1.5))
            want = np.array(want)
            ratio = np.abs(state['work'] - want[:, 0]) / (1e-12 * want[:, 1])
            print('first six rounds: work %s (steer_work %s)' % (first['work'].tolist(), w0.tolist()))
            print('after set_steer_state(clock=[3, 3, 20, 40], work=1.5) and six more: work %s, steer_work %s, |difference| / bound %s' %
                  (state['work'].tolist(), want[:, 0].tolist(), np.round(ratio, 4).tolist()))
            assert (np.abs(first['work'] - w0) <= 1e-12 * s0).all() and ratio.max() <= 1.
            assert state['work'][3] == 1.5      # past the end the centre rests: no work
    a, b = runs
    assert all(np.isfinite(v).all() for v in a)
    same = all(u.tobytes() == v.tobytes() for u, v in zip(a, b))
    print('two runs of 12 rounds: positions, momenta, work, clocks, centres and the recorded series bit-identical: %s' % same)
    assert same
    np.savez(os.path.join(work_dir, 'graph%s.npz' % g), pos=a[0], mom=a[1], work=a[2], clock=a[3], center=a[4], series=a[5])


# ---- 7. upside_hip -----------------------------------------------------------------------------------------------------------------------
def run_cli(args):
    exe = os.path.join(P.ROOT, 'upside-md_amd', 'csrc', 'upside_hip')
    try:
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


def cli(work_dir):
    specs, _ = md_specs()
    rows = md_rows(specs, 2, n_round=15)
    n = len(specs)
    moving_specs = [dict(sp, **dict((k, float(rows[1, a * n + c])) for a, k in enumerate(VALUES))) for c, sp in enumerate(specs)]
    path = steer_file(work_dir, 'cli', moving_specs, False)
    cfg.add_collective_variables(path, bare(specs))
    # one frame per round (3 steps of 0.009); recentring moves the coordinates between a round's end and its frame and with them the
    # last bits of a CV, so it is switched off where the work is to be restated from /output/cv to 1e-12
    run_cli(['--duration', '0.54', '--frame-interval', '0.027', '--seed', '3', '--temperature', '0.8', '--disable-recentering', path])
    with pkg.h5lite.open_file(path) as f:
        out = f.group('output')
        assert 'cv_steer' in out.keys() and out.group('cv_steer').keys() == [NODE]
        g = out.group('cv_steer').group(NODE)
        assert sorted(g.keys()) == ['center', 'clock', 'work']
        wk, ck, cn = g.read('work'), g.read('clock'), g.read('center')
        cv = f.read('output/cv'); n_frame = f.read('output/pos', 'f4').shape[0]
    print('/output/cv_steer/%s: work %s %s, clock %s %s, center %s %s; %d frames' % (NODE, wk.shape, wk.dtype, ck.shape, ck.dtype, cn.shape, cn.dtype, n_frame))
    assert n_frame == 20 and wk.shape == (20,) and ck.shape == (20,) and cn.shape == (20, n) and cv.shape == (20, 1, n)
    assert wk.dtype == np.float64 and cn.dtype == np.float64 and ck.dtype.kind == 'i' and ck.tolist() == list(range(20))
    want_c = cfg.steer_center(rows[1, :n].astype('f8'), rows[1, n:2 * n].astype('f8'), rows[1, 2 * n:3 * n].astype('f8'), np.arange(20))
    assert np.array_equal(cn, want_c)
    want, scale = work_of(cv[1:], rows[1:2], specs)
    ratio = abs(wk[-1] - want[0]) / (1e-12 * scale[0])
    print('last work %.15g, steer_work of /output/cv %.15g, |difference| / bound %.3e' % (wk[-1], want[0], ratio))
    assert wk[0] == 0. and wk[-1] != 0. and ratio <= 1.
    # a file without the node keeps the /output it had
    plain = os.path.join(work_dir, 'plain.up')
    shutil.copyfile(P.fixture(NAME), plain)
    run_cli(['--duration', '0.054', '--frame-interval', '0.027', '--seed', '3', '--temperature', '0.8', plain])
    with pkg.h5lite.open_file(plain) as f:
        keys = f.group('output').keys()
    print('/output of a file without the node: %s' % sorted(keys))
    assert 'cv_steer' not in keys and 'pos' in keys


# ---- 8. refusals -----------------------------------------------------------------------------------------------------------------------
def refusals(work_dir):
    import hamiltonian_files as H
    x = K.perturbed(NAME).astype('f4')
    two = [{'name': 'rg', 'kind': 'rg', 'atoms': [0, 1, 2], 'center': 1., 'rate': 0.1, 'center_end': 2., 'spring_const': 1.},
           {'name': 'd', 'kind': 'distance', 'pair': (1, 4), 'center': 3., 'rate': -0.1, 'center_end': 1., 'spring_const': 2., 'flat_width': 0.1}]
    good_path = steer_file(work_dir, 'good', two, False)
    good = rows_of(two)

    def row(**change):
        r = dict((k, good[a * 2:(a + 1) * 2].copy()) for a, k in enumerate(VALUES))
        r.update((k, np.asarray(v, 'f4')) for k, v in change.items())
        return r
    cases = [
        ('short center', row(center=[1.]), ['center holds 1 entries', '2 CVs'], None),
        ('long rate', row(rate=[0.1, -0.1, 0.]), ['rate holds 3 entries'], None),
        ('empty center_end', row(center_end=[]), ['center_end holds 0 entries'], None),
        ('center not finite', row(center=[np.nan, 3.]), ['center of CV 0 is not finite'], True),
        ('rate not finite', row(rate=[0.1, -np.inf]), ['rate of CV 1 is not finite'], True),
        ('center_end not finite', row(center_end=[np.inf, 1.]), ['center_end of CV 0 is not finite'], True),
        ('spring_const not finite', row(spring_const=[1., np.nan]), ['spring_const of CV 1 is not finite'], True),
        ('flat_width not finite', row(flat_width=[np.inf, 0.]), ['flat_width of CV 0 is not finite'], True),
        ('negative spring_const', row(spring_const=[1., -2.]), ['spring_const of CV 1 must not be negative'], True),
        ('negative flat_width', row(flat_width=[-0.5, 0.]), ['flat_width of CV 0 must not be negative'], True),
        ('the end behind the start', row(rate=[-0.1, -0.1]), ['center_end of CV 0 lies behind center'], True),
        ('the end behind the start (2)', row(center_end=[2., 5.]), ['center_end of CV 1 lies behind center'], True),
        ('rate 0 with an end', row(rate=[0.1, 0.]), ['rate of CV 1 is 0 but center_end differs from center'], True),
    ]

    def good_engine():
        ens = E.Ensemble(good_path, 2)
        ens.set_pos(x)
        return ens
    ens = good_engine()
    e0 = ens.energies()
    assert np.isfinite(e0).all()
    for i, (what, r, needles, settable) in enumerate(cases):
        # at construction: the group written dataset by dataset, past the checks of config.add_cv_steer
        path = os.path.join(work_dir, 'bad_%d.up' % i)
        shutil.copyfile(good_path, path)
        for k in VALUES:
            H.rewrite(path, NODE, k, lambda v, k=k: r[k])
        try:
            E.Ensemble(path, 2)
        except RuntimeError as err:
            print('%-30s refused at construction: %s' % (what, err))
            for nd in needles:
                assert nd in str(err), (what, nd, str(err))
            assert NODE in str(err)
        else:
            raise AssertionError('%s: the node was constructed' % what)
        if not settable:      # (a dataset of another length is no row: a ladder takes it for a structural difference)
            os.remove(path)
            continue
        # as a system's row of a ladder: refused with the file's name
        try:
            E.Ensemble.from_files([good_path, path])
        except RuntimeError as err:
            assert os.path.basename(path) in str(err) and needles[0] in str(err), (what, str(err))
        else:
            raise AssertionError('%s: the ladder was accepted' % what)
        os.remove(path)
        flat = np.concatenate([r[k] for k in VALUES])
        for system in (None, 1):
            try:
                ens.set_param(flat, NODE, system=system)
            except RuntimeError as err:
                if system is None:
                    print('%-30s refused by set_param: %s' % ('', err))
                assert needles[0] in str(err), (what, str(err))
            else:
                raise AssertionError('%s: set_param(system=%r) accepted it' % (what, system))
            assert np.array_equal(ens.get_param((10,), NODE, system=1), good) and np.array_equal(ens.get_param((10,), NODE), good)
            assert ens.energies().tobytes() == e0.tobytes(), what + ': the earlier row is no longer in force'
    for system in (None, 1):      # a vector of the wrong length
        try:
            ens.set_param(good[:9], NODE, system=system)
        except RuntimeError as err:
            print('%-30s refused by set_param(system=%r): %s' % ('9 values', system, err))
            assert 'expected 10 values' in str(err) and 'got 9' in str(err)
        else:
            raise AssertionError('a row of 9 values was accepted')
    assert ens.energies().tobytes() == e0.tobytes()
    # steer_write: a negative clock, work that is not finite; the state stays
    ens.set_steer_state(NODE, clock=[2, 3], work=[0.5, -0.25])
    for what, kw, needle in (('negative clock', dict(clock=[1, -1]), 'clock of system 1 is negative'), ('NaN work', dict(work=[np.nan, 0.]), 'work of system 0 is not finite'),
                             ('infinite work', dict(clock=[1, 1], work=[0., np.inf]), 'work of system 1 is not finite')):
        try:
            ens.set_steer_state(NODE, **kw)
        except RuntimeError as err:
            print('%-30s refused: %s' % (what, err))
            assert needle in str(err)
        else:
            raise AssertionError(what + ' was accepted')
        state = ens.steer_state(NODE)
        assert state['clock'].tolist() == [2, 3] and state['work'].tolist() == [0.5, -0.25]
    # steer_* on a node that is no cv_steer, and on no node at all
    for node in ('rama_coord', 'no_such_node'):
        for what, call in (('steer_state', lambda: ens.steer_state(node)), ('set_steer_state', lambda: ens.set_steer_state(node, clock=0)), ('steer_values', lambda: ens.steer_values(node))):
            try:
                call()
            except RuntimeError as err:
                if what == 'steer_state':
                    print('%-30s refused: %s' % ('%s(%r)' % (what, node), err))
                assert node == 'no_such_node' or (node in str(err) and 'is not a cv_steer' in str(err))
            else:
                raise AssertionError('%s(%r) was served' % (what, node))
    # a ladder whose files differ in a dataset outside the five, or in the CV definition
    def add_sigma(p):      # a dataset the node does not know, as another bias's width would be
        with pkg.h5lite.open_file(p, 'r+') as t:
            t.group('input/potential/' + NODE).write('sigma', np.ones(2, 'f4'))
    for tag, fix, dataset in (('foreign', add_sigma, 'sigma'),
                              ('atoms', lambda p: H.rewrite(p, NODE, 'atoms', lambda v: v[::-1].copy()), 'atoms'),
                              ('beta', lambda p: H.rewrite(p, NODE, 'contact_beta', lambda v: v + 1.), 'contact_beta')):
        other = os.path.join(work_dir, 'other_%s.up' % tag)
        shutil.copyfile(good_path, other)
        fix(other)
        try:
            E.Ensemble.from_files([good_path, other])
        except RuntimeError as err:
            print('a ladder differing in %-12s refused: %s' % (dataset, err))
            assert os.path.basename(other) in str(err) and NODE in str(err) and dataset in str(err)
        else:
            raise AssertionError('a ladder differing in %s was accepted' % dataset)
    # a ladder differing in the five values is served, each system with its row
    slow = os.path.join(work_dir, 'slow.up')
    shutil.copyfile(good_path, slow)
    H.rewrite(slow, NODE, 'rate', lambda v: (0.5 * v).astype('f4'))
    H.rewrite(slow, NODE, 'spring_const', lambda v: (3. * v).astype('f4'))
    lad = E.Ensemble.from_files([good_path, slow])
    lad.set_pos(x)
    lad.set_steer_state(NODE, clock=4)
    el = lad.energies()
    want_row = good.copy(); want_row[2:4] *= np.float32(0.5); want_row[6:8] *= np.float32(3.)
    assert np.array_equal(lad.get_param((10,), NODE, system=1), want_row) and np.array_equal(lad.get_param((10,), NODE), good)
    assert np.array_equal(lad.steer_state(NODE)['center'], [cfg.steer_center(r[0:2].astype('f8'), r[2:4].astype('f8'), r[4:6].astype('f8'), 4) for r in (good, want_row)])
    lad.close()
    ens.close()
    ens = good_engine()      # the process is still usable
    e1 = ens.energies()
    ens.close()
    print('after every refusal a fresh engine gives the energies it gave: %s; a ladder of two speeds: energies %s' % (e1.tobytes() == e0.tobytes(), el.tolist()))
    assert e1.tobytes() == e0.tobytes() and np.isfinite(el).all() and el[0] != el[1]


CHECKS = dict(static=static, moving=moving_check, batch=batch, work=work, pull=pull, graph=graph, cli=cli, refusals=refusals)

if __name__ == '__main__':
    import torch
    assert torch.cuda.is_available(), 'these checks need a GPU'
    which, workdir = sys.argv[1], sys.argv[2]
    CHECKS[which](workdir)
    print('CHECK %s PASSED' % which)
