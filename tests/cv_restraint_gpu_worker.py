"""Child process of tests/test_gpu_cv_restraint.py: one check of the cv_restraint node per invocation,

    python tests/cv_restraint_gpu_worker.py CHECK WORKDIR

prints every figure it compares before it asserts and ends with 'CHECK <name> PASSED'.  The yardstick is
tests/cv_restraint_reference.py (float64 numpy, pinned by tests/test_cv_restraint_config.py).  Where the bias must be seen alone, the
check runs on a copy of a fixture whose other potential groups are deleted: energy and derivative are then the node's own."""
import json
import os
import shutil
import subprocess
import sys
import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import parity_util as P                  # noqa: E402
import cv_reference as R                 # noqa: E402
import cv_restraint_reference as Y       # noqa: E402
import cv_restraint_cases as K           # noqa: E402

pkg = P.pkg
cfg = pkg.config
E = pkg.engine
RTOL = P.RTOL
NODE = 'cv_restraint'
VALUES = ('center', 'spring_const', 'flat_width')
CLI_LIMIT = 240      # seconds for one upside_hip run; tests/test_gpu_cv_restraint.py gives the whole check 600


def rounded_to_file(specs):
    """the specs with every number rounded to the float32 the file holds: the yardstick sees the same definition"""
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


def isolated(work, name, specs, tag='iso', node=NODE):
    """a copy of the fixture with nothing under /input/potential but the restraint"""
    p = os.path.join(work, '%s.%s.up' % (name, tag))
    shutil.copyfile(P.fixture(name), p)
    with pkg.h5lite.open_file(p, 'r+') as t:
        pot = t.group('input/potential')
        for k in pot.keys():
            pkg.h5lite.Node.delete(pot, k)
    cfg.add_cv_restraint(p, specs, name=node)
    return p


def with_restraint(work, name, specs, tag='full'):
    p = os.path.join(work, '%s.%s.up' % (name, tag))
    shutil.copyfile(P.fixture(name), p)
    cfg.add_cv_restraint(p, specs)
    return p


def rows_of(specs):
    return np.concatenate([[np.float32(sp.get(k, 0.)) for sp in specs] for k in VALUES]).astype('f4')


def compare_deriv(ref, got, what):
    e1 = P.rel_rms(ref, got); e2 = P.max_rel_to_scale(ref, got)
    print('%-44s derivative: rel_rms %.3e (bound %.0e), largest element / scale %.3e (bound %.0e)' % (what, e1, RTOL, e2, 10 * RTOL))
    assert e1 <= RTOL and e2 <= 10 * RTOL, what
    return e1, e2


# ---- 1. forces and energies against the yardstick ------------------------------------------------------------------------------
def forces(work):
    for name in ('trpcage20_7A', 'syn300_10A'):
        x = K.perturbed(name)
        specs = K.force_specs(name, x)
        stored = rounded_to_file(specs)
        inside = K.inside_flat(stored, x)
        assert inside.any() and (~inside).any() and all(sp['spring_const'] > 0 for sp in specs)
        ens = E.Ensemble(isolated(work, name, specs), 1)
        ens.set_pos(x.astype('f4'))
        assert ens.get_pos()[0].astype('f8').tobytes() == x.tobytes()
        e, d = ens.energies_and_derivs()
        e = e.astype('f8')      # (a float32 scalar would round the yardstick's number to float32 in every difference below)
        v = ens.restraint_values(NODE)[0]
        e_ref, g_ref, v_ref = Y.energy_and_gradient(stored, x)
        print('%s: %d CVs (%s), %d inside their flat bottom' % (name, len(specs), ', '.join(sp['name'] for sp in specs), inside.sum()))
        print('%s: energy gpu %.9g, f64 %.9g, relative difference %.3e (bound 1e-6)' % (name, e[0], e_ref, abs(e[0] - e_ref) / abs(e_ref)))
        print('%s: largest relative difference of a CV value %.3e' % (name, np.abs(v - v_ref).max() / np.abs(v_ref).max()))
        assert abs(e[0] - e_ref) <= 1e-6 * abs(e_ref)
        compare_deriv(g_ref, d[0], name)
        assert np.abs(v - v_ref).max() <= RTOL * np.abs(v_ref).max()
        # each CV alone, through set_param: the others switched off by spring_const = 0
        full = rows_of(specs)
        n = len(specs)
        for c, sp in enumerate(stored):
            row = full.copy(); row[n:2 * n] = 0.; row[n + c] = full[n + c]
            ens.set_param(row, NODE)
            e1, d1 = ens.energies_and_derivs()
            e1 = e1.astype('f8')
            er, gr, _ = Y.energy_and_gradient([sp], x)
            if inside[c]:
                print('  %-10s inside its flat bottom: energy %r, largest |derivative| %r' % (sp['name'], float(e1[0]), float(np.abs(d1).max())))
                assert e1[0] == 0. and not d1.any(), sp['name']
            else:
                print('  %-10s energy gpu %.9g, f64 %.9g (%.1e)' % (sp['name'], e1[0], er, abs(e1[0] - er) / er))
                assert abs(e1[0] - er) <= 1e-6 * er, sp['name']
                compare_deriv(gr, d1[0], '  ' + sp['name'])
        assert np.array_equal(ens.get_param((3 * n,), NODE), row)
        ens.close()
    small_values(work)


def small_values(work):
    """an rg / rmsd / distance of 0 and a contact pair at r = 0: finite energy, zero force"""
    name = 'trpcage20_7A'
    specs = [dict(sp, center=2., spring_const=3.) for sp in (
        {'kind': 'rg', 'atoms': [0, 1, 2]}, {'kind': 'distance', 'pair': (3, 4)}, {'kind': 'rmsd', 'atoms': [5, 6, 7], 'ref': np.zeros((3, 3))},
        {'kind': 'contacts', 'pairs': [(8, 9)], 'r0': 1., 'beta': 5., 'lambda': 1.})]
    x = K.perturbed(name).astype('f4')
    x[:10] = (1., -2., 3.)
    ens = E.Ensemble(isolated(work, name, specs, 'small'), 1)
    ens.set_pos(x)
    e, d = ens.energies_and_derivs()
    e = e.astype('f8')
    e_ref = Y.energy(rounded_to_file(specs), x.astype('f8'))
    print('coincident atoms: values %s, energy gpu %.9g, f64 %.9g, largest |derivative| %r' % (ens.restraint_values(NODE)[0], e[0], e_ref, float(np.abs(d).max())))
    assert np.isfinite(e).all() and abs(e[0] - e_ref) <= 1e-6 * e_ref and not d.any()
    ens.close()


# ---- 2. the same bits as the CV kernel --------------------------------------------------------------------------------------------
def same_bits(work):
    for name in ('trpcage20_7A', 'syn300_10A'):
        x0 = K.perturbed(name)
        specs = K.force_specs(name, x0)
        path = isolated(work, name, specs)
        for n_sys in (1, 64):
            rng = np.random.default_rng(n_sys)
            x = (x0[None] + np.linspace(0., 2., n_sys)[:, None, None] * rng.standard_normal((n_sys,) + x0.shape)).astype('f4')
            ens = E.Ensemble(path, n_sys)
            ens.define_cvs(bare(specs))
            ens.set_pos(x)
            ens.energies()
            a = ens.restraint_values(NODE); b = ens.cvs()
            n_diff = int((a.view('u4') != b.view('u4')).sum())
            print('%s x %d: restraint_values against cvs(): %d of %d values differ in their bits' % (name, n_sys, n_diff, a.size))
            assert a.shape == b.shape == (n_sys, len(specs)) and a.tobytes() == b.tobytes()
            one = np.zeros(len(specs), 'f4')
            assert ens.calc.get_value_by_name(len(specs), one.ctypes.data, ens.engine, NODE.encode(), b'cv_value') == 0
            assert one.tobytes() == a[0].tobytes()
            ens.close()


# ---- 3. a ladder equals separate engines --------------------------------------------------------------------------------------------
def g56_specs():
    pos = K.coords('proteinG56_7A')
    ca = np.arange(1, len(pos), 3, dtype='i4')
    pairs, r0 = cfg.native_contacts(pos, ca)
    return [{'name': 'rmsd', 'kind': 'rmsd', 'atoms': ca, 'ref': pos[ca] + 0.8 * np.random.default_rng(5).standard_normal((len(ca), 3)), 'center': 1., 'spring_const': 4.},
            {'name': 'q', 'kind': 'contacts', 'pairs': pairs, 'r0': r0, 'beta': 5., 'lambda': 1.2, 'center': 0.5, 'spring_const': 300.}]


def g56_windows(work, n, tag='w'):
    base = with_restraint(work, 'proteinG56_7A', g56_specs(), tag + 'base')
    i = np.arange(n)
    centers = np.column_stack((0.5 + 0.25 * i, 0.95 - 0.05 * i)); ks = np.column_stack((4. + 0.5 * i, 300. - 10. * i)); ws = np.column_stack((0.02 * i, 0.003 * i))
    outs = cfg.write_umbrella_windows(base, [os.path.join(work, '%s%d.up' % (tag, k)) for k in i], NODE, centers, ks, ws)
    return base, outs


def ladder(work):
    n = 8
    base, fs = g56_windows(work, n)
    assert list(E.group_configurations(fs)) == [0] * n
    pos = (P.golden('proteinG56_7A')['pos'].astype('f8').reshape(-1, 3) + 0.3 * np.random.default_rng(1).standard_normal((168, 3))).astype('f4')
    big = E.Ensemble.from_files(fs)
    big.set_pos(pos)
    e, d = big.energies_and_derivs()
    print('energies of the 8 windows at one structure:', e)
    assert len(set(e.tolist())) == n
    for i, f in enumerate(fs):
        same = E.Ensemble(f, n)
        same.set_pos(pos)
        e8, d8 = same.energies_and_derivs()
        same.close()
        up = pkg.Upside(f)
        e1 = float(np.asarray(up.energy(pos)).ravel()[0]); d1 = up.deriv(pos)
        up.close()
        print('window %d: %.9g; 8 copies of its file: %.9g (bitwise %s); an engine of its own: %.9g (%.1e), derivative rel_rms %.1e'
              % (i, e[i], e8[i], e8[i] == e[i] and np.array_equal(d8[i], d[i]), e1, abs(e1 - float(e[i])) / max(1., abs(e1)), P.rel_rms(d1, d[i])))
        assert e8[i] == e[i] and np.array_equal(d8[i], d[i]), i
        assert abs(e1 - float(e[i])) <= 1e-6 * max(1., abs(e1)) and P.rel_rms(d1, d[i]) < 1e-6, i
    copies = E.Ensemble.from_files([fs[0]] * n)
    copies.set_pos(pos)
    for i in range(n):
        row = big.get_param((6,), NODE, system=i)
        copies.set_param(row, NODE, system=i)
        assert np.array_equal(copies.get_param((6,), NODE, system=i), row)
    ec, dc = copies.energies_and_derivs()
    print('set_param_system on copies of window 0 against the file ladder: bitwise %s' % (np.array_equal(ec, e) and np.array_equal(dc, d)))
    assert np.array_equal(ec, e) and np.array_equal(dc, d)
    copies.set_param(big.get_param((6,), NODE, system=3), NODE)      # set_param: every system
    ea = copies.energies()
    assert np.all(ea == e[3]), (ea, e[3])
    for bad in (np.zeros(5, 'f4'), np.zeros(7, 'f4')):
        try:
            copies.set_param(bad, NODE, system=1)
        except RuntimeError as err:
            assert 'expected 6 values' in str(err), str(err)
        else:
            raise AssertionError('a vector of %d values was accepted' % len(bad))
    assert np.all(copies.energies() == e[3])
    big.close(); copies.close()


# ---- 4. determinism and batch independence ----------------------------------------------------------------------------------------
def batch(work):
    name = 'syn300_10A'
    x0 = K.perturbed(name)
    specs = K.force_specs(name, x0)
    path = isolated(work, name, specs)
    base_row = rows_of(specs)
    n = len(specs)
    rng = np.random.default_rng(3)
    one = E.Ensemble(path, 1)
    for n_sys in (64, 600):
        x = (x0[None] + rng.standard_normal((n_sys,) + x0.shape)).astype('f4')
        win = np.repeat(base_row[None], n_sys, 0)
        win[:, :n] *= (1. + 0.002 * (np.arange(n_sys) % 11))[:, None]      # the windows differ too
        win[:, n:2 * n] *= (1. + 0.01 * (np.arange(n_sys) % 7))[:, None]
        for s in (0, 7, n_sys - 1):
            x[s] = x[0]; win[s] = win[0]
        runs = []
        for rep in range(2):
            ens = E.Ensemble(path, n_sys)
            for s in range(n_sys):
                ens.set_param(win[s], NODE, system=s)
            ens.set_pos(x)
            runs.append(ens.energies_and_derivs())
            ens.close()
        assert runs[0][0].tobytes() == runs[1][0].tobytes() and runs[0][1].tobytes() == runs[1][1].tobytes(), 'two runs of %d systems differ' % n_sys
        e, d = runs[0]
        for s in (7, n_sys - 1):
            assert e[s] == e[0] and d[s].tobytes() == d[0].tobytes(), 'system %d of %d differs from system 0 at the same positions' % (s, n_sys)
        worst = 0.
        for s in range(n_sys):
            one.set_param(win[s], NODE); one.set_pos(x[s])
            e1, d1 = one.energies_and_derivs()
            de = abs(float(e1[0]) - float(e[s]))
            worst = max(worst, P.rel_rms(d1[0], d[s]), de / max(1e-30, abs(float(e1[0]))))
            assert P.rel_rms(d1[0], d[s]) <= RTOL and de <= RTOL * abs(float(e1[0])), (n_sys, s)
        print('%d systems: two runs bit-identical; systems 0, 7 and %d bit-identical; largest deviation from a one-system engine %.3e (bound %.0e)'
              % (n_sys, n_sys - 1, worst, RTOL))
    one.close()


# ---- 5. MD ------------------------------------------------------------------------------------------------------------------------
def rg_ladder(work, tag, k=50.):
    name = 'trpcage20_7A'
    pos0 = P.golden(name)['pos'].astype('f8').reshape(-1, 3)
    ca = np.arange(1, len(pos0), 3, dtype='i4')
    rg0 = R.rg(pos0[ca])
    spec = {'name': 'rg_ca', 'kind': 'rg', 'atoms': ca, 'center': rg0, 'spring_const': k}
    base = with_restraint(work, name, [spec], tag + 'base')
    centers = np.array([0.7 * rg0] * 4 + [1.5 * rg0] * 4)
    fs = cfg.write_umbrella_windows(base, [os.path.join(work, '%s%d.up' % (tag, i)) for i in range(8)], NODE, centers)
    return fs, spec, rg0, pos0


def md_run(fs, spec, pos0, n_round=200):
    ens = E.Ensemble.from_files(fs) if fs is not None else E.Ensemble(P.fixture('trpcage20_7A'), 8)
    ens.set_pos(pos0.astype('f4'))
    ens.init_md(0.8, 21)
    ens.define_cvs(bare([spec]))
    ens.record_cvs(1, n_round)
    ens.run_rounds(n_round)
    series = ens.read_cvs()[:, :, 0]
    out = ens.get_pos(), ens.get_mom(), series
    ens.close()
    return out


def md(work):
    """run under UPSIDE_HIP_GRAPH=1 and =0 by the parent, which compares the two files this leaves"""
    print('UPSIDE_HIP_GRAPH=%s' % os.environ.get('UPSIDE_HIP_GRAPH'))
    fs, spec, rg0, pos0 = rg_ladder(work, 'md' + os.environ.get('UPSIDE_HIP_GRAPH', 'x'))
    pa, ma, sa = md_run(fs, spec, pos0)
    pb, mb, sb = md_run(fs, spec, pos0)
    assert np.isfinite(pa).all() and np.isfinite(ma).all() and np.isfinite(sa).all()
    means = sa[100:].astype('f8').mean(0)
    print('Rg of the CA atoms in the starting structure %.4f; centres %.4f (systems 0-3), %.4f (systems 4-7); k = 50, T = 0.8' % (rg0, 0.7 * rg0, 1.5 * rg0))
    print('mean Rg over rounds 101-200: low windows %s, high windows %s' % (np.round(means[:4], 4).tolist(), np.round(means[4:], 4).tolist()))
    print('MD_MEANS ' + json.dumps(dict(rg0=round(rg0, 4), centers=[round(0.7 * rg0, 4), round(1.5 * rg0, 4)], spring_const=50., temperature=0.8, rounds=200,
                                        mean_rg_low_windows=np.round(means[:4], 4).tolist(), mean_rg_high_windows=np.round(means[4:], 4).tolist())))      # (tools/cv_restraint_rate.py reads this line)
    assert pa.tobytes() == pb.tobytes() and ma.tobytes() == mb.tobytes() and sa.tobytes() == sb.tobytes(), 'two runs differ'
    assert means[:4].max() < means[4:].min(), means
    pf, mf, sf = md_run(None, spec, pos0)
    print('without the restraint: %s' % np.round(sf[100:].astype('f8').mean(0), 4).tolist())
    np.savez(os.path.join(work, 'md_graph%s.npz' % os.environ.get('UPSIDE_HIP_GRAPH', 'x')), pos=pa, mom=ma, series=sa, free_pos=pf, free_mom=mf)


# ---- 6. values rewritten in place under a captured graph ------------------------------------------------------------------------------
def inplace(work):
    fs, spec, rg0, pos0 = rg_ladder(work, 'ip')
    a = E.Ensemble.from_files(fs[:4]); b = E.Ensemble.from_files(fs[:4])
    for x in (a, b):
        x.set_pos(pos0.astype('f4')); x.init_md(0.8, 5); x.run_rounds(20)
    assert a.get_pos().tobytes() == b.get_pos().tobytes()
    row = a.get_param((3,), NODE, system=1); new = row.copy(); new[0] = np.float32(1.5 * rg0)
    a.set_param(new, NODE, system=1)
    e = a.energies()
    moved = os.path.join(work, 'ip_moved.up')
    cfg.write_umbrella_windows(fs[1], [moved], NODE, [[float(new[0])]])
    fresh = E.Ensemble.from_files([fs[0], moved, fs[2], fs[3]])
    fresh.set_pos(a.get_pos())
    ef = fresh.energies()
    eb = b.energies()
    print('after 20 rounds and set_param_system(1, centre %.4f -> %.4f): energies %s; a fresh engine built with that centre %s; before the move %s'
          % (row[0], new[0], e, ef, eb))
    assert np.array_equal(e, ef) and e[1] != eb[1] and np.array_equal(e[[0, 2, 3]], eb[[0, 2, 3]])
    a.run_rounds(10); b.run_rounds(10)
    pa, pb = a.get_pos(), b.get_pos()
    same = [pa[s].tobytes() == pb[s].tobytes() for s in range(4)]
    print('10 more rounds: systems whose trajectory equals the unmoved engine: %s' % same)
    assert same == [True, False, True, True]
    fresh.set_pos(pa)
    assert np.array_equal(a.energies(), fresh.energies())
    for x in (a, b, fresh):
        x.close()


# ---- 7. swap sets -----------------------------------------------------------------------------------------------------------------
def swap(work):
    import ctypes as ct
    n = 16
    pos = K.coords('proteinG56_7A')
    ca = np.arange(1, len(pos), 3, dtype='i4')
    pairs, r0 = cfg.native_contacts(pos, ca)
    base = with_restraint(work, 'proteinG56_7A', [{'name': 'q', 'kind': 'contacts', 'pairs': pairs, 'r0': r0, 'beta': 5., 'lambda': 1.8, 'center': 0.9, 'spring_const': 200.}], 'qbase')
    fs = cfg.write_umbrella_windows(base, [os.path.join(work, 'q%d.up' % i) for i in range(n)], NODE, np.linspace(0.95, 0.5, n))
    temps = np.linspace(0.80, 0.90, n).astype('f4')
    lib = pkg.default_library(); c = lib.calc
    E.Ensemble._bind(c)
    c.upside_hip_swap_between.argtypes = [ct.c_void_p, ct.c_int, ct.c_void_p, ct.c_int]
    c.upside_replica_decide_lboltz.argtypes = [ct.c_int, ct.c_void_p, ct.c_uint32, ct.c_uint64, ct.c_int, ct.c_void_p]
    dev = E.Ensemble.from_files(fs, library=lib); host = E.Ensemble.from_files(fs, library=lib)
    for x in (dev, host):
        x.set_pos(P.golden('proteinG56_7A')['pos'])
        x.init_md(temps, 17)
    sets = [np.array([[i, i + 1] for i in range(0, n, 2)]), np.array([[i, i + 1] for i in range(1, n - 1, 2)])]
    dev.run_steps(30)
    host.set_pos(dev.get_pos())
    draw = 0
    for k, st in enumerate(sets):
        acc, nxt = dev.hamiltonian_swap(st, 101, 1, draw0=draw, want_accepted=True)
        old = -(1. / temps) * host.energies()
        for a, b in st:
            assert c.upside_hip_swap_between(host.engine, int(a), host.engine, int(b)) == 0
        new = -(1. / temps) * host.energies()
        diff = np.array([(new[a] + new[b]) - (old[a] + old[b]) for a, b in st], 'f4')
        href = np.zeros(len(st) + 1, 'i4')
        assert c.upside_replica_decide_lboltz(len(st), diff.ctypes.data, 101, 1, draw, href.ctypes.data) == 0
        for p, (a, b) in enumerate(st):
            if not href[p]:
                assert c.upside_hip_swap_between(host.engine, int(a), host.engine, int(b)) == 0
        print('swap set %d: log-Boltzmann differences %s; device verdicts %s, host verdicts %s' % (k, np.round(diff, 3).tolist(), acc.astype(int).tolist(), href[:-1].tolist()))
        assert np.array_equal(acc, href[:-1].astype(bool)) and nxt == href[-1]
        assert np.array_equal(dev.get_pos(), host.get_pos())
        draw = nxt
    dev.close(); host.close()


# ---- 8. upside_hip on window files --------------------------------------------------------------------------------------------------
def cli(work):
    exe = os.path.join(P.ROOT, 'upside-md_amd', 'csrc', 'upside_hip')
    base, fs = g56_windows(work, 4, 'c')
    args = ['--duration', '0.27', '--frame-interval', '0.054', '--seed', '3', '--temperature', '0.80,0.82,0.84,0.86', '--replica-interval', '0.055',
            '--swap-set', '0-1,2-3', '--swap-set', '1-2']
    try:      # a limit well inside the parent's: the run is over (killed by subprocess.run) before the parent gives up on this process
        r = subprocess.run([exe] + args + fs, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=CLI_LIMIT)
    except subprocess.TimeoutExpired as err:
        print((err.stdout or b'').decode()[-3000:])
        print('upside_hip did not finish in %d s' % CLI_LIMIT)
        sys.exit(124)      # a hang: the parent starts nothing more
    if r.returncode:
        print(r.stdout.decode()[-3000:])
        if r.returncode < 0 or r.returncode > 1:
            sys.exit(r.returncode if r.returncode > 0 else 128 - r.returncode)      # a signal: the parent starts nothing more
        raise AssertionError('upside_hip failed')
    res = []
    for f in fs:
        with pkg.h5lite.open_file(f) as t:
            out = t.group('output')
            keys = out.keys()
            assert 'replica_index' in keys and 'potential' in keys and 'pos' in keys, keys
            res.append((out.read('potential'), out.read('replica_index'), out.read('pos', 'f4')))
    # the initial structure as the run saw it: frame 0 is written after the recentring, before the first step and the first swap
    ens = E.Ensemble.from_files(fs)
    ens.set_pos(np.stack([r[2][0, 0] for r in res]))
    want = ens.energies()
    ens.close()
    for i, f in enumerate(fs):
        pot, ri, _ = res[i]
        print('%s: %d frames, replica_index %s, potential of frame 0 %.9g, from_files at the initial structure %.9g' %
              (os.path.basename(f), len(pot), ri.ravel().tolist(), pot.ravel()[0], want[i]))
        assert abs(float(pot.ravel()[0]) - float(want[i])) <= 1e-6 * max(1., abs(float(want[i]))) and len(pot) >= 5
    assert len(set(np.round(want, 4).tolist())) == 4


# ---- 9. refusals --------------------------------------------------------------------------------------------------------------------
def write_raw(work, tag, p, name='trpcage20_7A'):
    """a restraint group written dataset by dataset, past the checks of config.add_cv_restraint"""
    path = os.path.join(work, 'bad_%s.up' % tag)
    shutil.copyfile(P.fixture(name), path)
    with pkg.h5lite.open_file(path, 'r+') as t:
        g = t.group('input/potential').create_group(NODE)
        g.set_attr('arguments', ['pos'])
        for k, v in p.items():
            g.write(k, v)
    return path


def refusals(work):
    name = 'trpcage20_7A'
    n_atom = 60

    def packed(kind, lists, ref=(), r0=(), **values):
        n = len(kind)
        start = np.concatenate(([0], np.cumsum([len(l) for l in lists]))).astype('i4')
        p = dict(kind=np.asarray(kind, 'i4'), atom_start=start, atoms=np.concatenate([np.asarray(l, 'i4') for l in lists]),
                 ref_pos=np.asarray(ref, 'f4').reshape(-1, 3), contact_r0=np.asarray(r0, 'f4'), contact_beta=np.full(n, 5., 'f4'),
                 contact_lambda=np.full(n, 1.8, 'f4'), center=np.ones(n, 'f4'), spring_const=np.ones(n, 'f4'), flat_width=np.zeros(n, 'f4'))
        p.update((k, np.asarray(v, 'f4')) for k, v in values.items())
        return p

    good = packed([0, 3], [[0, 1, 2], [1, 4]])
    cases = [
        ('unknown kind', packed([0, 7], [[0, 1], [1, 2]]), ['unknown kind 7']),
        ('atom out of range', packed([0], [[0, n_atom]]), ['out of range', 'atom %d' % n_atom]),
        ('rmsd under 3 atoms', packed([1], [[0, 1]], ref=np.zeros((2, 3))), ['at least 3 atoms']),
        ('distance of 3 atoms', packed([3], [[0, 5, 6]]), ['exactly 2 atoms']),
        ('odd contacts list', packed([2], [[0, 5, 9]], r0=[5.]), ['even']),
        ('65 CVs', packed([3] * 65, [[0, 1]] * 65), ['limit of 64']),
        ('a list of 2^24 + 2 entries', packed([0], [np.zeros((1 << 24) + 2, 'i4')]), ['limit of 16777216']),
        ('short center', packed([0, 3], [[0, 1, 2], [1, 4]], center=[1.]), ['center holds 1 entries', '2 CVs']),
        ('long spring_const', packed([0, 3], [[0, 1, 2], [1, 4]], spring_const=[1., 1., 1.]), ['spring_const holds 3 entries']),
        ('short flat_width', packed([0, 3], [[0, 1, 2], [1, 4]], flat_width=[]), ['flat_width holds 0 entries']),
        ('negative spring_const', packed([0, 3], [[0, 1, 2], [1, 4]], spring_const=[1., -2.]), ['spring_const of CV 1 must be finite and not negative']),
        ('spring_const not finite', packed([0, 3], [[0, 1, 2], [1, 4]], spring_const=[np.inf, 1.]), ['spring_const of CV 0 must be finite and not negative']),
        ('negative flat_width', packed([0, 3], [[0, 1, 2], [1, 4]], flat_width=[-0.5, 0.]), ['flat_width of CV 0 must be finite and not negative']),
        ('flat_width not finite', packed([0, 3], [[0, 1, 2], [1, 4]], flat_width=[0., np.nan]), ['flat_width of CV 1 must be finite and not negative']),
    ]
    good_path = write_raw(work, 'good', good)
    x = K.perturbed(name).astype('f4')

    def good_energy():
        ens = E.Ensemble(good_path, 2)
        ens.set_pos(x)
        e = ens.energies()
        ens.close()
        return e
    e0 = good_energy()
    assert np.isfinite(e0).all() and e0[0] > 0.
    for i, (what, p, needles) in enumerate(cases):
        path = write_raw(work, str(i), p)
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
    # a ladder whose files differ in the definition
    import hamiltonian_files as H
    other = os.path.join(work, 'other_atoms.up')
    shutil.copyfile(good_path, other)
    H.rewrite(other, NODE, 'atoms', lambda v: v[::-1].copy())
    try:
        E.Ensemble.from_files([good_path, other])
    except RuntimeError as err:
        print('a ladder differing in atoms refused: %s' % err)
        assert 'other_atoms.up' in str(err) and NODE in str(err) and 'atoms' in str(err)
    else:
        raise AssertionError('a ladder differing in atoms was accepted')
    # per-system values of a bad window file are refused with the file's name
    badw = os.path.join(work, 'bad_window.up')
    shutil.copyfile(good_path, badw)
    H.rewrite(badw, NODE, 'spring_const', lambda v: -v)
    try:
        E.Ensemble.from_files([good_path, badw])
    except RuntimeError as err:
        print('a window with a negative spring_const refused: %s' % err)
        assert 'bad_window.up' in str(err) and 'spring_const' in str(err)
    else:
        raise AssertionError('a window with a negative spring_const was accepted')
    assert np.array_equal(good_energy(), e0)


CHECKS = dict(forces=forces, same_bits=same_bits, ladder=ladder, batch=batch, md=md, inplace=inplace, swap=swap, cli=cli, refusals=refusals)

if __name__ == '__main__':
    import torch
    assert torch.cuda.is_available(), 'these checks need a GPU'
    which, workdir = sys.argv[1], sys.argv[2]
    CHECKS[which](workdir)
    print('CHECK %s PASSED' % which)
