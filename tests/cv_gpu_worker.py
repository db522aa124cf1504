"""Child process of tests/test_gpu_cv.py: one check of the collective variables per invocation,

    python tests/cv_gpu_worker.py CHECK WORKDIR

prints every figure it compares before it asserts and ends with 'CHECK <name> PASSED'.  The yardstick is tests/cv_reference.py
(float64 numpy, RMSD by SVD).  Bound on every value: |gpu - float64| <= parity_util.RTOL x max(|value|, scale), scale = the Rg of
the reference structure for the length-valued CVs and 1 for Q."""
import os
import shutil
import subprocess
import sys
import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import parity_util as P      # noqa: E402
import cv_reference as R     # noqa: E402

pkg = P.pkg
cfg = pkg.config
RTOL = P.RTOL
FIXTURES = ['proteinG56_7A', 'syn300_10A', 'trpcage20_7A']


def fixture_specs(name):
    """the CVs of the checks: the four kinds over the CA atoms, and Rg / RMSD / a bonded distance over all atoms"""
    pos0 = cfg.read_pos(P.fixture(name)).astype('f8')
    ca = np.arange(1, len(pos0), 3, dtype='i4')
    pairs, r0 = cfg.native_contacts(pos0, ca, 8.0, 4)
    assert len(pairs) > 0
    specs = [{'name': 'rg_ca', 'kind': 'rg', 'atoms': ca},
             {'name': 'rmsd_ca', 'kind': 'rmsd', 'atoms': ca, 'ref': pos0[ca]},
             {'name': 'q', 'kind': 'contacts', 'pairs': pairs, 'r0': r0, 'beta': 5., 'lambda': 1.8},
             {'name': 'end_to_end', 'kind': 'distance', 'pair': (int(ca[0]), int(ca[-1]))},
             {'name': 'rg_all', 'kind': 'rg', 'atoms': np.arange(len(pos0), dtype='i4')},
             {'name': 'rmsd_all', 'kind': 'rmsd', 'atoms': np.arange(len(pos0), dtype='i4'), 'ref': pos0},
             {'name': 'bond', 'kind': 'distance', 'pair': (0, 1)}]
    return pos0, specs


def specs_as_stored(specs):
    """the specs with ref and r0 rounded to the float32 the engine is given: the yardstick sees the same definition"""
    out = []
    for sp in specs:
        sp = dict(sp)
        if 'ref' in sp:
            sp['ref'] = np.asarray(sp['ref'], 'f4').astype('f8')
        if 'r0' in sp:
            sp['r0'] = np.asarray(sp['r0'], 'f4').astype('f8')
        out.append(sp)
    return out


def scales(specs, pos0):
    rg_ref = R.rg(pos0[np.arange(1, len(pos0), 3)])
    return np.array([1. if sp['kind'] == 'contacts' else rg_ref for sp in specs])


def check_values(gpu, x32, specs, pos0, what):
    """gpu (n_sys, n_cv) against the yardstick at the float32 positions x32 (n_sys, n_atom, 3); prints the largest ratio per kind"""
    stored = specs_as_stored(specs)
    ref = np.array([R.evaluate(stored, x) for x in x32.astype('f8')])
    sc = scales(specs, pos0)
    assert np.isfinite(gpu).all(), (what, 'a value is not finite')
    ratio = np.abs(gpu.astype('f8') - ref) / (RTOL * np.maximum(np.abs(ref), sc[None]))
    for kind in ('rg', 'rmsd', 'contacts', 'distance'):
        cols = [c for c, sp in enumerate(specs) if sp['kind'] == kind]
        r = ratio[:, cols]
        s, c = np.unravel_index(np.argmax(r), r.shape)
        print('%-34s %-9s largest |gpu - f64| / bound = %.3e  (system %d, %s: gpu %.9g, f64 %.9g)' %
              (what, kind, r.max(), s, specs[cols[c]]['name'], gpu[s, cols[c]], ref[s, cols[c]]))
    assert ratio.max() <= 1., (what, 'largest ratio', ratio.max())
    return ref


# ---- values ---------------------------------------------------------------------------------------------------------
def stressed_positions(name, pos0, specs, n_sys=64):
    rng = np.random.default_rng({'proteinG56_7A': 11, 'syn300_10A': 12, 'trpcage20_7A': 13}[name])
    x = np.repeat(pos0[None], n_sys, 0)
    amp = np.linspace(0., 3., n_sys - 2)
    x[:n_sys - 2] += amp[:, None, None] * rng.standard_normal((n_sys - 2,) + pos0.shape)
    # an exact rigid motion of the reference
    x[n_sys - 2] = pos0 @ R.random_rotation(rng).T + np.array([13., -21., 34.])
    # a contact pair stretched to 900 Angstrom
    a, b = specs[2]['pairs'][0]
    x[n_sys - 1, b] = x[n_sys - 1, a] + np.array([900., 0., 0.])
    return x.astype('f4'), n_sys - 2, n_sys - 1


def values(work):
    for name in FIXTURES:
        pos0, specs = fixture_specs(name)
        x, i_rigid, i_far = stressed_positions(name, pos0, specs)
        ens = pkg.engine.BatchEngine(P.fixture(name), 64)
        ens.define_cvs(specs)
        assert ens.n_cv == len(specs) and ens.cv_names == [sp['name'] for sp in specs]
        ens.set_pos(x)
        gpu = ens.cvs()
        x_dev = ens.get_pos()
        assert x_dev.tobytes() == x.tobytes()
        ref = check_values(gpu, x_dev, specs, pos0, name)
        rg_ref = R.rg(pos0[np.arange(1, len(pos0), 3)])
        print('%s: rigid-motion system: rmsd_ca gpu %.3e, f64 %.3e (Rg %.3f: an fp32 accumulation would leave ~%.1e); identical system: rmsd_ca gpu %.3e'
              % (name, gpu[i_rigid, 1], ref[i_rigid, 1], rg_ref, 3e-4 * rg_ref, gpu[0, 1]))
        assert gpu[i_rigid, 1] <= RTOL * rg_ref and gpu[0, 1] <= RTOL * rg_ref and gpu[0, 5] <= RTOL * rg_ref
        d = float(np.sqrt(((x_dev[i_far, specs[2]['pairs'][0][0]].astype('f8') - x_dev[i_far, specs[2]['pairs'][0][1]].astype('f8')) ** 2).sum()))
        print('%s: stretched system: pair at %.1f A, Q gpu %.9g, f64 %.9g' % (name, d, gpu[i_far, 2], ref[i_far, 2]))
        assert abs(d - 900.) < 1e-3 and np.isfinite(gpu[i_far]).all()
        # one pair alone, 900 A apart: exactly 0
        ens.define_cvs([{'kind': 'contacts', 'pairs': [specs[2]['pairs'][0]], 'r0': [float(specs[2]['r0'][0])], 'beta': 5., 'lambda': 1.8}])
        q = ens.cvs()
        print('%s: the stretched pair alone: Q = %r (bound pair at the reference: %.6f)' % (name, float(q[i_far, 0]), q[0, 0]))
        assert q[i_far, 0] == 0. and q.shape == (64, 1) and q[0, 0] > 0.9
        ens.define_cvs([])
        assert ens.n_cv == 0
        try:
            ens.cvs()
        except RuntimeError as err:
            assert 'no collective variables defined' in str(err)
        else:
            raise AssertionError('cvs() without a definition did not raise')
        ens.close()


# ---- batch independence -----------------------------------------------------------------------------------------------
def batch(work):
    for name in FIXTURES:
        pos0, specs = fixture_specs(name)
        rng = np.random.default_rng(3)
        special = (pos0 + 0.7 * rng.standard_normal(pos0.shape)).astype('f4')
        rows = {}
        for n_sys in (64, 600):
            x = (pos0[None] + rng.standard_normal((n_sys,) + pos0.shape)).astype('f4')
            for s in (0, 7, n_sys - 1):
                x[s] = special
            runs = []
            for rep in range(2):
                ens = pkg.engine.BatchEngine(P.fixture(name), n_sys)
                ens.define_cvs(specs); ens.set_pos(x)
                runs.append(ens.cvs())
                ens.close()
            assert runs[0].tobytes() == runs[1].tobytes(), '%s: two runs of %d systems differ' % (name, n_sys)
            for s in (7, n_sys - 1):
                assert runs[0][s].tobytes() == runs[0][0].tobytes(), '%s: system %d of %d differs from system 0 at the same positions' % (name, s, n_sys)
            others = [s for s in range(n_sys) if s not in (0, 7, n_sys - 1)]
            assert all(runs[0][s].tobytes() != runs[0][0].tobytes() for s in others)
            check_values(runs[0], x, specs, pos0, '%s x %d' % (name, n_sys))
            rows[n_sys] = runs[0][0]
        assert rows[64].tobytes() == rows[600].tobytes(), '%s: the row depends on the batch size' % name
        print('%s: systems 0, 7 and the last of 64 and of 600 bit-identical, two runs bit-identical, 64 == 600: %s' % (name, rows[64]))


# ---- recording --------------------------------------------------------------------------------------------------------
def md_engine(name, specs, n_sys=8, seed=9):
    ens = pkg.engine.BatchEngine(P.fixture(name), n_sys)
    ens.set_pos(P.golden(name)['pos'])
    ens.init_md(np.linspace(0.7, 0.9, n_sys), seed)
    if specs is not None:
        ens.define_cvs(specs)
    return ens


def record(work):
    """runs under UPSIDE_HIP_GRAPH=0 and =1 (set by the parent): value identity, trajectory identity, overflow"""
    print('UPSIDE_HIP_GRAPH=%s' % os.environ.get('UPSIDE_HIP_GRAPH'))
    assert os.environ.get('UPSIDE_HIP_GRAPH') in ('0', '1')
    for name in FIXTURES:
        pos0, specs = fixture_specs(name)
        a = md_engine(name, specs)
        a.record_cvs(5, 64)
        a.run_rounds(200)
        series, n_stored, n_attempted = a.read_cvs(reset=False, with_counts=True)
        print('%s: %d samples stored, %d attempted, shape %s' % (name, n_stored, n_attempted, series.shape))
        assert series.shape == (40, 8, len(specs)) and n_stored == 40 and n_attempted == 40
        assert np.isfinite(series).all() and np.abs(series[-1] - series[0]).max() > 1e-3, 'the series does not move'
        pa, ma = a.get_pos(), a.get_mom()
        check_values(series[-1], pa, specs, pos0, name + ' last sample')
        # reading again gives the same; reset empties the buffer and the phase runs on
        again = a.read_cvs(reset=True)
        assert again.tobytes() == series.tobytes()
        assert a.cv_counts() == (0, 0)
        a.run_rounds(7)
        assert a.cv_counts() == (1, 1)      # rounds 201..207 since the call: round 205 is due
        a.record_cvs(0)
        try:
            a.read_cvs()
        except RuntimeError as err:
            assert 'not being recorded' in str(err)
        else:
            raise AssertionError('read_cvs after record_cvs(0) did not raise')
        a.close()

        b = md_engine(name, specs)
        manual = []
        for k in range(40):
            b.run_rounds(5)
            manual.append(b.cvs())
        manual = np.array(manual)
        pb, mb = b.get_pos(), b.get_mom()
        b.close()
        n_diff = int((manual.view('u4') != series.view('u4')).sum())
        print('%s: recorded series against run_rounds(5) + cvs() x 40: %d of %d values differ in their bits' % (name, n_diff, series.size))
        assert manual.tobytes() == series.tobytes(), name + ': recorded and computed series differ'

        c = md_engine(name, None)
        c.run_rounds(200)
        pc, mc = c.get_pos(), c.get_mom()
        c.close()
        print('%s: final positions / momenta against an engine without CVs: max |diff| %.3e / %.3e; against the run_rounds(5) engine: %.3e / %.3e'
              % (name, np.abs(pa - pc).max(), np.abs(ma - mc).max(), np.abs(pb - pc).max(), np.abs(mb - mc).max()))
        assert pa.tobytes() == pc.tobytes() and ma.tobytes() == mc.tobytes(), name + ': recording changed the trajectory'

        # overflow: a full buffer stops storing and keeps counting
        d = md_engine(name, specs)
        d.record_cvs(5, 10)
        d.run_rounds(200)
        short, n_stored, n_attempted = d.read_cvs(with_counts=True)
        d.close()
        print('%s: capacity 10: %d stored, %d attempted' % (name, n_stored, n_attempted))
        assert n_stored == 10 and n_attempted == 40 and short.tobytes() == series[:10].tobytes()


# ---- slots under exchange ---------------------------------------------------------------------------------------------
def slots(work):
    for name in FIXTURES:
        pos0, specs = fixture_specs(name)
        a = md_engine(name, specs); b = md_engine(name, specs)
        a.record_cvs(1, 8)
        a.run_rounds(3); b.run_rounds(3)
        before = b.cvs()
        a.swap_systems(1, 2); b.swap_systems(1, 2)
        after = b.cvs()
        assert after[1].tobytes() == before[2].tobytes() and after[2].tobytes() == before[1].tobytes() and after[0].tobytes() == before[0].tobytes()
        assert before[1].tobytes() != before[2].tobytes()
        a.run_rounds(1); b.run_rounds(1)
        want = b.cvs()
        series = a.read_cvs()
        assert series.shape[0] == 4
        print('%s: sample after swap_systems(1, 2): slots 1, 2 = %s, %s; cvs() of the traded coordinates one round on: %s, %s'
              % (name, series[3, 1, :3], series[3, 2, :3], want[1, :3], want[2, :3]))
        assert series[3].tobytes() == want.tobytes()
        assert series[2].tobytes() == before.tobytes()
        a.close(); b.close()


# ---- upside_hip -------------------------------------------------------------------------------------------------------
def cli(work):
    exe = os.path.join(P.ROOT, 'upside-md_amd', 'csrc', 'upside_hip')
    base = ['--duration', '0.27', '--frame-interval', '0.054', '--seed', '3']
    for name in FIXTURES:
        pos0 = cfg.read_pos(P.fixture(name)).astype('f8')
        with_cv = os.path.join(work, name + '.cv.up'); with_cv2 = os.path.join(work, name + '.cv2.up'); without = os.path.join(work, name + '.plain.up')
        for p in (with_cv, with_cv2, without):
            shutil.copyfile(P.fixture(name), p)
        specs = cfg.default_collective_variables(pos0)
        for p in (with_cv, with_cv2):
            cfg.add_collective_variables(p, specs)
        for files in ([with_cv], [without], [with_cv, with_cv2]):
            args = base + ['--temperature', ','.join(['0.8', '0.85'][:len(files)])]
            r = subprocess.run([exe] + args + files, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
            if r.returncode:
                print(r.stdout.decode()[-3000:])
                if r.returncode < 0 or r.returncode > 1:
                    sys.exit(r.returncode if r.returncode > 0 else 128 - r.returncode)      # a signal: the parent starts nothing more
                raise AssertionError('upside_hip failed on %s' % files)
        with pkg.h5lite.open_file(without) as f:
            keys = f.group('output').keys()
            assert 'cv' not in keys and 'pos' in keys and not f.has_attr('cv_names', 'output'), keys
        print('%s without the group: /output has %s' % (name, sorted(keys)))
        for p in (with_cv, with_cv2):
            with pkg.h5lite.open_file(p) as f:
                pos = f.read('output/pos', 'f4'); cv = f.read('output/cv')
                names = f.get_attr('cv_names', 'output'); names_d = f.get_attr('names', 'output/cv')
            print('%s: /output/pos %s, /output/cv %s %s, names %s' % (os.path.basename(p), pos.shape, cv.shape, cv.dtype, names))
            assert cv.dtype == np.float32 and cv.shape == (pos.shape[0], 1, len(specs)) and pos.shape[0] >= 5
            assert list(names) == [sp['name'] for sp in specs] == list(names_d)
            check_values(cv[:, 0], pos[:, 0], specs, pos0, os.path.basename(p))
            assert np.abs(cv[-1] - cv[0]).max() > 1e-3


# ---- refusals ---------------------------------------------------------------------------------------------------------
def refusals(work):
    name = 'trpcage20_7A'
    pos0, specs = fixture_specs(name)
    n_atom = len(pos0)
    ens = pkg.engine.BatchEngine(P.fixture(name), 4)
    ens.set_pos((pos0[None] + 0.5 * np.random.default_rng(2).standard_normal((4,) + pos0.shape)).astype('f4'))
    ens.define_cvs(specs)
    good = ens.cvs()

    def packed(kind, lists, ref=(), r0=(), beta=None, lam=None):
        start = np.concatenate(([0], np.cumsum([len(l) for l in lists]))).astype('i4')
        return dict(kind=np.asarray(kind, 'i4'), atom_start=start, atoms=np.concatenate([np.asarray(l, 'i4') for l in lists]) if len(start) > 1 and start[-1] else np.zeros(0, 'i4'),
                    ref_pos=np.asarray(ref, 'f4').reshape(-1, 3), contact_r0=np.asarray(r0, 'f4'),
                    contact_beta=np.full(len(kind), 5., 'f4') if beta is None else beta, contact_lambda=np.full(len(kind), 1.8, 'f4') if lam is None else lam,
                    names=['c%d' % i for i in range(len(kind))])

    cases = [
        ('unknown kind', packed([0, 7], [[0, 1], [1, 2]]), ['unknown kind 7', 'collective variable 1']),
        ('atom out of range', packed([0], [[0, n_atom]]), ['out of range', 'atom %d' % n_atom]),
        ('negative atom', packed([3], [[-1, 2]]), ['out of range']),
        ('empty selection', packed([0, 0], [[0, 1], []]), ['empty selection', 'collective variable 1']),
        ('rmsd under 3 atoms', packed([1], [[0, 1]], ref=np.zeros((2, 3))), ['at least 3 atoms']),
        ('odd contacts list', packed([2], [[0, 5, 9]], r0=[5.]), ['even']),
        ('r0 = 0', packed([2], [[0, 5, 1, 9]], r0=[5., 0.]), ['r0 must be positive']),
        ('r0 < 0', packed([2], [[0, 5]], r0=[-1.]), ['r0 must be positive']),
        ('distance of 3 atoms', packed([3], [[0, 5, 6]]), ['exactly 2 atoms']),
        ('65 CVs', packed([3] * 65, [[0, 1]] * 65), ['limit of 64', 'UPK_CV_MAX']),
        ('a list of 2^24 + 2 entries', packed([0], [np.zeros((1 << 24) + 2, 'i4')]), ['limit of 16777216', 'UPK_CV_MAX_LIST']),
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
        assert ens.n_cv == len(specs)
        now = ens.cvs()
        assert now.tobytes() == good.tobytes(), what + ': the previous definition is no longer in force'
    # recording needs a definition and a capacity; a bad file is refused by load_cvs
    try:
        ens.record_cvs(5, 0)
    except RuntimeError as err:
        assert 'capacity' in str(err)
    else:
        raise AssertionError('record_cvs with capacity 0 was accepted')
    assert ens.load_cvs(P.fixture(name)) == 0 and ens.n_cv == len(specs)       # no group: 0, nothing changes
    bad = os.path.join(work, 'bad.up')
    shutil.copyfile(P.fixture(name), bad)
    cfg.add_collective_variables(bad, specs)
    with pkg.h5lite.open_file(bad, 'r+') as f:
        f.delete('input/collective_variables/contact_r0'); f.write('input/collective_variables/contact_r0', np.ones(3, 'f4'))
    try:
        ens.load_cvs(bad)
    except RuntimeError as err:
        print('load_cvs refused: %s' % err)
        assert 'contact_r0' in str(err)
    else:
        raise AssertionError('a group with a short contact_r0 was accepted')
    assert ens.cvs().tobytes() == good.tobytes()
    ok = os.path.join(work, 'ok.up')
    shutil.copyfile(P.fixture(name), ok)
    cfg.add_collective_variables(ok, specs[:3])
    assert ens.load_cvs(ok) == 3 and ens.cv_names == ['rg_ca', 'rmsd_ca', 'q']
    assert ens.cvs().tobytes() == np.ascontiguousarray(good[:, :3]).tobytes()
    ens.close()


CHECKS = dict(values=values, batch=batch, record=record, slots=slots, cli=cli, refusals=refusals)

if __name__ == '__main__':
    import torch
    assert torch.cuda.is_available(), 'these checks need a GPU'
    which, workdir = sys.argv[1], sys.argv[2]
    CHECKS[which](workdir)
    print('CHECK %s PASSED' % which)
