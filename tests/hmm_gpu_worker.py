"""Child process of tests/test_gpu_hmm.py: one check of the TorusDBN backbone prior (torus_dbn -> fixed_hmm) per invocation,

    python tests/hmm_gpu_worker.py CHECK WORKDIR

prints every figure it compares before it asserts and ends with 'CHECK <name> PASSED'.  The yardstick is tests/hmm_reference.py
(float64 numpy, fed with the engine's own rama_coord output); tolerances are parity_util.RTOL as relative RMS and 10 x RTOL for
the largest element, both relative to the scale of the array compared (parity_util.compare)."""
import os
import re
import shutil
import subprocess
import sys
import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import parity_util as P      # noqa: E402
import hmm_reference as R    # noqa: E402

pkg = P.pkg
RTOL = P.RTOL
DBN, HMM = 'torus_dbn', 'fixed_hmm'
N_STATES = (1, 3, 5, 55, 64, 65, 128)      # no mixing, a partial group of 4, TorusDBN's own size, a wavefront boundary, two states per lane


def check(ref, act, what, rtol=RTOL):
    bad = P.compare(ref, act, rtol=rtol, verbose=True)
    assert not bad, (what, bad)


def check_against_scale(ref, act, scale_array, key):
    """ref vs act relative to the scale of scale_array (a difference of two engines is as exact as its larger operand)"""
    ref = np.asarray(ref, 'f8'); act = np.asarray(act, 'f8'); big = np.asarray(scale_array, 'f8')
    rms = np.sqrt(((ref - act) ** 2).sum() / (big ** 2).sum())
    mx = np.abs(ref - act).max() / np.abs(big).max()
    print('%-48s rel_rms %.3e  max/scale %.3e   (relative to the larger operand)' % (key, rms, mx))
    assert rms <= RTOL and mx <= 10 * RTOL, (key, rms, mx)


def rewrite(group, dset, arr):
    group.delete(dset); group.write(dset, arr)


def set_chain(path, par, ids=None, index=None):
    """replace id (with its restypes) and / or index of an appended prior; returns the updated parameters"""
    par = dict(par)
    with pkg.h5lite.open_file(path, 'r+') as f:
        pot = f.group('input/potential')
        if ids is not None:
            ids = np.asarray(ids, 'i4')
            old = dict(zip(par['id'].tolist(), par['restypes'].tolist()))
            par['id'] = ids; par['restypes'] = np.array([old[i] for i in ids.tolist()], 'i4')
            rewrite(pot.group(DBN), 'id', par['id']); rewrite(pot.group(DBN), 'restypes', par['restypes'])
            if index is None:
                index = np.arange(len(ids))
        if index is not None:
            par['index'] = np.asarray(index, 'i4')
            rewrite(pot.group(HMM), 'index', par['index'])
        del pot
    return par


def reference_for(up, par):
    return R.prior_backward(up.get_output('rama_coord'), par, par['index'])


def forward_dicts(up, back):
    return ({'out/' + DBN: back['energy'], 'pot/' + HMM: np.float64(back['pot'])},
            {'out/' + DBN: up.get_output(DBN), 'pot/' + HMM: up.get_output(HMM)[0, 0]})


def param_shapes(par):
    return {DBN: (par['aa_basin_energy'].size,), HMM: (par['transition_energy'].size,)}


def param_deriv_dicts(up, par, back):
    shp = param_shapes(par)
    return ({'param_deriv/' + DBN: back['d_prior'].ravel(), 'param_deriv/' + HMM: back['counts'].ravel()},
            {'param_deriv/' + DBN: up.get_param_deriv(shp[DBN], DBN), 'param_deriv/' + HMM: up.get_param_deriv(shp[HMM], HMM)})


# ---- check 1 ----------------------------------------------------------------------------------------------------------
def construct(work):
    for name in ('trpcage20_7A', 'proteinG56_7A'):
        path = os.path.join(work, name + '.dbn.up')
        R.append_hmm(P.fixture(name), path, n_state=55, seed=11)
        x = P.golden(name)['pos']
        up = pkg.Upside(path); base = pkg.Upside(P.fixture(name))
        e = up.energy(x); e0 = base.energy(x)
        term = up.get_output(HMM)[0, 0]
        print('%s: energy %.5f, without the prior %.5f, fixed_hmm term %.5f' % (name, e, e0, term))
        assert np.isfinite(e) and abs((e - e0) - term) <= 1e-4 * max(1., abs(e))
        up.close(); base.close()


# ---- check 2 ----------------------------------------------------------------------------------------------------------
def forward(work):
    name = 'trpcage20_7A'
    x = P.golden(name)['pos']
    for ns in N_STATES:
        path = os.path.join(work, 'ns%d.up' % ns)
        par = R.append_hmm(P.fixture(name), path, n_state=ns, seed=20 + ns)
        up = pkg.Upside(path)
        up.energy(x)
        print('%s, n_state = %d, the whole interior (%d residues)' % (name, ns, len(par['id'])))
        assert up.get_output_dims(DBN) == (len(par['id']), ns)
        check(*forward_dicts(up, reference_for(up, par)), what=('forward', ns))
        up.close()
    for ns, res in ((5, 7), (55, 1), (128, 18)):      # n_residue = 1: an id of length 1, no transition
        path = os.path.join(work, 'one%d.up' % ns)
        par = R.append_hmm(P.fixture(name), path, n_state=ns, seed=40 + ns)
        par = set_chain(path, par, ids=[res])
        up = pkg.Upside(path)
        up.energy(x)
        back = reference_for(up, par)
        print('%s, n_state = %d, one residue (id = [%d])' % (name, ns, res))
        assert abs(back['pot'] + R.logsumexp(-back['energy'][0])) <= 1e-12
        check(*forward_dicts(up, back), what=('one residue', ns))
        up.close()
    name = 'proteinG56_7A'
    path = os.path.join(work, 'g56.up')
    par = R.append_hmm(P.fixture(name), path, n_state=55, seed=12)
    up = pkg.Upside(path)
    up.energy(P.golden(name)['pos'])
    print('%s, n_state = 55' % name)
    check(*forward_dicts(up, reference_for(up, par)), what=name)
    up.close()


# ---- check 3 ----------------------------------------------------------------------------------------------------------
def backward(work):
    cases = [('trpcage20_7A', ns, False) for ns in N_STATES] + [('proteinG56_7A', 55, False), ('proteinG56_7A', 55, True), ('trpcage20_7A', 65, True)]
    bases = {}
    for name, ns, reverse in cases:
        path = os.path.join(work, '%s.%d.%d.up' % (name, ns, reverse))
        par = R.append_hmm(P.fixture(name), path, n_state=ns, seed=60 + ns)
        if reverse:      # a non-identity, injective index: the chain runs from the last interior residue to the first
            par = set_chain(path, par, index=np.arange(len(par['id']))[::-1])
        x = P.golden(name)['pos']
        up = pkg.Upside(path)
        up.deriv(x)
        if name not in bases:
            base = pkg.Upside(P.fixture(name)); base.deriv(x)
            bases[name] = base.get_sens('rama_coord'); base.close()
        back = reference_for(up, par)
        print('%s, n_state = %d%s' % (name, ns, ', reversed chain' if reverse else ''))
        check({'sens/' + DBN: back['sens']}, {'sens/' + DBN: up.get_sens(DBN)}, what=(name, ns, reverse))
        assert np.abs(back['sens'].sum(axis=1) - 1.).max() <= 1e-12
        with_prior = up.get_sens('rama_coord')
        check_against_scale(back['d_rama'], with_prior[:, :2] - bases[name][:, :2], with_prior[:, :2], 'sens/rama_coord (with - without the prior)')
        if reverse:
            plain = R.prior_backward(up.get_output('rama_coord'), par, None)
            assert np.abs(plain['sens'] - back['sens']).max() > 1e-3, 'the reversed chain cannot be told from the forward one'
        up.close()


# ---- check 4 ----------------------------------------------------------------------------------------------------------
def wide_parameters(n_state, seed):
    """transition energies spanning 0..60 and, within every residue, emission energies spanning 0..60 (exp(-60) is a normal fp32 number)"""
    rs = np.random.RandomState(seed)
    par = R.random_parameters(n_state, seed, kappa=1.)
    par['basin_param'][:, 0] = 0.
    aa = rs.uniform(0., 60., size=par['aa_basin_energy'].shape); aa[:, 0] = 0.; aa[:, -1] = 60.
    te = rs.uniform(0., 60., size=(n_state, n_state)); te[0, 0] = 0.; te[1, 2] = 60.
    par['aa_basin_energy'] = aa.astype('f4'); par['transition_energy'] = te.astype('f4')
    return par


def energy_range(work):
    for name, ns in (('trpcage20_7A', 5), ('proteinG56_7A', 55), ('trpcage20_7A', 128)):
        path = os.path.join(work, 'wide.%s.%d.up' % (name, ns))
        par = R.append_hmm(P.fixture(name), path, par=wide_parameters(ns, 70 + ns))
        x = P.golden(name)['pos']
        up = pkg.Upside(path)
        up.deriv(x)
        back = reference_for(up, par)
        span = back['energy'].max(axis=1) - back['energy'].min(axis=1)
        print('%s, n_state = %d: emission span per residue %.1f .. %.1f, transition span %.1f, -log Z %.4f' %
              (name, ns, span.min(), span.max(), np.ptp(par['transition_energy']), back['pot']))
        assert span.min() > 50. and np.ptp(par['transition_energy']) == 60.
        for v in back.values():
            assert np.isfinite(v).all()
        out, sens = up.get_output(DBN), up.get_sens(DBN)
        assert np.isfinite(out).all() and np.isfinite(sens).all() and np.isfinite(up.get_output(HMM)).all()
        check(*forward_dicts(up, back), what=('range forward', name, ns))
        check({'sens/' + DBN: back['sens']}, {'sens/' + DBN: sens}, what=('range backward', name, ns))
        check(*param_deriv_dicts(up, par, back), what=('range param_deriv', name, ns))
        up.close()


# ---- check 5 ----------------------------------------------------------------------------------------------------------
def agreement(work):
    exe = os.path.join(P.ROOT, 'upside-md_amd', 'csrc', 'upside_hip')
    assert os.path.exists(exe), 'upside_hip is not built'
    name = 'proteinG56_7A'
    plain = os.path.join(work, 'plain.up'); dbn = os.path.join(work, 'dbn.up')
    R.append_hmm(P.fixture(name), dbn, n_state=55, seed=11)
    shutil.copyfile(P.fixture(name), plain); os.chmod(plain, 0o644)
    args = ['--duration', '0.05', '--frame-interval', '0.05', '--temperature', '0.8', '--seed', '1', '--potential-deriv-agreement']
    fig = {}
    for tag, f in (('plain', plain), ('prior', dbn)):
        r = subprocess.run([exe] + args + [f], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
        txt = r.stdout.decode()
        assert r.returncode == 0, txt[-2000:]
        fig[tag] = float(re.search(r'overall potential relative error:\s+([0-9.eE+-]+)', txt).group(1))
        if tag == 'prior':
            m = re.search(r'^' + HMM + r':\s+(-?[0-9.]+)\s*$', txt, re.M)
            assert m, txt[-2000:]
            print('fixed_hmm term of the initial structure: %s' % m.group(1))
    print('potential-deriv-agreement, overall relative error: unmodified fixture %.5f, with the prior %.5f' % (fig['plain'], fig['prior']))
    assert fig['prior'] <= 2. * fig['plain'], fig


# ---- check 6 ----------------------------------------------------------------------------------------------------------
def parameters(work):
    name = 'proteinG56_7A'
    path = os.path.join(work, 'dbn.up')
    par = R.append_hmm(P.fixture(name), path, n_state=55, seed=11)
    shp = param_shapes(par)
    x = P.golden(name)['pos']
    up = pkg.Upside(path)
    up.deriv(x)
    back = reference_for(up, par)
    check(*param_deriv_dicts(up, par, back), what='param_deriv')
    assert abs(back['counts'].sum() - (len(par['id']) - 1)) <= 1e-9
    assert np.array_equal(up.get_param(shp[DBN], DBN), par['aa_basin_energy'].ravel())          # file order
    assert np.array_equal(up.get_param(shp[HMM], HMM), par['transition_energy'].ravel())        # row-major
    rs = np.random.RandomState(3)
    new = dict(par)
    new['aa_basin_energy'] = (par['aa_basin_energy'] + 0.5 * rs.normal(size=par['aa_basin_energy'].shape)).astype('f4')
    new['transition_energy'] = (par['transition_energy'] + rs.uniform(0., 2., size=par['transition_energy'].shape)).astype('f4')
    # one node at a time: the forward pass follows each
    up.set_param(new['aa_basin_energy'].ravel(), DBN)
    assert np.array_equal(up.get_param(shp[DBN], DBN), new['aa_basin_energy'].ravel())
    up.deriv(x)
    half = dict(par, aa_basin_energy=new['aa_basin_energy'])
    back1 = reference_for(up, half)
    assert abs(back1['pot'] - back['pot']) > 1e-2, 'the new prior table changes nothing'
    check(*forward_dicts(up, back1), what='forward after set_param of torus_dbn')
    up.set_param(new['transition_energy'].ravel(), HMM)
    assert np.array_equal(up.get_param(shp[HMM], HMM), new['transition_energy'].ravel())
    up.deriv(x)
    back2 = reference_for(up, new)
    assert abs(back2['pot'] - back1['pot']) > 1e-2, 'the new transition energies change nothing'
    check(*forward_dicts(up, back2), what='forward after set_param of fixed_hmm')
    check({'sens/' + DBN: back2['sens']}, {'sens/' + DBN: up.get_sens(DBN)}, what='sens after set_param')
    check(*param_deriv_dicts(up, new, back2), what='param_deriv after set_param')
    for node in (DBN, HMM):
        for wrong in (shp[node][0] - 1, shp[node][0] + 1):
            try:
                up.set_param(np.zeros(wrong, 'f4'), node)
            except RuntimeError as err:
                print('set_param of %d values on %s refused: %s' % (wrong, node, err))
            else:
                raise AssertionError('set_param of %d values on %s did not raise' % (wrong, node))
    up.deriv(x)
    check(*forward_dicts(up, back2), what='forward after the refused set_param')
    up.close()
    # an Ensemble that has run MD steps: the steps after set_param use the new transition energies
    S = 4
    ens = pkg.engine.Ensemble(path, S)
    ens.set_pos(x); ens.init_md(0.8, 5)
    ens.run_steps(12)
    ens.set_param(new['transition_energy'].ravel(), HMM)
    ens.run_steps(12)
    pos = ens.get_pos()
    e_ens = ens.energies()
    ens.close()
    new_path = os.path.join(work, 'dbn_new.up')
    R.append_hmm(P.fixture(name), new_path, par=dict(par, transition_energy=new['transition_energy']))
    e_fresh = {}
    for tag, p in (('new', new_path), ('old', path)):
        fresh = pkg.engine.Ensemble(p, S)
        fresh.set_pos(pos)
        e_fresh[tag] = fresh.energies()
        fresh.close()
    print('energies after set_param + steps:   ', e_ens)
    print('fresh engine, new transition energy:', e_fresh['new'])
    print('fresh engine, old transition energy:', e_fresh['old'])
    denom = np.maximum(1., np.abs(e_fresh['new']))
    assert (np.abs(e_ens - e_fresh['new']) / denom <= RTOL).all()
    assert (np.abs(e_fresh['old'] - e_fresh['new']) / denom > 100 * RTOL).all(), 'old and new transition energies cannot be told apart'


# ---- check 7 ----------------------------------------------------------------------------------------------------------
def batch(work, S):
    name = 'proteinG56_7A'
    path = os.path.join(work, 'dbn.up')
    par = R.append_hmm(P.fixture(name), path, n_state=55, seed=11)
    g = P.golden(name)
    rs = np.random.RandomState(S)
    x = (g['pos'][None] + np.float32(0.05) * rs.normal(size=(S,) + g['pos'].shape)).astype('f4')
    same = (0, 7, S - 1)
    for s in same:
        x[s] = x[0]
    nodes = param_shapes(par)

    def run():
        ens = pkg.engine.Ensemble(path, S)
        ens.set_pos(x)
        e, d = ens.energies_and_derivs()
        pd = {n: ens.param_deriv(n, shp) for n, shp in nodes.items()}
        w = np.random.RandomState(1).uniform(-1.5, 1.5, size=S).astype('f4')
        acc = {}
        for n, shp in nodes.items():
            ens.param_deriv_accumulate(n, w)
            acc[n] = ens.param_deriv_read(n, shp)[0]
        ens.close()
        return e, d, pd, w, acc

    e, d, pd, w, acc = run()
    e2, d2, pd2, _, acc2 = run()
    assert e.tobytes() == e2.tobytes() and d.tobytes() == d2.tobytes(), 'two identical runs differ'
    for n in nodes:
        assert pd[n].tobytes() == pd2[n].tobytes() and acc[n].tobytes() == acc2[n].tobytes(), n
    for s in same[1:]:      # a system's place in the batch does not change its bits
        assert e[s].tobytes() == e[0].tobytes() and d[s].tobytes() == d[0].tobytes(), s
        for n in nodes:
            assert pd[n][s].tobytes() == pd[n][0].tobytes(), (n, s)
    print('%d systems: systems %s are bit-identical; two runs are bit-identical' % (S, same))
    one = pkg.engine.Ensemble(path, 1)
    worst = dict(energy=0., deriv_rms=0., deriv_max=0.)
    worst.update({n: 0. for n in nodes})
    for s in range(S):
        one.set_pos(x[s])
        e1, d1 = one.energies_and_derivs()
        worst['energy'] = max(worst['energy'], abs(float(e1[0]) - float(e[s])) / max(1., abs(float(e1[0]))))
        worst['deriv_rms'] = max(worst['deriv_rms'], P.rel_rms(d1[0], d[s]))
        worst['deriv_max'] = max(worst['deriv_max'], P.max_rel_to_scale(d1[0], d[s]))
        for n, shp in nodes.items():
            p1 = one.param_deriv(n, shp)[0]
            worst[n] = max(worst[n], P.rel_rms(p1, pd[n][s]), P.max_rel_to_scale(p1, pd[n][s]) / 10.)
    one.close()
    print('%d systems against a one-system engine, worst over the systems:' % S, worst)
    assert worst['energy'] <= RTOL and worst['deriv_rms'] <= RTOL and worst['deriv_max'] <= 10 * RTOL, worst
    for n in nodes:
        assert worst[n] <= RTOL, (n, worst[n])
    for n, shp in nodes.items():
        host = np.zeros(shp, 'f8')
        for s in range(S):
            host += np.float64(w[s]) * pd[n][s].astype('f8')
        err = np.abs(acc[n] - host).max() / max(np.abs(host).max(), 1e-30)
        print('accumulate %-12s max deviation from the float64 weighted sum / scale %.3e' % (n, err))
        assert err <= RTOL, (n, err)


def batch64(work):
    batch(work, 64)


def batch600(work):
    batch(work, 600)


# ---- check 8 ----------------------------------------------------------------------------------------------------------
def md(work):
    name = 'proteinG56_7A'
    path = os.path.join(work, 'dbn.up')
    R.append_hmm(P.fixture(name), path, n_state=55, seed=11)
    x = P.golden(name)['pos']

    def run():
        ens = pkg.engine.Ensemble(path, 8)
        ens.set_pos(x); ens.init_md(0.8, 9)
        ens.run_steps(200)
        out = ens.get_pos(), ens.get_mom()
        ens.close()
        return out

    a = run(); b = run()
    assert np.isfinite(a[0]).all() and np.isfinite(a[1]).all()
    assert np.abs(a[0] - x[None]).max() > 1e-2, 'nothing moved'
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes(), 'two runs of 200 steps differ'
    print('200 steps on 8 systems with the prior: finite, bit-identical across two runs')


# ---- check 9 ----------------------------------------------------------------------------------------------------------
def errors(work):
    name = 'trpcage20_7A'
    good = os.path.join(work, 'good.up')
    R.append_hmm(P.fixture(name), good, n_state=5, seed=11)
    x = P.golden(name)['pos']
    n_case = [0]

    def refused(edit, *needles, **kw):
        n_case[0] += 1
        path = os.path.join(work, 'bad%d.up' % n_case[0])
        R.append_hmm(P.fixture(name), path, n_state=kw.get('n_state', 5), seed=11)
        with pkg.h5lite.open_file(path, 'r+') as f:
            pot = f.group('input/potential')
            edit(pot)
            del pot
        try:
            pkg.engine.Ensemble(path, 1)
        except RuntimeError as err:
            print('refused: %s' % err)
            for nd in needles:
                assert nd in str(err), (nd, str(err))
        else:
            raise AssertionError('a configuration that should be refused constructs: %r' % (needles,))
        ok = pkg.engine.Ensemble(good, 1)      # the process stays usable
        ok.set_pos(x)
        assert np.isfinite(ok.energies()).all()
        ok.close()

    refused(lambda pot: rewrite(pot.group(HMM), 'transition_energy', np.zeros((5, 4), 'f4')), HMM, 'not square')
    refused(lambda pot: rewrite(pot.group(HMM), 'transition_energy', np.zeros((4, 4), 'f4')), HMM, '4 states', 'elem_width 5')
    refused(lambda pot: rewrite(pot.group(HMM), 'index', np.zeros(0, 'i4')), HMM, 'index is empty')

    def edit_ints(node, dset, at, value):
        def edit(pot):
            v = pot.group(node).read(dset, 'i4'); v[at] = value
            rewrite(pot.group(node), dset, v)
        return edit
    refused(edit_ints(DBN, 'id', 3, 20), DBN, 'id', 'out of range')
    refused(edit_ints(DBN, 'id', 3, 5), DBN, 'id', 'repeated index')
    refused(edit_ints(HMM, 'index', 2, 18), HMM, 'index', 'out of range')
    refused(edit_ints(HMM, 'index', 2, 9), HMM, 'index', 'repeated index')
    refused(edit_ints(DBN, 'restypes', 4, len(R.RESTYPE_ORDER)), DBN, 'restypes', 'outside the %d rows' % len(R.RESTYPE_ORDER))
    refused(lambda pot: None, HMM, '129 states exceed the device limit', 'n_state <= 128', n_state=129)

    # a ladder whose files differ only in transition_energy: per-system values of this node are not offered, the files are refused
    other = os.path.join(work, 'other.up')
    R.append_hmm(P.fixture(name), other, n_state=5, seed=11)
    with pkg.h5lite.open_file(other, 'r+') as f:
        g = f.group('input/potential/' + HMM)
        t = g.read('transition_energy'); t[0, 0] += np.float32(0.5)
        rewrite(g, 'transition_energy', t)
        del g
    try:
        pkg.engine.Ensemble.from_files([good, other])
    except RuntimeError as err:
        print('ladder refused: %s' % err)
        for nd in (other, 'node ' + HMM, 'dataset transition_energy', 'cannot differ per system'):
            assert nd in str(err), (nd, str(err))
    else:
        raise AssertionError('a ladder with per-system transition energies constructs')
    ens = pkg.engine.Ensemble.from_files([good, good])
    ens.set_pos(x)
    e = ens.energies()
    assert np.isfinite(e).all() and e[0].tobytes() == e[1].tobytes()
    ens.close()


CHECKS = dict(construct=construct, forward=forward, backward=backward, energy_range=energy_range, agreement=agreement, parameters=parameters,
              batch64=batch64, batch600=batch600, md=md, errors=errors)

if __name__ == '__main__':
    import torch
    assert torch.cuda.is_available(), 'these checks need a GPU'
    which, workdir = sys.argv[1], sys.argv[2]
    CHECKS[which](workdir)
    print('CHECK %s PASSED' % which)
