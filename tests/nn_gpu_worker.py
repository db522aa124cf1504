"""Child process of tests/test_gpu_nn_nodes.py: one check of the learned backbone potential per invocation,

    python tests/nn_gpu_worker.py CHECK WORKDIR

prints every figure it compares before it asserts and ends with 'CHECK <name> PASSED'.  The yardstick is tests/nn_reference.py
(float64 numpy); tolerances are parity_util.RTOL as relative RMS and 10 x RTOL for the largest element, both relative to the
scale of the array compared (parity_util.compare)."""
import os
import re
import subprocess
import sys
import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import parity_util as P      # noqa: E402
import nn_reference as R     # noqa: E402

pkg = P.pkg
RTOL = P.RTOL
FEAT = 'backbone_featurizer'
SUM = 'scaled_sum_backbone_nn'
CASES = [('proteinG56_7A', R.THREE_LAYER), ('syn300_10A', R.THREE_LAYER), ('trpcage20_7A', R.SINGLE_LAYER)]


def conv(k):
    return 'conv1d_backbone_nn_%d' % k


def indices(path):
    with pkg.h5lite.open_file(path) as f:
        g = f.group('input/potential/' + FEAT)
        return g.read('rama_idx', 'i4'), g.read('hbond_idx', 'i4')


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


def reference_for(up, path, layers, scale):
    """the yardstick fed with the engine's own rama_coord and protein_hbond outputs"""
    rama = up.get_output('rama_coord'); hb = up.get_output('protein_hbond')
    rama_idx, hbond_idx = indices(path)
    feat = R.featurize(rama, hb, rama_idx, hbond_idx)
    back = R.network_backward(feat, layers, scale)
    d_rama, d_hb = R.featurize_backward(feat, back['feat_sens'], rama_idx, hbond_idx, len(rama), len(hb))
    return feat, back, d_rama, d_hb


def forward_dicts(up, feat, back, scale, n_layer):
    ref = {'out/' + FEAT: feat, 'pot/' + SUM: np.float64(scale * back['outs'][-1].sum())}
    act = {'out/' + FEAT: up.get_output(FEAT), 'pot/' + SUM: up.get_output(SUM)[0, 0]}
    for k in range(n_layer):
        ref['out/' + conv(k)] = back['outs'][k]; act['out/' + conv(k)] = up.get_output(conv(k))
    return ref, act


def backward_dicts(up, back, n_layer):
    ref = {'sens/' + FEAT: back['feat_sens']}; act = {'sens/' + FEAT: up.get_sens(FEAT)}
    for k in range(n_layer):
        ref['sens/' + conv(k)] = back['sens'][k]; act['sens/' + conv(k)] = up.get_sens(conv(k))
    return ref, act


def param_deriv_dicts(up, layers, back):
    ref = {'param_deriv/' + SUM: np.array([back['d_scale']])}
    act = {'param_deriv/' + SUM: up.get_param_deriv((1,), SUM)}
    for k, (w, b, a) in enumerate(layers):
        ref['param_deriv/' + conv(k)] = R.param_vector(back['dW'][k], back['db'][k])
        act['param_deriv/' + conv(k)] = up.get_param_deriv((w.size + b.size,), conv(k))
    return ref, act


# ---- check 3 ----------------------------------------------------------------------------------------------------------
def construct(work):
    for name, spec in CASES:
        path = os.path.join(work, name + '.net.up')
        R.append_network(P.fixture(name), path, spec, seed=11)
        up = pkg.Upside(path)
        e = up.energy(P.golden(name)['pos'])
        base = pkg.Upside(P.fixture(name))
        e0 = base.energy(P.golden(name)['pos'])
        net = up.get_output(SUM)[0, 0]
        print('%s: energy %.5f, without the network %.5f, network term %.5f, hbond_energy term %.5f' %
              (name, e, e0, net, up.get_output('hbond_energy')[0, 0]))
        assert np.isfinite(e) and abs((e - e0) - net) <= 1e-4 * max(1., abs(e))
        up.close(); base.close()


# ---- checks 4 and 5 ---------------------------------------------------------------------------------------------------
def forward(work):
    for name, spec in CASES:
        path = os.path.join(work, name + '.net.up')
        layers, scale, _ = R.append_network(P.fixture(name), path, spec, seed=11)
        up = pkg.Upside(path)
        up.energy(P.golden(name)['pos'])
        feat, back, _, _ = reference_for(up, path, layers, scale)
        print(name)
        check(*forward_dicts(up, feat, back, scale, len(layers)), what=name)
        up.close()


def backward(work):
    for name, spec in CASES:
        path = os.path.join(work, name + '.net.up')
        layers, scale, _ = R.append_network(P.fixture(name), path, spec, seed=11)
        x = P.golden(name)['pos']
        up = pkg.Upside(path); base = pkg.Upside(P.fixture(name))
        up.deriv(x); base.deriv(x)
        feat, back, d_rama, d_hb = reference_for(up, path, layers, scale)
        print(name)
        check(*backward_dicts(up, back, len(layers)), what=name)
        with_net = up.get_sens('rama_coord'); without = base.get_sens('rama_coord')
        check_against_scale(d_rama, with_net - without, with_net, 'sens/rama_coord (with - without the network)')
        with_net = up.get_sens('protein_hbond')[:, 6]; without = base.get_sens('protein_hbond')[:, 6]
        check_against_scale(d_hb, with_net - without, with_net, 'sens/protein_hbond[:, 6] (with - without the network)')
        up.close(); base.close()


# ---- check 6 ----------------------------------------------------------------------------------------------------------
def agreement(work):
    exe = os.path.join(P.ROOT, 'upside-md_amd', 'csrc', 'upside_hip')
    assert os.path.exists(exe), 'upside_hip is not built'
    name = 'proteinG56_7A'
    plain = os.path.join(work, 'plain.up'); net = os.path.join(work, 'net.up')
    R.append_network(P.fixture(name), net, R.THREE_LAYER_SMOOTH, seed=11)
    import shutil
    shutil.copyfile(P.fixture(name), plain); os.chmod(plain, 0o644)
    args = ['--duration', '0.05', '--frame-interval', '0.05', '--temperature', '0.8', '--seed', '1', '--potential-deriv-agreement']
    fig = {}
    for tag, f in (('plain', plain), ('network', net)):
        r = subprocess.run([exe] + args + [f], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
        txt = r.stdout.decode()
        assert r.returncode == 0, txt[-2000:]
        fig[tag] = float(re.search(r'overall potential relative error:\s+([0-9.eE+-]+)', txt).group(1))
        if tag == 'network':
            m = re.search(r'^' + SUM + r':\s+(-?[0-9.]+)\s*$', txt, re.M)
            assert m, txt[-2000:]
            print('network term of the initial structure: %s' % m.group(1))
    print('potential-deriv-agreement, overall relative error: unmodified fixture %.5f, with the network %.5f' % (fig['plain'], fig['network']))
    assert fig['network'] <= 2. * fig['plain'], fig


# ---- check 7 ----------------------------------------------------------------------------------------------------------
def weights(work):
    name = 'proteinG56_7A'
    path = os.path.join(work, 'net.up')
    layers, scale, _ = R.append_network(P.fixture(name), path, R.THREE_LAYER, seed=11)
    x = P.golden(name)['pos']
    up = pkg.Upside(path)
    up.deriv(x)
    feat, back, _, _ = reference_for(up, path, layers, scale)
    check(*param_deriv_dicts(up, layers, back), what='param_deriv')
    for k, (w, b, a) in enumerate(layers):
        assert np.array_equal(up.get_param((w.size + b.size,), conv(k)), R.param_vector(w, b)), k      # the file's values, weights then bias
    assert up.get_param((1,), SUM)[0] == np.float32(scale)
    # new weights: the forward pass follows
    rs = np.random.RandomState(3)
    new_layers = [((w + 0.1 * rs.normal(size=w.shape)).astype('f4'), (b + 0.1 * rs.normal(size=b.shape)).astype('f4'), a) for w, b, a in layers]
    new_scale = float(np.float32(1.25 * scale))
    for k, (w, b, a) in enumerate(new_layers):
        up.set_param(R.param_vector(w, b), conv(k))
        assert np.array_equal(up.get_param((w.size + b.size,), conv(k)), R.param_vector(w, b))
    up.set_param([new_scale], SUM)
    up.deriv(x)
    feat, back2, _, _ = reference_for(up, path, new_layers, new_scale)
    assert abs(back2['outs'][-1].sum() - back['outs'][-1].sum()) > 1e-3, 'the perturbation changes nothing'
    check(*forward_dicts(up, feat, back2, new_scale, len(layers)), what='forward after set_param')
    check(*param_deriv_dicts(up, new_layers, back2), what='param_deriv after set_param')
    for node, n in ((conv(0), layers[0][0].size + layers[0][1].size), (SUM, 1)):
        for wrong in (n - 1, n + 1):
            try:
                up.set_param(np.zeros(wrong, 'f4'), node)
            except RuntimeError:
                pass
            else:
                raise AssertionError('set_param of %d values on %s did not raise' % (wrong, node))
    up.deriv(x)
    check(*forward_dicts(up, feat, back2, new_scale, len(layers)), what='forward after the refused set_param')
    up.close()
    # an Ensemble that has run MD steps: the steps after set_param use the new weights
    S = 4
    ens = pkg.engine.Ensemble(path, S)
    ens.set_pos(x); ens.init_md(0.8, 5)
    ens.run_steps(12)
    for k, (w, b, a) in enumerate(new_layers):
        ens.set_param(R.param_vector(w, b), conv(k))
    ens.set_param([new_scale], SUM)
    ens.run_steps(12)
    pos = ens.get_pos()
    e_ens = ens.energies()
    ens.close()
    new_path = os.path.join(work, 'net_new.up')
    R.append_network(P.fixture(name), new_path, layers=new_layers)
    with pkg.h5lite.open_file(new_path, 'r+') as f:
        f.group('input/potential/' + SUM).set_attr('scale', new_scale)
    e_fresh = {}
    for tag, p in (('new', new_path), ('old', path)):
        fresh = pkg.engine.Ensemble(p, S)
        fresh.set_pos(pos)
        e_fresh[tag] = fresh.energies()
        fresh.close()
    print('energies after set_param + steps:', e_ens)
    print('fresh engine, new weights:       ', e_fresh['new'])
    print('fresh engine, old weights:       ', e_fresh['old'])
    denom = np.maximum(1., np.abs(e_fresh['new']))
    assert (np.abs(e_ens - e_fresh['new']) / denom <= RTOL).all()
    assert (np.abs(e_fresh['old'] - e_fresh['new']) / denom > 100 * RTOL).all(), 'old and new weights cannot be told apart'


# ---- check 8 ----------------------------------------------------------------------------------------------------------
def batch(work, S):
    name = 'proteinG56_7A'
    path = os.path.join(work, 'net.up')
    layers, scale, _ = R.append_network(P.fixture(name), path, R.THREE_LAYER, seed=11)
    g = P.golden(name)
    rs = np.random.RandomState(S)
    x = (g['pos'][None] + np.float32(0.05) * rs.normal(size=(S,) + g['pos'].shape)).astype('f4')
    same = (0, 7, S - 1)
    for s in same:
        x[s] = x[0]
    nodes = {conv(k): (w.size + b.size,) for k, (w, b, a) in enumerate(layers)}
    nodes[SUM] = (1,)

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
    for s in same[1:]:      # a system's place in the batch does not change a sum
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
        print('accumulate %-28s max deviation from the float64 weighted sum / scale %.3e' % (n, err))
        assert err <= RTOL, (n, err)


def batch64(work):
    batch(work, 64)


def batch600(work):
    batch(work, 600)


# ---- check 9 ----------------------------------------------------------------------------------------------------------
def md(work):
    name = 'proteinG56_7A'
    path = os.path.join(work, 'net.up')
    R.append_network(P.fixture(name), path, R.THREE_LAYER, seed=11)
    x = P.golden(name)['pos']

    def run(p, chunks):
        ens = pkg.engine.Ensemble(p, 8)
        ens.set_pos(x); ens.init_md(0.8, 9)
        for n in chunks:
            ens.run_steps(n)
        out = ens.get_pos(), ens.get_mom()
        ens.close()
        return out

    a = run(path, [200]); b = run(path, [200])
    assert np.isfinite(a[0]).all() and np.isfinite(a[1]).all()
    assert np.abs(a[0] - x[None]).max() > 1e-2, 'nothing moved'
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes(), 'two runs of 200 steps differ'
    print('200 steps on 8 systems with the network: finite, bit-identical across two runs')
    p0 = run(P.fixture(name), [200]); p1 = run(P.fixture(name), [1] * 200)
    if p0[0].tobytes() == p1[0].tobytes() and p0[1].tobytes() == p1[1].tobytes():
        c = run(path, [1] * 200)
        assert a[0].tobytes() == c[0].tobytes() and a[1].tobytes() == c[1].tobytes(), 'run_steps(200) and 200 x run_steps(1) differ'
        print('run_steps(200) and 200 x run_steps(1) are bit-identical, with and without the network')
    else:
        print('HALF SKIPPED: the unmodified fixture itself differs between run_steps(200) and 200 x run_steps(1)')


# ---- check 10 ---------------------------------------------------------------------------------------------------------
def full_check(name, path, layers, scale):
    x = P.golden(name)['pos']
    up = pkg.Upside(path)
    up.deriv(x)
    feat, back, _, _ = reference_for(up, path, layers, scale)
    check(*forward_dicts(up, feat, back, scale, len(layers)), what=name + ' forward')
    check(*backward_dicts(up, back, len(layers)), what=name + ' backward')
    check(*param_deriv_dicts(up, layers, back), what=name + ' param_deriv')
    up.close()


def edges(work):
    # the weights of a 15 x 64 x 64 layer do not fit a workgroup's LDS: channel-sliced tiles
    name = 'syn300_10A'
    path = os.path.join(work, 'wide.up')
    spec = ((15, 64, 'Tanh'), (15, 64, 'ReLU'), (1, 1, 'Identity'))
    layers, scale, _ = R.append_network(P.fixture(name), path, spec, seed=21)
    print('W = 15, 6 -> 64 -> 64 -> 1 on %s' % name)
    full_check(name, path, layers, scale)
    # W = chain length: one output row
    name = 'trpcage20_7A'
    path = os.path.join(work, 'one_row.up')
    layers, scale, _ = R.append_network(P.fixture(name), path, ((20, 1, 'Identity'),), seed=22)
    print('W = 20 on the 20 residues of %s' % name)
    up = pkg.Upside(path)
    assert up.get_output_dims(conv(0)) == (1, 1)
    up.close()
    full_check(name, path, layers, scale)
    # beyond the stated limits: right, or refused with the documented message
    path = os.path.join(work, 'huge.up')
    layers, scale, _ = R.append_network(P.fixture(name), path, ((1, 600, 'Tanh'), (1, 1, 'Identity')), seed=23)
    try:
        ens = pkg.engine.Ensemble(path, 1)
    except RuntimeError as err:
        print('6 -> 600 -> 1 refused: %s' % err)
        assert 'conv1d' in str(err) and 'exceeds the device limit' in str(err), err
    else:
        ens.close()
        print('6 -> 600 -> 1 constructs')
        full_check(name, path, layers, scale)


# ---- check 11 ---------------------------------------------------------------------------------------------------------
def errors(work):
    name = 'trpcage20_7A'
    good = os.path.join(work, 'good.up')
    layers, scale, _ = R.append_network(P.fixture(name), good, R.THREE_LAYER, seed=11)
    x = P.golden(name)['pos']
    n_case = [0]

    def refused(edit, *needles):
        n_case[0] += 1
        path = os.path.join(work, 'bad%d.up' % n_case[0])
        R.append_network(P.fixture(name), path, R.THREE_LAYER, seed=11)
        with pkg.h5lite.open_file(path, 'r+') as f:
            edit(f.group('input/potential'))
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

    def rewrite(group, dset, arr):
        group.delete(dset); group.write(dset, arr)

    refused(lambda pot: pot.group(conv(0)).set_attr('activation', ['Sigmoid']), conv(0), 'Invalid activation name')
    refused(lambda pot: pot.group(conv(1)).set_attr('activation', ['ReLU', 'Tanh']), conv(1), 'Invalid number of activations')
    refused(lambda pot: rewrite(pot.group(conv(0)), 'weights', np.zeros((5, 5, 32), 'f4')), conv(0), 'C_in = 5', 'elem_width 6')
    refused(lambda pot: rewrite(pot.group(conv(1)), 'bias', np.zeros(31, 'f4')), conv(1), 'bias has 31 entries')
    refused(lambda pot: rewrite(pot.group(conv(0)), 'weights', np.zeros((21, 6, 32), 'f4')), conv(0), 'fewer than the kernel width W = 21')

    def two_wide(pot):
        rewrite(pot.group(conv(2)), 'weights', np.zeros((1, 32, 2), 'f4')); rewrite(pot.group(conv(2)), 'bias', np.zeros(2, 'f4'))
    refused(two_wide, SUM, 'Sum only works on elem width 1')

    def rama_out_of_range(pot):
        idx = pot.group(FEAT).read('rama_idx', 'i4'); idx[3] = len(idx)
        rewrite(pot.group(FEAT), 'rama_idx', idx)
    refused(rama_out_of_range, FEAT, 'rama_idx', 'out of range')

    def hbond_out_of_range(pot):
        idx = pot.group(FEAT).read('hbond_idx', 'i4'); idx[3, 1] = 10000
        rewrite(pot.group(FEAT), 'hbond_idx', idx)
    refused(hbond_out_of_range, FEAT, 'hbond_idx', 'out of range')

    # a ladder whose files differ only in a network dataset: per-system weights are out of scope, the files are refused
    other = os.path.join(work, 'other.up')
    R.append_network(P.fixture(name), other, R.THREE_LAYER, seed=11)
    with pkg.h5lite.open_file(other, 'r+') as f:
        g = f.group('input/potential/' + conv(0))
        w = g.read('weights'); w[0, 0, 0] += np.float32(0.5)
        rewrite(g, 'weights', w)
    try:
        pkg.engine.Ensemble.from_files([good, other])
    except RuntimeError as err:
        print('ladder refused: %s' % err)
        for nd in (other, 'node ' + conv(0), 'dataset weights', 'cannot differ per system'):
            assert nd in str(err), (nd, str(err))
    else:
        raise AssertionError('a ladder with per-system network weights constructs')
    ens = pkg.engine.Ensemble.from_files([good, good])
    ens.set_pos(x)
    e = ens.energies()
    assert np.isfinite(e).all() and e[0].tobytes() == e[1].tobytes()
    ens.close()


CHECKS = dict(construct=construct, forward=forward, backward=backward, agreement=agreement, weights=weights, batch64=batch64,
              batch600=batch600, md=md, edges=edges, errors=errors)

if __name__ == '__main__':
    import torch
    assert torch.cuda.is_available(), 'these checks need a GPU'
    which, workdir = sys.argv[1], sys.argv[2]
    CHECKS[which](workdir)
    print('CHECK %s PASSED' % which)
