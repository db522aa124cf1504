"""CPU tests of the learned backbone potential's configuration writer (config.add_backbone_network) and of the float64
yardstick the GPU tests compare against (tests/nn_reference.py): the yardstick is pinned against central differences of
its own forward pass before anything is measured with it."""
import os
import shutil
import numpy as np
import pytest
import parity_util as P
import nn_reference as R

cfg = P.pkg.config
h5lite = P.pkg.h5lite


def test_add_backbone_network_writes_the_schema(tmp_path):
    path = str(tmp_path / 'net.up')
    layers, scale, names = R.append_network(P.fixture('proteinG56_7A'), path, R.THREE_LAYER, seed=3)
    assert names == ['backbone_featurizer', 'conv1d_backbone_nn_0', 'conv1d_backbone_nn_1', 'conv1d_backbone_nn_2', 'scaled_sum_backbone_nn']
    with h5lite.open_file(path) as f:
        pot = f.group('input/potential')
        n_res = pot.group('rama_coord').shape('id')[0]
        assert n_res == 56
        g = pot.group('backbone_featurizer')
        assert list(g.get_attr('arguments')) == ['rama_coord', 'protein_hbond']
        rama_idx = g.read('rama_idx'); hbond_idx = g.read('hbond_idx')
        assert rama_idx.dtype.kind == 'i' and hbond_idx.dtype.kind == 'i'
        assert np.array_equal(rama_idx, np.arange(n_res)) and hbond_idx.shape == (n_res, 2)
        ph = pot.group('protein_hbond')
        id1, id2 = ph.read('id1', 'i4'), ph.read('id2', 'i4')
        n_donor = len(id1)
        seq = [x.decode() for x in f.read('input/sequence')]
        for res in range(n_res):
            d, a = hbond_idx[res]
            # -1 exactly for the residues without that site: no donor on the first residue and on prolines, no acceptor on the last
            assert (d == -1) == (res not in id1) == (res == 0 or seq[res] == 'PRO'), res
            assert (a == -1) == (res not in id2) == (res == n_res - 1), res
            if d >= 0:
                assert 0 <= d < n_donor and id1[d] == res
            if a >= 0:
                assert n_donor <= a < n_donor + len(id2) and id2[a - n_donor] == res
        prev = 'backbone_featurizer'
        for k, (w, b, act) in enumerate(layers):
            g = pot.group('conv1d_backbone_nn_%d' % k)
            assert list(g.get_attr('arguments')) == [prev]
            assert g.shape('weights') == w.shape and g.shape('bias') == b.shape
            fw = g.read('weights'); fb = g.read('bias')
            assert fw.dtype == np.float32 and fb.dtype == np.float32        # get_param returns the file's values bit for bit
            assert np.array_equal(fw, w) and np.array_equal(fb, b)
            a = g.get_attr('activation')
            assert isinstance(a, list) and a == [act]                        # a string VECTOR of length 1
            prev = 'conv1d_backbone_nn_%d' % k
        g = pot.group('scaled_sum_backbone_nn')
        assert list(g.get_attr('arguments')) == [prev]
        assert float(np.ravel(g.get_attr('scale'))[0]) == scale
        assert scale == abs(float(np.float32(np.ravel(pot.group('hbond_energy').get_attr('protein_hbond_energy'))[0])))


def test_a_second_network_shares_the_featurizer(tmp_path):
    path = str(tmp_path / 'net.up')
    R.append_network(P.fixture('trpcage20_7A'), path, R.SINGLE_LAYER, seed=3)
    cfg.add_backbone_network(path, R.random_layers(R.SINGLE_LAYER, 5), 0.5, name='second')
    with h5lite.open_file(path) as f:
        assert 'conv1d_second_0' in f.group('input/potential') and 'scaled_sum_second' in f.group('input/potential')
    with pytest.raises(ValueError, match='already has a node'):
        cfg.add_backbone_network(path, R.random_layers(R.SINGLE_LAYER, 5), 0.5, name='second')


def test_add_backbone_network_refuses_bad_layer_lists(tmp_path):
    path = str(tmp_path / 'net.up')
    shutil.copyfile(P.fixture('trpcage20_7A'), path)
    os.chmod(path, 0o644)
    ok = R.random_layers(R.THREE_LAYER, 1)
    bad_channels = [ok[0], (np.zeros((5, 31, 32), 'f4'), np.zeros(32, 'f4'), 'Tanh'), ok[2]]
    with pytest.raises(ValueError, match='input channels'):
        cfg.add_backbone_network(path, bad_channels, 1.)
    with pytest.raises(ValueError, match='one output channel'):
        cfg.add_backbone_network(path, ok[:2], 1.)
    with pytest.raises(ValueError, match='bias'):
        cfg.add_backbone_network(path, [(np.zeros((3, 6, 1), 'f4'), np.zeros(2, 'f4'), 'Identity')], 1.)
    with pytest.raises(ValueError, match='activation'):
        cfg.add_backbone_network(path, [(np.zeros((3, 6, 1), 'f4'), np.zeros(1, 'f4'), 'Sigmoid')], 1.)
    # 20 residues: a summed halo of 20 leaves no row
    too_long = R.random_layers(((11, 4, 'Tanh'), (11, 1, 'Identity')), 2)
    with pytest.raises(ValueError, match='residues'):
        cfg.add_backbone_network(path, too_long, 1.)
    just_fits = R.random_layers(((11, 4, 'Tanh'), (10, 1, 'Identity')), 2)      # halo 19: one output row
    cfg.add_backbone_network(path, just_fits, 1.)
    with h5lite.open_file(path) as f:      # the refused calls wrote nothing
        keys = [k for k in f.group('input/potential').keys() if k.startswith(('conv1d', 'scaled_sum', 'backbone_featurizer'))]
    assert sorted(keys) == ['backbone_featurizer', 'conv1d_backbone_nn_0', 'conv1d_backbone_nn_1', 'scaled_sum_backbone_nn']


def _inputs(rs, n_res=23):
    rama = rs.uniform(-np.pi, np.pi, size=(n_res, 2))
    n_donor, n_acc = n_res - 3, n_res - 1
    hbond = rs.uniform(0., 1., size=(n_donor + n_acc, 7))
    rama_idx = np.arange(n_res)
    hbond_idx = np.full((n_res, 2), -1)
    hbond_idx[3:, 0] = np.arange(n_donor)
    hbond_idx[:-1, 1] = n_donor + np.arange(n_acc)
    return rama, hbond, rama_idx, hbond_idx


def _central(f, x, h):
    """d f / d x by central differences, x perturbed in place"""
    d = np.zeros_like(x)
    it = np.nditer(x, flags=['multi_index'])
    for _ in it:
        i = it.multi_index
        x0 = x[i]
        x[i] = x0 + h; fp = f()
        x[i] = x0 - h; fm = f()
        x[i] = x0
        d[i] = (fp - fm) / (2. * h)
    return d


@pytest.mark.parametrize('act', R.ACTIVATIONS)
def test_yardstick_backward_matches_central_differences_of_its_forward(act):
    h = 1e-6
    spec = ((3, 5, act), (4, 4, act), (1, 1, 'Identity'))
    def clear_of_kinks(feat, layers):
        x = feat
        for w, b, a in layers:
            if a == 'ReLU' and not (np.abs(R.conv1d(x, w, b, 'Identity')) > 1e-3).all():
                return False
            x = R.conv1d(x, w, b, a)
        return True

    for seed in range(200):      # draw until no ReLU pre-activation lies within 1e-3 (>> the difference step) of zero
        rs = np.random.RandomState(100 + seed)
        rama, hbond, rama_idx, hbond_idx = _inputs(rs)
        layers = [(w.astype('f8'), b.astype('f8'), a) for w, b, a in R.random_layers(spec, 200 + seed)]
        feat = R.featurize(rama, hbond, rama_idx, hbond_idx)
        if clear_of_kinks(feat, layers):
            break
    else:
        pytest.fail('no draw kept the ReLU pre-activations away from zero')
    scale = 0.7
    energy = lambda: R.network_energy(R.featurize(rama, hbond, rama_idx, hbond_idx), layers, scale)
    back = R.network_backward(feat, layers, scale)
    d_rama, d_hb = R.featurize_backward(feat, back['feat_sens'], rama_idx, hbond_idx, len(rama), len(hbond))

    def close(analytic, numeric, what):
        scale_ = np.abs(numeric).max()
        assert scale_ > 0., what
        err = np.abs(np.asarray(analytic) - numeric).max() / scale_
        assert err <= 1e-7, (what, act, err)

    close(d_rama, _central(energy, rama, h), 'rama')
    fd_hb = _central(energy, hbond, h)
    close(d_hb, fd_hb[:, 6], 'hbond column 6')
    assert not np.any(fd_hb[:, :6])
    for k, (w, b, a) in enumerate(layers):
        close(back['dW'][k], _central(energy, w, h), 'weights %d' % k)
        close(back['db'][k], _central(energy, b, h), 'bias %d' % k)
    # sens of an intermediate layer: perturb its output and run the rest of the network
    for k in range(len(layers) - 1):
        o = back['outs'][k].copy()
        rest = lambda: float(scale) * float(R.network_forward(o, layers[k + 1:])[-1].sum())
        close(back['sens'][k], _central(rest, o, h), 'sens %d' % k)
    # the layout of get_param
    assert R.param_vector(layers[0][0], layers[0][1]).shape == (3 * 6 * 5 + 5,)
    assert abs(back['d_scale'] * scale - energy()) <= 1e-12 * abs(energy())


def test_yardstick_handles_repeated_and_missing_indices():
    rs = np.random.RandomState(4)
    rama, hbond, rama_idx, hbond_idx = _inputs(rs, 9)
    rama_idx = rama_idx.copy(); rama_idx[3] = 2                      # the reference allows a repeat
    feat = R.featurize(rama, hbond, rama_idx, hbond_idx)
    assert np.array_equal(feat[2, :4], feat[3, :4]) and not np.any(feat[:3, 4]) and feat[-1, 5] == 0.
    sens = rs.normal(size=feat.shape)
    d_rama, d_hb = R.featurize_backward(feat, sens, rama_idx, hbond_idx, len(rama), len(hbond))
    assert not np.any(d_rama[3])
    assert abs(d_rama[2, 0] - sum(sens[r, 0] * feat[r, 1] - sens[r, 1] * feat[r, 0] for r in (2, 3))) < 1e-14
    assert abs(d_hb.sum() - sens[3:, 4].sum() - sens[:-1, 5].sum()) < 1e-12
