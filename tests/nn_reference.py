"""Yardstick of the learned backbone potential (backbone_featurizer -> conv1d stack -> scaled_sum): a float64 numpy
restatement of the nodes' formulas -- forward, backward and weight gradient -- that never calls the library, and a helper
that copies a fixture and appends a seeded network with config.add_backbone_network.

    features   row r = (sin phi, cos phi, sin psi, cos psi, don, acc); phi, psi = columns 0, 1 of rama row rama_idx[r];
               don, acc = column 6 of the hbond rows hbond_idx[r, 0], hbond_idx[r, 1] (0 where the index is -1)
    conv1d     out[r, co] = act(bias[co] + sum_{w, ci} in[r + w, ci] * weights[w, ci, co]),  r < n_in - W + 1
    scaled_sum potential = scale * sum_r in[r]
    backward   g = sens * act'(out)  (ReLU: out > 0, Tanh: 1 - out^2, from the output);
               in_sens[r + w, ci] += sum_co g[r, co] * weights[w, ci, co];
               dW[w, ci, co] = sum_r g[r, co] * in[r + w, ci];  db[co] = sum_r g[r, co]
               d/dphi = s0 * out1 - s1 * out0,  d/dpsi = s2 * out3 - s3 * out2,  s4 / s5 go to column 6 of the hbond rows
"""
import os
import shutil
import sys
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

ACTIVATIONS = ('ReLU', 'Tanh', 'Identity')


def activate(x, act):
    if act == 'ReLU':
        return np.maximum(x, 0.)
    if act == 'Tanh':
        return np.tanh(x)
    if act == 'Identity':
        return x
    raise ValueError(act)


def activation_deriv_from_output(y, act):
    if act == 'ReLU':
        return (y > 0.).astype('f8')
    if act == 'Tanh':
        return 1. - y * y
    if act == 'Identity':
        return np.ones_like(y)
    raise ValueError(act)


def featurize(rama, hbond, rama_idx, hbond_idx):
    rama = np.asarray(rama, 'f8'); hbond = np.asarray(hbond, 'f8')
    rama_idx = np.asarray(rama_idx); hbond_idx = np.asarray(hbond_idx)
    n = len(rama_idx)
    out = np.zeros((n, 6))
    phi, psi = rama[rama_idx, 0], rama[rama_idx, 1]
    out[:, 0] = np.sin(phi); out[:, 1] = np.cos(phi); out[:, 2] = np.sin(psi); out[:, 3] = np.cos(psi)
    for col in (0, 1):
        have = hbond_idx[:, col] >= 0
        out[have, 4 + col] = hbond[hbond_idx[have, col], 6]
    return out


def featurize_backward(feat, sens, rama_idx, hbond_idx, n_rama, n_hbond):
    """(d/d rama [n_rama, 2], d/d column 6 of hbond [n_hbond]); repeated indices add up"""
    feat = np.asarray(feat, 'f8'); sens = np.asarray(sens, 'f8')
    d_rama = np.zeros((n_rama, 2)); d_hb = np.zeros(n_hbond)
    np.add.at(d_rama[:, 0], rama_idx, sens[:, 0] * feat[:, 1] - sens[:, 1] * feat[:, 0])
    np.add.at(d_rama[:, 1], rama_idx, sens[:, 2] * feat[:, 3] - sens[:, 3] * feat[:, 2])
    hbond_idx = np.asarray(hbond_idx)
    for col in (0, 1):
        have = hbond_idx[:, col] >= 0
        np.add.at(d_hb, hbond_idx[have, col], sens[have, 4 + col])
    return d_rama, d_hb


def conv1d(x, weights, bias, act):
    x = np.asarray(x, 'f8'); weights = np.asarray(weights, 'f8'); bias = np.asarray(bias, 'f8')
    W, c_in, c_out = weights.shape
    assert x.shape[1] == c_in and x.shape[0] >= W
    n_out = x.shape[0] - W + 1
    pre = np.tile(bias, (n_out, 1))
    for w in range(W):
        pre += x[w:w + n_out].dot(weights[w])
    return activate(pre, act)


def conv1d_backward(x, weights, out, sens, act):
    """(in_sens [n_in, C_in], dW [W, C_in, C_out], db [C_out]) from the layer's input, its OUTPUT and the output's sens"""
    x = np.asarray(x, 'f8'); weights = np.asarray(weights, 'f8')
    g = np.asarray(sens, 'f8') * activation_deriv_from_output(np.asarray(out, 'f8'), act)
    W = weights.shape[0]
    n_out = g.shape[0]
    in_sens = np.zeros_like(x); dW = np.zeros_like(weights)
    for w in range(W):
        in_sens[w:w + n_out] += g.dot(weights[w].T)
        dW[w] = x[w:w + n_out].T.dot(g)
    return in_sens, dW, g.sum(axis=0)


def network_forward(feat, layers):
    """outputs of every layer, in order; layers = [(weights, bias, activation), ...]"""
    outs = []
    x = np.asarray(feat, 'f8')
    for w, b, a in layers:
        x = conv1d(x, w, b, a)
        outs.append(x)
    return outs


def network_energy(feat, layers, scale):
    return float(scale) * float(network_forward(feat, layers)[-1].sum())


def network_backward(feat, layers, scale):
    """dict: outs (per layer), sens (per layer: d energy / d that layer's output), feat_sens, dW, db (per layer), d_scale"""
    outs = network_forward(feat, layers)
    sens = [None] * len(layers); dW = [None] * len(layers); db = [None] * len(layers)
    s = np.full_like(outs[-1], float(scale))
    for k in range(len(layers) - 1, -1, -1):
        sens[k] = s
        x = outs[k - 1] if k else np.asarray(feat, 'f8')
        s, dW[k], db[k] = conv1d_backward(x, layers[k][0], outs[k], s, layers[k][2])
    return dict(outs=outs, sens=sens, feat_sens=s, dW=dW, db=db, d_scale=float(outs[-1].sum()))


def param_vector(weights, bias):
    """the layout of the node's get_param(): weights in file order, then bias"""
    return np.concatenate((np.asarray(weights).ravel(), np.asarray(bias).ravel()))


# ---- networks for the tests ---------------------------------------------------------------------------------------
THREE_LAYER = ((5, 32, 'ReLU'), (5, 32, 'Tanh'), (1, 1, 'Identity'))       # 6 -> 32 (W 5) -> 32 (W 5) -> 1 (W 1)
THREE_LAYER_SMOOTH = ((5, 32, 'Tanh'), (5, 32, 'Tanh'), (1, 1, 'Identity'))
SINGLE_LAYER = ((3, 1, 'Identity'),)


def random_layers(spec, seed, c_in=6):
    """seeded float32 layers [(weights, bias, activation)] for spec = ((W, C_out, activation), ...): weights of variance
    1 / (W * C_in), so that every layer's output is of order one whatever its size"""
    rs = np.random.RandomState(seed)
    layers = []
    for W, c_out, act in spec:
        w = (rs.normal(size=(W, c_in, c_out)) / np.sqrt(W * c_in)).astype('f4')
        b = (0.3 * rs.normal(size=c_out)).astype('f4')
        layers.append((w, b, act))
        c_in = c_out
    return layers


def append_network(fixture_path, out_path, spec=THREE_LAYER, seed=1, name='backbone_nn', layers=None):
    """copy a configuration and append a seeded network; returns (layers, scale, node names).  The last layer's output is
    of order one per residue, so with scale = |protein_hbond_energy| the network's energy is of the order of the
    hydrogen-bond energy (that energy per bond times a count of the order of the chain length)."""
    from __graft_entry__ import load_package
    pkg = load_package()
    shutil.copyfile(fixture_path, out_path)
    os.chmod(out_path, 0o644)
    with pkg.h5lite.open_file(out_path) as f:
        scale = abs(float(np.ravel(f.group('input/potential/hbond_energy').get_attr('protein_hbond_energy'))[0]))
    scale = float(np.float32(scale))
    if layers is None:
        layers = random_layers(spec, seed)
    names = pkg.config.add_backbone_network(out_path, layers, scale, name=name)
    return layers, scale, names
