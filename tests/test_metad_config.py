"""CPU tests of the metadynamics analysis: the float64 yardstick tests/metad_reference.py against a scalar double loop and against
config.metadynamics_free_energy, the rule for the hills a frame saw, the wrappers' shape and value errors (raised before the
library is touched), and the reweighting formula itself on a toy with a known free energy."""
import math
import numpy as np
import pytest
import parity_util as P
import metad_cases as C
import metad_reference as R

metad = P.pkg.metad
cfg = P.pkg.config


def scalar_bias(x, centers, weights, sigma, periods, m):
    v = a = 0.
    for h in range(m):
        q = 0.
        for c in range(len(sigma)):
            dx = float(x[c]) - float(centers[h][c])
            if periods[c] > 0:
                dx = dx - periods[c] * round(dx / periods[c])      # (round half to even, as rint)
            q += dx * dx / (sigma[c] * sigma[c])
        e = math.exp(-0.5 * q)
        v += float(weights[h]) * e; a += abs(float(weights[h])) * e
    return v, a


@pytest.mark.parametrize('periodic', [False, True])
@pytest.mark.parametrize('d', [1, 2, 3, 4])
def test_yardstick_equals_a_scalar_double_loop(d, periodic):
    c, w = C.hills(d, 7, 10 + d, periodic)
    per = C.periods_of(d, periodic)
    x = C.points_near(c, 6, 20 + d, d, periodic)
    m = np.array([0, 1, 3, 7, 7, 5])
    V, A = R.bias(x, c, w, C.SIGMA[:d], per, m)
    for i in range(len(x)):
        v, a = scalar_bias(x[i], c, w, C.SIGMA[:d], per, int(m[i]))
        assert abs(V[i] - v) <= 1e-14 * max(a, 1e-300) and abs(A[i] - a) <= 1e-14 * max(a, 1e-300), (d, periodic, i)
    assert V[0] == 0. and A[0] == 0.
    # the grid, with checkpoints and log-sum-exps
    axes = C.axes_over(d, (3, 2, 2, 2)[:d], periodic)
    gr = R.bias_grid(axes, c, w, C.SIGMA[:d], per, [0, 2, 7], C.SCALES)
    g = R.grid_points(axes)
    assert g.shape == (int(np.prod([len(a) for a in axes])), d) and np.array_equal(g[1], [a[0] for a in axes[:-1]] + [axes[-1][1]])      # C order
    for j, mm in enumerate((0, 2, 7)):
        ref = np.array([scalar_bias(p, c, w, C.SIGMA[:d], per, mm) for p in g])
        assert np.abs(gr['V'][j] - ref[:, 0]).max() <= 1e-14 * max(ref[:, 1].max(), 1e-300)
        for q, s in enumerate(C.SCALES):
            want = math.log(sum(math.exp(s * v - max(s * ref[:, 0])) for v in ref[:, 0])) + max(s * ref[:, 0])
            assert abs(gr['lse'][j, q] - want) <= 1e-13
    assert np.allclose(gr['lse'][0], math.log(len(g)), rtol=0, atol=1e-15)


def test_grid_bias_equals_the_host_free_energy():
    c, w = C.hills(2, 40, 3, True)
    per = C.periods_of(2, True)
    axes = C.axes_over(2, (9, 7), True)
    V = R.bias_grid(axes, c, w, C.SIGMA[:2], per)['V'][0]
    F = cfg.metadynamics_free_energy(c, w, C.SIGMA[:2], R.grid_points(axes), periods=per)
    assert np.abs(V + F).max() <= 1e-14 * np.abs(V).max()
    Fw = cfg.metadynamics_free_energy(c, w, C.SIGMA[:2], R.grid_points(axes), kT=0.8, kdT=2., periods=per)
    assert np.abs(R.free_energy(V, 0.8, 2.) - Fw).max() <= 1e-14 * np.abs(Fw).max()


def test_hills_visible():
    for f in (metad.hills_visible, R.hills_visible):
        pace = 5
        assert [int(f(r, pace)) for r in (1, pace, pace + 1, 2 * pace, 2 * pace + 1)] == [0, 0, 1, 1, 2]
        assert int(f(pace + 1, pace, n_walker=4)) == 4 and int(f(3 * pace + 1, pace, n_walker=4)) == 12      # walkers multiply
        assert int(f(pace + 1, pace, n_walker=4, n_initial=3)) == 7 and int(f(1, pace, n_initial=3)) == 3   # n_initial adds
        assert int(f(100 * pace + 1, pace, n_walker=2, n_initial=3, n_stored=50)) == 50                     # n_stored clips
        assert np.array_equal(f(np.array([1, 6, 11]), pace, 2, 1, 4), [1, 3, 4])
    assert isinstance(metad.hills_visible(7, 2), int)
    for bad in (dict(rounds=0, pace=2), dict(rounds=3, pace=0), dict(rounds=3, pace=2, n_walker=0), dict(rounds=3, pace=2, n_initial=-1)):
        with pytest.raises(ValueError):
            metad.hills_visible(**bad)


class Untouchable:
    """a library whose use fails the test: shape and value errors come before it"""
    @property
    def calc(self):
        raise AssertionError('the library was touched')


def test_wrapper_errors_come_before_the_library():
    c, w = C.hills(2, 5, 1)
    sg = C.SIGMA[:2]
    x = C.points_near(c, 4, 2, 2)
    axes = C.axes_over(2, (4, 3))
    lib = Untouchable()
    bad_bias = [dict(sigma=[0.1, 0.]), dict(sigma=[0.1, np.nan]), dict(sigma=np.ones(5)), dict(centers=c[:, :1]), dict(weights=w[:3]),
                dict(periods=[0., -1.]), dict(periods=[0.]), dict(points=x[:, :1]), dict(points=np.where(np.arange(8).reshape(4, 2) == 3, np.nan, x)),
                dict(n_visible=[0, 1, 2]), dict(n_visible=[0, 1, 2, 6]), dict(n_visible=[0, -1, 2, 5]), dict(hill_start=[0, 2, 4]), dict(hill_start=[1, 5]),
                dict(hill_start=[0, 3, 5]), dict(point_start=[0, 5, 4]), dict(centers=np.where(np.arange(10).reshape(5, 2) == 3, np.inf, c))]
    for kw in bad_bias:
        args = dict(centers=c, weights=w, sigma=sg, points=x, library=lib)
        args.update(kw)
        with pytest.raises(ValueError):
            metad.bias(**args)
    bad_grid = [dict(axes=axes[:1]), dict(axes=[axes[0], []]), dict(axes=[axes[0], [0., np.inf]]), dict(axes=[np.zeros(2048), np.zeros(2049)]),
                dict(checkpoints=[0, 6]), dict(checkpoints=[3, 2]), dict(checkpoints=[-1, 2]), dict(checkpoints=np.zeros((2, 2), 'i8')),
                dict(scales=np.ones(9)), dict(scales=[np.nan]), dict(want_V=False)]
    for kw in bad_grid:
        args = dict(centers=c, weights=w, sigma=sg, axes=axes, library=lib)
        args.update(kw)
        with pytest.raises(ValueError):
            metad.bias_grid(**args)
    for kw in (dict(kT=0.), dict(kT=np.inf), dict(kdT=-1.)):
        args = dict(centers=c, weights=w, sigma=sg, axes=axes, checkpoints=[5], kT=1., kdT=2., library=lib)
        args.update(kw)
        with pytest.raises(ValueError):
            metad.reweighting_offset(**args)
    for kw in (dict(rounds=[1, 2, 3]), dict(frames=x[:, :1]), dict(max_checkpoints=1), dict(rounds=[0, 1, 2, 3]), dict(pace=0)):
        args = dict(centers=c, weights=w, sigma=sg, frames=x, rounds=[1, 2, 3, 4], pace=2, kT=1., kdT=2., axes=axes, library=lib)
        args.update(kw)
        with pytest.raises(ValueError):
            metad.frame_log_weights(**args)
    with pytest.raises(ValueError):
        metad.free_energy_grid(c, w, sg, axes, kdT=2., library=lib)      # well-tempered without kT
    with pytest.raises(ValueError):
        metad.default_axes(c[:0], sg)
    with pytest.raises(ValueError):
        metad.reweighted_profile(np.zeros(3), np.zeros(4), 5, 1.)


def test_default_axes_and_profile():
    c, w = C.hills(2, 30, 4, True)
    ax = metad.default_axes(c, C.SIGMA[:2], C.periods_of(2, True), n=16)
    assert len(ax) == 2 and len(ax[0]) == 16 and len(ax[1]) == 16
    assert ax[0][0] == -np.pi and abs(ax[0][-1] - (np.pi - 2 * np.pi / 16)) < 1e-15      # one period, the end not duplicated
    assert abs(ax[1][0] - (c[:, 1].min() - 3 * C.SIGMA[1])) < 1e-6 and abs(ax[1][-1] - (c[:, 1].max() + 3 * C.SIGMA[1])) < 1e-6
    # a weighted histogram: weights 1 : 3 in two bins
    F, edges = metad.reweighted_profile(np.log([1., 1., 3., 3.]) - np.log(8.), [0.1, 0.2, 0.7, 0.8], np.array([0., 0.5, 1., 1.5]), 2.)
    assert np.allclose(F[:2], [-2. * np.log(0.25), -2. * np.log(0.75)]) and F[2] == np.inf and len(edges) == 4


@pytest.mark.parametrize('kdT', [4., 0.])
def test_reweighting_recovers_a_known_free_energy(kdT):
    """32 walkers sharing one list on U = 4 (x^2 - 1)^2 at kT = 1: overdamped Euler steps of 0.002, 20000 rounds, pace 50, frames every
    10 rounds, sigma 0.1, height 0.2, well-tempered (kdT = 4) and plain (tests/metad_cases.py: toy_run).  The yardstick's frame weights
    (grid: 501 points on [-2.5, 2.5]; the first fifth of the run dropped) give a profile over 28 bins on [-1.4, 1.4] that is compared
    with -ln of the bin averages of exp(-U), both normalised over the bins.  Measured here with RandomState seeds 1, 2, 3, max |F - U|
    in kT, reweighted / unweighted: well-tempered 0.12 / 2.48, 0.09 / 2.44, 0.16 / 2.40; plain 0.17 / 2.92, 0.13 / 2.95,
    0.18 / 2.86 (about 9 s a run).  The test runs seed 1 and requires at most 0.5 kT reweighted and at least
    2 kT unweighted: a wrong formula or an off-by-one in the prefix rule misses by an order of magnitude."""
    T = C.TOY
    c, w, frames, rounds = C.toy_run(1, kdT)
    out = R.frame_log_weights(c, w, [T['sigma']], frames, rounds, T['pace'], T['kT'], kdT, [T['grid']], n_walker=T['n_walker'])
    Fr, Fu, Fe = C.toy_profiles(frames, rounds, out['log_w'])
    err, raw = np.abs(Fr - Fe).max(), np.abs(Fu - Fe).max()
    print('kdT = %g: max |F - U| reweighted %.3f kT, unweighted %.3f kT; %d hills, %d frames, n_eff %.0f' % (kdT, err, raw, len(w), len(frames), out['n_eff']))
    assert abs(R.logsumexp(out['log_w'])) < 1e-12 and np.isfinite(Fr).all()
    assert err <= 0.5 and raw >= 2.
