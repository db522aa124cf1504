"""MBAR over the output files of an umbrella ladder run by `upside_hip`, on the GPU.

    python tools/umbrella_mbar.py --temperature 0.85 [--node cv_restraint] [--bins 40] [--tol 1e-8] [--solver newton] [--uncertainty] [--decorrelate] [--bootstrap B [--seed S] [--bootstrap-draw device [--bootstrap-block N|auto]]] w00.up ...

Every file is one window: its `cv_restraint` node (`--node`) holds the window's centre, spring constant and flat width, and its
/output/cv holds the CV series the run recorded at the frames (the CVs of /input/collective_variables; samples follow the window,
as /output does).  The node's CVs are found among the recorded ones by name; a CV of the node that was not recorded is an error that
names it.  Prints the free energy f_k of every window (in kT, f_0 = 0) and the unbiased free-energy profile along the node's first
CV (in energy units, lowest bin 0; `inf` where no sample fell).  `--uncertainty` adds the asymptotic standard deviation of
f_k - f_0 and a dF column to the profile (relative to the lowest bin; the frames are taken as uncorrelated, so give `--decorrelate`
for frames written more often than the correlation time; it is a large-sample estimate); `--bootstrap B` prints the BOOTSTRAP standard
deviation of f_k - f_0 and of the profile from B stratified resamples (every window keeps its frame count; `--seed` seeds the draw),
all solved in one batch on the GPU -- beside the asymptotic one with `--uncertainty`, in its place without; bootstrapping correlated
frames underestimates the errors, so `--decorrelate` goes with it -- or `--bootstrap-draw device --bootstrap-block auto`, which draws the
counts on the GPU as a circular block bootstrap with blocks of 5 g frames per window (mbar.block_lengths; g the statistical
inefficiency of the window's own reduced bias over all its frames) and keeps every frame; `--bootstrap-block N` sets the block length
itself, `--bootstrap-draw device` alone is the plain stratified resample drawn on the GPU (another stream of random numbers than the
default `host`); `--solver newton` converges a poorly overlapping ladder in a few
steps.  `--decorrelate` drops the start of every window up to the detected equilibration origin
t0 and keeps every ceil(g)-th frame of the rest, g the statistical inefficiency of the window's own reduced bias
(timeseries.detect_equilibration on the GPU); it prints one line per window (t0, g, frames kept) before the free energies."""
import argparse
import os
import sys
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from __graft_entry__ import load_package  # noqa: E402


def read_window(h5lite, config, path, node):
    """(series (n_frame, n_recorded), recorded names, node names, node row [center | spring_const | flat_width], periods)"""
    with h5lite.open_file(path) as t:
        inp = t.group('input')
        if 'collective_variables' not in inp:
            raise SystemExit('%s: no /input/collective_variables, so the run recorded no /output/cv' % path)
        recorded = [x.decode() for x in inp.group('collective_variables').read('names').ravel()]
        pot = inp.group('potential')
        if node not in pot:
            raise SystemExit('%s: no node %r in /input/potential' % (path, node))
        g = pot.group(node)
        names = [x.decode() for x in g.read('names').ravel()]
        row = np.concatenate([g.read(k, 'f4').ravel() for k in config.CV_RESTRAINT_VALUES])
        periods = config.cv_periods(dict(kind=g.read('kind')))
        out = t.group('output')
        if 'cv' not in out:
            raise SystemExit('%s: no /output/cv' % path)
        series = out.read('cv', 'f4')
        del g, pot, out, inp
    return series.reshape(series.shape[0], -1), recorded, names, row, periods


def own_bias(pkg, values, rows, periods, kT):
    """(bias (K, T) padded with zeros, lengths (K,)): every window's own reduced bias along its frames"""
    T = max(len(v) for v in values)
    bias = np.zeros((len(values), T))
    for k, v in enumerate(values):
        bias[k, :len(v)] = pkg.mbar.own_state_reduced_bias(v, 1. / kT, rows[k][None, :], periods, np.zeros(len(v), 'i8'))
    return bias, np.array([len(v) for v in values], 'i8')


def decorrelate(pkg, values, rows, periods, kT):
    """the kept frames of every window; prints one line per window"""
    bias, lengths = own_bias(pkg, values, rows, periods, kT)
    t0, g, n_eff = pkg.timeseries.detect_equilibration(bias, lengths=lengths)
    print('# window  equilibrated from t0  statistical inefficiency g  frames kept of')
    out = []
    for k, v in enumerate(values):
        keep = pkg.timeseries.subsample_indices(len(v), t0[k], g[k])
        print('#%4d  %8d  %12.4f  %7d  %7d' % (k, t0[k], g[k], len(keep), len(v)))
        out.append(v[keep])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('files', nargs='+')
    ap.add_argument('--temperature', type=float, required=True, help='the one temperature of every window (energy units)')
    ap.add_argument('--node', default='cv_restraint')
    ap.add_argument('--skip', type=int, default=0, help='frames to leave out at the start of every window')
    ap.add_argument('--bins', type=int, default=40)
    ap.add_argument('--tol', type=float, default=1e-8)
    ap.add_argument('--max-iter', type=int, default=10000)
    ap.add_argument('--solver', choices=('self-consistent', 'newton'), default='self-consistent')
    ap.add_argument('--uncertainty', action='store_true', help='print the standard deviation of f_k - f_0 and a dF column of the profile')
    ap.add_argument('--decorrelate', action='store_true', help='detect equilibration and subsample every window to uncorrelated frames first')
    ap.add_argument('--bootstrap', type=int, default=0, metavar='B', help='print bootstrap standard deviations from B stratified resamples')
    ap.add_argument('--seed', type=int, default=0, help='the seed of the bootstrap resamples')
    ap.add_argument('--bootstrap-draw', choices=('host', 'device'), default='host', help='where the bootstrap counts are drawn')
    ap.add_argument('--bootstrap-block', default=None, metavar='N|auto', help='block length of the circular block bootstrap (with --bootstrap-draw device)')
    args = ap.parse_args()
    if args.bootstrap_block is not None and args.bootstrap_draw != 'device':
        raise SystemExit('--bootstrap-block needs --bootstrap-draw device')
    if args.bootstrap_block == 'auto' and args.decorrelate:
        raise SystemExit('--bootstrap-block auto with --decorrelate: the kept frames are already uncorrelated')
    if args.bootstrap_block not in (None, 'auto'):
        try:
            args.bootstrap_block = int(args.bootstrap_block)
        except ValueError:
            raise SystemExit('--bootstrap-block takes a block length or auto, got %r' % args.bootstrap_block)
    pkg = load_package()
    values, rows, n_k, names0, periods0 = [], [], [], None, None
    for path in args.files:
        series, recorded, names, row, periods = read_window(pkg.h5lite, pkg.config, path, args.node)
        for nm in names:
            if nm not in recorded:
                raise SystemExit('%s: the collective variable %r of node %r is not among the recorded ones %r' % (path, nm, args.node, recorded))
        if names0 is None:
            names0, periods0 = names, periods
        elif names != names0:
            raise SystemExit('%s: the CVs of node %r are %r, the first file has %r' % (path, args.node, names, names0))
        v = series[args.skip:, [recorded.index(nm) for nm in names]]
        values.append(v); rows.append(row); n_k.append(len(v))
    kT = args.temperature
    if args.decorrelate:
        values = decorrelate(pkg, values, rows, periods0, kT)
        n_k = [len(v) for v in values]
    v = np.concatenate(values)
    problem = (v, None, 1. / kT, np.stack(rows), np.array(n_k, 'i8'))
    r = pkg.mbar.mbar(*problem, periods0, args.tol, args.max_iter, target=(1. / kT, None), solver=args.solver)
    print('# %d windows, %d samples, CVs %s; %d iterations%s, last max |df| = %.3e' %
          (len(rows), len(v), names0, r['n_iter'], ' and %d Newton steps' % r['n_newton'] if 'n_newton' in r else '', r['last_delta']))
    sigma = pkg.mbar.free_energy_uncertainty(*problem, r['f'], periods0) if args.uncertainty else None
    sigma_boot, counts = None, None
    if args.bootstrap > 0:      # the windows are concatenated, so the samples are grouped by window: the default origins
        import warnings
        block = args.bootstrap_block
        if block == 'auto':
            bias, lengths = own_bias(pkg, values, rows, periods0, kT)
            g = pkg.timeseries.statistical_inefficiency(bias, lengths=lengths)['g'][:, 0]
            block = pkg.mbar.block_lengths(g)
            print('# bootstrap blocks: statistical inefficiency g = %s, block lengths %s' % (np.round(g, 3).tolist(), block.tolist()))
        drawn = dict(draw=args.bootstrap_draw, block=block)
        boot = pkg.mbar.bootstrap(*problem, r['f'], n_bootstrap=args.bootstrap, seed=args.seed, periods=periods0, tol=args.tol, max_iter=args.max_iter, **drawn)
        counts = boot.get('counts')      # (drawn on the device, the same seed gives the profile below the same counts)
        with warnings.catch_warnings():
            warnings.simplefilter('ignore', RuntimeWarning)
            sigma_boot = pkg.mbar.bootstrap_sigma(boot)
        print('# bootstrap: %d replicates (seed %d), %d converged, %d .. %d iterations' %
              (args.bootstrap, args.seed, int(boot['converged'].sum()), boot['n_iter'].min(), boot['n_iter'].max()))
    print('# window  centre(%s)  samples  f_k / kT%s%s' % (names0[0], '  sigma(f_k - f_0)' if args.uncertainty else '', '  bootstrap sigma(f_k - f_0)' if args.bootstrap > 0 else ''))
    for k, (row, n) in enumerate(zip(rows, n_k)):
        print('%4d  %12.6g  %7d  %14.8f%s%s' % (k, row[0], n, r['f'][k], '  %12.6f' % sigma[k, 0] if args.uncertainty else '',
                                               '  %12.6f' % sigma_boot[k, 0] if args.bootstrap > 0 else ''))
    x = v[:, 0].astype('f8')
    if periods0[0] > 0:
        edges = np.linspace(-0.5 * periods0[0], 0.5 * periods0[0], args.bins + 1)
    else:
        edges = np.linspace(x.min(), np.nextafter(x.max(), np.inf), args.bins + 1)
    dF = None
    if args.uncertainty:
        prof, dF = pkg.mbar.profile(*problem, r['f'], edges, kT, period=periods0[0], target=(1. / kT, None), periods=periods0, cv=0)
    else:
        prof = pkg.config.mbar_profile(x, r['log_w'], edges, kT, period=periods0[0])
    dF_boot = None
    if args.bootstrap > 0:
        _, dF_boot = pkg.mbar.profile_bootstrap(*problem, r['f'], edges, kT, period=periods0[0], target=(1. / kT, None), periods=periods0, cv=0, counts=counts,
                                                n_bootstrap=args.bootstrap, seed=args.seed, tol=args.tol, max_iter=args.max_iter, **drawn)
    prof = prof - prof[np.isfinite(prof)].min()
    print('# unbiased profile along %s: bin centre, F%s%s' % (names0[0], ', dF' if args.uncertainty else '', ', bootstrap dF' if args.bootstrap > 0 else ''))
    for b in range(args.bins):
        print('%12.6g  %12.6f%s%s' % (0.5 * (edges[b] + edges[b + 1]), prof[b], '  %12.6f' % dF[b] if args.uncertainty else '',
                                     '  %12.6f' % dF_boot[b] if args.bootstrap > 0 else ''))


if __name__ == '__main__':
    main()
