"""Free energies from a metadynamics run of `upside_hip`, on the GPU (metad.py; upside_hip_metad_bias and upside_hip_metad_grid).

    python tools/metad_reweight.py RUN.up [MORE.up ...] --node cv_metadynamics --temperature KT --every ROUNDS
                                   [--along NAME --bins N] [--grid N] [--skip FRAMES] [--max-checkpoints M]

Every file is one system of a finished run: /input/potential/<node> holds the node (its CVs by name, sigma, pace, kdT, shared),
/output/metadynamics/<node> the hills at the end, /output/cv the CV series the run recorded at its frames (the CVs of
/input/collective_variables) and /input/metadynamics/<node>, where present, the hills the run started from.  /output/cv does not
carry the recording interval, so `--every` gives the MD rounds between two frames (frame interval / (3 x time step)); frame f was
recorded at completed round f x every, and frame 0, the starting structure, is left out (`--skip` leaves out more).
It prints
  - F_hills on a grid of --grid points per biased CV (metad.default_axes over the hills): -(kT + kdT) / kdT V for a well-tempered
    run, -V for a plain one, relative to its minimum;
  - with --along NAME, the reweighted free-energy profile along ANY recorded CV, -kT ln of the histogram of the frames weighted by
    exp((V(s_n, t_n) - c(t_n)) / kT) (Tiwary & Parrinello 2015), in --bins bins, relative to its minimum, with the Kish effective
    sample size.
A node with a list per system (shared = 0) is analysed file by file; the files of a shared list (shared = 1: give all the walkers'
files, in the engine's order) are pooled, with the hills of the first file.  c(t) is interpolated where a run has more than
--max-checkpoints distinct hill counts; the weights of plain metadynamics are defined but do not converge in the long-time limit."""
import argparse
import os
import sys
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from __graft_entry__ import load_package  # noqa: E402


def read_run(h5lite, path, node):
    """(series (n_frame, n_recorded), recorded names, centers, weights, n_initial)"""
    with h5lite.open_file(path) as t:
        inp = t.group('input')
        if 'collective_variables' not in inp:
            raise SystemExit('%s: no /input/collective_variables, so the run recorded no /output/cv' % path)
        recorded = [x.decode() for x in inp.group('collective_variables').read('names').ravel()]
        n_initial = 0
        if 'metadynamics' in inp and node in inp.group('metadynamics'):
            n_initial = len(inp.group('metadynamics').group(node).read('hill_weight', 'f4').ravel())
        out = t.group('output')
        if 'cv' not in out:
            raise SystemExit('%s: no /output/cv' % path)
        if 'metadynamics' not in out or node not in out.group('metadynamics'):
            raise SystemExit('%s: no /output/metadynamics/%s' % (path, node))
        m = out.group('metadynamics').group(node)
        w = m.read('hill_weight', 'f4').ravel()
        c = m.read('hill_center', 'f4').reshape(len(w), -1)
        series = out.read('cv', 'f4')
        del m, out, inp
    return series.reshape(series.shape[0], -1), recorded, c, w, n_initial


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('files', nargs='+')
    ap.add_argument('--node', default='cv_metadynamics')
    ap.add_argument('--temperature', type=float, required=True, help='kT of the run (energy units)')
    ap.add_argument('--every', type=int, required=True, help='MD rounds between two frames of /output/cv')
    ap.add_argument('--along', default=None, help='a recorded CV to print the reweighted profile along')
    ap.add_argument('--bins', type=int, default=30)
    ap.add_argument('--grid', type=int, default=64, help='grid points per biased CV')
    ap.add_argument('--skip', type=int, default=1, help='frames to leave out at the start (at least 1: frame 0 is the starting structure)')
    ap.add_argument('--max-checkpoints', type=int, default=4096)
    args = ap.parse_args()
    if args.every < 1 or args.skip < 1 or args.bins < 1 or args.grid < 1:
        raise SystemExit('--every, --skip, --bins and --grid must be at least 1')
    pkg = load_package()
    metad, cfg = pkg.metad, pkg.config
    kT = args.temperature
    p = cfg.metad_node_parameters(args.files[0], args.node)
    d = len(p['names'])
    runs = [read_run(pkg.h5lite, path, args.node) for path in args.files]
    for path, (series, recorded, c, w, n0) in zip(args.files, runs):
        for nm in p['names'] + ([args.along] if args.along else []):
            if nm not in recorded:
                raise SystemExit('%s: the collective variable %r is not among the recorded ones %r' % (path, nm, recorded))
        if len(series) <= args.skip:
            raise SystemExit('%s: %d frames, none left after --skip %d' % (path, len(series), args.skip))
        if not len(w):
            raise SystemExit('%s: /output/metadynamics/%s holds no hills' % (path, args.node))
    groups = [list(range(len(runs)))] if p['shared'] else [[i] for i in range(len(runs))]
    for grp in groups:
        series0, recorded, c, w, n0 = runs[grp[0]]
        cols = [recorded.index(nm) for nm in p['names']]
        axes = metad.default_axes(c, p['sigma'], p['periods'], n=args.grid)
        F = metad.free_energy_grid(c, w, p['sigma'], axes, kT, p['kdT'], p['periods'])
        what = ', '.join(args.files[i] for i in grp)
        print('# %s: node %s, %d hills (%d before the run), %s, kdT %g, pace %d' % (what, args.node, len(w), n0, 'shared by %d walkers' % len(grp) if p['shared'] else 'own list',
                                                                                    p['kdT'], p['pace']))
        print('# F_hills over %s, relative to its minimum: %s, F' % (' x '.join(str(len(a)) for a in axes), ', '.join(p['names'])))
        F = F - F.min()
        for idx in np.ndindex(*F.shape):
            print(' '.join('%.6g' % axes[k][i] for k, i in enumerate(idx)) + ' %.6g' % F[idx])
        if not args.along:
            continue
        n = min(len(runs[i][0]) for i in grp)
        rounds = np.arange(args.skip, n) * args.every
        S = len(grp)
        frames = np.stack([runs[i][0][args.skip:n][:, cols] for i in grp], axis=1).reshape(-1, d)      # (frame-major, the walkers side by side)
        along = np.stack([runs[i][0][args.skip:n][:, recorded.index(args.along)] for i in grp], axis=1).reshape(-1)
        r = metad.frame_log_weights(c, w, p['sigma'], frames, np.repeat(rounds, S), p['pace'], kT, p['kdT'], axes, n_walker=S, n_initial=n0, periods=p['periods'],
                                    max_checkpoints=args.max_checkpoints)
        prof, edges = metad.reweighted_profile(r['log_w'], along, args.bins, kT)
        print('# reweighted profile along %s from %d frames, effective sample size %.1f, c(t) at %d hill counts from %.4g to %.4g: bin centre, F' %
              (args.along, len(along), r['n_eff'], len(r['checkpoints']), r['c_checkpoints'][0], r['c_checkpoints'][-1]))
        prof = prof - prof[np.isfinite(prof)].min()
        for k in range(len(prof)):
            print('%.6g %s' % (0.5 * (edges[k] + edges[k + 1]), '%.6g' % prof[k] if np.isfinite(prof[k]) else 'inf'))


if __name__ == '__main__':
    main()
