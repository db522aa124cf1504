"""Cost of bootstrap error bars of MBAR on the GPU: all replicates in one device batch (mbar.bootstrap, upside_hip_mbar_bootstrap,
csrc/kernels_mbar_boot.hip) against what could be written before it, a Python loop of mbar.mbar over physically resampled copies of
the samples.

    python tools/mbar_bootstrap_rate.py [--shapes a,b,c] [--runs 3] [--out FILE]

Shapes (d = 1, harmonic windows along the CV with overlapping neighbours, samples grouped by window):
  a   K = 32,   N = 32 x 2048 = 65536,  B = 256 replicates     decorrelated sizes: a single problem leaves the device nearly empty
  b   K = 256,  N = 2^18,               B = 64
  c   K = 4096, N = 2^20,               B = 8                  a single problem already fills the device
Both sides solve the same resamples (mbar.bootstrap_counts, seed 1) from the same start f with the same tol and max_iter, which are
reported with the iterations the replicates took; the loop's replicate b is mbar.mbar(values[np.repeat(arange(N), counts[b])], ...,
f0=f).  Each side is timed as a whole (host work, copies and synchronisations included), best of --runs after one warm-up; the
spread (max - min of the timed runs) is reported for both.  Also: the host time of bootstrap_counts.  Prints one JSON line per
shape (profiles/mbar_bootstrap_rate.txt holds a run with its explanation); --out also writes them to a file."""
import argparse
import json
import os
import sys
import time
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from __graft_entry__ import load_package  # noqa: E402

#            K, samples per window, B, tol, max_iter of the replicates, iterations of the start
SHAPES = dict(a=(32, 2048, 256, 1e-8, 1000, 20000),
              b=(256, 1024, 64, 1e-8, 300, 20000),
              c=(4096, 256, 8, 1e-8, 10, 100))


def make_case(K, per_state, seed=1):
    """K harmonic windows (spring 4, kT 0.8) along one CV, neighbours at most 0.6 apart; float32 samples drawn around their window"""
    rng = np.random.RandomState(seed)
    centers = 4. + min(0.6, 26. / max(K - 1, 1)) * np.arange(K)
    owner = np.repeat(np.arange(K), per_state)
    v = centers[owner] + rng.normal(0., 0.5, K * per_state)
    rows = np.column_stack((centers, np.full(K, 4.0), np.zeros(K))).astype('f4')
    return dict(values=v.astype('f4')[:, None], energy=None, beta=np.full(K, 1.25), rows=rows, n_k=np.full(K, per_state, 'i8'), periods=np.zeros(1))


def timed(fn, runs, label):
    fn()      # warm-up
    t = []
    for i in range(runs):
        t0 = time.perf_counter()
        out = fn()
        t.append(time.perf_counter() - t0)
        print('#   %s run %d: %.3f s' % (label, i, t[-1])); sys.stdout.flush()
    return min(t), max(t) - min(t), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', default='a,b,c')
    ap.add_argument('--runs', type=int, default=3)
    ap.add_argument('--out', default=None, help='also write the JSON lines to this file')
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('mbar_bootstrap_rate.py: no GPU')
    pkg = load_package()
    mb = pkg.mbar
    lines = ['# tools/mbar_bootstrap_rate.py --shapes %s --runs %d, device %s' % (args.shapes, args.runs, torch.cuda.get_device_name(0))]
    for name in args.shapes.split(','):
        K, per, B, tol, max_iter, start_iter = SHAPES[name]
        case = make_case(K, per)
        N = K * per
        start = mb.mbar(tol=tol, max_iter=start_iter, want_denominators=False, **case)
        f = start['f']
        t0 = time.perf_counter()
        counts = mb.bootstrap_counts(case['n_k'], B, seed=1)
        t_counts = time.perf_counter() - t0
        print('# shape %s: K = %d, N = %d, B = %d; start after %d iterations (last delta %.2e); bootstrap_counts %.3f s' %
              (name, K, N, B, start['n_iter'], start['last_delta'], t_counts)); sys.stdout.flush()

        def batch():
            return mb.bootstrap(f=f, counts=counts, tol=tol, max_iter=max_iter, **case)

        def loop():
            out = np.zeros((B, K)); its = np.zeros(B, 'i8')
            everyone = np.arange(N)
            for b in range(B):
                idx = np.repeat(everyone, counts[b])
                r = mb.mbar(case['values'][idx], None, case['beta'], case['rows'], case['n_k'], case['periods'], tol, max_iter, f0=f, want_denominators=False)
                out[b] = r['f']; its[b] = r['n_iter']
            return out, its

        t_batch, s_batch, got = timed(batch, args.runs, 'batch')
        t_loop, s_loop, (f_loop, it_loop) = timed(loop, args.runs, 'loop ')
        assert np.isfinite(got['f_boot']).all() and np.isfinite(f_loop).all()
        out = dict(shape=name, states=K, samples=N, replicates=B, d=1, tol=tol, max_iter=max_iter,
                   iterations_batch=[int(got['n_iter'].min()), int(got['n_iter'].max())], iterations_loop=[int(it_loop.min()), int(it_loop.max())],
                   converged_batch=int(got['converged'].sum()),
                   batch_s=round(t_batch, 4), batch_spread_s=round(s_batch, 4), loop_s=round(t_loop, 4), loop_spread_s=round(s_loop, 4),
                   loop_over_batch=round(t_loop / t_batch, 2), loop_minus_batch_s=round(t_loop - t_batch, 4),
                   largest_difference_of_f=float(np.abs(got['f_boot'] - f_loop).max()),
                   bootstrap_counts_host_s=round(t_counts, 4))
        print(json.dumps(out)); sys.stdout.flush()
        lines.append(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
