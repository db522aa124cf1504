"""Cost of bootstrap error bars of MBAR on the GPU: all replicates in one device batch (mbar.bootstrap, upside_hip_mbar_bootstrap,
csrc/kernels_mbar_boot.hip) against what could be written before it, a Python loop of mbar.mbar over physically resampled copies of
the samples.

    python tools/mbar_bootstrap_rate.py [--shapes a,b,c] [--runs 3] [--out FILE]
    python tools/mbar_bootstrap_rate.py --draw [--shapes a,b,c,d] [--runs 3] [--out FILE]

Shapes (d = 1, harmonic windows along the CV with overlapping neighbours, samples grouped by window):
  a   K = 32,   N = 32 x 2048 = 65536,  B = 256 replicates     decorrelated sizes: a single problem leaves the device nearly empty
  b   K = 256,  N = 2^18,               B = 64
  c   K = 4096, N = 2^20,               B = 8                  a single problem already fills the device
  d   K = 64,   N = 2^20,               B = 200                (--draw only) a production ladder: the counts are a 419 MB host array
Both sides solve the same resamples (mbar.bootstrap_counts, seed 1) from the same start f with the same tol and max_iter, which are
reported with the iterations the replicates took; the loop's replicate b is mbar.mbar(values[np.repeat(arange(N), counts[b])], ...,
f0=f).  Each side is timed as a whole (host work, copies and synchronisations included), best of --runs after one warm-up; the
spread (max - min of the timed runs) is reported for both.  Also: the host time of bootstrap_counts.  Prints one JSON line per
shape (profiles/mbar_bootstrap_rate.txt holds a run with its explanation); --out also writes them to a file.

--draw measures where the counts are drawn instead (profiles/mbar_boot_draw_rate.txt), each figure after one warm-up as the minimum
and the median of --runs repeats:
  the draw alone   mbar.bootstrap_counts on the host (wall clock) against the device draw, upk_mbar_boot_draw into device buffers in the
                   chunks the solve uses, timed with device events (block length 1 and 45);
  the whole call   mbar.bootstrap with tol = 0 and the shape's max_iter (every replicate runs max_iter iterations on every path), with
                   draw='host' (bootstrap_counts inside the timed call), with the host's counts given (the batch_s of the run without
                   --draw: it shows whether the old path moved) and with draw='device' at block length 1 and 45."""
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
              c=(4096, 256, 8, 1e-8, 10, 100),
              d=(64, 16384, 200, 1e-8, 20, 2000))


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


def repeats(fn, runs, label, clock=None):
    """[seconds] of `runs` calls of fn after one warm-up; clock(fn) returns the seconds of one call (default: wall clock), and the last result"""
    def wall(f):
        t0 = time.perf_counter()
        out = f()
        return time.perf_counter() - t0, out
    clock = clock or wall
    fn()
    t, out = [], None
    for i in range(runs):
        dt, out = clock(fn)
        t.append(dt)
        print('#   %s run %d: %.4f s' % (label, i, dt)); sys.stdout.flush()
    return t, out


def min_median(t):
    return [round(min(t), 4), round(sorted(t)[len(t) // 2], 4)]


def device_draw(pkg, torch, n_k, B, seed, block):
    """a callable that draws B replicates into device buffers with upk_mbar_boot_draw, chunked as the solve chunks them"""
    import ctypes as ct
    c = pkg.default_library().calc
    vp, i32, i64, u64 = ct.c_void_p, ct.c_int, ct.c_longlong, ct.c_ulonglong
    c.upk_mbar_boot_draw.argtypes = [vp, i32, i64, vp, vp, vp, i32, ct.c_uint, u64, i64, vp, vp, vp]
    c.upk_mbar_boot_draw.restype = i32
    K, N = len(n_k), int(n_k.sum())
    chunk = min(B, pkg.mbar.boot_chunk(N, 512 << 20))
    dev = dict(device='cuda')
    start = torch.tensor(np.concatenate(([0], np.cumsum(n_k))), dtype=torch.int32, **dev)
    length = torch.tensor(np.minimum(block, np.maximum(n_k, 1)), dtype=torch.int32, **dev)
    scratch = torch.zeros(chunk * N, dtype=torch.int32, **dev)
    counts = torch.zeros(chunk * N, dtype=torch.int16, **dev)
    flag = torch.full((1,), -1, dtype=torch.int64, **dev)

    def run():
        for b0 in range(0, B, chunk):
            rc = c.upk_mbar_boot_draw(None, K, N, start.data_ptr(), length.data_ptr(), None, min(chunk, B - b0), b0, seed, int(n_k.max()),
                                      scratch.data_ptr(), counts.data_ptr(), flag.data_ptr())
            assert rc == 0, rc
        return counts
    return run


def draw_rates(args, pkg, torch):
    mb = pkg.mbar
    lines = ['# tools/mbar_bootstrap_rate.py --draw --shapes %s --runs %d, device %s' % (args.shapes, args.runs, torch.cuda.get_device_name(0))]

    def events(fn):      # device time of one call on the default stream
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); out = fn(); e1.record(); e1.synchronize()
        return e0.elapsed_time(e1) * 1e-3, out

    for name in args.shapes.split(','):
        K, per, B, tol, max_iter, start_iter = SHAPES[name]
        case = make_case(K, per)
        N, n_k = K * per, case['n_k']
        f = mb.mbar(tol=tol, max_iter=start_iter, want_denominators=False, **case)['f']
        print('# shape %s: K = %d, N = %d, B = %d, max_iter = %d' % (name, K, N, B, max_iter)); sys.stdout.flush()
        out = dict(shape=name, states=K, samples=N, replicates=B, d=1, max_iter=max_iter, counts_array_MB=round(2e-6 * B * N, 1))
        t, counts = repeats(lambda: mb.bootstrap_counts(n_k, B, seed=1), args.runs, 'host draw')
        out['draw_host_s'] = min_median(t)
        for L in (1, 45):
            t, drawn = repeats(device_draw(pkg, torch, n_k, B, 1, np.full(K, L)), args.runs, 'device draw, L = %d' % L, events)
            out['draw_device_L%d_s' % L] = [round(min(t), 6), round(sorted(t)[len(t) // 2], 6)]
            last = min(B, mb.boot_chunk(N, 512 << 20)); last = B - (B - 1) // last * last      # the replicates of the last chunk are what the buffer holds
            want = mb.bootstrap_counts_device(n_k, last, seed=1, block=L, first=B - last)
            assert np.array_equal(drawn.cpu().numpy().view('u2')[:last * N].reshape(last, N), want)
        kw = dict(case, f=f, tol=0., max_iter=max_iter)
        calls = (('call_host_s', dict(n_bootstrap=B, seed=1)), ('call_host_counts_given_s', dict(counts=counts)),
                 ('call_device_L1_s', dict(n_bootstrap=B, seed=1, draw='device')), ('call_device_L45_s', dict(n_bootstrap=B, seed=1, draw='device', block=45)))
        for key, extra in calls:
            t, got = repeats(lambda: mb.bootstrap(**dict(kw, **extra)), args.runs, key)
            assert np.isfinite(got['f_boot']).all() and (got['n_iter'] == max_iter).all()
            out[key] = min_median(t)
        print(json.dumps(out)); sys.stdout.flush()
        lines.append(json.dumps(out))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', default=None, help='default a,b,c (a,b,c,d with --draw)')
    ap.add_argument('--draw', action='store_true', help='measure where the counts are drawn: host against device')
    ap.add_argument('--runs', type=int, default=3)
    ap.add_argument('--out', default=None, help='also write the JSON lines to this file')
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('mbar_bootstrap_rate.py: no GPU')
    pkg = load_package()
    mb = pkg.mbar
    if args.shapes is None:
        args.shapes = 'a,b,c,d' if args.draw else 'a,b,c'
    if args.draw:
        lines = draw_rates(args, pkg, torch)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, 'w') as fh:
                fh.write('\n'.join(lines) + '\n')
        return
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
