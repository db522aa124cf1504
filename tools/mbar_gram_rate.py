"""Cost of one MBAR Gram pass on the GPU (upk_mbar_gram, csrc/kernels_mbar_gram.hip), of its colsum-only form and of one
self-consistent iteration in the same run, and of a float64 numpy yardstick on the host.

    python tools/mbar_gram_rate.py [--runs 3] [--threads 16] [--out FILE]

For (K, N) = (4096, 2^20), (64, 2^20) and (1024, 2^18) with d = 1 it reports
  - gram_ms, colsum_ms: upk_mbar_gram with and without G on arrays that already live on the device (torch tensors), with the
    workspace the public entry point uses for that M, between two synchronisations, best of --runs after a warm-up launch;
  - tile_ms: the device time of the k_mbar_gram_tile launches of one pass from torch's profiler (null where it records none), and
    from it the fraction of the fp64 matrix peak (78.6 TFLOP/s, the public figure for the MI355X) that N Mp (Mp + 64) FLOP -- the
    upper triangle of 64 x 64 tiles, Mp = M rounded up to 64 -- reach;
  - iteration_ms: upk_mbar_denominator + upk_mbar_free_energy, one self-consistent iteration;
  - newton_step_in_iterations: (gram_ms + colsum_ms) / iteration_ms -- a Newton step of mbar(solver='newton') is one Gram pass and
    one colsum-only pass (the check that the step lowered the gradient); the copies of a call are left out on both sides;
  - the yardstick: exp over the rows cut into --threads chunks run side by side, then W.T @ W by the BLAS numpy links, on a slab of
    rows for which W stays near 1 GB, EXTRAPOLATED in proportion to N.  The extrapolation is a multiplication, not a measurement.
Prints one JSON line per case (profiles/mbar_gram_rate.txt holds a run with its explanation); --out also writes them to a file."""
import argparse
import ctypes as ct
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
from __graft_entry__ import load_package  # noqa: E402
import mbar_reference as M                # noqa: E402
from mbar_rate import States, Samples, make_case  # noqa: E402

FP64_PEAK = 78.6e12
CASES = ((4096, 1 << 20), (64, 1 << 20), (1024, 1 << 18))


def host_gram(case, f, rows, n_thread):
    """(seconds of exp, seconds of W.T @ W) of the yardstick on the first `rows` samples"""
    v = case['values'][:rows]
    cuts = np.linspace(0, rows, n_thread + 1).astype(int)

    def chunk(i):
        a, b = cuts[i], cuts[i + 1]
        u = M.reduced_energy(v[a:b], None, case['beta'], case['rows'], case['periods'])
        D = M.denominators(u, case['n_k'], f)
        return np.exp(f[None, :] - u - D[:, None])
    t0 = time.perf_counter()
    with ThreadPoolExecutor(n_thread) as pool:
        W = np.concatenate(list(pool.map(chunk, range(n_thread))))
    t1 = time.perf_counter()
    G = W.T @ W
    t2 = time.perf_counter()
    assert np.isfinite(G).all()
    return t1 - t0, t2 - t1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=3)
    ap.add_argument('--threads', type=int, default=16)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('mbar_gram_rate.py: no GPU')
    pkg = load_package()
    lib = pkg.default_library().calc
    vp = ct.c_void_p
    lib.upk_mbar_denominator.argtypes = [vp, ct.POINTER(States), ct.POINTER(Samples), vp, vp]
    lib.upk_mbar_free_energy.argtypes = [vp, ct.POINTER(States), ct.POINTER(Samples), vp, vp]
    lib.upk_mbar_gram.argtypes = [vp, ct.POINTER(States), ct.POINTER(Samples), vp, vp, ct.c_int, vp, vp, vp, vp, ct.c_size_t]
    lib.upk_mbar_gram_rows.restype = ct.c_longlong
    lib.upk_mbar_gram_rows.argtypes = [ct.c_int, ct.c_size_t]
    lib.upk_mbar_gram_partial_bytes.restype = ct.c_size_t
    T = lib.upk_mbar_gram_tile()
    sync = torch.cuda.synchronize
    lines = ['# tools/mbar_gram_rate.py, device %s' % torch.cuda.get_device_name(0)]
    for K, N in CASES:
        case = make_case(K, N // K, 1)
        f_host = pkg.mbar.mbar(tol=0., max_iter=2, want_denominators=False, **case)['f']
        dev = lambda a, t: torch.from_numpy(np.ascontiguousarray(a, t)).cuda()      # noqa: E731
        values, beta, rows, f = dev(case['values'], 'f4'), dev(case['beta'], 'f8'), dev(case['rows'], 'f4'), dev(f_host, 'f8')
        a = dev(np.log(case['n_k'].astype('f8')) + f_host, 'f8')
        denom = torch.zeros(N, dtype=torch.float64, device='cuda'); f_out = torch.zeros(K, dtype=torch.float64, device='cuda')
        G = torch.zeros((K, K), dtype=torch.float64, device='cuda'); colsum = torch.zeros(K, dtype=torch.float64, device='cuda')
        mp = (K + T - 1) // T * T
        slab = min(65536, lib.upk_mbar_gram_rows(K, 512 << 20))      # the slab of upside_hip_mbar_gram for this M
        work = torch.zeros(lib.upk_mbar_gram_partial_bytes(K) // 8 + slab * mp, dtype=torch.float64, device='cuda')
        S = States(1, K, beta.data_ptr(), rows.data_ptr(), (ct.c_double * 8)(*([0.] * 8)))
        X = Samples(N, values.data_ptr(), None)
        stream = torch.cuda.current_stream().cuda_stream
        launches = dict(
            denominator=lambda: lib.upk_mbar_denominator(stream, S, X, a.data_ptr(), denom.data_ptr()),
            free_energy=lambda: lib.upk_mbar_free_energy(stream, S, X, denom.data_ptr(), f_out.data_ptr()),
            colsum=lambda: lib.upk_mbar_gram(stream, S, X, denom.data_ptr(), f.data_ptr(), 0, None, None, colsum.data_ptr(), None, 0),
            gram=lambda: lib.upk_mbar_gram(stream, S, X, denom.data_ptr(), f.data_ptr(), 0, None, G.data_ptr(), colsum.data_ptr(), work.data_ptr(),
                                           work.numel() * 8))
        ms = {}
        for name in ('denominator', 'free_energy', 'colsum', 'gram'):
            assert launches[name]() == 0
            sync()
            best = np.inf
            for _ in range(args.runs):
                t0 = time.perf_counter()
                assert launches[name]() == 0
                sync()
                best = min(best, time.perf_counter() - t0)
            ms[name] = 1e3 * best
        assert torch.isfinite(G).all() and torch.equal(G, G.T) and torch.isfinite(colsum).all()
        tile_ms = None
        try:
            from torch.profiler import profile, ProfilerActivity
            with profile(activities=[ProfilerActivity.CUDA]) as prof:
                assert launches['gram']() == 0
                sync()
            us = sum(e.device_time_total for e in prof.key_averages() if 'k_mbar_gram_tile' in e.key)
            tile_ms = round(us / 1e3, 3) if us > 0 else None
        except Exception as err:      # the profiler is a convenience of this tool only
            print('# torch profiler unavailable: %r' % (err,))
        flop = float(N) * mp * (mp + T)
        # the yardstick on a slab of the host's size
        n_cpu = int(min(N, 1.3e8 / K) // args.threads * args.threads)
        t_exp, t_blas = host_gram(case, f_host, n_cpu, args.threads)
        iteration = ms['denominator'] + ms['free_energy']
        out = dict(states=K, samples=N, d=1, slab_rows=int(slab), workspace_mb=round(work.numel() * 8 / 2 ** 20, 1),
                   gram_ms=round(ms['gram'], 3), colsum_ms=round(ms['colsum'], 3), tile_ms=tile_ms, tile_flop=flop,
                   tile_fraction_of_fp64_peak=None if tile_ms is None else round(flop / (tile_ms * 1e-3) / FP64_PEAK, 4),
                   whole_pass_fraction_of_fp64_peak=round(flop / (ms['gram'] * 1e-3) / FP64_PEAK, 4),
                   iteration_ms=round(iteration, 3), newton_step_in_iterations=round((ms['gram'] + ms['colsum']) / iteration, 2),
                   cpu_threads=args.threads, cpu_samples=n_cpu, cpu_exp_s=round(t_exp, 3), cpu_blas_s=round(t_blas, 3),
                   cpu_s_extrapolated_to_gpu_size=round((t_exp + t_blas) * N / n_cpu, 2),
                   speedup_extrapolated=round((t_exp + t_blas) * N / n_cpu / (ms['gram'] * 1e-3), 1))
        print(json.dumps(out)); sys.stdout.flush()
        lines.append(json.dumps(out))
        del G, work, denom
        torch.cuda.empty_cache()
    lines.append('# cpu_s_extrapolated_to_gpu_size = (cpu_exp_s + cpu_blas_s) x samples / cpu_samples: an extrapolation in proportion to N, not a measurement')
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
