"""Cost of one MBAR iteration on the GPU (upside_hip_mbar, csrc/kernels_mbar.hip) at the engine's natural size, and of the float64
numpy yardstick on the host for comparison.

    python tools/mbar_rate.py [--states 4096] [--samples-per-state 256] [--out FILE]

For d = 1, d = 2 (one CV periodic) and d = 0 with energies it reports
  - the time per iteration of the whole call: (t(max_iter = 6) - t(max_iter = 2)) / 4 with tol = 0, which leaves out the one copy of the
    samples, the allocations and the final pass; best of --runs;
  - the time of each pass alone: upk_mbar_denominator and upk_mbar_free_energy launched on arrays that already live on the device
    (torch tensors), between two synchronisations, best of --runs after a warm-up launch;
  - the yardstick tests/mbar_reference.py (float64 numpy) on this machine's CPUs, the samples cut into --threads chunks that run side
    by side and are combined by one more logsumexp, at the largest sample count for which one iteration stays near --cpu-seconds,
    and that time EXTRAPOLATED in proportion to N x K to the GPU's size.  The extrapolation is a multiplication, not a measurement.
Prints one JSON line per case (profiles/mbar_rate.txt holds a run with its explanation); --out also writes them to a file."""
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
from __graft_entry__ import load_package  # noqa: E402
import mbar_reference as M                # noqa: E402


class States(ct.Structure):      # upk_mbar_states_t
    _fields_ = [('d', ct.c_int), ('n_state', ct.c_int), ('beta', ct.c_void_p), ('rows', ct.c_void_p), ('period', ct.c_double * 8)]


class Samples(ct.Structure):     # upk_mbar_samples_t
    _fields_ = [('n', ct.c_longlong), ('values', ct.c_void_p), ('energy', ct.c_void_p)]


def make_case(K, per_state, d, seed=1):
    """K windows spread along the first CV with neighbouring windows overlapping; float32 samples drawn around their window"""
    rng = np.random.RandomState(seed)
    N = K * per_state
    owner = np.repeat(np.arange(K), per_state)
    case = dict(values=None, energy=None, rows=None, periods=None, n_k=np.full(K, per_state, 'i8'))
    if d == 0:
        T = np.geomspace(0.6, 1.2, K)
        case.update(energy=rng.normal(-300. + 250. * (T[owner] - 0.6), 8., N), beta=1. / T)
        return case
    centers = np.zeros((K, d)); spring = np.full((K, d), 4.0); flat = np.zeros((K, d))
    centers[:, 0] = np.linspace(-3.0, 3.0, K) if d == 2 else np.linspace(4., 30., K)
    if d == 2:
        centers[:, 1] = 8. + np.sin(np.arange(K) * 0.01); flat[:, 1] = 0.2
    v = centers[owner] + rng.normal(0., 0.5, (N, d))
    periods = np.zeros(d)
    if d == 2:
        periods[0] = 2 * np.pi; v[:, 0] -= 2 * np.pi * np.rint(v[:, 0] / (2 * np.pi))
    case.update(values=v.astype('f4'), rows=np.concatenate((centers, spring, flat), 1).astype('f4'), periods=periods, beta=np.full(K, 1.25))
    return case


def cpu_iteration(case, n_thread):
    """one yardstick iteration from f = 0 with the samples cut into n_thread chunks; seconds"""
    K = len(case['n_k'])
    N = len(case['values']) if case['values'] is not None else len(case['energy'])
    v = case['values'] if case['values'] is not None else np.zeros((N, 0), 'f4')
    f = np.zeros(K)
    cuts = np.linspace(0, N, n_thread + 1).astype(int)

    def chunk(i):
        a, b = cuts[i], cuts[i + 1]
        u = M.reduced_energy(v[a:b], None if case['energy'] is None else case['energy'][a:b], case['beta'], case['rows'], case['periods'])
        D = M.denominators(u, case['n_k'], f)
        return M.logsumexp(-u - D[:, None], axis=0)
    t0 = time.perf_counter()
    with ThreadPoolExecutor(n_thread) as pool:
        cols = list(pool.map(chunk, range(n_thread)))
    fn = -M.logsumexp(np.stack(cols), axis=0)
    fn -= fn[0]
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--states', type=int, default=4096)
    ap.add_argument('--samples-per-state', type=int, default=256)
    ap.add_argument('--runs', type=int, default=3)
    ap.add_argument('--threads', type=int, default=16)
    ap.add_argument('--cpu-seconds', type=float, default=20.)
    ap.add_argument('--out', default=None, help='also write the JSON lines to this file (profiles/mbar_rate.txt holds them with their explanation)')
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('mbar_rate.py: no GPU')
    pkg = load_package()
    lib = pkg.default_library().calc
    pkg.mbar._bind(lib)
    vp = ct.c_void_p
    lib.upk_mbar_denominator.argtypes = [vp, ct.POINTER(States), ct.POINTER(Samples), vp, vp]
    lib.upk_mbar_free_energy.argtypes = [vp, ct.POINTER(States), ct.POINTER(Samples), vp, vp]
    K, per = args.states, args.samples_per_state
    N = K * per
    sync = torch.cuda.synchronize
    lines = ['# tools/mbar_rate.py --states %d --samples-per-state %d (N = %d, N x K = %.3e), device %s' % (K, per, N, float(N) * K, torch.cuda.get_device_name(0))]
    for d in (1, 2, 0):
        case = make_case(K, per, d)
        call = {}
        for it in (2, 6):
            best = np.inf
            for _ in range(args.runs):
                t0 = time.perf_counter()
                r = pkg.mbar.mbar(tol=0., max_iter=it, want_denominators=False, **case)
                best = min(best, time.perf_counter() - t0)
            assert r['n_iter'] == it and np.isfinite(r['f']).all()
            call[it] = best
        # the two passes alone, on device-resident arrays
        dev = lambda a, t: None if a is None else torch.from_numpy(np.ascontiguousarray(a, t)).cuda()      # noqa: E731
        values, energy, beta, rows = dev(case['values'], 'f4'), dev(case['energy'], 'f8'), dev(case['beta'], 'f8'), dev(case['rows'], 'f4')
        a = torch.from_numpy(np.log(case['n_k'].astype('f8'))).cuda()
        denom = torch.zeros(N, dtype=torch.float64, device='cuda'); f = torch.zeros(K, dtype=torch.float64, device='cuda')
        ptr = lambda t: None if t is None else t.data_ptr()      # noqa: E731
        S = States(d, K, ptr(beta), ptr(rows), (ct.c_double * 8)(*(list(case['periods']) if d else []) + [0.] * (8 - d)))
        X = Samples(N, ptr(values), ptr(energy))
        stream = torch.cuda.current_stream().cuda_stream
        passes = {}
        for name, launch in (('denominator', lambda: lib.upk_mbar_denominator(stream, S, X, a.data_ptr(), denom.data_ptr())),
                             ('free_energy', lambda: lib.upk_mbar_free_energy(stream, S, X, denom.data_ptr(), f.data_ptr()))):
            assert launch() == 0
            sync()
            best = np.inf
            for _ in range(args.runs):
                t0 = time.perf_counter()
                assert launch() == 0
                sync()
                best = min(best, time.perf_counter() - t0)
            passes[name] = best
        assert torch.isfinite(f).all() and torch.isfinite(denom).all()
        # the yardstick on the host
        probe = dict(case)
        sel = np.arange(0, N, max(1, N // 4096))[:4096]
        for k in ('values', 'energy'):
            probe[k] = None if case[k] is None else case[k][sel]
        t1 = cpu_iteration(probe, args.threads)
        n_cpu = int(min(N, max(len(sel), len(sel) * args.cpu_seconds / t1, 1), 1.3e8 / K) // args.threads * args.threads)      # (1.3e8 / K: an N x K matrix of doubles stays near 1 GB)
        sel = np.arange(0, N, max(1, N // n_cpu))[:n_cpu]
        for k in ('values', 'energy'):
            probe[k] = None if case[k] is None else case[k][sel]
        t_cpu = cpu_iteration(probe, args.threads)
        per_iter = (call[6] - call[2]) / 4.
        out = dict(d=d, with_energy=bool(d == 0), states=K, samples=N, gpu_ms_per_iteration=round(1e3 * per_iter, 3),
                   gpu_call_ms={'max_iter_2': round(1e3 * call[2], 2), 'max_iter_6': round(1e3 * call[6], 2)},
                   gpu_pass_ms=dict((k, round(1e3 * t, 3)) for k, t in passes.items()),
                   dominant_pass=max(passes, key=passes.get),
                   pair_evaluations_per_second=round(float(N) * K / per_iter, -6),
                   cpu_threads=args.threads, cpu_samples=len(sel), cpu_s_per_iteration=round(t_cpu, 3),
                   cpu_s_per_iteration_extrapolated_to_gpu_size=round(t_cpu * N / len(sel), 1),
                   speedup_extrapolated=round(t_cpu * N / len(sel) / per_iter, 1))
        print(json.dumps(out)); sys.stdout.flush()
        lines.append(json.dumps(out))
    lines.append('# cpu_s_per_iteration_extrapolated_to_gpu_size = cpu_s_per_iteration x samples / cpu_samples: an extrapolation in proportion to N x K, not a measurement')
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
