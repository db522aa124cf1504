"""Cost of equilibration detection on the GPU (upside_hip_series_inefficiency, csrc/kernels_series.hip) and of a float64 numpy
yardstick on the host.

    python tools/series_rate.py [--runs 3] [--threads 16] [--cpu-series 64,16] [--out FILE]
    python tools/series_rate.py --resources          (no GPU needed: the resource usage of the kernels from the compiler)

For n_series x T x n_origin = 4096 x 65536 x 64 and 64 x 2^20 x 64, AR(1) series with a correlation time of 50 rounds
(phi = exp(-1 / 50)) and the origins of timeseries.detect_equilibration, it reports from upk_series_solve (the host side of the entry
point, which fills a stats array)
  - device_ms: between two HIP events around the kernels of the call, read-backs of the per-series flags included, the copy of the
    series excluded; wall_ms: the whole call after its argument checks, the copy of the series included; call_ms: the call as the
    caller sees it, the scan for entries that are not finite included.  Best of --runs after a warm-up call;
  - lag_blocks, series_blocks: launches over blocks of 128 lags and the unfinished series summed over them; stop lags seen;
  - tile_ms: the device time of the k_series_lags launches of one call from torch's profiler (null where it records none), and the
    fraction of the fp64 matrix peak (78.6 TFLOP/s, the public figure for the MI355X) that its 2048 FLOP per v_mfma_f64_16x16x4_f64
    reach;
  - the yardstick: per (series, origin) the autocorrelation of the tail by FFT (numpy.fft, zero-padded to a power of two), the way a
    careful user would do it on the host, over --threads threads, on the first --cpu-series series of each case, EXTRAPOLATED in
    proportion to n_series.  The extrapolation is a multiplication, not a measurement.  Its g and stop lags are compared with the
    device's on those series.
Prints one JSON line per case (profiles/series_rate.txt holds a run with its explanation); --out also writes them to a file."""
import argparse
import ctypes as ct
import json
import os
import re
import subprocess
import sys
import time
from concurrent.futures import ThreadPoolExecutor
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from __graft_entry__ import load_package  # noqa: E402

FP64_PEAK = 78.6e12
CASES = ((4096, 1 << 16, 64), (64, 1 << 20, 64))
TAU = 50.


class Problem(ct.Structure):
    _fields_ = [('n_series', ct.c_int), ('stride', ct.c_longlong), ('length', ct.c_void_p), ('a', ct.c_void_p), ('n_origin', ct.c_int),
                ('origin', ct.c_void_p), ('mintime', ct.c_int), ('max_lag', ct.c_longlong), ('g', ct.c_void_p), ('stop_lag', ct.c_void_p),
                ('mean', ct.c_void_p), ('variance', ct.c_void_p), ('stats', ct.c_void_p)]


def ar1(rng, K, T, phi):
    x = np.empty((K, T))
    e = rng.normal(size=K)
    s = np.sqrt(1. - phi * phi)
    for n in range(T):
        e = phi * e + s * rng.normal(size=K) if n else e
        x[:, n] = e
    return x


def fft_inefficiency(A, mintime=3):
    """(g, stop_lag) of one tail from its autocorrelation by FFT"""
    Tt = len(A)
    d = A - A.mean()
    s2 = float((d * d).mean())
    n = 1 << int(np.ceil(np.log2(2 * Tt)))
    f = np.fft.rfft(d, n)
    acf = np.fft.irfft(f * np.conj(f), n)[:Tt - 1]
    t = np.arange(1, Tt - 1)
    C = acf[1:] / ((Tt - t) * s2)
    stop = np.flatnonzero((C <= 0.) & (t > mintime))
    stop = int(t[stop[0]]) if len(stop) else Tt - 1
    return max(1., 1. + 2. * float((C[:stop - 1] * (1. - t[:stop - 1] / float(Tt))).sum())), stop


def host_yardstick(a, origins, n_thread):
    def one(k):
        return [fft_inefficiency(a[k, o:]) for o in origins]
    t0 = time.perf_counter()
    with ThreadPoolExecutor(n_thread) as pool:
        r = list(pool.map(one, range(len(a))))
    return time.perf_counter() - t0, np.array([[x[0] for x in row] for row in r]), np.array([[x[1] for x in row] for row in r])


def resources():
    """the resource usage of the kernels of csrc/kernels_series.hip as the compiler reports it"""
    csrc = os.path.join(ROOT, 'upside-md_amd', 'csrc')
    cmd = ['hipcc', '--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-I' + os.environ.get('HDF5_INC', '/opt/conda/include'),
           '-Rpass-analysis=kernel-resource-usage', '-c', os.path.join(csrc, 'kernels_series.hip'), '-o', os.devnull]
    err = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, check=True).stdout.decode()
    out, name = [], None
    for ln in err.splitlines():
        m = re.search(r'remark: +(Function Name|VGPRs|AGPRs|ScratchSize \[bytes/lane\]|LDS Size \[bytes/block\]|Occupancy \[waves/SIMD\]): (\S+)', ln)
        if not m:
            continue
        if m.group(1) == 'Function Name':
            name = re.search(r'k_series_[a-z]+', m.group(2)).group(0)
            out.append({'kernel': name})
        else:
            out[-1][m.group(1).split(' [')[0]] = int(m.group(2))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=3)
    ap.add_argument('--threads', type=int, default=16)
    ap.add_argument('--cpu-series', default='64,16', help='series of each case the host yardstick runs on')
    ap.add_argument('--resources', action='store_true')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if args.resources:
        for r in resources():
            print(json.dumps(r))
        return
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('series_rate.py: no GPU')
    pkg = load_package()
    lib = pkg.default_library().calc
    lib.upk_series_solve.argtypes = [ct.POINTER(Problem), ct.c_char_p, ct.c_int]
    lines = ['# tools/series_rate.py, device %s' % torch.cuda.get_device_name(0)]
    n_cpu = [int(x) for x in args.cpu_series.split(',')]
    for (K, T, J), kc in zip(CASES, n_cpu):
        a = ar1(np.random.RandomState(K + J), K, T, float(np.exp(-1. / TAU)))
        o = pkg.timeseries.equilibration_origins(T, J)
        n = np.full(K, T, 'i8')
        g = np.zeros((K, J)); stop = np.zeros((K, J), 'i8'); mean = np.zeros((K, J)); var = np.zeros((K, J)); stats = np.zeros(5)
        P = Problem(K, T, n.ctypes.data, a.ctypes.data, J, o.ctypes.data, 3, 1 << 62, g.ctypes.data, stop.ctypes.data, mean.ctypes.data,
                    var.ctypes.data, stats.ctypes.data)
        msg = ct.create_string_buffer(256)

        def call():
            t0 = time.perf_counter()
            if lib.upk_series_solve(ct.byref(P), msg, 256):
                raise SystemExit('series_rate.py: %s' % msg.value.decode())
            return 1e3 * (time.perf_counter() - t0)
        call()
        best = None
        for _ in range(args.runs):
            ms = call()
            if best is None or stats[0] < best[1][0]:
                best = (ms, stats.copy())
        call_ms, st = best
        tile_ms = None
        try:
            from torch.profiler import profile, ProfilerActivity
            with profile(activities=[ProfilerActivity.CUDA]) as prof:
                call()
            us = sum(e.device_time_total for e in prof.key_averages() if 'k_series_lags' in e.key)
            tile_ms = round(us / 1e3, 3) if us > 0 else None
        except Exception as err:      # the profiler is a convenience of this tool only
            print('# torch profiler unavailable: %r' % (err,))
        flop = 2048. * st[4]      # a wave-instruction is 16 x 16 x 4 multiply-adds
        t_cpu, g_cpu, stop_cpu = host_yardstick(a[:kc], o, args.threads)
        best_origin = np.argmax(np.where(g > 0, (T - o)[None, :] / np.where(g > 0, g, 1.), 0.), axis=1)
        out = dict(n_series=K, T=T, n_origin=J, tau=TAU, device_ms=round(st[0], 3), wall_ms=round(st[1], 3), call_ms=round(call_ms, 3),
                   lag_blocks=int(st[2]), series_blocks=int(st[3]), mfma=st[4], tile_ms=tile_ms, tile_flop=flop,
                   tile_fraction_of_fp64_peak=None if tile_ms is None else round(flop / (tile_ms * 1e-3) / FP64_PEAK, 4),
                   stop_lag_min=int(stop[stop > 0].min()), stop_lag_median=float(np.median(stop[stop > 0])), stop_lag_max=int(stop.max()),
                   g_median=float(np.median(g[g > 0])), t0_median=float(np.median(o[best_origin])),
                   cpu_threads=args.threads, cpu_series=kc, cpu_s=round(t_cpu, 3), cpu_s_extrapolated_to_gpu_size=round(t_cpu * K / kc, 2),
                   speedup_extrapolated_device=round(t_cpu * K / kc / (st[0] * 1e-3), 1), speedup_extrapolated_call=round(t_cpu * K / kc / (call_ms * 1e-3), 1),
                   cpu_g_largest_relative_difference=float((np.abs(g[:kc] - g_cpu) / np.maximum(1., g_cpu)).max()),
                   cpu_stop_lags_equal=bool(np.array_equal(stop[:kc], stop_cpu)))
        print(json.dumps(out)); sys.stdout.flush()
        lines.append(json.dumps(out))
        del a
    lines.append('# cpu_s_extrapolated_to_gpu_size = cpu_s x n_series / cpu_series: an extrapolation in proportion to n_series, not a measurement')
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
