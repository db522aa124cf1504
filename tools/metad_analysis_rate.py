"""Cost of the metadynamics analysis on the GPU (upside_hip_metad_bias and upside_hip_metad_grid, csrc/kernels_metad.hip) and of a float64
numpy yardstick on the host.

    python tools/metad_analysis_rate.py [--runs 3] [--threads 16] [--cases all] [--out FILE]
    python tools/metad_analysis_rate.py --resources      (no GPU needed: the resource usage of the kernels from the compiler)

Grids (hills uniform over the grid's box, sigma = 1/20 of the box, one checkpoint at the end unless stated, scales (1/kT + 1/kdT,
1/kdT)): one list of 10^5 hills on 100 x 100; one list of 10^6 hills on 256 x 256; 4096 lists of 4096 hills on 64 x 64 with 64
checkpoints each; d = 3, 48^3 with 10^5 hills; d = 4, 24^4 with 10^5 hills.  Each is run by shape (the factorised sum) and with the
direct sum forced (path = 1 of upk_metad_grid_solve), which is what upside_hip_metad_bias does over the same grid points.
Frames: 10^6 frames against 10^5 hills in time order; 4096 lists of 4096 frames against 4096 hills each, in time order.
From the stats array of the internal solves: device_ms between two HIP events around the kernels of the call (copies of the hills in
and of the last results out excluded), call_ms as the caller sees it (checks and copies included), the exponentials of the hill sums
and the v_mfma_f64_16x16x4_f64 count; minima of --runs after an untimed call.  tile_ms is the device time of the k_metad_tile launches of
one call from torch's profiler (null where it records none) and tile_fraction_of_fp64_peak what its 2048 FLOP per MFMA reach of 78.6
TFLOP/s, the public figure for the MI355X.  The yardstick is the chunked float64 numpy sum of tests/metad_reference.py's definition over
--threads threads on a SLICE of the case (at most 4096 points x 8192 hills), EXTRAPOLATED in proportion to points x hills: a
multiplication, not a measurement.  Prints one JSON line per case; --out also writes them to a file (profiles/metad_analysis_rate.txt
holds a run with its explanation)."""
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
KT, KDT = 0.8, 4.0


class Hills(ct.Structure):
    _fields_ = [('n_list', ct.c_int), ('d', ct.c_int)] + [(k, ct.c_void_p) for k in ('hill_start', 'centers', 'weights', 'sigma', 'periods')]


class BiasProblem(ct.Structure):
    _fields_ = [('H', Hills)] + [(k, ct.c_void_p) for k in ('point_start', 'points', 'n_visible', 'V', 'stats')]


class GridProblem(ct.Structure):
    _fields_ = [('H', Hills), ('n_axis', ct.c_void_p), ('axes', ct.c_void_p), ('n_checkpoint', ct.c_int), ('checkpoints', ct.c_void_p),
                ('n_scale', ct.c_int), ('scales', ct.c_void_p), ('V_last', ct.c_void_p), ('lse', ct.c_void_p), ('workspace_limit', ct.c_size_t),
                ('path', ct.c_int), ('stats', ct.c_void_p)]


GRID_CASES = (('1 list, 1e5 hills, 100x100', 1, 100000, (100, 100), 1), ('1 list, 1e6 hills, 256x256', 1, 1000000, (256, 256), 1),
              ('4096 lists, 4096 hills, 64x64, 64 checkpoints', 4096, 4096, (64, 64), 64), ('1 list, 1e5 hills, 48^3', 1, 100000, (48, 48, 48), 1),
              ('1 list, 1e5 hills, 24^4', 1, 100000, (24, 24, 24, 24), 1))
FRAME_CASES = (('1e6 frames, 1e5 hills, time order', 1, 1000000, 100000), ('4096 lists, 4096 frames, 4096 hills, time order', 4096, 4096, 4096))


def make_hills(rng, L, H, d):
    c = rng.uniform(0., 1., size=(L * H, d)).astype('f4')
    w = rng.uniform(0.05, 0.3, size=L * H).astype('f4')
    return c, w, (H * np.arange(L + 1)).astype('i8'), np.full(d, 0.05), np.zeros(d)


def host_yardstick(x, c, w, sg, n_thread):
    """seconds for V at the points x over the hills (c, w): chunks of 256 points over the threads"""
    def one(i0):
        q = np.zeros((len(x[i0:i0 + 256]), len(c)))
        for k in range(len(sg)):
            dx = x[i0:i0 + 256, None, k] - c[None, :, k]
            q += dx * dx / (sg[k] * sg[k])
        return np.exp(-0.5 * q) @ w
    t0 = time.perf_counter()
    with ThreadPoolExecutor(n_thread) as pool:
        list(pool.map(one, range(0, len(x), 256)))
    return time.perf_counter() - t0


def resources():
    csrc = os.path.join(ROOT, 'upside-md_amd', 'csrc')
    cmd = ['hipcc', '--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-I' + os.environ.get('HDF5_INC', '/opt/conda/include'),
           '-Rpass-analysis=kernel-resource-usage', '-c', os.path.join(csrc, 'kernels_metad.hip'), '-o', os.devnull]
    err = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, check=True).stdout.decode()
    out = []
    for ln in err.splitlines():
        m = re.search(r'remark: +(Function Name|VGPRs|AGPRs|ScratchSize \[bytes/lane\]|VGPRs Spill|SGPRs Spill|LDS Size \[bytes/block\]|Occupancy \[waves/SIMD\]): (\S+)', ln)
        if not m:
            continue
        if m.group(1) == 'Function Name':
            t = re.search(r'ILi(\d)E', m.group(2))
            out.append({'kernel': re.search(r'k_metad_[a-z_]+', m.group(2)).group(0) + ('<%s>' % t.group(1) if t else '')})
        else:
            out[-1][m.group(1).split(' [')[0]] = int(m.group(2))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=3)
    ap.add_argument('--threads', type=int, default=16)
    ap.add_argument('--cases', default='all', help="'all', or a comma-separated list of case numbers (grids 0 .. 4, frames 5 .. 6)")
    ap.add_argument('--resources', action='store_true')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if args.resources:
        for r in resources():
            print(json.dumps(r))
        return
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('metad_analysis_rate.py: no GPU')
    pkg = load_package()
    lib = pkg.default_library().calc
    lib.upk_metad_grid_solve.argtypes = [ct.c_void_p, ct.c_char_p, ct.c_int]
    lib.upk_metad_bias_solve.argtypes = [ct.c_void_p, ct.c_char_p, ct.c_int]
    want = None if args.cases == 'all' else set(int(x) for x in args.cases.split(','))
    lines = ['# tools/metad_analysis_rate.py, device %s' % torch.cuda.get_device_name(0)]
    msg = ct.create_string_buffer(256)

    def best_of(fn, problem, stats):
        def call():
            t0 = time.perf_counter()
            if fn(ct.byref(problem), msg, 256):
                raise SystemExit('metad_analysis_rate.py: %s' % msg.value.decode())
            return 1e3 * (time.perf_counter() - t0)
        call()
        best = None
        for _ in range(args.runs):
            ms = call()
            if best is None or stats[0] < best[1][0]:
                best = (ms, stats.copy())
        return best, call

    def emit(out):
        print(json.dumps(out)); sys.stdout.flush()
        lines.append(json.dumps(out))

    a_scale, b_scale = 1. / KT + 1. / KDT, 1. / KDT
    for i, (label, L, H, shape, K) in enumerate(GRID_CASES):
        if want is not None and i not in want:
            continue
        d = len(shape)
        rng = np.random.RandomState(100 + i)
        c, w, hs, sg, per = make_hills(rng, L, H, d)
        axes = [np.linspace(0., 1., n) for n in shape]
        n_axis = np.array(shape, 'i4'); flat = np.concatenate(axes)
        ck = np.ascontiguousarray(np.tile((H * (np.arange(K) + 1) // K).astype('i8'), (L, 1)))
        sc = np.array([a_scale, b_scale])
        G = int(np.prod(shape))
        V = np.zeros((L, G)); lse = np.zeros((L, K, 2)); stats = np.zeros(6)
        P = GridProblem()
        P.H = Hills(L, d, hs.ctypes.data, c.ctypes.data, w.ctypes.data, sg.ctypes.data, per.ctypes.data)
        P.n_axis = n_axis.ctypes.data; P.axes = flat.ctypes.data; P.n_checkpoint = K; P.checkpoints = ck.ctypes.data; P.n_scale = 2; P.scales = sc.ctypes.data
        P.V_last = V.ctypes.data; P.lse = lse.ctypes.data; P.stats = stats.ctypes.data
        res = {}
        for name, path in (('factorised', 0), ('direct', 1)):
            P.path = path
            (call_ms, st), call = best_of(lib.upk_metad_grid_solve, P, stats)
            res[name] = dict(device_ms=round(st[0], 3), call_ms=round(call_ms, 3), exponentials=st[2], mfma=st[3], path=int(st[4]), chunks=int(st[5]),
                             G_exp_per_s=round(st[2] / (st[0] * 1e-3) / 1e9, 2))
            res[name + '_V'] = V.copy()
            if path == 0 and st[4] == 2:
                tile_ms = None
                try:
                    from torch.profiler import profile, ProfilerActivity
                    with profile(activities=[ProfilerActivity.CUDA]) as prof:
                        call()
                    us = sum(e.device_time_total for e in prof.key_averages() if 'k_metad_tile' in e.key)
                    tile_ms = round(us / 1e3, 3) if us > 0 else None
                except Exception as err:      # the profiler is a convenience of this tool only
                    print('# torch profiler unavailable: %r' % (err,))
                res[name].update(tile_ms=tile_ms, tile_flop=2048. * st[3],
                                 tile_fraction_of_fp64_peak=None if tile_ms is None else round(2048. * st[3] / (tile_ms * 1e-3) / FP64_PEAK, 4))
        A = np.abs(res['direct_V']).max()
        agree = float(np.abs(res.pop('factorised_V') - res.pop('direct_V')).max() / A)
        mesh = np.stack([m.reshape(-1) for m in np.meshgrid(*axes, indexing='ij')], axis=1)
        n_pt, n_h = min(G, 4096), min(H, 8192)
        t_cpu = host_yardstick(mesh[:n_pt], c[:n_h].astype('f8'), w[:n_h].astype('f8'), sg, args.threads)
        cpu_all = t_cpu * (float(G) * H * L) / (float(n_pt) * n_h)
        emit(dict(case=label, n_list=L, hills=H, grid=list(shape), checkpoints=K, factorised=res['factorised'], direct=res['direct'],
                  direct_over_factorised_device=round(res['direct']['device_ms'] / res['factorised']['device_ms'], 2),
                  largest_difference_of_the_two_paths_over_largest_V=agree, cpu_threads=args.threads, cpu_slice=[n_pt, n_h], cpu_s=round(t_cpu, 3),
                  cpu_s_extrapolated=round(cpu_all, 1), speedup_extrapolated_device=round(cpu_all / (res['factorised']['device_ms'] * 1e-3), 1),
                  speedup_extrapolated_call=round(cpu_all / (res['factorised']['call_ms'] * 1e-3), 1)))
        del V, c, w, mesh
    for i, (label, L, N, H) in enumerate(FRAME_CASES):
        if want is not None and i + len(GRID_CASES) not in want:
            continue
        d = 2
        rng = np.random.RandomState(200 + i)
        c, w, hs, sg, per = make_hills(rng, L, H, d)
        x = rng.uniform(0., 1., size=(L * N, d))
        ps = (N * np.arange(L + 1)).astype('i8')
        nv = np.ascontiguousarray(np.tile((H * np.arange(N) // N).astype('i8'), L))      # time order: frame n saw the first H n / N hills
        V = np.zeros(L * N); stats = np.zeros(6)
        P = BiasProblem(Hills(L, d, hs.ctypes.data, c.ctypes.data, w.ctypes.data, sg.ctypes.data, per.ctypes.data), ps.ctypes.data, x.ctypes.data, nv.ctypes.data,
                        V.ctypes.data, stats.ctypes.data)
        (call_ms, st), _ = best_of(lib.upk_metad_bias_solve, P, stats)
        n_pt, n_h = min(N, 4096), min(H, 8192)
        t_cpu = host_yardstick(x[:n_pt], c[:n_h].astype('f8'), w[:n_h].astype('f8'), sg, args.threads)
        cpu_all = t_cpu * st[2] / (float(n_pt) * n_h)      # (the triangle: in proportion to the exponentials the device executed)
        emit(dict(case=label, n_list=L, frames=N, hills=H, d=d, device_ms=round(st[0], 3), call_ms=round(call_ms, 3), exponentials=st[2],
                  square=float(L) * N * H, G_exp_per_s=round(st[2] / (st[0] * 1e-3) / 1e9, 2), cpu_threads=args.threads, cpu_slice=[n_pt, n_h], cpu_s=round(t_cpu, 3),
                  cpu_s_extrapolated=round(cpu_all, 1), speedup_extrapolated_device=round(cpu_all / (st[0] * 1e-3), 1),
                  speedup_extrapolated_call=round(cpu_all / (call_ms * 1e-3), 1)))
    lines.append('# cpu_s_extrapolated = cpu_s x (points x hills of the case) / (points x hills of cpu_slice): an extrapolation, not a measurement')
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
