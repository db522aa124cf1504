#!/usr/bin/env python3
"""Rate of the pairwise RMSD on the device (csrc/kernels_rmsd.hip; upside-md_amd/cluster.py), on the GPU:

    python tools/rmsd_rate.py [--stub-library libupside_hip_stub.so] [--only matrix,nearest56,nearest168,gromos,cv] [--out FILE]

prints one JSON line per shape (and appends it to --out):
  matrix      symmetric 16384 x 16384 at n = 168 (protein G, all backbone atoms)
  nearest56, nearest168   2^20 frames against 1024 centres at n = 56 and n = 168
  gromos      cluster.gromos on 16384 frames of n = 168 made of 100 chains plus noise, as a whole call (wall time)
  cv          K = 32 rmsd CVs per frame through cvs() on 4096 systems of proteinG56_7A (all 168 backbone atoms): what the existing
              device route costs per pair (the method of tools/cv_path_rate.py: the mean of 20 synchronising calls, a one-distance call
              taken off as the floor)
tile_ms is the device time between HIP events around the tile kernel (upk_rmsd_solve's stats[0]), the minimum of three calls after a
warm-up call; pairs_per_s = pairs / tile_ms.  With --stub-library, a library built from the same sources with -DUPK_RMSD_STUB_SOLVE
(the eigenvalue replaced by tr M: for timing only, it is not shipped), accumulate_ms is the same call there and solve_ms the
difference; accumulate_fraction_of_fp64_peak = pairs x 18 n_pad FLOP / accumulate_ms / 78.6 TFLOP/s.  create_copy_ms and
create_kernel_ms: the copies of pos to the device and the centring kernel of Frames (wall, synchronised).  The yardstick: float64
numpy on 16 host threads (einsum for M, eigvalsh on Horn's matrix) on a slice of cpu_pairs pairs, multiplied up in proportion -- AN
EXTRAPOLATION, not a measurement."""
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

PEAK = 78.6e12


class FramesStruct(ct.Structure):      # upk_rmsd_frames_t
    _fields_ = [('magic', ct.c_int), ('n_atom', ct.c_int), ('n_pad', ct.c_int), ('n_frame', ct.c_longlong), ('y', ct.c_void_p), ('g', ct.c_void_p),
                ('create_ms', ct.c_double * 2)]


class Problem(ct.Structure):           # upk_rmsd_problem_t
    _fields_ = [('mode', ct.c_int), ('A', ct.c_void_p), ('B', ct.c_void_p), ('nA', ct.c_longlong), ('nB', ct.c_longlong), ('ia', ct.c_void_p),
                ('ib', ct.c_void_p), ('cutoff', ct.c_double), ('out', ct.c_void_p), ('index', ct.c_void_p), ('dist', ct.c_void_p), ('count', ct.c_void_p),
                ('stats', ct.c_void_p)]


def chains(F, n, seed):
    rng = np.random.default_rng(seed)
    step = rng.standard_normal((F, n, 3), dtype='f4')
    step *= np.float32(3.8) / np.linalg.norm(step, axis=2, keepdims=True)
    return np.cumsum(step, axis=1, dtype='f4')


def noisy(centres, F, seed, noise=0.05):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((F,) + centres.shape[1:], dtype='f4')
    x *= np.float32(noise)
    x += centres[np.arange(F) % len(centres)]
    return x


def solve_ms(calc, mode, A, B, out=None, index=None, dist=None, count=None, cutoff=0., repeats=3):
    """the minimum device time of `repeats` calls after a warm-up call"""
    stats = np.zeros(3)
    P = Problem(mode, A.value, B.value, ct.cast(A, ct.POINTER(FramesStruct)).contents.n_frame, ct.cast(B, ct.POINTER(FramesStruct)).contents.n_frame,
                None, None, cutoff, *(None if a is None else a.ctypes.data for a in (out, index, dist, count)), stats.ctypes.data)
    msg = ct.create_string_buffer(256)
    best = []
    for k in range(repeats + 1):
        if calc.upk_rmsd_solve(ct.byref(P), msg, 256):
            raise SystemExit('rmsd_rate.py: %s' % msg.value.decode())
        if k:
            best.append(stats[0])
    return min(best), [round(float(b), 3) for b in best]


def handle_of(calc, x):
    h = ct.c_void_p()
    msg = ct.create_string_buffer(256)
    t0 = time.perf_counter()
    if calc.upk_rmsd_frames_create(x.shape[1], x.shape[0], x.ctypes.data, ct.byref(h), msg, 256):
        raise SystemExit('rmsd_rate.py: %s' % msg.value.decode())
    wall = 1e3 * (time.perf_counter() - t0)
    ms = ct.cast(h, ct.POINTER(FramesStruct)).contents.create_ms
    return h, dict(create_copy_ms=round(ms[0], 3), create_kernel_ms=round(ms[1], 3), create_wall_ms_with_the_finite_check=round(wall, 3))


def bind(calc):
    calc.upk_rmsd_solve.argtypes = [ct.c_void_p, ct.c_char_p, ct.c_int]; calc.upk_rmsd_solve.restype = ct.c_int
    calc.upk_rmsd_frames_create.argtypes = [ct.c_int, ct.c_longlong, ct.c_void_p, ct.c_void_p, ct.c_char_p, ct.c_int]; calc.upk_rmsd_frames_create.restype = ct.c_int
    calc.upk_rmsd_frames_free.argtypes = [ct.c_void_p]; calc.upk_rmsd_frames_free.restype = None
    return calc


def yardstick_s(R, a, b, n_pairs, threads=16):
    """seconds of the numpy yardstick on the pairs a x b, 16 threads side by side, and the extrapolation to n_pairs"""
    parts = np.array_split(np.arange(len(a)), threads)
    t0 = time.perf_counter()
    with ThreadPoolExecutor(threads) as ex:
        list(ex.map(lambda p: R.d2_matrix(a[p], b), parts))
    s = time.perf_counter() - t0
    return dict(cpu_threads=threads, cpu_pairs=len(a) * len(b), cpu_s=round(s, 3), cpu_s_extrapolated_to_gpu_size=round(s * n_pairs / (len(a) * len(b)), 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--stub-library')
    ap.add_argument('--only', default='matrix,nearest56,nearest168,gromos,cv')
    ap.add_argument('--out')
    ap.add_argument('--frames', type=int, default=16384)
    ap.add_argument('--rows', type=int, default=1 << 20)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('rmsd_rate.py: no GPU')
    pkg = load_package()
    import rmsd_reference as R
    calc = bind(pkg.default_library().calc)
    stub = bind(pkg.UpsideLibrary(args.stub_library).calc) if args.stub_library else None
    only = args.only.split(',')

    def emit(row):
        line = json.dumps(row)
        print(line, flush=True)
        if args.out:
            with open(args.out, 'a') as f:
                f.write(line + '\n')

    def split(row, pairs, n, mode, x_a, x_b, **kw):
        """tile_ms here, and with the stub library the accumulation alone"""
        n_pad = (n + 3) // 4 * 4
        row.update(pairs=pairs, pairs_per_s=round(pairs / (row['tile_ms'] * 1e-3), 1))
        if stub is not None:
            hA, _ = handle_of(stub, x_a)
            hB = hA if x_b is None else handle_of(stub, x_b)[0]
            acc, runs = solve_ms(stub, mode, hA, hB, **kw)
            stub.upk_rmsd_frames_free(hA)
            if hB is not hA:
                stub.upk_rmsd_frames_free(hB)
            row.update(accumulate_ms=round(acc, 3), accumulate_ms_runs=runs, solve_ms=round(row['tile_ms'] - acc, 3), flop=pairs * 18 * n_pad,
                       accumulate_fraction_of_fp64_peak=round(pairs * 18 * n_pad / (acc * 1e-3) / PEAK, 4))

    if 'matrix' in only:
        F, n = args.frames, 168
        x = chains(F, n, 1)
        h, created = handle_of(calc, x)
        out = np.empty((F, F))
        ms, runs = solve_ms(calc, 0, h, h, out=out)
        calc.upk_rmsd_frames_free(h)
        row = dict(shape='matrix', frames=F, n_atom=n, tile_ms=round(ms, 3), tile_ms_runs=runs, **created)
        split(row, F * (F - 1) // 2, n, 0, x, None, out=out)
        row.update(yardstick_s(R, x[:512], x[512:1024], F * (F - 1) // 2))
        emit(row)
        del out
    for name, n in (('nearest56', 56), ('nearest168', 168)):
        if name not in only:
            continue
        F, C = args.rows, 1024
        cen = chains(C, n, 2)
        x = noisy(cen, F, 3)
        h, created = handle_of(calc, x)
        hc, _ = handle_of(calc, cen)
        index = np.zeros(F, 'i8'); dist = np.zeros(F)
        ms, runs = solve_ms(calc, 1, h, hc, index=index, dist=dist)
        calc.upk_rmsd_frames_free(h); calc.upk_rmsd_frames_free(hc)
        assert np.array_equal(index, np.arange(F) % C)
        row = dict(shape=name, rows=F, centres=C, n_atom=n, tile_ms=round(ms, 3), tile_ms_runs=runs, **created)
        split(row, F * C, n, 1, x, cen, index=index, dist=dist)
        row.update(yardstick_s(R, x[:512], cen[:512], F * C))
        emit(row)
        del x
    if 'gromos' in only:
        F, n = args.frames, 168
        x = noisy(chains(100, n, 4), F, 5)
        wall = []
        for k in range(4):
            t0 = time.perf_counter()
            with pkg.cluster.Frames(x) as fr:
                t1 = time.perf_counter()
                c, a, s = pkg.cluster.gromos(fr, 1.0)
            wall.append((round(1e3 * (time.perf_counter() - t0), 1), round(1e3 * (time.perf_counter() - t1), 1)))
        emit(dict(shape='gromos', frames=F, n_atom=n, cutoff=1.0, clusters=int(len(c)), largest=int(s[0]), pairs_two_passes=F * F * 2,
                  whole_call_ms_with_create=min(w[0] for w in wall[1:]), gromos_ms=min(w[1] for w in wall[1:]), runs=wall[1:],
                  pairs_per_s=round(2. * F * F / (min(w[1] for w in wall[1:]) * 1e-3), 1)))
    if 'cv' in only:
        path = os.path.join(ROOT, 'tests', 'golden', 'proteinG56_7A.up')
        S, K = 4096, 32
        eng = pkg.engine.BatchEngine(path, S)
        rs = np.random.RandomState(1)
        eng.set_pos(eng.initial_pos[None] + np.float32(0.05) * rs.normal(size=(S,) + eng.initial_pos.shape).astype('f4'))
        atoms = np.arange(eng.initial_pos.shape[0], dtype='i4')
        refs = noisy(eng.initial_pos[None].astype('f4'), K, 6, 1.0)

        def call_ms(specs, calls=20):
            eng.define_cvs(specs)
            eng.cvs(); torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(calls):
                eng.cvs()
            return 1e3 * (time.perf_counter() - t0) / calls
        rm = min(call_ms([{'name': 'f%d' % k, 'kind': 'rmsd', 'atoms': atoms, 'ref': refs[k].astype('f8')} for k in range(K)]) for _ in range(3))
        fl = min(call_ms([{'kind': 'distance', 'pair': (0, int(atoms[-1]))}]) for _ in range(3))
        emit(dict(shape='cv', systems=S, rmsd_cvs=K, n_atom=int(len(atoms)), pairs=S * K, cvs_call_ms=round(rm, 4), floor_ms=round(fl, 4),
                  pairs_per_s=round(S * K / ((rm - fl) * 1e-3), 1)))
        eng.close()


if __name__ == '__main__':
    main()
