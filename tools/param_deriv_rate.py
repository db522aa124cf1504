"""Time the batched parameter derivatives against the per-system path and one MD step, on the GPU.

    python tools/param_deriv_rate.py --config syn300_10A --systems 4096 --steps 30

--config is a fixture name (tests/golden/<name>.up) or a path to a configuration.  The engine holds --systems replicas of the
configuration's structure with 0.05 A of seeded noise each and runs --steps MD steps to de-phase them.  For every node with a
parameter derivative it then times, each call ending in a device synchronisation and after one untimed warm-up call:
  1. one upside_hip_param_deriv_accumulate + upside_hip_param_deriv_read (all systems; the read synchronises);
  2. the per-system upside_hip_get_param_deriv loop over --sample evenly spaced systems, scaled to all systems;
and once, for scale, the mean time of one MD step over --steps steps.  Prints one JSON line."""
import argparse
import ctypes as ct
import json
import os
import re
import sys
import time
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from __graft_entry__ import load_package  # noqa: E402


def n_param_of(ens, node):
    """the size the batched calls expect (0: no derivative), from the message of a request of the wrong size"""
    c = ens.calc
    if c.upside_hip_get_param_deriv_all(ens.engine, node.encode(), -1, None) != 1:
        raise RuntimeError('a request of size -1 was accepted for %s' % node)
    m = re.search(r'expected (\d+)', c.upside_hip_last_error().decode())
    if not m:
        raise RuntimeError('%s: %s' % (node, c.upside_hip_last_error().decode()))
    return int(m.group(1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--config', default='syn300_10A')
    ap.add_argument('--systems', type=int, default=4096)
    ap.add_argument('--steps', type=int, default=30)
    ap.add_argument('--sample', type=int, default=16, help='systems timed on the per-system path (scaled to all)')
    ap.add_argument('--repeats', type=int, default=3, help='timed accumulate + read calls per node (the mean is reported)')
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('param_deriv_rate.py: no GPU')
    pkg = load_package()
    path = args.config if os.path.exists(args.config) else os.path.join(ROOT, 'tests', 'golden', args.config + '.up')
    S = args.systems
    ens = pkg.engine.Ensemble(path, S)
    c = ens.calc
    c.upside_hip_get_param_deriv.argtypes = [ct.c_void_p, ct.c_char_p, ct.c_int, ct.c_int, ct.c_void_p]
    rs = np.random.RandomState(1)
    x = ens.initial_pos[None] + np.float32(0.05) * rs.normal(size=(S,) + ens.initial_pos.shape).astype('f4')
    ens.set_pos(x)
    ens.init_md(0.8, 1000)
    sync = torch.cuda.synchronize

    ens.run_steps(args.steps)            # warm-up and de-phasing
    sync()
    t0 = time.perf_counter()
    ens.run_steps(args.steps)
    sync()
    md_step_ms = 1e3 * (time.perf_counter() - t0) / args.steps
    ens.energies()                        # the force pass the derivatives belong to

    with pkg.h5lite.open_file(path) as t:
        names = sorted(t.group('input/potential').keys())
    nodes = [(n, k) for n, k in ((n, n_param_of(ens, n)) for n in names) if k > 0]
    w = rs.uniform(-1., 1., size=S).astype('f4')
    sample = sorted(set(int(round(v)) for v in np.linspace(0, S - 1, min(args.sample, S))))
    per_node = {}
    for node, n in nodes:
        total = np.zeros(n, 'f8')
        nf = np.zeros(1, 'i8')
        b = node.encode()

        def acc_read():
            ens._check(c.upside_hip_param_deriv_accumulate(ens.engine, b, w.ctypes.data), 'accumulate')
            ens._check(c.upside_hip_param_deriv_read(ens.engine, b, n, total.ctypes.data, nf.ctypes.data, 1), 'read')
        acc_read()
        sync()
        t0 = time.perf_counter()
        for _ in range(args.repeats):
            acc_read()
        sync()
        acc_ms = 1e3 * (time.perf_counter() - t0) / args.repeats
        buf = np.zeros(n, 'f4')
        ens._check(c.upside_hip_get_param_deriv(ens.engine, b, 0, n, buf.ctypes.data), 'get_param_deriv')
        sync()
        t0 = time.perf_counter()
        for s in sample:
            ens._check(c.upside_hip_get_param_deriv(ens.engine, b, s, n, buf.ctypes.data), 'get_param_deriv')
        sync()
        loop_ms = 1e3 * (time.perf_counter() - t0) / len(sample) * S
        per_node[node] = dict(n_param=n, accumulate_read_ms=round(acc_ms, 3), per_system_loop_ms=round(loop_ms, 1))
    acc_total = sum(v['accumulate_read_ms'] for v in per_node.values())
    loop_total = sum(v['per_system_loop_ms'] for v in per_node.values())
    print(json.dumps(dict(
        config=os.path.basename(path), systems=S, md_step_ms=round(md_step_ms, 3), n_nodes=len(per_node),
        accumulate_read_ms=round(acc_total, 3), per_system_loop_ms=round(loop_total, 1),
        speedup=round(loop_total / acc_total, 1) if acc_total > 0 else None,
        accumulate_over_md_step=round(acc_total / md_step_ms, 3), per_system_sample=len(sample), nodes=per_node)))
    ens.close()


if __name__ == '__main__':
    main()
