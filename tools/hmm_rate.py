"""Cost of the TorusDBN backbone prior (torus_dbn -> fixed_hmm) on the GPU.

    python tools/hmm_rate.py --config syn300_10A --systems 4096 --states 55 --steps 30 --runs 5 [--out profiles/hmm_rate.txt]

--config is a fixture name (tests/golden/<name>.up) or a path.  A copy of it gets a --states-state prior with seeded parameters
(config.add_torus_dbn; no TorusDBN library ships with the reference).  Two engines of --systems replicas each -- without and
with the prior, same library, same start -- run --steps MD steps alternately, --runs times each after an untimed warm-up (the
timed region ends with a device synchronisation; the first run of each engine is reported but left out of the mean).  Then,
on the engine with the prior, the per-kernel HIP-event times of upside_hip_profile_dump over --steps steps (profiling brackets
single launches, so those steps are not the timed ones), and one param_deriv_accumulate per node + one read.  Prints one JSON
line; --out also writes a text report."""
import argparse
import ctypes as ct
import json
import os
import shutil
import sys
import tempfile
import time
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from __graft_entry__ import load_package  # noqa: E402

RESTYPES = ['ALA', 'ARG', 'ASN', 'ASP', 'CYS', 'GLN', 'GLU', 'GLY', 'HIS', 'ILE', 'LEU', 'LYS', 'MET', 'PHE', 'PRO', 'SER', 'THR', 'TRP',
            'TYR', 'VAL', 'CPR']


def seeded_parameters(n_state, seed):
    rs = np.random.RandomState(seed)
    bp = np.zeros((n_state, 6), 'f4')
    bp[:, 0] = rs.normal(size=n_state)
    bp[:, 1] = rs.uniform(0.3, 4., size=n_state); bp[:, 2] = rs.uniform(-np.pi, np.pi, size=n_state)
    bp[:, 3] = rs.uniform(0.3, 4., size=n_state); bp[:, 4] = rs.uniform(-np.pi, np.pi, size=n_state)
    bp[:, 5] = rs.uniform(-1., 1., size=n_state)
    return bp, rs.normal(size=(len(RESTYPES), n_state)).astype('f4'), rs.uniform(0., 3., size=(n_state, n_state)).astype('f4')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--config', default='syn300_10A')
    ap.add_argument('--systems', type=int, default=4096)
    ap.add_argument('--states', type=int, default=55)
    ap.add_argument('--steps', type=int, default=30)
    ap.add_argument('--runs', type=int, default=5)
    ap.add_argument('--out', default='')
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('hmm_rate.py: no GPU')
    pkg = load_package()
    plain = args.config if os.path.exists(args.config) else os.path.join(ROOT, 'tests', 'golden', args.config + '.up')
    tmp = tempfile.mkdtemp(prefix='hmm_rate_')
    try:
        prior = os.path.join(tmp, 'prior.up')
        shutil.copyfile(plain, prior); os.chmod(prior, 0o644)
        bp, aa, te = seeded_parameters(args.states, 11)
        names = pkg.config.add_torus_dbn(prior, bp, aa, te, RESTYPES)
        S = args.systems
        sync = torch.cuda.synchronize
        engines = {}
        for tag, p in (('plain', plain), ('prior', prior)):
            ens = pkg.engine.Ensemble(p, S)
            rs = np.random.RandomState(1)
            ens.set_pos(ens.initial_pos[None] + np.float32(0.05) * rs.normal(size=(S,) + ens.initial_pos.shape).astype('f4'))
            ens.init_md(0.8, 1000)
            ens.run_steps(args.steps)        # warm-up, de-phasing, graph capture
            sync()
            engines[tag] = ens
        step_ms = {tag: [] for tag in engines}
        for _ in range(args.runs + 1):
            for tag, ens in engines.items():
                t0 = time.perf_counter()
                ens.run_steps(args.steps)
                sync()
                step_ms[tag].append(round(1e3 * (time.perf_counter() - t0) / args.steps, 3))
        kept = {t: v[1:] for t, v in step_ms.items()}
        out = dict(config=os.path.basename(plain), systems=S, states=args.states, steps=args.steps, step_ms=step_ms,
                   step_ms_mean={t: round(float(np.mean(v)), 3) for t, v in kept.items()},
                   step_ms_spread={t: round(float(np.max(v) - np.min(v)), 3) for t, v in kept.items()})
        out['prior_cost_ms'] = round(out['step_ms_mean']['prior'] - out['step_ms_mean']['plain'], 3)
        out['prior_over_step'] = round(out['prior_cost_ms'] / out['step_ms_mean']['plain'], 4)
        # per-kernel times: HIP events around single launches, in steps of their own
        ens = engines['prior']; c = ens.calc
        c.upside_hip_profile_reset.argtypes = [ct.c_void_p, ct.c_int]
        c.upside_hip_profile_dump.argtypes = [ct.c_void_p, ct.c_char_p, ct.c_int]
        assert c.upside_hip_profile_reset(ens.engine, 1) == 0
        ens.run_steps(args.steps)
        buf = ct.create_string_buffer(1 << 16)
        assert c.upside_hip_profile_dump(ens.engine, buf, len(buf)) == 0
        assert c.upside_hip_profile_reset(ens.engine, 0) == 0
        kernels = {}
        for ln in buf.value.decode().strip().split('\n'):
            nm, ms, n, by, pr = ln.split()
            kernels[nm] = dict(ms_per_launch=round(float(ms) / int(n), 4), launches=int(n),
                               GBps=round(float(by) / int(n) / (float(ms) / int(n) * 1e-3) / 1e9, 1) if float(by) else None)
        out['kernel_ms_per_launch'] = {k: v['ms_per_launch'] for k, v in kernels.items() if k.split(':')[-1] in names}
        out['kernel_GBps'] = {k: v['GBps'] for k, v in kernels.items() if k.split(':')[-1] in names}
        out['profiled_ms_per_step_all_kernels'] = round(sum(float(v['ms_per_launch']) * v['launches'] for v in kernels.values()) / args.steps, 3)
        # parameter derivatives: accumulate both nodes + read
        ens.energies()
        w = np.random.RandomState(2).uniform(-1., 1., size=S).astype('f4')
        nodes = {names[0]: (aa.size,), names[1]: (te.size,)}

        def acc_read():
            for nm in nodes:
                ens.param_deriv_accumulate(nm, w)
            for nm, shp in nodes.items():
                ens.param_deriv_read(nm, shp)
        acc_read()
        sync()
        t0 = time.perf_counter()
        for _ in range(args.runs):
            acc_read()
        sync()
        out['param_deriv_accumulate_read_ms'] = round(1e3 * (time.perf_counter() - t0) / args.runs, 3)
        print(json.dumps(out))
        if args.out:
            with open(args.out, 'w') as f:
                f.write('tools/hmm_rate.py --config %s --systems %d --states %d --steps %d --runs %d\n' % (args.config, S, args.states, args.steps, args.runs))
                f.write('MD step, ms (each engine %d runs of %d steps, alternating; first run of each left out of the mean):\n' % (args.runs + 1, args.steps))
                for t in ('plain', 'prior'):
                    f.write('  %-6s %s  mean %.3f  spread %.3f\n' % (t, step_ms[t], out['step_ms_mean'][t], out['step_ms_spread'][t]))
                f.write('cost of the prior: %.3f ms per step = %.2f %% of the step\n' % (out['prior_cost_ms'], 100. * out['prior_over_step']))
                f.write('per-kernel HIP-event times over %d steps of their own (ms per launch, algorithmic GB/s):\n' % args.steps)
                for k in sorted(out['kernel_ms_per_launch']):
                    f.write('  %-28s %.4f ms  %s GB/s\n' % (k, out['kernel_ms_per_launch'][k], out['kernel_GBps'][k]))
                f.write('param_deriv_accumulate of both nodes + read: %.3f ms\n' % out['param_deriv_accumulate_read_ms'])
        for e in engines.values():
            e.close()
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == '__main__':
    main()
