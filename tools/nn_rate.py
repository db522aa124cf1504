"""Cost of the learned backbone potential (backbone_featurizer -> conv1d stack -> scaled_sum) on the GPU.

    python tools/nn_rate.py --config syn300_10A --systems 4096 --steps 30 --runs 3

--config is a fixture name (tests/golden/<name>.up) or a path.  A copy of it gets the three-layer network
6 -> 32 (W 5, ReLU) -> 32 (W 5, Tanh) -> 1 (W 1, Identity) with seeded weights (config.add_backbone_network).  Two engines of
--systems replicas each -- without and with the network, same library, same start -- run --steps MD steps alternately, --runs
times each after an untimed warm-up; the mean step time of every run and the spread are reported.  Then, on the engine with the
network, one upside_hip_param_deriv_accumulate per network node + one read (the read synchronises), mean of --runs after a
warm-up call.  Prints one JSON line.  --only network|plain builds one engine only (for a kernel trace in a run of its own:
rocprofv3 --kernel-trace --stats -- python tools/nn_rate.py --only network --runs 1)."""
import argparse
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

SPEC = ((5, 32, 'ReLU'), (5, 32, 'Tanh'), (1, 1, 'Identity'))


def seeded_layers(seed, c_in=6):
    rs = np.random.RandomState(seed)
    layers = []
    for W, c_out, act in SPEC:
        layers.append(((rs.normal(size=(W, c_in, c_out)) / np.sqrt(W * c_in)).astype('f4'), (0.3 * rs.normal(size=c_out)).astype('f4'), act))
        c_in = c_out
    return layers


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--config', default='syn300_10A')
    ap.add_argument('--systems', type=int, default=4096)
    ap.add_argument('--steps', type=int, default=30)
    ap.add_argument('--runs', type=int, default=3)
    ap.add_argument('--only', choices=['plain', 'network'], default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('nn_rate.py: no GPU')
    pkg = load_package()
    plain = args.config if os.path.exists(args.config) else os.path.join(ROOT, 'tests', 'golden', args.config + '.up')
    tmp = tempfile.mkdtemp(prefix='nn_rate_')
    try:
        net = os.path.join(tmp, 'network.up')
        shutil.copyfile(plain, net); os.chmod(net, 0o644)
        layers = seeded_layers(11)
        names = pkg.config.add_backbone_network(net, layers, 1.0)
        S = args.systems
        sync = torch.cuda.synchronize
        engines = {}
        for tag, p in (('plain', plain), ('network', net)):
            if args.only and args.only != tag:
                continue
            ens = pkg.engine.Ensemble(p, S)
            rs = np.random.RandomState(1)
            ens.set_pos(ens.initial_pos[None] + np.float32(0.05) * rs.normal(size=(S,) + ens.initial_pos.shape).astype('f4'))
            ens.init_md(0.8, 1000)
            ens.run_steps(args.steps)        # warm-up, de-phasing, graph capture
            sync()
            engines[tag] = ens
        step_ms = {tag: [] for tag in engines}
        for _ in range(args.runs):
            for tag, ens in engines.items():
                t0 = time.perf_counter()
                ens.run_steps(args.steps)
                sync()
                step_ms[tag].append(round(1e3 * (time.perf_counter() - t0) / args.steps, 3))
        out = dict(config=os.path.basename(plain), systems=S, steps=args.steps, step_ms=step_ms,
                   step_ms_mean={t: round(float(np.mean(v)), 3) for t, v in step_ms.items()},
                   step_ms_spread={t: round(float(np.max(v) - np.min(v)), 3) for t, v in step_ms.items()})
        if 'plain' in engines and 'network' in engines:
            out['network_cost_ms'] = round(out['step_ms_mean']['network'] - out['step_ms_mean']['plain'], 3)
            out['network_over_step'] = round(out['network_cost_ms'] / out['step_ms_mean']['plain'], 4)
        if 'network' in engines:
            ens = engines['network']
            ens.energies()
            w = np.random.RandomState(2).uniform(-1., 1., size=S).astype('f4')
            nodes = {nm: (lay[0].size + lay[1].size,) for nm, lay in zip(names[1:-1], layers)}
            nodes[names[-1]] = (1,)

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
            out['n_param'] = {nm: int(shp[0]) for nm, shp in nodes.items()}
        print(json.dumps(out))
        for ens in engines.values():
            ens.close()
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == '__main__':
    main()
