"""Cost of a cv_metadynamics node in the MD loop, on the GPU.

    python tools/metad_rate.py --config syn300_10A --systems 4096 --steps 30 --runs 3 --capacity 4096 --fills 0,1024,4096

--config is a fixture name (tests/golden/<name>.up) or a path.  Two engines of --systems replicas are built from it: one unchanged,
one with a cv_metadynamics node of d = 2 (rmsd and Q -- the native contacts within 8 A -- over the CA atoms), unshared lists of
--capacity slots, pace 1, heights small enough for the trajectory to stay that of the benchmark.  For every fill level of --fills
each system's list is loaded with that many hills (centres within +-2 sigma of the input structure's values) and the two engines run
--steps MD steps (a multiple of 3: whole rounds) in turn, --runs times each; every timed run follows an untimed run of the same
length of the same engine.  The lists are rewritten before every run of the engine with the node, so the fill level holds (at the
full level every deposit is dropped; below it a run adds steps / 3 hills).  Reported per fill level: the mean step time of every run,
mean and spread (max - min) per engine and the difference.  The two kernels' own times come from a kernel trace of this tool, a run
of its own.  Prints one JSON line."""
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

NODE = 'cv_metadynamics'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--config', default='syn300_10A')
    ap.add_argument('--systems', type=int, default=4096)
    ap.add_argument('--steps', type=int, default=30)
    ap.add_argument('--runs', type=int, default=3)
    ap.add_argument('--capacity', type=int, default=4096)
    ap.add_argument('--fills', default='0,1024,4096')
    ap.add_argument('--settle', type=int, default=102, help='untimed steps before anything is measured (de-phases the pair-list rebuilds)')
    args = ap.parse_args()
    if args.steps % 3:
        raise SystemExit('metad_rate.py: --steps must be a multiple of 3 (whole rounds)')
    fills = [int(f) for f in args.fills.split(',')]
    if max(fills) > args.capacity:
        raise SystemExit('metad_rate.py: a fill level exceeds --capacity')
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('metad_rate.py: no GPU')
    pkg = load_package()
    path = args.config if os.path.exists(args.config) else os.path.join(ROOT, 'tests', 'golden', args.config + '.up')
    S = args.systems
    sync = torch.cuda.synchronize
    work = tempfile.mkdtemp(prefix='metad_rate_')
    try:
        with_node = os.path.join(work, 'with_node.up')
        shutil.copyfile(path, with_node)
        pos0 = pkg.config.read_pos(path).astype('f8')
        specs = [sp for sp in pkg.config.default_collective_variables(pos0) if sp['kind'] in ('rmsd', 'contacts')]
        assert [sp['kind'] for sp in specs] == ['rmsd', 'contacts']
        probe = pkg.engine.BatchEngine(path, 1)
        probe.define_cvs(specs); probe.set_pos(pos0.astype('f4'))
        v0 = probe.cvs()[0].astype('f8')
        probe.close()
        sigma = np.array([0.3, 0.03])
        pkg.config.add_cv_metadynamics(with_node, specs, sigma, 1e-4, 1, args.capacity)
        engines = {}
        for tag, p in (('without', path), ('with', with_node)):
            ens = pkg.engine.BatchEngine(p, S)
            rs = np.random.RandomState(1)
            ens.set_pos(ens.initial_pos[None] + np.float32(0.05) * rs.normal(size=(S,) + ens.initial_pos.shape).astype('f4'))
            ens.init_md(0.8, 1000)
            ens.run_steps(args.settle)
            engines[tag] = ens
        sync()
        rng = np.random.default_rng(2)
        out = dict(config=os.path.basename(path), systems=S, steps=args.steps, runs=args.runs, d=2, capacity=args.capacity,
                   n_contact_pairs=int(len(specs[1]['pairs'])), sigma=sigma.tolist(), fills={})

        def fill(n):      # every system the same n hills (the cost does not depend on their values)
            c = (v0[None] + rng.uniform(-2., 2., (n, 2)) * sigma[None]).astype('f4'); w = np.full(n, 1e-4, 'f4')
            for s in range(S):
                engines['with'].set_metad_hills(NODE, c, w, system=s)
            sync()

        for n in fills:
            step_ms = {tag: [] for tag in engines}
            for _ in range(args.runs):
                for tag, ens in engines.items():
                    for timed in (False, True):
                        if tag == 'with':
                            fill(n)
                        sync()
                        t0 = time.perf_counter()
                        ens.run_steps(args.steps)
                        sync()
                        if timed:
                            step_ms[tag].append(round(1e3 * (time.perf_counter() - t0) / args.steps, 4))
            mean = {t: float(np.mean(v)) for t, v in step_ms.items()}
            hills_end = len(engines['with'].metad_hills(NODE, system=S - 1)[1])
            out['fills'][str(n)] = dict(step_ms=step_ms, step_ms_mean={t: round(m, 4) for t, m in mean.items()},
                                        step_ms_spread={t: round(float(np.max(v) - np.min(v)), 4) for t, v in step_ms.items()},
                                        node_ms_per_step=round(mean['with'] - mean['without'], 4), node_fraction=round(mean['with'] / mean['without'] - 1., 5),
                                        hills_at_the_end_of_a_run=hills_end)
        out['metad_values_of_system_0'] = np.round(engines['with'].metad_values(NODE)[0], 4).tolist()
        for ens in engines.values():
            ens.close()
        print(json.dumps(out))
    finally:
        shutil.rmtree(work, ignore_errors=True)


if __name__ == '__main__':
    main()
