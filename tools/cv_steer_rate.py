"""Cost of a cv_steer node in the MD loop, on the GPU.

    python tools/cv_steer_rate.py --config syn300_10A --systems 4096 --steps 30 --runs 5

--config is a fixture name (tests/golden/<name>.up) or a path.  Two engines of --systems replicas are built from it: one unchanged,
one with a cv_steer node holding Rg, rmsd and Q (the native contacts within 8 A) over the CA atoms, the centres starting near the
input structure's values and moving slowly (1e-4 of the offset per round) with small spring constants, so that the trajectory stays
that of the benchmark while both kernels do all their work: k_cv_steer in every force pass, k_cv_steer_advance at the end of every
round.  The two run --steps MD steps (a multiple of 3: whole rounds) in turn, --runs times each; every timed run follows an untimed
run of the same length of the same engine.  Reported: the mean step time of every run, mean and spread (max - min) per engine, the
difference, clock and work of system 0 at the end, and the time of one cvs() call of the same three CVs (launch + read back,
synchronising; mean of 20 after a warm-up call) for comparison.  Prints one JSON line.  The time of the two kernels per launch comes
from a kernel trace of this tool, taken in a run of its own."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--config', default='syn300_10A')
    ap.add_argument('--systems', type=int, default=4096)
    ap.add_argument('--steps', type=int, default=30)
    ap.add_argument('--runs', type=int, default=5)
    ap.add_argument('--settle', type=int, default=102, help='untimed steps before anything is measured (de-phases the pair-list rebuilds)')
    args = ap.parse_args()
    if args.steps % 3:
        raise SystemExit('cv_steer_rate.py: --steps must be a multiple of 3 (whole rounds)')
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('cv_steer_rate.py: no GPU')
    pkg = load_package()
    path = args.config if os.path.exists(args.config) else os.path.join(ROOT, 'tests', 'golden', args.config + '.up')
    S = args.systems
    sync = torch.cuda.synchronize
    work = tempfile.mkdtemp(prefix='cv_steer_rate_')
    try:
        with_node = os.path.join(work, 'with_node.up')
        shutil.copyfile(path, with_node)
        pos0 = pkg.config.read_pos(path).astype('f8')
        specs = [sp for sp in pkg.config.default_collective_variables(pos0) if sp['kind'] != 'distance']
        assert [sp['kind'] for sp in specs] == ['rg', 'rmsd', 'contacts']
        probe = pkg.engine.BatchEngine(path, 1)
        probe.define_cvs(specs); probe.set_pos(pos0.astype('f4'))
        v0 = probe.cvs()[0]
        probe.close()
        offset = (0.5, 1.0, -0.1)
        steered = [dict(sp, center=float(v0[c]) + offset[c], center_end=float(v0[c]) + 2. * offset[c], rate=1e-4 * offset[c], spring_const=(0.5, 0.5, 20.)[c])
                   for c, sp in enumerate(specs)]
        pkg.config.add_cv_steer(with_node, steered)
        engines = {}
        for tag, p in (('without', path), ('with', with_node)):
            ens = pkg.engine.BatchEngine(p, S)
            rs = np.random.RandomState(1)
            ens.set_pos(ens.initial_pos[None] + np.float32(0.05) * rs.normal(size=(S,) + ens.initial_pos.shape).astype('f4'))
            ens.init_md(0.8, 1000)
            ens.run_steps(args.settle)
            engines[tag] = ens
        sync()
        step_ms = {tag: [] for tag in engines}
        for _ in range(args.runs):
            for tag, ens in engines.items():
                ens.run_steps(args.steps)            # untimed
                sync()
                t0 = time.perf_counter()
                ens.run_steps(args.steps)
                sync()
                step_ms[tag].append(round(1e3 * (time.perf_counter() - t0) / args.steps, 4))
        mean = {t: float(np.mean(v)) for t, v in step_ms.items()}
        out = dict(config=os.path.basename(path), systems=S, steps=args.steps, runs=args.runs, n_cv=len(specs),
                   n_contact_pairs=int(len(specs[2]['pairs'])), step_ms=step_ms, step_ms_mean={t: round(m, 4) for t, m in mean.items()},
                   step_ms_spread={t: round(float(np.max(v) - np.min(v)), 4) for t, v in step_ms.items()},
                   node_ms_per_step=round(mean['with'] - mean['without'], 4), node_fraction=round(mean['with'] / mean['without'] - 1., 5),
                   steer_values_of_system_0=np.round(engines['with'].steer_values('cv_steer')[0], 4).tolist())
        state = engines['with'].steer_state('cv_steer')
        out.update(clock_of_system_0=int(state['clock'][0]), work_of_system_0=float(state['work'][0]), centers_of_system_0=np.round(state['center'][0], 6).tolist(),
                   clocks_all_equal=bool((state['clock'] == state['clock'][0]).all()), work_finite=bool(np.isfinite(state['work']).all()))
        ens = engines['without']
        ens.define_cvs(specs)
        ens.cvs()
        sync()
        t0 = time.perf_counter()
        for _ in range(20):
            ens.cvs()
        out['cvs_call_ms'] = round(1e3 * (time.perf_counter() - t0) / 20, 4)
        for ens in engines.values():
            ens.close()
        print(json.dumps(out))
    finally:
        shutil.rmtree(work, ignore_errors=True)


if __name__ == '__main__':
    main()
