"""Cost of recording collective variables inside the MD loop, on the GPU.

    python tools/cv_rate.py --config syn300_10A --systems 4096 --steps 30 --runs 5

--config is a fixture name (tests/golden/<name>.up) or a path.  ONE engine of --systems replicas defines four CVs over the CA atoms
(rg, rmsd and contacts to the input structure, end-to-end distance) and runs --steps MD steps (a multiple of 3: whole rounds) under
three conditions taken in turn, --runs times each: recording off, recording every round, recording every 10th round.  Switching
the recording invalidates the captured MD graph, so every timed run follows an untimed run of the same length under the same
condition.  Reported: the mean step time of every run, mean and spread (max - min) per condition, the overhead of the two recording
conditions against recording off, system-steps/s of recording off (to set against bench.py of the parent commit on the same
machine), and the time of one cvs() call (launch + 64 KB read back, synchronising; mean of 20 after a warm-up call).
Prints one JSON line."""
import argparse
import json
import os
import sys
import time
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from __graft_entry__ import load_package  # noqa: E402

CONDITIONS = (('off', 0), ('every_round', 1), ('every_10th_round', 10))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--config', default='syn300_10A')
    ap.add_argument('--systems', type=int, default=4096)
    ap.add_argument('--steps', type=int, default=30)
    ap.add_argument('--runs', type=int, default=5)
    ap.add_argument('--settle', type=int, default=102, help='untimed steps before anything is measured (de-phases the pair-list rebuilds)')
    args = ap.parse_args()
    if args.steps % 3:
        raise SystemExit('cv_rate.py: --steps must be a multiple of 3 (whole rounds)')
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('cv_rate.py: no GPU')
    pkg = load_package()
    path = args.config if os.path.exists(args.config) else os.path.join(ROOT, 'tests', 'golden', args.config + '.up')
    S = args.systems
    sync = torch.cuda.synchronize
    ens = pkg.engine.BatchEngine(path, S)
    specs = pkg.config.default_collective_variables(ens.initial_pos)
    assert [sp['kind'] for sp in specs] == ['rg', 'rmsd', 'contacts', 'distance']
    ens.define_cvs(specs)
    rs = np.random.RandomState(1)
    ens.set_pos(ens.initial_pos[None] + np.float32(0.05) * rs.normal(size=(S,) + ens.initial_pos.shape).astype('f4'))
    ens.init_md(0.8, 1000)
    ens.run_steps(args.settle)
    sync()
    capacity = 2 * (args.steps // 3) + 2          # the untimed and the timed run of one condition
    step_ms = {tag: [] for tag, _ in CONDITIONS}
    n_sample = {}
    for _ in range(args.runs):
        for tag, every in CONDITIONS:
            ens.record_cvs(every, capacity if every else 0)
            ens.run_steps(args.steps)            # untimed: graph capture under this condition
            sync()
            t0 = time.perf_counter()
            ens.run_steps(args.steps)
            sync()
            step_ms[tag].append(round(1e3 * (time.perf_counter() - t0) / args.steps, 4))
            if every:
                n_sample[tag] = ens.cv_counts()[0]
    ens.record_cvs(0)
    mean = {t: float(np.mean(v)) for t, v in step_ms.items()}
    out = dict(config=os.path.basename(path), systems=S, steps=args.steps, runs=args.runs,
               n_cv=len(specs), n_contact_pairs=int(len(specs[2]['pairs'])), step_ms=step_ms,
               step_ms_mean={t: round(m, 4) for t, m in mean.items()},
               step_ms_spread={t: round(float(np.max(v) - np.min(v)), 4) for t, v in step_ms.items()},
               samples_per_condition=n_sample,
               system_steps_per_s_off=round(S / (mean['off'] * 1e-3), 1),
               overhead_ms_per_step={t: round(mean[t] - mean['off'], 4) for t in mean if t != 'off'},
               overhead_fraction={t: round(mean[t] / mean['off'] - 1., 5) for t in mean if t != 'off'})
    ens.cvs()
    sync()
    t0 = time.perf_counter()
    for _ in range(20):
        ens.cvs()
    out['cvs_call_ms'] = round(1e3 * (time.perf_counter() - t0) / 20, 4)
    print(json.dumps(out))
    ens.close()


if __name__ == '__main__':
    main()
