"""Cost of a cv_restraint node in the MD loop, on the GPU.

    python tools/cv_restraint_rate.py --config syn300_10A --systems 4096 --steps 30 --runs 5

--config is a fixture name (tests/golden/<name>.up) or a path.  Two engines of --systems replicas are built from it: one unchanged,
one with a cv_restraint node holding Rg, rmsd and Q (the native contacts within 8 A) over the CA atoms, centred on the input
structure's values with small spring constants (the trajectory stays that of the benchmark).  The two run --steps MD steps (a
multiple of 3: whole rounds) in turn, --runs times each; every timed run follows an untimed run of the same length of the same engine.
Reported: the mean step time of every run, mean and spread (max - min) per engine, the difference, and the time of one cvs() call of
the same three CVs (launch + read back, synchronising; mean of 20 after a warm-up call) for comparison.  Prints one JSON line.
With --md-means it also runs the MD check of tests/test_gpu_cv_restraint.py once (tests/cv_restraint_gpu_worker.py md, in a child
process: trpcage20_7A, 8 systems, T = 0.8, Rg over the CA atoms, k = 50, centres 0.7 and 1.5 x Rg0, 200 rounds) and adds the mean Rg
of every window over the last 100 rounds as that check prints them."""
import argparse
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from __graft_entry__ import load_package  # noqa: E402


def md_means(work):
    """the MD check of tests/test_gpu_cv_restraint.py (tests/cv_restraint_gpu_worker.py md), run once in a child process: the means
    it prints on its MD_MEANS line, so that the profile quotes the test's own run and constants"""
    worker = os.path.join(ROOT, 'tests', 'cv_restraint_gpu_worker.py')
    r = subprocess.run([sys.executable, worker, 'md', work], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300,
                       env=dict(os.environ, UPSIDE_HIP_GRAPH='1'))
    out = r.stdout.decode()
    if r.returncode:
        raise SystemExit('cv_restraint_rate.py: the MD check ended with status %d:\n%s' % (r.returncode, out[-2000:]))
    return json.loads([l for l in out.splitlines() if l.startswith('MD_MEANS ')][-1][len('MD_MEANS '):])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--config', default='syn300_10A')
    ap.add_argument('--systems', type=int, default=4096)
    ap.add_argument('--steps', type=int, default=30)
    ap.add_argument('--runs', type=int, default=5)
    ap.add_argument('--settle', type=int, default=102, help='untimed steps before anything is measured (de-phases the pair-list rebuilds)')
    ap.add_argument('--md-means', action='store_true')
    args = ap.parse_args()
    if args.steps % 3:
        raise SystemExit('cv_restraint_rate.py: --steps must be a multiple of 3 (whole rounds)')
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('cv_restraint_rate.py: no GPU')
    pkg = load_package()
    path = args.config if os.path.exists(args.config) else os.path.join(ROOT, 'tests', 'golden', args.config + '.up')
    S = args.systems
    sync = torch.cuda.synchronize
    work = tempfile.mkdtemp(prefix='cv_restraint_rate_')
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
        restrained = [dict(sp, center=float(v0[c]) + (0.5, 1.0, -0.1)[c], spring_const=(0.5, 0.5, 20.)[c]) for c, sp in enumerate(specs)]
        pkg.config.add_cv_restraint(with_node, restrained)
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
                   restraint_values_of_system_0=np.round(engines['with'].restraint_values('cv_restraint')[0], 4).tolist())
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
        if args.md_means:
            out['md_means'] = md_means(work)
        print(json.dumps(out))
    finally:
        shutil.rmtree(work, ignore_errors=True)


if __name__ == '__main__':
    main()
