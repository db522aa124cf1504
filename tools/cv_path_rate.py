"""Cost of the path collective variables (kinds path_s / path_z, csrc/cv_path_device.h), on the GPU.

    python tools/cv_path_rate.py --config syn300_10A --systems 4096 --frames 8,32,64 --steps 30 --runs 5

--config is a fixture name (tests/golden/<name>.up) or a path.  The selection is every CA atom; a path of K frames runs from the
input structure to the input structure plus seeded smooth noise of 4 A (config.interpolate_path), lambda = config.path_lambda.  For
every K of --frames, on one engine of --systems replicas:
  cvs_ms        one cvs() call with ONE path_s of K frames: launch, kernel and read-back, synchronising (mean of --calls calls after
                a warm-up call);
  rmsd_cvs_ms   the same K frames as K separate rmsd CVs through one cvs() call: the serial form (one alignment after the other, each
                with its own block reductions and its eigenproblem on one lane) that the path kernel replaces;
  floor_ms      one cvs() call with a single distance CV: what launch, read-back and synchronisation cost without any alignment.
  The three are measured in turn, --runs times; device time is estimated as the call time minus the floor, and
  path_over_rmsd = (cvs_ms - floor_ms) / (rmsd_cvs_ms - floor_ms).
Then the MD loop: an engine unchanged and one with a cv_restraint on path_s (centred 0.5 above the input structure's s, spring
constant 0.5: the trajectory stays that of the benchmark) run --steps MD steps (a multiple of 3: whole rounds) in turn, --runs times
each; every timed run follows an untimed run of the same length of the same engine.  Prints one JSON line."""
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


def smooth_noise(n_atom, amplitude, rng):
    t = np.arange(n_atom)[:, None] / float(n_atom)
    out = np.zeros((n_atom, 3))
    for m in range(3):
        out += rng.standard_normal(3)[None] * np.sin(2. * np.pi * (m + 1) * t + rng.uniform(0., 2. * np.pi))
    return amplitude * out / np.sqrt(3.)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--config', default='syn300_10A')
    ap.add_argument('--systems', type=int, default=4096)
    ap.add_argument('--frames', default='8,32,64')
    ap.add_argument('--steps', type=int, default=30)
    ap.add_argument('--runs', type=int, default=5)
    ap.add_argument('--calls', type=int, default=20)
    ap.add_argument('--settle', type=int, default=102, help='untimed steps before anything is measured (de-phases the pair-list rebuilds)')
    args = ap.parse_args()
    if args.steps % 3:
        raise SystemExit('cv_path_rate.py: --steps must be a multiple of 3 (whole rounds)')
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('cv_path_rate.py: no GPU')
    pkg = load_package()
    cfg = pkg.config
    path = args.config if os.path.exists(args.config) else os.path.join(ROOT, 'tests', 'golden', args.config + '.up')
    S = args.systems
    sync = torch.cuda.synchronize
    pos0 = cfg.read_pos(path).astype('f8').reshape(-1, 3)
    atoms = np.arange(1, len(pos0), 3, dtype='i4')      # the CA atoms
    end = pos0 + smooth_noise(len(pos0), 4.0, np.random.default_rng(11))
    work = tempfile.mkdtemp(prefix='cv_path_rate_')

    def start(p):
        ens = pkg.engine.BatchEngine(p, S)
        rs = np.random.RandomState(1)
        ens.set_pos(ens.initial_pos[None] + np.float32(0.05) * rs.normal(size=(S,) + ens.initial_pos.shape).astype('f4'))
        ens.init_md(0.8, 1000)
        ens.run_steps(args.settle)
        sync()
        return ens

    def call_ms(ens):
        ens.cvs()
        sync()
        t0 = time.perf_counter()
        for _ in range(args.calls):
            ens.cvs()
        return 1e3 * (time.perf_counter() - t0) / args.calls

    try:
        plain = start(path)
        out = dict(config=os.path.basename(path), systems=S, n_atom_selected=int(len(atoms)), steps=args.steps, runs=args.runs, calls=args.calls, frames={})
        for K in [int(k) for k in args.frames.split(',')]:
            fr = cfg.interpolate_path(pos0[atoms], end[atoms], K)
            s_spec = cfg.path_specs('path', atoms, fr)[0]
            definitions = dict(cvs_ms=[s_spec], rmsd_cvs_ms=[{'name': 'frame%d' % k, 'kind': 'rmsd', 'atoms': atoms, 'ref': fr[k]} for k in range(K)],
                               floor_ms=[{'kind': 'distance', 'pair': (int(atoms[0]), int(atoms[-1]))}])
            ms = dict((k, []) for k in definitions)
            for _ in range(args.runs):
                for k, specs in definitions.items():
                    plain.define_cvs(specs)
                    ms[k].append(round(call_ms(plain), 4))
            plain.define_cvs([s_spec])
            s0 = float(plain.cvs()[0, 0])
            mean = dict((k, float(np.mean(v))) for k, v in ms.items())
            row = dict(ms, **{'lambda': round(float(s_spec['lambda']), 4)})
            row['mean'] = dict((k, round(m, 4)) for k, m in mean.items())
            row['spread'] = dict((k, round(float(np.max(v) - np.min(v)), 4)) for k, v in ms.items())
            row['path_device_ms'] = round(mean['cvs_ms'] - mean['floor_ms'], 4)
            row['rmsd_device_ms'] = round(mean['rmsd_cvs_ms'] - mean['floor_ms'], 4)
            row['path_over_rmsd'] = round((mean['cvs_ms'] - mean['floor_ms']) / (mean['rmsd_cvs_ms'] - mean['floor_ms']), 4)
            # the MD loop with a restraint on s
            with_node = os.path.join(work, 'with_node_%d.up' % K)
            shutil.copyfile(path, with_node)
            cfg.add_cv_restraint(with_node, [dict(s_spec, center=s0 + 0.5, spring_const=0.5)])
            engines = dict(without=plain, **{'with': start(with_node)})
            step_ms = dict((t, []) for t in engines)
            for _ in range(args.runs):
                for tag, ens in engines.items():
                    ens.run_steps(args.steps)            # untimed
                    sync()
                    t0 = time.perf_counter()
                    ens.run_steps(args.steps)
                    sync()
                    step_ms[tag].append(round(1e3 * (time.perf_counter() - t0) / args.steps, 4))
            m = dict((t, float(np.mean(v))) for t, v in step_ms.items())
            row['step_ms'] = step_ms
            row['step_ms_mean'] = dict((t, round(v, 4)) for t, v in m.items())
            row['step_ms_spread'] = dict((t, round(float(np.max(v) - np.min(v)), 4)) for t, v in step_ms.items())
            row['node_ms_per_step'] = round(m['with'] - m['without'], 4)
            row['node_fraction'] = round(m['with'] / m['without'] - 1., 5)
            row['s_of_system_0'] = round(float(engines['with'].restraint_values('cv_restraint')[0, 0]), 4)
            engines['with'].close()
            out['frames'][str(K)] = row
        plain.close()
        print(json.dumps(out))
    finally:
        shutil.rmtree(work, ignore_errors=True)


if __name__ == '__main__':
    main()
