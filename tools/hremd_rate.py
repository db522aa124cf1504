"""Time a 64-window Hamiltonian ladder of protein G three ways, on the GPU, and write profiles/hremd_rate.txt.

    python tools/hremd_rate.py --windows 64 --rounds 600 --group-rounds 60

The ladder: copies of tests/golden/proteinG56_7A.up with the dist_spring equilibrium lengths stretched and the backbone
hydrogen-bond energy scaled per window (an umbrella plus a Hamiltonian scale), temperatures 0.80 .. 0.90.  Each way runs
`upside_main` in a fresh process (--no-output, one frame) and reports its own loop time (the "us/systems/step" it prints):
  merged    one engine holds every window (the default grouping), swap sets on the device (upside_hip_hamiltonian_swap);
  per-group UPSIDE_HIP_HAMILTONIAN_BATCH=0: one engine per window, the host procedure for every pair;
  identical 64 copies of one file, temperature exchange: the roof.
Each with exchange every 5 rounds (two alternating swap sets) and with exchange off.  Then, on one merged engine, the mean
time of one hamiltonian_swap set and of one MD round (3 steps), each call ending in a synchronisation."""
import argparse
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile
import time
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
DT = 0.009


def make_ladder(d, n, identical):
    import hamiltonian_files as H
    fs = []
    for i in range(n):
        f = H.copy_fixture('proteinG56_7A', os.path.join(d, 'w%02d.up' % i))
        if not identical:
            H.rewrite(f, 'dist_spring', 'equil_dist', lambda v, i=i: v * (1. + 0.002 * i))
            H.scale_hbond(f, 1. - 0.004 * i)
        fs.append(f)
    return fs


def child_main(files, rounds, exchange):
    from __graft_entry__ import load_package
    pkg = load_package()
    n = len(files)
    duration = rounds * 3 * DT
    args = ['--duration', repr(duration), '--frame-interval', repr(duration), '--no-output', '--seed', '7',
            '--temperature', ','.join('%.4f' % t for t in np.linspace(0.80, 0.90, n))]
    if exchange:
        args += ['--replica-interval', repr(5 * 3 * DT),
                 '--swap-set', ','.join('%d-%d' % (i, i + 1) for i in range(0, n - 1, 2)),
                 '--swap-set', ','.join('%d-%d' % (i, i + 1) for i in range(1, n - 1, 2))]
    pkg.default_library().in_process_upside(args + files, verbose=False)


def swap_cost(files, n_call):
    from __graft_entry__ import load_package
    pkg = load_package()
    import parity_util as P
    n = len(files)
    ens = pkg.engine.Ensemble.from_files(files)
    ens.set_pos(P.golden('proteinG56_7A')['pos'])
    ens.init_md(np.linspace(0.80, 0.90, n), 7)
    sets = [np.array([[i, i + 1] for i in range(0, n - 1, 2)]), np.array([[i, i + 1] for i in range(1, n - 1, 2)])]
    ens.run_rounds(20)
    ens.hamiltonian_swap(sets[0], 7, 1, 0, want_accepted=True)
    t0 = time.perf_counter()
    for k in range(n_call):
        ens.run_rounds(1)
    t_round = (time.perf_counter() - t0) / n_call
    t0 = time.perf_counter()
    n_acc = 0
    for k in range(n_call):
        acc, _ = ens.hamiltonian_swap(sets[k % 2], 7, 2 + k, 0, want_accepted=True)
        n_acc += int(acc.sum())
    t_swap = (time.perf_counter() - t0) / n_call
    print(json.dumps({'md_round_ms': t_round * 1e3, 'hamiltonian_swap_ms': t_swap * 1e3, 'accepted_fraction': n_acc / float(n_call * len(sets[0]))}))


def run_child(mode, files, rounds, exchange, timeout):
    env = dict(os.environ)
    if mode == 'per-group':
        env['UPSIDE_HIP_HAMILTONIAN_BATCH'] = '0'
    cmd = [sys.executable, os.path.abspath(__file__), '--child', str(rounds), '1' if exchange else '0'] + files
    out = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=timeout, env=env)
    text = out.stdout.decode(errors='replace')
    if out.returncode:
        raise RuntimeError('%s exited with %d:\n%s' % (mode, out.returncode, text[-2000:]))
    m = re.search(r'finished in ([0-9.]+) seconds \(([0-9.]+) us/systems/step', text)
    us = float(m.group(2))
    return {'mode': mode, 'exchange': bool(exchange), 'rounds': rounds, 'seconds': float(m.group(1)), 'us_per_system_step': us,
            'system_steps_per_s': 1e6 / us}


def main():
    if len(sys.argv) > 1 and sys.argv[1] == '--child':
        return child_main(sys.argv[4:], int(sys.argv[2]), sys.argv[3] == '1')
    if len(sys.argv) > 1 and sys.argv[1] == '--swap-cost':
        return swap_cost(sys.argv[3:], int(sys.argv[2]))
    ap = argparse.ArgumentParser()
    ap.add_argument('--windows', type=int, default=64)
    ap.add_argument('--rounds', type=int, default=600, help='MD rounds (3 steps) of the merged and identical runs')
    ap.add_argument('--group-rounds', type=int, default=60, help='MD rounds of the per-group runs (one engine per window)')
    ap.add_argument('--timeout', type=int, default=900, help='seconds allowed to each child run')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'hremd_rate.txt'))
    a = ap.parse_args()
    d = tempfile.mkdtemp(prefix='hremd_rate_')
    try:
        ladder = make_ladder(os.path.join(d), a.windows, False)
        os.makedirs(os.path.join(d, 'same'))
        same = make_ladder(os.path.join(d, 'same'), a.windows, True)
        rows = []
        for exchange in (False, True):
            rows.append(run_child('merged', ladder, a.rounds, exchange, a.timeout))
            rows.append(run_child('identical', same, a.rounds, exchange, a.timeout))
            rows.append(run_child('per-group', ladder, a.group_rounds, exchange, a.timeout))
        cost = subprocess.run([sys.executable, os.path.abspath(__file__), '--swap-cost', '50'] + ladder, stdout=subprocess.PIPE,
                              stderr=subprocess.STDOUT, timeout=a.timeout)
        if cost.returncode:
            raise RuntimeError(cost.stdout.decode(errors='replace')[-2000:])
        cost = json.loads(cost.stdout.decode().strip().splitlines()[-1])
    finally:
        shutil.rmtree(d, ignore_errors=True)
    rate = {(r['mode'], r['exchange']): r['system_steps_per_s'] for r in rows}
    lines = ['# tools/hremd_rate.py: %d-window protein G ladder (proteinG56_7A, dist_spring umbrella + scaled hbond_energy), upside_main --no-output'
             % a.windows, '# mode        exchange  rounds  loop_s   us/system/step  system-steps/s']
    for r in rows:
        lines.append('%-12s  %-8s  %6d  %7.2f  %14.3f  %14.0f' % (r['mode'], 'every5' if r['exchange'] else 'off', r['rounds'], r['seconds'],
                                                               r['us_per_system_step'], r['system_steps_per_s']))
    lines.append('merged / identical, exchange off: %.3f' % (rate[('merged', False)] / rate[('identical', False)]))
    lines.append('merged / identical, exchange every 5 rounds: %.3f' % (rate[('merged', True)] / rate[('identical', True)]))
    lines.append('merged / per-group, exchange every 5 rounds: %.1f' % (rate[('merged', True)] / rate[('per-group', True)]))
    lines.append('one hamiltonian_swap set (%d pairs, synchronised): %.3f ms; one MD round (3 steps, synchronised): %.3f ms; accepted fraction %.2f'
                 % (a.windows // 2, cost['hamiltonian_swap_ms'], cost['md_round_ms'], cost['accepted_fraction']))
    lines.append('JSON ' + json.dumps({'rows': rows, 'swap_cost': cost}))
    txt = '\n'.join(lines) + '\n'
    with open(a.out, 'w') as f:
        f.write(txt)
    print(txt)


if __name__ == '__main__':
    main()
