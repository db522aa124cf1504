"""Child process of tests/test_gpu_refine_groups.py: the hit lists of the list refine (csrc/kernels_igraph.hip d_pairlist_refine: a row served
by a group of LPR lanes, 64 / LPR rows per wavefront trip) at the row lengths and row counts where its trips change,

    python tests/refine_groups_gpu_worker.py CHECK [ARG ...]

under whatever UPSIDE_HIP_* environment the parent set.  The lists are read with Ensemble.walked_lists and checked by
walked_lists.check_graph against the oracle's pair lists at the device's positions; every comparison is exact.  Every tally is printed
before it is asserted, and the run ends with 'CHECK <name> PASSED'."""
import os
import re
import sys
import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import parity_util as P                        # noqa: E402
import walked_lists as WL                      # noqa: E402
import walked_lists_gpu_worker as WG           # noqa: E402

Ensemble = P.pkg.engine.Ensemble
# Structures of `static`: as shipped, and proteinG56_7A compressed and stretched about its centroid.  The factors were chosen on the CPU
# (tools/refine_groups.py cached_row_lengths with the 1.5 skin scale of a small batch, i.e. the yardstick on the oracle's node outputs):
# pooled over these structures, the cached rows of the 16-bit lists and of the 32-bit list each fill every class of lpr_classes for LPR 16
# and for LPR 32 (16-bit, LPR 16: 397 empty rows, 526 of 1..15, 10 of 16, 189 of 17..32, 491 longer, 53 / 131 / 56 with cnt % 16 = 0 / 1 / 15;
# 32-bit, LPR 16: 2, 209, 3, 80, 416, 45 / 33 / 41).  edge_gly5 has 5 rows per side, fewer than the groups of one wavefront, and empty rows.
STRUCTURES = [('edge_gly5', 1.0), ('trpcage20_7A', 1.0), ('proteinG56_7A', 1.0), ('proteinG56_7A', 0.5), ('proteinG56_7A', 2.0)]


def lanes_per_row():
    """{list word width: LPR} as compiled (csrc/launch_plan.h)"""
    text = open(os.path.join(P.ROOT, 'upside-md_amd', 'csrc', 'launch_plan.h')).read()
    got = {w: int(re.search(r'^#define %s (\d+)' % name, text, re.M).group(1)) for w, name in ((32, 'PLR_LPR_SYM'), (16, 'PLR_LPR_W16'))}
    assert all(v in (16, 32) for v in got.values()), got
    return got


def lpr_classes(cnt, lpr):
    """tally of cached row lengths by the classes at which the trips of a group of lpr lanes change"""
    c = np.asarray(cnt)
    return {'0': int((c == 0).sum()), '1..LPR-1': int(((c >= 1) & (c < lpr)).sum()), 'LPR': int((c == lpr).sum()),
            'LPR+1..2LPR': int(((c > lpr) & (c <= 2 * lpr)).sum()), '>2LPR': int((c > 2 * lpr).sum()),
            '%LPR==0': int(((c > 0) & (c % lpr == 0)).sum()), '%LPR==1': int((c % lpr == 1).sum()), '%LPR==LPR-1': int((c % lpr == lpr - 1).sum())}


def rows_per_run(S, n_cu, n_rows):
    """rows of a wavefront's run (launch_plan.h plan_refine_rows, a quarter of a workgroup's rows)"""
    rows = 256 if S >= n_cu else (64 if S >= 16 else 16)
    return (128 if n_rows <= 512 and rows > 128 else rows) // 4


def static(size):
    import torch
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    S = int(size)
    lpr = lanes_per_row()
    print('%d systems, lanes per row %r, switches %r' % (S, lpr, {k: v for k, v in os.environ.items() if k.startswith('UPSIDE_HIP_')}))
    by_width = {16: [], 32: []}
    ragged = []
    for name, f in STRUCTURES:
        if S > 3 and name != 'proteinG56_7A':
            continue
        g = P.golden(name)
        starts = [g['pos'], g.get('pos2', g['pos']), g['pos']]
        pos = np.stack([WG.scaled(starts[s % 3], f) if f != 1.0 else np.ascontiguousarray(starts[s % 3], 'f4') for s in range(S)])
        specs = {n: WL.graph_spec(P.pkg.h5lite, P.fixture(name), n) for n in WL.ORACLE_GRAPHS}
        oracle = WG.Oracle(name)
        ens = Ensemble(P.fixture(name), S)          # a fresh engine: the first pass builds and refines every list
        ens.set_pos(pos)
        ens.energies_and_derivs()
        t = {}
        for s in sorted({0, 1, 2, S - 1} & set(range(S))):
            WG.check_system(ens, oracle, specs, WL.ORACLE_GRAPHS, s, pos[s], True, t)
        for node in WL.ORACLE_GRAPHS:
            if node == 'protein_hbond':             # (its rows of three words go through k_pairlist_refine_short)
                continue
            for r in WG.records_of(ens, node, 0):
                if r['hit'] is None:
                    continue
                w = r['word_bits']
                by_width[w].append(r['cnt'])
                n_rows = r['n_rows']
                if n_rows % (64 // lpr[w]) and n_rows % rows_per_run(S, n_cu, n_rows):
                    ragged.append((name, node, r['side'], n_rows))
        ens.close()
        print('%s x%.2f' % (name, f)); WG.print_tallies(t)
    ok = True
    for w in (16, 32):
        cls = lpr_classes(np.concatenate(by_width[w]), lpr[w])
        print('cached row lengths of the %d-bit lists the refine walked, LPR %d: %r' % (w, lpr[w], cls))
        ok &= all(v > 0 for v in cls.values())
    print('graphs whose row count is no multiple of a set or of a wavefront\'s run: %r' % ragged)
    if S <= 3:
        assert ok, 'a class of cached row lengths is empty'
    assert ragged, 'every row count is a multiple of the rows of a set or of a run'


def md(size):
    """trpcage20_7A at a batch size past the device's CU count: 256 rows per workgroup; a few MD steps, so that some systems rebuild their
    lists and some only refine them"""
    import torch
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    S = n_cu + 8 if size == 'ncu+8' else int(size)
    name = 'trpcage20_7A'
    g = P.golden(name)
    specs = {n: WL.graph_spec(P.pkg.h5lite, P.fixture(name), n) for n in WL.ORACLE_GRAPHS}
    oracle = WG.Oracle(name)
    rng = np.random.RandomState(11)
    starts = [g['pos'], g.get('pos2', g['pos'])]
    pos0 = np.stack([starts[s % 2] for s in range(S)]).astype('f4') + (0.02 * rng.randn(S, g['pos'].shape[0], 3)).astype('f4')
    ens = Ensemble(P.fixture(name), S)
    ens.set_pos(pos0)
    ens.init_md(np.linspace(0.5, 1.5, S).astype('f4'), 5)
    print('%s, %d systems (%d CUs)' % (name, S, n_cu))
    tallies = {}
    n_some = 0
    for i, k in enumerate((0, 1, 5, 6, 7)):
        if k:
            ens.run_steps(k)
        ens.energies_and_derivs()
        pos = ens.get_pos()
        assert np.isfinite(pos).all()
        oracle.forget()
        line = []
        for node in WL.ORACLE_GRAPHS:
            fl = ens.rebuild_flags(node)
            n_fl = int((fl != 0).sum())
            n_some += 0 < n_fl < S
            quiet = np.flatnonzero(fl == 0); flagged = np.flatnonzero(fl)
            systems = sorted({0, S - 1} | set(flagged[:3].tolist()) | set(quiet[:3].tolist()))
            for s in systems:
                WG.check_system(ens, oracle, specs, [node], s, pos[s], i == 0, tallies)
            line.append('%s %d/%d' % (node, n_fl, len(systems)))
        print('after run_steps(%d): rebuilt/checked: %s' % (k, '; '.join(line)))
    ens.close()
    WG.print_tallies(tallies)
    print('check points of a graph at which some systems rebuilt and some did not: %d' % n_some)
    assert n_some > 0


CHECKS = dict(static=static, md=md)

if __name__ == '__main__':
    which = sys.argv[1]
    CHECKS[which](*sys.argv[2:])
    print('CHECK %s PASSED' % which)
