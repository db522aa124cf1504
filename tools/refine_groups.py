#!/usr/bin/env python3
"""Cached row lengths of the lists the refine walks, and the trips a wavefront of the refine makes over them when a row is served by a
group of LPR lanes (csrc/kernels_igraph.hip d_pairlist_refine).  CPU only: the lists are the all-pairs yardstick of tests/walked_lists.py
at cache_cutoff on the oracle's node outputs at the golden positions, i.e. the cached lists right after a rebuild.

    python tools/refine_groups.py [fixture ...]      (default: syn300_10A proteinG56_7A syn150_10A)

Model.  A wavefront serves a contiguous run of rows; its 64 / LPR groups take 64 / LPR consecutive rows (a set) and advance together,
LPR words of every row per trip, until the longest row of the set is done: trips(set) = ceil(max cnt / LPR).  LPR = 64 stands for the
two-rows-per-trip body this replaces (a set is two rows, a trip tests 64 words of each).  Every trip issues the same instructions
whatever its lanes carry, so trips per row is what the instruction count follows; `fill` is the share of the lanes of those trips that
carry a cached word."""
import os
import sys
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LPRS = (16, 32, 64)
# (node, walked side, skin scale of a batch that fills the device: launch_plan.h plan_skin_scale, rows per wavefront: plan_refine_rows / 4)
WALKED = [('rotamer', 1, 0.5), ('hbond_coverage', 2, 0.75), ('hbond_coverage_hydrophobe', 2, 0.75), ('environment_coverage', 1, 0.75)]


def rows_per_set(lpr):
    return 2 if lpr == 64 else 64 // lpr


def trips_of_run(cnt, lpr):
    """(trips, sets) of one wavefront over its run of rows with cached lengths cnt, in run order"""
    cnt = np.asarray(cnt, 'i8'); g = rows_per_set(lpr)
    n_set = (len(cnt) + g - 1) // g
    padded = np.zeros(n_set * g, 'i8'); padded[:len(cnt)] = cnt
    longest = padded.reshape(n_set, g).max(1)
    return int(((longest + lpr - 1) // lpr).sum()), n_set


def trips_of_rows(cnt, lpr, rows_per_wave):
    """(trips, sets, wavefronts) over all rows of a system: runs of rows_per_wave rows in row order"""
    t = s = w = 0
    for r0 in range(0, len(cnt), rows_per_wave):
        a, b = trips_of_run(cnt[r0:r0 + rows_per_wave], lpr)
        t += a; s += b; w += 1
    return t, s, w


def expected_trips_per_set(hist, lpr):
    """E[ceil(max cnt / LPR)] of a set whose rows draw their lengths independently from the histogram hist[length] = rows"""
    h = np.asarray(hist, 'f8'); p = h / h.sum()
    trips = (np.arange(len(h)) + lpr - 1) // lpr
    cdf = np.zeros(int(trips.max()) + 1)
    np.add.at(cdf, trips, p)
    cdf = np.cumsum(cdf) ** rows_per_set(lpr)          # P(max <= t)
    pmf = np.diff(np.concatenate(([0.], cdf)))
    return float((np.arange(len(pmf)) * pmf).sum())


def histogram_lines(cnt, width=16):
    c = np.asarray(cnt); top = int(c.max()) if len(c) else 0
    out = []
    for lo in range(0, top + 1, width):
        n = int(((c >= lo) & (c < lo + width)).sum())
        out.append('    %4d..%-4d %6d %s' % (lo, lo + width - 1, n, '#' * int(round(60. * n / max(len(c), 1)))))
    return out


def cached_row_lengths(fixture, pos=None, skin=None):
    """{(node, side): cached row lengths} for the walked lists of WALKED at the golden positions (or pos), with the skin scales of a
    batch that fills the device (or skin for every graph)"""
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    import parity_util as P
    import walked_lists as WL
    pos = np.ascontiguousarray(P.golden(fixture)['pos'] if pos is None else pos, 'f4')
    up = P.pkg.Upside(P.fixture(fixture), library=P.oracle_library())
    up.deriv(pos)
    out = {}
    for node, side, skin_full in WALKED:
        sp = WL.graph_spec(P.pkg.h5lite, P.fixture(fixture), node)
        o = {nm: up.get_output(nm) for nm in {sp['source1'], sp['source2']}}
        cut = WL.graph_cutoff(sp)
        cache = np.float32(cut + np.float32(skin_full if skin is None else skin) * (np.float32(1.) + np.float32(0.2) * cut))
        m = WL.in_range_matrix(o[sp['source1']][sp['index1'], :3], o[sp['source2']][sp['index2'], :3], sp['id1'], sp['id2'], cache,
                               sp['itype'], sp['symmetric'])
        out[(node, side)] = (m.sum(1) if side == 1 else m.sum(0)).astype('i8')
    up.close()
    return out


def report(fixture, out=sys.stdout):
    for (node, side), cnt in sorted(cached_row_lengths(fixture).items()):
        per_wave = 32 if len(cnt) <= 512 else 64        # plan_refine_rows: 128 rows per 4-wavefront workgroup up to 512 rows, else 256
        out.write('%s %s side %d: %d rows, %d cached words, mean %.1f, median %d, max %d; %d rows per wavefront\n' % (
            fixture, node, side, len(cnt), cnt.sum(), cnt.mean(), np.median(cnt), cnt.max(), per_wave))
        out.write('\n'.join(histogram_lines(cnt)) + '\n')
        hist = np.bincount(cnt)
        for lpr in LPRS:
            t, s, w = trips_of_rows(cnt, lpr, per_wave)
            out.write('    LPR %2d: %6.1f trips and %4.1f sets per wavefront, %.3f trips per row (independent rows: %.3f), fill %.2f\n' % (
                lpr, t / w, s / w, t / len(cnt), expected_trips_per_set(hist, lpr) / rows_per_set(lpr),
                cnt.sum() / (t * (128. if lpr == 64 else 64.))))


if __name__ == '__main__':
    for name in sys.argv[1:] or ['syn300_10A', 'proteinG56_7A', 'syn150_10A']:
        report(name)
