"""Plain-numpy checker of the lists the pair passes walk (upside_hip_get_walked_lists / Ensemble.walked_lists and
upside_hip_get_backbone_list / Ensemble.backbone_list).  No GPU code: the records are dicts of numpy arrays, so the checker is pinned
on hand-made records by tests/test_walked_lists_cases.py and used on the device's records by tests/walked_lists_gpu_worker.py.

The yardstick is the all-pairs definition of an interaction graph's edge set: every pair (i1, i2) whose ids are acceptable
(interaction_graph.h's acceptable_id_pair of the graph type) and whose squared distance ((dx*dx + dy*dy) + dz*dz), every operation
rounded to float32 once, lies below cutoff*cutoff (float32).  All comparisons are exact."""
import numpy as np

ROTAMER, HBOND_COVERAGE, ENVIRONMENT, PROTEIN_HBOND, RADIAL, HBOND_SC_RADIAL = range(6)
# graph type and the sides whose rows the MD path walks, by node type
NODE_ITYPE = {'rotamer': ROTAMER, 'hbond_coverage': HBOND_COVERAGE, 'hbond_coverage_hydrophobe': HBOND_COVERAGE,
              'environment_coverage': ENVIRONMENT, 'protein_hbond': PROTEIN_HBOND, 'radial': RADIAL,
              'hbond_sc_radial': HBOND_SC_RADIAL}
ORACLE_GRAPHS = ['rotamer', 'hbond_coverage', 'hbond_coverage_hydrophobe', 'environment_coverage', 'protein_hbond']
RADIAL_GRAPHS = ['radial', 'hbond_sc_radial']


def canonical_sort(edges):
    """(i1>>2, i2, i1&3): the reference's pair-list order (parity_util.canonical_sort, restated so that this module stands alone)"""
    e = np.asarray(edges, 'i4').reshape(-1, 2)
    return e[np.lexsort((e[:, 0] & 3, e[:, 1], e[:, 0] >> 2))]


def acceptable_id_pair(itype, id1, id2):
    """id1 [n1], id2 [n2] -> bool [n1, n2]"""
    a = np.asarray(id1, 'i8')[:, None]; b = np.asarray(id2, 'i8')[None, :]
    if itype == ROTAMER:
        return (a >> 4) != (b >> 4)
    if itype in (HBOND_COVERAGE, ENVIRONMENT, RADIAL, HBOND_SC_RADIAL):
        return (a - b > 2) | (b - a > 2)
    return np.ones((a.shape[0], b.shape[1]), bool)


def dist2_f32(p1, p2):
    """[n1, 3] x [n2, 3] -> float32 [n1, n2]: ((dx*dx + dy*dy) + dz*dz), one float32 rounding per operation (dist2_exact)"""
    p1 = np.asarray(p1, 'f4'); p2 = np.asarray(p2, 'f4')
    dx = p1[:, None, 0] - p2[None, :, 0]; dy = p1[:, None, 1] - p2[None, :, 1]; dz = p1[:, None, 2] - p2[None, :, 2]
    assert dx.dtype == np.float32
    return (dx * dx + dy * dy) + dz * dz


def in_range_matrix(pos1, pos2, id1, id2, cutoff, itype, symmetric):
    """bool [n1, n2]: the all-pairs definition; a symmetric graph never pairs an element with itself"""
    c = np.float32(cutoff)
    m = (dist2_f32(pos1, pos2) < c * c) & acceptable_id_pair(itype, id1, id2)
    if symmetric:
        m &= ~np.eye(len(m), dtype=bool)
    return m


def edges_yardstick(pos1, pos2, id1, id2, cutoff, itype, symmetric):
    """the edge set (canonical order): (i1, i2) over side 1 x side 2; a symmetric graph (pos2, id2 = pos1, id1) lists a pair once,
    i1 < i2.  With cache_cutoff for `cutoff`: the cached superset."""
    m = in_range_matrix(pos1, pos2, id1, id2, cutoff, itype, symmetric)
    if symmetric:
        m = np.triu(m, 1)
    return canonical_sort(np.argwhere(m))


class WalkedListError(AssertionError):
    pass


def _where(rec, row=None):
    s = 'node %s system %s side %s' % (rec.get('node'), rec.get('system'), rec.get('side'))
    return s + ('' if row is None else ' row %d' % int(row))


def _fail(rec, row, msg):
    raise WalkedListError('%s: %s' % (_where(rec, row), msg))


def _rows_matrix(rec, words, counts):
    """bool [n_rows, n_other] of the partners of every row's first counts[row] words"""
    m = np.zeros((rec['n_rows'], rec['n_other']), bool)
    k = np.arange(rec['cap'])[None, :] < counts[:, None]
    r = np.broadcast_to(np.arange(rec['n_rows'])[:, None], k.shape)[k]
    m[r, words[k]] = True
    return m


def _first_row(bad):
    return int(np.flatnonzero(bad.reshape(len(bad), -1).any(1))[0])


def walked_partners(rec):
    """(counts, partner indices [n_rows, cap]) of what the pair passes visit: the hit lists, or, for a graph that walks its cached lists
    and tests the distance itself (radial), the cached partners in range at cur_pos"""
    if rec['hit'] is not None:
        return rec['hcnt'], rec['hit']
    cnt, nbr, cap = rec['cnt'], rec['nbr'], rec['cap']
    c = np.float32(rec['cutoff'])
    valid = np.arange(cap)[None, :] < cnt[:, None]
    j = np.where(valid, nbr, 0)
    a = rec['cur_rows'][:, None, :]; b = rec['cur_other'][j]
    dx = a[..., 0] - b[..., 0]; dy = a[..., 1] - b[..., 1]; dz = a[..., 2] - b[..., 2]
    ok = valid & (((dx * dx + dy * dy) + dz * dz) < c * c)
    out = np.zeros_like(nbr); n = ok.sum(1).astype('i4')
    for r in np.flatnonzero(n):
        out[r, :n[r]] = nbr[r][ok[r]]
    return n, out


def walked_edges(rec):
    """the edge set the record's rows hold, in the caller's element numbering and canonical order (side 2 transposed to (i1, i2); a
    symmetric graph's pairs once, lower number first)"""
    n, part = walked_partners(rec)
    k = np.arange(rec['cap'])[None, :] < n[:, None]
    rows = np.broadcast_to(np.arange(rec['n_rows'])[:, None], k.shape)[k]
    a = rec['orig_rows'][rows]; b = rec['orig_other'][part[k]]
    if rec['symmetric']:
        if not rec['upper']:
            keep = rows < part[k]
            a, b = a[keep], b[keep]
        e = np.column_stack((np.minimum(a, b), np.maximum(a, b)))
    else:
        e = np.column_stack((a, b)) if rec['side'] == 1 else np.column_stack((b, a))
    return canonical_sort(e)


def check_graph(rec, reference_edges, first_pass=False, source_out=None):
    """every property of one record (tests/test_walked_lists_cases.py lists them).  reference_edges: the edge set in the caller's
    numbering ((i1, i2); a symmetric graph's pairs once); first_pass: the record follows a fresh engine's first force pass (the row
    order is then sorted); source_out: {node name: get_output array of THIS system} to hold cur_pos against, on top of the record's own
    copy of the source rows.  Returns a dict of tallies."""
    n_rows, n_other, cap = rec['n_rows'], rec['n_other'], rec['cap']
    cnt, nbr, nbr_word = rec['cnt'], rec['nbr'], rec['nbr_word']
    has_hit = rec['hit'] is not None
    col = np.arange(cap)[None, :]
    # 3. hcnt <= cnt <= cap
    if ((cnt < 0) | (cnt > cap)).any():
        r = _first_row((cnt < 0) | (cnt > cap)); _fail(rec, r, 'cnt %d outside [0, cap = %d]' % (cnt[r], cap))
    if has_hit:
        hcnt, hit, hit_word = rec['hcnt'], rec['hit'], rec['hit_word']
        if ((hcnt < 0) | (hcnt > cnt)).any():
            r = _first_row((hcnt < 0) | (hcnt > cnt)); _fail(rec, r, 'hcnt %d outside [0, cnt = %d]' % (hcnt[r], cnt[r]))
    # 2. rows strictly ascending, partners in range
    lists = [('cached', cnt, nbr)] + ([('hit', hcnt, hit)] if has_hit else [])
    for what, n, part in lists:
        valid = col < n[:, None]
        oob = valid & ((part < 0) | (part >= n_other))
        if oob.any():
            r = _first_row(oob); _fail(rec, r, '%s row names partner %d of %d' % (what, part[r][oob[r]][0], n_other))
        desc = valid[:, 1:] & (part[:, 1:] <= part[:, :-1])
        if desc.any():
            r = _first_row(desc); k = int(np.flatnonzero(desc[r])[0])
            _fail(rec, r, '%s row is not strictly ascending at word %d: %d then %d' % (what, k + 1, part[r, k], part[r, k + 1]))
    # 4. the hit row is a subsequence of the cached row, words unchanged (ascending rows: a subset with equal words)
    if has_hit:
        by_partner = []
        for part, words, n in ((nbr, nbr_word, cnt), (hit, hit_word, hcnt)):
            m = np.full((n_rows, n_other), -1, 'i8'); v = col < n[:, None]
            m[np.broadcast_to(np.arange(n_rows)[:, None], v.shape)[v], part[v]] = words.view('u4')[v]
            by_partner.append(m)
        bad = (by_partner[1] >= 0) & (by_partner[1] != by_partner[0])
        if bad.any():
            r = _first_row(bad); j = int(np.flatnonzero(bad[r])[0])
            _fail(rec, r, 'hit word 0x%x (partner %d) is not a word of the cached row (there: 0x%x)' % (by_partner[1][r, j], j, by_partner[0][r, j] & 0xFFFFFFFF))
    # 5. hlo = hit partners below the row
    if rec.get('hlo') is not None:
        lo = ((col < hcnt[:, None]) & (hit < np.arange(n_rows)[:, None])).sum(1)
        if (lo != rec['hlo']).any():
            r = _first_row(lo != rec['hlo']); _fail(rec, r, 'hlo %d but %d hit partners lie below the row' % (rec['hlo'][r], lo[r]))
    # 6. / 7. row orders
    n_w, part_w = walked_partners(rec)
    for key_name, key in (('ord', n_w), ('ordu', None if rec.get('hlo') is None else n_w - rec['hlo'])):
        o = rec.get(key_name)
        if o is None:
            continue
        seen = np.bincount(o[(o >= 0) & (o < n_rows)], minlength=n_rows)
        if len(o) != n_rows or (seen != 1).any():
            r = int(np.flatnonzero(seen != 1)[0]) if (seen != 1).any() else -1
            _fail(rec, r, '%s is no permutation of the rows: row %d appears %d times' % (key_name, r, seen[r] if r >= 0 else 0))
        if first_pass:
            k = key[o]
            up = np.flatnonzero(k[1:] > k[:-1])
            if len(up):
                _fail(rec, o[up[0] + 1], '%s is not sorted by descending count: position %d has %d after %d' % (key_name, up[0] + 1, k[up[0] + 1], k[up[0]]))
    # 8. cur_pos has the bits of the source node's output
    for sd in ('rows', 'other'):
        cur = rec['cur_' + sd].view('i4'); src = rec['src_' + sd].view('i4')
        refs = [('the source node %s' % rec.get('source_' + sd), src)]
        if source_out is not None:
            refs.append(('get_output(%s)' % rec['source_' + sd], np.ascontiguousarray(source_out[rec['source_' + sd]][rec['loc_' + sd], :3], 'f4').view('i4')))
        for what, ref in refs:
            if (cur != ref).any():
                r = _first_row(cur != ref)
                _fail(rec, r if sd == 'rows' else None, 'cur_pos of %s element %d %r has not the bits of %s %r' % (
                    'its' if sd == 'rows' else "the other side's", r, rec['cur_' + sd][r].tolist(), what, ref[r].view('f4').tolist()))
    # 9. every pair of the cached superset at cache_pos is in the cached row
    for sd in ('rows', 'other'):
        if (rec['cache_id_' + sd] != rec['id_' + sd]).any():
            r = _first_row(rec['cache_id_' + sd] != rec['id_' + sd]); _fail(rec, r if sd == 'rows' else None, 'cache_pos (%s) carries id %d for element %d, not %d' % (sd, rec['cache_id_' + sd][r], r, rec['id_' + sd][r]))
    id1, id2 = (rec['id_rows'], rec['id_other']) if rec['side'] == 1 else (rec['id_other'], rec['id_rows'])
    sup = in_range_matrix(rec['cache_rows'], rec['cache_other'], rec['id_rows'], rec['id_other'], rec['cache_cutoff'], rec['itype'], rec['symmetric']) \
        if rec['side'] == 1 else \
        in_range_matrix(rec['cache_other'], rec['cache_rows'], id1, id2, rec['cache_cutoff'], rec['itype'], False).T
    if rec['upper']:
        sup = np.triu(sup, 1)
    cached = _rows_matrix(rec, nbr, cnt)
    if (sup & ~cached).any():
        r = _first_row(sup & ~cached); j = int(np.flatnonzero(sup[r] & ~cached[r])[0])
        cc = np.float32(rec['cache_cutoff'])
        _fail(rec, r, 'cached row lacks partner %d, which is within cache_cutoff at cache_pos: d2 %.9g, cache_cutoff2 %.9g; the row holds %d of '
              'capacity %d; %d pairs of the superset are missing in %d rows, %d cached pairs lie outside it; the system %s in the last pass' % (
                  j, dist2_f32(rec['cache_rows'][r:r + 1], rec['cache_other'][j:j + 1])[0, 0], cc * cc, cnt[r], cap, int((sup & ~cached).sum()),
                  int((sup & ~cached).any(1).sum()), int((cached & ~sup).sum()), 'rebuilt' if rec.get('rebuilt') else 'did not rebuild'))
    # 10. rotamer slots
    n_pair_slots = 0
    if rec['itype'] == ROTAMER and rec['nbr_j_bits']:
        if has_hit:
            hs = rec['hit_slot']; v = col < hcnt[:, None]
            bad = v & ((hs == rec['slot_none']) | (hs >= rec['n_slot']) | (hs < 0))
            if bad.any():
                r = _first_row(bad); k = int(np.flatnonzero(bad[r])[0])
                _fail(rec, r, 'hit word %d carries slot %d (n_slot %d, none = %d)' % (k, hs[r, k], rec['n_slot'], rec['slot_none']))
        v = col < cnt[:, None]
        rows = np.broadcast_to(np.arange(n_rows)[:, None], v.shape)[v]
        na = rec['id_rows'][rows].astype('i8') >> 4; nb = rec['id_other'][nbr[v]].astype('i8') >> 4
        key = np.minimum(na, nb) * (1 << 31) + np.maximum(na, nb)
        slot = rec['nbr_slot'][v].astype('i8')
        for a, b, what in ((slot, key, 'slot %d is shared by two node pairs'), (key, slot, 'a node pair (key %d) carries two slots')):
            order = np.lexsort((b, a)); a_s, b_s = a[order], b[order]
            clash = np.flatnonzero((a_s[1:] == a_s[:-1]) & (b_s[1:] != b_s[:-1]))
            if len(clash):
                _fail(rec, rows[order[clash[0] + 1]], what % a_s[clash[0]])
        n_pair_slots = len(np.unique(slot))
    # 1. the edge set equals the reference, pair by pair
    walked = _rows_matrix(rec, part_w, n_w)
    if rec['symmetric'] and not rec['upper']:
        if (walked != walked.T).any():
            r = _first_row(walked != walked.T); j = int(np.flatnonzero(walked[r] != walked.T[r])[0])
            _fail(rec, r, 'row %d holds %d: %s, row %d holds %d: %s' % (r, j, walked[r, j], j, r, walked[j, r]))
    if rec['upper']:
        low = walked & ~np.triu(np.ones_like(walked), 1)
        if low.any():
            r = _first_row(low); _fail(rec, r, 'the upper list holds partner %d, not above its row' % int(np.flatnonzero(low[r])[0]))
    ref = canonical_sort(reference_edges)
    new_rows = np.empty(n_rows, 'i8'); new_rows[rec['orig_rows']] = np.arange(n_rows)
    new_other = np.empty(n_other, 'i8'); new_other[rec['orig_other']] = np.arange(n_other)
    want = np.zeros_like(walked)
    if rec['symmetric']:
        a, b = new_rows[ref[:, 0]], new_rows[ref[:, 1]]
        want[np.minimum(a, b), np.maximum(a, b)] = True
        if not rec['upper']:
            want |= want.T
    elif rec['side'] == 1:
        want[new_rows[ref[:, 0]], new_other[ref[:, 1]]] = True
    else:
        want[new_rows[ref[:, 1]], new_other[ref[:, 0]]] = True
    if (want != walked).any():
        r = _first_row(want != walked); j = int(np.flatnonzero(want[r] != walked[r])[0])
        d2 = dist2_f32(rec['cur_rows'][r:r + 1], rec['cur_other'][j:j + 1])[0, 0]
        _fail(rec, r, '%s partner %d (caller numbering %d, %d): d2 at cur_pos %.9g, cutoff2 %.9g; %d pairs differ in all' % (
            'the row lacks' if want[r, j] else 'the row holds, the reference does not,', j, rec['orig_rows'][r], rec['orig_other'][j],
            d2, np.float32(rec['cutoff']) * np.float32(rec['cutoff']), int((want != walked).sum())))
    got = walked_edges(rec)
    if got.shape != ref.shape or not np.array_equal(got, ref):
        _fail(rec, None, 'the edge list in canonical order differs from the reference (%d against %d edges)' % (len(got), len(ref)))
    return dict(n_edge=len(ref), n_cached=int(cnt.sum()), n_walked=int(n_w.sum()), n_slot_used=n_pair_slots, cnt=cnt.copy())


def cnt_classes(cnt):
    """tally of the cached row lengths by the classes at which the refine's 64-word trips change"""
    c = np.asarray(cnt)
    return {'0': int((c == 0).sum()), '1..63': int(((c >= 1) & (c <= 63)).sum()), '65..128': int(((c >= 65) & (c <= 128)).sum()),
            '>128': int((c > 128).sum()), '%64==0': int(((c > 0) & (c % 64 == 0)).sum()), '%64==1': int((c % 64 == 1).sum()),
            '%64==63': int((c % 64 == 63).sum())}


def check_backbone(rec, centres):
    """the cached residue-pair list of backbone_pairs for one system; centres [n_residue, 3]: the residues' current centres"""
    n, cap, cnt, lst, ids = rec['n_residue'], rec['cap'], rec['cnt'], rec['list'], rec['id']
    col = np.arange(cap)[None, :]
    if ((cnt < 0) | (cnt > cap)).any():
        r = _first_row((cnt < 0) | (cnt > cap)); _fail(rec, r, 'cnt %d outside [0, cap = %d]' % (cnt[r], cap))
    valid = col < cnt[:, None]
    oob = valid & ((lst < 0) | (lst >= n))
    if oob.any():
        r = _first_row(oob); _fail(rec, r, 'row names residue %d of %d' % (lst[r][oob[r]][0], n))
    desc = valid[:, 1:] & (lst[:, 1:] <= lst[:, :-1])
    if desc.any():
        r = _first_row(desc); _fail(rec, r, 'row is not strictly ascending')
    listed = np.zeros((n, n), bool)
    listed[np.broadcast_to(np.arange(n)[:, None], valid.shape)[valid], lst[valid]] = True
    i = np.asarray(ids, 'i8')
    sep = np.abs(i[:, None] - i[None, :]) > 1
    c = np.float32(rec['dist_cutoff']); far = np.float32(rec['dist_cutoff']) + np.float32(rec['skin'])
    near_now = sep & (dist2_f32(centres, centres) < c * c)
    if (near_now & ~listed).any():
        r = _first_row(near_now & ~listed)
        _fail(rec, r, 'row lacks residue %d, which is within dist_cutoff at the current centres' % int(np.flatnonzero(near_now[r] & ~listed[r])[0]))
    too_far = listed & ~(sep & (dist2_f32(rec['ref'], rec['ref']) < far * far))
    if too_far.any():
        r = _first_row(too_far)
        _fail(rec, r, 'row lists residue %d, farther than dist_cutoff + skin at the reference centres (or adjacent in sequence)' % int(np.flatnonzero(too_far[r])[0]))
    return dict(n_listed=int(cnt.sum()), n_near=int(near_now.sum()))


# -- the graphs of a configuration file, for the yardstick ---------------------------------------------------------------------------
def graph_spec(h5lite, config_path, node):
    """index / id of both sides, the source node names and the graph type of interaction-graph node `node` of a configuration"""
    with h5lite.open_file(config_path) as t:
        g = t.group('input/potential/' + node)
        args = [a.decode() if isinstance(a, bytes) else str(a) for a in g.get_attr('arguments')]
        if node == 'rotamer':
            g = g.group('pair_interaction')
        itype = NODE_ITYPE[node]
        symmetric = itype in (ROTAMER, RADIAL)
        if symmetric:
            idx = g.read('index', 'i4'); ids = g.read('id', 'i4')
            return dict(itype=itype, symmetric=True, index1=idx, index2=idx, id1=ids, id2=ids, source1=args[0], source2=args[0],
                        param=g.read('interaction_param', 'f4'))
        return dict(itype=itype, symmetric=False, index1=g.read('index1', 'i4'), index2=g.read('index2', 'i4'), id1=g.read('id1', 'i4'),
                    id2=g.read('id2', 'i4'), source1=args[0], source2=args[-1] if len(args) > 1 else args[0],
                    param=g.read('interaction_param', 'f4'))


def graph_cutoff(spec):
    """the graph's cutoff as the engine derives it from interaction_param (fp32; interaction_graph.h:383-398 and the functors' own
    cutoffs): the largest over the type pairs"""
    p = spec['param']; it = spec['itype']; n_param = p.shape[2]
    if it in (ROTAMER, HBOND_COVERAGE):
        n_knot, inv_dx = {34: (9, 1.), 40: (12, 1.), 62: (16, 2.), 30: (7, 1.), 54: (12, 2.)}[n_param]      # (knots from the table's width)
        return np.float32((n_knot - 2 - 1e-6) / inv_dx)
    if it in (RADIAL, HBOND_SC_RADIAL):
        return np.float32(max(np.float32((16 - 2 - 1e-6) / float(x)) for x in p[:, :, 0].ravel()))
    if it == ENVIRONMENT:
        return np.float32((p[:, :, 0] + np.float32(1.) / p[:, :, 1]).max())
    return np.sqrt(np.float32(3.5) * np.float32(3.5))


def yardstick_for(spec, outputs, cutoff=None):
    """edges_yardstick of a graph_spec on {node name: output array}"""
    p1 = outputs[spec['source1']][spec['index1'], :3]; p2 = outputs[spec['source2']][spec['index2'], :3]
    return edges_yardstick(p1, p2, spec['id1'], spec['id2'], graph_cutoff(spec) if cutoff is None else cutoff, spec['itype'], spec['symmetric'])
