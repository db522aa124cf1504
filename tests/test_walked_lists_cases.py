"""CPU pins of tests/walked_lists.py, the checker of the lists the pair passes walk (tests/test_gpu_walked_lists.py runs it on the
device's records): it passes a correct hand-made record of every list form and raises, naming the row, on one seeded fault each; and
its all-pairs yardstick equals the oracle's pair lists exactly on every fixture."""
import copy
import numpy as np
import pytest
import parity_util as P
import walked_lists as WL

FIXTURES = ['trpcage20_7A', 'proteinG56_7A', 'syn150_10A', 'syn300_10A', 'syn300_7A']


def make_record(kind, seed=0):
    """a correct record built by the definition.  kind: 'asym1' / 'asym2' (environment ids, 16-bit words, sides 1 and 2 of one graph),
    'upper' (rotamer: partners above the row, slot fields), 'full' (symmetric full list with hlo and ordu)"""
    rng = np.random.RandomState(seed)
    sym = kind in ('upper', 'full')
    n1 = 14; n2 = n1 if sym else 11
    pos1 = (rng.rand(n1, 3) * 6.).astype('f4'); pos2 = pos1 if sym else (rng.rand(n2, 3) * 6.).astype('f4')
    cache1 = pos1 + (rng.rand(n1, 3) * 0.2).astype('f4'); cache2 = cache1 if sym else pos2 + (rng.rand(n2, 3) * 0.2).astype('f4')
    if kind == 'upper':
        id1 = ((np.arange(n1) // 2) << 4 | 3).astype('i4'); itype = WL.ROTAMER      # two beads per node
    else:
        id1 = (np.arange(n1) * 2).astype('i4'); itype = WL.RADIAL if sym else WL.ENVIRONMENT
    id2 = id1 if sym else (np.arange(n2) * 3 + 1).astype('i4')
    cutoff, cache_cutoff = np.float32(3.), np.float32(4.5)
    side = 2 if kind == 'asym2' else 1
    hits = WL.in_range_matrix(pos1, pos2, id1, id2, cutoff, itype, sym)
    cached = WL.in_range_matrix(cache1, cache2, id1, id2, cache_cutoff, itype, sym)
    cached |= hits      # (a stale but valid cache: every in-range pair is cached)
    edges = WL.edges_yardstick(pos1, pos2, id1, id2, cutoff, itype, sym)
    if kind == 'upper':
        hits = np.triu(hits, 1); cached = np.triu(cached, 1)
    if side == 2:
        hits, cached = hits.T, cached.T
    rows_pos, other_pos, rows_cache, other_cache, rows_id, other_id = (
        (pos1, pos2, cache1, cache2, id1, id2) if side == 1 else (pos2, pos1, cache2, cache1, id2, id1))
    n_rows, n_other = hits.shape
    cap = n_other + 2
    bits = 13 if kind == 'upper' else 0
    slot_of = {}
    rec = dict(node='hand_' + kind, system=0, side=side, n_rows=n_rows, n_other=n_other, cap=cap, symmetric=sym, md_sides=3, itype=itype,
               word_bits=32 if bits else 16, nbr_j_bits=bits, n_slot=-1, upper=kind == 'upper', n_refine=1, slot_none=0x7FFFF, rebuilt=1,
               cutoff=cutoff, cache_cutoff=cache_cutoff, source_rows='a' if side == 1 else 'b', source_other='a' if (sym or side == 2) else 'b')
    for name, m in (('nbr', cached), ('hit', hits)):
        words = np.zeros((n_rows, cap), 'i4'); n = np.zeros(n_rows, 'i4')
        for r in range(n_rows):
            js = np.flatnonzero(m[r]); n[r] = len(js)
            for k, j in enumerate(js):
                w = int(j)
                if bits:
                    key = (min(rows_id[r] >> 4, other_id[j] >> 4), max(rows_id[r] >> 4, other_id[j] >> 4))
                    w |= slot_of.setdefault(key, len(slot_of)) << bits
                words[r, k] = w
        rec[name + '_word'] = words
        rec[name] = words & ((1 << bits) - 1) if bits else words.copy()
        rec[name + '_slot'] = (words >> bits) if bits else None
        rec['cnt' if name == 'nbr' else 'hcnt'] = n
    rec['n_slot'] = len(slot_of) if bits else -1
    rec['hlo'] = ((rec['hit'] < np.arange(n_rows)[:, None]) & (np.arange(cap)[None, :] < rec['hcnt'][:, None])).sum(1).astype('i4') if kind == 'full' else None
    rec['ord'] = np.argsort(-rec['hcnt'], kind='stable').astype('i4')
    rec['ordu'] = np.argsort(-(rec['hcnt'] - rec['hlo']), kind='stable').astype('i4') if kind == 'full' else None
    perm = rng.permutation(n_rows).astype('i4') if kind == 'upper' else np.arange(n_rows, dtype='i4')      # renumbered beads
    rec.update(id_rows=rows_id, id_other=other_id, orig_rows=perm, orig_other=perm if sym else np.arange(n_other, dtype='i4'),
               loc_rows=np.arange(n_rows, dtype='i4'), loc_other=np.arange(n_other, dtype='i4'),
               cur_rows=rows_pos.copy(), cur_other=other_pos.copy(), cache_rows=rows_cache.copy(), cache_other=other_cache.copy(),
               cache_id_rows=rows_id.copy(), cache_id_other=other_id.copy(), src_rows=rows_pos.copy(), src_other=other_pos.copy())
    if kind == 'upper':      # the reference in the caller's numbering
        e = perm[edges]; edges = WL.canonical_sort(np.column_stack((e.min(1), e.max(1))))
    return rec, edges


KINDS = ['asym1', 'asym2', 'upper', 'full']


@pytest.mark.parametrize('kind', KINDS)
def test_a_correct_record_passes(kind):
    rec, edges = make_record(kind)
    t = WL.check_graph(rec, edges, first_pass=True, source_out={'a': rec['src_rows'] if rec['side'] == 1 else rec['src_other'],
                                                                'b': rec['src_other'] if rec['side'] == 1 else rec['src_rows']})
    assert t['n_edge'] == len(edges) > 10 and t['n_cached'] > t['n_walked']
    assert (rec['hcnt'] >= 2).sum() >= 3 and (rec['cnt'] > rec['hcnt']).any()


def a_row(rec, need_hits=2, spare_cached=False):
    ok = rec['hcnt'] >= need_hits
    if spare_cached:
        ok &= rec['cnt'] > rec['hcnt']
    return int(np.flatnonzero(ok)[0])


def fault_missing_pair(rec):
    r = a_row(rec); rec['hcnt'][r] -= 1
    if rec['hlo'] is not None and rec['hit'][r, rec['hcnt'][r]] < r:
        rec['hlo'][r] -= 1
    return r


def fault_duplicated_pair(rec):
    r = a_row(rec); n = rec['hcnt'][r]
    for k in ('hit', 'hit_word'):
        rec[k][r, n] = rec[k][r, n - 1]
    if rec['hit_slot'] is not None:
        rec['hit_slot'][r, n] = rec['hit_slot'][r, n - 1]
    rec['hcnt'][r] += 1
    return r


def fault_swapped_order(rec):
    r = a_row(rec)
    for k in ('hit', 'hit_word') + (('hit_slot',) if rec['hit_slot'] is not None else ()):
        rec[k][r, [0, 1]] = rec[k][r, [1, 0]]
    return r


def fault_hlo_off_by_one(rec):
    r = a_row(rec); rec['hlo'][r] += 1
    return r


def fault_ord_repeats_a_row(rec):
    rec['ord'][3] = rec['ord'][2]
    return None      # (names the row that appears twice or never)


def fault_slot_shared(rec):
    # give one cached word the slot of a word of another node pair
    r = a_row(rec, spare_cached=True)
    slots = rec['nbr_slot'][r, :rec['cnt'][r]]
    k = int(np.flatnonzero(slots != slots[0])[0])
    w = (rec['nbr_word'][r, k] & 0x1FFF) | (int(slots[0]) << 13)
    in_hit = np.flatnonzero(rec['hit'][r, :rec['hcnt'][r]] == rec['nbr'][r, k])
    rec['nbr_word'][r, k] = w; rec['nbr_slot'][r, k] = slots[0]
    for h in in_hit:
        rec['hit_word'][r, h] = w; rec['hit_slot'][r, h] = slots[0]
    return None      # (names a row that carries the clashing slot)


def fault_cur_pos_one_ulp(rec):
    r = 5
    rec['cur_rows'][r, 1] = np.nextafter(rec['cur_rows'][r, 1], np.float32(np.inf))
    return r


def fault_cached_row_lacks_a_pair(rec):
    r = a_row(rec, 0, spare_cached=True)
    hit = set(rec['hit'][r, :rec['hcnt'][r]].tolist())
    k = [k for k in range(rec['cnt'][r]) if rec['nbr'][r, k] not in hit and
         WL.dist2_f32(rec['cache_rows'][r:r + 1], rec['cache_other'][rec['nbr'][r, k]][None])[0, 0] < rec['cache_cutoff'] ** 2][0]
    for key in ('nbr', 'nbr_word') + (('nbr_slot',) if rec['nbr_slot'] is not None else ()):
        rec[key][r, k:-1] = rec[key][r, k + 1:].copy()
    rec['cnt'][r] -= 1
    return r


FAULTS = [(fault_missing_pair, KINDS), (fault_duplicated_pair, KINDS), (fault_swapped_order, KINDS), (fault_hlo_off_by_one, ['full']),
          (fault_ord_repeats_a_row, KINDS), (fault_slot_shared, ['upper']), (fault_cur_pos_one_ulp, KINDS),
          (fault_cached_row_lacks_a_pair, KINDS)]


@pytest.mark.parametrize('fault,kind', [(f, k) for f, ks in FAULTS for k in ks], ids=lambda v: getattr(v, '__name__', v))
def test_every_seeded_fault_raises_and_names_its_row(fault, kind):
    rec, edges = make_record(kind)
    rec = copy.deepcopy(rec)
    row = fault(rec)
    with pytest.raises(WL.WalkedListError) as err:
        WL.check_graph(rec, edges, first_pass=False)      # (the sorted order has a test of its own below)
    msg = str(err.value)
    assert 'node hand_%s system 0 side %d' % (kind, rec['side']) in msg, msg
    assert ' row ' in msg, msg
    if row is not None:
        assert ' row %d:' % row in msg, (row, msg)


def test_a_first_pass_order_must_be_sorted_later_ones_only_a_permutation():
    rec, edges = make_record('asym1')
    o = rec['ord']; k = rec['hcnt'][o]
    i = int(np.flatnonzero(k[1:] < k[:-1])[0])
    o[[i, i + 1]] = o[[i + 1, i]]
    WL.check_graph(rec, edges, first_pass=False)
    with pytest.raises(WL.WalkedListError, match='not sorted by descending count'):
        WL.check_graph(rec, edges, first_pass=True)


def backbone_record(seed=1):
    rng = np.random.RandomState(seed)
    n = 20; cap = 12
    ref = (rng.rand(n, 3) * 12.).astype('f4'); centres = ref + (rng.rand(n, 3) * 0.3).astype('f4')
    ids = np.arange(n, dtype='i4'); cutoff, skin = np.float32(5.), np.float32(1.5)
    far = cutoff + skin
    near = (np.abs(ids[:, None] - ids[None, :]) > 1) & (WL.dist2_f32(ref, ref) < far * far)
    lst = np.zeros((n, cap), 'i4'); cnt = near.sum(1).astype('i4')
    for r in range(n):
        lst[r, :cnt[r]] = np.flatnonzero(near[r])
    return dict(node='backbone_pairs', system=0, side=0, n_residue=n, cap=cap, skin=skin, dist_cutoff=cutoff, cnt=cnt, id=ids, list=lst,
                ref=ref, centre=centres), centres


def test_backbone_checker_on_hand_made_lists():
    rec, centres = backbone_record()
    t = WL.check_backbone(rec, centres)
    assert t['n_near'] > 10 and t['n_listed'] > t['n_near']
    near_now = WL.dist2_f32(centres, centres) < rec['dist_cutoff'] ** 2
    r = int(np.flatnonzero(rec['cnt'] >= 2)[0])
    k = [k for k in range(rec['cnt'][r]) if near_now[r, rec['list'][r, k]]][0]
    bad = copy.deepcopy(rec); bad['list'][r, k:-1] = bad['list'][r, k + 1:].copy(); bad['cnt'][r] -= 1
    with pytest.raises(WL.WalkedListError, match=' row %d: row lacks residue' % r):
        WL.check_backbone(bad, centres)
    bad = copy.deepcopy(rec); bad['list'][r, [0, 1]] = bad['list'][r, [1, 0]]
    with pytest.raises(WL.WalkedListError, match=' row %d: row is not strictly ascending' % r):
        WL.check_backbone(bad, centres)
    bad = copy.deepcopy(rec)
    out = [j for j in range(rec['n_residue']) if j > bad['list'][r, bad['cnt'][r] - 1]
           and WL.dist2_f32(rec['ref'][r:r + 1], rec['ref'][j:j + 1])[0, 0] > (rec['dist_cutoff'] + rec['skin']) ** 2][0]
    bad['list'][r, bad['cnt'][r]] = out; bad['cnt'][r] += 1
    with pytest.raises(WL.WalkedListError, match=' row %d: row lists residue %d' % (r, out)):
        WL.check_backbone(bad, centres)
    bad = copy.deepcopy(rec); bad['cnt'][r] = rec['cap'] + 1
    with pytest.raises(WL.WalkedListError, match=' row %d: cnt' % r):
        WL.check_backbone(bad, centres)


def test_cnt_classes():
    t = WL.cnt_classes([0, 1, 63, 64, 65, 128, 129, 191, 192])
    assert t == {'0': 1, '1..63': 2, '65..128': 2, '>128': 3, '%64==0': 3, '%64==1': 3, '%64==63': 2}


def oracle_outputs(orc, pos, names):
    orc.deriv(pos)
    return {nm: orc.get_output(nm) for nm in names}


@pytest.mark.parametrize('name', FIXTURES)
def test_yardstick_equals_the_oracle_pair_lists(name):
    """the five oracle-listed graphs at pos and pos2: edges_yardstick on the oracle's own source-node outputs is P.oracle_pairlist,
    pair for pair"""
    g = P.golden(name)
    orc = P.pkg.Upside(P.fixture(name), library=P.oracle_library())
    specs = {node: WL.graph_spec(P.pkg.h5lite, P.fixture(name), node) for node in WL.ORACLE_GRAPHS}
    sources = sorted({s[k] for s in specs.values() for k in ('source1', 'source2')})
    for tag in ('pos', 'pos2'):
        out = oracle_outputs(orc, g[tag], sources)
        for node in WL.ORACLE_GRAPHS:
            ref = P.canonical_sort(P.oracle_pairlist(orc, node))
            got = WL.yardstick_for(specs[node], out)
            print('%s %s %s: %d edges (oracle %d)' % (name, tag, node, len(got), len(ref)))
            assert len(ref) > 0 and got.shape == ref.shape and np.array_equal(got, ref), (name, tag, node, got.shape, ref.shape)
    orc.close()


def test_yardstick_on_the_radial_graphs():
    """radial / hbond_sc_radial (proteinG56_restraints): no oracle list exists, the yardstick is the only reference; its edge sets are
    not empty where the oracle's node potentials are not zero"""
    name = 'proteinG56_restraints'
    g = P.golden(name)
    orc = P.pkg.Upside(P.fixture(name), library=P.oracle_library())
    specs = {node: WL.graph_spec(P.pkg.h5lite, P.fixture(name), node) for node in WL.RADIAL_GRAPHS}
    sources = sorted({s[k] for s in specs.values() for k in ('source1', 'source2')})
    out = oracle_outputs(orc, g['pos'], sources)
    for node in WL.RADIAL_GRAPHS:
        e = WL.yardstick_for(specs[node], out)
        pot = float(orc.get_output(node)[0, 0])
        print('%s: %d edges, potential %.6g' % (node, len(e), pot))
        assert len(e) > 0 and pot != 0.
        sup = WL.yardstick_for(specs[node], out, cutoff=WL.graph_cutoff(specs[node]) + np.float32(1.5))
        assert {tuple(x) for x in e} <= {tuple(x) for x in sup} and len(sup) > len(e)
    orc.close()
