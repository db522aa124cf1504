"""CPU tests of the device draw of the MBAR bootstrap counts: the numpy yardstick tests/mbar_boot_draw_reference.py (its Threefry
against the oracle's, the properties the definition promises, the block bootstrap's error bar on a correlated series), the block
lengths, and every refusal of upside_hip_mbar_bootstrap_drawn and upside_hip_mbar_bootstrap_counts through the built library (they
return before any device call) with the ValueErrors of the Python layer."""
import ctypes as ct
import os
import numpy as np
import pytest
import parity_util as P
import mbar_boot_draw_reference as D
import mbar_boot_draw_cases as DC

pkg = P.pkg
KNOWN = [([0] * 4, [0] * 4, [0x9c6ca96a, 0xe17eae66, 0xfc10ecd4, 0x5256a7d8]),
         ([0xffffffff] * 4, [0xffffffff] * 4, [0x2a881696, 0x57012287, 0xf6c7446e, 0xa16a6732]),
         ([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], [0xa4093822, 0x299f31d0, 0x082efa98, 0xec4e6c89], [0x59cd1dbb, 0xb8879579, 0x86b5d00c, 0xac8b6d84])]


def test_the_yardsticks_threefry_reproduces_the_known_answers():
    for ctr, key, want in KNOWN:
        assert D.threefry4x32(np.array([ctr], 'u4'), np.array(key, 'u4'))[0].tolist() == want


def test_the_yardsticks_threefry_equals_the_oracles():
    if not os.path.exists(P.ORACLE_LIB):
        pytest.skip('oracle not built')
    c = P.oracle_library().calc
    rs = np.random.RandomState(12)
    ctr = np.concatenate((np.array([k[0] for k in KNOWN], 'u4'), rs.randint(0, 1 << 32, (100, 4), dtype='u8').astype('u4')))
    key = np.concatenate((np.array([k[1] for k in KNOWN], 'u4'), rs.randint(0, 1 << 32, (100, 4), dtype='u8').astype('u4')))
    got = D.threefry4x32(ctr, key)
    for i in range(len(ctr)):
        out = np.zeros(4, 'u4'); a = ctr[i].copy(); k = key[i].copy()
        c.oracle_threefry4x32(out.ctypes.data, a.ctypes.data, k.ctypes.data)
        assert got[i].tolist() == out.tolist(), i


def test_the_high_half_of_the_product():
    rs = np.random.RandomState(4)
    a = np.concatenate((rs.randint(0, 1 << 63, 200, dtype='i8').astype('u8') * np.uint64(2) + np.uint64(1), np.array([0, 2 ** 64 - 1, 2 ** 64 - 1], 'u8')))
    b = np.concatenate((rs.randint(0, 1 << 63, 200, dtype='i8').astype('u8'), np.array([2 ** 64 - 1, 2 ** 64 - 1, 1], 'u8')))
    assert [int(x) for x in D.mulhi64(a, b)] == [(int(p) * int(q)) >> 64 for p, q in zip(a, b)]


def test_the_counts_are_the_blocks_laid_one_by_one():
    """the difference array against a loop over blocks and offsets, and the sums"""
    for m, L in ((1, 1), (257, 1), (257, 7), (4099, 64), (10, 50), (10, 3)):
        got = D.state_counts(DC.SEED, 2, 5, m, L)
        Lc = min(L, m); n_block = -(-m // Lc)
        s = D.block_starts(DC.SEED, 2, 5, m, n_block)
        want = np.zeros(m, 'i8')
        for j in range(n_block):
            for t in range(Lc if j < n_block - 1 else m - Lc * (n_block - 1)):
                want[(int(s[j]) + t) % m] += 1
        assert (0 <= s).all() and (s < m).all()
        assert np.array_equal(got, want) and got.sum() == m, (m, L)


def test_what_the_definition_promises():
    n_k = np.array([0, 1, 2, 255, 300, 41], 'i8')
    block = np.array([3, 1, 2, 7, 1, 41])
    start = np.concatenate(([0], np.cumsum(n_k)))
    c = D.counts(n_k, 9, seed=DC.SEED, block=block)
    for k in range(len(n_k)):      # per state and replicate the counts add up to n_k
        assert (c[:, start[k]:start[k + 1]].sum(axis=1) == n_k[k]).all()
    assert (c[:, start[5]:] == 1).all() and (D.counts(n_k, 2, seed=1, block=10 ** 6) == 1).all()      # L >= m: all ones
    assert np.array_equal(D.counts(n_k, 2, seed=DC.SEED, block=block, first=3), c[3:5])      # unchanged by B and by first
    assert np.array_equal(D.counts(n_k, 1, seed=DC.SEED, block=block, first=8), c[8:9])
    sos = DC.shuffled_origins(n_k)
    order = np.argsort(sos, kind='stable')
    shuffled = D.counts(n_k, 9, seed=DC.SEED, state_of_sample=sos, block=block)
    assert np.array_equal(shuffled[:, order], c) and not np.array_equal(shuffled, c)      # the grouped counts permuted
    assert not np.array_equal(D.counts(n_k, 2, seed=7, block=block), D.counts(n_k, 2, seed=7 + (1 << 32), block=block))      # a 64-bit seed
    assert not np.array_equal(c[0], c[1])
    assert np.array_equal(D.counts(n_k, 2, seed=3), D.counts(n_k, 2, seed=3, block=1))      # no block = blocks of one


def test_block_lengths():
    bl = pkg.mbar.block_lengths
    assert bl([9., 1., 0., 0.5, 2.3, np.nan]).tolist() == [45, 5, 1, 1, 12, 1] and bl(9.).tolist() == [45]
    assert bl([9., 1.2], factor=1).tolist() == [9, 2] and bl([3.], factor=2.5).tolist() == [8]
    assert bl([9.]).dtype == np.int64
    with pytest.raises(ValueError):
        bl([9.], factor=0)


def test_blocks_of_five_g_give_the_error_bar_of_a_correlated_series():
    """AR(1), phi = 0.8, n = 4096: g = (1 + phi) / (1 - phi) = 9 and the standard deviation of the mean is sqrt(var g / n).  Over 200
    replicates of the yardstick's draw, blocks of block_lengths(9) = 45 samples give it within 15 % (the derivation in
    mbar.block_lengths: 5 % low, and 5 % sampling noise of 200 replicates), the plain bootstrap (L = 1) less than half of it"""
    phi, n = 0.8, 4096
    x = DC.ar1(n, phi, np.random.default_rng(2))
    g = 9.      # (1 + phi) / (1 - phi), which floating point puts an ulp above 9
    L = int(pkg.mbar.block_lengths(g)[0])
    want = np.sqrt(x.var() * g / n)
    sd = dict((l, float((D.counts([n], 200, seed=7, block=l).astype('f8') @ x / n).std(ddof=1))) for l in (L, 1))
    print('sqrt(var g / n) = %.4f; bootstrap sd of the mean: %.4f at L = %d (ratio %.3f), %.4f at L = 1 (ratio %.3f)' %
          (want, sd[L], L, sd[L] / want, sd[1], sd[1] / want))
    assert L == 45
    assert abs(sd[L] / want - 1.) <= 0.15
    assert sd[1] < 0.5 * want


def need_library():
    if not os.path.exists(pkg.PRODUCT_LIB):
        pytest.fail('libupside_hip.so not built (run __graft_entry__.build())')
    return pkg.default_library().calc


def test_the_drawn_entry_point_states_its_refusals():
    calc = need_library()
    good, cases = DC.drawn_refusal_cases()
    for label, change, fragment in cases:
        with pytest.raises(RuntimeError) as err:
            pkg.mbar.bootstrap(**dict(good, **change))
        assert fragment in str(err.value), (label, str(err.value))
        assert 'mbar_bootstrap_drawn: ' in str(err.value), (label, str(err.value))
    for label, override, fragment in DC.RAW_DRAWN_REFUSALS:
        rc, msg = DC.raw_drawn(calc, good, **override)
        assert rc == 1 and fragment in msg and msg.startswith('mbar_bootstrap_drawn: '), (label, msg)
    # the host side without a problem or without a draw
    pkg.mbar._bind(calc)
    p = pkg.mbar._BootProblem(); dr = pkg.mbar._BootDraw()
    buf = ct.create_string_buffer(256)
    assert calc.upk_mbar_boot_solve_drawn(None, ct.byref(dr), buf, 256) == 1 and b'no problem or no draw' in buf.value
    assert calc.upk_mbar_boot_solve_drawn(ct.byref(p), None, buf, 256) == 1 and b'no problem or no draw' in buf.value


def test_the_counts_entry_point_states_its_refusals():
    calc = need_library()
    for label, change, fragment in DC.COUNTS_REFUSALS:
        with pytest.raises(RuntimeError) as err:
            pkg.mbar.bootstrap_counts_device(**dict(DC.COUNTS_GOOD, **change))
        assert fragment in str(err.value), (label, str(err.value))
        assert 'mbar_bootstrap_counts: ' in str(err.value), (label, str(err.value))
    for label, override, fragment in DC.RAW_COUNTS_REFUSALS:
        rc, msg = DC.raw_counts(calc, **override)
        assert rc == 1 and fragment in msg and msg.startswith('mbar_bootstrap_counts: '), (label, msg)


def test_what_python_refuses_before_the_library_is_asked():
    need_library()
    good, _ = DC.drawn_refusal_cases()
    host = dict(good, draw='host', counts=np.ones((2, 30), 'u2'))
    for kw in (dict(host, block=3), dict(good, counts=np.ones((2, 30), 'u2')), dict(good, draw='gpu'), dict(good, seed=-1), dict(good, seed=1 << 64),
               dict(good, block=np.ones(2, 'i8')), dict(good, block=1.5), dict(good, f=np.zeros(2)), dict(good, state_of_sample=np.zeros(7, 'i4'))):
        with pytest.raises(ValueError):
            pkg.mbar.bootstrap(**kw)
    for kw in (dict(seed=-1), dict(block=np.ones(3, 'i8')), dict(block=2.5), dict(state_of_sample=np.zeros(5, 'i4'))):
        with pytest.raises(ValueError):
            pkg.mbar.bootstrap_counts_device(**dict(DC.COUNTS_GOOD, **kw))
    import inspect
    sig = inspect.signature(pkg.engine.Ensemble.umbrella_mbar).parameters
    assert sig['bootstrap_draw'].default == 'host' and sig['bootstrap_block'].default is None and sig['bootstrap_block_factor'].default == 5
    sig = inspect.signature(pkg.mbar.profile_bootstrap).parameters
    assert sig['draw'].default == 'host' and sig['block'].default is None
