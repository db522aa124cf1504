"""The yardstick of the device draw of the MBAR bootstrap counts (upside_hip_mbar_bootstrap_counts, upside_hip_mbar_bootstrap_drawn;
k_mbar_boot_draw* of csrc/kernels_mbar_boot.hip): the definition of include/upside_engine_c.h restated in vectorised numpy, pinned by
tests/test_mbar_boot_draw_config.py.  Integers only, so "equal" is equality.

For replicate b and state k with m = n_k[k] > 0 samples and L = min(max(block[k], 1), m): n_block = ceil(m / L) blocks, block j of
length L (the last one m - L (n_block - 1)) starting at s_j = floor(r_j m / 2^64), r_j from Threefry4x32-20 with counter
(q lo32, q hi32, k, b), q = j >> 1, key (seed lo32, seed hi32, 0x4d424152, 0): X[0] | X[1] << 32 for even j, X[2] | X[3] << 32 for
odd j.  Block j covers the positions (s_j + t) mod m of the state's samples in their order of appearance; a sample's count is the
number of blocks that cover it."""
import numpy as np

KEY2 = 0x4d424152
_ROT = ((10, 26), (11, 21), (13, 27), (23, 5), (6, 20), (17, 11), (25, 10), (18, 20))
_M32 = np.uint64(0xffffffff)


def _rotl(x, n):
    return (x << np.uint32(n)) | (x >> np.uint32(32 - n))


def threefry4x32(counter, key):
    """Threefry4x32-20 on (..., 4) uint32 counters and keys (broadcast against each other): (..., 4) uint32"""
    c = np.asarray(counter, 'u4'); k = np.asarray(key, 'u4')
    c, k = np.broadcast_arrays(c, k)
    ks = [k[..., i].copy() for i in range(4)]
    ks.append(np.uint32(0x1BD11BDA) ^ ks[0] ^ ks[1] ^ ks[2] ^ ks[3])
    X = [c[..., i] + ks[i] for i in range(4)]
    for r in range(20):
        a, b = _ROT[r % 8]
        if r % 2 == 0:
            X[0] = X[0] + X[1]; X[1] = _rotl(X[1], a) ^ X[0]
            X[2] = X[2] + X[3]; X[3] = _rotl(X[3], b) ^ X[2]
        else:
            X[0] = X[0] + X[3]; X[3] = _rotl(X[3], a) ^ X[0]
            X[2] = X[2] + X[1]; X[1] = _rotl(X[1], b) ^ X[2]
        if r % 4 == 3:
            s = r // 4 + 1
            for i in range(4):
                X[i] = X[i] + ks[(s + i) % 5]
            X[3] = X[3] + np.uint32(s)
    return np.stack(X, axis=-1)


def mulhi64(a, b):
    """the high 64 bits of the 128-bit product of uint64 arrays, from 32-bit halves"""
    a = np.asarray(a, 'u8'); b = np.asarray(b, 'u8')
    a0, a1, b0, b1 = a & _M32, a >> np.uint64(32), b & _M32, b >> np.uint64(32)
    p00, p01, p10, p11 = a0 * b0, a0 * b1, a1 * b0, a1 * b1
    carry = ((p00 >> np.uint64(32)) + (p01 & _M32) + (p10 & _M32)) >> np.uint64(32)
    return p11 + (p01 >> np.uint64(32)) + (p10 >> np.uint64(32)) + carry


def block_starts(seed, b, k, m, n_block):
    """(n_block,) int64: s_j of replicate b, state k with m samples"""
    seed = int(seed)
    j = np.arange(n_block, dtype='u8')
    q = j >> np.uint64(1)
    ctr = np.stack([(q & _M32).astype('u4'), (q >> np.uint64(32)).astype('u4'), np.full(n_block, k, 'u4'), np.full(n_block, b, 'u4')], axis=-1)
    key = np.array([seed & 0xffffffff, seed >> 32, KEY2, 0], 'u4')
    X = threefry4x32(ctr, key).astype('u8')
    odd = (j & np.uint64(1)).astype(bool)
    r = np.where(odd, X[:, 2] | (X[:, 3] << np.uint64(32)), X[:, 0] | (X[:, 1] << np.uint64(32)))
    return mulhi64(r, np.uint64(m)).astype('i8')


def state_counts(seed, b, k, m, L):
    """(m,) int64: the counts of state k in replicate b, by a difference array over the blocks' one or two linear intervals"""
    L = min(max(int(L), 1), m)
    n_block = -(-m // L)
    s = block_starts(seed, b, k, m, n_block)
    length = np.full(n_block, L, 'i8'); length[-1] = m - L * (n_block - 1)
    end = s + length                      # exclusive, up to 2 m - 1
    diff = np.zeros(m + 1, 'i8')
    np.add.at(diff, s, 1)
    np.add.at(diff, np.minimum(end, m), -1)
    wrap = end > m                        # the part past the end covers 0 .. end - m - 1
    np.add.at(diff, np.zeros(int(wrap.sum()), 'i8'), 1)
    np.add.at(diff, end[wrap] - m, -1)
    return np.cumsum(diff[:m])


def counts(n_k, n_bootstrap, seed=0, state_of_sample=None, block=None, first=0):
    """(B, N) uint16: replicates first .. first + B - 1.  block: None, an int or (K,); state_of_sample: None = grouped by state"""
    n_k = np.asarray(n_k, 'i8').reshape(-1)
    K, N, B = len(n_k), int(n_k.sum()), int(n_bootstrap)
    blk = np.ones(K, 'i8') if block is None else np.broadcast_to(np.asarray(block, 'i8'), (K,))
    start = np.concatenate(([0], np.cumsum(n_k)))
    order = np.arange(N) if state_of_sample is None else np.argsort(np.asarray(state_of_sample), kind='stable')
    out = np.zeros((B, N), 'i8')
    for i in range(B):
        for k in range(K):
            if n_k[k]:
                out[i, order[start[k]:start[k + 1]]] = state_counts(seed, first + i, k, int(n_k[k]), int(blk[k]))
    assert out.max() <= 65535
    return out.astype('u2')
