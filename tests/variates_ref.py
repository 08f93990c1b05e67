"""numpy / float64 restatement of m3pc_draw_variates (include/m3pc_hip.h): Philox4x32-10 with key = (seed lo, seed hi) and
counter = (block, step lo, step hi, array); block b gives the flat elements 4b .. 4b+3 of array 0 (eps, Box-Muller normals) or
array 1 (expo, Exp(1), never 0).  Shared by tests/test_variates_cpu.py and tests/test_variates_gpu.py."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF


def philox4x32_10(counter, key, swap_counter_words=False):
    """counter: four uint32 arrays (or ints) of one shape, key: two uint32 -> four uint32 arrays.  swap_counter_words: the seeded
    bug of the CPU test (counter words 0 and 1 exchanged)."""
    c = [np.asarray(x, dtype=np.uint64) & MASK for x in counter]
    c = list(np.broadcast_arrays(*c))
    if swap_counter_words:
        c[0], c[1] = c[1], c[0]
    k0, k1 = int(key[0]) & MASK, int(key[1]) & MASK
    for _ in range(10):
        p0 = c[0] * np.uint64(M0)  # (32 x 32 bits: fits 64)
        p1 = c[2] * np.uint64(M1)
        hi0, lo0 = p0 >> np.uint64(32), p0 & np.uint64(MASK)
        hi1, lo1 = p1 >> np.uint64(32), p1 & np.uint64(MASK)
        c = [hi1 ^ c[1] ^ np.uint64(k0), lo1, hi0 ^ c[3] ^ np.uint64(k1), lo0]
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return [x.astype(np.uint32) for x in c]


def _words(seed, step, array, n_blocks, **kw):
    b = np.arange(n_blocks, dtype=np.uint64)
    key = (seed & MASK, (seed >> 32) & MASK)
    return philox4x32_10((b, step & MASK, (step >> 32) & MASK, array), key, **kw)


def eps(seed, step, n_total, row_elems, **kw):
    """(n_total, row_elems) float64 standard normals of (seed, step)."""
    n = n_total * row_elems
    w = _words(seed, step, 0, (n + 3) // 4, **kw)

    def bm(wa, wb):
        u1 = ((wa >> np.uint32(8)).astype(np.float64) + 1.0) * 2.0 ** -24
        u2 = (wb >> np.uint32(8)).astype(np.float64) * 2.0 ** -24
        r = np.sqrt(-2.0 * np.log(u1))
        return r * np.cos(2.0 * np.pi * u2), r * np.sin(2.0 * np.pi * u2)

    z0, z1 = bm(w[0], w[1])
    z2, z3 = bm(w[2], w[3])
    return np.stack([z0, z1, z2, z3], axis=1).reshape(-1)[:n].reshape(n_total, row_elems)


def expo(seed, step, n_total, **kw):
    """(n_total,) float64 Exp(1) of (seed, step); 2^-25 where -ln u is 0."""
    w = _words(seed, step, 1, (n_total + 3) // 4, **kw)
    u = ((np.stack(w, axis=1).reshape(-1) >> np.uint32(8)).astype(np.float64) + 1.0) * 2.0 ** -24
    q = -np.log(u)
    q[q <= 0.0] = 2.0 ** -25
    return q[:n_total]
