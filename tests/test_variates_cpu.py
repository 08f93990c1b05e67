"""The generator of m3pc_draw_variates restated in numpy / float64 (tests/variates_ref.py), without a GPU: Philox4x32-10 known
answers (the Random123 vectors), the moments of the normals and the exponentials it is turned into, and a seeded bug."""
import numpy as np

import variates_ref as V

KAT = [
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), "d16cfe09 94fdcceb 5001e420 24126ea1"),
]


def test_philox_known_answers():
    for counter, key, want in KAT:
        got = " ".join(f"{int(w):08x}" for w in V.philox4x32_10(counter, key))
        assert got == want, (counter, key, got)


def test_moments_of_80000_draws():
    n = 80000
    z = V.eps(1234, 7, n // 32, 32).reshape(-1)
    q = V.expo(1234, 7, n)
    assert z.size == q.size == n
    mz, vz, mq = abs(z.mean()), abs(z.var() - 1.0), abs(q.mean() - 1.0)
    print(f"|mean z| {mz:.4f} |var z - 1| {vz:.4f} |mean q - 1| {mq:.4f} min q {q.min():.3g} max |z| {np.abs(z).max():.3f}")
    assert mz <= 5.0 / np.sqrt(n)
    assert vz <= 5.0 * np.sqrt(2.0 / n)
    assert mq <= 5.0 / np.sqrt(n)
    assert q.min() > 0.0
    assert np.abs(z).max() <= 6.7  # (u1 >= 2^-24: the radius is at most sqrt(48 ln 2) = 5.77)


def test_layout_and_slices():
    """Block b gives the flat elements 4b .. 4b+3 whatever the row length: a (5, 7) array is the first 35 elements of the flat
    stream, and step / seed / array move every block."""
    flat = V.eps(9, 3, 1, 36).reshape(-1)
    assert np.array_equal(V.eps(9, 3, 5, 7).reshape(-1), flat[:35])
    assert np.array_equal(V.expo(9, 3, 5), V.expo(9, 3, 8)[:5])
    assert not np.any(V.eps(9, 4, 1, 36) == flat) and not np.any(V.eps(10, 3, 1, 36) == flat)
    assert not np.any(V.eps(9 + (1 << 32), 3, 1, 36) == flat) and not np.any(V.eps(9, 3 + (1 << 32), 1, 36) == flat)


def test_exponential_is_never_zero():
    """u = 1 (the word's top 24 bits all set) gives -ln u = 0: the value is 2^-25 there."""
    u = ((np.array([0xFFFFFFFF, 0xFFFFFF00, 0xFFFFFE00], dtype=np.uint32) >> np.uint32(8)).astype(np.float64) + 1.0) * 2.0 ** -24
    assert u[0] == u[1] == 1.0 and u[2] < 1.0
    q = -np.log(u)
    q[q <= 0.0] = 2.0 ** -25
    assert q[0] == q[1] == 2.0 ** -25 and 0.0 < q[2] < 1e-7


def test_seeded_bug_swapped_counter_words_moves_values():
    good = V.eps(1234, 7, 16, 8).reshape(-1)
    bad = V.eps(1234, 7, 16, 8, swap_counter_words=True).reshape(-1)
    same = good == bad
    assert same[28:32].all() and not same[:28].any() and not same[32:].any()  # (block 7 of step 7: the swap is the identity there)
    assert (V.expo(1234, 7, 64) == V.expo(1234, 7, 64, swap_counter_words=True)).sum() == 4
    # and the known answers notice it
    counter, key, want = KAT[2]
    assert " ".join(f"{int(w):08x}" for w in V.philox4x32_10(counter, key, swap_counter_words=True)) != want
