"""CPU checks of tests/step_ref.py, the references that tests/test_gpu_step_kernels.py holds the per-step
kernels to: the Philox4x32-10 generator against the published Random123 known-answer vectors, the range of
the uniforms, and the statistics of the reference normal stream."""
import math

import numpy as np

import step_ref as sr

# Random123 kat_vectors, philox4x32 with 10 rounds: counter, key, output
KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
     (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
]


def test_philox_known_answers():
    for ctr, key, out in KAT:
        got = tuple(int(w[0]) for w in sr.philox4x32(ctr, key))
        assert got == out, (ctr, key, [hex(v) for v in got])
    # vectorised over counters and keys alike: the three vectors in one call
    got = sr.philox4x32([np.array([k[0][i] for k in KAT]) for i in range(4)],
                        [np.array([k[1][i] for k in KAT]) for i in range(2)])
    assert [tuple(int(w[j]) for w in got) for j in range(3)] == [k[2] for k in KAT]


def test_draw_words_layout():
    """counter words {ctr_lo, ctr_hi, 0x5eed, 0}, key {seed_lo, seed_hi}: every 32-bit half reaches the
    generator, and a negative seed is read as its 64-bit pattern."""
    seed, ctr = 0x9E3779B97F4A7C15, (3 << 32) | 7
    w = sr.draw_words(seed, np.array([ctr], dtype=np.uint64))
    ref = sr.philox4x32((7, 3, 0x5EED, 0), (0x7F4A7C15, 0x9E3779B9))
    assert [int(a[0]) for a in w] == [int(a[0]) for a in ref]
    base = [int(a[0]) for a in sr.draw_words(seed & 0xFFFFFFFF, [7])]
    assert [int(a[0]) for a in sr.draw_words(seed, [7])] != base
    assert [int(a[0]) for a in sr.draw_words(seed & 0xFFFFFFFF, [ctr])] != base
    assert [int(a[0]) for a in sr.draw_words(-1, [5])] == [int(a[0]) for a in sr.draw_words(2 ** 64 - 1, [5])]
    c = sr.counters(2 ** 64 - 2, 4)
    assert [int(v) for v in c] == [2 ** 64 - 2, 2 ** 64 - 1, 0, 1]
    c = sr.counters(2 ** 32 - 2, 4)
    assert [int(v) >> 32 for v in c] == [0, 0, 1, 1]


def test_u01_range_over_all_mantissas():
    """u = ((v >> 8) + 0.5) 2^-24 in float32 over all 2^24 values of v >> 8: [2^-25, 1], 1.0 reached (the sum
    rounds to 2^24 at the top) and 0 never, so log(u) is finite and <= 0."""
    v = np.arange(1 << 24, dtype=np.uint32) << np.uint32(8)
    u = sr.u01(v)
    assert u.dtype == np.float32
    assert float(u.min()) == 2.0 ** -25 and float(u.max()) == 1.0
    assert float(u[0]) == 2.0 ** -25 and float(u[-1]) == 1.0
    assert np.all(np.diff(u.astype(np.float64)) >= 0)
    # the low 8 bits of v never matter
    assert np.array_equal(sr.u01(v[::4097] | np.uint32(0xFF)), u[::4097])


def test_normals_finite_at_corner_words():
    for w0 in (0, 0xFFFFFFFF):
        for w1 in (0, 0xFFFFFFFF):
            z = sr.normal_from_words(np.array([w0], np.uint32), np.array([w1], np.uint32))[0]
            assert math.isfinite(z.real) and math.isfinite(z.imag), (w0, w1, z)
            # the largest radius any draw can have: sqrt(-2 log 2^-25) * sqrt(1/2) = 4.16 per part
            assert abs(z) <= math.sqrt(25 * math.log(2.0)) + 1e-12
    z = sr.normal_from_words(np.array([0xFFFFFFFF], np.uint32), np.array([0], np.uint32))[0]
    assert z == 0  # u0 = 1: a zero radius


def test_real_part_takes_cosine_of_word_1():
    """Word 0 gives the radius and word 1 the angle; the real part is the cosine."""
    w0, w1 = np.array([0x12345678], np.uint32), np.array([0x40000000], np.uint32)  # u1 ~ 1/4: angle ~ pi/2
    z = sr.normal_from_words(w0, w1)[0]
    assert abs(z.real) < 1e-6 and z.imag > 0.1
    rad = math.sqrt(-2.0 * math.log(float(sr.u01(w0)[0]))) * math.sqrt(0.5)
    assert abs(abs(z) - rad) < 1e-12


def test_reference_stream_statistics():
    """2e6 counters of one seed: |mean| and |var - 1/2| within 2e-3, |corr(re, im)| and the lag-1
    autocorrelation within 3e-3 (about 4 sigma of 2e6 samples).  Conditions on the reference."""
    z = sr.normals(0x1234, sr.counters(0, 2_000_000))
    mean, var, corr, lag = sr.stream_stats(z)
    print(f"reference stream, 2e6 counters: |mean| {mean:.2e} |var - 1/2| {var:.2e} |corr| {corr:.2e} lag-1 {lag:.2e}")
    assert mean < sr.STAT_BOUND and var < sr.STAT_BOUND
    assert corr < sr.CORR_BOUND and lag < sr.CORR_BOUND


def test_small_draw_meets_the_correlation_bounds():
    """The [2, 256, 64] draw that the GPU test holds to the same 3e-3: at 32768 samples that is half a sigma, so
    its seed is one at which the reference stream meets the bound with room for the kernel's 4e-6 per element
    (chosen from this reference alone)."""
    B, H, W = sr.SMALL_DRAW_SHAPE
    z = sr.batch_normals(sr.SMALL_DRAW_SEED, 0, B, H * W)
    _, _, corr, lag = sr.stream_stats(z)
    print(f"reference [2, 256, 64] draw: |corr| {corr:.2e} lag-1 {lag:.2e}")
    assert corr < 0.9 * sr.CORR_BOUND and lag < 0.9 * sr.CORR_BOUND


def test_counter_ranges():
    a = sr.counter_ranges(0, 2, 200)
    b = sr.counter_ranges(400, 2, 200)
    assert sr.ranges_disjoint([a, b]) and not sr.ranges_disjoint([a, sr.counter_ranges(399, 2, 200)])
    r0 = sr.counter_ranges(0, 3, 200, row_seeds=[5, -7, 5])
    r1 = sr.counter_ranges(1, 3, 200, row_seeds=[5, -7, 5])
    assert sr.ranges_disjoint([r0, r1]) and not sr.ranges_disjoint([r0, r0])
    assert r0[1][0] == 2 ** 64 - 7


def test_step_formulas_on_hand_values():
    """The float64 step references on values worked by hand."""
    pyr = np.array([[[1.0, 2.0, -1.0, 0.5]]])
    w = np.array([[1.0, 0.5, 2.0, -1.0], [0.0, 1.0, 1.0, 4.0]])
    b = np.array([0.25, -0.5])
    x = np.array([[2.0 - 1.0j]])
    sc, m = sr.head(pyr, w, b, [0.5], 0, x)
    # h = pyr / t = (2, 4, -2, 1): dnn = 0.25 + (2 + 2 - 4 - 1) + i (-0.5 + (0 + 4 - 2 + 4))
    assert sc[0, 0] == -(-0.75 + 5.5j) and m[0, 0] == (0.25 + 9) + 1j * (0.5 + 10)
    sc1, m1 = sr.head(pyr, w, b, [0.5], 1, x)
    te = 0.499
    cs, co = 0.25 / (te * te + 0.25), 0.5 * te / math.sqrt(0.5)
    assert abs(sc1[0, 0] - (cs * x[0, 0] + co * (-0.75 + 5.5j))) < 1e-15
    assert abs(m1[0, 0] - (cs * (2 + 1j) + co * (9.25 + 10.5j))) < 1e-14
    xm, xo, mm, mo = sr.update(x, [[2.0, -1.0, 0.5, 3.0]], y=np.array([[1.0 + 1.0j]]), score=np.array([[4.0j]]),
                               z=np.array([[1.0 - 1.0j]]))
    assert xm[0, 0] == 3.0 - 1.0j and xo[0, 0] == 6.0 - 4.0j
    assert mm[0, 0] == 5.0 + 5.0j and mo[0, 0] == 8.0 + 8.0j
    assert sr.ratio(np.array([1.0 + sr.U + 0j]), np.array([1.0 + 0j]), np.array([2.0 + 2.0j])) == 0.5
    assert sr.spec_fwd(np.array([0j, 4.0, -9.0j]))[0] == 0 and abs(sr.spec_fwd(np.array([4.0 + 0j]))[0] - 0.3) < 1e-16
    assert abs(sr.spec_back(sr.spec_fwd(np.array([3.0 - 4.0j])))[0] - (3.0 - 4.0j)) < 1e-14
