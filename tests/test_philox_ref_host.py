"""The Philox4x32-10 model of tests/philox_ref.py on the CPU: the published Random123 known answers, the (state, site, element)
-> (counter, key, word) mapping of the rule, the fp32 threshold table, and that every mutation of the model changes the keep
bits — so the bit-for-bit comparisons of test_dropout_edges_gpu.py would notice each of those bugs in a kernel."""
import numpy as np
import pytest

import philox_ref as R

# Random123 kat_vectors, philox4x32 with 10 rounds: (counter, key) -> output
KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]
SEED, OFFSET, SITE = 0x0123456789abcdef, 0x0000000300000007, 7        # both high words nonzero


@pytest.mark.parametrize("counter,key,want", KAT)
def test_known_answers(counter, key, want):
    got = R.philox4x32(counter, key)
    assert tuple(int(w) for w in got) == want
    assert all(w.dtype == np.uint32 for w in got)


def test_known_answers_vectorised():
    """the three vectors as one call over arrays: the model is elementwise"""
    counter = [np.array([k[0][i] for k in KAT]) for i in range(4)]
    key = [np.array([k[1][i] for k in KAT]) for i in range(2)]
    got = R.philox4x32(counter, key)
    for j, (_, _, want) in enumerate(KAT):
        assert tuple(int(w[j]) for w in got) == want


def test_first_four_elements_are_the_first_vector():
    got = R.draws(0, 0, 0, np.arange(4))
    assert got.dtype == np.uint32 and tuple(int(v) for v in got) == KAT[0][2]


def test_mapping_of_state_site_and_element():
    """draws == raw Philox at counter {idx/4 lo, idx/4 hi, site, offset lo}, key {seed lo, seed hi ^ offset hi}, word idx % 4:
    written out here with plain Python ints, for a seed and an offset with high words and elements past 2^34"""
    idx = [0, 1, 5, 4 * 0xffffffff + 3, (1 << 34) + 2, (1 << 34) + 7, (3 << 40) + 9, (1 << 63) + 6]
    got = R.draws(SEED, OFFSET, SITE, np.array(idx, dtype=np.uint64))
    for i, g in zip(idx, got):
        q = i // 4
        counter = (q & 0xffffffff, q >> 32, SITE, OFFSET & 0xffffffff)
        key = (SEED & 0xffffffff, (SEED >> 32) ^ (OFFSET >> 32))
        assert int(g) == int(R.philox4x32(counter, key)[i % 4]), i
    assert (idx[3] // 4) >> 32 == 0 and (idx[4] // 4) >> 32 == 1               # both sides of the carry into counter word 1
    # int64 and uint64 element arrays, and any shape, give the same draws
    small = np.arange(12, dtype=np.int64).reshape(3, 4)
    assert np.array_equal(R.draws(SEED, OFFSET, SITE, small), R.draws(SEED, OFFSET, SITE, small.astype(np.uint64).ravel()).reshape(3, 4))
    # every part of the state matters
    base = R.draws(SEED, OFFSET, SITE, np.arange(64))
    for other in ((SEED ^ 1, OFFSET, SITE), (SEED ^ (1 << 32), OFFSET, SITE), (SEED, OFFSET ^ 1, SITE), (SEED, OFFSET ^ (1 << 32), SITE),
                  (SEED, OFFSET, SITE + 1)):
        assert not np.array_equal(base, R.draws(*other, np.arange(64)))


def test_threshold_table():
    table = {0.1: 429496736, 0.25: 1 << 30, 0.5: 1 << 31, 2.0 ** -24: 256, 1 - 2.0 ** -24: 4294967040, 0.0: 0}
    for p, want in table.items():
        t = R.threshold(p)
        assert t.dtype == np.uint32 and int(t) == want, (p, int(t))
    assert int(R.threshold(np.nextafter(np.float32(1), np.float32(0)))) == R.THR_MAX          # the clamp: largest p below 1
    assert bool(R.keep_draws(np.array([0], dtype=np.uint32), 0.0)[0])                          # p = 0 keeps a draw of 0
    assert not bool(R.keep_draws(np.array([255], dtype=np.uint32), 2.0 ** -24)[0])
    assert bool(R.keep_draws(np.array([256], dtype=np.uint32), 2.0 ** -24)[0])


def test_inv_is_the_fp32_quotient():
    assert R.inv(0.5) == np.float32(2) and R.inv(0.75) == np.float32(4) and R.inv(0.0) == np.float32(1)
    assert R.inv(0.1).dtype == np.float32 and R.inv(0.1) == np.float32(1) / np.float32(0.9)
    assert float(R.inv(0.1)) != 1 / 0.9


@pytest.mark.parametrize("mutate", [m for m in R.MUTATIONS if m != "thr_floor_f64"])
def test_generator_mutants_change_the_keep_bits(mutate):
    """65 536 keep bits at p = 0.5 under a state with high words: a wrong generator agrees on about half of them"""
    idx = np.arange(65536)
    good = R.keep(SEED, OFFSET, SITE, idx, 0.5)
    bad = R.keep(SEED, OFFSET, SITE, idx, 0.5, mutate=mutate)
    frac = float((good != bad).mean())
    assert frac > 0.40, (mutate, frac)
    assert abs(float(good.mean()) - 0.5) < 4 * 0.5 / 256                                       # 4 sigma of 65 536 fair bits


def test_no_offset_hi_shows_only_with_a_high_offset_word():
    """why the GPU states include offsets at and past 2^32"""
    idx = np.arange(4096)
    assert np.array_equal(R.draws(SEED, 7, SITE, idx), R.draws(SEED, 7, SITE, idx, mutate="no_offset_hi"))
    assert not np.array_equal(R.draws(SEED, 1 << 32, SITE, idx), R.draws(SEED, 1 << 32, SITE, idx, mutate="no_offset_hi"))


def test_threshold_mutant_and_its_witnesses():
    """p = 0.1 is no fp32 number: the fp32 threshold is 429496736, floor(0.1 * 2^32) in float64 is 429496729.  A draw between
    the two is dropped by the rule and kept by the mutant; at p = 0.5 the two agree everywhere."""
    lo, hi = int(R.threshold(0.1, mutate="thr_floor_f64")), int(R.threshold(0.1))
    assert (lo, hi) == (429496729, 429496736)
    r = np.array([lo - 1, lo, hi - 1, hi], dtype=np.uint32)
    assert R.keep_draws(r, 0.1).tolist() == [False, False, False, True]
    assert R.keep_draws(r, 0.1, mutate="thr_floor_f64").tolist() == [False, True, True, True]
    assert int(R.threshold(0.5, mutate="thr_floor_f64")) == int(R.threshold(0.5))
    # the recorded elements whose draws lie in that window: what the GPU file launches the kernels on
    for seed, offset, site, idx in (R.WITNESS, R.WITNESS_DROPPATH):
        d = int(R.draws(seed, offset, site, np.array([idx]))[0])
        assert lo <= d < hi, d
        assert not R.keep(seed, offset, site, np.array([idx]), R.WITNESS_P)[0]
        assert R.keep(seed, offset, site, np.array([idx]), R.WITNESS_P, mutate="thr_floor_f64")[0]
    assert R.WITNESS[3] < 264 * 384 and R.WITNESS_DROPPATH[3] < 257
