"""An independent model of the library's random draws (numpy, uint64 arithmetic, no torch, no GPU code; imported by
test_philox_ref_host.py and test_dropout_edges_gpu.py).

The rule, as sais_amd/csrc/philox.hpp and include/sais_hip.h publish it: the draw of element `idx` of dropout site `site` under
the state {seed, offset} is word idx % 4 of Philox4x32-10 (Salmon et al., SC'11) at
    counter = {idx / 4 low word, idx / 4 high word, site, offset low word}
    key     = {seed low word, seed high word ^ offset high word}
and the element is kept  <=>  draw >= (unsigned) min(p * 2^32, 4294967040), the product taken in fp32 (p is a float in the ABI).
Kept values are scaled by the fp32 quotient 1 / (1 - p).

This file follows that rule and the paper, not the kernel source.  `mutate=` turns the model into one of the wrong generators
the GPU comparisons have to notice (test_philox_ref_host.py shows that each one changes the keep bits)."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57                  # the two multipliers of Philox4x32
W0, W1 = 0x9E3779B9, 0xBB67AE85                  # the Weyl increments of the key (golden ratio, sqrt(3) - 1)
MASK32 = np.uint64(0xFFFFFFFF)
THR_MAX = 4294967040                             # 2^32 - 256: the largest fp32 below 2^32
MUTATIONS = ("rounds9", "swap_mult", "no_offset_hi", "idx_not_div4", "word_order", "thr_floor_f64")

# (seed, offset, site, idx) whose draw lies between the fp32 threshold of p = 0.1 (429496736) and floor(0.1 * 2^32) in
# float64 (429496729): kept only if the threshold is NOT taken in fp32.  Found by a search over seeds with this model
# (test_philox_ref_host.py re-derives the draws); idx < 264 * 384, so the element exists in every fused site's smallest
# full-size case.  WITNESS_DROPPATH is the same for sais_droppath_scales: site = the branch, idx = the sample, below 257.
WITNESS_P = 0.1
WITNESS = (7350, 0x0000000300000007, 7, 27554)              # draw 429496730
WITNESS_DROPPATH = (458762, 0x0000000300000007, 20, 169)     # draw 429496735


def _u64(x):
    return np.asarray(x).astype(np.uint64)


def philox4x32(counter, key, rounds=10, mult=(M0, M1)):
    """Philox4x32-`rounds`: counter = four arrays (or ints) of 32-bit words, key = two; returns four uint32 arrays"""
    c = [_u64(w) & MASK32 for w in counter]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = (_u64(w) & MASK32 for w in key)
    m0, m1 = np.uint64(mult[0]), np.uint64(mult[1])
    s = np.uint64(32)
    for _ in range(rounds):
        p0, p1 = m0 * c[0], m1 * c[2]                       # 32 x 32 -> 64 bits: no overflow in uint64
        c = [(p1 >> s) ^ c[1] ^ k0, p1 & MASK32, (p0 >> s) ^ c[3] ^ k1, p0 & MASK32]
        k0, k1 = (k0 + np.uint64(W0)) & MASK32, (k1 + np.uint64(W1)) & MASK32
    return [w.astype(np.uint32) for w in c]


def counter_key(seed, offset, site, idx, mutate=None):
    """the counter and key words of the rule for elements `idx` (seed, offset: Python ints in [0, 2^64))"""
    assert 0 <= seed < 1 << 64 and 0 <= offset < 1 << 64 and 0 <= site < 1 << 32
    idx = _u64(idx)
    q = idx if mutate == "idx_not_div4" else idx >> np.uint64(2)
    off_hi = 0 if mutate == "no_offset_hi" else offset >> 32
    counter = (q & MASK32, q >> np.uint64(32), np.uint64(site), np.uint64(offset & 0xFFFFFFFF))
    key = (np.uint64(seed & 0xFFFFFFFF), np.uint64((seed >> 32) ^ off_hi))
    return counter, key


def draws(seed, offset, site, idx, mutate=None):
    """uint32 draws of the elements `idx` (an int64 / uint64 array, any shape)"""
    assert mutate is None or mutate in MUTATIONS
    idx = _u64(idx)
    counter, key = counter_key(seed, offset, site, idx, mutate)
    words = philox4x32(counter, key, rounds=9 if mutate == "rounds9" else 10, mult=(M1, M0) if mutate == "swap_mult" else (M0, M1))
    w = (idx & np.uint64(3)).astype(np.int64)
    if mutate == "word_order":
        w = 3 - w
    return np.choose(w, words).astype(np.uint32)


def threshold(p, mutate=None):
    """the uint32 threshold of a drop probability p in [0, 1): fp32 product, clamped below 2^32"""
    if mutate == "thr_floor_f64":
        return np.uint32(min(int(np.floor(np.float64(p) * 2.0 ** 32)), THR_MAX))
    t = np.float32(p) * np.float32(2 ** 32)
    return np.uint32(min(t, np.float32(THR_MAX)))


def keep_draws(r, p, mutate=None):
    """keep bits of the draws `r` at probability p"""
    return np.asarray(r, dtype=np.uint32) >= threshold(p, mutate)


def keep(seed, offset, site, idx, p, mutate=None):
    return keep_draws(draws(seed, offset, site, idx, mutate), p, mutate)


def inv(p):
    """the fp32 scale of a kept value"""
    return np.float32(1) / (np.float32(1) - np.float32(p))
