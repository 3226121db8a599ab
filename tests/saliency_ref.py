"""Plain numpy statements of csrc/saliency.hip for tests/test_hip_saliency.py; tests/test_saliency_host.py pins them to np.sort.

* the select: the k-th largest of the uint32 magnitudes bits(g) & 0x7fffffff, by sorting them -- with the counts strictly above / at or
  above it and the count of non-finite keys (>= 0x7f800000);
* the mask: bit (i & 31) of word (i >> 5) = key(g[i]) >= threshold, the bits beyond n zero;
* the masked update has no restatement of its own: it IS the whole-buffer pair of csrc/optimizer.hip run on gradients multiplied by
  the mask, restricted to the masked-in elements (masked_gradient / merge below say how the two are put together).
"""
import numpy as np

NONFINITE = 0x7f800000
SWEEP = 2048 * 256 * 4                   # floats one grid-stride round of the select / the update covers
SIZES = [1, 3, 4, 255, 1025, SWEEP + 5]


def keys(g):
    g = np.ascontiguousarray(g, dtype=np.float32)
    return g.view(np.uint32) & np.uint32(0x7fffffff)


def select(g, k):
    """{threshold_bits, count_gt, count_ge, nonfinite} of the k-th largest magnitude, 1 <= k <= n."""
    ks = keys(g)
    assert 1 <= k <= ks.size
    thr = np.sort(ks)[ks.size - k]
    return dict(threshold_bits=int(thr), count_gt=int((ks > thr).sum()), count_ge=int((ks >= thr).sum()),
                nonfinite=int((ks >= NONFINITE).sum()))


def pack(flags):
    """bool flags -> uint32 words, little-endian bit order inside a word, the tail bits zero."""
    flags = np.asarray(flags, dtype=bool).reshape(-1)
    nwords = (flags.size + 31) // 32
    padded = np.zeros(nwords * 32, dtype=bool)
    padded[:flags.size] = flags
    return np.packbits(padded.reshape(nwords, 32), axis=1, bitorder="little").view(np.uint32).reshape(nwords)


def unpack(words, n):
    words = np.ascontiguousarray(words).view(np.uint32)
    return np.unpackbits(words.view(np.uint8).reshape(-1, 4), axis=1, bitorder="little").reshape(-1)[:n].astype(bool)


def mask_words(g, threshold_bits):
    return pack(keys(g) >= np.uint32(threshold_bits))


def masked_gradient(g, flags):
    """g where the flag is set, +0 elsewhere (what the masked pass 1 sums)."""
    return np.where(flags, g, np.float32(0)).astype(np.float32)


def merge(old, new, flags):
    """The buffer a masked pass 2 leaves: the whole-buffer run's value where the flag is set, the old bytes elsewhere."""
    out = np.array(old, copy=True)
    out[flags] = new[flags]
    return out


# ---------------------------------------------------------------------------------------------------------------- inputs of the select
def scaled_normal(n, seed):
    """N(0, 1) times a log-uniform scale over 2^-140 .. 2^20: every exponent from the denormals up."""
    rng = np.random.default_rng(seed)
    return (rng.standard_normal(n) * np.exp2(rng.uniform(-140, 20, n))).astype(np.float32)


def heavy_ties(n, seed):
    rng = np.random.default_rng(seed)
    vals = np.array([0.0, 1.0, -1.0, 0.5, 1.0000001, -3e-39, 7.25], dtype=np.float32)
    return vals[rng.integers(0, 7, n)]


def half_zeros(n, seed):
    """Half exact zeros with -0.0 mixed in, the rest Gaussian."""
    rng = np.random.default_rng(seed)
    g = rng.standard_normal(n).astype(np.float32)
    z = rng.random(n) < 0.5
    g[z] = np.where(rng.random(int(z.sum())) < 0.5, np.float32(0.0), np.float32(-0.0))
    return g


def denormals(n, seed):
    """Magnitudes around the smallest normal 2^-126, so that thresholds fall among denormals and just above them."""
    rng = np.random.default_rng(seed)
    bits = rng.integers(0x00000001, 0x01000000, n, dtype=np.uint32)      # keys below 2^-125: denormals and the first normal binade
    bits |= rng.integers(0, 2, n, dtype=np.uint32) << np.uint32(31)
    return bits.view(np.float32)


INPUTS = {"scaled": scaled_normal, "ties": heavy_ties, "zeros": half_zeros, "denormal": denormals}


def ranks(g, n):
    """k in {1, n // 2, n} where 1 <= k <= n allows, and the number of non-zeros where the buffer has zeros and non-zeros."""
    ks = {1, n // 2, n}
    nz = int((keys(g) != 0).sum())
    if 0 < nz < n:
        ks.add(nz)
    return sorted(k for k in ks if 1 <= k <= n)


def random_mask(n, density, seed):
    return np.random.default_rng(seed).random(n) < density


def zero_word_mask(n, seed):
    """Density 0.5 with every other 32-float word (and so whole granules) cleared."""
    m = random_mask(n, 0.5, seed)
    m[(np.arange(n) // 32) % 2 == 1] = False
    return m


def single_bit_mask(n, seed):
    m = np.zeros(n, dtype=bool)
    m[int(np.random.default_rng(seed).integers(0, n))] = True
    return m
