"""Plain restatement of the device sampler (csrc/sampling.hip) in Python / numpy, shared by
tests/test_target_sampling_host.py and tests/test_gpu_target_edges.py: Philox-4x32-10 with counter
(idx, stream, offset_lo, offset_hi) and key (seed_lo, seed_hi), the float32 `u01` / `below`, Floyd's subset, and from
them the exact picks of `proposal_target_sample_kernel` and the exact survivors of `anchor_target_subsample_kernel`.
Not a test module."""
import numpy as np

M32 = 0xFFFFFFFF
_MUL0, _MUL1 = 0xD2511F53, 0xCD9E8D57
_W0, _W1 = 0x9E3779B9, 0xBB67AE85  # key schedule (golden ratio, sqrt(3) - 1)

# the published Random123 known-answer vectors: (counter, key, output)
KNOWN_ANSWERS = (
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((M32, M32, M32, M32), (M32, M32), (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
)


def philox4x32_10(ctr4, key2):
    """ten Philox-4x32 rounds -> 4 x 32 random bits"""
    c0, c1, c2, c3 = [int(c) & M32 for c in ctr4]
    k0, k1 = [int(k) & M32 for k in key2]
    for _ in range(10):
        p0, p1 = _MUL0 * c0, _MUL1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & M32, (p0 >> 32) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + _W0) & M32, (k1 + _W1) & M32
    return c0, c1, c2, c3


def draw(seed, offset, stream, idx):
    """the word the kernels use: .x of Philox at counter (idx, stream, offset) under key seed (both 64 bit, split low / high)"""
    seed, offset = int(seed), int(offset)
    return philox4x32_10((idx, stream, offset & M32, (offset >> 32) & M32), (seed & M32, (seed >> 32) & M32))[0]


def u01(x):
    """[0, 1) from the top 24 bits, evaluated in float32 like the kernel"""
    return np.float32(int(x) >> 8) * np.float32(1.0 / 16777216.0)


def below(x, n):
    """uniform integer in [0, n): float32 product, truncated, clamped to n - 1"""
    v = int(np.float32(u01(x) * np.float32(n)))
    return v if v < n else n - 1


def floyd_subset(n, k, seed, offset, stream):
    """Floyd's uniform k-subset of range(n) -> sorted list: for j = n-k .. n-1 draw t = (x * (j + 1)) >> 32 (uniform
    in [0, j]); take t, or j when t is already in the set"""
    taken = set()
    for j in range(n - k, n):
        t = (draw(seed, offset, stream, j) * (j + 1)) >> 32
        taken.add(j if t in taken else t)
    assert len(taken) == k
    return sorted(taken)


def proposal_picks(counts, R, fg_per, seed, offset):
    """counts [B][2] = (fg, bg) candidates per image -> (picks int32 [B, R], fg_taken int32 [B]): positions in the
    image's fg list for slots < fg_taken, in its bg list behind. Stream 4b: the fg subset (emitted ascending), stream
    4b + 1: the with-replacement picks, indexed by the absolute slot."""
    counts = np.asarray(counts).reshape(-1, 2)
    B = counts.shape[0]
    picks = np.zeros((B, R), np.int32)
    taken = np.zeros((B,), np.int32)
    for b in range(B):
        nf, nb = int(counts[b, 0]), int(counts[b, 1])
        if nf > 0 and nb > 0:
            fg_n = min(fg_per, nf)
            picks[b, :fg_n] = floyd_subset(nf, fg_n, seed, offset, 4 * b)
            n = nb
        else:
            fg_n = R if nf > 0 else 0
            n = nf if nf > 0 else max(nb, 1)  # neither list has an entry: below(x, 1) = 0
        first = fg_n if (nf > 0 and nb > 0) else 0
        for j in range(first, R):
            picks[b, j] = below(draw(seed, offset, 4 * b + 1, j), n)
        taken[b] = fg_n
    return picks, taken


def anchor_keep_masks(counts, batchsize, num_fg, seed, offset):
    """counts [B][2] -> ([(kept fg-list positions or None, kept bg-list positions or None)] per image, float32
    1 / max(num_examples of the LAST image, 1)). None: that list is not subsampled (everything stays)."""
    counts = np.asarray(counts).reshape(-1, 2)
    keeps, ne = [], 0
    for b in range(counts.shape[0]):
        nf, nb = int(counts[b, 0]), int(counts[b, 1])
        kf = floyd_subset(nf, num_fg, seed, offset, 4 * b + 2) if nf > num_fg else None
        fg_after = min(nf, num_fg)
        num_bg = batchsize - fg_after
        kb = floyd_subset(nb, num_bg, seed, offset, 4 * b + 3) if nb > num_bg else None
        keeps.append((kf, kb))
        ne = fg_after + min(nb, num_bg)
    return keeps, np.float32(1.0) / np.float32(max(ne, 1))
