"""Inputs of the batched QLFC front end's tests (CPU and GPU): "sorted blocks" are plain byte strings here — the front end's
rules (split, runs, ranks) do not care whether a BWT produced them."""
import numpy as np

KI = 1 << 10
SIZES = [1, 2, 29, 255, 64 * KI, 256 * KI - 1, 256 * KI, 600 * KI, 1024 * KI - 1]
ALPHABETS = [2, 17, 33, 65, 200]


def runs_block(rng, n, k, mean_run=6.0, skew=1.3):
    """n bytes of geometric runs over k symbols (a random subset of the bytes) with a skewed distribution, as a BWT leaves text"""
    if n == 0:
        return np.zeros(0, np.uint8)
    alpha = rng.permutation(256)[:k].astype(np.uint8)
    p = 1.0 / np.arange(1, k + 1) ** skew
    p /= p.sum()
    m = int(n / mean_run) + 16
    lens = rng.geometric(1.0 / mean_run, m)
    while lens.sum() < n:
        lens = np.concatenate([lens, rng.geometric(1.0 / mean_run, m)])
    syms = alpha[rng.choice(k, lens.size, p=p)]
    return np.repeat(syms, lens)[:n].copy()


def mixed_batch(seed=0):
    """every size with every alphabet once over the batch (sizes cycle against alphabets), plus the blocks whose sampled positions
    hold fewer run starts than sub-blocks: they take the equal-split branch of coder.cpp:100-108"""
    rng = np.random.default_rng(seed)
    blocks = []
    for i, n in enumerate(SIZES):
        for j in range(2):
            blocks.append(runs_block(rng, n, ALPHABETS[(i + 3 * j) % len(ALPHABETS)], mean_run=3.0 + 4.0 * ((i + j) % 3)))
    blocks.append(np.zeros(0, np.uint8))
    const = np.full(256 * KI, 7, np.uint8)                         # no run start at all
    one = np.full(300 * KI, 9, np.uint8); one[1000] = 3            # two run starts, neither at a sampled position
    two = np.full(256 * KI + 5, 1, np.uint8); two[33:] = 2; two[65 + 32 * 100:] = 3      # exactly two sampled run starts: still <= nblocks
    three = np.full(400 * KI, 1, np.uint8); three[33:] = 2; three[97:] = 3; three[200001:] = 4   # three sampled (1 + 32 q): the adaptive branch, cuts 64 bytes apart
    blocks += [const, one, two, three]
    order = rng.permutation(len(blocks))
    return [blocks[i] for i in order]


def raw_second_sub_block(seed=5):
    """>= 256 KiB: long runs over four symbols, then noise.  The cut falls where half of the sampled run starts have been seen, inside
    the first part, so the second sub-block holds all the noise and is stored raw while the block as a whole still compresses."""
    rng = np.random.default_rng(seed)
    head = runs_block(rng, 420 * KI, 4, mean_run=4.0)
    return np.concatenate([head, rng.integers(0, 256, 100 * KI, dtype=np.uint8)])


def host_runs(a):
    """(sym, start) of the maximal runs of a"""
    if a.size == 0:
        return np.zeros(0, np.uint8), np.zeros(0, np.uint32)
    heads = np.flatnonzero(np.concatenate([[True], a[1:] != a[:-1]]))
    return a[heads], heads.astype(np.uint32)


def layouts_equal(a, b):
    """array-for-array comparison of two FrontBatch objects -> list of the names that differ"""
    bad = []
    if a.nsub != b.nsub or a.m != b.m:
        return [f"nsub {a.nsub}/{b.nsub} m {a.m}/{b.m}"]
    for name in ("blk_sub", "sub_start", "sub_size", "sub_run", "nsym", "sym", "start", "rank"):
        x, y = getattr(a, name), getattr(b, name)
        if not np.array_equal(x, y):
            w = np.flatnonzero(x != y)
            bad.append(f"{name}: {w.size} differ, first at {int(w[0])} ({int(x[w[0]])} != {int(y[w[0]])})")
    for s in range(a.nsub):
        if not np.array_equal(a.first_seen(s), b.first_seen(s)):
            bad.append(f"first_seen[{s}]")
            break
    return bad
