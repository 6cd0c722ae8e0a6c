"""Inputs of the BWT key-geometry sweep (test_bwt_geometry_plan.py checks what the list covers, test_gpu_bwt_geometry.py runs it).

Data: an order-2 Markov source over K symbols spread over the byte range (0 and 255 included) with planted repeats — uniform noise
would be sorted completely by the first pass and never reach the rounds."""
import numpy as np

from pipeline_model import key_geometry

OS_MIN_RECORDS = 512 * 7680          # above this the default mode sorts with the single-read digit passes
BATCH_MAX_N = 1 << 20                # BSCGPU_BATCH_MAX_N: larger blocks leave the batched route


def alphabet(K):
    """K byte values in increasing order, 0 and 255 among them (K >= 2)"""
    if K == 1:
        return np.array([0], np.uint8)
    return np.unique(np.round(np.linspace(0, 255, K)).astype(np.uint8))


def markov(K, n, seed, p_same=None, plant=True):
    """n symbols of an order-2 Markov source over K codes: next = (A[prev] + B[prev2] + g) mod K with g geometric (mostly 0: the
    likeliest successor), 4096 independent chains side by side; every code occurs (the first K positions); phrases planted.
    p_same = P(g = 0); by default such that a first-sort key of w characters carries some 13 bits of entropy whatever the alphabet —
    most suffixes then share their key with others and go on to the rounds."""
    rng = np.random.default_rng(seed)
    if p_same is None:
        p_same = {16: 0.8, 12: 0.73, 10: 0.68, 9: 0.64, 8: 0.6}[key_geometry(K, n)["w"]]
    lanes = 4096 if n >= 1 << 16 else 16
    steps = -(-n // lanes)
    A, B = rng.permutation(K), rng.permutation(K)
    out = np.empty((steps, lanes), np.int64)
    g = rng.geometric(p_same, (steps, lanes)) - 1
    p1, p2 = rng.integers(0, K, lanes), rng.integers(0, K, lanes)
    for t in range(steps):
        x = (A[p1] + B[p2] + g[t]) % K
        out[t] = x
        p2, p1 = p1, x
    c = np.ascontiguousarray(out.T).ravel()[:n]
    if n >= K:
        c[:K] = rng.permutation(K)
    if plant and n >= 20000:
        ph = rng.integers(0, K, 48)
        for plen, times in ((13, n // 2000), (40, n // 4000)):
            for p in rng.choice((n - 64) // 64, min(times, 3000), replace=False) * 64:
                c[p:p + plen] = ph[:plen]
    return alphabet(K)[c]


# ---- single blocks: (K, n) --------------------------------------------------------------------------------------------------
SINGLE_CASES = []
for _K in (16, 17, 32, 33, 64, 65, 128, 129, 256):           # both sides of every power of two: cb changes between K and K + 1
    SINGLE_CASES += [(_K, 3001), (_K, 100_003)]
SINGLE_CASES += [(2, 3001), (15, 15), (16, 16), (16, 17)]    # cb = 4: w = 16, blocks of w - 1, w, w + 1 characters (only here can n reach down to w: n >= K)
SINGLE_CASES += [(_K, OS_MIN_RECORDS + 70_003) for _K in (16, 32, 64, 128, 256)]     # one per cb through the single-read passes
SINGLE_CASES += [(256, 1 << 24), (256, (1 << 24) + 1)]       # cb = 8: the last n whose values carry the predecessor's code, the first that gathers


def single_text(K, n):
    return markov(K, n, seed=1000 * K + n % 997)


# ---- batched passes: (K of the pass, block sizes) ---------------------------------------------------------------------------
def _sizes(K, count, big=0):
    g = key_geometry(K, 1, count)
    w = g["w"]
    pat = [w - 1, w, w + 1, 3001, K + 1, 700, 2 * w - 1, 2 * w + 1]
    s = [pat[i % len(pat)] for i in range(count)]
    if big:
        s[0] = big
    if max(s) < K:                                           # some block must hold the whole alphabet
        s[-1] = max(K, 3001)
    return s


BATCH_CASES = []
for _K in (15, 16, 31, 32, 63, 64, 127, 128, 255, 256):      # the batch codes K + 1 values: cb changes between K and K + 1 here
    BATCH_CASES.append((_K, _sizes(_K, 100, big=100_003)))  # batch_bb = 7
BATCH_CASES += [(15, [3001]), (256, [100_003]), (9, [15]), (9, [16]), (9, [17])]                         # batch_bb = 0
BATCH_CASES += [(31, _sizes(31, 2)), (128, _sizes(128, 2, big=100_003))]                                # 1
BATCH_CASES += [(63, _sizes(63, 4)), (255, _sizes(255, 4)), (16, _sizes(16, 3))]                        # 2
BATCH_CASES += [(32, _sizes(32, 40)), (127, _sizes(127, 40)), (256, _sizes(256, 64))]                   # 6
BATCH_CASES += [(15, _sizes(15, 2100)), (256, _sizes(256, 4096))]                                       # 12
BATCH_CASES += [(_K, [500_009] * 8) for _K in (15, 31, 63, 127, 255, 256)]                              # one per cb through the single-read passes


def batch_texts(K, sizes):
    return [markov(K, n, seed=7000 + 31 * K + 17 * b + n % 1009, plant=n >= 100_000) if n >= K else alphabet(K)[np.random.default_rng(b + n).integers(0, K, n)]
            for b, n in enumerate(sizes)]


# ---- the debug-log check: per single-block cb a text whose long groups are split, and one that goes on to prefix doubling ---
LOG_CASES = {4: 16, 5: 32, 6: 64, 7: 128, 8: 256}           # cb -> K
LOG_N, LOG_PLANTS = 2 << 20, 3000


def log_texts(K):
    """(split, doubling): the source without its own planted phrases, plus 3000 copies of a phrase of exactly w characters, each followed by
    two uniformly random ones (one group of 3000 > 1024 records after the first sort, which the top bits of the next round's key tell
    apart), or of a phrase of 5 w characters (dozens of such groups that agree far beyond any round's key)."""
    w = key_geometry(K, LOG_N)["w"]
    out = []
    for plen, rnd in ((w, 2), (5 * w, 0)):
        rng = np.random.default_rng(50 + K + plen)
        c = markov(K, LOG_N, seed=90 + K, p_same=0.6, plant=False)
        a = alphabet(K)
        ph = a[rng.integers(0, K, plen)]
        for p in rng.choice((LOG_N - 256) // 256, LOG_PLANTS, replace=False) * 256:
            c[p:p + plen] = ph
            c[p + plen:p + plen + rnd] = a[rng.integers(0, K, rnd)]
        out.append(c)
    return out
