"""Inputs and a plain oracle for the inverse BWT's verdict on damaged (L, primary index) pairs.

Rows 0..n: row 0 is the empty suffix, row `idx` (1-based primary index) carries the sentinel, sym(row) = L[row] below idx and
L[row - 1] above.  LF over the n other rows is the stable counting sort of their symbols, shifted by one (row 0 is the smallest);
with the sentinel row sent to row 0 it is a permutation of the n + 1 rows.  The pair is VALID iff that permutation is one cycle:
the walk from row 0 meets the sentinel row after exactly n steps, and the text is what it reads off backwards.  Anything else is
LIBBSC_DATA_CORRUPT (-6).  numpy and Python only: nothing here imports the library under test (the large texts come from
libbsc_amd.synth, a numpy generator).
"""
import functools

import numpy as np

DATA_CORRUPT = -6

SIZES = (2, 3, 7, 15, 31, 63, 127, 254, 255, 256, 383, 384)      # rows / 128 goes 1 -> 2 -> 3 across these
ALPHABETS = (2, 4, 26)
LARGE_SIZES = (65536, 300_000, (1 << 20) + 17)


def _lf(L, idx):
    """-> (sym[row], lf[row]) for rows 0..n; the sentinel row's entries are 0"""
    L = np.ascontiguousarray(L, dtype=np.uint8)
    n = L.size
    rows = np.concatenate([np.arange(0, idx), np.arange(idx + 1, n + 1)])       # the non-sentinel rows, in row order
    order = np.argsort(L, kind="stable")                                         # stable counting sort of their symbols
    rank = np.empty(n, np.int64)
    rank[order] = np.arange(n)
    sym = np.zeros(n + 1, np.uint8)
    lf = np.zeros(n + 1, np.int64)
    sym[rows] = L
    lf[rows] = rank + 1
    return sym, lf


def lf_verdict(L, idx):
    """-> (0, text) when the rows form one cycle of n + 1, (-6, None) otherwise"""
    L = np.ascontiguousarray(L, dtype=np.uint8)
    n = L.size
    assert 1 <= idx <= n
    sym, lf = _lf(L, idx)
    nxt = lf.tolist()
    seen = []
    row = 0
    for _ in range(n):
        if row == idx:
            return DATA_CORRUPT, None                   # the sentinel row before step n
        seen.append(row)
        row = nxt[row]
    if row != idx:
        return DATA_CORRUPT, None                       # not on the sentinel row at step n
    return 0, sym[np.array(seen[::-1], np.int64)] if n else np.zeros(0, np.uint8)


def parent_host_rule(L, idx):
    """The rule bsc_bwt_decode had before the sentinel trap: the sentinel row leads back to row 0 with a 0 byte, and only the
    row after n steps is compared -> (0, text) or (-6, None).  Kept so the tests can show that the list holds pairs it accepts."""
    L = np.ascontiguousarray(L, dtype=np.uint8)
    n = L.size
    sym, lf = _lf(L, idx)
    nxt = lf.tolist()
    out = np.zeros(n, np.uint8)
    row = 0
    for k in range(n - 1, -1, -1):
        out[k] = sym[row]
        row = nxt[row]
    return (0, out) if row == idx else (DATA_CORRUPT, None)


# ---- forward transform, from the definition --------------------------------------------------------------------------------------
def suffix_array(T):
    """suffix array of T with the end of the text below every symbol: naive for short texts, prefix doubling for long ones"""
    T = np.ascontiguousarray(T, dtype=np.uint8)
    n = T.size
    if n <= 512:
        b = T.tobytes()
        return np.array(sorted(range(n), key=lambda i: b[i:]), np.int64)
    rank = T.astype(np.int64) + 1                        # 0 = past the end
    k = 1
    while True:
        second = np.zeros(n, np.int64)
        second[:n - k] = rank[k:]
        key = rank * (n + 2) + second
        sa = np.argsort(key, kind="stable")
        ks = key[sa]
        new = np.empty(n, np.int64)
        new[sa] = np.concatenate([[0], np.cumsum(ks[1:] != ks[:-1])]) + 1
        rank = new
        if int(rank.max()) == n or k >= n:
            return sa
        k *= 2


def aux_rate(n):
    m = n // 8
    return 1 if m == 0 else 1 << (m.bit_length() - 1)


def bwt(T, aux=False):
    """-> (L, 1-based primary index[, aux indexes]) as bsc_bwt_encode writes them"""
    T = np.ascontiguousarray(T, dtype=np.uint8)
    n = T.size
    sa = suffix_array(T)
    L = np.concatenate([T[n - 1:], T[sa[sa != 0] - 1]])
    isa = np.empty(n, np.int64)
    isa[sa] = np.arange(n)
    idx = int(isa[0]) + 1
    if not aux:
        return L, idx
    r = aux_rate(n)
    return L, idx, [int(isa[t * r]) for t in range(1, (n - 1) // r + 1)]


# ---- the lists ------------------------------------------------------------------------------------------------------------------------
class Pair:
    __slots__ = ("kind", "L", "idx", "aux", "T", "rc", "text", "cls")

    def __init__(self, kind, L, idx, T, aux=None):
        self.kind, self.L, self.idx, self.T, self.aux = kind, np.ascontiguousarray(L, dtype=np.uint8), int(idx), T, aux
        self.rc, self.text = lf_verdict(self.L, self.idx)
        if self.rc != 0:
            self.cls = "broken"
        else:
            self.cls = "valid" if T is not None and np.array_equal(self.text, T) else "valid-other"

    def __repr__(self):
        return f"<{self.kind} n={self.L.size} idx={self.idx} {self.cls}>"


def _rand_text(rng, n, alphabet):
    return (rng.integers(0, alphabet, n) + ord("a")).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def index_pairs(seed=20):
    """every primary index 1..n of random texts of SIZES x ALPHABETS: the right one (valid) and every wrong one"""
    rng = np.random.default_rng(seed)
    out = []
    for n in SIZES:
        for a in ALPHABETS:
            T = _rand_text(rng, n, a)
            L, idx = bwt(T)
            out += [Pair(f"index/a{a}", L, i, T) for i in range(1, n + 1)]
            assert out[-n + idx - 1].cls == "valid", (n, a)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def column_pairs(seed=21):
    """300 blocks of 8..400 bytes with 1 to 3 bytes of L changed at the right index (with the undamaged block's aux indexes)"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(300):
        n, a = int(rng.integers(8, 401)), int(rng.choice(ALPHABETS))
        T = _rand_text(rng, n, a)
        L, idx, aux = bwt(T, aux=True)
        L = L.copy()
        for pos in rng.choice(n, int(rng.integers(1, 4)), replace=False):
            L[pos] = (L[pos] - ord("a") + int(rng.integers(1, max(a, 2)))) % max(a, 2) + ord("a")       # another symbol of the alphabet
        out.append(Pair(f"column/a{a}", L, idx, T, aux))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def tiny_pairs():
    """every L of 2 and 3 bytes over three symbols with every primary index: the blocks a batched pass packs by the hundred into
    one tile of its keys kernel"""
    out = []
    for n in (2, 3):
        for code in range(3 ** n):
            L = np.array([ord("a") + code // 3 ** j % 3 for j in range(n)], np.uint8)
            out += [Pair("tiny", L, i, None) for i in range(1, n + 1)]
    return tuple(out)


def small_pairs():
    return index_pairs() + column_pairs() + tiny_pairs()


@functools.lru_cache(maxsize=None)
def large_pairs():
    """synth_text_v1 blocks of LARGE_SIZES: the right pair, index +- 1, index 1, index n, and a 100-byte stretch of L overwritten"""
    from libbsc_amd.synth import synth_text_v1
    out = []
    for k, n in enumerate(LARGE_SIZES):
        T = synth_text_v1(40 + k, n)
        L, idx, aux = bwt(T, aux=True)
        out.append(Pair("large/right", L, idx, T, aux))
        for bad in sorted({idx - 1, idx + 1, 1, n} - {idx, 0, n + 1}):
            out.append(Pair("large/index", L, bad, T))
        L2 = L.copy()
        L2[1000:1100] = L2[5000:5100]
        out.append(Pair("large/column", L2, idx, T, aux))
    return tuple(out)


def census(pairs):
    """-> {class: count} and the number of broken pairs the parent's host rule accepts"""
    count = {"valid": 0, "valid-other": 0, "broken": 0}
    accepted = 0
    for p in pairs:
        count[p.cls] += 1
        if p.cls == "broken" and parent_host_rule(p.L, p.idx)[0] == 0:
            accepted += 1
    return count, accepted
