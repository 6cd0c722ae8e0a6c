"""The BWT's first sort with the key's leftover low digit folded into key packing (bwt.hip: bwt_fold_count / _scan / bwt_pack_fold kernels,
BSCGPU_OPT_BWT_FOLD): against libsais and the reference's compress, against the route it replaces, and — the sort's own result, not only
the BWT behind it — against a stable numpy sort of the packed keys."""
import os
import subprocess
import sys

import numpy as np
import pytest

import bwt_geometry_cases as gc
from pipeline_model import key_geometry

pytestmark = pytest.mark.gpu

PACK_TILE = 1024                     # FOLD_TILE of bwt.hip: suffixes per packing tile
BIG_N = gc.OS_MIN_RECORDS + 70_003   # through the single-read passes under the default mode


@pytest.fixture(scope="module")
def gctx():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but torch.cuda.is_available() is False")
    from libbsc_amd import GpuContext
    c = GpuContext(0, max_n=BIG_N + 4096)
    assert c.option_get(c.OPT_BWT_FOLD) == 1                          # the default under test
    c.option_set(c.OPT_RS_ONESWEEP, 2)                                # sorts of four tiles and more take the single-read passes
    yield c
    c.close()


# ---- texts ------------------------------------------------------------------------------------------------------------------
def _codes(K, T):
    return np.searchsorted(gc.alphabet(K), T).astype(np.int64)


def variant(K, n, kind):
    """markov(K, n) as is ("plain"); with a run of 40 copies of the smallest byte mid-block and 5 at the very end ("runs": tail suffixes share
    their padded keys with ordinary ones, stability decides); with every code's low four bits cleared ("one": one bucket takes everything —
    but for the first K characters, which keep the alphabet, and with it the geometry, what it was); with the codes' low four bits cycling
    0..15 along the text ("cycle": equal buckets; the first K characters are the codes 0..K-1, which is the same cycle)."""
    T = gc.markov(K, n, seed=500 + 7 * K + n % 991)
    a = gc.alphabet(K)
    if kind == "runs":
        T[n // 2:n // 2 + 40] = a[0]
        T[n - 5:] = a[0]
    elif kind == "one":
        c = _codes(K, T)
        c[K:] &= ~15
        T = a[c]
    elif kind == "cycle":
        c = _codes(K, T)
        i = np.arange(n)
        c2 = (c & ~15) | (i & 15)
        c2 = np.where(c2 < K, c2, i & 15)
        c2[:K] = np.arange(K)
        T = a[c2]
    assert T.size == n and np.unique(T).size == K
    return np.ascontiguousarray(T)


def packed_input(T, K):
    """The (key, value) records in the order key packing defines: the tail suffixes first, shortest first, then suffix order."""
    n = T.size
    g = key_geometry(K, n)
    cb, w, ps = g["cb"], g["w"], g["pred_shift"]
    c = np.searchsorted(np.unique(T), T).astype(np.uint64)
    cp = np.concatenate([c, np.zeros(w, np.uint64)])
    keys = np.zeros(n, np.uint64)
    for t in range(w):
        keys |= cp[t:t + n] << np.uint64(64 - cb * (t + 1))
    vals = np.arange(n, dtype=np.uint32)
    if ps:
        pred = np.concatenate([np.zeros(1, np.uint64), c[:-1]]).astype(np.uint32)
        vals = vals | (pred << np.uint32(ps))
    order = np.concatenate([np.arange(n - 1, n - w, -1), np.arange(0, n - w + 1)])
    return keys[order], vals[order]


def _bwt(gctx, T, fold):
    import torch
    gctx.option_set(gctx.OPT_BWT_FOLD, fold)
    before = gctx.option_get(gctx.CNT_BWT_FOLDED)
    d = torch.from_numpy(T).cuda()
    idx, _ = gctx.bwt_device(d, d, T.size)
    return d.cpu().numpy(), idx, gctx.option_get(gctx.CNT_BWT_FOLDED) - before


def _first_sort(gctx, T, fold):
    import torch
    gctx.option_set(gctx.OPT_BWT_FOLD, fold)
    return gctx.bwt_first_sort_device(torch.from_numpy(T).cuda(), T.size)


def check_case(gctx, ref, K, n, kind, folds=True):
    import torch
    T = variant(K, n, kind)
    want_L, want_idx, _ = ref.bwt_encode(T, aux=False)
    try:
        L1, idx1, moved1 = _bwt(gctx, T, 1)
        L0, idx0, moved0 = _bwt(gctx, T, 0)
        assert moved1 == (1 if folds else 0) and moved0 == 0, (K, n, kind, moved1, moved0)
        assert idx1 == want_idx and np.array_equal(L1, want_L[:n]), (K, n, kind)
        assert idx0 == idx1 and np.array_equal(L0, L1), (K, n, kind)
        kin, vin = packed_input(T, K)
        order = np.argsort(kin, kind="stable")
        for fold in (1, 0):
            k, v = _first_sort(gctx, T, fold)
            assert np.array_equal(k, kin[order]), (K, n, kind, fold)
            assert np.array_equal(v, vin[order]), (K, n, kind, fold)
        if n <= 200_000:
            gctx.option_set(gctx.OPT_BWT_FOLD, 1)
            want = ref.compress(T, 1, 1)
            assert gctx.compress_device(torch.from_numpy(T).cuda(), n, 1, 1).tobytes() == want, (K, n, kind)
            gctx.option_set(gctx.OPT_BWT_FOLD, 0)
            assert gctx.compress_device(torch.from_numpy(T).cuda(), n, 1, 1).tobytes() == want, (K, n, kind)
    finally:
        gctx.option_set(gctx.OPT_BWT_FOLD, 1)


KINDS = ("plain", "runs", "one", "cycle")
# exactly four pass tiles of 7680 records, one record more, ragged; and the records that are no tails (n - w + 1 of them) one short of
# thirty-two packing tiles, exactly that many, one more (w = 12 at K = 32, 10 at K = 64)
CASES = [(K, n) for K in (17, 32, 33, 64) for n in (30_720, 30_721, 100_003)]
CASES += [(32, 32 * PACK_TILE - 1), (32, 32 * PACK_TILE + 1), (32, 32 * PACK_TILE + 10), (32, 32 * PACK_TILE + 11), (32, 32 * PACK_TILE + 12),
          (64, 32 * PACK_TILE - 1), (64, 32 * PACK_TILE + 9), (64, 32 * PACK_TILE + 10)]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("K,n", CASES, ids=[f"K{K}-n{n}" for K, n in CASES])
def test_folded_first_sort(gctx, ref, K, n, kind):
    check_case(gctx, ref, K, n, kind)


@pytest.mark.parametrize("K", [32, 64])
def test_folded_first_sort_under_the_default_mode(gctx, ref, K):
    """one case per character width above the default mode's threshold for the single-read passes"""
    gctx.option_set(gctx.OPT_RS_ONESWEEP, 3)
    try:
        check_case(gctx, ref, K, BIG_N, "plain")
    finally:
        gctx.option_set(gctx.OPT_RS_ONESWEEP, 2)


@pytest.mark.parametrize("K", [16, 128, 256])
def test_other_character_widths_keep_their_plan(gctx, ref, K):
    """cb = 4 and 8 leave no bits over, cb = 7 leaves seven: the counter stays where it is and the outputs are right"""
    check_case(gctx, ref, K, 100_003, "plain", folds=False)


def test_a_small_block_keeps_its_plan(gctx, ref):
    """below four pass tiles the sort takes the three-kernel passes, and packing stays what it was"""
    check_case(gctx, ref, 32, 30_719, "plain", folds=False)


def test_a_batched_pass_keeps_its_plan(gctx, ref):
    import torch
    sizes = [50_000, 50_003, 40_001]
    Ts = [gc.markov(32, n, seed=900 + b) for b, n in enumerate(sizes)]
    dT = torch.from_numpy(np.ascontiguousarray(np.concatenate(Ts))).cuda()
    dL = torch.empty_like(dT)
    before = gctx.option_get(gctx.CNT_BWT_FOLDED)
    got = gctx.bwt_batch(dT, sizes, aux=False, dL=dL)
    assert gctx.option_get(gctx.CNT_BWT_FOLDED) == before
    for T, (L, p, _) in zip(Ts, got):
        wL, wp, _ = ref.bwt_encode(T, aux=False)
        assert p == wp and np.array_equal(L, wL[:T.size])


def test_retry_after_a_give_up_takes_the_three_kernel_passes(ref):
    """BSC_RS_FAULT=1 in a child process: the first check reports a give-up that did not happen; the folded first attempt is thrown away,
    the transform is redone with the plan and the passes it had before, and the result is libsais's"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = r"""
import sys
sys.path.insert(0, %r)
sys.path.insert(0, %r)
import numpy as np
import torch
import bwt_geometry_cases as gc
from libbsc_amd import GpuContext
from oracle.refbind import Ref
ref = Ref()
n = 100_003
T = gc.markov(32, n, seed=77)
ctx = GpuContext(0, max_n=n + 4096)
ctx.option_set(ctx.OPT_RS_ONESWEEP, 2)
d = torch.from_numpy(T).cuda()
idx, _ = ctx.bwt_device(d, d, n)
wL, widx, _ = ref.bwt_encode(T, aux=False)
assert idx == widx and np.array_equal(d.cpu().numpy(), wL[:n])
assert ctx.option_get(ctx.CNT_OS_RETRIES) == 1, ctx.option_get(ctx.CNT_OS_RETRIES)
assert ctx.option_get(ctx.CNT_BWT_FOLDED) == 1, ctx.option_get(ctx.CNT_BWT_FOLDED)      # the first attempt only
assert ctx.option_get(ctx.OPT_RS_ONESWEEP) == 2
ctx.close()
print("retry ok", flush=True)
""" % (root, os.path.join(root, "tests"))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=dict(os.environ, BSC_RS_FAULT="1"), cwd=root)
    assert r.returncode == 0 and "retry ok" in r.stdout, (r.stdout + r.stderr)[-3000:]
