"""The first sort of the BWT at every key geometry (bwt_device_once: character width, key length, digit passes, text rounds' key length, values
with and without the predecessor's code, the block field of a batched pass): every case of bwt_geometry_cases.py — test_bwt_geometry_plan.py
checks what the list covers — against libsais (the reference's bwt_encode) and the reference's compress, single and batched."""
import os
import subprocess
import sys

import numpy as np
import pytest

import bwt_geometry_cases as gc
from pipeline_model import key_geometry

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gctx():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but torch.cuda.is_available() is False")
    from libbsc_amd import GpuContext
    c = GpuContext(0, max_n=(1 << 24) + 4096)
    yield c
    c.close()


def _aux_rate(n):
    m = n // 8
    return 1 if m == 0 else 1 << (m.bit_length() - 1)


@pytest.mark.parametrize("K,n", gc.SINGLE_CASES, ids=[f"K{K}-n{n}" for K, n in gc.SINGLE_CASES])
def test_single_block_geometry_matches_libsais(gctx, ref, K, n):
    """bscgpu_bwt_aux (host pointers) and bscgpu_bwt_device (in place, with aux indexes): L, primary index and aux indexes"""
    import torch
    T = gc.single_text(K, n)
    assert T.size == n and np.unique(T).size == K                       # the geometry under test is this alphabet's
    want_L, want_idx, want_aux = ref.bwt_encode(T, aux=(n >= 16))
    r = _aux_rate(n)
    if n >= 16:
        L, idx, I = gctx.bwt(T, aux_rate=r)
        assert [x - 1 for x in I[1:]][: (n - 1) // r] == want_aux, (K, n)
    else:
        L, idx, _ = gctx.bwt(T)
    assert idx == want_idx and np.array_equal(L, want_L[:n]), (K, n, key_geometry(K, n))
    d = torch.from_numpy(T).cuda()
    idx2, I2 = gctx.bwt_device(d, d, n, aux_rate=r)
    assert idx2 == want_idx and np.array_equal(d.cpu().numpy(), want_L[:n]), (K, n)
    if n >= 16:
        assert [x - 1 for x in I2[1:]][: (n - 1) // r] == want_aux, (K, n)
    if n <= 200_000:                                                   # whole block through the same first sort (the large ones: test_gpu_compress.py's sizes)
        assert gctx.compress_device(torch.from_numpy(T).cuda(), n, 1, 1).tobytes() == ref.compress(T, 1, 1), (K, n)


_BATCH_IDS = [f"K{K}-x{len(s)}-{sum(s)}" for K, s in gc.BATCH_CASES]


@pytest.mark.parametrize("K,sizes", gc.BATCH_CASES, ids=_BATCH_IDS)
def test_batched_geometry_matches_libsais_and_the_reference(gctx, ref, K, sizes):
    """bscgpu_bwt_batch_device with aux indexes, bscgpu_compress_batch_device and bscgpu_unbwt_batch_device on one pass of blocks whose
    common alphabet and count give the geometry under test; every block as the reference has it alone"""
    import torch
    Ts = gc.batch_texts(K, sizes)
    flat = np.ascontiguousarray(np.concatenate(Ts))
    assert np.unique(flat).size == K
    g = key_geometry(K, flat.size, len(sizes))
    dT = torch.from_numpy(flat).cuda()
    dL = torch.empty_like(dT)
    # with aux indexes (a block too short for them is refused by both, with the same code), then without: every block has a primary index
    got = gctx.bwt_batch(dT, sizes, aux=True, dL=dL)
    for b, (T, (L, p, idx)) in enumerate(zip(Ts, got)):
        wL, wp, widx = ref.bwt_encode(T, aux=True)
        assert p == wp, (K, b, T.size, g)
        if wp >= 0:
            assert np.array_equal(L, wL[:T.size]) and idx == widx, (K, b, T.size, g)
    got = gctx.bwt_batch(dT, sizes, aux=False, dL=dL)
    prim = []
    for b, (T, (L, p, _)) in enumerate(zip(Ts, got)):
        wL, wp, _ = ref.bwt_encode(T, aux=False)
        assert p == wp >= 0 and np.array_equal(L, wL[:T.size]), (K, b, T.size, g)
        prim.append(wp)
    back, res = gctx.unbwt_batch(dL, sizes, prim)
    assert all(r >= 0 for r in res), res
    assert np.array_equal(back.cpu().numpy()[:flat.size], flat), (K, g)
    # whole blocks: sampled where the batch is large (the reference codes every block on the CPU)
    step = max(1, len(sizes) // 64)
    blocks = gctx.compress_batch_device(dT, sizes, 1, 1)
    for b in range(0, len(sizes), step):
        assert blocks[b] == ref.compress(Ts[b], 1, 1), (K, b, sizes[b], g)


@pytest.mark.parametrize("cb", sorted(gc.LOG_CASES))
def test_rounds_run_at_every_character_width(ref, cb):
    """One child process per single-block width with the debug log on: a round on text keys, a long group split by the top key bits and a
    prefix-doubling round must all appear, and both texts must equal libsais's output (test_bwt_geometry_plan.py shows from the first
    sort's arithmetic that the two texts leave the long groups for it)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    K = gc.LOG_CASES[cb]
    code = r"""
import sys
sys.path.insert(0, %r)
sys.path.insert(0, %r)
import numpy as np
import bwt_geometry_cases as gc
from libbsc_amd import GpuContext
from oracle.refbind import Ref
ref = Ref()
ctx = GpuContext(0, max_n=gc.LOG_N + 4096)
for kind, T in zip(("split", "doubling"), gc.log_texts(%d)):
    print("==", kind, flush=True); sys.stderr.flush()
    L, idx, _ = ctx.bwt(T)
    sys.stderr.flush()
    wL, widx, _ = ref.bwt_encode(T, aux=False)
    assert idx == widx and np.array_equal(L, wL), kind
    print(kind, "ok", flush=True)
""" % (root, os.path.join(root, "tests"), K)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=dict(os.environ, BSCGPU_DEBUG="1"), cwd=root)
    log = r.stdout + r.stderr
    assert r.returncode == 0 and "split ok" in log and "doubling ok" in log, log[-3000:]
    assert "[bwt] text round" in log and " depth " in log, log[-3000:]              # a round on text keys ran to its end
    assert "split by the top key bits -> sorted" in log, log[-3000:]
    assert "[bwt] round " in log and " h=" in log, log[-3000:]                      # a prefix-doubling round
