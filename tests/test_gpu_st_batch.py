"""Batched sort transform (bscgpu_st_batch_device, and ST3..ST8 blocks in bscgpu_compress_batch*): many blocks in one sort per pass,
every block's bytes and index equal to what the reference gives for that block alone."""
import os
import subprocess
import sys

import numpy as np
import pytest

from test_gpu_batch import _hazards

pytestmark = pytest.mark.gpu

MIB = 1 << 20
KS = [3, 4, 5, 6, 7, 8]


@pytest.fixture(scope="module")
def bctx():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from libbsc_amd import GpuContext
    c = GpuContext(0, max_n=(16 << 20) + 4096)
    yield c
    c.close()


def _cases(rng):
    """the BWT batch's hazard list with blocks shorter than the order (n = 2 .. 8, constant and all-distinct) between the larger ones"""
    big = _hazards(rng)
    short = []
    for n in range(2, 9):
        short.append((f"const{n}", np.full(n, 65 + n, np.uint8)))
        short.append((f"distinct{n}", np.arange(10 * n, 11 * n, dtype=np.uint8)))
    out = []
    for i, c in enumerate(big):
        out.append(c)
        if i < len(short):
            out.append(short[i])
    out += short[len(big):]
    # neighbours that share content with a short block: the short block is a prefix of what follows it
    out += [("ab", np.frombuffer(b"ab", np.uint8).copy()), ("abab-long", np.tile(np.frombuffer(b"ab", np.uint8), 500)),
            ("abc", np.frombuffer(b"abc", np.uint8).copy()), ("abc", np.frombuffer(b"abc", np.uint8).copy())]
    return out


def _expect(ctx, ref, name, data, k, got, idx, features=None):
    n = data.size
    if n < 2:
        assert idx == 0 and np.array_equal(got, data), f"{name} (n={n}, k={k}): a block of < 2 bytes is unchanged, index 0"
        return
    if k <= 6:
        want, widx = ref.st_encode(data, k, features)
        assert idx == widx, f"{name} (n={n}, k={k}): index {idx} != {widx}"
        assert np.array_equal(got, want), f"{name} (n={n}, k={k}): bytes differ from the reference"
    else:   # the reference's CPU encoder stops at k = 6: its decoder judges, and this library's single-block path
        back, rc = ref.st_decode(got, k, idx, features)
        assert rc == 0 and np.array_equal(back, data), f"{name} (n={n}, k={k}): the reference's decoder does not give the block back"
        sout, sidx = ctx.st_encode(data, k)
        assert idx == sidx and np.array_equal(got, sout), f"{name} (n={n}, k={k}): differs from the single-block path"


@pytest.mark.parametrize("k", KS)
def test_st_batch_matches_reference(bctx, ref, k):
    import torch
    rng = np.random.default_rng(1)
    cases = _cases(rng)
    order = rng.permutation(len(cases))
    for part in (cases, [cases[i] for i in order]):           # the same block beside different neighbours, at other alignments
        sizes = [c[1].size for c in part]
        flat = np.concatenate([c[1] for c in part])
        # in place: dOut is dT
        dT = torch.from_numpy(flat).cuda()
        got = bctx.st_batch(dT, sizes, k)
        assert len(got) == len(part)
        for (name, data), (out, idx) in zip(part, got):
            _expect(bctx, ref, name, data, k, out, idx)
        # dOut apart: the same result, and dT is left as it was
        dT = torch.from_numpy(flat).cuda()
        dOut = torch.full((flat.size + 8,), 0xEE, dtype=torch.uint8, device="cuda")
        got2 = bctx.st_batch(dT, sizes, k, dOut=dOut)
        assert np.array_equal(dT.cpu().numpy(), flat), "dT changed although dOut is another buffer"
        assert (dOut[flat.size:].cpu().numpy() == 0xEE).all(), "bytes written past the batch"
        for (o1, i1), (o2, i2) in zip(got, got2):
            assert i1 == i2 and np.array_equal(o1, o2)


def test_st_batch_starts_anywhere(bctx, ref):
    """a pass that does not start on a 4-byte boundary of the caller's buffers (a single-path block of odd size in front of it)"""
    import torch
    from libbsc_amd.synth import synth_text_v1
    cases = [("lead", synth_text_v1(1, MIB + 3)), ("a", synth_text_v1(2, 4001)), ("b", synth_text_v1(3, 77)), ("c", synth_text_v1(4, 30000))]
    sizes = [c[1].size for c in cases]
    from libbsc_amd.gpu import st_batch_plan
    assert st_batch_plan(sizes, 5, bctx.max_n)[1] == [-1, 0, 0, 0]
    for k in (4, 8):
        dT = torch.from_numpy(np.concatenate([c[1] for c in cases])).cuda()
        for (name, data), (out, idx) in zip(cases, bctx.st_batch(dT, sizes, k)):
            _expect(bctx, ref, name, data, k, out, idx)


def test_several_passes_and_block_cap(ref):
    """a small context: thousands of tiny blocks (more than one pass's block cap) and a few hundred small ones (more bytes than
    one pass holds); every block against the reference (called without its own threads: thousands of calls), a sample against the
    single-block path"""
    import torch
    from libbsc_amd import GpuContext
    from libbsc_amd.gpu import ST_BATCH_MAX_BLOCKS, st_batch_plan
    from libbsc_amd.synth import synth_text_v1
    rng = np.random.default_rng(99)
    sizes = [int(x) for x in rng.integers(0, 40, 4200)] + [int(x) for x in rng.integers(1, 24000, 300)]
    text = synth_text_v1(77, sum(sizes))
    offs = np.concatenate([[0], np.cumsum(sizes)])
    cases = [text[offs[b]:offs[b + 1]] for b in range(len(sizes))]
    c = GpuContext(0, max_n=1 << 20)
    try:
        for k in (5, 6, 8):
            npass, plan = st_batch_plan(sizes, k, c.max_n)
            assert npass >= 4
            assert max(plan[:4200]) >= 1 and 4200 > ST_BATCH_MAX_BLOCKS, "the tiny blocks alone overflow one pass's block cap"
            dT = torch.from_numpy(text).cuda()
            got = c.st_batch(dT, sizes, k)
            for b, (out, idx) in enumerate(got):
                if k == 8 and b % 40:                      # (k = 8: the reference's decoder on every block, the single path on a sample)
                    if cases[b].size >= 2:
                        back, rc = ref.st_decode(out, k, idx, 1)
                        assert rc == 0 and np.array_equal(back, cases[b]), f"block {b} (n={cases[b].size}, k={k})"
                    else:
                        assert idx == 0 and np.array_equal(out, cases[b])
                    continue
                _expect(c, ref, f"block {b}", cases[b], k, out, idx, features=1)
    finally:
        c.close()


def _compress_list(rng):
    cases = [c[1] for c in _cases(rng)]
    cases += [rng.integers(0, 256, n, dtype=np.uint8) for n in (5000, 70000)]                      # stored
    cases += [np.frombuffer(bytes(range(40)) * 2, np.uint8)[:n].copy() for n in (27, 28, 29, 30)]   # around the header size
    return cases


@pytest.mark.parametrize("sorter", [3, 5, 8])
def test_compress_batch_st_matches_reference(bctx, ref, sorter):
    import torch
    from libbsc_amd import api
    from libbsc_amd.gpu import st_batch_plan
    rng = np.random.default_rng(sorter)
    cases = _compress_list(rng)
    sizes = [c.size for c in cases]
    assert st_batch_plan(sizes, sorter, bctx.max_n)[0] >= 1

    def check(got, lzp):
        for data, blk in zip(cases, got):
            if sorter <= 6:
                assert blk == ref.compress(data, sorter, 1, lzp[0], lzp[1]), f"n={data.size} sorter={sorter} lzp={lzp}"
            else:
                assert blk == api.bsc_compress(data, sorter, 1, lzp[0], lzp[1]), f"n={data.size} sorter={sorter} lzp={lzp}: != bsc_compress"
                assert ref.decompress(blk) == data.tobytes(), f"n={data.size} sorter={sorter} lzp={lzp}: the reference does not decode it"

    for lzp in ((0, 0), (15, 128)):
        check(bctx.compress_batch(cases, sorter, 1, lzp[0], lzp[1]), lzp)
    flat = torch.from_numpy(np.concatenate(cases)).cuda()
    check(bctx.compress_batch_device(flat, sizes, sorter, 1), (0, 0))


@pytest.mark.parametrize("k", [5, 8])
def test_the_batched_route_is_taken(bctx, k):
    """one pack launch per planned pass plus one per block of >= 2 bytes that the plan sends alone — not one per block"""
    import torch
    from libbsc_amd.gpu import st_batch_plan
    from libbsc_amd.synth import synth_text_v1
    sizes = [3000] * 300 + [MIB + 5, 0, 1, 2 * MIB] + [70000] * 200 + [0, 9]
    npass, plan = st_batch_plan(sizes, k, bctx.max_n)
    assert npass == 3 and plan.count(-1) == 4
    alone = sum(1 for n, p in zip(sizes, plan) if p < 0 and n >= 2)
    assert alone == 2
    dT = torch.from_numpy(synth_text_v1(8, sum(sizes))).cuda()
    bctx.profile(True)
    try:
        bctx.profile_reset()
        bctx.st_batch(dT, sizes, k)
        assert bctx.profile_get()["pack"]["launches"] == npass + alone
        # the compress call: the same passes (the two large blocks go through the call's pipe)
        few = sizes[:300]
        bctx.profile_reset()
        bctx.compress_batch_device(dT, few, k, 1)
        assert bctx.profile_get()["pack"]["launches"] == st_batch_plan(few, k, bctx.max_n)[0] == 1
        bctx.profile_reset()
        bctx.compress_batch([synth_text_v1(9 + i, 3000) for i in range(100)], k, 1)
        assert bctx.profile_get()["pack"]["launches"] == 1
    finally:
        bctx.profile(False)


def test_bad_arguments(bctx):
    import torch
    from libbsc_amd import _native as N
    L = N.lib()
    sz = np.array([10, 20], np.int32)
    neg = np.array([10, -5], np.int32)
    idx = np.full(2, 7, np.int32)
    d = torch.full((64,), 0xAB, dtype=torch.uint8, device="cuda")
    p = d.data_ptr()
    torch.cuda.synchronize()
    for k in (2, 9, 0, 1):
        assert L.bscgpu_st_batch_device(bctx.h, p, p, N.np_ptr(sz), 2, k, N.np_ptr(idx)) == -1
    assert L.bscgpu_st_batch_device(bctx.h, p, p, N.np_ptr(neg), 2, 5, N.np_ptr(idx)) == -1
    assert L.bscgpu_st_batch_device(bctx.h, p, p, N.np_ptr(sz), -1, 5, N.np_ptr(idx)) == -1
    assert L.bscgpu_st_batch_device(bctx.h, None, p, N.np_ptr(sz), 2, 5, N.np_ptr(idx)) == -1
    assert L.bscgpu_st_batch_device(bctx.h, p, None, N.np_ptr(sz), 2, 5, N.np_ptr(idx)) == -1
    assert L.bscgpu_st_batch_device(bctx.h, p, p, None, 2, 5, N.np_ptr(idx)) == -1
    assert L.bscgpu_st_batch_device(bctx.h, p, p, N.np_ptr(sz), 2, 5, None) == -1
    assert L.bscgpu_st_batch_device(None, p, p, N.np_ptr(sz), 2, 5, N.np_ptr(idx)) == -1
    assert (idx == 7).all() and (d.cpu().numpy() == 0xAB).all(), "a refused call wrote something"
    assert L.bscgpu_st_batch_device(bctx.h, None, None, N.np_ptr(sz), 0, 5, N.np_ptr(idx)) == 0      # an empty batch is fine


def test_give_up_is_retried_with_the_text_intact():
    """dOut = dT and a single-read digit pass that gives up (injected: BSC_RS_FAULT_DEV, see test_gpu_device): the post kernel has
    written the failed attempt over the caller's text by the time the give-up is seen, so the retry must sort the context's own copy"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = r"""
import sys
sys.path.insert(0, %r)
import numpy as np, torch
from libbsc_amd import GpuContext, api
ctx = GpuContext(0, max_n=(4 << 20) + 4096)
sizes = [60000] * 40 + [7, 1, 0, 100001]
T = api.synth_text_v1(5, sum(sizes))
for k in (5, 8):
    before = ctx.option_get(ctx.CNT_OS_RETRIES)
    got = ctx.st_batch(torch.from_numpy(T).cuda(), sizes, k)          # (k = 5: the process's first single-read sort — injected)
    retried = ctx.option_get(ctx.CNT_OS_RETRIES) - before
    assert retried == (1 if k == 5 else 0), retried
    o = 0
    for n, (out, idx) in zip(sizes, got):
        if n < 2:
            assert idx == 0 and np.array_equal(out, T[o:o + n]), (k, n)
        else:
            sout, sidx = ctx.st_encode(T[o:o + n], k)
            assert idx == sidx and np.array_equal(out, sout), (k, n)
        o += n
print("retried ok")
""" % root
    env = dict(os.environ, BSC_RS_FAULT_DEV="1", BSC_RS_ONESWEEP="2")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, cwd=root)
    assert r.returncode == 0 and "retried ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
