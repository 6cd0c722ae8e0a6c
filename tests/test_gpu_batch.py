"""Batched compression of many small blocks (bscgpu_bwt_batch_device / bscgpu_compress_batch*): every block's output must equal
what the reference (and our single-block path) produce for that block alone."""
import numpy as np
import pytest

from test_gpu_device import _corpus

pytestmark = pytest.mark.gpu

MIB = 1 << 20


@pytest.fixture(scope="module")
def bctx():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from libbsc_amd import GpuContext
    c = GpuContext(0, max_n=(16 << 20) + 4096)
    yield c
    c.close()


def _hazards(rng):
    from libbsc_amd.synth import synth_text_v1
    t = synth_text_v1(11, 70000)
    fib = [b"a", b"ab"]
    while len(fib[-1]) < 100000:
        fib.append(fib[-1] + fib[-2])
    cases = [
        ("twin-a", t[:30000]), ("twin-b", t[:30000].copy()),
        ("prefix", t[:20000]), ("whole", t[:45000]),
        ("head", t[:50000]), ("its-tail", t[40000:50000]),
        ("ones", np.full(40000, 7, np.uint8)), ("rand256", rng.integers(0, 256, 40000, dtype=np.uint8)),
        ("ones-short", np.full(3000, 200, np.uint8)),
        ("fib", np.frombuffer(fib[-1], np.uint8).copy()), ("periodic", np.tile(np.frombuffer(b"abcab", np.uint8), 30000)),
        ("text", synth_text_v1(3, 80000)),
    ]
    for n in [0, 1, 15, 16, 17, 29, 65535, 65536, MIB - 1]:
        cases.append((f"n{n}", synth_text_v1(13 + n, n) if n else np.zeros(0, np.uint8)))
    return cases


def _bwt_check(bctx, ref, cases, aux):
    import torch
    sizes = [c[1].size for c in cases]
    flat = np.concatenate([c[1] for c in cases]) if sum(sizes) else np.zeros(1, np.uint8)
    dT = torch.from_numpy(np.ascontiguousarray(flat)).cuda()
    got = bctx.bwt_batch(dT, sizes, aux=aux)
    for (name, data), (L, prim, idx) in zip(cases, got):
        wL, wprim, widx = ref.bwt_encode(data, aux=aux)
        assert prim == wprim, f"{name} (n={data.size}): primary {prim} != {wprim}"
        if wprim < 0:
            continue
        assert np.array_equal(L, wL[:data.size]), f"{name} (n={data.size}): L differs"
        if aux:
            assert idx == widx, f"{name}: aux indexes differ"


@pytest.mark.parametrize("aux", [True, False])
def test_bwt_batch_matches_reference(bctx, ref, aux):
    rng = np.random.default_rng(1)
    cases = [c for c in _corpus(rng) if c[1].size < 4 * MIB] + _hazards(rng)
    order = rng.permutation(len(cases))
    shuffled = [cases[i] for i in order]
    # several batches, so that the same block sits beside different neighbours
    for k in range(3):
        part = shuffled[k::3]
        _bwt_check(bctx, ref, part, aux)


def _compress_cases(rng):
    from libbsc_amd.synth import synth_text_v1
    cases = [synth_text_v1(21 + i, int(n)) for i, n in enumerate(rng.integers(1000, 200000, 12))]
    cases += [rng.integers(0, 256, n, dtype=np.uint8) for n in (5000, 70000)]            # stored
    cases += [np.frombuffer(bytes(range(40)) * 2, np.uint8)[:n].copy() for n in (27, 28, 29, 30)]
    cases += [np.zeros(0, np.uint8), np.zeros(100, np.uint8), synth_text_v1(5, 65536), synth_text_v1(6, 65535)]
    return cases


def _roundtrip(ref, blk, data):
    from libbsc_amd import api
    assert ref.decompress(blk) == data.tobytes()
    assert bytes(api.bsc_decompress(blk)) == data.tobytes()


@pytest.mark.parametrize("coder", [1, 2, 3])
@pytest.mark.parametrize("lzp", [(0, 0), (15, 128)])
def test_compress_batch_matches_reference(bctx, ref, coder, lzp):
    rng = np.random.default_rng(coder * 7 + lzp[0])
    cases = _compress_cases(rng)
    got = bctx.compress_batch(cases, 1, coder, lzp[0], lzp[1], 3)
    for data, blk in zip(cases, got):
        want = ref.compress(data, 1, coder, lzp[0], lzp[1])
        assert blk == want, f"n={data.size} coder={coder} lzp={lzp}"
        _roundtrip(ref, blk, data)


def test_compress_batch_mixed_routes(bctx, ref):
    """small blocks, blocks at and above the threshold, and a whole batch sorted by ST5 (all single path)"""
    import torch
    from libbsc_amd.synth import synth_text_v1
    cases = [synth_text_v1(31, 50000), synth_text_v1(32, MIB - 1), synth_text_v1(33, MIB), synth_text_v1(34, 3 * MIB // 2),
             synth_text_v1(35, 1000), np.zeros(10, np.uint8)]
    for sorter in (1, 5):
        got = bctx.compress_batch(cases, sorter, 1)
        for data, blk in zip(cases, got):
            assert blk == ref.compress(data, sorter, 1), f"sorter={sorter} n={data.size}"
        flat = torch.from_numpy(np.concatenate(cases)).cuda()
        got_d = bctx.compress_batch_device(flat, [c.size for c in cases], sorter, 1)
        assert got_d == got
    for data, blk in zip(cases, got):
        _roundtrip(ref, blk, data)


def test_compress_batch_device_matches_reference(bctx, ref):
    import torch
    rng = np.random.default_rng(5)
    cases = _compress_cases(rng)
    flat = torch.from_numpy(np.concatenate(cases)).cuda()
    for coder in (1, 2, 3):
        got = bctx.compress_batch_device(flat, [c.size for c in cases], 1, coder)
        for data, blk in zip(cases, got):
            assert blk == ref.compress(data, 1, coder), f"n={data.size} coder={coder}"


def test_several_passes(ref):
    """a small context: a few thousand blocks take many passes; every output equals the single-block path and the reference"""
    import torch
    from libbsc_amd import GpuContext
    from libbsc_amd.synth import synth_text_v1
    rng = np.random.default_rng(99)
    sizes = [int(x) for x in rng.integers(1, 24000, 2500)]
    text = synth_text_v1(77, sum(sizes))
    offs = np.concatenate([[0], np.cumsum(sizes)])
    cases = [text[offs[b]:offs[b + 1]].copy() for b in range(len(sizes))]
    c = GpuContext(0, max_n=4 << 20)
    try:
        got = c.compress_batch(cases, 1, 1)
        dT = torch.from_numpy(text).cuda()
        got_d = c.compress_batch_device(dT, sizes, 1, 1)
        assert got_d == got
        for b in range(0, len(cases), 5):
            d = torch.from_numpy(cases[b]).cuda()
            single = c.compress_device(d, cases[b].size, 1, 1).tobytes() if cases[b].size > 0 else None
            if single is not None:
                assert got[b] == single, f"block {b}: batch != single-block path"
            assert got[b] == ref.compress(cases[b], 1, 1), f"block {b}: batch != reference"
    finally:
        c.close()


def test_bad_arguments(bctx):
    import ctypes as C
    from libbsc_amd import _native as N
    L = N.lib()
    sz = np.array([10, 20], np.int32)
    inp = np.arange(30, dtype=np.uint8)
    out = np.full(100, 0xAB, np.uint8)
    res = np.full(2, 12345, np.int32)
    assert L.bscgpu_compress_batch(bctx.h, N.np_ptr(inp), N.np_ptr(sz), -1, N.np_ptr(out), N.np_ptr(res), 0, 0, 1, 1, 3) == -1
    assert L.bscgpu_compress_batch(bctx.h, None, N.np_ptr(sz), 2, N.np_ptr(out), N.np_ptr(res), 0, 0, 1, 1, 3) == -1
    assert L.bscgpu_compress_batch(bctx.h, N.np_ptr(inp), None, 2, N.np_ptr(out), N.np_ptr(res), 0, 0, 1, 1, 3) == -1
    assert L.bscgpu_compress_batch(bctx.h, N.np_ptr(inp), N.np_ptr(sz), 2, None, N.np_ptr(res), 0, 0, 1, 1, 3) == -1
    assert L.bscgpu_compress_batch(None, N.np_ptr(inp), N.np_ptr(sz), 2, N.np_ptr(out), N.np_ptr(res), 0, 0, 1, 1, 3) == -1
    neg = np.array([10, -5], np.int32)
    assert L.bscgpu_compress_batch(bctx.h, N.np_ptr(inp), N.np_ptr(neg), 2, N.np_ptr(out), N.np_ptr(res), 0, 0, 1, 1, 3) == -1
    assert L.bscgpu_compress_batch_device(bctx.h, None, N.np_ptr(sz), 2, N.np_ptr(out), N.np_ptr(res), 1, 1, 3) == -1
    prim = np.full(2, 7, np.int32)
    assert L.bscgpu_bwt_batch_device(bctx.h, None, None, N.np_ptr(sz), 2, N.np_ptr(prim), None, None) == -1
    assert L.bscgpu_bwt_batch_device(bctx.h, None, None, N.np_ptr(neg), 2, N.np_ptr(prim), None, None) == -1
    assert (out == 0xAB).all() and (res == 12345).all() and (prim == 7).all(), "a refused call wrote something"
    # a bad mode is every block's own error, as bsc_compress(block) returns it
    res2 = bctx.compress_batch([inp[:10], inp[:20]], sorter=9)
    assert res2 == [-1, -1]
