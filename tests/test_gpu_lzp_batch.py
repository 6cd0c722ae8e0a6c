"""The LZP stage over all blocks of a pass (csrc/device/lzp.hip: bscgpu_lzp_batch_device; DESIGN §3.9, "A pass of small blocks") must give,
per block, what api.bsc_lzp_compress gives (and the reference, where it was built), with the path counters of the CPU stand-in summed
over the pass.  Inputs and the host encoder's answers: tests/lzp_batch_inputs.py."""
import os

import numpy as np
import pytest

import lzp_batch_inputs as B
import lzp_device_inputs as I
from libbsc_amd import api, gpu

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but torch.cuda.is_available() is False")
    return torch


@pytest.fixture(scope="module")
def ctx(torch_cuda):
    from libbsc_amd import GpuContext
    c = GpuContext(0, max_n=B.MAX_N)
    yield c
    c.close()


@pytest.fixture(scope="module")
def reference():
    """the compiled reference where it was built (oracle/_ref), else None: the host encoder, which the CPU tests pin to it, stands in"""
    from oracle.refbind import REF_SO, Ref
    return Ref() if os.path.exists(REF_SO) else None


_UP = {}


def _uploaded(torch, name, blocks):
    """a pass in HBM, uploaded once per name, and its host copy"""
    if name not in _UP:
        T = B.joined(blocks)
        _UP[name] = (torch.from_numpy(T if T.size else np.zeros(1, np.uint8)).cuda(), T)
    return _UP[name]


def _check(ctx, torch, name, blocks, h, m, f, reference=None):
    """the stage over the pass: results and bytes per block, the counters, the input left alone -> the counters"""
    want = B.wants(blocks, h, m, f)
    if reference is not None:
        for (key, T), w in zip(blocks, want):
            assert reference.lzp_compress(T, h, m, features=f) == w, (key, h, m, f, "host encoder vs reference")
    d, T = _uploaded(torch, name, blocks)
    got = ctx.lzp_compress_batch(d, B.sizes_of(blocks), h, m, f, device=True)
    for b, (g, w) in enumerate(zip(got, want)):
        assert g == w, (name, b, blocks[b][0], h, m, f)
    cnt = ctx.lzp_counters()
    assert cnt == B.staged_counters(blocks, h, m, f), (name, h, m, f)
    assert d[:T.size].cpu().numpy().tobytes() == T.tobytes(), "the input in HBM is the caller's"
    return cnt


# ---- the stage ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("features", I.FEATURES)
@pytest.mark.parametrize("h", I.HASHES)
def test_corpora_as_one_pass(ctx, torch_cuda, reference, h, features):
    blocks = B.corpora_pass()
    for m in I.MINLENS:
        _check(ctx, torch_cuda, "corpora", blocks, h, m, features, reference if features == 3 and h == 15 and m in (32, 128) else None)


def test_host_blocks_go_up_first(ctx, torch_cuda):
    """the list form of GpuContext.lzp_compress_batch"""
    blocks = B.corpora_pass()[:4]
    assert ctx.lzp_compress_batch([T for _, T in blocks], None, 15, 128, 3) == B.wants(blocks, 15, 128, 3)
    assert ctx.lzp_compress_batch([], None, 15, 128, 3) == []


@pytest.mark.parametrize("m", [8, 40])
def test_links_do_not_cross_chunks(ctx, torch_cuda, m):
    """every copy's stream is the stream of the block alone: a link into the chunk in front would be a match at the chunk's first
    positions (the copies are the same bytes, so every context of a copy sits at the same place in the chunk before it)"""
    blocks = B.neighbours_pass()
    for f in I.FEATURES:
        _check(ctx, torch_cuda, "neighbours", blocks, 15, m, f)
        got = ctx.lzp_compress_batch(_uploaded(torch_cuda, "neighbours", blocks)[0], B.sizes_of(blocks), 15, m, f, device=True)
        assert got[0] == got[1] == got[2] == ctx.lzp_compress(blocks[0][1], 15, m, features=f)
        assert got[3] == ctx.lzp_compress(blocks[3][1], 15, m, features=f)


@pytest.mark.parametrize("features", I.FEATURES)
@pytest.mark.parametrize("m", [4, 32, 255])
def test_thresholds_inside_a_pass(ctx, torch_cuda, reference, m, features):
    blocks = B.threshold_pass(m)
    assert sorted(B.sizes_of(blocks)) == sorted([262143, 262144, 262145, (1 << 20) - 1, 1, 17, 18, m + 31, m + 32, 0])
    _check(ctx, torch_cuda, ("thresholds", m), blocks, 15, m, features, reference if m == 32 else None)
    want = B.wants(blocks, 15, m, features)
    for (key, T), w in zip(blocks, want):
        if T.size in (0, 1, 17, 18, m + 31):
            assert w == api.NOT_COMPRESSIBLE, (key, "refused by size")


@pytest.mark.parametrize("features", I.FEATURES)
def test_raw_chunks(ctx, torch_cuda, reference, features):
    blocks = B.raw_pass()
    cnt = _check(ctx, torch_cuda, "raw", blocks, 15, 32, features, reference)
    want = B.wants(blocks, 15, 32, features)
    assert not isinstance(want[0], int) and not isinstance(want[1], int) and want[2] == api.NOT_COMPRESSIBLE
    assert cnt["raw_chunks"] == 2 == sum(gpu.lzp_staged_host(T, 15, 32, features=features)[1]["raw_chunks"] for _, T in blocks)


def test_more_chunks_than_cus(ctx, torch_cuda):
    blocks = B.many_small_pass()
    assert len(blocks) == 700
    for h, m in ((15, 8), (15, 40), (10, 4)):
        cnt = _check(ctx, torch_cuda, "many_small", blocks, h, m, 3)
        assert cnt["matches"] > 0


def test_block_limit(ctx, torch_cuda):
    blocks = B.tiny_pass()
    assert len(blocks) == 4096
    for h, m in ((15, 4), (14, 9), (10, 40)):
        _check(ctx, torch_cuda, "tiny", blocks, h, m, 3)
    d, T = _uploaded(torch_cuda, "tiny", blocks)
    out = torch_cuda.full((T.size + 64,), 0xA5, dtype=torch_cuda.uint8, device=d.device)
    from libbsc_amd import GpuError
    with pytest.raises(GpuError) as e:
        ctx.lzp_compress_batch(d, B.sizes_of(blocks) + [40], 15, 4, 3, device=True, dOut=out)
    assert e.value.code == api.BAD_PARAMETER
    assert bool((out == 0xA5).all()), "a refused pass writes nothing"


@pytest.mark.parametrize("name", list(I.PATHS))
def test_every_path_inside_a_pass(ctx, torch_cuda, name):
    _, h, m, f, counter = I.PATHS[name]
    blocks = B.path_pass(name)
    cnt = _check(ctx, torch_cuda, ("path", name), blocks, h, m, f)
    alone = gpu.lzp_staged_host(blocks[1][1], h, m, features=f)[1]
    if counter is None:
        assert B.wants(blocks, h, m, f)[1] == api.NOT_COMPRESSIBLE
    else:
        assert alone[counter] > 0 and cnt[counter] >= alone[counter], (name, cnt)


def test_refusals(ctx, torch_cuda):
    from libbsc_amd import GpuError
    blocks = B.corpora_pass()[:2]
    d, T = _uploaded(torch_cuda, "refusals", blocks)
    out = torch_cuda.full((T.size,), 0xA5, dtype=torch_cuda.uint8, device=d.device)
    sizes = B.sizes_of(blocks)
    for h, m, code in ((16, 32, gpu.NOT_SUPPORTED), (18, 32, gpu.NOT_SUPPORTED), (15, 3, api.BAD_PARAMETER), (15, 256, api.BAD_PARAMETER),
                       (9, 32, api.BAD_PARAMETER)):
        with pytest.raises(GpuError) as e:
            ctx.lzp_compress_batch(d, sizes, h, m, 3, device=True, dOut=out)
        assert e.value.code == code, (h, m)
    for bad in ([1 << 20], [100, -1], [(1 << 20) - 1] * 5):             # a block of 1 MiB, a negative size, a sum above max_n
        with pytest.raises(GpuError) as e:
            ctx.lzp_compress_batch(d, bad, 15, 32, 3, device=True, dOut=out)
        assert e.value.code == api.BAD_PARAMETER, bad
    assert bool((out == 0xA5).all()), "a refused pass writes nothing"
    assert ctx.lzp_compress_batch(d, [0, 0, 5], 15, 32, 3, device=True) == [api.NOT_COMPRESSIBLE] * 3, "no block reaches the encoder"


def test_tables_are_counted(torch_cuda):
    """the stage's tables are allocated on first use and counted by bscgpu_arena_bytes from then on"""
    from libbsc_amd import GpuContext
    c = GpuContext(0, max_n=1 << 20)
    try:
        before = c.arena_bytes
        T = I.corpora()["zeros"]
        assert c.lzp_compress_batch([T, T], None, 15, 32, 3) == [I.want("zeros", T, 15, 32, 3)] * 2
        grown = c.arena_bytes - before
        assert 600_000 < grown < 800_000, grown
        c.lzp_compress_batch([T], None, 15, 32, 3)
        assert c.arena_bytes - before == grown
    finally:
        c.close()


# ---- batched compression with the stage in front ------------------------------------------------------------------------------------------
LZPS = ((15, 128), (10, 8))


def _mixed_blocks():
    """compressible blocks of one and two chunks, a block LZP cannot shrink, 20 bytes, nothing, and 1 MiB + 5 that leaves the pass"""
    return [("text", I.corpora()["text"]), ("repeat", I.corpora()["repeat"]), ("random", I.corpora()["random"]),
            ("short", I.corpora()["text"][:20]), ("empty", np.zeros(0, np.uint8)), ("copied", I.corpora()["copied"]),
            ("big", I.threshold_block()[:(1 << 20) + 5]), ("f2_runs", I.corpora()["f2_runs"])]


_COMPRESSED = {}


def _want_blocks(sorter, coder, h, m):
    """api.bsc_compress per block, computed once"""
    k = (sorter, coder, h, m)
    if k not in _COMPRESSED:
        _COMPRESSED[k] = [api.bsc_compress(T, sorter, coder, lzp_hash=h, lzp_min=m) for _, T in _mixed_blocks()]
    return _COMPRESSED[k]


@pytest.mark.parametrize("coder", [1, 3])
@pytest.mark.parametrize("sorter", [1, 5])
def test_compress_batch_device_lzp(ctx, torch_cuda, reference, sorter, coder):
    blocks = _mixed_blocks()
    d, _ = _uploaded(torch_cuda, "mixed", blocks)
    sizes = B.sizes_of(blocks)
    for h, m in LZPS:
        want = _want_blocks(sorter, coder, h, m)
        p0, b0 = ctx.option_get(ctx.CNT_BATCH_LZP_PASSES), ctx.option_get(ctx.CNT_BATCH_LZP_BLOCKS)
        got = ctx.compress_batch_device(d, sizes, sorter, coder, lzp_hash=h, lzp_min=m)
        for i, (g, w) in enumerate(zip(got, want)):
            assert g == w, (blocks[i][0], sorter, coder, h, m)
            assert not isinstance(w, int) and api.bsc_decompress(w) == blocks[i][1].tobytes(), (blocks[i][0], sorter, coder, h, m)
        assert ctx.option_get(ctx.CNT_BATCH_LZP_PASSES) - p0 >= 1 and ctx.option_get(ctx.CNT_BATCH_LZP_BLOCKS) - b0 == 5
        if reference is not None and coder == 1 and (h, m) == (15, 128):
            for (key, T), w in zip(blocks, want):
                assert reference.compress(T, sorter, coder, lzp_hash=h, lzp_min=m) == w, (key, "bsc_compress vs reference")
    # the block LZP cannot shrink goes on without LZP: its header is the one of a call without LZP; a coded one says LZP
    assert _want_blocks(sorter, coder, 15, 128)[2] == _want_blocks(sorter, coder, 0, 0)[2]
    assert _want_blocks(sorter, coder, 15, 128)[1] != _want_blocks(sorter, coder, 0, 0)[1]      # (`repeat`: long copies)
    assert ctx.compress_batch_device(d, sizes, sorter, coder, lzp_hash=0, lzp_min=0) == ctx.compress_batch_device(d, sizes, sorter, coder)
    assert ctx.compress_batch_device(d, sizes, sorter, coder) == _want_blocks(sorter, coder, 0, 0)


def test_compress_batch_device_lzp_refusals(ctx, torch_cuda):
    from libbsc_amd import GpuError
    blocks = _mixed_blocks()
    d, _ = _uploaded(torch_cuda, "mixed", blocks)
    with pytest.raises(GpuError) as e:
        ctx.compress_batch_device(d, B.sizes_of(blocks), 1, 1, lzp_hash=16, lzp_min=128)
    assert e.value.code == gpu.NOT_SUPPORTED


@pytest.mark.parametrize("sorter,coder", [(1, 1), (5, 3)])
def test_compress_batch_host_input_with_the_option(ctx, torch_cuda, sorter, coder):
    blocks = _mixed_blocks()
    arrs = [T for _, T in blocks]
    try:
        for h, m in LZPS + ((16, 128),):
            ctx.option_set(ctx.OPT_BATCH_DEVICE_LZP, 0)
            p0 = ctx.option_get(ctx.CNT_BATCH_LZP_PASSES)
            off = ctx.compress_batch(arrs, sorter, coder, lzp_hash=h, lzp_min=m)
            assert ctx.option_get(ctx.CNT_BATCH_LZP_PASSES) == p0, "off: host LZP"
            if h <= 15:
                assert off == _want_blocks(sorter, coder, h, m)
            ctx.option_set(ctx.OPT_BATCH_DEVICE_LZP, 1)
            d0 = ctx.option_get(ctx.CNT_LZP_DECLINED)
            on = ctx.compress_batch(arrs, sorter, coder, lzp_hash=h, lzp_min=m)
            assert on == off, (sorter, coder, h, m)
            if h <= 15:
                assert ctx.option_get(ctx.CNT_BATCH_LZP_PASSES) > p0
                assert ctx.option_get(ctx.CNT_LZP_DECLINED) == d0
            else:
                assert ctx.option_get(ctx.CNT_BATCH_LZP_PASSES) == p0 and ctx.option_get(ctx.CNT_LZP_DECLINED) > d0
    finally:
        ctx.option_set(ctx.OPT_BATCH_DEVICE_LZP, 0)


def test_modelled_pass_is_fed_the_same_way(ctx, torch_cuda, monkeypatch):
    """-e1 with the front end and the static coder's model of a pass on: the stage's output in dL is what the host route uploads"""
    monkeypatch.setenv("BSC_BATCH_MODEL_MIN_PASS", "0")
    blocks = _mixed_blocks()
    d, _ = _uploaded(torch_cuda, "mixed", blocks)
    old = (ctx.option_set(ctx.OPT_BATCH_FRONT, 1), ctx.option_set(ctx.OPT_BATCH_MODEL, 1))
    try:
        m0 = ctx.option_get(ctx.CNT_BATCH_MODEL_PASSES)
        assert ctx.compress_batch_device(d, B.sizes_of(blocks), 1, 1, lzp_hash=15, lzp_min=128) == _want_blocks(1, 1, 15, 128)
        assert ctx.option_get(ctx.CNT_BATCH_MODEL_PASSES) > m0, "the pass took the device model"
        ctx.option_set(ctx.OPT_BATCH_DEVICE_LZP, 1)
        assert ctx.compress_batch([T for _, T in blocks], 1, 1, lzp_hash=15, lzp_min=128) == _want_blocks(1, 1, 15, 128)
    finally:
        ctx.option_set(ctx.OPT_BATCH_DEVICE_LZP, 0)
        ctx.option_set(ctx.OPT_BATCH_FRONT, old[0]); ctx.option_set(ctx.OPT_BATCH_MODEL, old[1])
