"""The QLFC front end of a whole pass on the GPU: the stage (bscgpu_qlfc_front_batch_device) against its CPU stand-in
(bscgpu_front_batch_host) array for array, and the compress-batch calls with BSCGPU_OPT_BATCH_FRONT on and off against the compiled
reference block for block, with the route counters showing which route ran."""
import numpy as np
import pytest

from front_inputs import KI, layouts_equal, mixed_batch, runs_block

pytestmark = pytest.mark.gpu

MIB = 1 << 20
CTX_N = (16 << 20) + 4096


@pytest.fixture(scope="module")
def fctx():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from libbsc_amd import GpuContext
    c = GpuContext(0, max_n=CTX_N)
    yield c
    c.close()


def _stage(ctx, blocks, lead=0):
    import torch
    from libbsc_amd.gpu import front_batch_host
    sizes = [b.size for b in blocks]
    flat = np.concatenate(blocks) if sum(sizes) else np.zeros(1, np.uint8)
    want = front_batch_host(flat, sizes)
    d = torch.from_numpy(np.concatenate([np.zeros(lead, np.uint8), flat])).cuda()
    got = ctx.qlfc_front_batch(d[lead:], sizes)
    bad = layouts_equal(got, want)
    assert not bad, "; ".join(bad)
    return got


@pytest.mark.parametrize("lead", [0, 5])
def test_stage_matches_host_on_mixed_batch(fctx, lead):
    """every size class with every alphabet, the equal-split blocks, an empty block; lead: a pass that starts anywhere in a tensor"""
    blocks = mixed_batch(0)
    got = _stage(fctx, blocks, lead)
    assert got.nsub > len(blocks), "blocks of 256 KiB and more have two sub-blocks"


def test_stage_pass_of_4096_blocks(fctx):
    rng = np.random.default_rng(11)
    sizes = rng.integers(0, 3000, 4096)
    sizes[::512] = 300 * KI                                     # a few with two sub-blocks among them
    text = runs_block(rng, int(sizes.sum()), 40, mean_run=2.5)
    offs = np.concatenate([[0], np.cumsum(sizes)])
    _stage(fctx, [text[offs[b]:offs[b + 1]] for b in range(4096)])


def test_stage_pass_that_fills_max_n():
    from libbsc_amd import GpuContext
    rng = np.random.default_rng(12)
    cap = 2 * MIB
    sizes = [700 * KI, 0, 700 * KI - 3, cap - 1400 * KI + 3]
    assert sum(sizes) == cap
    c = GpuContext(0, max_n=cap)
    try:
        _stage(c, [runs_block(rng, n, 70, mean_run=1.5) for n in sizes])
        import torch
        sz = np.array([700 * KI, 700 * KI, 700 * KI], np.int32)   # over max_n: refused, nothing run
        from libbsc_amd.gpu import GpuError
        with pytest.raises(GpuError):
            c.qlfc_front_batch(torch.zeros(int(sz.sum()), dtype=torch.uint8, device="cuda"), sz)
    finally:
        c.close()


def test_stage_tiles_straddling_many_sub_block_ends(fctx):
    """hundreds of 1..300-byte blocks: every 4096-byte tile holds dozens of forced heads, every 256-run tile several sub-block ends"""
    rng = np.random.default_rng(13)
    sizes = rng.integers(1, 301, 900)
    sizes[:40] = 1
    blocks = [runs_block(rng, int(n), int(rng.integers(1, 20)), mean_run=float(rng.uniform(1.0, 9.0))) for n in sizes]
    blocks += [np.full(int(n), 5, np.uint8) for n in rng.integers(1, 40, 100)]       # neighbours with the same byte: only the forced head separates them
    order = rng.permutation(len(blocks))
    _stage(fctx, [blocks[i] for i in order])


@pytest.mark.parametrize("K", [2, 17, 32, 33, 48, 64, 65, 200])
def test_stage_rank_set_layouts_on_skewed_alphabets(fctx, K):
    """qf_rank's three set layouts (32-bit sets, one 64-bit word, four words) at batch sizes: frequent symbols come back inside the lifted
    tile, middling ones inside the halo, the rarest only after tens of thousands of runs (tile and super-tile sets, the serial tail) or
    never before the sub-block ends; the pass's union alphabet picks the layout"""
    rng = np.random.default_rng(1000 + K)
    p = 1.0 / np.arange(1, K + 1) ** 1.6
    p /= p.sum()
    n = 3 * MIB
    T = rng.choice(K, size=n // 3 + 1, p=p).astype(np.uint8)
    T = np.repeat(T, 3)[:n].copy()
    T[::97] = K - 1
    T[n // 2:n // 2 + 300 * KI:2] = 0                              # a stretch where the rare symbols stay away for > 65536 runs
    T[n // 2 + 1:n // 2 + 300 * KI:2] = 1 % K
    T = rng.permutation(256)[:K].astype(np.uint8)[T]
    sizes = [900 * KI, 100, 260 * KI, 64 * KI, 1000 * KI, 5, 0, 300 * KI]
    sizes.append(n - sum(sizes))
    assert 0 < sizes[-1] < MIB
    offs = np.concatenate([[0], np.cumsum(sizes)])
    got = _stage(fctx, [T[offs[b]:offs[b + 1]] for b in range(len(sizes))])
    assert int(np.diff(got.sub_run.astype(np.int64)).max()) > 65536 or K == 2


# ---- whole calls -----------------------------------------------------------------------------------------------------------------
def _cases(rng):
    from libbsc_amd.synth import synth_text_v1
    cases = [synth_text_v1(21 + i, int(n)) for i, n in enumerate(rng.integers(1000, 200000, 8))]
    cases += [synth_text_v1(41, 300 * KI), synth_text_v1(42, 256 * KI), synth_text_v1(43, MIB - 1)]          # two sub-blocks
    cases += [np.concatenate([synth_text_v1(44, 500 * KI), rng.integers(0, 256, 120 * KI, dtype=np.uint8)])]
    cases += [rng.integers(0, 256, n, dtype=np.uint8) for n in (5000, 70000, 300 * KI)]                      # stored
    cases += [np.frombuffer(bytes(range(40)) * 2, np.uint8)[:n].copy() for n in (1, 27, 28, 29, 30)]
    cases += [np.zeros(0, np.uint8), np.zeros(100, np.uint8), np.zeros(3000, np.uint8), synth_text_v1(5, 65536), synth_text_v1(6, 65535)]
    return cases


def _want(ref, data, sorter, coder, lzp=(0, 0)):
    """the compiled reference's block; ST7 / ST8, which its CPU build does not encode (LIBBSC_NOT_SUPPORTED): this library's single-block
    bsc_compress, and the reference must decode it (the rule of tests/test_gpu_st_batch.py)"""
    if sorter <= 6:
        return ref.compress(data, sorter, coder, lzp[0], lzp[1])
    from libbsc_amd import api
    blk = api.bsc_compress(data, sorter, coder, lzp[0], lzp[1])
    if isinstance(blk, int):
        return blk
    blk = bytes(blk)
    assert ref.decompress(blk) == data.tobytes(), f"n={data.size} sorter={sorter}: the reference does not decode the single-block path's block"
    return blk


def _plan(cases, sorter, cap=CTX_N):
    from libbsc_amd.gpu import batch_plan, st_batch_plan
    sizes = [c.size for c in cases]
    return (batch_plan(sizes, sorter, cap) if sorter == 1 else st_batch_plan(sizes, sorter, cap))[0]


def _counters(ctx):
    return ctx.option_get(ctx.CNT_BATCH_FRONT_PASSES), ctx.option_get(ctx.CNT_BATCH_L_PASSES)


def _with_option(ctx, value, fn):
    old = ctx.option_set(ctx.OPT_BATCH_FRONT, value)
    try:
        f0, l0 = _counters(ctx)
        out = fn()
        f1, l1 = _counters(ctx)
        return out, f1 - f0, l1 - l0
    finally:
        ctx.option_set(ctx.OPT_BATCH_FRONT, old)


@pytest.mark.parametrize("coder", [1, 2, 3])
@pytest.mark.parametrize("sorter", [1, 5, 8])
def test_compress_batch_host_input(fctx, ref, sorter, coder):
    rng = np.random.default_rng(7 * sorter + coder)
    cases = _cases(rng)
    passes = _plan(cases, sorter)
    assert passes >= 1
    for lzp in ((0, 0), (15, 128)):
        on, f, l = _with_option(fctx, 1, lambda: fctx.compress_batch(cases, sorter, coder, lzp[0], lzp[1], 3))
        assert (f, l) == (passes, 0), f"option on: {f} front passes, {l} L passes, planned {passes}"
        for data, blk in zip(cases, on):
            assert blk == _want(ref, data, sorter, coder, lzp), f"n={data.size} sorter={sorter} coder={coder} lzp={lzp}"
        off, f, l = _with_option(fctx, 0, lambda: fctx.compress_batch(cases, sorter, coder, lzp[0], lzp[1], 3))
        assert (f, l) == (0, passes), f"option off: {f} front passes, {l} L passes, planned {passes}"
        assert off == on


@pytest.mark.parametrize("sorter", [1, 5, 8])
def test_compress_batch_device_input(fctx, ref, sorter):
    import torch
    rng = np.random.default_rng(50 + sorter)
    cases = _cases(rng)
    passes = _plan(cases, sorter)
    flat = torch.from_numpy(np.concatenate(cases)).cuda()
    sizes = [c.size for c in cases]
    for coder in (1, 2, 3):
        on, f, l = _with_option(fctx, 1, lambda: fctx.compress_batch_device(flat, sizes, sorter, coder))
        assert (f, l) == (passes, 0)
        for data, blk in zip(cases, on):
            assert blk == _want(ref, data, sorter, coder), f"n={data.size} sorter={sorter} coder={coder}"
        off, f, l = _with_option(fctx, 0, lambda: fctx.compress_batch_device(flat, sizes, sorter, coder))
        assert (f, l) == (0, passes)
        assert off == on


def test_features_without_multithreading(fctx, ref):
    """the serial framing rule (coder.cpp:111-155) through coder_compress_views: LIBBSC_FEATURE_FASTMODE alone"""
    rng = np.random.default_rng(77)
    cases = _cases(rng)
    on, f, _ = _with_option(fctx, 1, lambda: fctx.compress_batch(cases, 1, 1, 0, 0, 1))
    assert f >= 1
    for data, blk in zip(cases, on):
        assert blk == ref.compress(data, 1, 1, features=1), f"n={data.size}"


def test_mixed_routes(fctx, ref):
    """blocks of 1 MiB and more (single path) between pass members, empty and <= 28-byte blocks, an LZP output too short for the sorter"""
    import torch
    from libbsc_amd.synth import synth_text_v1
    cases = [synth_text_v1(31, 50000), synth_text_v1(32, MIB - 1), synth_text_v1(33, MIB), np.zeros(0, np.uint8), synth_text_v1(34, 3 * MIB // 2),
             synth_text_v1(35, 1000), np.zeros(10, np.uint8), synth_text_v1(36, 400 * KI), np.zeros(28, np.uint8), np.zeros(2000, np.uint8)]
    for sorter in (1, 5):
        passes = _plan(cases, sorter)
        for lzp in ((0, 0), (15, 128)):
            on, f, l = _with_option(fctx, 1, lambda: fctx.compress_batch(cases, sorter, 1, lzp[0], lzp[1]))
            assert (f, l) == (passes, 0)
            for data, blk in zip(cases, on):
                assert blk == ref.compress(data, sorter, 1, lzp[0], lzp[1]), f"sorter={sorter} n={data.size} lzp={lzp}"
        flat = torch.from_numpy(np.concatenate(cases)).cuda()
        got_d, f, l = _with_option(fctx, 1, lambda: fctx.compress_batch_device(flat, [c.size for c in cases], sorter, 1))
        assert (f, l) == (passes, 0)
        for data, blk in zip(cases, got_d):
            assert blk == ref.compress(data, sorter, 1), f"device input: sorter={sorter} n={data.size}"


def test_several_passes(ref):
    """total > max_n: many passes through the two pinned run buffers, the coding of pass k beside the sort of pass k + 1"""
    import torch
    from libbsc_amd import GpuContext
    from libbsc_amd.synth import synth_text_v1
    rng = np.random.default_rng(99)
    sizes = [int(x) for x in rng.integers(1, 24000, 1500)]
    for k in range(0, 1500, 100):
        sizes[k] = 300 * KI + k
    text = synth_text_v1(77, sum(sizes))
    offs = np.concatenate([[0], np.cumsum(sizes)])
    cases = [text[offs[b]:offs[b + 1]].copy() for b in range(len(sizes))]
    cap = 4 << 20
    c = GpuContext(0, max_n=cap)
    try:
        passes = _plan(cases, 1, cap)
        assert passes >= 5
        on, f, l = _with_option(c, 1, lambda: c.compress_batch(cases, 1, 1))
        assert (f, l) == (passes, 0)
        arena_on = c.arena_bytes
        off, f, l = _with_option(c, 0, lambda: c.compress_batch(cases, 1, 1))
        assert (f, l) == (0, passes)
        assert on == off
        dT = torch.from_numpy(text).cuda()
        on_d, f, l = _with_option(c, 1, lambda: c.compress_batch_device(dT, sizes, 1, 1))
        assert (f, l) == (passes, 0)
        assert on_d == on
        for b in list(range(0, len(cases), 37)) + list(range(0, 1500, 100)):
            assert on[b] == ref.compress(cases[b], 1, 1), f"block {b}"
        assert c.arena_bytes == arena_on, "the front end's tables are allocated once"
    finally:
        c.close()


def test_option_and_arena(ref):
    from libbsc_amd import GpuContext
    from libbsc_amd.synth import synth_text_v1
    c = GpuContext(0, max_n=1 << 20)
    try:
        assert c.option_get(c.OPT_BATCH_FRONT) in (0, 1)
        a0 = c.arena_bytes
        c.option_set(c.OPT_BATCH_FRONT, 1)
        assert c.option_set(c.OPT_BATCH_FRONT, 0) == 1 and c.option_get(c.OPT_BATCH_FRONT) == 0
        with pytest.raises(Exception):
            c.option_set(c.OPT_BATCH_FRONT, 2)
        with pytest.raises(Exception):
            c.option_set(c.CNT_BATCH_FRONT_PASSES, 0)
        c.option_set(c.OPT_BATCH_FRONT, 1)
        c.compress_batch([synth_text_v1(1, 5000)], 1, 1)
        assert c.arena_bytes > a0 + (8 << 20), "the sub-block and first-run tables are counted once allocated"
    finally:
        c.close()
