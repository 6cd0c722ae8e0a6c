"""The static coder's model (-e1) of a whole pass on the GPU: the stage (bscgpu_static_pstream_batch_device) against its CPU stand-in
(bscgpu_static_pstream_host) entry for entry and poff for poff, the exits with the pass as the unit, and the compress-batch calls
with BSCGPU_OPT_BATCH_MODEL on and off against the compiled reference block for block, with the route counters showing which ran.
Every pass that is not a decline case asserts that the device kept it (the stage raises otherwise)."""
import numpy as np
import pytest

import model_batch_inputs as mb
from front_inputs import KI, layouts_equal

pytestmark = pytest.mark.gpu

MIB = 1 << 20
CTX_N = (16 << 20) + 4096
NOT_SUPPORTED = -4


@pytest.fixture(scope="module")
def mctx():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from libbsc_amd import GpuContext
    c = GpuContext(0, max_n=CTX_N)
    yield c
    c.close()


def _stage(ctx, blocks, lead=0):
    """the device's stream of the pass, checked against the stand-in's: layout, poff, every entry"""
    import torch
    want, flat = mb.layout(blocks)
    want_ps, want_poff = mb.host_streams(want)
    d = torch.from_numpy(np.concatenate([np.zeros(lead, np.uint8), flat])).cuda()
    fb, ps, poff = ctx.static_pstream_batch(d[lead:], [b.size for b in blocks])         # raises GpuError(-4) on a declined pass
    assert ctx.option_get(ctx.CNT_DC_LAST_FAIL) == 0
    bad = layouts_equal(fb, want)
    assert not bad, "; ".join(bad)
    assert np.array_equal(poff, want_poff), f"poff: first difference at sub-block {int(np.flatnonzero(poff != want_poff)[0])}"
    assert ps.size == want_ps.size
    w = np.flatnonzero(ps != want_ps)
    if w.size:
        s = int(np.searchsorted(want_poff, w[0], side="right")) - 1
        raise AssertionError(f"{w.size} of {ps.size} entries differ, first at {int(w[0])} (sub-block {s}, its decision {int(w[0]) - int(want_poff[s])}): "
                             f"{int(ps[w[0]]):#x} != {int(want_ps[w[0]]):#x}; sub-blocks touched: {sorted(set(np.searchsorted(want_poff, w, side='right') - 1))[:12]}")
    return fb, ps, poff


@pytest.mark.parametrize("lead", [0, 5])
def test_stage_matches_stand_in_on_mixed_batch(mctx, lead):
    """every size class including 1, 2, 29, 256 KiB - 1, 256 KiB and 1 MiB - 1, an empty block, the constant block (one run of 2^18)"""
    blocks = mb.mixed_batch(0)
    fb, _, _ = _stage(mctx, blocks, lead)
    assert fb.nsub > len(blocks)


def test_stage_pass_of_4096_blocks(mctx):
    fb, ps, _ = _stage(mctx, mb.pass_of_4096())
    assert fb.nsub > 4000 and ps.size > 64 * 8192, "sub-block starts in every tile, avg lane and evaluation chunk"


def test_chain_identity_is_exact(mctx):
    """a symbol, and a set of decision types, that occur in sub-blocks 3, 11, 67, 131, 259 only: an id kept modulo 8, 64 or 128 would
    walk two of their chains as one"""
    _stage(mctx, mb.chain_identity_pass())


def test_long_chains_and_replay(mctx):
    _stage(mctx, mb.long_chain_pass())
    assert mctx.option_get(mctx.CNT_DC_REPLAYS) > 0, "a chain longer than an evaluation chunk whose bracket stays open must be replayed"


@pytest.mark.parametrize("case", ["avg", "hist"])
def test_stage_declines_the_whole_pass(mctx, case):
    import torch
    from libbsc_amd.gpu import GpuError
    blocks, flag = (mb.fail_avg_pass(), mctx.DC_FAIL_AVG) if case == "avg" else (mb.fail_hist_pass(), mctx.DC_FAIL_HIST)
    d = torch.from_numpy(np.concatenate(blocks)).cuda()
    with pytest.raises(GpuError) as e:
        mctx.static_pstream_batch(d, [b.size for b in blocks])
    assert e.value.code == NOT_SUPPORTED
    assert mctx.option_get(mctx.CNT_DC_LAST_FAIL) == flag


def test_stage_pass_that_fills_max_n():
    from libbsc_amd import GpuContext
    assert sum(mb.FILL_SIZES) == 2 * MIB
    c = GpuContext(0, max_n=2 * MIB)
    try:
        a0 = c.arena_bytes
        _stage(c, mb.fill_pass())
        a1 = c.arena_bytes
        assert a1 >= a0 + 8 * 4 * 2 * MIB, "the events' sub-block ids (8 bytes per decision of capacity) are counted once allocated"
        _stage(c, mb.fill_pass()[::-1])
        assert c.arena_bytes == a1, "allocated once"
    finally:
        c.close()


def test_stage_bad_arguments(mctx):
    import ctypes as C
    import torch
    from libbsc_amd import _native as N
    from libbsc_amd.gpu import FrontBatch
    fb = FrontBatch([100, 200])
    d = torch.zeros(300, dtype=torch.uint8, device="cuda")
    out = np.zeros(4096, np.uint16)
    poff = np.zeros(8, np.uint32)
    f = mctx.L.bscgpu_static_pstream_batch_device
    assert f(mctx.h, d.data_ptr(), N.np_ptr(fb.sizes), 2, C.byref(fb.lay), N.np_ptr(out), out.size, None) == -1
    assert f(None, d.data_ptr(), N.np_ptr(fb.sizes), 2, C.byref(fb.lay), N.np_ptr(out), out.size, N.np_ptr(poff)) == -1
    assert f(mctx.h, d.data_ptr(), N.np_ptr(fb.sizes), 2, None, N.np_ptr(out), out.size, N.np_ptr(poff)) == -1
    _, want_poff = mb.host_streams(mb.layout([np.zeros(100, np.uint8), np.zeros(200, np.uint8)])[0])
    out[:] = 0xffff
    D = f(mctx.h, d.data_ptr(), N.np_ptr(fb.sizes), 2, C.byref(fb.lay), N.np_ptr(out), 1, N.np_ptr(poff))       # too small: counted, not copied
    assert D == int(want_poff[2]) and list(poff[:3]) == [int(x) for x in want_poff] and (out == 0xffff).all()


# ---- whole calls -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(autouse=True)
def every_pass_size_goes_to_the_model(monkeypatch):
    """the route's minimum pass size is 16 MiB; the whole-call tests use passes of a few MiB (the same code path: the minimum is one
    comparison in front of it), so they lift it through the library's own knob"""
    monkeypatch.setenv("BSC_BATCH_MODEL_MIN_PASS", "0")


def _counters(ctx):
    return ctx.option_get(ctx.CNT_BATCH_MODEL_PASSES), ctx.option_get(ctx.CNT_BATCH_MODEL_DECLINED)


def _with_model(ctx, value, fn):
    old = ctx.option_set(ctx.OPT_BATCH_MODEL, value)
    try:
        p0, d0 = _counters(ctx)
        out = fn()
        p1, d1 = _counters(ctx)
        return out, p1 - p0, d1 - d0
    finally:
        ctx.option_set(ctx.OPT_BATCH_MODEL, old)


@pytest.mark.parametrize("features", [3, 1])
@pytest.mark.parametrize("sorter", [1, 5])
def test_compress_batch_host_input(mctx, ref, sorter, features):
    cases = mb.whole_call_cases(mb.WHOLE_SEEDS['host', sorter])
    for lzp in ((0, 0), (15, 128)):
        want = [ref.compress(x, sorter, 1, lzp[0], lzp[1], features=features) for x in cases]
        on, p, d = _with_model(mctx, 1, lambda: mctx.compress_batch(cases, sorter, 1, lzp[0], lzp[1], features))
        assert p > 0 and d == 0, f"option on: {p} model passes, {d} declined"
        for x, blk, w in zip(cases, on, want):
            assert blk == w, f"n={x.size} sorter={sorter} lzp={lzp} features={features}"
        off, p, d = _with_model(mctx, 0, lambda: mctx.compress_batch(cases, sorter, 1, lzp[0], lzp[1], features))
        assert (p, d) == (0, 0)
        assert off == on


@pytest.mark.parametrize("sorter", [1, 5])
def test_compress_batch_device_input(mctx, ref, sorter):
    import torch
    cases = mb.whole_call_cases(mb.WHOLE_SEEDS['device', sorter])
    flat = torch.from_numpy(np.concatenate(cases)).cuda()
    sizes = [c.size for c in cases]
    on, p, d = _with_model(mctx, 1, lambda: mctx.compress_batch_device(flat, sizes, sorter, 1))
    assert p > 0 and d == 0
    for x, blk in zip(cases, on):
        assert blk == ref.compress(x, sorter, 1), f"n={x.size} sorter={sorter}"
    off, p, d = _with_model(mctx, 0, lambda: mctx.compress_batch_device(flat, sizes, sorter, 1))
    assert (p, d) == (0, 0) and off == on


@pytest.mark.parametrize("coder", [3, 2])
def test_other_coders_take_todays_route(mctx, coder):
    cases = mb.whole_call_cases(mb.WHOLE_SEEDS['host', 1])
    on, p, d = _with_model(mctx, 1, lambda: mctx.compress_batch(cases, 1, coder))
    assert (p, d) == (0, 0)
    off, _, _ = _with_model(mctx, 0, lambda: mctx.compress_batch(cases, 1, coder))
    assert on == off


@pytest.mark.parametrize("case", ["avg", "hist"])
def test_compress_batch_declined_pass(mctx, ref, case):
    """a text whose BWT trips the exit, among ordinary text: the pass is declined as a whole, every block takes the host model"""
    import devcoder_inputs as di
    from libbsc_amd.synth import synth_text_v1
    bad = di.text_with_bwt_like(di.runs_to_block(di.const_rank(40, 200_000), np.tile([1, 1, 2, 4], 50_000)) if case == "avg" else di.hist_chain(40_000))
    cases = [synth_text_v1(81, 700 * KI), bad, synth_text_v1(82, 300 * KI)]
    on, p, d = _with_model(mctx, 1, lambda: mctx.compress_batch(cases, 1, 1))
    assert (p, d) == (0, 1)
    assert mctx.option_get(mctx.CNT_DC_LAST_FAIL) == (mctx.DC_FAIL_AVG if case == "avg" else mctx.DC_FAIL_HIST)
    for x, blk in zip(cases, on):
        assert blk == ref.compress(x, 1, 1), f"n={x.size}"


def test_option_and_small_pass(mctx, monkeypatch):
    from libbsc_amd.synth import synth_text_v1
    assert mctx.option_get(mctx.OPT_BATCH_MODEL) in (0, 1)
    with pytest.raises(Exception):
        mctx.option_set(mctx.OPT_BATCH_MODEL, 2)
    with pytest.raises(Exception):
        mctx.option_set(mctx.CNT_BATCH_MODEL_PASSES, 0)
    monkeypatch.delenv("BSC_BATCH_MODEL_MIN_PASS")
    small = [synth_text_v1(1, 300 * KI), synth_text_v1(2, 900 * KI)]
    _, p, d = _with_model(mctx, 1, lambda: mctx.compress_batch(small, 1, 1))
    assert (p, d) == (0, 0), "a pass below the minimum size takes the host model"
    monkeypatch.setenv("BSC_BATCH_MODEL_MIN_PASS", str(1 << 20))
    _, p, d = _with_model(mctx, 1, lambda: mctx.compress_batch(small, 1, 1))
    assert (p, d) == (1, 0)


@pytest.mark.parametrize("features", [3, 1])
def test_device_range_coder_codes_a_model_pass(mctx, ref, features):
    """BSCGPU_OPT_DEVICE_RC = 1: the pass's streams through one launch of the device's range coder; identical bytes, counted"""
    cases = mb.whole_call_cases(mb.WHOLE_SEEDS['host', 1])
    plain, p, d = _with_model(mctx, 1, lambda: mctx.compress_batch(cases, 1, 1, 0, 0, features))
    assert p > 0 and d == 0
    old = mctx.option_set(mctx.OPT_DEVICE_RC, 1)
    try:
        n0 = mctx.option_get(mctx.CNT_DEVICE_RC_BLOCKS)
        got, p, d = _with_model(mctx, 1, lambda: mctx.compress_batch(cases, 1, 1, 0, 0, features))
        assert p > 0 and d == 0 and mctx.option_get(mctx.CNT_DEVICE_RC_BLOCKS) == n0 + p
    finally:
        mctx.option_set(mctx.OPT_DEVICE_RC, old)
    assert got == plain
    for x, blk in zip(cases, got):
        assert blk == ref.compress(x, 1, 1, features=features), f"n={x.size}"
