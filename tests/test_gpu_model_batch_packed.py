"""The packed 13-bit stream of a pass on the GPU (BSCGPU_OPT_BATCH_MODEL_PACKED): the stage (bscgpu_static_pstream_batch_packed_device)
against the CPU stand-in of the layout (bscgpu_pstream_pack13_host of the stand-in's streams) byte for byte, padding included, with
poff and pbase; the void rule; the segmented stage in the packed form; and the compress-batch calls with the option on against the
same calls with every model option off, with the counters showing what ran.  The inputs' properties are proved on the CPU
(test_model_batch_packed_host.py)."""
import numpy as np
import pytest

import model_batch_inputs as mb
import model_segment_inputs as ms
import packed_batch_inputs as pb
from front_inputs import layouts_equal

pytestmark = pytest.mark.gpu

CTX_N = (16 << 20) + 4096
CALL_CTX_N = (8 << 20) + 4096
NOT_SUPPORTED, BAD_PARAMETER = -4, -1


def _ctx(max_n):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from libbsc_amd import GpuContext
    return GpuContext(0, max_n=max_n)


@pytest.fixture(scope="module")
def mctx():
    c = _ctx(CTX_N)
    yield c
    c.close()


@pytest.fixture(scope="module")
def small():
    """the 2 MiB context of the segment tests: the CPU numbers were checked against its capacity"""
    c = _ctx(ms.SMALL_CTX_N)
    assert c.option_get(c.CNT_DC_DCAP) == ms.SMALL_CTX_DCAP
    yield c
    c.close()


@pytest.fixture(scope="module")
def cctx():
    c = _ctx(CALL_CTX_N)
    yield c
    c.close()


def _same_bytes(got, want, pbase, what):
    assert got.size == want.size, f"{what}: {got.size} bytes, stand-in {want.size}"
    w = np.flatnonzero(got != want)
    if w.size:
        g = int(w[0]) // 13
        s = int(np.searchsorted(pbase, g * 8, side="right")) - 1
        raise AssertionError(f"{what}: {w.size} of {got.size} bytes differ, first at byte {int(w[0])} (group {g}, sub-block {s}, its decision "
                             f"{g * 8 - int(pbase[s])}..): {int(got[w[0]]):#x} != {int(want[w[0]]):#x}; sub-blocks touched: "
                             f"{sorted(set(np.searchsorted(pbase, w // 13 * 8, side='right') - 1))[:12]}")


def _stage(ctx, name):
    """the device's packed stream of a named pass against the stand-in's: layout, poff, pbase, every byte of the buffer"""
    import torch
    _, want, flat, _, want_poff, want_packed, want_pbase = pb.reference(name)
    fb, got, poff, pbase = ctx.static_pstream_batch_packed(torch.from_numpy(flat.copy()).cuda(), want.sizes)     # raises GpuError(-4): declined or void
    assert ctx.option_get(ctx.CNT_DC_LAST_FAIL) == 0
    bad = layouts_equal(fb, want)
    assert not bad, "; ".join(bad)
    assert np.array_equal(poff, want_poff), f"poff: first difference at sub-block {int(np.flatnonzero(poff != want_poff)[0])}"
    assert np.array_equal(pbase, want_pbase), f"pbase: first difference at sub-block {int(np.flatnonzero(pbase != want_pbase)[0])}"
    _same_bytes(got, want_packed, want_pbase, name)
    return fb


# ---- 1. the stage against the stand-in ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["boundary", "mixed", "pass_of_4096", "chain_identity", "long_chain"])
def test_stage_matches_stand_in(mctx, name):
    fb = _stage(mctx, name)
    assert fb.nsub >= 5


def test_stage_pass_that_fills_max_n():
    c = _ctx(2 << 20)
    try:
        a0 = c.arena_bytes
        _stage(c, "fill")
        assert c.arena_bytes >= a0 + 2 * 4 * 8192, "the pad / pbase tables are counted with the batch tables, from first use"
    finally:
        c.close()


def test_void_pass_is_refused_packed_and_served_in_16_bits(mctx):
    import torch
    from libbsc_amd.gpu import GpuError
    _, want, flat, want_ps, want_poff, _, _ = pb.reference("void")
    d = torch.from_numpy(flat.copy()).cuda()
    with pytest.raises(GpuError) as e:
        mctx.static_pstream_batch_packed(d, want.sizes)
    assert e.value.code == NOT_SUPPORTED and mctx.option_get(mctx.CNT_DC_LAST_FAIL) == 0, "void, not declined: no reason flag"
    _, ps, poff = mctx.static_pstream_batch(d, want.sizes)
    assert np.array_equal(poff, want_poff) and np.array_equal(ps, want_ps)


def test_stage_counts_above_cap_and_bad_arguments(mctx):
    import ctypes as C
    import torch
    from libbsc_amd import _native as N
    from libbsc_amd.gpu import FrontBatch, GpuError
    _, want, flat, _, want_poff, want_packed, want_pbase = pb.reference("boundary")
    d = torch.from_numpy(flat.copy()).cuda()
    fb = FrontBatch(want.sizes)
    out = np.full(4096, 0xa5, np.uint8)
    poff, pbase = np.zeros(2 * fb.count + 2, np.uint32), np.zeros(2 * fb.count + 2, np.int64)
    f, p = mctx.L.bscgpu_static_pstream_batch_packed_device, N.np_ptr
    D = f(mctx.h, d.data_ptr(), p(fb.sizes), fb.count, C.byref(fb.lay), p(out), 4096, p(poff), p(pbase))
    assert D == int(want_poff[-1]) and want_packed.size > 4096, "too small: counted, not copied"
    assert (out == 0xa5).all() and np.array_equal(poff[:fb.nsub + 1], want_poff) and np.array_equal(pbase[:fb.nsub + 1], want_pbase)
    assert f(mctx.h, d.data_ptr(), p(fb.sizes), fb.count, C.byref(fb.lay), p(out), 4096, p(poff), None) == BAD_PARAMETER
    assert f(mctx.h, d.data_ptr(), p(fb.sizes), fb.count, C.byref(fb.lay), p(out), 4096, None, p(pbase)) == BAD_PARAMETER
    assert f(None, d.data_ptr(), p(fb.sizes), fb.count, C.byref(fb.lay), p(out), 4096, p(poff), p(pbase)) == BAD_PARAMETER
    with pytest.raises(GpuError) as e:
        mctx.pstream_batch_segments_packed(d, want.sizes, coder=3)
    assert e.value.code == BAD_PARAMETER, "the packed form is the static coder's"


# ---- 2. the segmented stage in the packed form ------------------------------------------------------------------------------------------
def _packed_counters(ctx):
    return ctx.option_get(ctx.CNT_BATCH_PACKED_PASSES), ctx.option_get(ctx.CNT_BATCH_PACKED_VOID)


def _segmented(ctx, flat, want, want_ps, want_poff, target=0, cap_bytes=None):
    """the segmented packed stage against the stand-in's streams of the blocks it kept, packed by the stand-in of the layout"""
    import torch
    c0 = _packed_counters(ctx)
    fb, got, poff, pbase, state = ctx.pstream_batch_segments_packed(torch.from_numpy(flat.copy()).cuda(), want.sizes, 1, target, cap_bytes)
    moved = tuple(b - a for a, b in zip(c0, _packed_counters(ctx)))
    bad = layouts_equal(fb, want)
    assert not bad, "; ".join(bad)
    e_bytes, e_poff, e_pbase = pb.expected_packed(want, want_ps, want_poff, state)
    assert np.array_equal(poff, e_poff), f"poff: first difference at sub-block {int(np.flatnonzero(poff != e_poff)[0])}"
    assert np.array_equal(pbase, e_pbase), f"pbase: first difference at sub-block {int(np.flatnonzero(pbase != e_pbase)[0])}"
    _same_bytes(got, e_bytes, e_pbase, "segments")
    reasons = 0
    for x in state:
        reasons |= int(x)
    assert ctx.option_get(ctx.CNT_DC_LAST_FAIL) == reasons
    return state, moved


@pytest.mark.parametrize("name", ["over_capacity", "noise_under"])
def test_segments_land_packed_where_16_bit_entries_do_not_fit(small, name):
    """A pass above the 2 MiB context's capacity as a whole: two segments, pbase running on across them.  Then the landing space: a
    byte capacity between the packed form's 13 / 8 bytes per decision (plus padding) and the 16-bit form's 2 — computed from the
    stand-in — takes the whole pass packed, every block kept, while the same bytes as 16-bit entries (cap_bytes / 2 of them) cannot
    take it: that stage counts and delivers nothing, so its caller is left with the host model."""
    import torch
    from libbsc_amd.gpu import GpuError
    _, want, flat, want_ps, want_poff = ms.reference(name, ms.STATIC)
    D = int(want_poff[-1])
    packed_bytes = int(pb.pbase_rule(want_poff)[-1]) // 8 * 13
    assert D > ms.SMALL_CTX_DCAP and packed_bytes < 2 * D
    cap_bytes = (packed_bytes + 2 * D) // 2
    assert 13 * D // 8 <= packed_bytes <= cap_bytes < 2 * D
    state, moved = _segmented(small, flat, want, want_ps, want_poff, cap_bytes=cap_bytes)
    assert not state.any() and moved == (2, 0), "two segments, both packed, every block kept"
    with pytest.raises(GpuError) as e:
        small.pstream_batch_segments(torch.from_numpy(flat.copy()).cuda(), want.sizes, 1, 0, cap_bytes // 2)
    assert e.value.code == -2, "the 16-bit entries of the pass exceed the same bytes"


def test_segments_cut_between_boundary_blocks(mctx):
    """a target of a tenth of the small blocks' decisions: at least ten cuts among blocks of a handful of runs, segments that begin
    and end inside one wavefront's 64 runs (the two text blocks are above the target: segments of their own)"""
    _, want, flat, want_ps, want_poff, _, _ = pb.reference("boundary")
    per_block = ms.block_counts(want, np.diff(want_poff.astype(np.int64)))
    target = int(per_block[1:-1].sum()) // 10
    assert per_block[1:-1].max() < target < min(per_block[0], per_block[-1])
    state, moved = _segmented(mctx, flat, want, want_ps, want_poff, target=target)
    assert not state.any() and moved[0] >= 12 and moved[1] == 0


def test_void_segment_is_packed_into_place(mctx):
    """target: each block a segment of its own.  The long-run block's packed form is void; its segment comes down as 16-bit entries and
    is packed on the host, so the caller still gets one form and every block keeps the device's model"""
    _, want, flat, want_ps, want_poff, _, _ = pb.reference("void")
    per_block = ms.block_counts(want, np.diff(want_poff.astype(np.int64)))
    state, moved = _segmented(mctx, flat, want, want_ps, want_poff, target=int(per_block.max()))
    assert not state.any() and moved[1] >= 1 and moved[0] >= 1


# ---- 3. whole calls -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(autouse=True)
def every_pass_size_goes_to_the_model(monkeypatch):
    monkeypatch.setenv("BSC_BATCH_MODEL_MIN_PASS", "0")


def _call(ctx, fn, model=0, packed=0, segments=0, device_rc=0, fast=0):
    """fn() with the options set -> (its result, packed passes, void passes, model passes it counted)"""
    keys = [(ctx.OPT_BATCH_MODEL, model), (ctx.OPT_BATCH_MODEL_PACKED, packed), (ctx.OPT_BATCH_MODEL_SEGMENTS, segments),
            (ctx.OPT_DEVICE_RC, device_rc), (ctx.OPT_BATCH_MODEL_FAST, fast)]
    old = [ctx.option_set(k, v) for k, v in keys]
    try:
        c0 = _packed_counters(ctx) + (ctx.option_get(ctx.CNT_BATCH_MODEL_PASSES),)
        out = fn()
        c1 = _packed_counters(ctx) + (ctx.option_get(ctx.CNT_BATCH_MODEL_PASSES),)
        return (out,) + tuple(b - a for a, b in zip(c0, c1))
    finally:
        for (k, _), v in zip(keys, old):
            ctx.option_set(k, v)


ROUTES = [dict(model=1, packed=1), dict(model=1, packed=1, segments=1), dict(model=1, packed=1, device_rc=1)]


@pytest.mark.parametrize("kind,sorter", sorted(mb.WHOLE_SEEDS))
def test_compress_batch_packed_equals_option_off(cctx, kind, sorter):
    import torch
    cases = mb.whole_call_cases(mb.WHOLE_SEEDS[kind, sorter])
    if kind == "device":
        flat, sizes = torch.from_numpy(np.concatenate(cases)).cuda(), [c.size for c in cases]
        fn = lambda: cctx.compress_batch_device(flat, sizes, sorter, 1)
    else:
        fn = lambda: cctx.compress_batch(cases, sorter, 1)
    off, p, v, m = _call(cctx, fn)
    assert (p, v, m) == (0, 0, 0)
    for route in ROUTES:
        on, p, v, m = _call(cctx, fn, **route)
        assert p > 0 and v == 0 and m > 0, f"{route}: {p} packed, {v} void, {m} model passes"
        assert on == off, f"{route}: bytes differ from the option-off call"


@pytest.mark.parametrize("sorter", [1, 5])
def test_compress_batch_void_pass_goes_down_as_16_bit_entries(cctx, ref, sorter):
    """the void text first in the call (so that its transform's first 64 runs are one wavefront's): the pass, or its segment, is void"""
    cases = [pb.void_text()] + mb.whole_call_cases(mb.WHOLE_SEEDS["host", sorter])
    fn = lambda: cctx.compress_batch(cases, sorter, 1)
    off, _, _, _ = _call(cctx, fn)
    assert off[0] == ref.compress(cases[0], sorter, 1)
    for route in ROUTES:
        on, p, v, m = _call(cctx, fn, **route)
        assert v > 0 and m > 0, f"{route}: {p} packed, {v} void, {m} model passes"
        assert on == off, f"{route}: bytes differ from the option-off call"


def test_fast_coder_is_not_affected(cctx):
    cases = mb.whole_call_cases(mb.WHOLE_SEEDS["host", 1])
    fn = lambda: cctx.compress_batch(cases, 1, 3)
    off, _, _, _ = _call(cctx, fn)
    for route in (dict(model=1, packed=1, fast=1), dict(model=1, packed=1, fast=1, segments=1)):
        on, p, v, _ = _call(cctx, fn, **route)
        assert (p, v) == (0, 0) and on == off


def test_option(cctx):
    assert cctx.option_get(cctx.OPT_BATCH_MODEL_PACKED) == 0, "off by default"
    with pytest.raises(Exception):
        cctx.option_set(cctx.OPT_BATCH_MODEL_PACKED, 2)
    with pytest.raises(Exception):
        cctx.option_set(cctx.CNT_BATCH_PACKED_PASSES, 0)
    cases = mb.whole_call_cases(mb.WHOLE_SEEDS["host", 1])
    _, p, v, m = _call(cctx, lambda: cctx.compress_batch(cases, 1, 1), model=0, packed=1)
    assert (p, v, m) == (0, 0, 0), "without BSCGPU_OPT_BATCH_MODEL the option does nothing"
