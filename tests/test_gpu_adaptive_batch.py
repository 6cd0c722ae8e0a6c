"""The adaptive coder's model (-e2) of a whole pass on the GPU: the stage (bscgpu_adaptive_pstream_batch_device) against its CPU stand-in
(bscgpu_adaptive_pstream_host) entry for entry and poff for poff — with both sets of debug planes, so that a mismatch says whether a
counter value, the mixer id or the mixed probability differs first —, the capacity and the chain-cap exits with the pass as the unit,
and the compress-batch calls with BSCGPU_OPT_BATCH_MODEL_ADAPTIVE on and off against the compiled reference block for block, with
the route's own counters showing which ran.  Every pass that is not a decline case asserts that the device kept it."""
import ctypes as C

import numpy as np
import pytest

import adaptive_batch_inputs as ab
import fast_batch_inputs as fbi
import model_batch_inputs as mb
from front_inputs import KI, layouts_equal

pytestmark = pytest.mark.gpu

MIB = 1 << 20
NOT_SUPPORTED = -4


@pytest.fixture(scope="module")
def actx():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from libbsc_amd import GpuContext
    c = GpuContext(0, max_n=ab.CTX_N)
    yield c
    c.close()


@pytest.fixture(scope="module")
def wctx():
    """the whole-call tests' context.  Their cases hold a block of 1 MiB - 1 bytes of text: sub-blocks of 512 KiB whose longest mixer
    chain, about a fifth of 1.6 M decisions, is above the default step cap of 1 << 18 — a pass the default declines, because the host is
    the faster one there.  What these tests check is the route (the same bytes, the counters), so the context lifts the cap through the
    library's own knob, read at creation, as the tests lift the route's minimum pass."""
    import os
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from libbsc_amd import GpuContext
    old = os.environ.get("BSC_DC_MIX_CHAIN_CAP")
    os.environ["BSC_DC_MIX_CHAIN_CAP"] = str(1 << 20)
    try:
        c = GpuContext(0, max_n=ab.CTX_N)
    finally:
        if old is None:
            del os.environ["BSC_DC_MIX_CHAIN_CAP"]
        else:
            os.environ["BSC_DC_MIX_CHAIN_CAP"] = old
    yield c
    c.close()


def _stage(ctx, name, lead=0, order=1):
    """the device's stream of the pass, checked against the stand-in's: layout, poff, every entry, every debug plane"""
    import torch
    blocks, want, want_ps, want_poff, want_dbg = ab.reference(name)
    if order < 0:
        blocks = blocks[::-1]
        want, _ = mb.layout(blocks)
        want_ps, want_poff, want_dbg = ab.host_streams(want, dbg=True)
    flat = np.concatenate(blocks)
    d = torch.from_numpy(np.concatenate([np.zeros(lead, np.uint8), flat])).cuda()
    fb, ps, poff, dbg = ctx.adaptive_pstream_batch(d[lead:], [b.size for b in blocks], dbg=True)      # raises GpuError(-4) on a declined pass
    assert ctx.option_get(ctx.CNT_DC_LAST_FAIL) == 0
    bad = layouts_equal(fb, want)
    assert not bad, "; ".join(bad)
    assert np.array_equal(poff, want_poff), f"poff: first difference at sub-block {int(np.flatnonzero(poff != want_poff)[0])}"
    assert ps.size == want_ps.size
    msg = ab.first_difference(ps, want_ps, want_poff, dbg, want_dbg)
    assert msg is None, msg
    for p in range(4):
        w = np.flatnonzero(dbg[p] != want_dbg[p])
        assert not w.size, f"{ab.PLANES[p]}: {w.size} differ, first at {int(w[0])}: {int(dbg[p][w[0]])} != {int(want_dbg[p][w[0]])}"
    return fb, ps, poff, dbg


@pytest.mark.parametrize("lead", [0, 5])
def test_stage_matches_stand_in_on_mixed_batch(actx, lead):
    """every size class including 1, 2, 29, 256 KiB - 1, 256 KiB and 1 MiB - 1, an empty block, the constant block; lead 5: an
    unaligned device pointer"""
    fb, ps, _, dbg = _stage(actx, "mixed", lead)
    assert fb.nsub > fb.count
    chains = actx.option_get(actx.CNT_DC_MIX_CHAINS)
    sub = np.repeat(np.arange(fb.nsub, dtype=np.int64), np.diff(ab.reference("mixed")[3].astype(np.int64)))
    ids, counts = np.unique(sub << 11 | dbg[3].astype(np.int64), return_counts=True)
    assert chains == ids.size and actx.option_get(actx.CNT_DC_MIX_LONGEST) == int(counts.max())


def test_stage_pass_of_4096_blocks(actx):
    fb, ps, _, _ = _stage(actx, "pass_of_4096")
    assert fb.nsub > 4000 and ps.size > 64 * 8192, "13 bits of sub-block in the chain key"


def test_chain_identity_is_exact(actx):
    """the same mixer id in neighbouring sub-blocks must be separate chains"""
    _stage(actx, "chain_identity")


def test_run_hist_above_the_static_clamp(actx):
    _, _, _, dbg = _stage(actx, "hist_above_clamp")
    assert ab.run_exp_rows(dbg[3]).max() > 7


def test_escape_mixers(actx):
    _stage(actx, "escape")


def test_tiny_alphabets(actx):
    _stage(actx, "tiny_alphabets")


def test_stage_pass_that_fills_max_n():
    from libbsc_amd import GpuContext
    assert sum(mb.FILL_SIZES) == 2 * MIB
    c = GpuContext(0, max_n=2 * MIB)
    try:
        a0 = c.arena_bytes
        _stage(c, "fill")
        a1 = c.arena_bytes
        assert a1 >= a0 + (8 + 24) * 4 * 2 * MIB, "the batch model's arena and the adaptive stage's (24 bytes per decision) are counted once allocated"
        _stage(c, "fill", order=-1)
        assert c.arena_bytes == a1, "allocated once"
    finally:
        c.close()


def _raw_call(c, blocks, cap=16):
    import torch
    from libbsc_amd import _native as N
    from libbsc_amd.gpu import FrontBatch
    flat = np.concatenate(blocks)
    d = torch.from_numpy(flat).cuda()
    fb = FrontBatch([b.size for b in blocks])
    out = np.zeros(cap, np.uint16)
    poff = np.zeros(2 * len(blocks) + 2, np.uint32)
    r = c.L.bscgpu_adaptive_pstream_batch_device(c.h, d.data_ptr(), N.np_ptr(fb.sizes), fb.count, C.byref(fb.lay), N.np_ptr(out), out.size, N.np_ptr(poff), None)
    return r, fb, out, poff


def _declined_pass_still_codes(fb, blocks, want, ref):
    bad = layouts_equal(fb, want)
    assert not bad, "a declined pass still fills the layout: " + "; ".join(bad)
    for b, a in enumerate(blocks):
        if a.size:
            assert fb.code(b, 2) == ref.coder_compress(a, 2, 3), f"block {b} (n={a.size})"


def test_stage_declines_the_whole_pass_for_capacity(ref):
    from libbsc_amd import GpuContext
    blocks = fbi.noise_pass()
    want, _ = mb.layout(blocks)
    c = GpuContext(0, max_n=2 * MIB)
    try:
        r, fb, _, _ = _raw_call(c, blocks)
        assert r == NOT_SUPPORTED
        assert c.option_get(c.CNT_DC_LAST_FAIL) == c.DC_FAIL_CAP
        _declined_pass_still_codes(fb, blocks, want, ref)
    finally:
        c.close()


def test_stage_declines_the_whole_pass_for_the_chain_cap(ref, monkeypatch):
    from libbsc_amd import GpuContext
    blocks, want = ab.reference("mixed")[:2]
    monkeypatch.setenv("BSC_DC_MIX_CHAIN_CAP", "64")               # read when the context is created
    c = GpuContext(0, max_n=ab.CTX_N)
    try:
        r, fb, _, _ = _raw_call(c, blocks)
        assert r == NOT_SUPPORTED
        assert c.option_get(c.CNT_DC_LAST_FAIL) == c.DC_FAIL_MIX
        assert c.option_get(c.CNT_DC_MIX_LONGEST) > 64
        _declined_pass_still_codes(fb, blocks, want, ref)
    finally:
        c.close()


def test_stage_bad_arguments(actx):
    import torch
    from libbsc_amd import _native as N
    from libbsc_amd.gpu import FrontBatch
    fb = FrontBatch([100, 200])
    d = torch.zeros(300, dtype=torch.uint8, device="cuda")
    out = np.zeros(4096, np.uint16)
    poff = np.zeros(8, np.uint32)
    f = actx.L.bscgpu_adaptive_pstream_batch_device
    assert f(actx.h, d.data_ptr(), N.np_ptr(fb.sizes), 2, C.byref(fb.lay), N.np_ptr(out), out.size, None, None) == -1
    assert f(None, d.data_ptr(), N.np_ptr(fb.sizes), 2, C.byref(fb.lay), N.np_ptr(out), out.size, N.np_ptr(poff), None) == -1
    assert f(actx.h, d.data_ptr(), N.np_ptr(fb.sizes), 2, None, N.np_ptr(out), out.size, N.np_ptr(poff), None) == -1
    _, want_poff = ab.host_streams(mb.layout([np.zeros(100, np.uint8), np.zeros(200, np.uint8)])[0])
    out[:] = 0xffff
    D = f(actx.h, d.data_ptr(), N.np_ptr(fb.sizes), 2, C.byref(fb.lay), N.np_ptr(out), 1, N.np_ptr(poff), None)       # too small: counted, not copied
    assert D == int(want_poff[2]) and list(poff[:3]) == [int(x) for x in want_poff] and (out == 0xffff).all()


# ---- whole calls -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(autouse=True)
def every_pass_size_goes_to_the_model(monkeypatch):
    """the whole-call tests use passes of a few MiB, below the route's minimum (the same code path: the minimum is one comparison in
    front of it), so they lift it through the library's own knob"""
    monkeypatch.setenv("BSC_BATCH_MODEL_MIN_PASS", "0")


def _counters(ctx):
    return ctx.option_get(ctx.CNT_BATCH_ADAPTIVE_PASSES), ctx.option_get(ctx.CNT_BATCH_ADAPTIVE_DECLINED)


def _others(ctx):
    return tuple(ctx.option_get(k) for k in (ctx.CNT_BATCH_MODEL_PASSES, ctx.CNT_BATCH_MODEL_DECLINED, ctx.CNT_BATCH_FAST_PASSES, ctx.CNT_BATCH_FAST_DECLINED))


def _with_adaptive(ctx, value, fn):
    old = ctx.option_set(ctx.OPT_BATCH_MODEL_ADAPTIVE, value)
    try:
        p0, d0 = _counters(ctx)
        o0 = _others(ctx)
        out = fn()
        p1, d1 = _counters(ctx)
        assert _others(ctx) == o0, "the static and the fast route's counters do not move"
        return out, p1 - p0, d1 - d0
    finally:
        ctx.option_set(ctx.OPT_BATCH_MODEL_ADAPTIVE, old)


@pytest.mark.parametrize("sorter", [1, 5])
def test_compress_batch_host_input(wctx, ref, sorter):
    cases = mb.whole_call_cases(mb.WHOLE_SEEDS['host', sorter])
    want = [ref.compress(x, sorter, 2) for x in cases]
    on, p, d = _with_adaptive(wctx, 1, lambda: wctx.compress_batch(cases, sorter, 2))
    assert p > 0 and d == 0, f"option on: {p} adaptive-model passes, {d} declined (reason mask {wctx.option_get(wctx.CNT_DC_LAST_FAIL)})"
    for x, blk, w in zip(cases, on, want):
        assert blk == w, f"n={x.size} sorter={sorter}"
    off, p, d = _with_adaptive(wctx, 0, lambda: wctx.compress_batch(cases, sorter, 2))
    assert (p, d) == (0, 0)
    assert off == on


@pytest.mark.parametrize("sorter", [1, 5])
def test_compress_batch_device_input(wctx, ref, sorter):
    import torch
    cases = mb.whole_call_cases(mb.WHOLE_SEEDS['device', sorter])
    flat = torch.from_numpy(np.concatenate(cases)).cuda()
    sizes = [c.size for c in cases]
    on, p, d = _with_adaptive(wctx, 1, lambda: wctx.compress_batch_device(flat, sizes, sorter, 2))
    assert p > 0 and d == 0
    for x, blk in zip(cases, on):
        assert blk == ref.compress(x, sorter, 2), f"n={x.size} sorter={sorter}"
    off, p, d = _with_adaptive(wctx, 0, lambda: wctx.compress_batch_device(flat, sizes, sorter, 2))
    assert (p, d) == (0, 0) and off == on


def test_compress_batch_pass_declined_for_the_chain_cap(ref, monkeypatch):
    from libbsc_amd import GpuContext
    cases = mb.whole_call_cases(mb.WHOLE_SEEDS['host', 1])
    monkeypatch.setenv("BSC_DC_MIX_CHAIN_CAP", "64")
    c = GpuContext(0, max_n=ab.CTX_N)
    try:
        on, p, d = _with_adaptive(c, 1, lambda: c.compress_batch(cases, 1, 2))
        assert p == 0 and d > 0
        assert c.option_get(c.CNT_DC_LAST_FAIL) == c.DC_FAIL_MIX
        for x, blk in zip(cases, on):
            assert blk == ref.compress(x, 1, 2), f"n={x.size}"
    finally:
        c.close()


@pytest.mark.parametrize("coder", [1, 3])
def test_other_coders_are_not_touched(wctx, coder):
    """only the new option on: -e1 and -e0 move no model counter and give the option-off bytes"""
    cases = mb.whole_call_cases(mb.WHOLE_SEEDS['host', 1])
    on, p, d = _with_adaptive(wctx, 1, lambda: wctx.compress_batch(cases, 1, coder))
    assert (p, d) == (0, 0)
    off, _, _ = _with_adaptive(wctx, 0, lambda: wctx.compress_batch(cases, 1, coder))
    assert on == off


def test_their_own_options_still_route_them(wctx, ref):
    """-e1 with its own option and the new one on: the static route's counter moves, the adaptive one's does not"""
    cases = mb.whole_call_cases(mb.WHOLE_SEEDS['host', 1])
    old = wctx.option_set(wctx.OPT_BATCH_MODEL, 1), wctx.option_set(wctx.OPT_BATCH_MODEL_ADAPTIVE, 1)
    try:
        c0, m0 = _counters(wctx), wctx.option_get(wctx.CNT_BATCH_MODEL_PASSES)
        got = wctx.compress_batch(cases, 1, 1)
        assert _counters(wctx) == c0 and wctx.option_get(wctx.CNT_BATCH_MODEL_PASSES) > m0
        assert got[0] == ref.compress(cases[0], 1, 1)
    finally:
        wctx.option_set(wctx.OPT_BATCH_MODEL, old[0]); wctx.option_set(wctx.OPT_BATCH_MODEL_ADAPTIVE, old[1])


def test_segments_packed_and_device_rc_do_not_apply(wctx, ref):
    """with those options on an -e2 pass takes the whole-pass 16-bit host-coded route"""
    cases = mb.whole_call_cases(mb.WHOLE_SEEDS['host', 1])
    keys = (wctx.OPT_BATCH_MODEL_SEGMENTS, wctx.OPT_BATCH_MODEL_PACKED, wctx.OPT_DEVICE_RC)
    old = [wctx.option_set(k, 1) for k in keys]
    try:
        n0 = wctx.option_get(wctx.CNT_DEVICE_RC_BLOCKS), wctx.option_get(wctx.CNT_BATCH_SEGMENTS), wctx.option_get(wctx.CNT_BATCH_PACKED_PASSES)
        got, p, d = _with_adaptive(wctx, 1, lambda: wctx.compress_batch(cases, 1, 2))
        assert p > 0 and d == 0
        assert n0 == (wctx.option_get(wctx.CNT_DEVICE_RC_BLOCKS), wctx.option_get(wctx.CNT_BATCH_SEGMENTS), wctx.option_get(wctx.CNT_BATCH_PACKED_PASSES))
    finally:
        for k, v in zip(keys, old):
            wctx.option_set(k, v)
    for x, blk in zip(cases, got):
        assert blk == ref.compress(x, 1, 2), f"n={x.size}"


def test_option_and_small_pass(wctx, monkeypatch):
    from libbsc_amd.synth import synth_text_v1
    assert wctx.option_get(wctx.OPT_BATCH_MODEL_ADAPTIVE) == 0, "the default"
    with pytest.raises(Exception):
        wctx.option_set(wctx.OPT_BATCH_MODEL_ADAPTIVE, 2)
    with pytest.raises(Exception):
        wctx.option_set(wctx.CNT_BATCH_ADAPTIVE_PASSES, 0)
    with pytest.raises(Exception):
        wctx.option_set(wctx.CNT_BATCH_ADAPTIVE_DECLINED, 0)
    monkeypatch.delenv("BSC_BATCH_MODEL_MIN_PASS")
    small = [synth_text_v1(1, 20 * KI), synth_text_v1(2, 30 * KI)]
    _, p, d = _with_adaptive(wctx, 1, lambda: wctx.compress_batch(small, 1, 2))
    assert (p, d) == (0, 0), "a pass below the minimum takes the host model"
    monkeypatch.setenv("BSC_BATCH_MODEL_MIN_PASS", str(40 * KI))
    _, p, d = _with_adaptive(wctx, 1, lambda: wctx.compress_batch(small, 1, 2))
    assert (p, d) == (1, 0)


def test_default_cap_declines_the_pass_with_the_long_chain(actx, ref):
    """the same cases in a context with the default cap: the pass that holds the 1 MiB - 1 block is declined for its longest chain and
    coded by the host model, same bytes"""
    cases = mb.whole_call_cases(mb.WHOLE_SEEDS['host', 1])
    on, p, d = _with_adaptive(actx, 1, lambda: actx.compress_batch(cases, 1, 2))
    assert (p, d) == (0, 1) and actx.option_get(actx.CNT_DC_LAST_FAIL) == actx.DC_FAIL_MIX
    assert actx.option_get(actx.CNT_DC_MIX_LONGEST) > 1 << 18
    for x, blk in zip(cases, on):
        assert blk == ref.compress(x, 1, 2), f"n={x.size}"
