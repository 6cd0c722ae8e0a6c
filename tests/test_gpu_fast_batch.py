"""The fast coder's model (-e0) of a whole pass on the GPU: the stage (bscgpu_fast_pstream_batch_device) against its CPU stand-in
(bscgpu_fast_pstream_host) entry for entry and poff for poff, the capacity exit with the pass as the unit, and the compress-batch
calls with BSCGPU_OPT_BATCH_MODEL_FAST on and off against the compiled reference block for block, with the route's own counters
showing which ran.  Every pass that is not the decline case asserts that the device kept it (the stage raises otherwise)."""
import numpy as np
import pytest

import fast_batch_inputs as fbi
import model_batch_inputs as mb
from front_inputs import KI, layouts_equal

pytestmark = pytest.mark.gpu

MIB = 1 << 20
CTX_N = fbi.CTX_N
NOT_SUPPORTED = -4


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
    """the device's stream of the pass, checked against the stand-in's: layout, poff, every entry"""
    import torch
    want, flat = mb.layout(blocks)
    want_ps, want_poff = fbi.host_streams(want)
    d = torch.from_numpy(np.concatenate([np.zeros(lead, np.uint8), flat])).cuda()
    fb, ps, poff = ctx.fast_pstream_batch(d[lead:], [b.size for b in blocks])           # raises GpuError(-4) on a declined pass
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
def test_stage_matches_stand_in_on_mixed_batch(fctx, lead):
    """every size class including 1, 2, 29, 256 KiB - 1, 256 KiB and 1 MiB - 1, an empty block, the constant block (one run of 2^18);
    lead 5: an unaligned device pointer"""
    blocks = mb.mixed_batch(0)
    fb, ps, _ = _stage(fctx, blocks, lead)
    assert fb.nsub > len(blocks)
    assert (ps & fbi.PSF_SIDE).any() and not (ps & fbi.PSF_SIDE).all()


def test_stage_pass_of_4096_blocks(fctx):
    fb, ps, _ = _stage(fctx, mb.pass_of_4096())
    assert fb.nsub > 4000 and ps.size > 64 * 8192, "sub-block starts in every tile and evaluation chunk"


def test_chain_identity_is_exact(fctx):
    """a symbol that occurs in sub-blocks 3, 11, 67, 131, 259 only: with the sub-block id kept modulo 8 (the event's signature alone)
    its chains of neighbouring sub-blocks would be walked as one"""
    _stage(fctx, mb.chain_identity_pass())


def test_long_chains_and_replay(fctx):
    blocks = mb.long_chain_pass()
    _stage(fctx, blocks)
    replays = fctx.option_get(fctx.CNT_DC_REPLAYS)
    print(f"long_chain_pass: {replays} evaluation chunks replayed")
    if fbi.replay_must_happen(mb.layout(blocks)[0]):         # the CPU walk of the brackets (test_fast_batch_host.py pins its answer)
        assert replays > 0, "a chain of alternating bits over more than three evaluation chunks must be replayed"


def test_stage_pass_that_fills_max_n():
    from libbsc_amd import GpuContext
    assert sum(mb.FILL_SIZES) == 2 * MIB
    c = GpuContext(0, max_n=2 * MIB)
    try:
        a0 = c.arena_bytes
        _stage(c, mb.fill_pass())
        a1 = c.arena_bytes
        assert a1 >= a0 + 8 * 4 * 2 * MIB, "the arena of the batch model (devcoder_batch_ensure, as the static route's) is counted once allocated"
        _stage(c, mb.fill_pass()[::-1])
        assert c.arena_bytes == a1, "allocated once"
    finally:
        c.close()


def _decline_in_small_context(check):
    from libbsc_amd import GpuContext
    c = GpuContext(0, max_n=2 * MIB)
    try:
        check(c)
    finally:
        c.close()


def test_stage_declines_the_whole_pass_for_capacity():
    import ctypes as C
    import torch
    from libbsc_amd import _native as N
    from libbsc_amd.gpu import FrontBatch
    blocks = fbi.noise_pass()
    want, flat = mb.layout(blocks)

    def check(c):
        d = torch.from_numpy(flat).cuda()
        fb = FrontBatch([b.size for b in blocks])
        out = np.zeros(16, np.uint16)
        poff = np.zeros(8, np.uint32)
        r = c.L.bscgpu_fast_pstream_batch_device(c.h, d.data_ptr(), N.np_ptr(fb.sizes), fb.count, C.byref(fb.lay), N.np_ptr(out), out.size, N.np_ptr(poff))
        assert r == NOT_SUPPORTED
        assert c.option_get(c.CNT_DC_LAST_FAIL) == c.DC_FAIL_CAP
        bad = layouts_equal(fb, want)
        assert not bad, "a declined pass still fills the layout: " + "; ".join(bad)
    _decline_in_small_context(check)


def test_stage_bad_arguments(fctx):
    import ctypes as C
    import torch
    from libbsc_amd import _native as N
    from libbsc_amd.gpu import FrontBatch
    fb = FrontBatch([100, 200])
    d = torch.zeros(300, dtype=torch.uint8, device="cuda")
    out = np.zeros(4096, np.uint16)
    poff = np.zeros(8, np.uint32)
    f = fctx.L.bscgpu_fast_pstream_batch_device
    assert f(fctx.h, d.data_ptr(), N.np_ptr(fb.sizes), 2, C.byref(fb.lay), N.np_ptr(out), out.size, None) == -1
    assert f(None, d.data_ptr(), N.np_ptr(fb.sizes), 2, C.byref(fb.lay), N.np_ptr(out), out.size, N.np_ptr(poff)) == -1
    assert f(fctx.h, d.data_ptr(), N.np_ptr(fb.sizes), 2, None, N.np_ptr(out), out.size, N.np_ptr(poff)) == -1
    _, want_poff = fbi.host_streams(mb.layout([np.zeros(100, np.uint8), np.zeros(200, np.uint8)])[0])
    out[:] = 0xffff
    D = f(fctx.h, d.data_ptr(), N.np_ptr(fb.sizes), 2, C.byref(fb.lay), N.np_ptr(out), 1, N.np_ptr(poff))       # too small: counted, not copied
    assert D == int(want_poff[2]) and list(poff[:3]) == [int(x) for x in want_poff] and (out == 0xffff).all()


# ---- whole calls -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(autouse=True)
def every_pass_size_goes_to_the_model(monkeypatch):
    """the whole-call tests use passes of a few MiB, below the route's compiled minimum (the same code path: the minimum is one
    comparison in front of it), so they lift it through the library's own knob"""
    monkeypatch.setenv("BSC_BATCH_MODEL_MIN_PASS", "0")


def _counters(ctx):
    return ctx.option_get(ctx.CNT_BATCH_FAST_PASSES), ctx.option_get(ctx.CNT_BATCH_FAST_DECLINED)


def _with_fast(ctx, value, fn):
    old = ctx.option_set(ctx.OPT_BATCH_MODEL_FAST, value)
    try:
        p0, d0 = _counters(ctx)
        out = fn()
        p1, d1 = _counters(ctx)
        return out, p1 - p0, d1 - d0
    finally:
        ctx.option_set(ctx.OPT_BATCH_MODEL_FAST, old)


@pytest.mark.parametrize("features", [3, 1])
@pytest.mark.parametrize("sorter", [1, 5])
def test_compress_batch_host_input(fctx, ref, sorter, features):
    cases = mb.whole_call_cases(mb.WHOLE_SEEDS['host', sorter])
    for lzp in ((0, 0), (15, 128)):
        want = [ref.compress(x, sorter, 3, lzp[0], lzp[1], features=features) for x in cases]
        on, p, d = _with_fast(fctx, 1, lambda: fctx.compress_batch(cases, sorter, 3, lzp[0], lzp[1], features))
        assert p > 0 and d == 0, f"option on: {p} fast-model passes, {d} declined"
        for x, blk, w in zip(cases, on, want):
            assert blk == w, f"n={x.size} sorter={sorter} lzp={lzp} features={features}"
        off, p, d = _with_fast(fctx, 0, lambda: fctx.compress_batch(cases, sorter, 3, lzp[0], lzp[1], features))
        assert (p, d) == (0, 0)
        assert off == on


@pytest.mark.parametrize("sorter", [1, 5])
def test_compress_batch_device_input(fctx, ref, sorter):
    import torch
    cases = mb.whole_call_cases(mb.WHOLE_SEEDS['device', sorter])
    flat = torch.from_numpy(np.concatenate(cases)).cuda()
    sizes = [c.size for c in cases]
    on, p, d = _with_fast(fctx, 1, lambda: fctx.compress_batch_device(flat, sizes, sorter, 3))
    assert p > 0 and d == 0
    for x, blk in zip(cases, on):
        assert blk == ref.compress(x, sorter, 3), f"n={x.size} sorter={sorter}"
    off, p, d = _with_fast(fctx, 0, lambda: fctx.compress_batch_device(flat, sizes, sorter, 3))
    assert (p, d) == (0, 0) and off == on


@pytest.mark.parametrize("coder", [1, 2])
def test_other_coders_are_not_touched(fctx, coder):
    """only the new option on: -e1 and -e2 move neither of its counters (nor the static route's) and give the option-off bytes"""
    cases = mb.whole_call_cases(mb.WHOLE_SEEDS['host', 1])
    m0 = fctx.option_get(fctx.CNT_BATCH_MODEL_PASSES), fctx.option_get(fctx.CNT_BATCH_MODEL_DECLINED)
    on, p, d = _with_fast(fctx, 1, lambda: fctx.compress_batch(cases, 1, coder))
    assert (p, d) == (0, 0)
    assert m0 == (fctx.option_get(fctx.CNT_BATCH_MODEL_PASSES), fctx.option_get(fctx.CNT_BATCH_MODEL_DECLINED))
    off, _, _ = _with_fast(fctx, 0, lambda: fctx.compress_batch(cases, 1, coder))
    assert on == off


def test_the_static_option_does_not_move_the_fast_counters(fctx):
    cases = mb.whole_call_cases(mb.WHOLE_SEEDS['host', 1])
    old = fctx.option_set(fctx.OPT_BATCH_MODEL, 1)
    try:
        c0 = _counters(fctx)
        fctx.compress_batch(cases, 1, 3)
        assert _counters(fctx) == c0
    finally:
        fctx.option_set(fctx.OPT_BATCH_MODEL, old)


def test_compress_batch_declined_pass(ref):
    """a pass of noise in a 2 MiB context: more than ten decisions per byte against a capacity of four — declined as a whole, every
    block takes the host model (and ends stored: noise)"""
    from libbsc_amd.synth import synth_text_v1
    cases = fbi.noise_pass() + [synth_text_v1(81, 300 * KI)]

    def check(c):
        on, p, d = _with_fast(c, 1, lambda: c.compress_batch(cases, 1, 3))
        assert (p, d) == (0, 1)
        assert c.option_get(c.CNT_DC_LAST_FAIL) == c.DC_FAIL_CAP
        for x, blk in zip(cases, on):
            assert blk == ref.compress(x, 1, 3), f"n={x.size}"
    _decline_in_small_context(check)


def test_option_and_small_pass(fctx, monkeypatch):
    from libbsc_amd.synth import synth_text_v1
    assert fctx.option_get(fctx.OPT_BATCH_MODEL_FAST) in (0, 1)
    with pytest.raises(Exception):
        fctx.option_set(fctx.OPT_BATCH_MODEL_FAST, 2)
    with pytest.raises(Exception):
        fctx.option_set(fctx.CNT_BATCH_FAST_PASSES, 0)
    with pytest.raises(Exception):
        fctx.option_set(fctx.CNT_BATCH_FAST_DECLINED, 0)
    monkeypatch.delenv("BSC_BATCH_MODEL_MIN_PASS")
    small = [synth_text_v1(1, 20 * KI), synth_text_v1(2, 30 * KI)]
    _, p, d = _with_fast(fctx, 1, lambda: fctx.compress_batch(small, 1, 3))
    assert (p, d) == (0, 0), "a pass below the compiled minimum takes the host model"
    monkeypatch.setenv("BSC_BATCH_MODEL_MIN_PASS", str(40 * KI))
    _, p, d = _with_fast(fctx, 1, lambda: fctx.compress_batch(small, 1, 3))
    assert (p, d) == (1, 0)


@pytest.mark.parametrize("features", [3, 1])
def test_device_range_coder_codes_a_fast_pass(fctx, ref, features):
    """BSCGPU_OPT_DEVICE_RC = 1 on top: the pass's streams through one launch of the device's range coder in the FAST16 form;
    identical bytes, counted"""
    cases = mb.whole_call_cases(mb.WHOLE_SEEDS['host', 1])
    plain, p, d = _with_fast(fctx, 1, lambda: fctx.compress_batch(cases, 1, 3, 0, 0, features))
    assert p > 0 and d == 0
    old = fctx.option_set(fctx.OPT_DEVICE_RC, 1)
    try:
        n0 = fctx.option_get(fctx.CNT_DEVICE_RC_BLOCKS)
        got, p, d = _with_fast(fctx, 1, lambda: fctx.compress_batch(cases, 1, 3, 0, 0, features))
        assert p > 0 and d == 0 and fctx.option_get(fctx.CNT_DEVICE_RC_BLOCKS) == n0 + p
    finally:
        fctx.option_set(fctx.OPT_DEVICE_RC, old)
    assert got == plain
    for x, blk in zip(cases, got):
        assert blk == ref.compress(x, 1, 3, features=features), f"n={x.size}"
