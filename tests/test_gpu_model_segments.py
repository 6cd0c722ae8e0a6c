"""A pass's model in segments on the GPU (bscgpu_pstream_batch_segments_device, BSCGPU_OPT_BATCH_MODEL_SEGMENTS): a pass over the
arena's capacity is cut instead of declined, a block the device cannot model leaves alone instead of taking its pass with it, and
wherever the cuts fall every kept entry and poff equal the CPU stand-in's.  Then the compress-batch calls with the option on against
the compiled reference block for block, with the counters showing what ran."""
import numpy as np
import pytest

import model_batch_inputs as mb
import model_segment_inputs as ms
from front_inputs import KI, layouts_equal
from pipeline_model import segment_counters

pytestmark = pytest.mark.gpu

CTX_N = (16 << 20) + 4096
NOT_SUPPORTED, BAD_PARAMETER = -4, -1
CODERS = [ms.STATIC, ms.FAST]


@pytest.fixture(scope="module")
def mctx():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from libbsc_amd import GpuContext
    c = GpuContext(0, max_n=CTX_N)
    yield c
    c.close()


@pytest.fixture(scope="module")
def small():
    """the 2 MiB context; its capacity is the one the CPU tests checked the inputs against"""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from libbsc_amd import GpuContext
    c = GpuContext(0, max_n=ms.SMALL_CTX_N)
    assert c.option_get(c.CNT_DC_DCAP) == ms.SMALL_CTX_DCAP
    yield c
    c.close()


def _seg_counters(ctx):
    return tuple(ctx.option_get(k) for k in (ctx.CNT_BATCH_SEGMENTS, ctx.CNT_BATCH_SEG_RERUNS, ctx.CNT_BATCH_SEG_HOST_BLOCKS))


def _segmented(ctx, name, coder, target=0, lead=0):
    """the segmented stage on a named pass, checked against the stand-in's streams of the blocks it kept: layout, poff, every entry
    -> (layout, entries, poff, blk_state, (segments, re-runs, host blocks) it counted)"""
    import torch
    _, want, flat, want_ps, want_poff = ms.reference(name, coder)
    d = torch.from_numpy(np.concatenate([np.zeros(lead, np.uint8), flat])).cuda()
    c0 = _seg_counters(ctx)
    fb, ps, poff, state = ctx.pstream_batch_segments(d[lead:], want.sizes, coder, target)
    moved = tuple(b - a for a, b in zip(c0, _seg_counters(ctx)))
    bad = layouts_equal(fb, want)
    assert not bad, "; ".join(bad)
    e_ps, e_poff = ms.expected(want, want_ps, want_poff, state)
    assert np.array_equal(poff, e_poff), f"poff: first difference at sub-block {int(np.flatnonzero(poff != e_poff)[0])}"
    assert ps.size == e_ps.size
    w = np.flatnonzero(ps != e_ps)
    if w.size:
        s = int(np.searchsorted(e_poff, w[0], side="right")) - 1
        raise AssertionError(f"{w.size} of {ps.size} entries differ, first at {int(w[0])} (sub-block {s}, its decision {int(w[0]) - int(e_poff[s])}): "
                             f"{int(ps[w[0]]):#x} != {int(e_ps[w[0]]):#x}; sub-blocks touched: {sorted(set(np.searchsorted(e_poff, w, side='right') - 1))[:12]}")
    reasons = 0
    for x in state:
        reasons |= int(x)
    assert ctx.option_get(ctx.CNT_DC_LAST_FAIL) == reasons, "after a segmented pass: the OR of the excluded blocks' reasons"
    assert moved[2] == int(np.count_nonzero(state))
    return fb, ps, poff, state, moved


def _block_counts(name, coder):
    _, fb, _, _, poff = ms.reference(name, coder)
    return ms.block_counts(fb, np.diff(poff.astype(np.int64)))


def _restated_counters(ctx, name, coder, target=0, decline=(), und_blocks=()):
    """(segments, re-runs, host blocks) of pipeline_model's restatement of the schedule for a named pass: the stand-in's decisions per
    sub-block, the context's capacity, the blocks of `decline` declining while they run, those of und_blocks holding an undecided flag"""
    _, fb, _, _, poff = ms.reference(name, coder)
    blk_sub = [int(fb.blk_sub[b]) for b in range(fb.count + 1)]
    und = np.zeros(fb.nsub, np.int64)
    for b in und_blocks:
        und[blk_sub[b]:blk_sub[b + 1]] = 1
    return segment_counters(np.diff(poff.astype(np.int64)), blk_sub, ctx.option_get(ctx.CNT_DC_DCAP), target, decline, ctx.DC_FAIL_HIST, und)


# ---- 1. over capacity ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("coder", CODERS)
def test_pass_over_capacity_is_cut_not_declined(small, coder):
    import torch
    from libbsc_amd.gpu import GpuError
    _, want, flat, _, _ = ms.reference("over_capacity", coder)
    d = torch.from_numpy(flat).cuda()
    with pytest.raises(GpuError) as e:                                 # the whole-pass stage, as today
        (small.fast_pstream_batch if coder == ms.FAST else small.static_pstream_batch)(d, want.sizes)
    assert e.value.code == NOT_SUPPORTED and small.option_get(small.CNT_DC_LAST_FAIL) == small.DC_FAIL_CAP
    _, ps, _, state, moved = _segmented(small, "over_capacity", coder)
    assert not state.any() and moved[0] >= 2 and moved[1] == 0
    assert ps.size > ms.SMALL_CTX_DCAP


def test_noise_pass_under_capacity_block_by_block_takes_two_segments(small):
    _, _, _, state, moved = _segmented(small, "noise_under", ms.FAST)
    assert not state.any() and moved[0] == 2


def test_noise_pass_over_capacity_block_by_block_is_left_to_the_host(small):
    """fast_batch_inputs.noise_pass(): each block alone holds more decisions than the 2 MiB context's arena (9 685 312 and 9 686 356
    against 8 470 528; test_model_segments_host.py), so no segment can hold one: both are excluded for capacity, nothing is an error"""
    _, ps, poff, state, moved = _segmented(small, "noise", ms.FAST)
    assert list(state) == [small.DC_FAIL_CAP] * 2 and moved[0] == 0 and ps.size == 0 and not poff.any()


# ---- 2. the facts: decisions and undecided flags per sub-block -----------------------------------------------------------------------
@pytest.mark.parametrize("lead", [0, 5])
@pytest.mark.parametrize("coder", CODERS)
def test_sub_dec_equals_the_stand_ins_counts(mctx, coder, lead):
    """sizes 1, 2, 29, 256 KiB +- 1, 1 MiB - 1, the empty block, the constant block; lead 5: an unaligned device pointer"""
    import torch
    _, want, flat, _, want_poff = ms.reference("mixed", coder)
    d = torch.from_numpy(np.concatenate([np.zeros(lead, np.uint8), flat])).cuda()
    fb, dec, und = mctx.model_segment_facts(d[lead:], want.sizes, coder)
    bad = layouts_equal(fb, want)
    assert not bad, "; ".join(bad)
    w = np.flatnonzero(dec != np.diff(want_poff.astype(np.int64)))
    assert w.size == 0, f"sub_dec differs for {w.size} of {fb.nsub} sub-blocks, first {int(w[0])}: {int(dec[w[0]])} != {int(want_poff[w[0] + 1]) - int(want_poff[w[0]])}"
    assert not und.any()


def test_sub_und_names_the_sub_blocks_of_the_undecided_block(mctx):
    import torch
    _, want, flat, _, want_poff = ms.reference("fail_avg", ms.STATIC)
    fb, dec, und = mctx.model_segment_facts(torch.from_numpy(flat).cuda(), want.sizes, ms.STATIC)
    s0, s1 = int(fb.blk_sub[1]), int(fb.blk_sub[2])
    assert und[s0:s1].any() and not und[:s0].any() and not und[s1:].any()
    assert int(und.sum()) == mb.avg_undecided(want), "the numpy restatement of the bracket walk, over the same lanes"
    assert np.array_equal(dec[:s0], np.diff(want_poff.astype(np.int64))[:s0]), "decided flags: the counts of the other blocks are exact"


# ---- 3. cuts everywhere ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("coder", CODERS)
def test_cuts_in_a_pass_of_4096_blocks(mctx, coder):
    total = int(_block_counts("pass_of_4096", coder).sum())
    _, _, _, state, moved = _segmented(mctx, "pass_of_4096", coder, target=total // 20)
    assert not state.any() and moved[0] >= 16


@pytest.mark.parametrize("coder", CODERS)
def test_cuts_between_the_chain_identity_blocks(mctx, coder):
    from libbsc_amd.gpu import model_segment_plan
    per_block = _block_counts("chain_identity", coder)
    dcap = mctx.option_get(mctx.CNT_DC_DCAP)
    for target, together, apart in ((int(per_block[:8].sum()), (), ((3, 11),)), (int(per_block[:100].sum()), ((3, 11), (11, 67)), ((67, 131),))):
        _, seg = model_segment_plan(per_block, np.zeros(per_block.size), np.arange(per_block.size + 1), dcap, target)
        assert all(seg[a] == seg[b] for a, b in together) and all(seg[a] != seg[b] for a, b in apart)
        _, _, _, state, moved = _segmented(mctx, "chain_identity", coder, target=target)
        assert not state.any() and moved[0] == max(seg) + 1
        assert moved == _restated_counters(mctx, "chain_identity", coder, target=target)


@pytest.mark.parametrize("coder", CODERS)
def test_cuts_at_unaligned_run_offsets(mctx, coder):
    _, _, _, state, moved = _segmented(mctx, "mixed", coder, target=200_000, lead=5)
    assert not state.any() and moved[0] >= 8


@pytest.mark.parametrize("coder", CODERS)
def test_one_segment_equals_the_whole_pass_stage(mctx, coder):
    import torch
    _, want, flat, _, _ = ms.reference("mixed", coder)
    d = torch.from_numpy(flat).cuda()
    _, w_ps, w_poff = (mctx.fast_pstream_batch if coder == ms.FAST else mctx.static_pstream_batch)(d, want.sizes)
    _, ps, poff, state, moved = _segmented(mctx, "mixed", coder, target=0)
    assert moved[0] == 1 and not state.any()
    assert np.array_equal(poff, w_poff) and np.array_equal(ps, w_ps)


# ---- 4. exclusion -----------------------------------------------------------------------------------------------------------------------
def test_undecided_block_is_excluded_by_the_plan(mctx):
    _, _, _, state, moved = _segmented(mctx, "fail_avg", ms.STATIC)
    assert list(state) == [0, mctx.DC_FAIL_AVG, 0] and moved[0] == 2 and moved[1] == 0, "known before any segment runs: no re-run"
    # (block 1 is the one that cannot be modelled; its open flags are facts, so the plan leaves it out before it could decline:
    # test_sub_und_names_the_sub_blocks_of_the_undecided_block)
    assert moved == _restated_counters(mctx, "fail_avg", ms.STATIC, decline={1}, und_blocks=(1,))
    assert mctx.option_get(mctx.CNT_DC_AVG_UNDECIDED) > 0


def test_block_that_declines_while_it_runs_is_found_by_halving(mctx):
    _, _, _, state, moved = _segmented(mctx, "fail_hist", ms.STATIC)
    assert list(state) == [0, mctx.DC_FAIL_HIST, 0]
    assert moved == _restated_counters(mctx, "fail_hist", ms.STATIC, decline={1})
    assert 1 <= moved[1] <= 2 * 2 + 2, "re-runs within 2 ceil(log2(3 blocks)) + 2"
    assert moved[0] == 2


def test_long_chains_still_replay_in_small_segments(mctx):
    _, _, _, state, _ = _segmented(mctx, "long_chain", ms.STATIC, target=1_000_000)
    assert not state.any()
    assert mctx.option_get(mctx.CNT_DC_REPLAYS) > 0, "a chain longer than an evaluation chunk whose bracket stays open must be replayed"


# ---- 6. arguments -----------------------------------------------------------------------------------------------------------------------
def test_stage_bad_arguments(mctx):
    import ctypes as C
    import torch
    from libbsc_amd import _native as N
    from libbsc_amd.gpu import FrontBatch
    fb = FrontBatch([100, 200])
    d = torch.zeros(300, dtype=torch.uint8, device="cuda")
    out, poff, state = np.zeros(4096, np.uint16), np.zeros(8, np.uint32), np.zeros(2, np.int32)
    f = mctx.L.bscgpu_pstream_batch_segments_device
    p = N.np_ptr
    args = lambda **kw: [kw.get("h", mctx.h), d.data_ptr(), p(fb.sizes), 2, kw.get("lay", C.byref(fb.lay)), kw.get("coder", 1), 0,
                         kw.get("out", p(out)), kw.get("cap", out.size), kw.get("poff", p(poff)), kw.get("state", p(state))]
    assert f(*args(h=None)) == BAD_PARAMETER
    assert f(*args(lay=None)) == BAD_PARAMETER
    assert f(*args(poff=None)) == BAD_PARAMETER
    assert f(*args(state=None)) == BAD_PARAMETER
    assert f(*args(out=None)) == BAD_PARAMETER
    assert f(*args(coder=2)) == BAD_PARAMETER and f(*args(coder=0)) == BAD_PARAMETER
    assert f(*args(cap=-1)) == BAD_PARAMETER
    for coder in CODERS:
        want = mb.layout([np.zeros(100, np.uint8), np.zeros(200, np.uint8)])[0]
        counts = ms.sub_counts(want, coder)
        out[:] = 0xffff
        state[:] = 7
        D = f(*args(coder=coder, cap=1))                              # too small: counted, not copied
        assert D == int(counts.sum()) and list(poff[:3]) == [0, int(counts[0]), int(counts.sum())] and list(state) == [0, 0] and (out == 0xffff).all()
        D = f(*args(coder=coder, out=None, cap=0))
        assert D == int(counts.sum())


# ---- 5. whole calls ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(autouse=True)
def every_pass_size_goes_to_the_model(monkeypatch):
    """the route's minimum pass size is 16 / 32 MiB; the whole-call tests use passes of a few MiB through the library's own knob"""
    monkeypatch.setenv("BSC_BATCH_MODEL_MIN_PASS", "0")


def _route(ctx, coder, segments, fn, device_rc=0):
    """fn() with the coder's model option on and the segments option as given -> (its result, model passes, declined, segment counters moved)"""
    fast = coder == ms.FAST
    opt = ctx.OPT_BATCH_MODEL_FAST if fast else ctx.OPT_BATCH_MODEL
    keys = (ctx.CNT_BATCH_FAST_PASSES, ctx.CNT_BATCH_FAST_DECLINED) if fast else (ctx.CNT_BATCH_MODEL_PASSES, ctx.CNT_BATCH_MODEL_DECLINED)
    old = ctx.option_set(opt, 1), ctx.option_set(ctx.OPT_BATCH_MODEL_SEGMENTS, segments), ctx.option_set(ctx.OPT_DEVICE_RC, device_rc)
    try:
        p0, s0 = [ctx.option_get(k) for k in keys], _seg_counters(ctx)
        out = fn()
        p1, s1 = [ctx.option_get(k) for k in keys], _seg_counters(ctx)
        return out, p1[0] - p0[0], p1[1] - p0[1], tuple(b - a for a, b in zip(s0, s1))
    finally:
        ctx.option_set(opt, old[0]); ctx.option_set(ctx.OPT_BATCH_MODEL_SEGMENTS, old[1]); ctx.option_set(ctx.OPT_DEVICE_RC, old[2])


@pytest.mark.parametrize("coder", CODERS)
@pytest.mark.parametrize("sorter", [1, 5])
def test_compress_batch_host_input_in_segments(mctx, ref, monkeypatch, sorter, coder):
    monkeypatch.setenv("BSC_BATCH_MODEL_SEGMENT", "300000")
    cases = mb.whole_call_cases(mb.WHOLE_SEEDS['host', sorter])
    for lzp in ((0, 0), (15, 128)):
        want = [ref.compress(x, sorter, coder, lzp[0], lzp[1]) for x in cases]
        got, p, d, seg = _route(mctx, coder, 1, lambda: mctx.compress_batch(cases, sorter, coder, lzp[0], lzp[1]))
        assert (p, d) == (1, 0) and seg[0] >= 2, f"{p} model passes, {d} declined, segments / re-runs / host blocks {seg}"
        for x, blk, w in zip(cases, got, want):
            assert blk == w, f"n={x.size} sorter={sorter} coder={coder} lzp={lzp}"


@pytest.mark.parametrize("coder", CODERS)
@pytest.mark.parametrize("sorter", [1, 5])
def test_compress_batch_device_input_in_segments(mctx, ref, monkeypatch, sorter, coder):
    import torch
    monkeypatch.setenv("BSC_BATCH_MODEL_SEGMENT", "300000")
    cases = mb.whole_call_cases(mb.WHOLE_SEEDS['device', sorter])
    flat = torch.from_numpy(np.concatenate(cases)).cuda()
    got, p, d, seg = _route(mctx, coder, 1, lambda: mctx.compress_batch_device(flat, [c.size for c in cases], sorter, coder))
    assert (p, d) == (1, 0) and seg[0] >= 2
    for x, blk in zip(cases, got):
        assert blk == ref.compress(x, sorter, coder), f"n={x.size} sorter={sorter} coder={coder}"


@pytest.mark.parametrize("case", ["avg", "hist"])
def test_block_that_declined_its_pass_now_leaves_alone(mctx, ref, case):
    """the two inputs of test_gpu_model_batch.test_compress_batch_declined_pass: one block takes the host model, the pass stays"""
    import devcoder_inputs as di
    from libbsc_amd.synth import synth_text_v1
    bad = di.text_with_bwt_like(di.runs_to_block(di.const_rank(40, 200_000), np.tile([1, 1, 2, 4], 50_000)) if case == "avg" else di.hist_chain(40_000))
    cases = [synth_text_v1(81, 700 * KI), bad, synth_text_v1(82, 300 * KI)]
    got, p, d, seg = _route(mctx, ms.STATIC, 1, lambda: mctx.compress_batch(cases, 1, 1))
    assert (p, d) == (1, 0) and seg[2] == 1 and seg[0] >= 1
    assert mctx.option_get(mctx.CNT_DC_LAST_FAIL) == (mctx.DC_FAIL_AVG if case == "avg" else mctx.DC_FAIL_HIST)
    for x, blk in zip(cases, got):
        assert blk == ref.compress(x, 1, 1), f"n={x.size}"


def test_streams_beyond_the_landing_buffer_take_the_host_model(small, ref):
    """two 500 KiB noise texts with -e0 in the 2 MiB context: each block's streams fit the pinned landing buffer, both do not; the two
    are over the capacity together, so each is a segment of its own: exactly one is kept and exactly one block goes to the host"""
    cases = ms.noise_under_capacity_pass()
    got, p, d, seg = _route(small, ms.FAST, 1, lambda: small.compress_batch(cases, 1, ms.FAST))
    assert (p, d) == (1, 0) and seg[0] == 1 and seg[2] == 1, f"segments / re-runs / host blocks {seg}"
    for x, blk in zip(cases, got):
        assert blk == ref.compress(x, 1, ms.FAST)


@pytest.mark.parametrize("coder", CODERS)
def test_option_off_and_device_range_coder_take_todays_route(mctx, monkeypatch, coder):
    monkeypatch.setenv("BSC_BATCH_MODEL_SEGMENT", "300000")
    cases = mb.whole_call_cases(mb.WHOLE_SEEDS['host', 1])
    on, p, d, seg = _route(mctx, coder, 1, lambda: mctx.compress_batch(cases, 1, coder))
    assert (p, d) == (1, 0) and seg[0] >= 2
    off, p, d, seg = _route(mctx, coder, 0, lambda: mctx.compress_batch(cases, 1, coder))
    assert (p, d) == (1, 0) and seg == (0, 0, 0) and off == on
    rc, p, d, seg = _route(mctx, coder, 1, lambda: mctx.compress_batch(cases, 1, coder), device_rc=1)
    assert (p, d) == (1, 0) and seg == (0, 0, 0) and rc == on
    assert mctx.option_get(mctx.OPT_BATCH_MODEL_SEGMENTS) == 0, "the default"
    with pytest.raises(Exception):
        mctx.option_set(mctx.OPT_BATCH_MODEL_SEGMENTS, 2)
    with pytest.raises(Exception):
        mctx.option_set(mctx.CNT_BATCH_SEGMENTS, 0)


@pytest.mark.parametrize("coder", CODERS)
def test_three_passes_in_segments_code_in_order(small, ref, monkeypatch, coder):
    """a call of three passes in the 2 MiB context, each cut into several segments: a pass's coder thread starts with the pass's plan
    and takes its groups while the model runs, behind the previous pass's coding and beside the next pass's sort; every block of
    every pass equals the reference's, and the counters show three model passes of at least two segments each"""
    from libbsc_amd.synth import synth_text_v1
    monkeypatch.setenv("BSC_BATCH_MODEL_SEGMENT", "400000")
    # (two blocks of 700 KiB to a pass of 2 MiB: about 6 M decisions, inside the landing buffer of the context)
    cases = [synth_text_v1(90 + i, n) for i, n in enumerate([700 * KI, 20, 700 * KI, 0, 700 * KI, 29, 700 * KI, 700 * KI, 1, 700 * KI])]
    got, p, d, seg = _route(small, coder, 1, lambda: small.compress_batch(cases, 1, coder))
    assert (p, d) == (3, 0) and seg[0] >= 6 and seg[2] == 0, f"{p} model passes, {d} declined, segments / re-runs / host blocks {seg}"
    for x, blk in zip(cases, got):
        assert blk == ref.compress(x, 1, coder), f"n={x.size} coder={coder}"
