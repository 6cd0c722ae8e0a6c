"""The adaptive coder's model (-e2) of a pass in segments on the GPU (bscgpu_adaptive_segment_facts_device,
bscgpu_adaptive_pstream_batch_segments_device, BSCGPU_OPT_BATCH_ADAPTIVE_SEGMENTS): the three facts against the CPU stand-in, a pass
over the arena's capacity cut instead of declined, every kept entry and poff equal to the stand-in's wherever the cuts fall, the step
cap read per block (BSCGPU_DC_FAIL_MIX known before anything runs), and the compress-batch calls with the option on against the
compiled reference block for block, with the counters showing what ran."""
import numpy as np
import pytest

import adaptive_batch_inputs as ab
import adaptive_segment_inputs as asi
import model_batch_inputs as mb
import model_segment_inputs as ms
from front_inputs import layouts_equal

pytestmark = pytest.mark.gpu

NOT_SUPPORTED, BAD_PARAMETER = -4, -1


def _ctx(max_n, mix_cap=None):
    import os
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from libbsc_amd import GpuContext
    old = os.environ.get("BSC_DC_MIX_CHAIN_CAP")
    if mix_cap is not None:
        os.environ["BSC_DC_MIX_CHAIN_CAP"] = str(mix_cap)             # read when the context is created
    try:
        return GpuContext(0, max_n=max_n)
    finally:
        if mix_cap is not None:
            if old is None:
                del os.environ["BSC_DC_MIX_CHAIN_CAP"]
            else:
                os.environ["BSC_DC_MIX_CHAIN_CAP"] = old


@pytest.fixture(scope="module")
def actx():
    """the 16 MiB + 4096 context of the sibling tests, with the default step cap"""
    c = _ctx(ab.CTX_N)
    yield c
    c.close()


@pytest.fixture(scope="module")
def small():
    """the 2 MiB context; its capacity is the one the CPU tests checked the inputs against"""
    c = _ctx(ms.SMALL_CTX_N)
    assert c.option_get(c.CNT_DC_DCAP) == ms.SMALL_CTX_DCAP
    yield c
    c.close()


def _seg_counters(ctx):
    return tuple(ctx.option_get(k) for k in (ctx.CNT_BATCH_SEGMENTS, ctx.CNT_BATCH_SEG_RERUNS, ctx.CNT_BATCH_SEG_HOST_BLOCKS))


def _segmented(ctx, name, target=0, lead=0):
    """the segmented stage on a named pass, checked against the stand-in's streams of the blocks it kept: layout, poff, every entry
    -> (layout, entries, poff, blk_state, (segments, re-runs, host blocks) it counted)"""
    import torch
    _, want, flat, want_ps, want_poff, _ = asi.reference(name)
    d = torch.from_numpy(np.concatenate([np.zeros(lead, np.uint8), flat])).cuda()
    c0 = _seg_counters(ctx)
    fb, ps, poff, state = ctx.adaptive_pstream_batch_segments(d[lead:], want.sizes, target)
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


def _kept_longest(name, state):
    """the longest chain among the sub-blocks of the kept blocks, by the stand-in"""
    _, fb, _, _, _, mix = asi.reference(name)
    kept = [int(mix[s]) for b in range(fb.count) if state[b] == 0 for s in range(fb.blk_sub[b], fb.blk_sub[b + 1])]
    return max(kept) if kept else 0


# ---- 1. the facts ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,lead", [("mixed", 0), ("mixed", 5), ("escape", 0), ("hist_above_clamp", 0), ("tiny_alphabets", 0), ("chain_identity", 0)])
def test_facts_equal_the_stand_ins(actx, name, lead):
    """sub_dec and sub_und are the static coder's; sub_mix is the longest mixer chain of every sub-block, compared where sub_und == 0;
    lead 5: an unaligned device pointer"""
    import torch
    _, want, flat, _, want_poff, want_mix = asi.reference(name)
    d = torch.from_numpy(np.concatenate([np.zeros(lead, np.uint8), flat])).cuda()
    fb, dec, und, mix = actx.adaptive_segment_facts(d[lead:], want.sizes)
    bad = layouts_equal(fb, want)
    assert not bad, "; ".join(bad)
    w = np.flatnonzero(dec != np.diff(want_poff.astype(np.int64)))
    assert w.size == 0, f"sub_dec differs for {w.size} of {fb.nsub} sub-blocks, first {int(w[0])}"
    assert not und.any(), "none of these passes leaves a flag open (the whole-pass stage keeps them)"
    decided = und == 0
    w = np.flatnonzero((mix.astype(np.int64) != want_mix) & decided)
    assert w.size == 0, f"sub_mix differs for {w.size} of {fb.nsub} sub-blocks, first {int(w[0])}: {int(mix[w[0]])} != {int(want_mix[w[0]])}"
    _, dec1, und1 = actx.model_segment_facts(d[lead:], want.sizes, ms.STATIC)
    assert np.array_equal(dec1, dec) and np.array_equal(und1, und), "same decisions, same flags as coder 1"


def test_the_other_exports_keep_refusing_coder_2(actx):
    import torch
    from libbsc_amd.gpu import GpuError
    d = torch.zeros(300, dtype=torch.uint8, device="cuda")
    for call in (lambda: actx.model_segment_facts(d, [100, 200], asi.ADAPTIVE), lambda: actx.pstream_batch_segments(d, [100, 200], asi.ADAPTIVE)):
        with pytest.raises(GpuError) as e:
            call()
        assert e.value.code == BAD_PARAMETER


def test_stage_bad_arguments(actx):
    import ctypes as C
    import torch
    from libbsc_amd import _native as N
    from libbsc_amd.gpu import FrontBatch
    fb = FrontBatch([100, 200])
    d = torch.zeros(300, dtype=torch.uint8, device="cuda")
    out, poff, state = np.zeros(4096, np.uint16), np.zeros(8, np.uint32), np.zeros(2, np.int32)
    f = actx.L.bscgpu_adaptive_pstream_batch_segments_device
    p = N.np_ptr
    args = lambda **kw: [kw.get("h", actx.h), d.data_ptr(), p(fb.sizes), 2, kw.get("lay", C.byref(fb.lay)), 0,
                         kw.get("out", p(out)), kw.get("cap", out.size), kw.get("poff", p(poff)), kw.get("state", p(state))]
    assert f(*args(h=None)) == BAD_PARAMETER
    assert f(*args(lay=None)) == BAD_PARAMETER
    assert f(*args(poff=None)) == BAD_PARAMETER
    assert f(*args(state=None)) == BAD_PARAMETER
    assert f(*args(out=None)) == BAD_PARAMETER
    assert f(*args(cap=-1)) == BAD_PARAMETER
    g = actx.L.bscgpu_adaptive_segment_facts_device
    assert g(actx.h, d.data_ptr(), p(fb.sizes), 2, C.byref(fb.lay), p(poff), p(poff), None) == BAD_PARAMETER
    counts = ms.sub_counts(mb.layout([np.zeros(100, np.uint8), np.zeros(200, np.uint8)])[0], ms.STATIC)
    out[:] = 0xffff
    state[:] = 7
    D = f(*args(cap=1))                                                # too small: counted, not copied
    assert D == int(counts.sum()) and list(poff[:3]) == [0, int(counts[0]), int(counts.sum())] and list(state) == [0, 0] and (out == 0xffff).all()


# ---- 2. over capacity -----------------------------------------------------------------------------------------------------------------
def test_pass_over_capacity_is_cut_not_declined(small):
    """FAILS WITHOUT THE FEATURE: the whole-pass -e2 stage can only decline this pass (FAIL_CAP)"""
    import torch
    from libbsc_amd.gpu import GpuError, adaptive_longest_chain_host
    _, want, flat, _, _, want_mix = asi.reference("over_capacity")
    d = torch.from_numpy(np.array(flat)).cuda()
    with pytest.raises(GpuError) as e:                                 # the whole-pass stage, as today
        small.adaptive_pstream_batch(d, want.sizes)
    assert e.value.code == NOT_SUPPORTED and small.option_get(small.CNT_DC_LAST_FAIL) == small.DC_FAIL_CAP
    _, ps, _, state, moved = _segmented(small, "over_capacity")
    assert not state.any() and moved[0] >= 2 and moved[1] == 0
    assert ps.size > ms.SMALL_CTX_DCAP
    assert small.option_get(small.CNT_DC_MIX_LONGEST) == int(want_mix.max())
    chains = sum(int(np.count_nonzero(adaptive_longest_chain_host(want, s, per_mixer=True)[1])) for s in range(want.nsub))
    assert small.option_get(small.CNT_DC_MIX_CHAINS) == chains, "the sum over the kept segments"


# ---- 3. cuts everywhere ---------------------------------------------------------------------------------------------------------------
def _block_counts(name):
    _, fb, _, _, poff, _ = asi.reference(name)
    return ms.block_counts(fb, np.diff(poff.astype(np.int64)))


def test_cuts_in_a_pass_of_4096_blocks(actx):
    total = int(_block_counts("pass_of_4096").sum())
    _, _, _, state, moved = _segmented(actx, "pass_of_4096", target=total // 20)
    assert not state.any() and moved[0] >= 16 and moved[1] == 0
    assert actx.option_get(actx.CNT_DC_MIX_LONGEST) == _kept_longest("pass_of_4096", state)


def test_cuts_between_the_chain_identity_blocks(actx):
    """the sub-block ids in the mixer key are the segment's own: a cut between two blocks that share a mixer id changes nothing"""
    from libbsc_amd.gpu import model_segment_plan
    per_block = _block_counts("chain_identity")
    dcap = actx.option_get(actx.CNT_DC_DCAP)
    for target, together, apart in ((int(per_block[:8].sum()), (), ((3, 11),)), (int(per_block[:100].sum()), ((3, 11), (11, 67)), ((67, 131),))):
        _, seg = model_segment_plan(per_block, np.zeros(per_block.size), np.arange(per_block.size + 1), dcap, target)
        assert all(seg[a] == seg[b] for a, b in together) and all(seg[a] != seg[b] for a, b in apart)
        _, _, _, state, moved = _segmented(actx, "chain_identity", target=target)
        assert not state.any() and moved == (max(seg) + 1, 0, 0)


def test_cuts_at_unaligned_run_offsets(actx):
    _, _, _, state, moved = _segmented(actx, "mixed", target=200_000, lead=5)
    assert not state.any() and moved[0] >= 8 and moved[1] == 0


def test_one_segment_equals_the_whole_pass_stage(actx):
    import torch
    _, want, flat, _, _, want_mix = asi.reference("mixed")
    d = torch.from_numpy(np.array(flat)).cuda()
    _, w_ps, w_poff = actx.adaptive_pstream_batch(d, want.sizes)
    whole = actx.option_get(actx.CNT_DC_MIX_CHAINS), actx.option_get(actx.CNT_DC_MIX_LONGEST)
    _, ps, poff, state, moved = _segmented(actx, "mixed", target=0)
    assert moved == (1, 0, 0) and not state.any()
    assert np.array_equal(poff, w_poff) and np.array_equal(ps, w_ps)
    assert whole == (actx.option_get(actx.CNT_DC_MIX_CHAINS), actx.option_get(actx.CNT_DC_MIX_LONGEST)) and whole[1] == int(want_mix.max())


# ---- 4. the step cap per block ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cap", [asi.MIX_CAP_BETWEEN, None])
def test_block_above_the_step_cap_is_excluded_by_the_plan(actx, cap):
    """a cap between the block maxima (and the default, which bars three): exactly the blocks the stand-in puts above it are left out,
    before anything runs — no re-run — and the others equal the stand-in"""
    _, fb, _, _, _, mix = asi.reference("cap_sides")
    per_block = asi.block_max(fb, mix)
    c = actx if cap is None else _ctx(ab.CTX_N, cap)
    try:
        barred = per_block > (asi.MIX_CAP_DEFAULT if cap is None else cap)
        assert barred.sum() == (3 if cap is None else 2)
        _, _, _, state, moved = _segmented(c, "cap_sides")
        assert list(state) == [c.DC_FAIL_MIX if x else 0 for x in barred]
        assert moved[1] == 0 and moved[2] == int(barred.sum()) and moved[0] >= 2, "a barred block ends the segment before it"
        assert c.option_get(c.CNT_DC_LAST_FAIL) == c.DC_FAIL_MIX
        assert c.option_get(c.CNT_DC_MIX_LONGEST) == _kept_longest("cap_sides", state)
    finally:
        if cap is not None:
            c.close()


# ---- 5. whole calls ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(autouse=True)
def every_pass_size_goes_to_the_model(monkeypatch):
    """the route's minimum pass size is 16 MiB; the whole-call tests use passes of a few MiB through the library's own knob"""
    monkeypatch.setenv("BSC_BATCH_MODEL_MIN_PASS", "0")


def _route(ctx, segments, fn, adaptive=1):
    """fn() with BSCGPU_OPT_BATCH_MODEL_ADAPTIVE and the new option as given -> (its result, adaptive passes, declined, segment counters
    moved); the other coders' counters must not move"""
    others = (ctx.CNT_BATCH_MODEL_PASSES, ctx.CNT_BATCH_MODEL_DECLINED, ctx.CNT_BATCH_FAST_PASSES, ctx.CNT_BATCH_FAST_DECLINED,
              ctx.CNT_BATCH_PACKED_PASSES, ctx.CNT_DEVICE_RC_BLOCKS)
    keys = (ctx.CNT_BATCH_ADAPTIVE_PASSES, ctx.CNT_BATCH_ADAPTIVE_DECLINED)
    old = ctx.option_set(ctx.OPT_BATCH_MODEL_ADAPTIVE, adaptive), ctx.option_set(ctx.OPT_BATCH_ADAPTIVE_SEGMENTS, segments)
    try:
        p0, s0, o0 = [ctx.option_get(k) for k in keys], _seg_counters(ctx), [ctx.option_get(k) for k in others]
        out = fn()
        p1, s1 = [ctx.option_get(k) for k in keys], _seg_counters(ctx)
        assert o0 == [ctx.option_get(k) for k in others], "the static and the fast route's counters do not move"
        return out, p1[0] - p0[0], p1[1] - p0[1], tuple(b - a for a, b in zip(s0, s1))
    finally:
        ctx.option_set(ctx.OPT_BATCH_MODEL_ADAPTIVE, old[0]); ctx.option_set(ctx.OPT_BATCH_ADAPTIVE_SEGMENTS, old[1])


@pytest.mark.parametrize("sorter", [1, 5])
def test_compress_batch_host_input_keeps_the_pass_with_the_long_chain(actx, ref, sorter):
    """FAILS WITHOUT THE FEATURE: in a default-cap context the pass that holds the 1 MiB - 1 block is declined whole today
    (test_gpu_adaptive_batch.py); in segments it is kept and that block alone takes the host model"""
    cases = mb.whole_call_cases(mb.WHOLE_SEEDS['host', sorter])
    want = [ref.compress(x, sorter, 2) for x in cases]
    on, p, d, seg = _route(actx, 1, lambda: actx.compress_batch(cases, sorter, 2))
    assert (p, d) == (1, 0) and seg[0] >= 2 and seg[1] == 0 and seg[2] == 1, f"{p} adaptive passes, {d} declined, segments / re-runs / host blocks {seg}"
    assert actx.option_get(actx.CNT_DC_LAST_FAIL) == actx.DC_FAIL_MIX
    for x, blk, w in zip(cases, on, want):
        assert blk == w, f"n={x.size} sorter={sorter}"
    off, p, d, seg = _route(actx, 0, lambda: actx.compress_batch(cases, sorter, 2))
    assert (p, d) == (0, 1) and seg == (0, 0, 0), "the option off: the whole pass, declined for its longest chain as today"
    assert off == on


@pytest.mark.parametrize("sorter", [1, 5])
def test_compress_batch_device_input_in_segments(actx, ref, monkeypatch, sorter):
    import torch
    monkeypatch.setenv("BSC_BATCH_MODEL_SEGMENT", "300000")
    cases = mb.whole_call_cases(mb.WHOLE_SEEDS['device', sorter])
    flat = torch.from_numpy(np.concatenate(cases)).cuda()
    sizes = [c.size for c in cases]
    on, p, d, seg = _route(actx, 1, lambda: actx.compress_batch_device(flat, sizes, sorter, 2))
    assert (p, d) == (1, 0) and seg[0] >= 4 and seg[1] == 0 and seg[2] == 1
    for x, blk in zip(cases, on):
        assert blk == ref.compress(x, sorter, 2), f"n={x.size} sorter={sorter}"
    off, p, d, seg = _route(actx, 0, lambda: actx.compress_batch_device(flat, sizes, sorter, 2))
    assert (p, d) == (0, 1) and seg == (0, 0, 0) and off == on


def test_lzp_and_a_small_target(actx, ref, monkeypatch):
    monkeypatch.setenv("BSC_BATCH_MODEL_SEGMENT", "300000")
    cases = mb.whole_call_cases(mb.WHOLE_SEEDS['host', 1])
    got, p, d, seg = _route(actx, 1, lambda: actx.compress_batch(cases, 1, 2, 15, 128))
    assert (p, d) == (1, 0) and seg[0] >= 4
    for x, blk in zip(cases, got):
        assert blk == ref.compress(x, 1, 2, 15, 128), f"n={x.size}"


@pytest.mark.parametrize("coder", [1, 3])
def test_other_coders_are_not_touched(actx, coder):
    """both -e2 options on: -e1 and -e0 move no model or segment counter and give the options-off bytes"""
    cases = mb.whole_call_cases(mb.WHOLE_SEEDS['host', 1])
    on, p, d, seg = _route(actx, 1, lambda: actx.compress_batch(cases, 1, coder))
    assert (p, d) == (0, 0) and seg == (0, 0, 0)
    off, p, d, seg = _route(actx, 0, lambda: actx.compress_batch(cases, 1, coder), adaptive=0)
    assert (p, d) == (0, 0) and seg == (0, 0, 0) and on == off


def test_option_alone_routes_nothing(actx):
    """the new option without BSCGPU_OPT_BATCH_MODEL_ADAPTIVE: an -e2 call takes the host model; its default and its values"""
    assert actx.option_get(actx.OPT_BATCH_ADAPTIVE_SEGMENTS) == 0, "the default"
    with pytest.raises(Exception):
        actx.option_set(actx.OPT_BATCH_ADAPTIVE_SEGMENTS, 2)
    cases = mb.whole_call_cases(mb.WHOLE_SEEDS['host', 1])[:4]
    on, p, d, seg = _route(actx, 1, lambda: actx.compress_batch(cases, 1, 2), adaptive=0)
    assert (p, d) == (0, 0) and seg == (0, 0, 0)
    # ... and BSCGPU_OPT_BATCH_MODEL_SEGMENTS keeps not applying to -e2
    old = actx.option_set(actx.OPT_BATCH_MODEL_SEGMENTS, 1)
    try:
        got, p, d, seg = _route(actx, 0, lambda: actx.compress_batch(cases, 1, 2))
        assert (p, d) == (1, 0) and seg == (0, 0, 0) and got == on
    finally:
        actx.option_set(actx.OPT_BATCH_MODEL_SEGMENTS, old)


def test_three_passes_in_segments_code_in_order(small, ref, monkeypatch):
    """a call of three passes in the 2 MiB context, each cut into several segments: a pass's coder thread starts with the pass's plan
    and takes its groups while the model runs, behind the previous pass's coding and beside the next pass's sort"""
    monkeypatch.setenv("BSC_BATCH_MODEL_SEGMENT", "400000")
    cases = asi.three_pass_cases()
    got, p, d, seg = _route(small, 1, lambda: small.compress_batch(cases, 1, 2))
    assert (p, d) == (3, 0) and seg[0] >= 6 and seg[2] == 0, f"{p} adaptive passes, {d} declined, segments / re-runs / host blocks {seg}"
    for x, blk in zip(cases, got):
        assert blk == ref.compress(x, 1, 2), f"n={x.size}"
