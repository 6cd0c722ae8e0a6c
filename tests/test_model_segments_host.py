"""Model segments without a GPU: the plan (bscgpu_model_segment_plan) as a pure function, and the preconditions of the inputs the GPU
tests rely on, from the CPU stand-ins alone."""
import numpy as np
import pytest

import model_batch_inputs as mb
import model_segment_inputs as ms
from libbsc_amd.gpu import model_segment_plan

BAD_PARAMETER = -1


def _one_sub(dec, und=None):
    """every block one sub-block"""
    dec = list(dec)
    return dec, (list(und) if und is not None else [0] * len(dec)), list(range(len(dec) + 1))


def test_plan_of_nothing():
    assert model_segment_plan([], [], [0], 100) == (0, [])


def test_plan_one_segment():
    dec, und, bs = _one_sub([10, 20, 30])
    assert model_segment_plan(dec, und, bs, 100) == (1, [0, 0, 0])
    assert model_segment_plan(dec, und, bs, 100, 100) == (1, [0, 0, 0])
    assert model_segment_plan(dec, und, bs, 100, 1000) == (1, [0, 0, 0]), "a target above the capacity is the capacity"
    assert model_segment_plan(dec, und, bs, 100, -5) == (1, [0, 0, 0])


def test_plan_cuts_exactly_above_the_capacity():
    dec, und, bs = _one_sub([40, 30, 30, 1])
    assert model_segment_plan(dec, und, bs, 100) == (2, [0, 0, 0, 1]), "a sum of exactly dcap is kept, dcap + 1 is cut"
    assert model_segment_plan(dec, und, bs, 101) == (1, [0, 0, 0, 0])
    assert model_segment_plan(dec, und, bs, 1000, 100) == (2, [0, 0, 0, 1]), "the target cuts as the capacity does"
    assert model_segment_plan(dec, und, bs, 1000, 99) == (2, [0, 0, 1, 1])


def test_plan_target_below_a_single_block():
    dec, und, bs = _one_sub([5, 50, 5, 5, 60, 5])
    n, seg = model_segment_plan(dec, und, bs, 100, 10)
    assert seg == [0, 1, 2, 2, 3, 4] and n == 5, "a block above the target but under the capacity is a segment of its own"


def test_plan_excluded_block_ends_a_segment_on_each_side():
    dec, und, bs = _one_sub([10, 10, 10, 10, 10], [0, 0, 3, 0, 0])
    assert model_segment_plan(dec, und, bs, 100) == (2, [0, 0, -1, 1, 1])
    dec, und, bs = _one_sub([10, 10, 10], [1, 0, 1])
    assert model_segment_plan(dec, und, bs, 100) == (1, [-1, 0, -1])


def test_plan_block_over_the_capacity_is_excluded():
    dec, und, bs = _one_sub([10, 101, 10, 100])
    assert model_segment_plan(dec, und, bs, 100) == (3, [0, -1, 1, 2])
    assert model_segment_plan(dec, und, bs, 100, 5) == (3, [0, -1, 1, 2]), "the target never excludes a block"


def test_plan_empty_blocks_end_nothing():
    #       block: 0   1(empty)  2   3(empty) 4(empty)  5
    dec, und = [10, 10, 10], [0, 0, 0]
    bs = [0, 1, 1, 2, 2, 2, 3]
    assert model_segment_plan(dec, und, bs, 100) == (1, [0, -1, 0, -1, -1, 0])
    assert model_segment_plan(dec, und, bs, 100, 20) == (2, [0, -1, 0, -1, -1, 1])
    assert model_segment_plan([], [], [0, 0, 0], 100) == (0, [-1, -1])


def test_plan_never_splits_a_block_of_two_sub_blocks():
    dec, und = [30, 30, 30, 30, 30, 30], [0] * 6
    bs = [0, 2, 4, 6]
    assert model_segment_plan(dec, und, bs, 100) == (3, [0, 1, 2]), "60 + 60 is over: the second block moves whole"
    assert model_segment_plan(dec, und, bs, 120) == (2, [0, 0, 1])
    assert model_segment_plan(dec, und, bs, 59) == (0, [-1, -1, -1]), "its own decisions are the sum over its sub-blocks"
    assert model_segment_plan(dec, [0, 0, 0, 1, 0, 0], bs, 200) == (2, [0, -1, 1]), "one undecided sub-block excludes the block"


def test_plan_bad_arguments():
    from libbsc_amd import _native as N
    f = N.lib().bscgpu_model_segment_plan
    dec, und = np.array([1, 2], np.uint32), np.zeros(2, np.uint32)
    bs, seg = np.array([0, 1, 2], np.int32), np.full(2, 77, np.int32)
    p = N.np_ptr
    assert f(p(dec), p(und), p(bs), 2, 100, 0, p(seg)) == 1 and list(seg) == [0, 0]
    seg[:] = 77
    assert f(None, p(und), p(bs), 2, 100, 0, p(seg)) == BAD_PARAMETER
    assert f(p(dec), None, p(bs), 2, 100, 0, p(seg)) == BAD_PARAMETER
    assert f(p(dec), p(und), None, 2, 100, 0, p(seg)) == BAD_PARAMETER
    assert f(p(dec), p(und), p(bs), 2, 100, 0, None) == BAD_PARAMETER
    assert f(p(dec), p(und), p(bs), -1, 100, 0, p(seg)) == BAD_PARAMETER
    assert f(p(dec), p(und), p(bs), 2, 0, 0, p(seg)) == BAD_PARAMETER
    assert f(p(dec), p(und), p(np.array([0, 2, 1], np.int32)), 2, 100, 0, p(seg)) == BAD_PARAMETER, "blk_sub must not decrease"
    assert f(p(dec), p(und), p(np.array([-1, 1, 2], np.int32)), 2, 100, 0, p(seg)) == BAD_PARAMETER
    assert list(seg) == [77, 77], "nothing is written"
    assert f(None, None, None, 0, 100, 0, None) == 0


# ---- preconditions of the GPU inputs ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("coder", [ms.STATIC, ms.FAST])
def test_over_capacity_pass_is_over_as_a_whole_and_under_block_by_block(coder):
    blocks, fb, _, _, poff = ms.reference("over_capacity", coder)
    assert len(blocks) == 32 and all(b.size == 64 << 10 for b in blocks) and sum(b.size for b in blocks) == ms.SMALL_CTX_N
    counts = ms.sub_counts(fb, coder)
    assert np.array_equal(counts, np.diff(poff.astype(np.int64))), "cap 0 returns the count the full walk writes"
    per_block = ms.block_counts(fb, counts)
    print(f"coder {coder}: {int(counts.sum())} decisions in all against {ms.SMALL_CTX_DCAP}, largest block {int(per_block.max())}")
    assert counts.sum() > ms.SMALL_CTX_DCAP, "the pass as a whole must be over the small context's capacity"
    assert per_block.max() < ms.SMALL_CTX_DCAP, "every block alone must be under it"
    n, seg = model_segment_plan(counts, np.zeros_like(counts), fb.blk_sub, ms.SMALL_CTX_DCAP)
    assert n >= 2 and min(seg) == 0, "the plan keeps every block, in at least two segments"


def test_over_capacity_pass_leaves_no_flag_undecided():
    blocks, fb, _, _, _ = ms.reference("over_capacity", ms.STATIC)
    assert mb.avg_undecided(fb) == 0, "in the pass's own run index space"
    for b, x in enumerate(blocks):
        assert mb.avg_undecided(mb.layout([x])[0]) == 0, f"block {b} alone"


def test_noise_passes_against_the_capacity():
    """The fast coder's noise passes in the small context.  fast_batch_inputs.noise_pass() was meant to have each of its two blocks under
    the capacity alone; it has not: 9 685 312 and 9 686 356 decisions against 8 470 528 (13.5 per byte of 700 KiB), so the plan excludes
    both and the GPU test asserts exactly that.  noise_under_capacity_pass() (2 x 500 KiB) is the pass that is under block by block and
    over as a whole: two segments."""
    _, fb, _, _, _ = ms.reference("noise", ms.FAST)
    counts = ms.sub_counts(fb, ms.FAST)
    per_block = ms.block_counts(fb, counts)
    print(f"noise_pass: {[int(x) for x in per_block]} decisions per block against {ms.SMALL_CTX_DCAP}")
    assert fb.count == 2 and per_block.min() > ms.SMALL_CTX_DCAP
    assert model_segment_plan(counts, np.zeros(fb.nsub), fb.blk_sub, ms.SMALL_CTX_DCAP) == (0, [-1, -1])
    _, fb, _, _, _ = ms.reference("noise_under", ms.FAST)
    counts = ms.sub_counts(fb, ms.FAST)
    per_block = ms.block_counts(fb, counts)
    print(f"noise_under_capacity_pass: {[int(x) for x in per_block]} decisions per block")
    assert fb.count == 2 and per_block.max() < ms.SMALL_CTX_DCAP < per_block.sum()
    assert model_segment_plan(counts, np.zeros(fb.nsub), fb.blk_sub, ms.SMALL_CTX_DCAP) == (2, [0, 1])


def test_expected_streams_of_a_partly_kept_pass():
    """the helper the GPU tests compare with: dropping block 1 empties its sub-blocks' ranges and closes the gap"""
    _, fb, _, ps, poff = ms.reference("fail_avg", ms.STATIC)
    e_ps, e_poff = ms.expected(fb, ps, poff, [0, 2, 0])
    s0, s1 = int(fb.blk_sub[1]), int(fb.blk_sub[2])
    assert (np.diff(e_poff.astype(np.int64))[s0:s1] == 0).all() and e_ps.size == ps.size - (int(poff[s1]) - int(poff[s0]))
    assert np.array_equal(e_ps[:int(poff[s0])], ps[:int(poff[s0])]) and np.array_equal(e_ps[int(poff[s0]):], ps[int(poff[s1]):])
    full_ps, full_poff = ms.expected(fb, ps, poff, [0, 0, 0])
    assert np.array_equal(full_ps, ps) and np.array_equal(full_poff, poff)
