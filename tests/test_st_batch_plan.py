"""bscgpu_st_batch_plan: which blocks of a batch share one sort-transform pass (pure function, no GPU)."""
import numpy as np
import pytest

from libbsc_amd.gpu import ST_BATCH_MAX_BLOCKS, ST_BATCH_MAX_N, batch_plan, st_batch_plan

MIB = 1 << 20
CUT = 1 << 20                       # BSCGPU_ST_BATCH_MAX_N
BLOCKS = 4096                       # BSCGPU_ST_BATCH_MAX_BLOCKS, the same for every k
KS = [3, 4, 5, 6, 7, 8]


def _rule(sizes, cap):
    """the rule restated: consecutive blocks of 1 .. CUT - 1 bytes (and <= cap) share a pass of <= cap bytes and <= BLOCKS
    entries; an empty block is an entry of the pass around it; any other block goes alone and ends the pass"""
    plan, npass, cur, used, span = [], 0, -1, 0, 0
    for n in sizes:
        if n == 0 or n >= CUT or n > cap:
            plan.append(-1)
            cur, span = (cur, span + (cur >= 0)) if n == 0 else (-1, span)
            continue
        if cur < 0 or used + n > cap or span + 1 > BLOCKS:
            cur, npass, used, span = npass, npass + 1, 0, 0
        plan.append(cur)
        used, span = used + n, span + 1
    return npass, plan


def _check(sizes, k, cap):
    npass, plan = st_batch_plan(sizes, k, cap)
    assert len(plan) == len(sizes)
    assert all(-1 <= p < npass for p in plan), "every block gets a pass or -1"
    seen = [p for p in plan if p >= 0]
    assert seen == sorted(seen), "passes follow the input order"
    assert set(seen) == set(range(npass)), "no pass is empty, numbering is dense"
    for p in range(npass):
        members = [b for b in range(len(sizes)) if plan[b] == p]
        assert sum(sizes[b] for b in members) <= cap
        assert members[-1] + 1 - members[0] <= BLOCKS, "the pass's table (empty entries included) fits the block cap"
        for b in range(members[0], members[-1] + 1):
            assert plan[b] == p or sizes[b] == 0, "one contiguous range of the input: only empty blocks between members"
    for b, n in enumerate(sizes):
        if n >= CUT or n == 0 or n > cap:
            assert plan[b] == -1
        else:
            assert plan[b] >= 0
    assert (npass, plan) == _rule(sizes, cap)
    return npass, plan


def test_constants_match_the_header():
    assert (ST_BATCH_MAX_N, ST_BATCH_MAX_BLOCKS) == (CUT, BLOCKS)


@pytest.mark.parametrize("k", KS)
def test_small_blocks_share_passes(k):
    npass, plan = _check([65536] * 64, k, 4 * MIB)
    assert npass == 1 and plan == [0] * 64
    npass, plan = _check([65536] * 200, k, 4 * MIB)
    assert npass == 4


@pytest.mark.parametrize("k", KS)
def test_threshold_routes_to_single_path(k):
    sizes = [1000, CUT - 1, CUT, 2 * MIB, 5000, 1, 2]
    npass, plan = _check(sizes, k, 64 * MIB)
    assert plan == [0, 0, -1, -1, 1, 1, 1]


def test_the_bwt_plan_still_leaves_st_alone():
    npass, plan = batch_plan([1000, 5000], 5, 64 * MIB)
    assert npass == 0 and plan == [-1, -1]


def test_zero_sizes_and_oversized():
    sizes = [0, 100, 0, 0, 200, 0]
    npass, plan = _check(sizes, 5, 1000)
    assert npass == 1 and plan == [-1, 0, -1, -1, 0, -1]
    npass, plan = _check([0, 0, 0], 5, 1000)
    assert npass == 0
    npass, plan = _check([500, 2000, 500], 5, 1000)        # larger than the cap: a block of its own
    assert plan == [0, -1, 1]
    npass, plan = _check([], 5, 1000)
    assert npass == 0 and plan == []


@pytest.mark.parametrize("k", KS)
def test_block_count_cap(k):
    npass, plan = _check([16] * 10000, k, 64 * MIB)
    assert npass == 3
    assert max(plan.count(p) for p in range(npass)) == BLOCKS
    sizes = [16, 0] * 5000                                  # empty entries count against the cap
    npass, plan = _check(sizes, k, 64 * MIB)
    assert npass == 3


def test_seeded_random():
    rng = np.random.default_rng(7)
    for t in range(60):
        cnt = int(rng.integers(0, 300))
        sizes = [int(x) for x in rng.integers(0, 2 * CUT, cnt)]
        for i in rng.integers(0, max(cnt, 1), cnt // 5):
            if cnt:
                sizes[int(i)] = int(rng.integers(0, 3))
        _check(sizes, KS[t % 6], int(rng.integers(1, 16)) * CUT)
    for t in range(10):                                      # many tiny blocks: the block cap decides
        sizes = [int(x) for x in rng.integers(0, 40, 9000)]
        _check(sizes, KS[t % 6], int(rng.integers(1, 200)) * 1000)


def test_bad_arguments():
    for k in (0, 1, 2, 9, -5):
        n, plan = st_batch_plan([10, 20], k, MIB)
        assert n == -1 and plan == [-2, -2], "a refused call writes nothing"
    n, plan = st_batch_plan([10, 20, -1, 10], 5, MIB)
    assert n == -1 and plan == [-2] * 4
