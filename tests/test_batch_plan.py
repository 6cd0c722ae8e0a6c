"""bscgpu_batch_plan: which blocks of a batch share a suffix-sort pass (pure function, no GPU)."""
import numpy as np

from libbsc_amd.gpu import batch_plan

BWT, ST5 = 1, 5
MIB = 1 << 20
CUT = 1 << 20                       # BSCGPU_BATCH_MAX_N


def _check(sizes, sorter, cap):
    npass, plan = batch_plan(sizes, sorter, cap)
    assert len(plan) == len(sizes)
    seen = [p for p in plan if p >= 0]
    assert seen == sorted(seen), "passes follow the input order"
    assert set(seen) == set(range(npass)), "no pass is empty, numbering is dense"
    for p in range(npass):
        members = [b for b in range(len(sizes)) if plan[b] == p]
        assert sum(sizes[b] for b in members) <= cap
        assert len(members) <= 4096
        # one contiguous range of the input: only empty blocks between members
        for b in range(members[0], members[-1] + 1):
            assert plan[b] == p or sizes[b] == 0
    for b, n in enumerate(sizes):
        if sorter != BWT or n >= CUT or n == 0 or n > cap:
            assert plan[b] == -1
        else:
            assert plan[b] >= 0
    return npass, plan


def test_small_blocks_share_passes():
    npass, plan = _check([65536] * 64, BWT, 4 * MIB)
    assert npass == 1 and plan == [0] * 64
    npass, plan = _check([65536] * 200, BWT, 4 * MIB)
    assert npass == 4


def test_threshold_and_sorter_route_to_single_path():
    sizes = [1000, CUT - 1, CUT, 2 * MIB, 5000]
    npass, plan = _check(sizes, BWT, 64 * MIB)
    assert plan == [0, 0, -1, -1, 1]
    npass, plan = _check(sizes, ST5, 64 * MIB)
    assert npass == 0 and plan == [-1] * 5


def test_zero_sizes_and_oversized():
    sizes = [0, 100, 0, 0, 200, 0]
    npass, plan = _check(sizes, BWT, 1000)
    assert npass == 1 and plan == [-1, 0, -1, -1, 0, -1]
    npass, plan = _check([0, 0, 0], BWT, 1000)
    assert npass == 0
    npass, plan = _check([500, 2000, 500], BWT, 1000)        # larger than the cap: a block of its own
    assert plan == [0, -1, 1]


def test_block_count_cap():
    npass, plan = _check([16] * 10000, BWT, 64 * MIB)
    assert npass == 3


def test_seeded_random():
    rng = np.random.default_rng(7)
    for _ in range(50):
        k = int(rng.integers(0, 300))
        sizes = [int(x) for x in rng.integers(0, 2 * CUT, k)]
        for i in rng.integers(0, max(k, 1), k // 5):
            if k:
                sizes[int(i)] = 0
        _check(sizes, BWT, int(rng.integers(1, 16)) * CUT)


def test_bad_arguments():
    n, _ = batch_plan([10, -1, 10], BWT, MIB)
    assert n == -1
