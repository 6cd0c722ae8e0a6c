"""bscgpu_unbwt_batch_plan: which blocks of a decompress batch share an inverse-BWT pass (pure function, no GPU)."""
import numpy as np

from libbsc_amd.gpu import unbwt_batch_plan

MIB = 1 << 20
OWN = -1                             # a block of another route: stored, ST3..ST8, a header that fails


def _limit(cap):
    return min(4096, cap // 256 + 16)


def _check(sizes, cap):
    npass, plan = unbwt_batch_plan(sizes, cap)
    assert len(plan) == len(sizes)
    seen = [p for p in plan if p >= 0]
    assert seen == sorted(seen), "passes follow the input order"
    assert set(seen) == set(range(npass)), "no pass is empty, numbering is dense"
    for p in range(npass):
        members = [b for b in range(len(sizes)) if plan[b] == p]
        assert sum(sizes[b] for b in members) <= cap
        assert len(members) <= _limit(cap)
        # consecutive: only blocks of their own between members
        for b in range(members[0], members[-1] + 1):
            assert plan[b] == p or plan[b] == -1
    for b, n in enumerate(sizes):
        assert (plan[b] >= 0) == (2 <= n <= cap), (b, n)
    return npass, plan


def test_small_blocks_share_passes():
    npass, plan = _check([65536] * 64, 4 * MIB)
    assert npass == 1 and plan == [0] * 64
    npass, plan = _check([65536] * 200, 4 * MIB)
    assert npass == 4


def test_no_size_ceiling_below_the_cap():
    """a large block fills a pass by itself; only blocks above the cap go their own way"""
    npass, plan = _check([1000, 3 * MIB, 6 * MIB, 2000], 4 * MIB)
    assert plan == [0, 0, -1, 0]
    npass, plan = _check([3 * MIB, 6 * MIB, 2 * MIB], 4 * MIB)
    assert plan == [0, -1, 1]
    npass, plan = _check([64 * MIB] * 3, 64 * MIB)
    assert plan == [0, 1, 2]


def test_st_and_stored_routes_do_not_end_a_pass():
    sizes = [5000, OWN, 7000, OWN, OWN, 9000]
    npass, plan = _check(sizes, MIB)
    assert npass == 1 and plan == [0, -1, 0, -1, -1, 0]
    npass, plan = _check([OWN] * 5, MIB)
    assert npass == 0 and plan == [-1] * 5


def test_zero_and_one_byte_blocks():
    npass, plan = _check([0, 100, 1, 0, 200, 2], 1000)
    assert npass == 1 and plan == [-1, 0, -1, -1, 0, 0]
    npass, plan = _check([0, 0, 1], 1000)
    assert npass == 0


def test_block_count_limit():
    npass, plan = _check([16] * 10000, 64 * MIB)            # 4096 per pass
    assert npass == 3
    cap = 64 * 1024                                          # a small context: min(4096, cap / 256 + 16) = 272 blocks per pass
    npass, plan = _check([16] * 1000, cap)
    assert npass == 4 and plan.count(0) == 272


def test_seeded_random():
    rng = np.random.default_rng(11)
    for _ in range(50):
        k = int(rng.integers(0, 400))
        cap = int(rng.integers(1, 64)) * 65536
        sizes = [int(x) for x in rng.integers(0, 2 * cap // 3 + 2, k)]
        for i in rng.integers(0, max(k, 1), k // 4):
            if k:
                sizes[int(i)] = int(rng.choice([OWN, 0, 1]))
        _check(sizes, cap)


def test_bad_arguments():
    out = np.full(3, 77, np.int32)
    from libbsc_amd import _native as N
    L = N.lib()
    sz = np.array([10, -2, 10], np.int32)
    assert L.bscgpu_unbwt_batch_plan(N.np_ptr(sz), 3, MIB, N.np_ptr(out)) == -1
    assert (out == 77).all(), "a refused call wrote something"
    ok = np.array([10, 20], np.int32)
    assert L.bscgpu_unbwt_batch_plan(N.np_ptr(ok), -1, MIB, N.np_ptr(out)) == -1
    assert L.bscgpu_unbwt_batch_plan(None, 2, MIB, N.np_ptr(out)) == -1
    assert L.bscgpu_unbwt_batch_plan(N.np_ptr(ok), 2, MIB, None) == -1
    assert L.bscgpu_unbwt_batch_plan(N.np_ptr(ok), 2, -5, N.np_ptr(out)) == -1
    assert (out == 77).all()
    assert unbwt_batch_plan([], MIB) == (0, [])
