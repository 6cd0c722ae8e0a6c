"""The batched QLFC front end's layout built on the CPU (bscgpu_front_batch_host) and the coding of one block from a layout
(bscgpu_front_batch_code), against the compiled reference.  No GPU."""
import ctypes as C

import numpy as np
import pytest

from front_inputs import KI, host_runs, mixed_batch, raw_second_sub_block, runs_block

NOT_COMPRESSIBLE = -3


def _layout(blocks):
    from libbsc_amd.gpu import front_batch_host
    sizes = [b.size for b in blocks]
    flat = np.concatenate(blocks) if sum(sizes) else np.zeros(1, np.uint8)
    return front_batch_host(flat, sizes)


def _orc_split(a, nb):
    from oracle.refbind import Oracle
    L = Oracle().L
    st, sz = (C.c_int * 8)(), (C.c_int * 8)()
    L.orc_split_blocks.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    L.orc_split_blocks.restype = None
    L.orc_split_blocks(a.ctypes.data, a.size, nb, st, sz)
    return list(st[:nb]), list(sz[:nb])


def test_layout_matches_reference_split_and_ranks(ref):
    from libbsc_amd import api
    blocks = mixed_batch(0)
    fb = _layout(blocks)
    equal_split = 0
    assert fb.blk_sub[0] == 0 and fb.blk_sub[len(blocks)] == fb.nsub and fb.sub_run[fb.nsub] == fb.m
    for b, a in enumerate(blocks):
        s0, s1 = int(fb.blk_sub[b]), int(fb.blk_sub[b + 1])
        want_nb = 0 if a.size == 0 else (1 if a.size < 256 * KI else 2)
        assert s1 - s0 == want_nb, f"block {b} (n={a.size}): {s1 - s0} sub-blocks"
        if want_nb == 0:
            continue
        st, sz = ([0], [a.size]) if want_nb == 1 else _orc_split(a, want_nb)
        assert list(fb.sub_start[s0:s1]) == st and list(fb.sub_size[s0:s1]) == sz, f"block {b} (n={a.size}): split"
        if want_nb == 2:
            # the reference's own split, read from the frame table its coder writes (coder.cpp:121-127)
            blk = ref.coder_compress(a, 1)
            if not isinstance(blk, int):
                got = [int(np.frombuffer(blk[1 + 8 * q:5 + 8 * q], np.int32)[0]) for q in range(2)]
                assert blk[0] == 2 and got == sz, f"block {b}: reference split {got} != {sz}"
            sampled = int(np.count_nonzero(a[1::32] != a[0:a.size - 1:32][:a[1::32].size]))
            equal_split += sampled <= 2
        for q in range(want_nb):
            s = s0 + q
            sub = a[st[q]:st[q] + sz[q]]
            r0, r1 = int(fb.sub_run[s]), int(fb.sub_run[s + 1])
            want_ranks, _ = ref.qlfc_transform(sub)
            assert np.array_equal(fb.rank[r0:r1], want_ranks), f"block {b} sub {q}: ranks"
            sym, start = host_runs(sub)
            assert np.array_equal(fb.sym[r0:r1], sym) and np.array_equal(fb.start[r0:r1], start + st[q]), f"block {b} sub {q}: runs"
            _, first = api.bsc_qlfc_ranks(sub)
            assert np.array_equal(fb.first_seen(s), np.asarray(first, np.uint8)[:fb.nsym[s]]) and fb.nsym[s] == len(first)
    assert equal_split >= 3, "the batch must hold blocks of the equal-split branch"


def _coding_blocks():
    rng = np.random.default_rng(3)
    return [runs_block(rng, 5000, 17), raw_second_sub_block(), rng.integers(0, 256, 300 * KI, dtype=np.uint8),
            runs_block(rng, 300 * KI, 65), rng.integers(0, 256, 5000, dtype=np.uint8), runs_block(rng, 1, 2), runs_block(rng, 29, 2),
            runs_block(rng, 256 * KI - 1, 200, mean_run=2.0), np.zeros(0, np.uint8), runs_block(rng, 700 * KI, 33)]


@pytest.mark.parametrize("features", [1, 3])
@pytest.mark.parametrize("coder", [1, 2, 3])
def test_code_matches_reference_coder(ref, coder, features):
    blocks = _coding_blocks()
    fb = _layout(blocks)
    raw_seen = noise_seen = False
    for b, a in enumerate(blocks):
        if a.size == 0:
            assert fb.code(b, coder, features) == -1
            continue
        want = ref.coder_compress(a, coder, features)
        got = fb.code(b, coder, features)
        assert got == want, f"block {b} (n={a.size}) coder={coder} features={features}: {got if isinstance(got, int) else len(got)} != {want if isinstance(want, int) else len(want)}"
        if b == 1:
            assert not isinstance(got, int) and got[0] == 2
            size1, res1 = (int(x) for x in np.frombuffer(got[9:17], np.int32))
            raw_seen = size1 == res1 and len(got) < a.size
        if b == 2:
            noise_seen = got == NOT_COMPRESSIBLE
    assert raw_seen, "the crafted block's second sub-block must be stored raw inside a block that compresses"
    assert noise_seen, "the all-noise block must be NOT_COMPRESSIBLE"


def test_bad_arguments():
    from libbsc_amd import _native as N
    from libbsc_amd.gpu import FrontBatch
    L = N.lib()
    fb = FrontBatch([10, 20])
    a = np.arange(30, dtype=np.uint8)
    assert L.bscgpu_front_batch_host(N.np_ptr(a), N.np_ptr(fb.sizes), -1, C.byref(fb.lay)) == -1
    assert L.bscgpu_front_batch_host(N.np_ptr(a), N.np_ptr(fb.sizes), 2, None) == -1
    assert L.bscgpu_front_batch_host(None, N.np_ptr(fb.sizes), 2, C.byref(fb.lay)) == -1
    big = FrontBatch([10])
    big.sizes[0] = 1 << 20                                  # a pass holds blocks below BSCGPU_BATCH_MAX_N only
    assert L.bscgpu_front_batch_host(N.np_ptr(a), N.np_ptr(big.sizes), 1, C.byref(big.lay)) == -1
    assert L.bscgpu_front_batch_host(N.np_ptr(a), N.np_ptr(fb.sizes), 2, C.byref(fb.lay)) == 0
    out = np.zeros(5000, np.uint8)
    assert L.bscgpu_front_batch_code(C.byref(fb.lay), 2, N.np_ptr(out), 1, 3) == -1
    assert L.bscgpu_front_batch_code(C.byref(fb.lay), 0, N.np_ptr(out), 9, 3) == -1
    assert L.bscgpu_front_batch_code(None, 0, N.np_ptr(out), 1, 3) == -1
