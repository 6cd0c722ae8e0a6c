"""The static coder's model of a pass on the CPU (no GPU): the stand-in bscgpu_static_pstream_host against the oracle's trace of the
reference model, its streams through the range coder stage against the reference's coded sub-blocks, and the coding of a block
from its sub-blocks' streams (bscgpu_front_batch_code_ps) against bscgpu_front_batch_code and the compiled reference."""
import ctypes as C

import numpy as np
import pytest

import model_batch_inputs as mb
import rc_inputs as ri
from libbsc_amd import gpu


@pytest.fixture(scope="module")
def orc():
    from oracle.refbind import Oracle
    return Oracle()


@pytest.fixture(scope="module")
def mixed():
    blocks = mb.mixed_batch(0)
    fb, _ = mb.layout(blocks)
    ps, poff = mb.host_streams(fb)
    return blocks, fb, ps, poff


def test_stand_in_equals_the_oracle_trace(mixed, orc):
    blocks, fb, ps, poff = mixed
    assert fb.nsub > len(blocks) - 1
    for s in range(fb.nsub):
        sub = mb.sub_bytes(fb, blocks, s)
        want, _ = orc.static_pstream(sub)
        got = ps[int(poff[s]):int(poff[s + 1])]
        assert got.size == want.size, f"sub-block {s} (n={sub.size}): {got.size} decisions, oracle {want.size}"
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, f"sub-block {s} (n={sub.size}): {bad.size} entries differ, first at {int(bad[0])}"
        runs = int(fb.sub_run[s + 1]) - int(fb.sub_run[s])
        assert int(np.count_nonzero(got & (1 << 13))) == runs, f"sub-block {s}: one run-start mark per run"


def test_stand_in_streams_code_to_the_reference_sub_blocks(mixed, ref):
    blocks, fb, ps, poff = mixed
    coded = 0
    for s in range(fb.nsub):
        sub = mb.sub_bytes(fb, blocks, s)
        want = ref.qlfc_encode_block(sub, 1)
        pre = gpu.rc_prefix(fb.first_seen(s), sub.size, 1)
        cnt = int(poff[s + 1]) - int(poff[s])
        res, out = gpu.rc_encode_host(ri.STATIC16, ps, pre, [(int(poff[s]), cnt, 0, len(pre), 0, sub.size)])
        got = res[0] if res[0] < 0 else out[:res[0]].tobytes()
        assert got == want, f"sub-block {s} (n={sub.size})"
        coded += isinstance(want, bytes)
    assert coded >= 20


@pytest.mark.parametrize("features", [1, 3])
def test_code_from_streams_equals_code_from_runs_and_the_reference(mixed, ref, features):
    blocks, fb, ps, poff = mixed
    for b, a in enumerate(blocks):
        if a.size == 0:
            assert gpu.front_batch_code_ps(fb, b, ps, poff, features) == -1
            continue
        got = gpu.front_batch_code_ps(fb, b, ps, poff, features)
        assert got == fb.code(b, 1, features), f"block {b} (n={a.size}) features={features}: differs from front_batch_code"
        assert got == ref.coder_compress(a, 1, features), f"block {b} (n={a.size}) features={features}: differs from the reference"


@pytest.mark.parametrize("features", [1, 3])
def test_code_from_streams_with_a_raw_sub_block(ref, features):
    a = mb.raw_second_sub_block()
    rng = np.random.default_rng(8)
    blocks = [mb.runs_block(rng, 5000, 17), a, rng.integers(0, 256, 5000, dtype=np.uint8)]
    fb, _ = mb.layout(blocks)
    ps, poff = mb.host_streams(fb)
    for b, x in enumerate(blocks):
        got = gpu.front_batch_code_ps(fb, b, ps, poff, features)
        assert got == fb.code(b, 1, features) and got == ref.coder_compress(x, 1, features), f"block {b}"
    got = gpu.front_batch_code_ps(fb, 1, ps, poff, features)
    size1, res1 = (int(x) for x in np.frombuffer(got[9:17], np.int32))
    assert got[0] == 2 and size1 == res1 and len(got) < a.size, "the second sub-block must be stored raw inside a block that compresses"
    assert gpu.front_batch_code_ps(fb, 2, ps, poff, features) == -3, "the noise block is LIBBSC_NOT_COMPRESSIBLE"


def test_bad_arguments(mixed):
    from libbsc_amd import _native as N
    _, fb, ps, poff = mixed
    L = N.lib()
    out = np.zeros(1 << 21, np.uint8)
    e = np.zeros(16, np.uint16)
    assert L.bscgpu_static_pstream_host(None, 0, N.np_ptr(e), 16) == -1
    assert L.bscgpu_static_pstream_host(C.byref(fb.lay), fb.nsub, N.np_ptr(e), 16) == -1
    assert L.bscgpu_static_pstream_host(C.byref(fb.lay), -1, N.np_ptr(e), 16) == -1
    n = int(L.bscgpu_static_pstream_host(C.byref(fb.lay), 0, None, 0))               # counting only
    assert n == int(poff[1]) - int(poff[0])
    assert L.bscgpu_front_batch_code_ps(C.byref(fb.lay), fb.count, N.np_ptr(ps), N.np_ptr(poff), N.np_ptr(out), 3) == -1
    assert L.bscgpu_front_batch_code_ps(C.byref(fb.lay), 0, None, N.np_ptr(poff), N.np_ptr(out), 3) == -1
    assert L.bscgpu_front_batch_code_ps(None, 0, N.np_ptr(ps), N.np_ptr(poff), N.np_ptr(out), 3) == -1


@pytest.mark.parametrize("name", ["mixed", "pass_of_4096", "chain_identity", "long_chain", "fill"])
def test_gpu_inputs_would_not_be_declined_for_avg_rank(name):
    """the passes the GPU tests expect the device to keep: no avg_rank flag may stay undecided (the exit that depends on where the
    pass's run index space is cut into lanes); the two decline passes must trip what their names say"""
    blocks = dict(mixed=lambda: mb.mixed_batch(0), pass_of_4096=mb.pass_of_4096, chain_identity=mb.chain_identity_pass,
                  long_chain=mb.long_chain_pass, fill=mb.fill_pass)[name]()
    fb, _ = mb.layout(blocks)
    assert mb.avg_undecided(fb) == 0
    cap = (2 << 20) if name == "fill" else (16 << 20)                       # the context the GPU test uses
    _, poff = mb.host_streams(fb)
    assert fb.m <= cap and int(poff[-1]) <= 4 * cap, "runs and decisions within the arena's capacity (FAIL_CAP otherwise)"
    if name == "chain_identity":
        assert fb.nsub == 300 and all(int(fb.blk_sub[b]) == b for b in range(301)), "sub-block id = block index"
        for b in range(300):
            has9 = bool((blocks[b] == 99).any())
            assert has9 == (b in mb.CHAIN_NINTH) and (blocks[b].size > 5000) == (b in mb.CHAIN_LONG)


def test_decline_inputs_trip_their_exits():
    fb, _ = mb.layout(mb.fail_avg_pass())
    assert mb.avg_undecided(fb) > 0
    fb, _ = mb.layout(mb.fail_hist_pass())
    assert mb.avg_undecided(fb) == 0
    s = 1                                                                    # the hist_chain block: one sub-block, one symbol with 40000 runs of 2
    r0, r1 = int(fb.sub_run[s]), int(fb.sub_run[s + 1])
    lens = np.diff(np.concatenate([fb.start[r0:r1], [fb.sub_size[s]]]).astype(np.int64))
    sym = fb.sym[r0:r1]
    assert int(np.count_nonzero((sym == sym[1]) & (lens == 2))) > 9216


@pytest.mark.parametrize("kind,sorter", sorted(mb.WHOLE_SEEDS))
def test_whole_call_cases_would_not_be_declined_for_avg_rank(ref, kind, sorter):
    """the sorted blocks of the compress-batch tests' pass, as the reference's own transforms give them"""
    cases = mb.whole_call_cases(mb.WHOLE_SEEDS[kind, sorter])
    Ls = [x if x.size <= 28 else np.ascontiguousarray(ref.bwt_encode(x)[0] if sorter == 1 else ref.st_encode(x, sorter)[0]) for x in cases]
    fb, _ = mb.layout(Ls)
    assert mb.avg_undecided(fb) == 0
    assert fb.m > 0
