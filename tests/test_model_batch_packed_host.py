"""The packed 13-bit stream of a pass on the CPU (no GPU): that the inputs of the GPU tests have the boundary properties their names
promise, the stand-in of the layout (bscgpu_pstream_pack13_host) against rc_inputs.pack_p13 sub-block by sub-block, the layout's
rule and its zero padding, and the coding of a block from the packed stream (bscgpu_front_batch_code_ps13) against
bscgpu_front_batch_code and the compiled reference — a sub-block whose packed stream runs out of its budget included."""
import ctypes as C

import numpy as np
import pytest

import model_batch_inputs as mb
import packed_batch_inputs as pb
import rc_inputs as ri
from libbsc_amd import gpu


# ---- the inputs ----------------------------------------------------------------------------------------------------------------------
def test_boundary_pass_has_the_properties_its_name_promises():
    blocks, fb, _, ps, poff, _, _ = pb.reference("boundary")
    sizes = np.array([b.size for b in blocks])
    small = sizes[sizes < 1000]
    assert 300 <= small.size <= 500 and small.min() == 1 and 380 <= small.max() <= 400 and np.count_nonzero(sizes >= 300 * 1024) == 2
    assert any(b.size > 1 and (b == b[0]).all() for b in blocks), "single-run (constant) blocks"
    dec = np.diff(poff.astype(np.int64))
    assert set(int(x) for x in dec % 8) == set(range(8)), "sub-block decision counts cover every residue modulo 8"
    assert (dec < 8).any(), "a sub-block of fewer than 8 decisions: seven whole zero groups behind its only group"
    assert ((dec % 64 >= 57) & (dec % 64 <= 63)).any(), "a sub-block whose last group is the last of its extent"
    assert ((dec % 64 >= 1) & (dec % 64 <= 56)).any(), "the padding spans whole zero groups"
    starts = fb.sub_run[:-1].astype(np.int64)
    per_wave = np.bincount(starts // pb.WAVE_RUNS)
    assert per_wave.max() >= 10, "some wavefront's 64 runs hold at least ten sub-block starts"
    inner = starts[starts > 0]
    assert (inner % pb.WAVE_RUNS == 0).any() and ((inner % pb.WAVE_RUNS == 0) & (inner % pb.WG_RUNS != 0)).any(), "a sub-block starts on a wavefront's first run"
    assert (inner % pb.WG_RUNS == 0).any(), "... and one on a workgroup's first run"
    assert mb.avg_undecided(fb) == 0
    assert pb.max_wave_decisions(fb, ps, poff) <= pb.DC_PS_STAGE, "every wavefront's piece fits the staging buffer: the packed form is not void"
    assert fb.m <= (2 << 20) and int(poff[-1]) <= 4 * (2 << 20), "within the capacity of the smallest context the tests use"


@pytest.mark.parametrize("name", ["mixed", "pass_of_4096", "chain_identity", "fill", "long_chain"])
def test_kept_passes_fit_the_staging_buffer(name):
    _, fb, _, ps, poff, _, _ = pb.reference(name)
    assert pb.max_wave_decisions(fb, ps, poff) <= pb.DC_PS_STAGE


def test_void_pass_overflows_a_wavefronts_staging_buffer():
    blocks, fb, _, ps, poff, _, _ = pb.reference("void")
    assert len(blocks) == 3 and blocks[1].size < (1 << 20)
    assert mb.avg_undecided(fb) == 0
    nd = pb.run_decisions(fb, ps, poff)
    r0, r1 = int(fb.sub_run[fb.blk_sub[1]]), int(fb.sub_run[fb.blk_sub[2]])
    w = np.arange(nd.size) // pb.WAVE_RUNS
    over = [int(k) for k in np.unique(w) if int(nd[w == k].sum()) > pb.DC_PS_STAGE]
    assert over and all(r0 // pb.WAVE_RUNS <= k <= (r1 - 1) // pb.WAVE_RUNS for k in over), "only wavefronts on the long-run block overflow"


@pytest.mark.parametrize("sorter", [1, 5])
def test_void_text_overflows_after_the_transform(ref, sorter):
    """the whole-call test gives the void case as a TEXT, first in its pass: its transform's first 64 runs must be above the buffer"""
    x = pb.void_text()
    L = np.ascontiguousarray(ref.bwt_encode(x)[0] if sorter == 1 else ref.st_encode(x, sorter)[0])
    fb, _ = mb.layout([L])
    ps, poff = mb.host_streams(fb)
    assert mb.avg_undecided(fb) == 0
    assert int(pb.run_decisions(fb, ps, poff)[:pb.WAVE_RUNS].sum()) > pb.DC_PS_STAGE


# ---- the layout ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["boundary", "mixed", "raw_second"])
def test_pack13_host_is_pack_p13_at_the_layouts_offsets(name):
    _, fb, _, ps, poff, packed, pbase = pb.reference(name)
    assert np.array_equal(pbase, pb.pbase_rule(poff)), "pbase[0] = 0, pbase[s + 1] = pbase[s] + roundup64(poff[s + 1] - poff[s])"
    assert packed.size == int(pbase[-1]) // 8 * 13
    covered = np.zeros(packed.size, bool)
    for s in range(fb.nsub):
        want = ri.pack_p13(ps[int(poff[s]):int(poff[s + 1])])
        at = int(pbase[s]) // 8 * 13
        assert np.array_equal(packed[at:at + want.size], want), f"sub-block {s}"
        covered[at:at + want.size] = True
        assert at + want.size <= int(pbase[s + 1]) // 8 * 13
    assert not packed[~covered].any(), "every byte of the padding is zero"


def test_pack13_host_arguments():
    from libbsc_amd import _native as N
    L = N.lib()
    ps = np.arange(200, dtype=np.uint16)
    poff = np.array([0, 3, 3, 200], np.uint32)
    pbase = np.zeros(4, np.int64)
    out = np.full(1024, 0xa5, np.uint8)
    f = L.bscgpu_pstream_pack13_host
    assert f(N.np_ptr(ps), N.np_ptr(poff), 3, N.np_ptr(out), 10, N.np_ptr(pbase)) == (64 + 256) // 8 * 13, "above cap: counted"
    assert (out == 0xa5).all() and list(pbase) == [0, 64, 64, 320]
    assert f(N.np_ptr(ps), N.np_ptr(poff), 3, N.np_ptr(out), 1024, N.np_ptr(pbase)) == 520
    assert (out[520:] == 0xa5).all()
    assert f(N.np_ptr(ps), None, 3, N.np_ptr(out), 1024, N.np_ptr(pbase)) == -1
    assert f(N.np_ptr(ps), N.np_ptr(poff), 3, N.np_ptr(out), 1024, None) == -1
    assert f(N.np_ptr(ps), N.np_ptr(poff), -1, N.np_ptr(out), 1024, N.np_ptr(pbase)) == -1
    assert f(N.np_ptr(ps), N.np_ptr(np.array([0, 5, 3], np.uint32)), 2, N.np_ptr(out), 1024, N.np_ptr(pbase)) == -1
    assert f(None, N.np_ptr(poff), 0, None, 0, N.np_ptr(pbase)) == 0


# ---- coding from the packed stream ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("features", [1, 3])
@pytest.mark.parametrize("name", ["mixed", "boundary", "raw_second"])
def test_code_from_the_packed_stream_equals_code_from_runs(name, features):
    blocks, fb, _, _, poff, packed, pbase = pb.reference(name)
    for b, a in enumerate(blocks):
        got = gpu.front_batch_code_ps13(fb, b, packed, poff, pbase, features)
        if a.size == 0:
            assert got == -1
            continue
        assert got == fb.code(b, 1, features), f"block {b} (n={a.size}) features={features}: differs from front_batch_code"


def _packed_coder_result(fb, s, nb, packed, poff, pbase):
    """what the packed form's range coder alone says to sub-block s under the budget the framing gives it"""
    pre = gpu.rc_prefix(fb.first_seen(s), int(fb.sub_size[s]), 1)
    room = int(fb.sub_size[s]) - (1 if nb == 1 else 0)
    body = np.concatenate([packed, np.zeros(gpu.P13_SLACK, np.uint8)])
    res, _ = gpu.rc_encode_host(ri.STATIC13, body, pre, [(int(pbase[s]), int(poff[s + 1]) - int(poff[s]), 0, len(pre), 0, room)])
    return res[0]


@pytest.mark.parametrize("features", [1, 3])
def test_sub_block_that_reaches_its_budget_takes_the_references_answer(ref, features):
    """raw_second_sub_block(): the second sub-block is noise.  Its packed stream ends LIBBSC_NOT_COMPRESSIBLE in the packed coder — at
    whatever decision the output filled up, not at the run start where the reference stops — so the block's result must come from
    the host model's second look: equal to the reference's, bytes and return value."""
    blocks, fb, _, _, poff, packed, pbase = pb.reference("raw_second")
    assert fb.nsub == 2
    assert _packed_coder_result(fb, 0, 2, packed, poff, pbase) > 0
    assert _packed_coder_result(fb, 1, 2, packed, poff, pbase) == gpu.NOT_COMPRESSIBLE, "the stream that reaches its budget"
    got = gpu.front_batch_code_ps13(fb, 0, packed, poff, pbase, features)
    want = ref.coder_compress(blocks[0], 1, features)
    assert got == want and isinstance(got, bytes)
    size1, res1 = (int(x) for x in np.frombuffer(got[9:17], np.int32))
    assert got[0] == 2 and size1 == res1 and len(got) < blocks[0].size, "the second sub-block is stored raw inside a block that compresses"
    # ... and a block that is noise altogether: the reference's return value
    rng = np.random.default_rng(8)
    noise = [rng.integers(0, 256, 5000, dtype=np.uint8)]
    nfb, _ = mb.layout(noise)
    nps, npoff = mb.host_streams(nfb)
    npk, npb = gpu.pstream_pack13_host(nps, npoff)
    assert _packed_coder_result(nfb, 0, 1, npk, npoff, npb) == gpu.NOT_COMPRESSIBLE
    assert gpu.front_batch_code_ps13(nfb, 0, npk, npoff, npb, features) == ref.coder_compress(noise[0], 1, features) == gpu.NOT_COMPRESSIBLE


def test_code_ps13_bad_arguments():
    from libbsc_amd import _native as N
    _, fb, _, _, poff, packed, pbase = pb.reference("raw_second")
    L = N.lib()
    out = np.zeros(1 << 21, np.uint8)
    body = np.concatenate([packed, np.zeros(gpu.P13_SLACK, np.uint8)])
    lay, p = C.byref(fb.lay), N.np_ptr
    po, pba = np.ascontiguousarray(poff), np.ascontiguousarray(pbase)
    assert L.bscgpu_front_batch_code_ps13(lay, fb.count, p(body), p(po), p(pba), p(out), 3) == -1
    assert L.bscgpu_front_batch_code_ps13(lay, 0, None, p(po), p(pba), p(out), 3) == -1
    assert L.bscgpu_front_batch_code_ps13(lay, 0, p(body), p(po), None, p(out), 3) == -1
    assert L.bscgpu_front_batch_code_ps13(None, 0, p(body), p(po), p(pba), p(out), 3) == -1
    odd = pba.copy(); odd[1] += 4
    assert L.bscgpu_front_batch_code_ps13(lay, 0, p(body), p(po), p(odd), p(out), 3) == -1, "a body that does not start on a group"
