"""A single block modelled in sub-block segments on a context whose device-model arena is divided (BSCGPU_OPT_DC_ARENA_DIV; DESIGN §3.6,
"A block in sub-block segments"): the facts the plan is made of, the stream of every divisor against the undivided context's — both
forms, the void packed segment, the three exact resolves on —, whole blocks against the compiled reference, a pipe, the same through
the sender's events route (BSC_D2H_DMA=0, a child process), the capacity exit, the arena's size and the option's semantics.  Segment counts are computed from the facts by bscgpu_block_segment_plan, never written down."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import block_segment_inputs as bs
import devcoder_inputs as di
import resolve_combined_inputs as rci
from libbsc_amd import GpuContext
from libbsc_amd.gpu import GpuError, block_segment_plan, pstream_pack13_host

pytestmark = pytest.mark.gpu
BAD_PARAMETER, NOT_SUPPORTED = -1, -4


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but torch.cuda.is_available() is False")
    return torch


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    d = tmp_path_factory.mktemp("block_segments")
    exe = di.build_probe(d)
    return lambda L: bs.stand_in_facts(exe, L, d)


def _ctx(max_n, k=1, options=()):
    c = GpuContext(0, max_n=max_n)
    if k != 1:
        assert c.option_set(c.OPT_DC_ARENA_DIV, k) == 1
    for o in options:
        c.option_set(o, 1)
    return c


_SORTED = {}


def _sorted_block(name):
    """the BWT of a text block (computed on the GPU once per process, shared and never written)"""
    if name not in _SORTED:
        T = bs.text(name)
        c = GpuContext(0, max_n=T.size)
        try:
            L = c.bwt(T)[0].copy()
        finally:
            c.close()
        L.setflags(write=False)
        _SORTED[name] = L
    return _SORTED[name]


_WHOLE = {}


def _whole(key, L, options=()):
    """the undivided context's streams of L: (entries, sub_start, sub_size, poff, packed result or the GpuError code, avg_undecided)"""
    if key not in _WHOLE:
        c = _ctx(L.size, 1, options)
        try:
            ent, st, sz, poff, _ = c.qlfc_static_pstream(L)
            und = c.option_get(c.CNT_DC_AVG_UNDECIDED)
            assert c.option_get(c.CNT_DC_BLOCK_SEGMENTS) == 0, "an undivided arena: the whole-block route, no facts"
            try:
                packed = c.qlfc_static_pstream_packed(L)
            except GpuError as e:
                packed = e.code
            ent = ent.copy()
            ent.setflags(write=False)
        finally:
            c.close()
        _WHOLE[key] = (ent, st, sz, poff, packed, und)
    return _WHOLE[key]


def _used_bytes(packed_bytes, poff, pbase):
    """the bytes of a packed stream that hold decisions: per sub-block its groups of eight (the rest of its padded extent is nobody's)"""
    return [bytes(packed_bytes[pbase[b] // 8 * 13: pbase[b] // 8 * 13 + (poff[b + 1] - poff[b] + 7) // 8 * 13]) for b in range(len(poff) - 1)]


def _plan_of(c, facts):
    mcap, dcap = bs.capacity(c.max_n, c.option_get(c.OPT_DC_ARENA_DIV))
    assert c.option_get(c.CNT_DC_DCAP) == dcap
    _, _, runs, dec, _ = facts
    return block_segment_plan(runs, dec, mcap, dcap)


# ---- facts ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(bs.SIZES))
def test_facts(name, probe):
    L = _sorted_block(name)
    ent, st, sz, poff, _, und_total = _whole(name, L)
    c = _ctx(L.size)
    try:
        f_st, f_sz, runs, dec, und = c.qlfc_pstream_facts(L, 1)
        fast = c.qlfc_pstream_facts(L, 3)
    finally:
        c.close()
    assert len(dec) == {"1m+1": 2, "4m": 4, "16m": 8}[name]
    assert (f_st, f_sz) == (st, sz)
    assert dec == [poff[b + 1] - poff[b] for b in range(len(dec))], "the poff differences of the whole block's stream"
    want_runs, want_dec, want_und = probe(L)
    assert runs == want_runs and dec == want_dec, "the CPU stand-in's counts"
    assert und == want_und and sum(und) == und_total
    # the fast coder: the same runs, no flags, counts of its own (max_rank 7 everywhere)
    assert fast[2] == runs and fast[4] == [0] * len(runs) and all(d > 0 for d in fast[3])


def test_facts_of_open_flags(probe):
    """a block whose first sub-block leaves avg_rank flags open: counted per sub-block as the stand-in counts them, and the divided
    context declines it before any segment runs, as the undivided one declines it at its first sync"""
    L = rci.block("all_concat")
    want_runs, want_dec, want_und = probe(L)
    assert sum(want_und) > 0
    for k in (1, 2):
        c = _ctx(2 * L.size, k)
        try:
            _, _, runs, dec, und = c.qlfc_pstream_facts(L, 1)
            assert (runs, dec, und) == (want_runs, want_dec, want_und)
            with pytest.raises(GpuError) as e:
                c.qlfc_static_pstream(L)
            # (the undivided context judges every exit of its first sync together and may name more reasons; the divided one stops at the facts)
            fail = c.option_get(c.CNT_DC_LAST_FAIL)
            assert e.value.code == NOT_SUPPORTED and (fail == c.DC_FAIL_AVG if k > 1 else fail & c.DC_FAIL_AVG)
            assert c.option_get(c.CNT_DC_AVG_UNDECIDED) == sum(und) and c.option_get(c.CNT_DC_BLOCK_SEGMENTS) == 0
        finally:
            c.close()


def test_facts_fast_coder_through_compress(ref, torch_cuda):
    """-e0: the segments a whole block runs in are the plan of its facts (the stage has no -e0 stream to compare poff with)"""
    name = "4m"
    T = bs.text(name)
    c = _ctx(T.size, 4)
    try:
        facts = c.qlfc_pstream_facts(_sorted_block(name), 3)
        nseg, _ = _plan_of(c, facts)
        got = c.compress_device(torch_cuda.from_numpy(T).cuda(), T.size, 1, 3).tobytes()
        assert c.option_get(c.CNT_DC_BLOCK_SEGMENTS) == nseg > 1 and c.option_get(c.CNT_DC_LAST_FAIL) == 0
    finally:
        c.close()
    assert got == _reference(ref, name, 1, 3)


# ---- stream identity -----------------------------------------------------------------------------------------------------------------
def _check_identity(c, L, whole, allow_cap_exit):
    """both forms of the divided context c against the whole block's -> (segments, packed-void segments)"""
    ent, st, sz, poff, packed, _ = whole
    facts = c.qlfc_pstream_facts(L, 1)
    try:
        nseg, seg_of = _plan_of(c, facts)
    except GpuError as e:
        assert allow_cap_exit and e.code == NOT_SUPPORTED
        with pytest.raises(GpuError) as e2:
            c.qlfc_static_pstream(L)
        assert e2.value.code == NOT_SUPPORTED and c.option_get(c.CNT_DC_LAST_FAIL) == c.DC_FAIL_CAP and c.option_get(c.CNT_DC_BLOCK_SEGMENTS) == 0
        return 0, 0
    got = c.qlfc_static_pstream(L)
    assert c.option_get(c.CNT_DC_BLOCK_SEGMENTS) == nseg and c.option_get(c.CNT_DC_LAST_FAIL) == 0
    assert got[1:4] == (st, sz, poff) and np.array_equal(got[0], ent)
    void0 = c.option_get(c.CNT_BATCH_PACKED_VOID)
    fields, st2, sz2, poff2, pbase2, pbytes = c.qlfc_static_pstream_packed(L)
    void = c.option_get(c.CNT_BATCH_PACKED_VOID) - void0
    assert c.option_get(c.CNT_DC_BLOCK_SEGMENTS) == nseg
    assert (st2, sz2, poff2) == (st, sz, poff) and np.array_equal(fields, ent & 0x1fff)
    want_bytes, want_pbase = pstream_pack13_host(ent, poff)
    assert pbase2 == [int(x) for x in want_pbase]
    assert _used_bytes(pbytes, poff, pbase2) == _used_bytes(want_bytes, poff, pbase2)
    if not isinstance(packed, int):
        assert pbase2 == packed[4] and _used_bytes(pbytes, poff, pbase2) == _used_bytes(packed[5], poff, pbase2), "the whole block's packed bytes"
        assert void == 0 or nseg == 1
    return nseg, void


@pytest.mark.parametrize("k", bs.DIVISORS)
@pytest.mark.parametrize("name", list(bs.SIZES))
def test_stream_identity(name, k):
    L = _sorted_block(name)
    c = _ctx(L.size, k)
    try:
        nseg, _ = _check_identity(c, L, _whole(name, L), allow_cap_exit=True)
        if (name, k) == ("16m", 2):
            # a segment of several sub-blocks followed by a shorter one
            _, seg_of = _plan_of(c, c.qlfc_pstream_facts(L, 1))
            sizes = [seg_of.count(i) for i in range(nseg)]
            assert nseg >= 2 and sizes[0] > 1 and sizes[-1] < sizes[0], sizes
    finally:
        c.close()


def test_uneven_sub_blocks_and_a_void_packed_segment():
    L = bs.uneven_block()
    whole = _whole("uneven", L)
    assert whole[4] == NOT_SUPPORTED, "run whole, the block's packed form is void"
    c = _ctx(L.size, 4)
    try:
        _, sz, runs, dec, _ = c.qlfc_pstream_facts(L, 1)
        assert max(sz) > 4 * min(sz), (sz, runs, dec)
        nseg, void = _check_identity(c, L, whole, allow_cap_exit=False)
        assert nseg >= 2 and 1 <= void < nseg, "some segments went down packed, the one with the long runs was packed by the host"
    finally:
        c.close()


def test_with_the_three_exact_resolves_on():
    L = rci.block("all_concat")
    probe_ctx = GpuContext(0, max_n=L.size)
    options = (probe_ctx.OPT_DC_AVG_EXACT, probe_ctx.OPT_DC_HIST_EXACT, probe_ctx.OPT_DC_REPLAY_EXACT)
    try:
        for o in options:
            probe_ctx.option_set(o, 1)
        facts = probe_ctx.qlfc_pstream_facts(L, 1)
    finally:
        probe_ctx.close()
    # max_n: the smallest multiple of an eighth of the block, from the block's size on, at which the plan of k = 4 has several segments
    max_n = next((n for n in range(L.size, 8 * L.size, L.size // 8) if _segments(facts, *bs.capacity(n, 4)) >= 2), None)
    assert max_n is not None, facts
    whole = _whole("all_concat/exact", L, options)
    c = _ctx(max_n, 4, options)
    try:
        nseg, _ = _check_identity(c, L, whole, allow_cap_exit=False)
        assert nseg >= 2
    finally:
        c.close()


def _segments(facts, mcap, dcap):
    try:
        return block_segment_plan(facts[2], facts[3], mcap, dcap)[0]
    except GpuError:
        return 0


# ---- whole blocks --------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _reference_bytes(name, sorter, coder, _ref):
    return _ref.compress(bs.text(name), sorter, coder)


def _reference(ref, name, sorter, coder):
    return _reference_bytes(name, sorter, coder, ref)


def _process_counters():
    from libbsc_amd import _native as N
    lib = N.lib()
    lib.bscgpu_process_counter.restype = C.c_longlong
    lib.bscgpu_process_counter.argtypes = [C.c_int]
    return [lib.bscgpu_process_counter(k) for k in (1, 2)]           # BSCGPU_PCNT_DEVICE_MODEL_BLOCKS, _REDONE_ON_HOST_MODEL


@pytest.mark.parametrize("coder", [1, 3])
@pytest.mark.parametrize("sorter", [1, 5])
@pytest.mark.parametrize("name", ["4m", "16m"])
def test_whole_blocks_match_the_reference(ref, torch_cuda, name, sorter, coder):
    T = bs.text(name)
    c = _ctx(T.size, 4)
    try:
        before = _process_counters()
        got = c.compress_device(torch_cuda.from_numpy(T).cuda(), T.size, sorter, coder).tobytes()
        after = _process_counters()
        assert c.option_get(c.CNT_DC_BLOCK_SEGMENTS) >= 2 and c.option_get(c.CNT_DC_LAST_FAIL) == 0
    finally:
        c.close()
    assert got == _reference(ref, name, sorter, coder)
    assert after[0] == before[0] + 1 and after[1] == before[1]


def test_pipe_of_depth_3(torch_cuda):
    """four 4 MiB blocks in flight on one context: the two stream buffers' guards across segments and across blocks"""
    texts = bs.pipe_texts()
    out = {}
    for k in (1, 4):
        c = _ctx(4 * bs.MIB, k)
        try:
            pipe = c.pipe(3)
            d = [torch_cuda.from_numpy(T).cuda() for T in texts]
            tickets = [pipe.submit(d[i], texts[i].size, 1, 1) for i in range(3)]
            res = [pipe.wait(tickets[0]).tobytes()]
            tickets.append(pipe.submit(d[3], texts[3].size, 1, 1))
            res += [pipe.wait(t).tobytes() for t in tickets[1:]]
            pipe.close()
            if k == 4:
                assert c.option_get(c.CNT_DC_BLOCK_SEGMENTS) >= 2
        finally:
            c.close()
        out[k] = res
    assert out[4] == out[1]


def test_two_sub_blocks_at_divisor_2(ref, torch_cuda):
    """the smallest block in segments: two sub-blocks, one segment each"""
    name = "1m+1"
    T = bs.text(name)
    c = _ctx(T.size, 2)
    try:
        got = c.compress_device(torch_cuda.from_numpy(T).cuda(), T.size, 1, 1).tobytes()
        assert c.option_get(c.CNT_DC_BLOCK_SEGMENTS) == 2 and c.option_get(c.CNT_DC_LAST_FAIL) == 0
    finally:
        c.close()
    assert got == _reference(ref, name, 1, 1)


def test_events_route_of_the_sender(torch_cuda):
    """BSC_D2H_DMA=0 keeps hipMemcpyAsync on the copy stream and an event per piece (block.cpp: PsSender), for a block in segments as for a
    whole one: several segments at divisor 4, two at divisor 2, and the pipe, where a stream buffer is reused behind an event guard —
    in a child process, the switch being read once"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    selection = "(whole_blocks_match_the_reference and 4m) or pipe_of_depth_3 or two_sub_blocks_at_divisor_2"
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(root, "tests", "test_gpu_block_segments.py"), "-q", "-x", "-k", selection],
                       capture_output=True, text=True, env=dict(os.environ, BSC_D2H_DMA="0"), cwd=root)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "6 passed" in r.stdout, r.stdout[-2000:]


# ---- the capacity exit -----------------------------------------------------------------------------------------------------------------
def test_capacity_exit(ref, torch_cuda, probe):
    name, k = "4m", 8
    L, T = _sorted_block(name), bs.text(name)
    mcap, dcap = bs.capacity(T.size, k)
    runs, dec, _ = probe(L)
    assert all(d > dcap for d in dec), "every sub-block alone exceeds the decisions the arena holds (the stand-in's counts)"
    c = _ctx(T.size, k)
    try:
        with pytest.raises(GpuError) as e:
            _plan_of(c, c.qlfc_pstream_facts(L, 1))
        assert e.value.code == NOT_SUPPORTED
        before = _process_counters()
        got = c.compress_device(torch_cuda.from_numpy(T).cuda(), T.size, 1, 1).tobytes()
        assert c.option_get(c.CNT_DC_LAST_FAIL) == c.DC_FAIL_CAP and c.option_get(c.CNT_DC_BLOCK_SEGMENTS) == 0
        assert _process_counters() == before, "the host model, not a redo"
    finally:
        c.close()
    assert got == _reference(ref, name, 1, 1)


# ---- the arena -------------------------------------------------------------------------------------------------------------------------
def test_arena_is_a_quarter():
    """max_n 16 MiB: the model's arena after the first model block (bscgpu_model_arena_bytes: bscgpu_arena_bytes has never counted this
    arena, and tests hold it to that) at k = 4 against k = 1.  What does not scale: cnt (1088 x 4096 x 4 B = 17.8 MB), the other
    fixed tables (under 1 MB), ge32 (a byte per run of the whole block: 16 MiB) and alignment — 64 MiB bounds them."""
    L = _sorted_block("4m")
    arena = {}
    for k in (1, 4):
        c = _ctx(16 * bs.MIB, k)
        try:
            assert c.model_arena_bytes == 0
            c.qlfc_static_pstream(L)
            arena[k] = c.model_arena_bytes
        finally:
            c.close()
    assert arena[1] > 200 * 16 * bs.MIB, "about 221 bytes per byte of max_n"
    assert arena[4] <= arena[1] // 4 + 64 * bs.MIB, arena


# ---- the option ------------------------------------------------------------------------------------------------------------------------
def test_option_semantics(monkeypatch):
    L = _sorted_block("1m+1")
    c = GpuContext(0, max_n=L.size)
    try:
        assert c.option_get(c.OPT_DC_ARENA_DIV) == 1, "the default"
        assert c.option_set(c.OPT_DC_ARENA_DIV, 4) == 1 and c.option_set(c.OPT_DC_ARENA_DIV, 2) == 4, "set before first use returns the previous value"
        for bad in (0, 3, 16, -1):
            with pytest.raises(GpuError) as e:
                c.option_set(c.OPT_DC_ARENA_DIV, bad)
            assert e.value.code == BAD_PARAMETER and c.option_get(c.OPT_DC_ARENA_DIV) == 2
        with pytest.raises(GpuError) as e:
            c.option_set(c.CNT_DC_BLOCK_SEGMENTS, 1)
        assert e.value.code == BAD_PARAMETER, "get only"
        c.qlfc_static_pstream(L)                                   # the arena exists from here on
        assert c.option_get(c.CNT_DC_BLOCK_SEGMENTS) == 2
        with pytest.raises(GpuError) as e:
            c.option_set(c.OPT_DC_ARENA_DIV, 4)
        assert e.value.code == NOT_SUPPORTED and c.option_get(c.OPT_DC_ARENA_DIV) == 2
        assert c.option_set(c.OPT_DC_ARENA_DIV, 2) == 2, "the value the arena was carved by"
    finally:
        c.close()
    monkeypatch.setenv("BSC_DC_ARENA_DIV", "8")
    c = GpuContext(0, max_n=L.size)
    try:
        assert c.option_get(c.OPT_DC_ARENA_DIV) == 8 and c.option_get(c.CNT_DC_DCAP) == bs.capacity(L.size, 8)[1]
    finally:
        c.close()
