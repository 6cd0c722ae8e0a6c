"""Open avg_rank flags resolved exactly on the GPU (BSCGPU_OPT_DC_AVG_EXACT; devcoder.hip 1a'): with the option on a block, a pass or a
segment whose bracket leaves flags open is not declined — the counters say how many flags were open (the CPU probes' count) and that
all of them were settled, and the streams and bytes equal the references'.  Inputs: avg_resolve_inputs.py (each checked on the CPU by
test_avg_resolve_host.py to leave flags open), devcoder_inputs.py, model_batch_inputs.py.  Everything is bit-exact."""
import ctypes as C

import numpy as np
import pytest

import avg_resolve_inputs as ar
import devcoder_inputs as di
import model_batch_inputs as mb
import model_segment_inputs as ms
from front_inputs import layouts_equal

pytestmark = pytest.mark.gpu

CTX_N = (16 << 20) + 4096
NOT_SUPPORTED = -4


@pytest.fixture(scope="module")
def ctx():
    from libbsc_amd import GpuContext
    c = GpuContext(0, max_n=CTX_N)
    yield c
    c.close()


@pytest.fixture
def on(ctx):
    """the module's context with the option on for one test"""
    old = ctx.option_set(ctx.OPT_DC_AVG_EXACT, 1)
    assert old == 0, "the default"
    yield ctx
    ctx.option_set(ctx.OPT_DC_AVG_EXACT, old)


@pytest.fixture(scope="module")
def probes(tmp_path_factory):
    d = tmp_path_factory.mktemp("avg_probes")
    exe, pexe = ar.build_probe(d), di.build_probe(d)
    return (lambda L: ar.probe_block(exe, d, L)), (lambda L: di.run_probe(pexe, L, d))


def _avg_counters(ctx):
    return dict(fail=ctx.option_get(ctx.CNT_DC_LAST_FAIL), und=ctx.option_get(ctx.CNT_DC_AVG_UNDECIDED), resolved=ctx.option_get(ctx.CNT_DC_AVG_RESOLVED))


def _stage_equals_oracle(ctx, probes, name, L):
    """bscgpu_qlfc_static_pstream with the option on: kept, the bracket's count is the paths probe's, all of it resolved, and every
    sub-block's stream is the oracle's trace of the reference model (what test_gpu_devcoder_paths.py holds its avg_decides cases to)"""
    from oracle.refbind import Oracle
    v, p = probes[0](L), probes[1](L)
    assert p["fail_mask"] == di.FAIL_AVG and p["avg_und"] == v["und"] > 0 and v["resolved"] == v["und"], (name, p["fail_mask"], p["avg_und"], v)
    ps, st, sz, poff, _ = ctx.qlfc_static_pstream(L)
    got = _avg_counters(ctx)
    print(f"{name}: probe und {p['avg_und']} chunks {v['chunks']} chain steps {v['chain_steps']} | gpu {got}")
    assert got == dict(fail=0, und=p["avg_und"], resolved=p["avg_und"]), (name, got)
    assert poff[0] == 0 and poff[-1] == len(ps) == p["decisions"] and len(st) == p["nb"], name
    orc = Oracle()
    for b in range(len(st)):
        tr, _ = orc.static_pstream(L[st[b]:st[b] + sz[b]], counters=False)
        mine = ps[poff[b]:poff[b + 1]]
        assert np.array_equal(tr, mine), (name, b, int(np.argmax(tr != mine)) if tr.size == mine.size else (tr.size, mine.size))
    return p


GENERATOR_BLOCKS = {"rank32": lambda: di.const_rank(32, 5000), "rank62": lambda: di.const_rank(62, 5000),
                    "rank40_warm_front_255": di.GENERATORS["rank40_warm_front_255"][2], "rank40_warm_1856": di.GENERATORS["rank40_warm_1856"][2]}


@pytest.mark.parametrize("name", list(GENERATOR_BLOCKS))
def test_generator_blocks_stay_on_the_device(ctx, probes, name):
    """the generators tagged fail_avg, a few thousand runs each: declined today (the switch does something), kept with the option on"""
    from libbsc_amd.gpu import GpuError
    L = GENERATOR_BLOCKS[name]()
    assert ctx.option_get(ctx.OPT_DC_AVG_EXACT) == 0
    with pytest.raises(GpuError) as e:
        ctx.qlfc_static_pstream(L)
    assert e.value.code == NOT_SUPPORTED
    off = _avg_counters(ctx)
    assert off["fail"] == ctx.DC_FAIL_AVG and off["und"] > 0 and off["resolved"] == 0
    old = ctx.option_set(ctx.OPT_DC_AVG_EXACT, 1)
    try:
        p = _stage_equals_oracle(ctx, probes, name, L)
        assert p["avg_und"] == off["und"], "_AVG_UNDECIDED keeps its meaning: what the bracket left open"
        # the packed form of the same stage
        ps, *_ = ctx.qlfc_static_pstream(L)
        try:
            f, *_ = ctx.qlfc_static_pstream_packed(L)
        except GpuError as e2:                                         # a refusal of the FORM leaves the reason mask at 0
            assert e2.code == NOT_SUPPORTED and ctx.option_get(ctx.CNT_DC_LAST_FAIL) == 0, name
        else:
            assert np.array_equal(f, ps & 0x1fff) and _avg_counters(ctx) == dict(fail=0, und=p["avg_und"], resolved=p["avg_und"])
    finally:
        ctx.option_set(ctx.OPT_DC_AVG_EXACT, old)


@pytest.mark.parametrize("runs,sub_runs", [(ar.LONG_RUNS, None), (ar.LONG_RUNS_TWO, ar.LONG_TWO_SUB_RUNS)])
def test_long_open_stretch_chains_groups(on, probes, runs, sub_runs):
    """constant rank 40, every chunk open from the sub-block's first run to its last: 196 chunks in one sub-block, and 264 in two whose
    second starts in the middle of a chunk — more than DC_AVG_GROUP chunks either way, so groups are composed and chained"""
    L = di.const_rank(40, runs)
    p = _stage_equals_oracle(on, probes, f"const_rank(40, {runs})", L)
    assert p["runs"] > 2 * 64 * 1024 and (sub_runs is None or p["sub_runs"] == sub_runs)


def test_varying_ranks_equal_the_host_stand_in(on, probes):
    """kind (b), m = 20 000: the start brackets differ from chunk to chunk, and so do the maps"""
    L = ar.stretches_block()
    v = probes[0](L)
    assert v["und"] > 10_000
    fb, _ = mb.layout([L])
    want_ps, want_poff = mb.host_streams(fb)
    ps, st, sz, poff, _ = on.qlfc_static_pstream(L)
    assert _avg_counters(on) == dict(fail=0, und=v["und"], resolved=v["und"])
    assert list(poff) == [int(x) for x in want_poff] and np.array_equal(ps, want_ps)


# ---- whole blocks -----------------------------------------------------------------------------------------------------------------
def _process_counters():
    from libbsc_amd import _native
    lib = _native.lib()
    lib.bscgpu_process_counter.restype = C.c_longlong
    lib.bscgpu_process_counter.argtypes = [C.c_int]
    return [lib.bscgpu_process_counter(k) for k in (1, 2)]           # BSCGPU_PCNT_DEVICE_MODEL_BLOCKS, _REDONE_ON_HOST_MODEL


@pytest.mark.parametrize("name", ["fail_avg", "realistic"])
def test_whole_block_takes_the_device_model(ref, probes, name):
    """bsc_compress's route (compress_device, and the pipe) on a text whose BWT leaves flags open: with the option on the block is a
    device-model block, nothing is redone on the host model and the bytes are the reference's; with it off the same block declines"""
    import torch
    from libbsc_amd import GpuContext
    T = di.text_with_bwt_like(di.WHOLE_BLOCKS["fail_avg"][2]()) if name == "fail_avg" else ar.realistic_text()
    L, _, _ = ref.bwt_encode(T)
    p = probes[1](L)
    assert p["fail_mask"] == di.FAIL_AVG and p["avg_und"] > 0 and T.size >= 1 << 20 and p["nb"] >= 2 and p["runs"] <= 0.70 * T.size
    want = ref.compress(T, 1, 1)
    c = GpuContext(0, max_n=max(T.size, p["decisions"]) + 4096)
    try:
        d = torch.from_numpy(T).cuda()
        c0 = _process_counters()
        assert c.compress_device(d, T.size, 1, 1).tobytes() == want
        c1 = _process_counters()
        assert _avg_counters(c) == dict(fail=di.FAIL_AVG, und=p["avg_und"], resolved=0) and c1[0] == c0[0], "option off: declined as today"
        c.option_set(c.OPT_DC_AVG_EXACT, 1)
        assert c.compress_device(d, T.size, 1, 1).tobytes() == want
        c2 = _process_counters()
        got = _avg_counters(c)
        print(f"{name}: probe und {p['avg_und']} | gpu {got}, device-model blocks +{c2[0] - c1[0]}, redone on the host model +{c2[1] - c1[1]}")
        assert got == dict(fail=0, und=p["avg_und"], resolved=p["avg_und"])
        assert c2[0] == c1[0] + 1 and c2[1] == c1[1]
        pipe = c.pipe(2)
        try:
            t = pipe.submit(d, T.size, 1, 1)
            assert pipe.wait(t).tobytes() == want
        finally:
            pipe.close()
        c3 = _process_counters()
        assert c3[0] == c2[0] + 1 and c3[1] == c2[1] and _avg_counters(c)["resolved"] == p["avg_und"]
    finally:
        c.close()


# ---- the batched pass ---------------------------------------------------------------------------------------------------------------
def _first_difference(ps, want_ps, want_poff):
    w = np.flatnonzero(ps != want_ps)
    s = int(np.searchsorted(want_poff, w[0], side="right")) - 1
    return f"{w.size} of {ps.size} entries differ, first at {int(w[0])} (sub-block {s}): {int(ps[w[0]]):#x} != {int(want_ps[w[0]]):#x}"


def test_pass_is_kept_and_equals_the_stand_in(on):
    import torch
    _, want, flat, want_ps, want_poff = ms.reference("fail_avg", ms.STATIC)
    und = mb.avg_undecided(want)
    assert und > 0
    fb, ps, poff = on.static_pstream_batch(torch.from_numpy(flat).cuda(), want.sizes)
    assert _avg_counters(on) == dict(fail=0, und=und, resolved=und)
    assert not layouts_equal(fb, want)
    assert np.array_equal(poff, want_poff) and ps.size == want_ps.size
    assert np.array_equal(ps, want_ps), _first_difference(ps, want_ps, want_poff)


def test_pass_packed_form(on):
    import torch
    from libbsc_amd.gpu import pstream_pack13_host
    _, want, flat, want_ps, want_poff = ms.reference("fail_avg", ms.STATIC)
    want_bytes, want_pbase = pstream_pack13_host(want_ps, want_poff)
    _, packed, poff, pbase = on.static_pstream_batch_packed(torch.from_numpy(flat).cuda(), want.sizes)
    assert _avg_counters(on)["fail"] == 0 and _avg_counters(on)["resolved"] == mb.avg_undecided(want)
    assert np.array_equal(poff, want_poff) and np.array_equal(pbase, want_pbase) and np.array_equal(packed, want_bytes)


def test_segments_exclude_no_block_for_its_flags(on):
    import torch
    _, want, flat, want_ps, want_poff = ms.reference("fail_avg", ms.STATIC)
    d = torch.from_numpy(flat).cuda()
    keys = (on.CNT_BATCH_SEGMENTS, on.CNT_BATCH_SEG_RERUNS, on.CNT_BATCH_SEG_HOST_BLOCKS)
    fb, dec, und = on.model_segment_facts(d, want.sizes, ms.STATIC)
    assert not und.any(), "sub_und: what is left behind the resolve"
    assert np.array_equal(dec, np.diff(want_poff.astype(np.int64))), "resolved flags: every sub-block's count is exact"
    c0 = [on.option_get(k) for k in keys]
    fb, ps, poff, state = on.pstream_batch_segments(d, want.sizes, ms.STATIC, 0)
    moved = [on.option_get(k) - a for k, a in zip(keys, c0)]
    assert list(state) == [0, 0, 0] and moved == [1, 0, 0], "one segment, no re-run, no block left to the host"
    und_total = mb.avg_undecided(want)
    assert _avg_counters(on) == dict(fail=0, und=und_total, resolved=und_total)
    assert np.array_equal(poff, want_poff) and ps.size == want_ps.size
    assert np.array_equal(ps, want_ps), _first_difference(ps, want_ps, want_poff)


def test_compress_batch_in_segments_keeps_every_block(on, ref, monkeypatch):
    """the call of test_gpu_model_segments.test_block_that_declined_its_pass_now_leaves_alone: no block leaves"""
    from libbsc_amd.synth import synth_text_v1
    monkeypatch.setenv("BSC_BATCH_MODEL_MIN_PASS", "0")
    bad = di.text_with_bwt_like(di.runs_to_block(di.const_rank(40, 200_000), np.tile([1, 1, 2, 4], 50_000)))
    cases = [synth_text_v1(81, 700 * 1024), bad, synth_text_v1(82, 300 * 1024)]
    keys = (on.CNT_BATCH_MODEL_PASSES, on.CNT_BATCH_MODEL_DECLINED, on.CNT_BATCH_SEG_HOST_BLOCKS)
    old = on.option_set(on.OPT_BATCH_MODEL, 1), on.option_set(on.OPT_BATCH_MODEL_SEGMENTS, 1)
    try:
        c0 = [on.option_get(k) for k in keys]
        got = on.compress_batch(cases, 1, 1)
        moved = [on.option_get(k) - a for k, a in zip(keys, c0)]
    finally:
        on.option_set(on.OPT_BATCH_MODEL, old[0]); on.option_set(on.OPT_BATCH_MODEL_SEGMENTS, old[1])
    assert moved == [1, 0, 0], f"model passes / declined / blocks left to the host: {moved}"
    got_c = _avg_counters(on)
    assert got_c["fail"] == 0 and got_c["und"] > 0 and got_c["resolved"] == got_c["und"]
    import torch
    for x, blk in zip(cases, got):
        assert blk == ref.compress(x, 1, 1), f"n={x.size}"
    single = on.compress_device(torch.from_numpy(bad).cuda(), bad.size, 1, 1).tobytes()
    assert got[1] == single, "the single-block path's bytes"


# ---- -e0: no avg flags ---------------------------------------------------------------------------------------------------------------
def test_fast_coder_is_not_affected(ctx, ref):
    import torch
    _, want, flat, _, _ = ms.reference("mixed", ms.FAST)
    d = torch.from_numpy(flat).cuda()
    T = ar.realistic_text(n=300 * 1024)
    dT = torch.from_numpy(T).cuda()
    _, ps0, poff0 = ctx.fast_pstream_batch(d, want.sizes)
    blk0 = ctx.compress_device(dT, T.size, 1, 3).tobytes()
    old = ctx.option_set(ctx.OPT_DC_AVG_EXACT, 1)
    try:
        _, ps1, poff1 = ctx.fast_pstream_batch(d, want.sizes)
        assert _avg_counters(ctx) == dict(fail=0, und=0, resolved=0)
        assert np.array_equal(ps0, ps1) and np.array_equal(poff0, poff1)
        assert ctx.compress_device(dT, T.size, 1, 3).tobytes() == blk0 == ref.compress(T, 1, 3)
        assert _avg_counters(ctx) == dict(fail=0, und=0, resolved=0)
    finally:
        ctx.option_set(ctx.OPT_DC_AVG_EXACT, old)


# ---- the option ---------------------------------------------------------------------------------------------------------------------
def test_option_keys_and_environment(ctx, monkeypatch):
    from libbsc_amd import GpuContext
    from libbsc_amd.gpu import GpuError
    assert ctx.option_get(ctx.OPT_DC_AVG_EXACT) == 0, "the default"
    with pytest.raises(GpuError):
        ctx.option_set(ctx.OPT_DC_AVG_EXACT, 2)
    assert ctx.option_get(ctx.CNT_DC_AVG_RESOLVED) >= 0
    with pytest.raises(GpuError):
        ctx.option_set(ctx.CNT_DC_AVG_RESOLVED, 0)
    a0 = ctx.arena_bytes
    monkeypatch.setenv("BSC_DC_AVG_EXACT", "1")                       # what bsc_compress's default contexts take the option from
    c = GpuContext(0, max_n=1 << 20)
    try:
        assert c.option_get(c.OPT_DC_AVG_EXACT) == 1
        a1 = c.arena_bytes
        c.qlfc_static_pstream(di.const_rank(40, 3000))
        assert _avg_counters(c)["resolved"] > 0
        assert 0 < c.arena_bytes - a1 < 0.1 * (1 << 20) + 65536, "the resolve's buffers: under 0.1 byte per byte of max_n, counted from first use"
    finally:
        c.close()
    assert ctx.arena_bytes == a0


def test_buffers_that_do_not_fit_decline_the_unit(monkeypatch):
    """BSC_DC_AVG_FAIL_ALLOC: the resolve's buffers do not fit.  A block that leaves flags open is declined with no reason bit (an arena
    did not fit), nothing is allocated, now or at the next call; with the option off the same context declines it with FAIL_AVG"""
    from libbsc_amd import GpuContext
    from libbsc_amd.gpu import GpuError
    L = GENERATOR_BLOCKS[ar.FAIL_AVG_GENERATORS[0]]()
    monkeypatch.setenv("BSC_DC_AVG_FAIL_ALLOC", "1")
    c = GpuContext(0, max_n=1 << 20)
    try:
        c.option_set(c.OPT_DC_AVG_EXACT, 1)
        c.qlfc_static_pstream((np.arange(50_000) % 3).astype(np.uint8))      # (no sub-block can escape: the flags are not walked)
        a1 = c.arena_bytes
        for call in range(2):
            with pytest.raises(GpuError) as e:
                c.qlfc_static_pstream(L)
            got = _avg_counters(c)
            print(f"call {call}: code {e.value.code}, gpu {got}, arena bytes {c.arena_bytes} (before: {a1})")
            assert e.value.code == NOT_SUPPORTED and got["fail"] == 0 and got["resolved"] == 0
            assert c.arena_bytes == a1, "no buffers, and no second attempt"
        c.option_set(c.OPT_DC_AVG_EXACT, 0)
        with pytest.raises(GpuError) as e:
            c.qlfc_static_pstream(L)
        got = _avg_counters(c)
        assert e.value.code == NOT_SUPPORTED and got["fail"] == c.DC_FAIL_AVG and got["und"] > 0 and got["resolved"] == 0, got
        assert c.arena_bytes == a1
    finally:
        c.close()
