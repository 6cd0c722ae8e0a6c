"""Open run_hist brackets resolved exactly on the GPU (BSCGPU_OPT_DC_HIST_EXACT; devcoder.hip 1c'): with the option on a block, a pass or
a segment with a chain of more than 9216 same-class runs is not declined — the counters say how many runs the nine predecessors left
open (the CPU probes' count) and that all of them were settled, and the streams and bytes equal the references'.  Inputs:
devcoder_inputs.py, model_batch_inputs.py (each checked on the CPU by test_hist_resolve_host.py to take today's path and to leave
brackets open).  Everything is bit-exact."""
import ctypes as C

import numpy as np
import pytest

import devcoder_inputs as di
import hist_resolve_inputs as hr
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
    old = ctx.option_set(ctx.OPT_DC_HIST_EXACT, 1)
    assert old == 0, "the default"
    yield ctx
    ctx.option_set(ctx.OPT_DC_HIST_EXACT, old)


@pytest.fixture(scope="module")
def probes(tmp_path_factory):
    d = tmp_path_factory.mktemp("hist_probes")
    exe, pexe = hr.build_probe(d), di.build_probe(d)
    return (lambda L: hr.probe_block(exe, d, L)), (lambda L: di.run_probe(pexe, L, d))


def _hist_counters(ctx):
    return dict(fail=ctx.option_get(ctx.CNT_DC_LAST_FAIL), ext=ctx.option_get(ctx.CNT_DC_HIST_EXTENDED), resolved=ctx.option_get(ctx.CNT_DC_HIST_RESOLVED))


def _stage_equals_oracle(ctx, probes, name, L, fail_today=True):
    """bscgpu_qlfc_static_pstream with the option on: kept, the bracket's count is the paths probe's, all of it resolved, and every
    sub-block's stream is the oracle's trace of the reference model"""
    v, p = probes[0](L), probes[1](L)
    assert p["fail_mask"] == (di.FAIL_HIST if fail_today else 0) and p["hist_ext"] == v["ext"] > 0 and v["resolved"] == v["ext"], (name, p["fail_mask"], p["hist_ext"], v)
    ps, st, sz, poff, _ = ctx.qlfc_static_pstream(L)
    got = _hist_counters(ctx)
    print(f"{name}: probe ext {p['hist_ext']} chunks {v['chunks']} groups {v['groups']} chain steps {v['chain_steps']} | gpu {got}")
    assert got == dict(fail=0, ext=p["hist_ext"], resolved=p["hist_ext"]), (name, got)
    assert poff[0] == 0 and poff[-1] == len(ps) == p["decisions"] and len(st) == p["nb"], name
    _streams_equal_oracle(name, L, ps, st, sz, poff)
    return p


def _streams_equal_oracle(name, L, ps, st, sz, poff):
    from oracle.refbind import Oracle
    orc = Oracle()
    for b in range(len(st)):
        tr, _ = orc.static_pstream(L[st[b]:st[b] + sz[b]], counters=False)
        mine = ps[poff[b]:poff[b + 1]]
        assert np.array_equal(tr, mine), (name, b, int(np.argmax(tr != mine)) if tr.size == mine.size else (tr.size, mine.size))


# ---- 1: blocks declined today -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", hr.FAIL_HIST_GENERATORS)
def test_generator_blocks_stay_on_the_device(ctx, probes, name):
    """the generators tagged fail_hist: declined today (the switch does something), kept with the option on"""
    from libbsc_amd.gpu import GpuError
    L = di.GENERATORS[name][2]()
    assert ctx.option_get(ctx.OPT_DC_HIST_EXACT) == 0
    with pytest.raises(GpuError) as e:
        ctx.qlfc_static_pstream(L)
    assert e.value.code == NOT_SUPPORTED
    off = _hist_counters(ctx)
    assert off["fail"] == ctx.DC_FAIL_HIST and off["ext"] > 0 and off["resolved"] == 0
    old = ctx.option_set(ctx.OPT_DC_HIST_EXACT, 1)
    try:
        p = _stage_equals_oracle(ctx, probes, name, L)
        assert p["hist_ext"] == off["ext"], "_HIST_EXTENDED keeps its meaning: what the nine predecessors left open"
        # the packed form of the same stage
        ps, *_ = ctx.qlfc_static_pstream(L)
        try:
            f, *_ = ctx.qlfc_static_pstream_packed(L)
        except GpuError as e2:                                         # a refusal of the FORM leaves the reason mask at 0
            assert e2.code == NOT_SUPPORTED and ctx.option_get(ctx.CNT_DC_LAST_FAIL) == 0, name
        else:
            assert np.array_equal(f, ps & 0x1fff) and _hist_counters(ctx) == dict(fail=0, ext=p["hist_ext"], resolved=p["hist_ext"])
    finally:
        ctx.option_set(ctx.OPT_DC_HIST_EXACT, old)


# ---- 2: blocks the extended look-back keeps today -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["hist_q9216", "hist_mixed_p5000"])
def test_kept_blocks_are_the_same_either_way(ctx, probes, name):
    L = di.GENERATORS[name][2]()
    ext = probes[1](L)["hist_ext"]
    assert ext > 0 and ctx.option_get(ctx.OPT_DC_HIST_EXACT) == 0
    ps0, st0, sz0, poff0, _ = ctx.qlfc_static_pstream(L)
    assert _hist_counters(ctx) == dict(fail=0, ext=ext, resolved=0)
    old = ctx.option_set(ctx.OPT_DC_HIST_EXACT, 1)
    try:
        ps1, st1, sz1, poff1, _ = ctx.qlfc_static_pstream(L)
        assert _hist_counters(ctx) == dict(fail=0, ext=ext, resolved=ext)
    finally:
        ctx.option_set(ctx.OPT_DC_HIST_EXACT, old)
    assert np.array_equal(poff0, poff1) and np.array_equal(ps0, ps1) and list(st0) == list(st1) and list(sz0) == list(sz1)


# ---- 3, 4: more than one group, more than one round of groups ---------------------------------------------------------------------------
def test_long_chains_compose_and_chain_groups(on, probes):
    """hist_chain(140 000): two sub-blocks, 70 000 runs in each open chain — more than DC_HIST_GROUP chunks"""
    p = _stage_equals_oracle(on, probes, "hist_chain(140000)", di.hist_chain(140_000))
    assert p["nb"] == 2 and min(p["sub_runs"]) // 2 > hr.GROUP * hr.CH


def test_more_than_64_groups_in_the_launch(on, probes):
    """hist_chain(2 200 000): 4.4 million runs in four sub-blocks, more than 4096 chunks, so the groups kernel takes a second round of
    64 groups.  The counters against the resolve's probe alone (the paths probe would walk every run's five look-backs of today: 15 s),
    the streams against the oracle (it traces a sub-block of 1.65 MB in 0.1 s)"""
    L = di.hist_chain(2_200_000)
    v = probes[0](L)
    assert v["groups"] > 64 and v["runs"] > 4096 * hr.CH and v["ext"] > 2_000_000 and v["values_equal"] and v["nb"] == 4
    ps, st, sz, poff, _ = on.qlfc_static_pstream(L)
    assert _hist_counters(on) == dict(fail=0, ext=v["ext"], resolved=v["ext"])
    assert len(st) == 4 and poff[0] == 0 and poff[-1] == len(ps)
    _streams_equal_oracle("hist_chain(2200000)", L, ps, st, sz, poff)


# ---- 5: whole blocks ------------------------------------------------------------------------------------------------------------------
def _process_counters():
    from libbsc_amd import _native
    lib = _native.lib()
    lib.bscgpu_process_counter.restype = C.c_longlong
    lib.bscgpu_process_counter.argtypes = [C.c_int]
    return [lib.bscgpu_process_counter(k) for k in (1, 2)]           # BSCGPU_PCNT_DEVICE_MODEL_BLOCKS, _REDONE_ON_HOST_MODEL


def test_whole_block_takes_the_device_model(ref, probes):
    """bsc_compress's route (compress_device, and the pipe) on a text whose BWT holds a chain of 400 000 same-class runs: with the option
    on the block is a device-model block, nothing is redone on the host model and the bytes are the reference's; with it off the same
    block declines"""
    import torch
    from libbsc_amd import GpuContext
    T = di.text_with_bwt_like(di.WHOLE_BLOCKS["fail_hist"][2]())
    L, _, _ = ref.bwt_encode(T)
    p, v = probes[1](L), probes[0](L)
    assert p["fail_mask"] == di.FAIL_HIST and p["hist_fail"] > 0 and T.size >= 1 << 20 and p["nb"] >= 2 and p["runs"] <= 0.70 * T.size
    assert v["ext"] == p["hist_ext"] and v["values_equal"]
    want = ref.compress(T, 1, 1)
    c = GpuContext(0, max_n=max(T.size, p["decisions"]) + 4096)
    try:
        d = torch.from_numpy(T).cuda()
        c0 = _process_counters()
        assert c.compress_device(d, T.size, 1, 1).tobytes() == want
        c1 = _process_counters()
        assert _hist_counters(c) == dict(fail=di.FAIL_HIST, ext=p["hist_ext"], resolved=0) and c1[0] == c0[0], "option off: declined as today"
        c.option_set(c.OPT_DC_HIST_EXACT, 1)
        assert c.compress_device(d, T.size, 1, 1).tobytes() == want
        c2 = _process_counters()
        got = _hist_counters(c)
        print(f"fail_hist: probe ext {p['hist_ext']} | gpu {got}, device-model blocks +{c2[0] - c1[0]}, redone on the host model +{c2[1] - c1[1]}")
        assert got == dict(fail=0, ext=p["hist_ext"], resolved=p["hist_ext"])
        assert c2[0] == c1[0] + 1 and c2[1] == c1[1]
        pipe = c.pipe(2)
        try:
            t = pipe.submit(d, T.size, 1, 1)
            assert pipe.wait(t).tobytes() == want
        finally:
            pipe.close()
        c3 = _process_counters()
        assert c3[0] == c2[0] + 1 and c3[1] == c2[1] and _hist_counters(c)["resolved"] == p["hist_ext"]
    finally:
        c.close()


# ---- 6: the batched pass ----------------------------------------------------------------------------------------------------------------
def _first_difference(ps, want_ps, want_poff):
    w = np.flatnonzero(ps != want_ps)
    s = int(np.searchsorted(want_poff, w[0], side="right")) - 1
    return f"{w.size} of {ps.size} entries differ, first at {int(w[0])} (sub-block {s}): {int(ps[w[0]]):#x} != {int(want_ps[w[0]]):#x}"


def test_pass_is_kept_and_equals_the_stand_in(on):
    import torch
    _, want, flat, want_ps, want_poff = ms.reference("fail_hist", ms.STATIC)
    fb, ps, poff = on.static_pstream_batch(torch.from_numpy(flat).cuda(), want.sizes)
    got = _hist_counters(on)
    assert got["fail"] == 0 and got["ext"] > 40000 - 9 - 1 and got["resolved"] == got["ext"], got
    assert not layouts_equal(fb, want)
    assert np.array_equal(poff, want_poff) and ps.size == want_ps.size
    assert np.array_equal(ps, want_ps), _first_difference(ps, want_ps, want_poff)


def test_pass_packed_form(on):
    import torch
    from libbsc_amd.gpu import pstream_pack13_host
    _, want, flat, want_ps, want_poff = ms.reference("fail_hist", ms.STATIC)
    want_bytes, want_pbase = pstream_pack13_host(want_ps, want_poff)
    _, packed, poff, pbase = on.static_pstream_batch_packed(torch.from_numpy(flat).cuda(), want.sizes)
    got = _hist_counters(on)
    assert got["fail"] == 0 and got["resolved"] == got["ext"] > 0
    assert np.array_equal(poff, want_poff) and np.array_equal(pbase, want_pbase) and np.array_equal(packed, want_bytes)


def test_segments_exclude_no_block_for_its_run_hist(on):
    import torch
    _, want, flat, want_ps, want_poff = ms.reference("fail_hist", ms.STATIC)
    d = torch.from_numpy(flat).cuda()
    keys = (on.CNT_BATCH_SEGMENTS, on.CNT_BATCH_SEG_RERUNS, on.CNT_BATCH_SEG_HOST_BLOCKS)
    c0 = [on.option_get(k) for k in keys]
    fb, ps, poff, state = on.pstream_batch_segments(d, want.sizes, ms.STATIC, 0)
    moved = [on.option_get(k) - a for k, a in zip(keys, c0)]
    assert list(state) == [0, 0, 0] and moved == [1, 0, 0], "one segment, no re-run, no block left to the host"
    got = _hist_counters(on)
    assert got["fail"] == 0 and got["resolved"] == got["ext"] > 0
    assert np.array_equal(poff, want_poff) and ps.size == want_ps.size
    assert np.array_equal(ps, want_ps), _first_difference(ps, want_ps, want_poff)


def test_compress_batch_in_segments_keeps_every_block(on, ref, monkeypatch):
    """the call of test_gpu_model_segments.test_block_that_declined_its_pass_now_leaves_alone: no block leaves"""
    from libbsc_amd.synth import synth_text_v1
    monkeypatch.setenv("BSC_BATCH_MODEL_MIN_PASS", "0")
    bad = di.text_with_bwt_like(di.hist_chain(200_000))
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
    got_c = _hist_counters(on)
    assert got_c["fail"] == 0 and got_c["ext"] > 100_000 and got_c["resolved"] == got_c["ext"], got_c
    for x, blk in zip(cases, got):
        assert blk == ref.compress(x, 1, 1), f"n={x.size}"


# ---- 7: -e0 has no run_hist -------------------------------------------------------------------------------------------------------------
def test_fast_coder_is_not_affected(ctx, ref):
    import torch
    from libbsc_amd.synth import synth_text_v1
    _, want, flat, _, _ = ms.reference("mixed", ms.FAST)
    d = torch.from_numpy(flat).cuda()
    T = synth_text_v1(7, 300 * 1024)
    dT = torch.from_numpy(T).cuda()
    _, ps0, poff0 = ctx.fast_pstream_batch(d, want.sizes)
    blk0 = ctx.compress_device(dT, T.size, 1, 3).tobytes()
    old = ctx.option_set(ctx.OPT_DC_HIST_EXACT, 1)
    try:
        _, ps1, poff1 = ctx.fast_pstream_batch(d, want.sizes)
        assert _hist_counters(ctx) == dict(fail=0, ext=0, resolved=0)
        assert np.array_equal(ps0, ps1) and np.array_equal(poff0, poff1)
        assert ctx.compress_device(dT, T.size, 1, 3).tobytes() == blk0 == ref.compress(T, 1, 3)
        assert _hist_counters(ctx) == dict(fail=0, ext=0, resolved=0)
    finally:
        ctx.option_set(ctx.OPT_DC_HIST_EXACT, old)


# ---- 8: the option ----------------------------------------------------------------------------------------------------------------------
def test_option_keys_and_environment(ctx, monkeypatch):
    from libbsc_amd import GpuContext
    from libbsc_amd.gpu import GpuError
    assert ctx.option_get(ctx.OPT_DC_HIST_EXACT) == 0, "the default"
    with pytest.raises(GpuError):
        ctx.option_set(ctx.OPT_DC_HIST_EXACT, 2)
    assert ctx.option_get(ctx.CNT_DC_HIST_RESOLVED) >= 0
    with pytest.raises(GpuError):
        ctx.option_set(ctx.CNT_DC_HIST_RESOLVED, 0)
    a0 = ctx.arena_bytes
    monkeypatch.setenv("BSC_DC_HIST_EXACT", "1")                      # what bsc_compress's default contexts take the option from
    c = GpuContext(0, max_n=1 << 20)
    try:
        assert c.option_get(c.OPT_DC_HIST_EXACT) == 1
        a1 = c.arena_bytes
        c.qlfc_static_pstream(di.hist_chain(3000))
        assert _hist_counters(c) == dict(fail=0, ext=3000 - 9, resolved=3000 - 9)
        assert 0 < c.arena_bytes - a1 < 0.5 * (1 << 20) + 65536, "the resolve's buffers: under 0.5 byte per byte of max_n, counted from first use"
    finally:
        c.close()
    assert ctx.arena_bytes == a0


def test_buffers_that_do_not_fit_leave_the_option_without_effect(monkeypatch):
    """BSC_DC_HIST_FAIL_ALLOC: the resolve's buffers do not fit.  A block whose brackets the nine predecessors leave open comes out as
    from a context with the option off: the same entries, the same seven counters, the same bytes of arena"""
    from libbsc_amd import GpuContext
    L = di.GENERATORS["hist_q9216"][2]()
    monkeypatch.setenv("BSC_DC_HIST_FAIL_ALLOC", "1")
    seen = []
    for option in (0, 1):
        c = GpuContext(0, max_n=1 << 20)
        try:
            c.option_set(c.OPT_DC_HIST_EXACT, option)
            ps, st, sz, poff, _ = c.qlfc_static_pstream(L)
            keys = (c.CNT_DC_LAST_FAIL, c.CNT_DC_REPLAYS, c.CNT_DC_AVG_UNDECIDED, c.CNT_DC_AVG_RESOLVED, c.CNT_DC_REPLAY_RESOLVED,
                    c.CNT_DC_HIST_EXTENDED, c.CNT_DC_HIST_RESOLVED)
            seen.append((ps, list(st), list(sz), list(poff), [c.option_get(k) for k in keys], c.arena_bytes))
        finally:
            c.close()
    off, on_ = seen
    print(f"counters: option off {off[4]}, option on {on_[4]}; arena bytes {off[5]} / {on_[5]}")
    assert off[4][0] == 0 and off[4][5] > 0, "the input: kept, with open brackets"
    assert on_[4] == off[4] and on_[4][6] == 0
    assert np.array_equal(on_[0], off[0]) and on_[1:4] == off[1:4]
    assert on_[5] == off[5]
