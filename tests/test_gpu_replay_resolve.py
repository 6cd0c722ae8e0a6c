"""Open chunk starts of the evaluation resolved exactly on the GPU (BSCGPU_OPT_DC_REPLAY_EXACT; devcoder.hip 3'): with the option on a
block, a pass or a segment whose counter chains stay open over evaluation chunks is neither replayed serially nor declined — the
counters say how many chunk starts the resolve settled (the host restatement's count: tools/replay_resolve_probe.cpp, pinned on the CPU
by test_replay_resolve_host.py), that nothing was replayed, and the streams and bytes equal the references'.  Inputs: devcoder_inputs.py,
replay_resolve_inputs.py, model_batch_inputs.py.  Everything is bit-exact."""
import ctypes as C

import numpy as np
import pytest

import devcoder_inputs as di
import fast_batch_inputs as fbi
import model_batch_inputs as mb
import replay_resolve_inputs as ri
from front_inputs import layouts_equal

pytestmark = pytest.mark.gpu

CTX_N = (16 << 20) + 4096
NOT_SUPPORTED = -4
STATIC = 1


@pytest.fixture(scope="module")
def ctx():
    from libbsc_amd import GpuContext
    c = GpuContext(0, max_n=CTX_N)
    yield c
    c.close()


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    d = tmp_path_factory.mktemp("replay_probe")
    exe = ri.build_probe(d)
    return lambda L, key, cand=None: ri.probe_block(exe, d, L, cand=cand, key=key)


def _counters(ctx):
    return dict(fail=ctx.option_get(ctx.CNT_DC_LAST_FAIL), replays=ctx.option_get(ctx.CNT_DC_REPLAYS), resolved=ctx.option_get(ctx.CNT_DC_REPLAY_RESOLVED))


def _stage_equals_oracle(ctx, name, L, v):
    """bscgpu_qlfc_static_pstream and its packed form with the option on: kept, nothing replayed, the resolved count the restatement's,
    every sub-block's stream the oracle's trace of the reference model"""
    from libbsc_amd.gpu import GpuError
    from oracle.refbind import Oracle
    ps, st, sz, poff, _ = ctx.qlfc_static_pstream(L)
    got = _counters(ctx)
    print(f"{name}: restatement open {v['on']['open']} stretches {v['stretches']} longest {v['longest']} widest {v['max_width']} | gpu {got}")
    assert got == dict(fail=0, replays=0, resolved=v["on"]["resolved"]), (name, got, v["on"])
    assert poff[0] == 0 and poff[-1] == len(ps) == v["decisions"] and len(st) == v["nb"], name
    orc = Oracle()
    for b in range(len(st)):
        tr, _ = orc.static_pstream(L[st[b]:st[b] + sz[b]], counters=False)
        mine = ps[poff[b]:poff[b + 1]]
        assert np.array_equal(tr, mine), (name, b, int(np.argmax(tr != mine)) if tr.size == mine.size else (tr.size, mine.size))
    try:
        f, *_ = ctx.qlfc_static_pstream_packed(L)
    except GpuError as e:                                              # a refusal of the FORM leaves the reason mask at 0
        assert e.code == NOT_SUPPORTED and ctx.option_get(ctx.CNT_DC_LAST_FAIL) == 0, name
    else:
        assert np.array_equal(f, ps & 0x1fff) and _counters(ctx) == got, name
    return ps


# ---- 1. blocks that are declined today --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ri.FAIL)
def test_fail_replay_generators_stay_on_the_device(ctx, probe, name):
    """the three fail_replay generators and the second table's fail_replay block: declined today with FAIL_REPLAY (the switch does
    something), kept with the option on"""
    from libbsc_amd.gpu import GpuError
    L = ri.block_of(name)
    v = probe(L, name)
    assert v["off"]["fail_replay"] and v["on"]["resolved"] == v["on"]["open"] > 0
    assert ctx.option_get(ctx.OPT_DC_REPLAY_EXACT) == 0
    with pytest.raises(GpuError) as e:
        ctx.qlfc_static_pstream(L)
    assert e.value.code == NOT_SUPPORTED and _counters(ctx)["fail"] == ctx.DC_FAIL_REPLAY and _counters(ctx)["resolved"] == 0
    old = ctx.option_set(ctx.OPT_DC_REPLAY_EXACT, 1)
    try:
        _stage_equals_oracle(ctx, name, L, v)
    finally:
        ctx.option_set(ctx.OPT_DC_REPLAY_EXACT, old)


# ---- 2. blocks that are replayed today --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ri.KEPT)
def test_replay_kept_generators_are_not_replayed(ctx, probe, name):
    """a stretch of one open chunk to stretches of dozens, start brackets of 2 to 186 values (one, two and four candidates per lane), the
    escape class: the stream of the option-off call (serial replays), the option-on call and the oracle are the same"""
    L = di.GENERATORS[name][2]()
    v = probe(L, name)
    assert not v["off"]["fail_replay"] and v["off"]["replays"] > 0
    off_ps, *_ = ctx.qlfc_static_pstream(L)
    off = _counters(ctx)
    assert off == dict(fail=0, replays=v["off"]["replays"], resolved=0), (name, off, v["off"])
    old = ctx.option_set(ctx.OPT_DC_REPLAY_EXACT, 1)
    try:
        ps = _stage_equals_oracle(ctx, name, L, v)
    finally:
        ctx.option_set(ctx.OPT_DC_REPLAY_EXACT, old)
    assert np.array_equal(ps, off_ps), name


# ---- 4. the guard -------------------------------------------------------------------------------------------------------------------------
def test_guard_leaves_wide_brackets_to_the_serial_replay(ctx, probe, monkeypatch):
    """BSC_DC_REPLAY_CAND below an input's widest start bracket: what lies behind such a bracket in its stretch is replayed serially
    (same stream), and a fail_replay input is declined as today"""
    from libbsc_amd import GpuContext
    from libbsc_amd.gpu import GpuError
    name, cand = ri.GUARD_KEPT
    L = di.GENERATORS[name][2]()
    v = probe(L, name, cand)
    assert v["max_width"] > cand and v["on"]["wide"] > 0 and 0 < v["on"]["replays"]
    want, *_ = ctx.qlfc_static_pstream(L)
    monkeypatch.setenv("BSC_DC_REPLAY_CAND", str(cand))
    c = GpuContext(0, max_n=CTX_N)
    try:
        c.option_set(c.OPT_DC_REPLAY_EXACT, 1)
        ps, *_ = c.qlfc_static_pstream(L)
        got = _counters(c)
        print(f"{name} cap {cand}: restatement {v['on']} | gpu {got}")
        assert got == dict(fail=0, replays=v["on"]["replays"], resolved=v["on"]["resolved"]) and got["replays"] > 0
        assert np.array_equal(ps, want)
    finally:
        c.close()
    name, cand = ri.GUARD_FAIL
    L = di.GENERATORS[name][2]()
    v = probe(L, name, cand)
    assert v["max_width"] > cand and v["on"]["fail_replay"]
    monkeypatch.setenv("BSC_DC_REPLAY_CAND", str(cand))
    c = GpuContext(0, max_n=CTX_N)
    try:
        c.option_set(c.OPT_DC_REPLAY_EXACT, 1)
        for call in (c.qlfc_static_pstream, c.qlfc_static_pstream_packed):
            with pytest.raises(GpuError) as e:
                call(L)
            assert e.value.code == NOT_SUPPORTED and _counters(c)["fail"] == c.DC_FAIL_REPLAY == 16
    finally:
        c.close()


# ---- 5. the fast coder, the table form ----------------------------------------------------------------------------------------------------
def test_fast_coder_pass_is_not_replayed(ctx):
    """bscgpu_fast_pstream_batch_device on the pass whose chains must be replayed (test_fast_batch_host.py): chain ends come from the
    marks of the sub-block ids here, the rates are the fast coder's"""
    import torch
    blocks = mb.long_chain_pass()
    want, flat = mb.layout(blocks)
    assert fbi.replay_must_happen(want)
    want_ps, want_poff = fbi.host_streams(want)
    d = torch.from_numpy(flat).cuda()
    sizes = [b.size for b in blocks]
    _, ps0, poff0 = ctx.fast_pstream_batch(d, sizes)
    off = _counters(ctx)
    assert off["fail"] == 0 and off["replays"] > 0 and off["resolved"] == 0
    old = ctx.option_set(ctx.OPT_DC_REPLAY_EXACT, 1)
    try:
        fb, ps, poff = ctx.fast_pstream_batch(d, sizes)
        got = _counters(ctx)
    finally:
        ctx.option_set(ctx.OPT_DC_REPLAY_EXACT, old)
    print(f"long_chain_pass -e0: off {off} | on {got}")
    assert got["fail"] == 0 and got["replays"] == 0 and got["resolved"] > 0
    assert not layouts_equal(fb, want)
    assert np.array_equal(poff, want_poff) and np.array_equal(ps, want_ps) and np.array_equal(ps0, want_ps)


# ---- 6. a batched -e1 pass in model segments ------------------------------------------------------------------------------------------------
def test_segments_keep_the_fail_replay_block(ctx, probe):
    """a block that declines with FAIL_REPLAY between two text-like blocks: today its segment is split and re-run until the block is left
    to the host; with the option on one segment, no re-run, no block left, entries equal to the stand-in's and to the block's own call"""
    import torch
    blocks = ri.fail_replay_pass()
    v = probe(blocks[1], "skewed")
    assert blocks[1].size < 1 << 20 and v["off"]["fail_replay"] and v["on"]["resolved"] == v["on"]["open"]
    want, flat = mb.layout(blocks)
    want_ps, want_poff = mb.host_streams(want)
    d = torch.from_numpy(flat).cuda()
    keys = (ctx.CNT_BATCH_SEGMENTS, ctx.CNT_BATCH_SEG_RERUNS, ctx.CNT_BATCH_SEG_HOST_BLOCKS)
    c0 = [ctx.option_get(k) for k in keys]
    _, _, _, state = ctx.pstream_batch_segments(d, want.sizes, STATIC, 0)
    moved = [ctx.option_get(k) - a for k, a in zip(keys, c0)]
    print(f"option off: state {list(state)} segments / re-runs / host blocks {moved}")
    assert list(state) == [0, ctx.DC_FAIL_REPLAY, 0] and moved[1] >= 1 and moved[2] == 1 and ctx.option_get(ctx.CNT_DC_LAST_FAIL) == ctx.DC_FAIL_REPLAY
    old = ctx.option_set(ctx.OPT_DC_REPLAY_EXACT, 1)
    try:
        c0 = [ctx.option_get(k) for k in keys]
        fb, ps, poff, state = ctx.pstream_batch_segments(d, want.sizes, STATIC, 0)
        moved = [ctx.option_get(k) - a for k, a in zip(keys, c0)]
        got = _counters(ctx)
        one, st, sz, one_poff, _ = ctx.qlfc_static_pstream(blocks[1])
        alone = _counters(ctx)
        others = {b: ctx.qlfc_static_pstream(blocks[b])[0] for b in (0, 2)}
    finally:
        ctx.option_set(ctx.OPT_DC_REPLAY_EXACT, old)
    print(f"option on: state {list(state)} segments / re-runs / host blocks {moved} | gpu {got}, the block alone {alone}")
    assert list(state) == [0, 0, 0] and moved == [1, 0, 0]
    assert got["fail"] == 0 and got["replays"] == 0 and got["resolved"] >= v["on"]["resolved"] > 0
    assert alone == dict(fail=0, replays=0, resolved=v["on"]["resolved"])
    assert not layouts_equal(fb, want)
    assert np.array_equal(poff, want_poff) and np.array_equal(ps, want_ps)
    for b, alone_ps in ((0, others[0]), (1, one), (2, others[2])):
        s0, s1 = int(want.blk_sub[b]), int(want.blk_sub[b + 1])
        assert np.array_equal(ps[int(poff[s0]):int(poff[s1])], alone_ps), f"block {b}: the per-block call's stream"


# ---- 7. the whole block ---------------------------------------------------------------------------------------------------------------------
def _process_counters():
    from libbsc_amd import _native
    lib = _native.lib()
    lib.bscgpu_process_counter.restype = C.c_longlong
    lib.bscgpu_process_counter.argtypes = [C.c_int]
    return [lib.bscgpu_process_counter(k) for k in (1, 2)]           # BSCGPU_PCNT_DEVICE_MODEL_BLOCKS, _REDONE_ON_HOST_MODEL


def test_whole_block_takes_the_device_model(ref, probe, monkeypatch, tmp_path):
    """bsc_compress's route (compress_device, and the pipe) on the text whose BWT declines with FAIL_REPLAY (test_devcoder_paths.py pins
    that), in a context created with BSC_DC_REPLAY_EXACT=1 as the default contexts are: a device-model block, not redone on the host,
    the restatement's count of resolved chunks, the reference's bytes"""
    import torch
    from libbsc_amd import GpuContext
    T = di.text_with_bwt_like(di.WHOLE_BLOCKS["fail_replay"][2]())
    L, _, _ = ref.bwt_encode(T)
    p = di.run_probe(di.build_probe(tmp_path), L, tmp_path)
    assert p["fail_mask"] == di.FAIL_REPLAY and T.size >= 1 << 20
    v = probe(L, "whole block's BWT")
    assert v["off"]["fail_replay"] and v["on"]["resolved"] == v["on"]["open"] > 0
    want = ref.compress(T, 1, 1)
    monkeypatch.setenv("BSC_DC_REPLAY_EXACT", "1")
    c = GpuContext(0, max_n=max(T.size, p["decisions"]) + 4096)
    try:
        assert c.option_get(c.OPT_DC_REPLAY_EXACT) == 1
        d = torch.from_numpy(T).cuda()
        c0 = _process_counters()
        assert c.compress_device(d, T.size, 1, 1).tobytes() == want
        c1 = _process_counters()
        got = _counters(c)
        print(f"whole block: gpu {got}, device-model blocks +{c1[0] - c0[0]}, redone on the host model +{c1[1] - c0[1]}")
        assert got == dict(fail=0, replays=0, resolved=v["on"]["resolved"]), (got, v["on"])
        assert c1[0] == c0[0] + 1 and c1[1] == c0[1]
        pipe = c.pipe(2)
        try:
            t = pipe.submit(d, T.size, 1, 1)
            assert pipe.wait(t).tobytes() == want
        finally:
            pipe.close()
        c1p = _process_counters()
        assert c1p[0] == c1[0] + 1 and c1p[1] == c1[1] and _counters(c) == got, "the pipe: a device-model block again"
        c1 = c1p
        c.option_set(c.OPT_DC_REPLAY_EXACT, 0)
        assert c.compress_device(d, T.size, 1, 1).tobytes() == want
        c2 = _process_counters()
        assert _counters(c)["fail"] == di.FAIL_REPLAY and _counters(c)["resolved"] == 0 and c2[0] == c1[0], "option off: declined as today"
    finally:
        c.close()


# ---- 8. nothing to resolve; the option ----------------------------------------------------------------------------------------------------
PLAIN = (np.arange(50_000) % 3).astype(np.uint8)


def test_blocks_without_an_open_chunk(ctx):
    from libbsc_amd.synth import synth_text_v1
    text = synth_text_v1(7, 300 * 1024)
    for name, L in (("PLAIN", PLAIN), ("text", text)):
        ps0, *_ = ctx.qlfc_static_pstream(L)
        assert _counters(ctx) == dict(fail=0, replays=0, resolved=0)
        old = ctx.option_set(ctx.OPT_DC_REPLAY_EXACT, 1)
        try:
            ps1, *_ = ctx.qlfc_static_pstream(L)
            assert _counters(ctx) == dict(fail=0, replays=0, resolved=0), name
            # the counters are the last unit's: a block with open chunks, then this one again
            ctx.qlfc_static_pstream(di.GENERATORS["alt_rf_static_5_chunks"][2]())
            assert _counters(ctx)["resolved"] > 0
            ps2, *_ = ctx.qlfc_static_pstream(L)
            assert _counters(ctx) == dict(fail=0, replays=0, resolved=0), name
        finally:
            ctx.option_set(ctx.OPT_DC_REPLAY_EXACT, old)
        assert np.array_equal(ps0, ps1) and np.array_equal(ps0, ps2), name


def test_option_keys_environment_and_buffers(ctx, monkeypatch):
    from libbsc_amd import GpuContext
    from libbsc_amd.gpu import GpuError
    assert ctx.option_get(ctx.OPT_DC_REPLAY_EXACT) == 0, "the default"
    with pytest.raises(GpuError):
        ctx.option_set(ctx.OPT_DC_REPLAY_EXACT, 2)
    assert ctx.option_get(ctx.CNT_DC_REPLAY_RESOLVED) >= 0
    with pytest.raises(GpuError):
        ctx.option_set(ctx.CNT_DC_REPLAY_RESOLVED, 0)
    assert (ctx.OPT_DC_REPLAY_EXACT, ctx.CNT_DC_REPLAY_RESOLVED) == (32, 33)
    L = di.GENERATORS["alt_rf_static_5_chunks"][2]()
    monkeypatch.setenv("BSC_DC_REPLAY_EXACT", "1")                    # what bsc_compress's default contexts take the option from
    n = 1 << 20
    c = GpuContext(0, max_n=n)
    try:
        assert c.option_get(c.OPT_DC_REPLAY_EXACT) == 1
        c.option_set(c.OPT_DC_REPLAY_EXACT, 0)
        c.qlfc_static_pstream(L)
        a1 = c.arena_bytes
        c.option_set(c.OPT_DC_REPLAY_EXACT, 1)
        c.profile(True); c.profile_reset()
        c.qlfc_static_pstream(L)
        st = c.profile_get()
        c.profile(False)
        assert _counters(c) == dict(fail=0, replays=0, resolved=4)
        # 771 bytes per chunk slot, four jobs of Dcap / DC_EV + 16 slots, Dcap = 4 decisions per byte of max_n (+ 64 Ki)
        assert 1.5 * n < c.arena_bytes - a1 < 1.5 * n + 100_000, "the resolve's buffers: counted from first use"
        assert st["dc_replay"]["launches"] == 1 and st["dc_replay"]["ms"] > 0 and st["dc_eval"]["launches"] == 2, "the stage is a class of its own in the profile"
    finally:
        c.close()
    # buffers that do not fit: the option is without effect, the block is replayed serially as today
    monkeypatch.setenv("BSC_DC_REPLAY_FAIL_ALLOC", "1")
    c = GpuContext(0, max_n=n)
    try:
        c.qlfc_static_pstream(L)
        assert _counters(c)["fail"] == 0 and _counters(c)["replays"] > 0 and _counters(c)["resolved"] == 0
    finally:
        c.close()
