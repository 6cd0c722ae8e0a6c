"""The device model's three exact resolves (BSCGPU_OPT_DC_AVG_EXACT, _HIST_EXACT, _REPLAY_EXACT) switched on together, and in every
other combination: blocks with more than one reason to leave the device (resolve_combined_inputs.py, each pinned on the CPU by
test_resolve_combined_host.py) must be declined with exactly the mask the paths probe gives for the option set, or be kept with the
oracle's streams and the three resolve probes' counts.  Nothing may carry over from one block to the next in the resolves' arenas.
Everything is bit-exact.

The order of the stages (devcoder.hip: devcoder_pstream, dc_static_run) says which counters a declined call still reports: the avg
kernels (1a, 1a'), the contexts with the run_hist resolve (1c, 1c') and dc_setup_kernel all run before the FIRST sync, where FAIL_AVG
and FAIL_HIST leave — so the avg and the hist counters are complete whichever of the two declines the block, and the evaluation (3,
with the resolve of open chunk starts 3') has not run: replays and replay-resolved are 0.  FAIL_REPLAY leaves at the SECOND sync, with
the avg and hist counters complete again."""
import ctypes as C
import contextlib
import functools

import numpy as np
import pytest

import devcoder_inputs as di
import model_segment_inputs as ms
import resolve_combined_inputs as rc
from front_inputs import layouts_equal

pytestmark = pytest.mark.gpu

CTX_N = (16 << 20) + 4096
NOT_SUPPORTED = -4
MIB = 1 << 20


@pytest.fixture(scope="module")
def ctx():
    from libbsc_amd import GpuContext
    c = GpuContext(0, max_n=CTX_N)
    yield c
    c.close()


@pytest.fixture(scope="module")
def t(tmp_path_factory):
    return rc.tools(tmp_path_factory.mktemp("combined_probes"))


def _keys(ctx):
    return {rc.AVG: ctx.OPT_DC_AVG_EXACT, rc.HIST: ctx.OPT_DC_HIST_EXACT, rc.REPLAY: ctx.OPT_DC_REPLAY_EXACT}


@contextlib.contextmanager
def options(ctx, on):
    """the context with exactly the options of `on` (probe words) on; all three back to the default afterwards"""
    keys = _keys(ctx)
    for o, k in keys.items():
        ctx.option_set(k, 1 if o in on else 0)
    try:
        yield ctx
    finally:
        for k in keys.values():
            ctx.option_set(k, 0)


@pytest.fixture
def on3(ctx):
    with options(ctx, rc.ALL_ON):
        yield ctx


def _counters(ctx):
    g = ctx.option_get
    return dict(fail=g(ctx.CNT_DC_LAST_FAIL), avg_und=g(ctx.CNT_DC_AVG_UNDECIDED), avg_res=g(ctx.CNT_DC_AVG_RESOLVED), hist_ext=g(ctx.CNT_DC_HIST_EXTENDED),
                hist_res=g(ctx.CNT_DC_HIST_RESOLVED), replays=g(ctx.CNT_DC_REPLAYS), replay_res=g(ctx.CNT_DC_REPLAY_RESOLVED))


def _expected_counters(mask, on, a, h, r):
    """what the context must say about a block under the option set `on`, from the probes' counts (module docstring: the stage order)"""
    want = dict(fail=mask, avg_und=a["und"], avg_res=a["und"] if rc.AVG in on else 0, hist_ext=h["ext"], hist_res=h["ext"] if rc.HIST in on else 0)
    if mask & (di.FAIL_AVG | di.FAIL_HIST):
        want.update(replays=0, replay_res=0)                             # left at the first sync: no evaluation
    elif mask:
        want.update(replays=r["off"]["replays"], replay_res=0)           # FAIL_REPLAY: the restatement's count of chunks replayed when it gives up
    elif rc.REPLAY in on:
        want.update(replays=0, replay_res=r["on"]["resolved"])
    else:
        want.update(replays=r["off"]["replays"], replay_res=0)
    return want


@functools.lru_cache(maxsize=None)
def _oracle_trace(key, b, start, size):
    from oracle.refbind import Oracle
    tr, _ = Oracle().static_pstream(rc_block_of(key)[start:start + size], counters=False)
    tr.setflags(write=False)
    return tr


_extra_blocks = {}


def rc_block_of(key):
    return _extra_blocks[key] if key in _extra_blocks else rc.block(key)


def _stage(ctx, t, key, L, on):
    """bscgpu_qlfc_static_pstream on L under the option set `on` (already set on ctx): declined with the paths probe's mask, or kept with
    the oracle's streams; the counters are the probes' either way -> the entries, or None"""
    from libbsc_amd.gpu import GpuError
    if key not in rc.BLOCKS:
        _extra_blocks[key] = L
    mask = rc.masks(t, key, L)[rc.set_index(on)]
    p, a, h, r = rc.paths(t, key, L), rc.avg(t, key, L), rc.hist(t, key, L), rc.replay(t, key, L)
    want = _expected_counters(mask, on, a, h, r)
    if mask:
        with pytest.raises(GpuError) as e:
            ctx.qlfc_static_pstream(L)
        got = _counters(ctx)
        print(f"{key} [{rc.set_id(on)}]: probe mask {mask} | gpu {got}")
        assert e.value.code == NOT_SUPPORTED and got["fail"] == mask, (key, on, got)
        assert {k: got[k] for k in want} == want, (key, on, got, want)
        return None
    ps, st, sz, poff, _ = ctx.qlfc_static_pstream(L)
    got = _counters(ctx)
    print(f"{key} [{rc.set_id(on)}]: kept | gpu {got}")
    assert got == want, (key, on, got, want)
    assert poff[0] == 0 and poff[-1] == len(ps) == p["decisions"] and len(st) == p["nb"], key
    for b in range(len(st)):
        tr = _oracle_trace(key, b, st[b], sz[b])
        mine = ps[poff[b]:poff[b + 1]]
        assert np.array_equal(tr, mine), (key, on, b, int(np.argmax(tr != mine)) if tr.size == mine.size else (tr.size, mine.size))
    try:
        f, *_ = ctx.qlfc_static_pstream_packed(L)
    except GpuError as e2:                                             # a refusal of the FORM leaves the reason mask at 0
        assert e2.code == NOT_SUPPORTED and ctx.option_get(ctx.CNT_DC_LAST_FAIL) == 0, key
    else:
        assert np.array_equal(f, ps & 0x1fff) and _counters(ctx) == want, (key, on)
    return ps


# ---- 1. the option lattice ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("on", rc.OPTION_SETS, ids=rc.set_id)
@pytest.mark.parametrize("name", list(rc.LATTICE))
def test_option_lattice(ctx, t, name, on):
    """every block with two or three reasons under every option set: the mask is the reasons of the first sync that no option takes
    away, alone (6 with both; never with bit 16 beside them), else FAIL_REPLAY alone, else the block is kept"""
    L = rc.block(name)
    m = rc.masks(t, name, L)
    assert rc.reasons(rc.paths(t, name, L)) == rc.LATTICE[name] and m[7] == 0
    with options(ctx, on):
        ps = _stage(ctx, t, name, L, on)
    assert (ps is None) == (m[rc.set_index(on)] != 0)


# ---- 2. a block that is kept either way -----------------------------------------------------------------------------------------------------
def test_kept_block_is_the_same_in_all_four_settings(ctx, t):
    """same_runs_small: avg-exact keeps it; its run_hist brackets close within today's look-back and its 14 open chunks are within the
    serial replay's reach, so the other two options change how the stream is computed and never what it is"""
    name = rc.KEPT_EITHER_WAY
    L = rc.block(name)
    r = rc.replay(t, name, L)
    assert rc.masks(t, name, L)[1::2] == [0, 0, 0, 0] and r["off"]["replays"] > 0 and rc.hist(t, name, L)["ext"] > 0
    streams = []
    for on in [o for o in rc.OPTION_SETS if rc.AVG in o]:
        with options(ctx, on):
            streams.append(_stage(ctx, t, name, L, on))
            assert ctx.option_get(ctx.CNT_DC_REPLAYS) == (0 if rc.REPLAY in on else r["off"]["replays"])
    assert len(streams) == 4 and all(np.array_equal(streams[0], s) for s in streams[1:])


# ---- 3. nothing carries over between blocks -------------------------------------------------------------------------------------------------
def test_nothing_carries_over_between_blocks(ctx, t):
    """one context, the arenas of all three resolves alive: a block open in all three ways in the same runs, a small block with open
    run_hist brackets only, one with no open flag at all (a single avg lane, exact from its first run), the first block again — then the
    options go off one at a time.  Every call's counters are its own block's"""
    small = rc.block(rc.KEPT_EITHER_WAY)
    with options(ctx, rc.ALL_ON):
        first = _stage(ctx, t, "same_runs", rc.block("same_runs"), rc.ALL_ON)
        assert _stage(ctx, t, "hist_chain_3000", di.hist_chain(3000), rc.ALL_ON) is not None
        assert ctx.option_get(ctx.CNT_DC_HIST_RESOLVED) == 3000 - 9 and ctx.option_get(ctx.CNT_DC_AVG_UNDECIDED) == 0
        assert _stage(ctx, t, "const_rank_40_1024", di.const_rank(40, 1024), rc.ALL_ON) is not None
        assert ctx.option_get(ctx.CNT_DC_AVG_RESOLVED) == 0 and ctx.option_get(ctx.CNT_DC_HIST_EXTENDED) == 0
        again = _stage(ctx, t, "same_runs", rc.block("same_runs"), rc.ALL_ON)
        assert np.array_equal(first, again)
        all_on = _stage(ctx, t, rc.KEPT_EITHER_WAY, small, rc.ALL_ON)
        keys = _keys(ctx)
        ctx.option_set(keys[rc.REPLAY], 0)
        no_replay = _stage(ctx, t, rc.KEPT_EITHER_WAY, small, (rc.AVG, rc.HIST))
        ctx.option_set(keys[rc.HIST], 0)
        no_hist = _stage(ctx, t, rc.KEPT_EITHER_WAY, small, (rc.AVG,))
        ctx.option_set(keys[rc.AVG], 0)
        assert _stage(ctx, t, rc.KEPT_EITHER_WAY, small, ()) is None
        assert np.array_equal(all_on, no_replay) and np.array_equal(all_on, no_hist)


# ---- 4. arena accounting --------------------------------------------------------------------------------------------------------------------
def _env_all_on(monkeypatch):
    for k in ("BSC_DC_AVG_EXACT", "BSC_DC_HIST_EXACT", "BSC_DC_REPLAY_EXACT"):
        monkeypatch.setenv(k, "1")


def test_arenas_of_all_three_are_counted_from_first_use(ctx, t, monkeypatch):
    from libbsc_amd import GpuContext
    a0 = ctx.arena_bytes
    _env_all_on(monkeypatch)
    n = MIB
    c = GpuContext(0, max_n=n)
    try:
        assert [c.option_get(k) for k in _keys(c).values()] == [1, 1, 1]
        a1 = c.arena_bytes
        assert _stage(c, t, rc.KEPT_EITHER_WAY, rc.block(rc.KEPT_EITHER_WAY), rc.ALL_ON) is not None
        grown = c.arena_bytes - a1
        # the single-option tests' bounds: 0.1 (avg), 0.5 (hist) and 1.5 (replay) bytes per byte of max_n, plus their constants
        bound = (0.1 * n + 65536) + (0.5 * n + 65536) + (1.5 * n + 100_000)
        print(f"arena growth at first use: {grown} bytes, bound {bound:.0f}")
        assert 0 < grown < bound
        assert grown > 1.5 * n, "the replay resolve's buffers alone are more than 1.5 bytes per byte of max_n"
    finally:
        c.close()
    assert ctx.arena_bytes == a0


# ---- 5. the whole block ---------------------------------------------------------------------------------------------------------------------
def _process_counters():
    from libbsc_amd import _native
    lib = _native.lib()
    lib.bscgpu_process_counter.restype = C.c_longlong
    lib.bscgpu_process_counter.argtypes = [C.c_int]
    return [lib.bscgpu_process_counter(k) for k in (1, 2)]           # BSCGPU_PCNT_DEVICE_MODEL_BLOCKS, _REDONE_ON_HOST_MODEL


def test_whole_block_takes_the_device_model(ref, t, monkeypatch):
    """bsc_compress's route (compress_device, and the pipe) on the text whose BWT has all three reasons, in a context created with the
    three environment switches as the default contexts are: a device-model block, not redone on the host, the probes' counts, the
    reference's bytes — with the host range coder and with the device's; with any one option off again the block declines for that
    option's reason alone, and the bytes stay"""
    import torch
    from libbsc_amd import GpuContext
    T = rc.whole_block_text()
    L, _, _ = ref.bwt_encode(T)
    m, p = rc.masks(t, "whole", L), rc.paths(t, "whole", L)
    a, h, r = rc.avg(t, "whole", L), rc.hist(t, "whole", L), rc.replay(t, "whole", L)
    assert rc.reasons(p) == {rc.AVG, rc.HIST, rc.REPLAY} and m[0] == 6 and m[7] == 0 and T.size >= MIB and p["nb"] >= 2 and p["runs"] <= 0.70 * T.size
    want = ref.compress(T, 1, 1)
    want_kept = _expected_counters(0, rc.ALL_ON, a, h, r)
    _env_all_on(monkeypatch)
    c = GpuContext(0, max_n=max(T.size, p["decisions"]) + 4096)
    try:
        keys = _keys(c)
        assert [c.option_get(k) for k in keys.values()] == [1, 1, 1]
        d = torch.from_numpy(np.array(T)).cuda()
        for device_rc in (0, 1):
            c.option_set(c.OPT_DEVICE_RC, device_rc)
            c0 = _process_counters()
            assert c.compress_device(d, T.size, 1, 1).tobytes() == want, f"device rc {device_rc}"
            c1 = _process_counters()
            got = _counters(c)
            print(f"whole block (device rc {device_rc}): gpu {got}, device-model blocks +{c1[0] - c0[0]}, redone on the host model +{c1[1] - c0[1]}")
            assert got == want_kept, (got, want_kept)
            assert c1[0] == c0[0] + 1 and c1[1] == c0[1]
            pipe = c.pipe(2)
            try:
                tk = pipe.submit(d, T.size, 1, 1)
                assert pipe.wait(tk).tobytes() == want
            finally:
                pipe.close()
            c2 = _process_counters()
            assert c2[0] == c1[0] + 1 and c2[1] == c1[1] and _counters(c) == want_kept, "the pipe: a device-model block again"
        c.option_set(c.OPT_DEVICE_RC, 0)
        for o, bit in zip(rc.ALL_ON, (di.FAIL_AVG, di.FAIL_HIST, di.FAIL_REPLAY)):
            on = tuple(w for w in rc.ALL_ON if w != o)
            assert m[rc.set_index(on)] == bit
            c.option_set(keys[o], 0)
            c0 = _process_counters()
            assert c.compress_device(d, T.size, 1, 1).tobytes() == want, f"{o} off"
            c1 = _process_counters()
            got = _counters(c)
            want_off = _expected_counters(bit, on, a, h, r)
            print(f"whole block, {o} off: gpu {got}")
            assert got["fail"] == bit and {k: got[k] for k in want_off} == want_off and c1[0] == c0[0], f"{o} off: declined for that reason alone"
            c.option_set(keys[o], 1)
    finally:
        c.close()


# ---- 6. the batched pass --------------------------------------------------------------------------------------------------------------------
def _first_difference(ps, want_ps, want_poff):
    w = np.flatnonzero(ps != want_ps)
    s = int(np.searchsorted(want_poff, w[0], side="right")) - 1
    return f"{w.size} of {ps.size} entries differ, first at {int(w[0])} (sub-block {s}): {int(ps[w[0]]):#x} != {int(want_ps[w[0]]):#x}"


def _pass_counts(t):
    """the probes on every block of the pass -> (avg flags the pass leaves open: model_batch_inputs' restatement over the pass's lanes,
    run_hist brackets open: a chain is a sub-block's, so the blocks' own counts add up)"""
    import model_batch_inputs as mb
    blocks, fb, _, _, _ = rc.pass_reference()
    ext = 0
    for b, L in enumerate(blocks):
        p = rc.paths(t, f"pass{b}", L)
        assert int(fb.blk_sub[b + 1] - fb.blk_sub[b]) == p["nb"], "the pass splits a block as the single-block stage does"
        ext += rc.hist(t, f"pass{b}", L)["ext"]
    return mb.avg_undecided(fb), ext


def _pass_kept(ctx, t):
    und, ext = _pass_counts(t)
    got = _counters(ctx)
    print(f"pass: avg open {und}, run_hist open {ext} | gpu {got}")
    assert und > 0 and ext > 0
    assert {k: got[k] for k in ("fail", "avg_und", "avg_res", "hist_ext", "hist_res", "replays")} == dict(fail=0, avg_und=und, avg_res=und, hist_ext=ext, hist_res=ext, replays=0)
    assert got["replay_res"] > 0


def test_pass_is_kept_and_equals_the_stand_in(on3, t):
    import torch
    _, want, flat, want_ps, want_poff = rc.pass_reference()
    fb, ps, poff = on3.static_pstream_batch(torch.from_numpy(np.array(flat)).cuda(), want.sizes)
    _pass_kept(on3, t)
    assert not layouts_equal(fb, want)
    assert np.array_equal(poff, want_poff) and ps.size == want_ps.size
    assert np.array_equal(ps, want_ps), _first_difference(ps, want_ps, want_poff)


def test_pass_packed_form(on3, t):
    import torch
    from libbsc_amd.gpu import pstream_pack13_host
    _, want, flat, want_ps, want_poff = rc.pass_reference()
    want_bytes, want_pbase = pstream_pack13_host(want_ps, want_poff)
    _, packed, poff, pbase = on3.static_pstream_batch_packed(torch.from_numpy(np.array(flat)).cuda(), want.sizes)
    _pass_kept(on3, t)
    assert np.array_equal(poff, want_poff) and np.array_equal(pbase, want_pbase) and np.array_equal(packed, want_bytes)


def test_segments_keep_every_block(on3, t):
    import torch
    _, want, flat, want_ps, want_poff = rc.pass_reference()
    d = torch.from_numpy(np.array(flat)).cuda()
    keys = (on3.CNT_BATCH_SEGMENTS, on3.CNT_BATCH_SEG_RERUNS, on3.CNT_BATCH_SEG_HOST_BLOCKS)
    c0 = [on3.option_get(k) for k in keys]
    fb, ps, poff, state = on3.pstream_batch_segments(d, want.sizes, ms.STATIC, 0)
    moved = [on3.option_get(k) - a for k, a in zip(keys, c0)]
    assert list(state) == [0] * want.count and moved == [1, 0, 0], "one segment, no re-run, no block left to the host"
    _pass_kept(on3, t)
    assert np.array_equal(poff, want_poff) and ps.size == want_ps.size
    assert np.array_equal(ps, want_ps), _first_difference(ps, want_ps, want_poff)


@pytest.mark.parametrize("missing", rc.ALL_ON, ids=lambda o: "no_" + o[:-len("_exact")])
def test_segments_leave_the_missing_options_blocks_to_the_host(ctx, t, missing):
    """two of the three on: exactly the blocks whose mask under that option set is not 0 (the paths probe, block by block) go to the
    host, each with its own reason; what is kept is the stand-in's"""
    import torch
    blocks, want, flat, want_ps, want_poff = rc.pass_reference()
    on = tuple(w for w in rc.ALL_ON if w != missing)
    want_state = [rc.masks(t, f"pass{b}", L)[rc.set_index(on)] for b, L in enumerate(blocks)]
    bit = {rc.AVG: di.FAIL_AVG, rc.HIST: di.FAIL_HIST, rc.REPLAY: di.FAIL_REPLAY}[missing]
    assert set(want_state) == {0, bit} and want_state[0] == want_state[-1] == 0
    d = torch.from_numpy(np.array(flat)).cuda()
    host_blocks = ctx.CNT_BATCH_SEG_HOST_BLOCKS
    with options(ctx, on):
        c0 = ctx.option_get(host_blocks)
        fb, ps, poff, state = ctx.pstream_batch_segments(d, want.sizes, ms.STATIC, 0)
        moved = ctx.option_get(host_blocks) - c0
    print(f"{missing} off: state {list(state)}, blocks left to the host +{moved}")
    assert list(state) == want_state and moved == sum(1 for s in want_state if s)
    exp_ps, exp_poff = ms.expected(want, want_ps, want_poff, want_state)
    assert np.array_equal(poff, exp_poff) and ps.size == exp_ps.size
    assert np.array_equal(ps, exp_ps), _first_difference(ps, exp_ps, exp_poff)


def _text_pass_masks(t, ref):
    out = []
    for b, T in enumerate(rc.text_pass()):
        L, _, _ = ref.bwt_encode(T)
        out.append(rc.masks(t, f"text{b}", L))
        assert rc.reasons(rc.paths(t, f"text{b}", L)) == rc.TEXT_PASS_REASONS[b]
    return out


@pytest.mark.parametrize("missing", (None,) + rc.ALL_ON, ids=lambda o: "all_on" if o is None else "no_" + o[:-len("_exact")])
def test_compress_batch_in_segments(ctx, t, ref, monkeypatch, missing):
    """bsc_compress's batched route on texts whose BWT has one reason each: with all three on one model pass, nothing declined, no block
    left to the host; with one option missing exactly its blocks go to the host.  The bytes are the reference's either way"""
    monkeypatch.setenv("BSC_BATCH_MODEL_MIN_PASS", "0")
    cases = [np.array(x) for x in rc.text_pass()]
    on = tuple(w for w in rc.ALL_ON if w != missing)
    left = sum(1 for m in _text_pass_masks(t, ref) if m[rc.set_index(on)])
    assert left == (0 if missing is None else 1)
    keys = (ctx.CNT_BATCH_MODEL_PASSES, ctx.CNT_BATCH_MODEL_DECLINED, ctx.CNT_BATCH_SEG_HOST_BLOCKS)
    with options(ctx, on):
        old = ctx.option_set(ctx.OPT_BATCH_MODEL, 1), ctx.option_set(ctx.OPT_BATCH_MODEL_SEGMENTS, 1)
        try:
            c0 = [ctx.option_get(k) for k in keys]
            got = ctx.compress_batch(cases, 1, 1)
            moved = [ctx.option_get(k) - a for k, a in zip(keys, c0)]
        finally:
            ctx.option_set(ctx.OPT_BATCH_MODEL, old[0]); ctx.option_set(ctx.OPT_BATCH_MODEL_SEGMENTS, old[1])
    print(f"{missing} off: model passes / declined / blocks left to the host: {moved}")
    assert moved == [1, 0, left]
    for x, blk in zip(cases, got):
        assert blk == ref.compress(x, 1, 1), f"n={x.size}"


# ---- 7. the fast coder ------------------------------------------------------------------------------------------------------------------------
def test_fast_coder_is_what_it_is_with_replay_exact_alone(ctx, ref):
    """-e0 has no avg_rank flags and no run_hist: with all three on a pass and a whole block are entry for entry, byte for byte what they
    are with replay-exact alone"""
    import torch
    _, want, flat, _, _ = ms.reference("mixed", ms.FAST)
    d = torch.from_numpy(np.array(flat)).cuda()
    T = rc.whole_block_text()
    dT = torch.from_numpy(np.array(T)).cuda()
    none = dict(avg_und=0, avg_res=0, hist_ext=0, hist_res=0)
    results = []
    for on in ((rc.REPLAY,), rc.ALL_ON):
        with options(ctx, on):
            _, ps, poff = ctx.fast_pstream_batch(d, want.sizes)
            got = _counters(ctx)
            assert got["fail"] == 0 and {k: got[k] for k in none} == none, (on, got)
            blk = ctx.compress_device(dT, T.size, 1, 3).tobytes()
            got = _counters(ctx)
            assert {k: got[k] for k in none} == none, (on, got)
            results.append((ps, poff, blk, got))
    (ps0, poff0, blk0, cnt0), (ps1, poff1, blk1, cnt1) = results
    assert np.array_equal(ps0, ps1) and np.array_equal(poff0, poff1) and cnt0 == cnt1
    assert blk0 == blk1 == ref.compress(T, 1, 3)
