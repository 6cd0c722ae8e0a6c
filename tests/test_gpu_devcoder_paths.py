"""The device coder's rare exits on the GPU (devcoder.hip): serial replay of evaluation chunks, the extended run_hist look-back, undecided
avg_rank flags and the three data-driven declines.  Inputs and their tags come from tests/devcoder_inputs.py; WHICH path an input must
take is judged on the CPU by tools/devcoder_paths_probe.cpp (test_devcoder_paths.py pins every tag to it), and here the context's
counters (BSCGPU_CNT_DC_*) have to say the same, the streams have to equal the oracle's trace of the reference model, and a declined
block has to come out of bsc_compress byte-identical to the reference through the host model.  Everything is bit-exact."""
import ctypes as C

import numpy as np
import pytest

import devcoder_inputs as di

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from libbsc_amd import GpuContext
    c = GpuContext(0, max_n=(16 << 20) + 4096)        # 4 decisions per byte of THIS size is the arena: none of the inputs comes near it
    yield c
    c.close()


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    d = tmp_path_factory.mktemp("paths_probe")
    exe = di.build_probe(d)
    return lambda L: di.run_probe(exe, L, d)


def _counters(ctx):
    return dict(fail=ctx.option_get(ctx.CNT_DC_LAST_FAIL), replays=ctx.option_get(ctx.CNT_DC_REPLAYS),
                und=ctx.option_get(ctx.CNT_DC_AVG_UNDECIDED), ext=ctx.option_get(ctx.CNT_DC_HIST_EXTENDED))


PLAIN = (np.arange(50_000) % 3).astype(np.uint8)      # three symbols, runs of one byte: nothing to replay, look back for or decline


def _check_plain_call_resets(ctx, name):
    ps, *_ = ctx.qlfc_static_pstream(PLAIN)
    assert len(ps) > 0
    assert _counters(ctx) == dict(fail=0, replays=0, und=0, ext=0), name


def _check_stage(ctx, probe, name, L):
    from libbsc_amd.gpu import GpuError
    from oracle.refbind import Oracle
    orc = Oracle()
    v = probe(L)
    want_mask = v["fail_mask"]
    if want_mask:
        for call in (ctx.qlfc_static_pstream, ctx.qlfc_static_pstream_packed):
            with pytest.raises(GpuError) as e:
                call(L)
            assert e.value.code == -4, name
            got = _counters(ctx)
            print(f"{name}: probe mask {want_mask} und {v['avg_und']} ext {v['hist_ext']} | gpu {got}")
            assert got["fail"] == want_mask, (name, got, v)       # exactly the predicted reason
            assert got["und"] == v["avg_und"] and got["ext"] == v["hist_ext"], (name, got, v)
            _check_plain_call_resets(ctx, name)                    # the call after a decline succeeds, counters reset
        return
    debug = L.size <= (1 << 20)
    ps, st, sz, poff, dbg = ctx.qlfc_static_pstream(L, debug=debug)
    got = _counters(ctx)
    print(f"{name}: probe mask 0 und {v['avg_und']} ext {v['hist_ext']} replay_certain {v['replay_certain']} | gpu {got}")
    assert got["fail"] == 0 and got["und"] == 0 == v["avg_und"] and got["ext"] == v["hist_ext"], (name, got, v)
    if v["replay_certain"]:
        assert got["replays"] > 0, (name, got)
    if v["no_replay_certain"]:
        assert got["replays"] == 0, (name, got)
    assert poff[0] == 0 and poff[-1] == len(ps) == v["decisions"] and len(st) == v["nb"], name
    for b in range(len(st)):
        tr, ct = orc.static_pstream(L[st[b]:st[b] + sz[b]], counters=debug)
        assert np.array_equal(tr, ps[poff[b]:poff[b + 1]]), (name, b, int(np.argmax(tr != ps[poff[b]:poff[b + 1]])))
        if debug:
            assert np.array_equal(dbg[:, poff[b]:poff[b + 1]], ct.T), (name, b)
    # the packed form, where it is produced (a refusal of the FORM leaves the reason mask at 0), and the same counters from that call
    try:
        f, st2, sz2, poff2, pbase, raw = ctx.qlfc_static_pstream_packed(L)
    except GpuError as e:
        assert e.code == -4 and ctx.option_get(ctx.CNT_DC_LAST_FAIL) == 0, name
    else:
        assert st == st2 and sz == sz2 and poff == poff2 and np.array_equal(f, ps & 0x1fff), name
        g2 = _counters(ctx)
        assert g2["fail"] == 0 and g2["ext"] == got["ext"] and (g2["replays"] > 0) == (got["replays"] > 0), (name, got, g2)


@pytest.mark.parametrize("name", list(di.GENERATORS))
def test_stage_takes_the_predicted_path_and_matches_the_oracle(ctx, probe, name):
    """bscgpu_qlfc_static_pstream (+ the packed form) on every generator: stays on the device -> every sub-block's stream equals
    Oracle.static_pstream (blocks <= 1 MiB: the three counter values behind every probability too), replays > 0 where the probe says a
    replay is certain and == 0 where it says none is possible, extended look-backs and undecided flags equal to the probe's counts;
    declined -> -4 with exactly the predicted reason bit, the same counts, and the next call succeeds with the counters reset."""
    tag, extra, build = di.GENERATORS[name]
    L = build()
    _check_stage(ctx, probe, name, L)
    # the tag itself (pinned on the CPU by test_devcoder_paths.py) as the GPU saw it
    got = _counters(ctx)
    if tag.startswith("fail_"):
        return
    if tag == "replay_kept":
        assert got["replays"] > 0 and got["fail"] == 0, (name, got)
    if tag == "hist_ext":
        assert got["ext"] > 0 and got["fail"] == 0, (name, got)


def test_counter_keys_are_get_only(ctx):
    from libbsc_amd.gpu import GpuError
    for key in (ctx.CNT_DC_REPLAYS, ctx.CNT_DC_LAST_FAIL, ctx.CNT_DC_AVG_UNDECIDED, ctx.CNT_DC_HIST_EXTENDED):
        assert ctx.option_get(key) >= 0
        with pytest.raises(GpuError):
            ctx.option_set(key, 0)


def test_capacity_decline_names_its_reason(ctx):
    """the one decline the suite already had (4 decisions per byte of the context's size), now with its reason bit"""
    from libbsc_amd import GpuContext
    from libbsc_amd.gpu import GpuError
    small = GpuContext(0, max_n=(1 << 20) + 4096)
    try:
        with pytest.raises(GpuError) as e:
            small.qlfc_static_pstream(np.random.default_rng(11).integers(0, 256, 1 << 20, dtype=np.uint8))
        assert e.value.code == -4 and small.option_get(small.CNT_DC_LAST_FAIL) == small.DC_FAIL_CAP
    finally:
        small.close()


@pytest.mark.parametrize("name", list(di.WHOLE_BLOCKS))
def test_whole_block_through_the_predicted_path_equals_the_reference(ref, probe, name):
    """bsc_compress of a text whose reference BWT takes the path (the probe judges ref.bwt_encode of the text): coder 1 — and coder 3,
    whose device model runs the char family's chains — byte-identical to the reference and round-tripping through it; a block that stays
    on the device counts as a device-model block with replays > 0, a declined one does not count and leaves its reason in the context."""
    import torch
    from libbsc_amd import GpuContext, _native
    lib = _native.lib()
    lib.bscgpu_process_counter.restype = C.c_longlong
    lib.bscgpu_process_counter.argtypes = [C.c_int]
    tag, extra, build = di.WHOLE_BLOCKS[name]
    T = di.text_with_bwt_like(build())
    L, _, _ = ref.bwt_encode(T)
    v = probe(L)
    di.check_tag(name, v, di.WHOLE_BLOCKS)
    assert T.size >= 1 << 20 and v["nb"] >= 2 and v["runs"] <= 0.70 * T.size
    # (the arena holds 4 decisions per byte of the context's size: sized by the decisions, capacity is not among the reasons)
    c = GpuContext(0, max_n=max(T.size, v["decisions"]) + 4096)
    try:
        d = torch.from_numpy(T).cuda()
        c0 = [lib.bscgpu_process_counter(k) for k in (1, 2)]
        got = c.compress_device(d, T.size, 1, 1).tobytes()
        c1 = [lib.bscgpu_process_counter(k) for k in (1, 2)]
        cnt = _counters(c)
        print(f"{name}: probe mask {v['fail_mask']} und {v['avg_und']} ext {v['hist_ext']} | gpu {cnt}, device-model blocks +{c1[0] - c0[0]}")
        want = ref.compress(T, 1, 1)
        assert got == want, name
        assert ref.decompress(got) == T.tobytes(), name
        assert cnt["fail"] == v["fail_mask"] and cnt["und"] == v["avg_und"] and cnt["ext"] == v["hist_ext"], (name, cnt, v)
        if v["fail_mask"]:
            assert c1[0] == c0[0], (name, c0, c1)                     # never counted as a device-model block: the host model coded it
        else:
            assert c1[0] == c0[0] + 1 and c1[1] == c0[1] and cnt["replays"] > 0, (name, c0, c1, cnt)
        got3 = c.compress_device(d, T.size, 1, 3).tobytes()
        assert got3 == ref.compress(T, 1, 3) and ref.decompress(got3) == T.tobytes(), name
    finally:
        c.close()
