"""The adaptive coder's model (-e2) in segments on the CPU (no GPU): the stand-in of the third fact
(bscgpu_adaptive_longest_chain_host) against the stand-in's own mixer-id plane and the numpy restatement, the preconditions the GPU
tests rest on, the plan with the third fact through tools/dc_segment_probe.cpp, and the route's new option through
tools/batch_pass_probe.cpp."""
import ctypes as C
import itertools
import json
import os
import subprocess

import numpy as np
import pytest

import adaptive_batch_inputs as ab
import adaptive_segment_inputs as asi
import model_batch_inputs as mb
import model_segment_inputs as ms

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAIL_AVG, FAIL_CAP, FAIL_REPLAY, FAIL_MIX = 2, 8, 16, 32         # include/bscgpu.h: BSCGPU_DC_FAIL_*


# ---- the stand-in of the third fact ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tiny_alphabets", "escape", "hist_above_clamp", "chain_identity"])
def test_longest_chain_is_the_bincount_of_the_stand_ins_own_plane(name):
    from libbsc_amd.gpu import adaptive_longest_chain_host
    _, fb, _, poff, dbg = ab.reference(name)
    for s in range(fb.nsub):
        ids = dbg[3][int(poff[s]):int(poff[s + 1])].astype(np.int64)
        want = np.bincount(ids, minlength=ab.NUM_MIX)
        longest, per_mixer = adaptive_longest_chain_host(fb, s, per_mixer=True)
        assert per_mixer.size == ab.NUM_MIX and np.array_equal(per_mixer, want), f"{name}: sub-block {s}"
        assert longest == int(want.max()) == adaptive_longest_chain_host(fb, s)
        if name != "chain_identity":
            assert np.array_equal(np.bincount(ab.mixer_ids(fb, s).astype(np.int64), minlength=ab.NUM_MIX), per_mixer), f"{name}: sub-block {s} against the table restated"


def test_longest_chain_bad_arguments():
    from libbsc_amd import _native as N
    fb = ab.reference("tiny_alphabets")[1]
    f = N.lib().bscgpu_adaptive_longest_chain_host
    assert f(None, 0, None) == -1
    assert f(C.byref(fb.lay), fb.nsub, None) == -1
    assert f(C.byref(fb.lay), -1, None) == -1
    assert f(C.byref(fb.lay), 0, None) > 0


# ---- preconditions of the GPU tests --------------------------------------------------------------------------------------------------
def test_over_capacity_pass_is_over_as_a_whole_with_short_chains():
    _, fb, _, _, poff, mix = asi.reference("over_capacity")
    per_block = ms.block_counts(fb, np.diff(poff.astype(np.int64)))
    assert int(per_block.sum()) == 9_438_639 > ms.SMALL_CTX_DCAP and int(per_block.max()) < ms.SMALL_CTX_DCAP
    assert int(mix.max()) == 24_280 < asi.MIX_CAP_DEFAULT
    assert mb.avg_undecided(fb) == 0
    # the -e2 decisions are the static coder's: same decisions, same flags
    assert np.array_equal(np.diff(poff.astype(np.int64)), ms.sub_counts(fb, ms.STATIC))


def test_cap_sides_pass_has_blocks_on_both_sides_of_the_cap():
    _, fb, _, _, poff, mix = asi.reference("cap_sides")
    per_block = asi.block_max(fb, mix)
    above = per_block[per_block > asi.MIX_CAP_DEFAULT]
    assert sorted(int(x) for x in above) == [283_948, 476_792, 791_884]
    below = per_block[per_block <= asi.MIX_CAP_DEFAULT]
    assert below.size == fb.count - 3 and int(below.max()) < asi.MIX_CAP_BETWEEN < 476_792 and 283_948 < asi.MIX_CAP_BETWEEN
    assert mb.avg_undecided(fb) == 0, "no block is left out for another reason"
    assert int(np.diff(poff.astype(np.int64)).sum()) < 4 * ab.CTX_N, "one segment of the module context holds the pass"


@pytest.mark.parametrize("kind,sorter", [("host", 1), ("host", 5), ("device", 1), ("device", 5)])
def test_whole_call_cases_hold_one_block_above_the_default_cap(ref, kind, sorter):
    """the sorted 1 MiB - 1 block of text is the one block whose longest mixer chain is above 1 << 18 (BWT and ST5 alike): the pass a
    default-cap context declines whole and the segmented route keeps"""
    cases = mb.whole_call_cases(mb.WHOLE_SEEDS[kind, sorter])
    L = [(ref.bwt_encode(x)[0] if sorter == 1 else ref.st_encode(x, sorter)[0]) if x.size > 28 else x for x in cases]
    fb, _ = mb.layout(L)
    per_block = asi.block_max(fb, asi.longest_chains(fb))
    assert [b for b in range(fb.count) if per_block[b] > asi.MIX_CAP_DEFAULT] == [7] and cases[7].size == (1 << 20) - 1


def test_three_pass_cases_stay_under_the_default_cap(ref):
    cases = asi.three_pass_cases()
    fb, _ = mb.layout([ref.bwt_encode(x)[0] if x.size > 28 else x for x in cases])
    assert int(asi.longest_chains(fb).max()) == 208_520 < asi.MIX_CAP_DEFAULT


# ---- the plan with the third fact (tools/dc_segment_probe.cpp) ------------------------------------------------------------------------
@pytest.fixture(scope="module")
def seg_probe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("dc_segment_probe") / "dc_segment_probe")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "libbsc_amd", "csrc", "device"),
                    os.path.join(ROOT, "tools", "dc_segment_probe.cpp"), "-o", exe], check=True)

    def ask(lines):
        r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True)
        out = [json.loads(l) for l in r.stdout.splitlines()]
        assert len(out) == len(lines)
        return out
    return ask


def _seg_line(subs, dcap, target=0, cap=1 << 40, fit=0, und=(), decline=None, mix=None, mix_cap=0):
    """subs: per block the decisions of its sub-blocks; und: sub-blocks with an undecided flag; decline: {block: reason}; mix: per
    block the longest chain of its sub-blocks (None: the line ends where today's ends)"""
    blk_sub = [0]
    for b in subs:
        blk_sub.append(blk_sub[-1] + len(b))
    dec = [d for b in subs for d in b]
    f = [len(subs), len(dec), dcap, target, cap, fit, 0] + blk_sub + dec + [int(s in und) for s in range(len(dec))]
    decline = dict(decline or {})
    f += [len(decline)] + [x for b, why in sorted(decline.items()) for x in (b, why)] + [0, 0]
    if mix is not None:
        f += [mix_cap] + [m for b in mix for m in b]
    return " ".join(str(int(x)) for x in f)


def _ranges(g):
    return [(r[0], r[1], r[6]) for r in g["ranges"]]


def test_plan_bars_a_block_for_its_chain_and_ends_the_segment(seg_probe):
    subs = [[10], [20, 5], [30], [5, 5], [40]]
    mix = [[3], [9, 2], [4], [2, 8], [9]]
    got = seg_probe([
        _seg_line(subs, 200),                                              # 0: today's line: one segment
        _seg_line(subs, 200, mix=mix, mix_cap=9),                          # 1: a cap nobody exceeds (equal is allowed)
        _seg_line(subs, 200, mix=mix, mix_cap=8),                          # 2: blocks 1 and 4 are barred; block 1 ends the segment before it
        _seg_line(subs, 200, mix=mix, mix_cap=7),                          # 3: block 3 too, for its second sub-block
        _seg_line(subs, 200, mix=mix, mix_cap=8, und=(2,)),                # 4: an undecided flag comes first: sub_mix is not read there
        _seg_line([[10], [200], [30]], 100, mix=[[1], [50], [1]], mix_cap=8),      # 5: over the capacity comes before the chain
        _seg_line(subs, 200, mix=[[0], [0, 0], [0], [0, 0], [0]], mix_cap=0),      # 6: a cap of 0 with chains of 0 bars nothing
        _seg_line(subs, 200, mix=mix, mix_cap=8, decline={2: FAIL_REPLAY}),        # 7: a kept range can still decline while it runs
    ])
    assert got[0]["excluded"] == [0] * 5 and _ranges(got[0]) == [(0, 5, "kept")] and got[0]["planned"] == 1
    assert got[1] == got[0], "a third fact that bars nothing changes nothing"
    assert got[2]["excluded"] == [0, FAIL_MIX, 0, 0, FAIL_MIX] and _ranges(got[2]) == [(0, 1, "kept"), (2, 4, "kept")]
    assert (got[2]["planned"], got[2]["kept"], got[2]["reruns"], got[2]["host_blocks"], got[2]["fail"]) == (2, 2, 0, 2, FAIL_MIX)
    assert got[2]["poff"] == [0, 10, 10, 10, 40, 45, 50, 50] and got[2]["decisions"] == 50
    assert got[3]["excluded"] == [0, FAIL_MIX, 0, FAIL_MIX, FAIL_MIX] and _ranges(got[3]) == [(0, 1, "kept"), (2, 3, "kept")]
    assert got[4]["excluded"] == [0, FAIL_AVG, 0, 0, FAIL_MIX] and got[4]["fail"] == FAIL_AVG | FAIL_MIX
    assert got[5]["excluded"] == [0, FAIL_CAP, 0] and _ranges(got[5]) == [(0, 1, "kept"), (2, 3, "kept")]
    assert got[6]["excluded"] == [0] * 5 and _ranges(got[6]) == [(0, 5, "kept")]
    assert got[7]["blk_state"] == [0, FAIL_MIX, FAIL_REPLAY, 0, FAIL_MIX] and got[7]["reruns"] == 2 and got[7]["kept"] == 2


def test_plan_without_the_third_fact_is_todays(seg_probe):
    """the existing edge table's lines (tests/test_dc_segment_plan_host.py builds them the same way) end where they ended: the
    exported plan and the probe give the same segments, and FAIL_MIX never appears"""
    from libbsc_amd.gpu import model_segment_plan
    rows = [([[10], [20], [30], [40]], 100, 0, ()), ([[10], [20], [30], [41]], 100, 0, ()), ([[50], [20, 50], [10]], 100, 0, ()),
            ([[10], [20], [30]], 100, 0, (1,)), ([[60, 60], [5]], 100, 0, ()), ([[10], [], [20], [30]], 100, 25, ())]
    got = seg_probe([_seg_line(subs, dcap, target, und=und) for subs, dcap, target, und in rows])
    for (subs, dcap, target, und), g in zip(rows, got):
        dec = [d for b in subs for d in b]
        blk_sub = np.concatenate([[0], np.cumsum([len(b) for b in subs])])
        n, seg = model_segment_plan(dec, [int(s in und) for s in range(len(dec))], blk_sub, dcap, target)
        assert g["planned"] == n and not any(x == FAIL_MIX for x in g["blk_state"])
        kept = [(r[0], r[1]) for r in g["ranges"]]
        members = [b for b in range(len(subs)) if subs[b] and seg[b] >= 0]
        assert sorted(b for a, e in kept for b in range(a, e) if subs[b]) == members
        for a, e in kept:
            assert len({seg[b] for b in range(a, e) if subs[b]}) == 1, "a range is one segment of the plan"


# ---- the route (tools/batch_pass_probe.cpp) ---------------------------------------------------------------------------------------------
OPTS = ("front", "model", "fast", "segments", "packed", "device_rc")


@pytest.fixture(scope="module")
def pass_probe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("batch_pass_probe") / "batch_pass_probe")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "libbsc_amd", "csrc", "host"),
                    os.path.join(ROOT, "tools", "batch_pass_probe.cpp"), "-o", exe], check=True)

    def ask(lines):
        r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True)
        out = [json.loads(l) for l in r.stdout.splitlines()]
        assert len(out) == len(lines)
        return out
    return ask


def _pass_line(opts, coder, trailing=(), state=(0, 0), mrc=0):
    """a call of one pass of two blocks with a segmented model's answer; trailing: () as today, (adaptive_segments,) or
    (adaptive_segments, model_adaptive)"""
    sizes = [1000, 2000]
    f = [2, 1, coder, 4 << 20, 0] + list(opts) + [0, 0, 0, 1, 1, 1 << 24] + sizes + sizes + [1, 0, 2, mrc, 3000, 0, 0, len(state)] + list(state)
    return " ".join(str(int(x)) for x in f + list(trailing))


def test_new_option_routes_only_the_adaptive_coder_with_its_model_on(pass_probe):
    lines, keys = [], []
    for opts, coder in itertools.product(itertools.product(*[(0, 1)] * 6), (1, 2, 3)):
        for trailing in ((), (0,), (1,), (0, 1), (1, 0), (1, 1)):
            lines.append(_pass_line(opts, coder, trailing))
            keys.append((opts, coder, trailing))
    got = dict(zip(keys, pass_probe(lines)))
    for (opts, coder, trailing), g in got.items():
        today = got[opts, coder, ()]
        o = dict(zip(OPTS, opts))
        if trailing in ((0,), (1,), (1, 0)):
            # without BSCGPU_OPT_BATCH_MODEL_ADAPTIVE the new option is nobody's: today's route, whatever the coder
            rest = {k: v for k, v in g.items() if k not in ("adaptive_model", "passes")}
            assert rest == {k: v for k, v in today.items() if k != "passes"} and g["adaptive_model"] == 0, (opts, coder, trailing)
            for r, t in zip(g["passes"], today["passes"]):
                assert {k: v for k, v in r.items() if k != "adaptive"} == t and r["adaptive"] == [0, 0]
        if trailing in ((0, 1), (1, 1)):
            adaptive = bool(o["front"]) and coder == 2
            assert g["adaptive_model"] == int(adaptive)
            if not adaptive:                                           # -e1 and -e0 are untouched by either option
                assert g["route"] == today["route"] and [r["step"] for r in g["passes"]] == [r["step"] for r in today["passes"]]
                assert all(r["adaptive"] == [0, 0] for r in g["passes"])
                continue
            seg = trailing[0]
            assert g["route"] == [1, 1, 0, seg, 0, 0], "segments only by its own option; packed and the device's range coder never"
            r = g["passes"][0]
            assert r["step"] == ("segments" if seg else "whole") and r["adaptive"] == [1, 0] and r["sources"] == ["ps16"] * 2
            assert r["counters"]["model"] == r["counters"]["fast"] == r["counters"]["packed"] == r["counters"]["device_rc"] == 0


def test_segmented_adaptive_pass_counts_by_the_segmented_verdict(pass_probe):
    on = (1, 0, 0, 0, 0, 0)
    got = pass_probe([_pass_line(on, 2, (1, 1), state=(0, FAIL_MIX)), _pass_line(on, 2, (1, 1), state=(FAIL_MIX, FAIL_CAP)),
                      _pass_line(on, 2, (1, 1), mrc=-4), _pass_line(on, 2, (1, 1), mrc=-8)])
    r = [g["passes"][0] for g in got]
    assert (r[0]["kept"], r[0]["adaptive"], r[0]["sources"]) == (1, [1, 0], ["ps16", "runs"]), "kept where the stream serves any block"
    assert (r[1]["kept"], r[1]["adaptive"], r[1]["sources"]) == (0, [0, 1], ["runs", "runs"])
    assert (r[2]["kept"], r[2]["adaptive"]) == (0, [0, 1]), "an arena that did not fit: declined"
    assert got[3]["error"] == -8
