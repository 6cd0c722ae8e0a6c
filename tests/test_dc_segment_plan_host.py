"""The schedule of a pass in model segments (libbsc_amd/csrc/device/dc_segment_plan.h — what devcoder_pstream_segments launches by)
judged on the CPU through tools/dc_segment_probe.cpp, where a rule stands for the model: against pipeline_model.segment_schedule (the
driver's host side restated from the function it was taken out of) over a fixed-seed sweep of about two thousand passes, and against a
hand-written table of its edges."""
import json
import os
import random
import subprocess

import pytest

from pipeline_model import FAIL_AVG, FAIL_CAP, segment_counters, segment_schedule

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIST, REPLAY = 4, 16                                            # BSCGPU_DC_FAIL_HIST / _REPLAY: what a range can decline with while it runs


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("dc_segment_probe") / "dc_segment_probe")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "libbsc_amd", "csrc", "device"),
                    os.path.join(ROOT, "tools", "dc_segment_probe.cpp"), "-o", exe], check=True)

    def ask(scenarios):
        r = subprocess.run([exe], input="\n".join(_line(**sc) for sc in scenarios) + "\n", capture_output=True, text=True, check=True)
        out = [json.loads(l) for l in r.stdout.splitlines()]
        assert len(out) == len(scenarios)
        return out
    return ask


def _scenario(subs, dcap, target=0, cap=1 << 40, fit=0, packed=0, und=(), decline=None, void=(), skew=()):
    """subs: per block the decisions of its sub-blocks; und: sub-blocks with an undecided flag; decline: {block: reason}"""
    blk_sub = [0]
    for b in subs:
        blk_sub.append(blk_sub[-1] + len(b))
    dec = [d for b in subs for d in b]
    return dict(blk_sub=blk_sub, dec=dec, und=[int(s in und) for s in range(len(dec))], dcap=dcap, target=target, cap=cap, fit=fit, packed=packed,
                decline=dict(decline or {}), void=sorted(void), skew=sorted(skew))


def _line(blk_sub, dec, und, dcap, target, cap, fit, packed, decline, void, skew):
    f = [len(blk_sub) - 1, len(dec), dcap, target, cap, fit, packed] + blk_sub + dec + und + [len(decline)]
    for b, why in sorted(decline.items()):
        f += [b, why]
    return " ".join(str(x) for x in f + [len(void)] + void + [len(skew)] + skew)


def _model(sc):
    """the probe's rule: (OR of the reasons of the range's declining blocks, holds a void block, holds a skewed block)"""
    def model(b0, b1):
        why = 0
        for b, w in sc["decline"].items():
            if b0 <= b < b1:
                why |= w
        return why, any(b0 <= b < b1 for b in sc["void"]), any(b0 <= b < b1 for b in sc["skew"])
    return model


def _restated(sc):
    return segment_schedule(sc["dec"], sc["und"], sc["blk_sub"], sc["dcap"], sc["target"], sc["cap"], sc["fit"], sc["packed"], _model(sc))


def _sweep():
    rng = random.Random(20261019)
    out = []
    for i in range(2000):
        count = rng.randint(1, 40) if i % 4 else rng.randint(1, 6)
        sizes = [0, 1, 63, 64, 65, 128]
        subs = [[rng.choice(sizes) if rng.random() < 0.3 else rng.randint(0, 5000) for _ in range(rng.choice([0, 1, 1, 2, 2]))] for _ in range(count)]
        per_block = sorted(sum(b) for b in subs)
        total = sum(per_block)
        # the arena: holds every block, all but the largest (an over-Dcap block), or about a third of the pass
        dcap = max(1, rng.choice([per_block[-1], per_block[-1] - 1, total // 3, total + 1]))
        nsub = sum(len(b) for b in subs)
        und = {s for s in range(nsub) if rng.random() < 0.06}
        target = rng.choice([0, -1, dcap // 4, dcap - 1, dcap, dcap + 1, 4 * dcap])
        packed, fit = rng.randint(0, 1), rng.randint(0, 1)
        members = [b for b in range(count) if subs[b]]
        decline = {b: rng.choice([HIST, REPLAY]) for b in rng.sample(members, min(len(members), rng.choice([0, 0, 1, 2, 3])))}
        void = rng.sample(members, min(len(members), rng.choice([0, 0, 1, 2]))) if packed else []
        sc = _scenario(subs, dcap, target, 0, fit, packed, und, decline, void)
        need = _restated(sc)["need"]
        sc["cap"] = max(0, rng.choice([need - 1, need, need + 1, need // 2, need // 3, 2 * need, 0]))
        out.append(sc)
    return out


def test_schedule_equals_the_restatement_over_a_sweep(probe):
    sweep = _sweep()
    got = probe(sweep)
    seen = dict(split=0, gave_up=0, nofit=0, void=0, kept=0, avg=0, cap=0, counted=0, budget=0, inner_empty=0, edge_empty=0)
    for sc, g in zip(sweep, got):
        want = _restated(sc)
        assert g == want, (sc, g, want)
        for r in g["ranges"]:
            seen[r[6]] += 1
            empties = [b for b in range(r[0], r[1]) if sc["blk_sub"][b] == sc["blk_sub"][b + 1]]
            seen["inner_empty"] += any(r[0] < b < r[1] - 1 for b in empties)
            seen["edge_empty"] += any(b in (r[0], r[1] - 1) for b in empties)
            seen["budget"] += r[6] == "gave_up" and sum(sc["blk_sub"][b] < sc["blk_sub"][b + 1] for b in range(r[0], r[1])) >= 2
        seen["avg"] += FAIL_AVG in g["excluded"]
        seen["cap"] += FAIL_CAP in g["excluded"]
        seen["counted"] += not g["copy_all"]
    assert all(seen.values()), f"the sweep never reached: {[k for k, v in seen.items() if not v]}"


def _outcomes(g):
    return [(r[0], r[1], r[6]) for r in g["ranges"]]


def test_schedule_at_its_edges(probe):
    one = lambda *dec: [[d] for d in dec]
    table = [
        # 0: an exact tie of |2 acc - expect| (10 | 20 10 and 10 20 | 10 are 20 off both): the first boundary found wins
        _scenario(one(10, 20, 10), 1000, decline={2: HIST}),
        # 1: a range of two members
        _scenario(one(5, 7), 1000, decline={0: REPLAY}),
        # 2: after the cut, a range whose only other "members" are empty blocks: given up without a re-run of its own
        _scenario([[5], [], [7]], 1000, decline={2: HIST}),
        # 3: the re-run budget hit exactly: 8 blocks allow 2 * 3 + 2 = 8; the split that takes them to 8 is made, the next range that
        # declines is given up whole
        _scenario(one(*[10] * 8), 1000, decline={0: HIST, 7: REPLAY}),
        # 4, 5: per_segment_fit: base + need == cap is kept, one less is not
        _scenario(one(10, 10), 1000, target=10, cap=20, fit=1),
        _scenario(one(10, 10), 1000, target=10, cap=19, fit=1),
        # 6: the packed need of sub-blocks of 0, 1, 64 and 65 decisions: 0, 104, 104 and 208 bytes
        _scenario(one(0, 1, 64, 65), 1000, target=1, packed=1),
        # 7: a void segment: the fields of its sub-blocks derived from their decisions
        _scenario([[1, 65]], 1000, packed=1, void=[0]),
        # 8: excluded blocks end a segment on both sides (an undecided flag; more decisions than the arena holds); the sub-blocks that are
        # never modelled end where their predecessor does
        _scenario([[10], [10], [3, 7], [10], [101], [10]], 100, und={3}),
        # 9: a packed layout that is not the plan's ends the pass
        _scenario(one(10, 10), 1000, target=10, packed=1, skew=[1]),
        # 10: not per_segment_fit and the plan over the buffer: counted, not copied — nothing is given up for room
        _scenario(one(10, 10), 1000, target=10, cap=19, fit=0),
    ]
    g = probe(table)
    for sc, got in zip(table, g):
        assert got == _restated(sc), sc

    assert _outcomes(g[0]) == [(0, 3, "split"), (0, 1, "kept"), (1, 3, "split"), (1, 2, "kept"), (2, 3, "gave_up")]
    assert (g[0]["blk_state"], g[0]["poff"], g[0]["kept"], g[0]["reruns"], g[0]["host_blocks"]) == ([0, 0, HIST], [0, 10, 30, 30], 2, 4, 1)

    assert _outcomes(g[1]) == [(0, 2, "split"), (0, 1, "gave_up"), (1, 2, "kept")]
    assert (g[1]["blk_state"], g[1]["poff"], g[1]["reruns"], g[1]["fail"]) == ([REPLAY, 0], [0, 0, 7], 2, REPLAY)

    assert _outcomes(g[2]) == [(0, 3, "split"), (0, 1, "kept"), (1, 3, "gave_up")]
    assert (g[2]["blk_state"], g[2]["reruns"], g[2]["host_blocks"]) == ([0, 0, HIST], 2, 1), "the empty block carries no reason"

    assert _outcomes(g[3]) == [(0, 8, "split"), (0, 4, "split"), (0, 2, "split"), (0, 1, "gave_up"), (1, 2, "kept"), (2, 4, "kept"),
                               (4, 8, "split"), (4, 6, "kept"), (6, 8, "gave_up")]
    assert (g[3]["blk_state"], g[3]["reruns"], g[3]["kept"], g[3]["host_blocks"]) == ([HIST, 0, 0, 0, 0, 0, REPLAY, REPLAY], 8, 3, 3)
    assert g[3]["poff"] == [0, 0, 10, 20, 30, 40, 50, 50, 50] and g[3]["fail"] == HIST | REPLAY

    assert _outcomes(g[4]) == [(0, 1, "kept"), (1, 2, "kept")] and g[4]["blk_state"] == [0, 0] and [r[7] for r in g[4]["ranges"]] == [0, 10]
    assert _outcomes(g[5]) == [(0, 1, "kept"), (1, 2, "nofit")] and g[5]["blk_state"] == [0, FAIL_CAP] and g[5]["poff"] == [0, 10, 10]
    assert g[5]["copy_all"] and g[5]["decisions"] == 10

    assert [(r[0], r[1], r[5]) for r in g[6]["ranges"]] == [(0, 2, 104), (2, 3, 104), (3, 4, 208)] and g[6]["need"] == 416
    assert g[6]["pbase"] == [0, 0, 64, 128, 256] and [x // 8 * 13 for x in g[6]["pbase"]] == [0, 0, 104, 208, 416]
    assert [r[7] for r in g[6]["ranges"]] == [0, 104, 208] and (g[6]["packed"], g[6]["void"]) == (3, 0)

    assert _outcomes(g[7]) == [(0, 1, "void")] and g[7]["pbase"] == [0, 64, 192] and (g[7]["packed"], g[7]["void"], g[7]["need"]) == (0, 1, 312)

    assert g[8]["excluded"] == [0, 0, FAIL_AVG, 0, FAIL_CAP, 0] and g[8]["planned"] == 3
    assert _outcomes(g[8]) == [(0, 2, "kept"), (3, 4, "kept"), (5, 6, "kept")]
    assert g[8]["poff"] == [0, 10, 20, 20, 20, 30, 30, 40] and (g[8]["host_blocks"], g[8]["fail"]) == (2, FAIL_AVG | FAIL_CAP)

    assert g[9]["error"] and _outcomes(g[9]) == [(0, 1, "kept"), (1, 2, "layout")] and "poff" not in g[9]

    assert not g[10]["copy_all"] and _outcomes(g[10]) == [(0, 1, "kept"), (1, 2, "kept")] and g[10]["decisions"] == 20


def test_counters_of_three_blocks_with_the_middle_one_declining():
    """what test_gpu_model_segments.py holds the device's counters to, for any three blocks that fit one segment: the pass declines and
    is cut twice (4 re-runs), the outer blocks are kept, the middle one is the host's; left out by the plan instead: no re-run"""
    for dec in ([100, 50, 100], [7, 900, 3], [500, 1, 2]):
        assert segment_counters(dec, [0, 1, 2, 3], 10_000, decline={1}) == (2, 4, 1)
        assert segment_counters(dec, [0, 1, 2, 3], 10_000, decline={1}, und=[0, 1, 0]) == (2, 0, 1)
