"""What the driver of a batched-compress call decides (libbsc_amd/csrc/host/batch_pass_plan.h — the rules compress_batch_impl acts on)
judged on the CPU through tools/batch_pass_probe.cpp, where the device's answers are read from the input: against
pipeline_model.batch_call (the driver's decisions restated from the function they were taken out of) over a fixed-seed sweep of about
two thousand calls, and against a hand-written table of its edges."""
import itertools
import json
import os
import random
import subprocess

import pytest

from pipeline_model import BATCH_FAST_MIN_PASS, BATCH_MAX_BLOCKS, BATCH_MAX_N, BATCH_MIN_PASS, NOT_SUPPORTED, batch_call

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GPU_ERROR = -8                                                   # any code of a model that is neither success nor "declined"
OPTS = ("front", "model", "fast", "segments", "packed", "device_rc")


def build_probe(exe, extra=()):
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", *extra, "-I", os.path.join(ROOT, "libbsc_amd", "csrc", "host"),
                    os.path.join(ROOT, "tools", "batch_pass_probe.cpp"), "-o", exe], check=True)


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("batch_pass_probe") / "batch_pass_probe")
    build_probe(exe)

    def ask(calls):
        r = subprocess.run([exe], input="\n".join(line(c) for c in calls) + "\n", capture_output=True, text=True, check=True)
        out = [json.loads(l) for l in r.stdout.splitlines()]
        assert len(out) == len(calls)
        return out
    return ask


def call(sizes, sorter=1, coder=1, cap=4 << 20, dev=0, lz=None, min_pass=0, target=0, front_host=1, model_host=1, entries=1 << 24, facts=None, **opts):
    """opts: the option values by name (default 0); facts: {pass: dict(nsub, mrc, D, pk, pbytes, blk_state)}"""
    return dict(sizes=list(sizes), sorter=sorter, coder=coder, cap=cap, dev=dev, lz=list(sizes) if lz is None else list(lz), min_pass=min_pass, target=target,
                front_host=front_host, model_host=model_host, entries=entries, facts=dict(facts or {}), opts={k: opts.get(k, 0) for k in OPTS})


def line(c):
    mins = (BATCH_MIN_PASS, BATCH_FAST_MIN_PASS) if c["min_pass"] is None else (c["min_pass"], c["min_pass"])
    f = [len(c["sizes"]), c["sorter"], c["coder"], c["cap"], c["dev"]] + [c["opts"][k] for k in OPTS]
    f += [mins[0], mins[1], c["target"], c["front_host"], c["model_host"], c["entries"]] + c["sizes"] + c["lz"] + [len(c["facts"])]
    for p, x in sorted(c["facts"].items()):
        st = x.get("blk_state", [])
        f += [p, x.get("nsub", 0), x.get("mrc", 0), x.get("D", 0), x.get("pk", 0), x.get("pbytes", 0), len(st)] + list(st)
    return " ".join(str(int(v)) for v in f)


def restated(c):
    return batch_call(c["sizes"], c["sorter"], c["coder"], c["cap"], bool(c["dev"]), c["lz"], c["opts"], c["facts"], c["entries"], c["min_pass"],
                      c["target"], bool(c["front_host"]), bool(c["model_host"]))


def sweep():
    rng = random.Random(20261020)
    combos = list(itertools.product(*[(0, 1)] * 6, (1, 2, 3), (1, 5)))                 # every option set x coder x BWT / ST5: 384
    rng.shuffle(combos)
    out = []
    for i in range(2000):
        *o, coder, sorter = combos[i % len(combos)]
        cap = rng.choice([100_000, 300_000, 2 << 20, 4 << 20])
        edge = [0, 1, 15, 16, 27, 28, 29, 30, 65535, 65536, BATCH_MAX_N - 1, BATCH_MAX_N, cap, cap + 1]
        if i == 7:
            sizes = [rng.choice([0, 1, 20, 29, 40, 200]) for _ in range(5000)]         # the block cap cuts
        else:
            sizes = [rng.choice(edge) if rng.random() < 0.35 else 0 if rng.random() < 0.15 else rng.randint(1, rng.choice([100, 70_000, 400_000]))
                     for _ in range(rng.randint(1, 40) if i % 4 else rng.randint(1, 5))]
        dev = rng.randint(0, 1)
        lzp = not dev and rng.random() < 0.4
        lz = [n if not lzp or n <= 28 or rng.random() < 0.3 else rng.choice([8, 15, 16, 17, n // 2, n]) for n in sizes]
        c = call(sizes, sorter, coder, cap, dev, lz, rng.choice([None, 0, 0, 0]), rng.choice([0, 0, 1000]), int(rng.random() < 0.9), int(rng.random() < 0.9),
                 rng.choice([1000, 50_000, 1 << 22]), **dict(zip(OPTS, o)))
        plain = restated(c)["passes"]
        if plain and c["min_pass"] == 0 and rng.random() < 0.3:                         # the smallest modelled pass at one pass's own size
            c["min_pass"] = max(0, rng.choice(plain)["pos"] + rng.choice([-1, 0, 1]))
        for p, row in enumerate(plain):
            n, ent = len(row["psz"]), c["entries"]
            c["facts"][p] = dict(nsub=0 if rng.random() < 0.05 else sum(x > 0 for x in row["psz"]), mrc=rng.choice([0] * 8 + [NOT_SUPPORTED, GPU_ERROR]),
                                 D=ent + rng.choice([-1, 0, 1, -ent // 2, ent]), pk=int(rng.random() < 0.7), pbytes=2 * ent - 8 + rng.choice([-1, 0, 1, -ent, ent]),
                                 blk_state=[rng.choice([0, 0, 0, 2, 8]) if rng.random() < 0.8 else 8 for _ in range(n)] if rng.random() < 0.7 else [8] * n)
        out.append(c)
    return out


def test_decisions_equal_the_restatement_over_a_sweep(probe):
    calls = sweep()
    got = probe(calls)
    seen = dict(block_cap=0, byte_cap=0, error=0, l_down=0, none=0, whole=0, segments=0, kept_whole=0, host_whole=0, declined=0, kept_segments=0, fast=0,
                packed=0, void=0, device_rc=0, one_by_one=0, pipe=0, inner_empty=0, first_empty=0, last_empty=0,
                **{k: 0 for k in ("empty", "stored", "rides", "single", "sorted", "l", "runs", "ps16", "ps13", "device_rc_src")})
    for c, g in zip(calls, got):
        want = restated(c)
        assert g == want, (c, g, want)
        seen["error"] += g["error"] != 0
        seen["first_empty"] += c["sizes"][0] == 0
        seen["last_empty"] += c["sizes"][-1] == 0
        spans = [r["e"] - r["b"] for r in g["passes"]]
        seen["block_cap"] += BATCH_MAX_BLOCKS in spans
        seen["byte_cap"] += any(g["passes"][i + 1]["b"] == r["e"] and r["e"] - r["b"] < BATCH_MAX_BLOCKS for i, r in enumerate(g["passes"][:-1]))
        for r in g["passes"]:
            seen[r["step"]] += 1
            seen["inner_empty"] += "empty" in r["classes"]
            for k in set(r["classes"]):
                seen[k] += 1
            for k in set(r.get("sources", [])) - {""}:
                seen["device_rc_src" if k == "device_rc" else k] += 1
            n = r["counters"]
            if r["step"] in ("whole", "segments"):
                seen["kept_" + r["step"]] += r["kept"]
            seen["host_whole"] += r["step"] == "whole" and not r["kept"] and not n["declined"] and not n["fast_declined"] and not g["error"]
            seen["declined"] += n["declined"] + n["fast_declined"]
            for k in ("fast", "packed", "void", "device_rc"):
                seen[k] += n[k]
        for k in set(g["leftover"]) - {"none"}:
            seen[k] += 1
    assert all(seen.values()), f"the sweep never reached: {[k for k, v in seen.items() if not v]}"


def test_landing_room_on_both_sides_of_its_boundary(probe):
    sizes, ent = [1000, 2000], 5000
    rows = [(dict(D=ent), 0, 1), (dict(D=ent + 1), 0, 0), (dict(pk=1, pbytes=2 * ent - 8, D=10 * ent), 1, 1), (dict(pk=1, pbytes=2 * ent - 7), 1, 0),
            (dict(pk=0, D=ent), 1, 1), (dict(pk=0, D=ent + 1, pbytes=0), 1, 0), (dict(pk=1, pbytes=0, D=ent + 1), 0, 0)]
    calls = [call(sizes, entries=ent, front=1, model=1, packed=packed, facts={0: dict(nsub=2, **f)}) for f, packed, _ in rows]
    for c, g, (f, packed, kept) in zip(calls, probe(calls), rows):
        assert g == restated(c)
        r = g["passes"][0]
        assert (r["step"], r["kept"], r["counters"]["model"]) == ("whole", kept, kept), f
        assert (r["counters"]["packed"], r["counters"]["void"]) == ((kept * f.get("pk", 0), kept * (1 - f.get("pk", 0))) if packed else (0, 0)), f
        assert r["sources"] == [("ps13" if packed and f.get("pk") else "ps16") if kept else "runs"] * 2


def test_decisions_at_their_edges(probe):
    on = dict(front=1, model=1)
    table = [
        # 0: host input, a pass of only empty and stored blocks: nothing is sorted, no counter moves
        call([10, 0, 28, 5], **on),
        # 1: the same from HBM: the blocks ride along, the pass is sorted and takes the front end; its layout has sub-blocks, so it is modelled
        call([10, 0, 28, 5], dev=1, facts={0: dict(nsub=3)}, **on),
        # 2: nsub == 0: no model
        call([1000, 2000], facts={0: dict(nsub=0)}, **on),
        # 3, 4: pos one below the minimum pass, and at it
        call([1000, 2000], min_pass=3001, facts={0: dict(nsub=2)}, **on),
        call([1000, 2000], min_pass=3000, facts={0: dict(nsub=2)}, **on),
        # 5: the device declines the whole pass; 6: it fails: the call ends there
        call([1000, 2000, BATCH_MAX_N, 500], facts={0: dict(nsub=2, mrc=NOT_SUPPORTED), 1: dict(nsub=1)}, **on),
        call([1000, 2000, BATCH_MAX_N, 500], facts={0: dict(nsub=2, mrc=GPU_ERROR), 1: dict(nsub=1)}, **on),
        # 7: segments requested with the device's range coder on: whole passes, coded on the device
        call([1000, 2000], segments=1, device_rc=1, facts={0: dict(nsub=2)}, **on),
        # 8: segments: one block is the host's; 9: every block is: the pass counts as declined; 10: an arena did not fit
        call([1000, 2000, 0, 30], segments=1, packed=1, facts={0: dict(nsub=3, blk_state=[0, 8, 0, 0])}, **on),
        call([1000, 2000], segments=1, facts={0: dict(nsub=2, blk_state=[2, 8])}, **on),
        call([1000, 2000], segments=1, facts={0: dict(nsub=2, mrc=NOT_SUPPORTED, blk_state=[8, 8])}, **on),
        # 11: LZP leaves fewer than 16 bytes of a block: the single path decides, one by one; ST has no aux indexes and sorts it
        call([4096, 1000], lz=[9, 1000]),
        call([4096, 1000], sorter=5, lz=[9, 1000]),
        # 13: -e0 takes its own option and counters; 14: -e2 has no device model; 15: the pinned stream buffers are not to be had
        call([1000, 2000], coder=3, front=1, model=1, fast=1, packed=1, facts={0: dict(nsub=2, pk=1)}),
        call([1000, 2000], coder=2, front=1, model=1, fast=1, facts={0: dict(nsub=2)}),
        call([1000, 2000], model_host=0, facts={0: dict(nsub=2)}, **on),
        # 16, 17: larger than the context, at BSCGPU_BATCH_MAX_N, empty outside a pass (an empty block's result comes from the single path): host and HBM
        call([5 << 20, BATCH_MAX_N, 0, 20, 1000], cap=4 << 20),
        call([5 << 20, BATCH_MAX_N, 0, 20, 1000], cap=4 << 20, dev=1),
        # 18: the pinned run buffers are not to be had: L comes down
        call([1000], front_host=0, **on),
    ]
    g = probe(table)
    for c, got in zip(table, g):
        assert got == restated(c), c
    zero = dict(front=0, l=0, model=0, declined=0, fast=0, fast_declined=0, packed=0, void=0, device_rc=0)
    row = lambda i, p=0: g[i]["passes"][p]

    assert (row(0)["classes"], row(0)["pos"], row(0)["step"], row(0)["counters"]) == (["stored", "empty", "stored", "stored"], 0, "none", zero)
    assert g[0]["leftover"] == ["none", "one_by_one", "none", "none"] and g[0]["pass_of"] == [0, -1, 0, 0]
    assert (row(1)["classes"], row(1)["psz"], row(1)["prate"], row(1)["at"], row(1)["pos"]) == (["rides", "empty", "rides", "rides"], [10, 0, 28, 5], [-1] * 4, [0, 10, 10, 38], 43)
    assert (row(1)["step"], row(1)["kept"], row(1)["counters"]) == ("whole", 1, dict(zero, front=1, model=1))
    assert (row(2)["step"], row(2)["counters"], row(2)["sources"]) == ("none", dict(zero, front=1), ["runs", "runs"])
    assert (row(3)["step"], row(4)["step"], row(4)["sources"]) == ("none", "whole", ["ps16", "ps16"])
    assert (row(5)["counters"], row(5)["sources"], len(g[5]["passes"]), g[5]["leftover"]) == (dict(zero, front=1, declined=1), ["runs"] * 2, 2, ["none", "none", "pipe", "none"])
    assert (g[6]["error"], len(g[6]["passes"]), row(6)["counters"], g[6]["leftover"]) == (GPU_ERROR, 1, dict(zero, front=1), [])
    assert (g[7]["route"], row(7)["step"], row(7)["counters"], row(7)["sources"]) == ([1, 1, 0, 0, 0, 1], "whole", dict(zero, front=1, model=1, device_rc=1), ["device_rc"] * 2)
    assert (row(8)["step"], row(8)["kept"], row(8)["counters"], row(8)["sources"]) == ("segments", 1, dict(zero, front=1, model=1), ["ps13", "runs", "", "ps13"])
    assert (row(8)["psz"], row(8)["prate"], row(8)["at"]) == ([1000, 2000, 0, 30], [64, 128, -1, 2], [0, 1000, 3000, 3000])
    for i in (9, 10):
        assert (row(i)["step"], row(i)["kept"], row(i)["counters"], row(i)["sources"]) == ("segments", 0, dict(zero, front=1, declined=1), ["runs"] * 2)
    assert (row(11)["classes"], row(11)["psz"], row(11)["pos"], g[11]["leftover"]) == (["single", "sorted"], [0, 1000], 1000, ["one_by_one", "none"])
    assert (row(12)["classes"], row(12)["psz"], row(12)["prate"], g[12]["leftover"]) == (["sorted", "sorted"], [9, 1000], [0, 0], ["none", "none"])
    assert (g[13]["route"], row(13)["counters"], row(13)["sources"]) == ([1, 1, 1, 0, 0, 0], dict(zero, front=1, fast=1), ["fast"] * 2)
    assert (g[14]["route"], row(14)["step"]) == ([1, 0, 0, 0, 0, 0], "none")
    assert (row(15)["step"], row(15)["counters"]) == ("none", dict(zero, front=1))
    assert (g[16]["pass_of"], g[16]["leftover"]) == ([-1, -1, -1, 0, 0], ["one_by_one", "pipe", "one_by_one", "none", "none"])
    assert (g[17]["pass_of"], g[17]["leftover"]) == ([-1, -1, -1, 0, 0], ["one_by_one", "pipe", "pipe", "none", "none"])
    assert (g[18]["route"], row(18)["step"], row(18)["counters"], row(18)["sources"]) == ([0] * 6, "l_down", dict(zero, l=1), ["l"])
