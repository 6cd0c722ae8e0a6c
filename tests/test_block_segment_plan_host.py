"""The host arithmetic of a single block's device model (libbsc_amd/csrc/device/dc_block_plan.h) judged on the CPU through
tools/block_plan_probe.cpp.  The plan of a block in sub-block segments — what devcoder_block_begin cuts by and block.cpp's sender copies
by: against a Python restatement over a fixed-seed sweep of random tables, against brute force over all cut sets, at its edges, and its
joining of the segments' streams against the layout of bscgpu_pstream_pack13_host.  The schedule of a block modelled in one go — what
gpu_stage lands a whole stream by and the stage functions lay their output out by: against the arithmetic gpu_stage had of its own.
max_rank of a sub-block, and the three decisions of the driver of one block, every combination against the conditions they replace.
The probe is also built with AddressSanitizer and UBSan and run, as that program, on the same inputs."""
import itertools
import json
import os
import random
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD_PARAMETER, NOT_SUPPORTED = -1, -4
UNTOUCHED = [-7] * 8


def _build(tmp_path_factory, name, extra):
    exe = str(tmp_path_factory.mktemp(name) / name)
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", *extra, "-I", os.path.join(ROOT, "libbsc_amd", "csrc", "device"),
                    os.path.join(ROOT, "tools", "block_plan_probe.cpp"), "-o", exe], check=True)
    return exe


def _ask(exe, scenarios, env=None):
    text = "\n".join(sc if isinstance(sc, str) else _line(**sc) for sc in scenarios) + "\n"
    r = subprocess.run([exe], input=text, capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    out = [json.loads(l) for l in r.stdout.splitlines()]
    assert len(out) == len(scenarios)
    return out, r.stderr


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    exe = _build(tmp_path_factory, "block_plan_probe", [])
    return lambda scenarios: _ask(exe, scenarios)[0]


def _scenario(runs, dec, mcap, dcap, packed=0, nsub=None, nullmask=0, void_seg=-1):
    return dict(nsub=len(runs) if nsub is None else nsub, runs=list(runs), dec=list(dec), mcap=mcap, dcap=dcap, packed=packed, nullmask=nullmask,
                void_seg=void_seg)


def _line(nsub, runs, dec, mcap, dcap, packed, nullmask, void_seg):
    return " ".join(str(x) for x in [nsub, len(runs), mcap, dcap, packed, nullmask, void_seg] + runs + dec)


def _restated(sc):
    """the rules of the plan, restated: -> rc, seg_of"""
    runs, dec, n = sc["runs"], sc["dec"], sc["nsub"]
    if sc["nullmask"] or not 1 <= n <= 8 or sc["mcap"] <= 0 or sc["dcap"] <= 0:
        return BAD_PARAMETER, None
    if any(r > sc["mcap"] or d > sc["dcap"] for r, d in zip(runs[:n], dec[:n])):
        return NOT_SUPPORTED, None
    seg_of, r_sum, d_sum = [], 0, 0
    for s in range(n):
        if s == 0 or r_sum + runs[s] > sc["mcap"] or d_sum + dec[s] > sc["dcap"]:
            seg_of.append(seg_of[-1] + 1 if seg_of else 0)
            r_sum = d_sum = 0
        else:
            seg_of.append(seg_of[-1])
        r_sum += runs[s]
        d_sum += dec[s]
    return seg_of[-1] + 1, seg_of


def _fewest_by_brute_force(sc):
    """the fewest contiguous segments within both capacities over all 2^(nsub - 1) cut sets (None: no cut set is within them)"""
    runs, dec, n = sc["runs"], sc["dec"], sc["nsub"]
    best = None
    for cuts in itertools.product((0, 1), repeat=n - 1):
        bounds = [0] + [s + 1 for s in range(n - 1) if cuts[s]] + [n]
        if all(sum(runs[a:b]) <= sc["mcap"] and sum(dec[a:b]) <= sc["dcap"] for a, b in zip(bounds, bounds[1:])):
            best = len(bounds) - 1 if best is None else min(best, len(bounds) - 1)
    return best


def _pack13_layout(dec):
    """pbase of bscgpu_pstream_pack13_host for sub-blocks of these sizes (entries of any value), and the packed bytes"""
    from libbsc_amd.gpu import pstream_pack13_host
    poff = np.concatenate([[0], np.cumsum(dec)]).astype(np.uint32)
    ps = (np.arange(int(poff[-1]), dtype=np.uint32) * 40503 + 977).astype(np.uint16)
    return pstream_pack13_host(ps, poff)


def _check_schedule(sc, got):
    """what DcBlockSchedule derives of a plan: offsets, rebased run tables, the pieces' places"""
    runs, dec, n, packed = sc["runs"], sc["dec"], sc["nsub"], sc["packed"]
    poff = [0]
    pbase = [0]
    for d in dec[:n]:
        poff.append(poff[-1] + d)
        pbase.append(pbase[-1] + (d + 63) // 64 * 64)
    first = [0]
    for r in runs[:n]:
        first.append(first[-1] + r)
    assert got["poff"] == poff and got["pbase"] == pbase
    assert got["zone"] == (pbase[-1] // 8 * 13 if packed else 2 * poff[-1])
    assert got["segments"] == got["rc"] == len(got["segs"])
    for i, g in enumerate(got["segs"]):
        members = [s for s in range(n) if got["seg_of"][s] == i]
        assert (g["s0"], g["s1"]) == (members[0], members[-1] + 1)
        assert (g["r0"], g["r1"]) == (first[g["s0"]], first[g["s1"]]) and g["expect"] == poff[g["s1"]] - poff[g["s0"]]
        assert g["first"] == [first[min(g["s0"] + b, g["s1"])] - g["r0"] for b in range(9)]
        for k, s in enumerate(members):
            if packed:
                assert (g["src"][k], g["dst"][k], g["len"][k]) == ((pbase[s] - pbase[g["s0"]]) // 8 * 13, pbase[s] // 8 * 13, (dec[s] + 7) // 8 * 13)
            else:
                assert (g["src"][k], g["dst"][k], g["len"][k]) == (2 * (poff[s] - poff[g["s0"]]), 2 * poff[s], 2 * dec[s])
    assert got["join"] is True


def _sweep():
    rng = random.Random(20261020)
    out = []
    for i in range(3000):
        n = rng.randint(1, 8)
        mcap, dcap = rng.choice([1, 50, 1000, 4096, 1 << 20]), rng.choice([1, 300, 5000, 65536, 1 << 22])
        runs = [rng.choice([0, 1, mcap, mcap // 2, mcap // 3 + 1]) if rng.random() < 0.4 else rng.randint(0, max(1, mcap)) for _ in range(n)]
        dec = [rng.choice([0, 1, 63, 64, 65, dcap, dcap // 2]) if rng.random() < 0.4 else rng.randint(0, max(1, dcap)) for _ in range(n)]
        if i % 9 == 0:                                            # a sub-block alone above a capacity
            s = rng.randrange(n)
            if rng.random() < 0.5:
                runs[s] = mcap + rng.randint(1, 3)
            else:
                dec[s] = dcap + rng.randint(1, 3)
        dec = [min(d, 20000) for d in dec] if i % 9 else dec      # (the probe lays the joined streams out: keep them small)
        out.append(_scenario(runs, dec, mcap, dcap, packed=i & 1, void_seg=rng.choice([-1, 0, 1, 2])))
    return out


def _judge(scenarios, results):
    for sc, got in zip(scenarios, results):
        rc, seg_of = _restated(sc)
        assert got["rc"] == rc, sc
        if rc < 0:
            assert got["seg_of"] == UNTOUCHED, "nothing is written on an error"
            if rc == NOT_SUPPORTED:
                assert _fewest_by_brute_force(sc) is None
            continue
        assert got["seg_of"][:sc["nsub"]] == seg_of and got["seg_of"][sc["nsub"]:] == UNTOUCHED[sc["nsub"]:], sc
        assert rc == _fewest_by_brute_force(sc), ("greedy is the fewest", sc)
        for i in range(rc):
            members = [s for s in range(sc["nsub"]) if seg_of[s] == i]
            assert members == list(range(members[0], members[-1] + 1))
            assert sum(sc["runs"][s] for s in members) <= sc["mcap"] and sum(sc["dec"][s] for s in members) <= sc["dcap"]
        _check_schedule(sc, got)


def test_sweep_against_restatement_and_brute_force(probe):
    scenarios = _sweep()
    results = probe(scenarios)
    assert sum(r["rc"] == NOT_SUPPORTED for r in results) > 100 and sum(r["rc"] > 1 for r in results) > 500
    _judge(scenarios, results)


def test_edges(probe):
    cases = [
        (_scenario([10], [40], 10, 40), 1, [0]),                                          # one sub-block, exactly at both capacities
        (_scenario([5, 5], [20, 20], 10, 40), 1, [0, 0]),                                 # two, together exactly at capacity
        (_scenario([5, 6], [20, 20], 10, 40), 2, [0, 1]),                                 # one run over
        (_scenario([5, 5], [20, 21], 10, 40), 2, [0, 1]),                                 # one decision over
        (_scenario([4, 4, 4, 4, 4, 4, 4, 4], [9] * 8, 12, 1000), 3, [0, 0, 0, 1, 1, 1, 2, 2]),     # several, then a shorter one
        (_scenario([11, 1], [1, 1], 10, 40), NOT_SUPPORTED, None),                        # a sub-block alone too large: runs
        (_scenario([1, 1], [1, 41], 10, 40), NOT_SUPPORTED, None),                        # ... decisions
        (_scenario([0, 0], [0, 0], 10, 40), 1, [0, 0]),                                   # empty sub-blocks join
    ]
    results = probe([c[0] for c in cases])
    for (sc, rc, seg_of), got in zip(cases, results):
        assert got["rc"] == rc, sc
        assert got["seg_of"] == (UNTOUCHED if seg_of is None else seg_of + UNTOUCHED[len(seg_of):]), sc
    _judge([c[0] for c in cases], results)


def test_bad_arguments(probe):
    ok = dict(runs=[1, 2], dec=[3, 4], mcap=10, dcap=40)
    bad = [_scenario(**ok, nullmask=1), _scenario(**ok, nullmask=2), _scenario(**ok, nullmask=4), _scenario(**ok, nsub=0),
           _scenario(**{**ok, "runs": [1] * 9, "dec": [1] * 9}), _scenario(**{**ok, "mcap": 0}), _scenario(**{**ok, "dcap": 0}),
           _scenario(**{**ok, "mcap": -5})]
    for sc, got in zip(bad, probe(bad)):
        assert got["rc"] == BAD_PARAMETER and got["seg_of"] == UNTOUCHED, sc


def test_joining_against_the_packed_layout(probe):
    """poff / pbase of the schedule are those of bscgpu_pstream_pack13_host for the same sub-blocks, in both forms, whatever the cuts —
    and the probe's own join (every segment laid out alone, copied by src / dst / len, one of them packed by the host) gives that stream"""
    dec = [700, 64, 1, 129, 0, 4000, 63, 65]
    runs = [100, 30, 1, 60, 0, 900, 20, 20]
    packed_bytes, pbase = _pack13_layout(dec)
    for mcap, dcap in [(10000, 1 << 20), (1000, 4100), (900, 4000), (1030, 4764)]:
        for packed in (0, 1):
            for void_seg in (-1, 0, 1):
                sc = _scenario(runs, dec, mcap, dcap, packed=packed, void_seg=void_seg)
                got, = probe([sc])
                assert got["rc"] == _restated(sc)[0] >= 1
                assert got["pbase"] == [int(x) for x in pbase] and got["join"] is True
                if packed:
                    assert got["zone"] == len(packed_bytes)
                _check_schedule(sc, got)


def test_exported_plan_is_the_headers():
    """bscgpu_block_segment_plan (the library's export, libbsc_amd.gpu.block_segment_plan) gives what the probe's header gives"""
    from libbsc_amd.gpu import GpuError, block_segment_plan
    for sc in _sweep()[:400]:
        rc, seg_of = _restated(sc)
        if rc < 0:
            with pytest.raises(GpuError) as e:
                block_segment_plan(sc["runs"], sc["dec"], sc["mcap"], sc["dcap"])
            assert e.value.code == rc
        else:
            assert block_segment_plan(sc["runs"], sc["dec"], sc["mcap"], sc["dcap"]) == (rc, seg_of)


# ---- a block modelled in one go --------------------------------------------------------------------------------------------------------
def _whole_sweep():
    rng = random.Random(20261021)
    special = [0, 1, 7, 8, 63, 64, 65]
    out = [(n, packed, [d] * n) for n in range(1, 9) for packed in (0, 1) for d in special]
    for i in range(600):
        n = rng.randint(1, 8)
        out.append((n, i & 1, [rng.choice(special) if rng.random() < 0.5 else rng.randint(0, 50000) for _ in range(n)]))
    return out


def _gpu_stage_had(dec, packed):
    """the layout of a whole block's stream as gpu_stage wrote it out by hand before DcBlockSchedule::whole:
    -> poff, pbase (the packed form's; it left zeros otherwise, which nothing read), piece_lo, piece_hi, zone_entries"""
    poff = [0]
    for d in dec:
        poff.append(poff[-1] + d)
    ndec = poff[-1]
    piece_lo, piece_hi, pbase, pb13 = [], [], [], 0
    zone_entries = ndec + 64
    for b in range(len(dec)):
        cnt = poff[b + 1] - poff[b]
        pbase.append(pb13)
        if packed:
            piece_lo.append(pb13 // 8 * 13)
            piece_hi.append(piece_lo[b] + (cnt + 7) // 8 * 13)
            pb13 += (cnt + 63) // 64 * 64
        else:
            piece_lo.append(poff[b] * 2)
            piece_hi.append(poff[b + 1] * 2)
    pbase.append(pb13)
    if packed:
        zone_entries = (pb13 // 8 * 13 + 1) // 2 + 64
    return poff, pbase, piece_lo, piece_hi, zone_entries


def _judge_whole(cases, results):
    for (n, packed, dec), got in zip(cases, results):
        poff, pbase, lo, hi, zone_entries = _gpu_stage_had(dec, packed)
        assert got["segments"] == 1 == len(got["segs"]) and got["decisions"] == poff[-1], (n, packed, dec)
        g = got["segs"][0]
        assert (g["s0"], g["s1"], g["expect"]) == (0, n, poff[-1])
        assert g["src"] == g["dst"] == lo and g["len"] == [h - l for l, h in zip(lo, hi)], (n, packed, dec)
        assert got["poff"] == poff
        assert (got["zone"] + 1) // 2 + 64 == zone_entries and got["zone"] == (pbase[-1] // 8 * 13 if packed else 2 * poff[-1])
        if packed:
            assert got["pbase"] == pbase, (n, dec)
        else:
            assert got["pbase"] == _gpu_stage_had(dec, 1)[1], "the packed space's, whichever form the block is in"


def _whole_line(case):
    n, packed, dec = case
    return " ".join(str(x) for x in ["whole", n, packed] + dec)


def test_whole_block_schedule(probe):
    cases = _whole_sweep()
    _judge_whole(cases, probe([_whole_line(c) for c in cases]))
    for n, packed, dec in cases[::40]:
        if packed:
            packed_bytes, pbase = _pack13_layout(dec)
            got, = probe([_whole_line((n, packed, dec))])
            assert got["pbase"] == [int(x) for x in pbase] and got["zone"] == len(packed_bytes)
    for bad in ("whole 0 0", "whole 9 1 1 1 1 1 1 1 1 1 1"):
        assert probe([bad])[0]["segments"] == BAD_PARAMETER


# ---- max_rank ----------------------------------------------------------------------------------------------------------------------------
MAX_RANK_LINES = ["maxrank 8 1 2 3 4 5 33 255 256", "maxrank 3 17 16 0", "maxrank 0"]


def _judge_max_rank(lines, results):
    for line, got in zip(lines, results):
        nsym = [int(x) for x in line.split()[2:]]
        assert got["max_rank"] == [max(0, (k - 1).bit_length() - 1) for k in range(1, 257)]
        assert got["table"] == [max(0, (k - 1).bit_length() - 1) for k in nsym] + UNTOUCHED[len(nsym):]


def test_max_rank(probe):
    _judge_max_rank(MAX_RANK_LINES, probe(MAX_RANK_LINES))


# ---- what the driver of one block decides ----------------------------------------------------------------------------------------------
SENT, DEVICE_RC, LANDED, HOST_MODEL, ERROR = range(5)


def _decision_lines():
    tries = [f"tries {a} {e} {st} {fa} {nsub} {n} {min_n}" for a, e, st, fa in itertools.product((0, 1), repeat=4) for nsub in (0, 1, 2, 8)
             for n, min_n in ((1 << 20, 1 << 20), ((1 << 20) - 1, 1 << 20), (5, 0), (2147483647, 1 << 20))]
    dense = [f"dense {m} {n}" for n in (10, 7, 1 << 20, 1000003, 2147483647, 3) for m in
             sorted({0, n, *(max(0, int(0.70 * n) + d) for d in (-2, -1, 0, 1, 2))})]
    verdict = [f"verdict {code} {s} {rc} {z}" for code in (0, -4, -1, -2, -3, -5, -9, -10, 1) for s, rc, z in itertools.product((0, 1), repeat=3)]
    return tries + dense + verdict


def _decided_before(line):
    """the conditions of gpu_stage that the three functions replace"""
    kind, *v = line.split()
    v = [int(x) for x in v]
    if kind == "tries":
        allow_devcoder, enabled, coder_static, coder_fast_and_enabled, nblocks, n, min_n = v
        return {"tries": int(bool(allow_devcoder and enabled and (coder_static or coder_fast_and_enabled) and nblocks > 1 and n >= min_n))}
    if kind == "dense":
        m, n = v
        return {"dense": int(not float(m) <= 0.70 * float(n))}
    r2, sent, device_rc, zone_had = v
    whole = r2 == 0 and not sent
    if r2 == 0 and sent:
        return {"verdict": SENT}
    if whole and device_rc:
        return {"verdict": DEVICE_RC}
    if whole and zone_had:
        return {"verdict": LANDED}
    if r2 != NOT_SUPPORTED and r2 != 0:
        return {"verdict": ERROR}
    return {"verdict": HOST_MODEL}


def test_decisions_of_one_block(probe):
    lines = _decision_lines()
    results = probe(lines)
    assert results == [_decided_before(l) for l in lines]
    verdicts = [r["verdict"] for r in results if "verdict" in r]
    assert set(verdicts) == {SENT, DEVICE_RC, LANDED, HOST_MODEL, ERROR}, "every result is reached, every combination has exactly one"
    assert {r["dense"] for r in results if "dense" in r} == {0, 1} and {r["tries"] for r in results if "tries" in r} == {0, 1}


def test_sanitizer_build_runs_clean(tmp_path_factory):
    """the probe as a stand-alone program under AddressSanitizer and UBSan, on the sweeps and the edges: same answers, nothing reported"""
    exe = _build(tmp_path_factory, "block_plan_probe_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])
    scenarios = _sweep() + [_scenario([1, 2], [3, 4], 10, 40, nullmask=7), _scenario([1] * 9, [1] * 9, 10, 40), _scenario([1], [1], 10, 40, nsub=0)]
    whole, decisions = _whole_sweep(), _decision_lines()
    env = {k: v for k, v in os.environ.items() if k != "LD_PRELOAD"}
    results, stderr = _ask(exe, scenarios + [_whole_line(c) for c in whole] + MAX_RANK_LINES + decisions, env=env)
    assert "ERROR" not in stderr and "runtime error" not in stderr, stderr[-2000:]
    _judge(scenarios, results[:len(scenarios)])
    rest = results[len(scenarios):]
    _judge_whole(whole, rest[:len(whole)])
    _judge_max_rank(MAX_RANK_LINES, rest[len(whole):len(whole) + len(MAX_RANK_LINES)])
    assert rest[len(whole) + len(MAX_RANK_LINES):] == [_decided_before(l) for l in decisions]
