"""The exact resolve of open chunk starts (BSCGPU_OPT_DC_REPLAY_EXACT) judged on the CPU: the bound its candidate cap rests on, and the
host restatement of its kernels (devcoder_model.h: replay_resolve_host, driven through tools/replay_resolve_probe.cpp) against the
plain serial walk of every chain — the start value of every chunk, with the resolve and without.  Every case must leave chunks open:
one that does not tests nothing.  The GPU tests (test_gpu_replay_resolve.py) then hold the device to the same counts."""
import numpy as np
import pytest

import devcoder_inputs as di
import replay_resolve_inputs as ri


@pytest.fixture(scope="module")
def tools(tmp_path_factory):
    d = tmp_path_factory.mktemp("replay_resolve_probe")
    return ri.build_probe(d), d


def _check(v, name, fail_off=None):
    print(name, {k: v[k] for k in ("ev", "chunks", "stretches", "longest", "max_width")}, "off", v["off"], "on", v["on"])
    on, off = v["on"], v["off"]
    assert on["open"] == off["open"] > 0, f"{name}: no open chunk, the case tests nothing"
    assert off["starts_equal"] and on["starts_equal"], f"{name}: a chunk's start differs from the serial walk's"
    assert off["resolved"] == 0 and off["replays"] > 0
    assert on["resolved"] == on["open"] and on["replays"] == 0 and not on["fail_replay"] and on["wide"] == 0, name
    assert v["max_width"] <= v["DC_RP_CAND"]
    if fail_off is not None:
        assert off["fail_replay"] == fail_off, name
    assert off["fail_replay"] == (v["longest"] > v["DC_REPLAY_MAX"]), "a chunk more than DC_REPLAY_MAX behind the stretch's head"


def test_bound(tools):
    """Both update maps contract a bracket of width d by at least floor(d a / 4096) per step (exhaustively, every pair of attainable
    values and both bits), so DC_EV >= 4096 steps leave at most ceil(4096 / a) values: 373 for the static coder's slowest rate, 11,
    and 128 for the fast coder's, 32.  Rounded up to whole wavefronts that is the cap.  Periodic patterns really leave brackets of more
    than one wavefront of values in the static coder's state family, and never more than the bound."""
    b = ri.probe_bound(tools[0])
    print(b)
    s, f = b["static"], b["fast"]
    assert s["contraction_holds"] and f["contraction_holds"]
    assert (s["slowest_rate"], s["bound_width"]) == (11, 373) and (f["slowest_rate"], f["bound_width"]) == (32, 128)
    assert s["bound_width"] == -(-4096 // 11) and f["bound_width"] == 4096 // 32
    assert b["cap"] == b["DC_RP_CAND"] == ri.DC_RP_CAND == 384 and b["cap"] % 64 == 0 and b["cap"] - 64 < s["bound_width"]
    assert b["DC_EV"] == ri.DC_EV >= 4096
    assert 64 < s["periodic_width"] <= s["bound_width"] and f["periodic_width"] <= 64
    for c in range(8):
        for fam in range(3):
            assert s["periodic_by_class"][c][fam] <= s["bound_by_class"][c][fam] and f["periodic_by_class"][c][fam] <= f["bound_by_class"][c][fam]


@pytest.mark.parametrize("name", ri.KEPT + ri.FAIL)
def test_generators(tools, name):
    """the event sequences of every replay_kept and fail_replay generator and of the second table's fail_replay block, laid out
    chain-major as the device lays them out"""
    _check(ri.probe_block(tools[0], tools[1], ri.block_of(name), key=name), name, fail_off=name in ri.FAIL)


def test_generators_hold_brackets_wider_than_a_wavefront(tools):
    """a lane holds several candidates: at least one input has a start bracket of more than 64 values (two per lane) and one of more
    than 128 (four per lane); none exceeds the cap"""
    w = {name: ri.probe_block(tools[0], tools[1], ri.block_of(name), key=name)["max_width"] for name in ri.KEPT + ri.FAIL}
    print(w)
    assert any(64 < x <= 128 for x in w.values()) and any(128 < x <= 256 for x in w.values())
    assert max(w.values()) <= ri.DC_RP_CAND
    assert w[ri.GUARD_KEPT[0]] > ri.GUARD_KEPT[1] and w[ri.GUARD_FAIL[0]] > ri.GUARD_FAIL[1], "the guard cases' caps are below their inputs' widths"


def test_block_under_one_mib_that_declines(tools, tmp_path):
    """the batched pass's fail_replay block: two sub-blocks, the second holds nearly all runs; the paths probe agrees on the exit"""
    L = ri.skewed_fail_replay_block()
    v = ri.probe_block(tools[0], tools[1], L, key="skewed")
    _check(v, "skewed_fail_replay_block", fail_off=True)
    p = di.run_probe(di.build_probe(tmp_path), L, tmp_path)
    assert L.size < 1 << 20 and p["nb"] == 2 and p["fail_mask"] == di.FAIL_REPLAY and p["sub_runs"][1] > 100 * p["sub_runs"][0]


@pytest.mark.parametrize("ev", ri.EVS)
@pytest.mark.parametrize("name", list(ri.EDGE_CASES))
def test_stretch_edges(tools, name, ev):
    build, n_open, n_stretches = ri.EDGE_CASES[name]
    v = ri.probe_events(tools[0], tools[1], build(ev), ev)
    _check(v, f"{name} ev {ev}")
    assert v["ev"] == ev and (v["on"]["open"], v["stretches"]) == (n_open, n_stretches), name


@pytest.mark.parametrize("ev", ri.EVS)
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_random_bits_with_planted_stretches(tools, seed, ev):
    """three families at once: random bits close a bracket within a few hundred events, the planted alternations keep it open across
    chunk boundaries wherever they happen to lie; several chains per row, rows of three classes"""
    n = 30 * ev + 1000 * seed + 17
    R = lambda sd, k, sig=0: ri.random_with_stretches(sd, k, sig, stretch=7 * ev // 2)
    jobs = [(ri.FAM_STATIC, [(ri.TAU_RF, np.concatenate([R(seed, n), R(seed + 10, n // 2, 3 << 8)]))]),
            (ri.FAM_CHAR, [(ri.TAU_RF, R(seed + 20, n, 65)), (ri.TAU_NF, R(seed + 30, n, 65 | (1 << 8)))]),
            (ri.FAM_STATE, [(ri.TAU_RE + 2, R(seed + 40, n, 9)), (ri.TAU_RM + 5, ri.pattern(5 * ev, [0, 1, 1, 0, 1], sig=200))])]
    v = ri.probe_events(tools[0], tools[1], jobs, ev)
    _check(v, f"random seed {seed} ev {ev}")
    assert v["stretches"] >= 3 and v["max_width"] > 64, "the planted stretches of at least two families and the state family's pattern"


@pytest.mark.parametrize("ev", ri.EVS)
def test_fast_coder_rates(tools, ev):
    """the fast coder's one family with its shift updates: the RF chain under alternating bits (fast_batch_inputs: the bracket stays open)"""
    v = ri.probe_events(tools[0], tools[1], [(ri.FAM_CHAR, [(ri.TAU_RF, ri.alternating(200, sig=1))]), (ri.FAM_CHAR, [(ri.TAU_RF, ri.alternating(6 * ev + 100, sig=66))])], ev, coder=1)
    _check(v, f"fast ev {ev}")
    assert v["on"]["open"] == 5 and v["max_width"] <= 128


def test_guard(tools):
    """a cap below an input's widest start bracket: the chunk behind that bracket is not walked, it and what follows it in its stretch
    are replayed serially as today (same start values), or the unit is declined as today"""
    name, cand = ri.GUARD_KEPT
    v = ri.probe_block(tools[0], tools[1], di.GENERATORS[name][2](), cand=cand, key=name)
    print(name, cand, v["max_width"], v["on"])
    on = v["on"]
    assert v["max_width"] > cand and on["wide"] > 0 and on["starts_equal"] and not on["fail_replay"]
    assert 0 < on["resolved"] < on["open"] and 0 < on["replays"] < v["off"]["replays"]
    name, cand = ri.GUARD_FAIL
    v = ri.probe_block(tools[0], tools[1], di.GENERATORS[name][2](), cand=cand, key=name)
    print(name, cand, v["max_width"], v["on"])
    on = v["on"]
    assert v["max_width"] > cand and on["wide"] > 0 and on["fail_replay"] and on["starts_equal"] and on["resolved"] < on["open"]


def test_paths_probe_says_what_the_resolve_changes(tmp_path):
    """tools/devcoder_paths_probe.cpp with the resolve on: a fail_replay input is no longer declined, every other verdict stays"""
    exe = di.build_probe(tmp_path)
    L = di.GENERATORS["alt_rf_static_2x73_chunks"][2]()
    off = di.run_probe(exe, L, tmp_path)
    path = tmp_path / "probe_input.bin"
    import json
    import subprocess
    r = subprocess.run([exe, str(path), "replay_exact"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    on = json.loads(r.stdout)
    assert off["fail_mask"] == di.FAIL_REPLAY and "replay_exact" not in off
    assert on["fail_mask"] == 0 and on["replay_exact"] and on["no_fail_replay_certain"] and on["no_replay_certain"]
    assert {k: v for k, v in on.items() if k not in ("fail_mask", "replay_exact", "replay_certain", "no_replay_certain", "no_fail_replay_certain")} == \
           {k: v for k, v in off.items() if k not in ("fail_mask", "replay_certain", "no_replay_certain", "no_fail_replay_certain")}
