"""The exact resolve of open avg_rank flags (BSCGPU_OPT_DC_AVG_EXACT) judged on the CPU: the bound it rests on, and the host restatement
of its kernels (devcoder_model.h: avg_resolve_host, driven through tools/avg_resolve_probe.cpp) against the plain serial walk of
avg_rank_next — every flag, and every chunk's exact start inside the chunk's start bracket.  Every case must leave flags open: one
that does not tests nothing.  The GPU tests (test_gpu_avg_resolve.py) then hold the device to the same counts."""
import numpy as np
import pytest

import avg_resolve_inputs as ar
import devcoder_inputs as di


@pytest.fixture(scope="module")
def tools(tmp_path_factory):
    d = tmp_path_factory.mktemp("avg_resolve_probe")
    return ar.build_probe(d), di.build_probe(d), d


def _check(v, name):
    print(name, v)
    assert v["und"] > 0, f"{name}: no open flag, the case tests nothing"
    assert v["flags_equal"], f"{name}: {v['flags_differ']} flags differ from the serial walk, first at run {v['first_differ']}"
    assert v["resolved"] == v["und"] and v["left"] == 0 and v["sub_left"] == 0, name
    assert v["domain_ok"], f"{name}: an exact start outside its lane's [lo0, hi0], or not the serial walk's value"
    assert v["max_width"] < 33


def test_bound(tools):
    """d' <= floor(124 d / 128) + 1 from 255: at most 32 after DC_AVG_WARM steps (after 128 already), so at most 33 candidates; every
    constant rank leaves at most 31; one wavefront of candidates covers that with room"""
    b = ar.probe_bound(tools[0])
    assert b["DC_AVG_WARM"] >= 128 and b["recursion_width"] <= 32 and b["recursion_width_128"] <= 32
    assert b["constant_rank_width"] <= 31
    assert b["DC_AVG_CAND"] > 33 and b["DC_AVG_CAND"] == 64 and b["DC_AVG_GROUP"] == 64
    assert b["DC_AVG_CH"] == 1024 and b["DC_AVG_WARM"] == 768


@pytest.mark.parametrize("name", ar.FAIL_AVG_GENERATORS)
def test_generators_tagged_fail_avg(tools, name):
    exe, pexe, d = tools
    tag, _, build = di.GENERATORS[name]
    assert tag == "fail_avg"
    L = build()
    v = ar.probe_block(exe, d, L)
    _check(v, name)
    assert v["launched"] and v["und"] == di.run_probe(pexe, L, d)["avg_und"], "the bracket's count: the paths probe's"


@pytest.mark.parametrize("seed,m", ar.STRETCH_CASES)
def test_alternating_stretches(tools, seed, m):
    rank, first = ar.stretches(seed, m)
    _check(ar.probe_ranks(tools[0], tools[2], rank, first), f"stretches({seed}, {m}) sub-blocks at {first}")


@pytest.mark.parametrize("seed,m", ar.WALK_CASES)
def test_random_walk(tools, seed, m):
    rank, first = ar.random_walk(seed, m)
    _check(ar.probe_ranks(tools[0], tools[2], rank, first), f"random_walk({seed}, {m}) sub-blocks at {first}")


def test_table_form_top(tools):
    """the bracket's upper end of a table: 2^(max_rank + 1) - 1 = 127 for ranks up to 60"""
    rank, first = ar.stretches(1, 9000)
    _check(ar.probe_ranks(tools[0], tools[2], rank, first, top=127), "stretches(1, 9000), top 127")


@pytest.mark.parametrize("runs,sub_runs", [(ar.LONG_RUNS, None), (ar.LONG_RUNS_TWO, ar.LONG_TWO_SUB_RUNS)])
def test_long_open_stretch_chains_more_than_one_group(tools, runs, sub_runs):
    exe, pexe, d = tools
    L = di.const_rank(40, runs)
    v = ar.probe_block(exe, d, L)
    _check(v, f"const_rank(40, {runs})")
    assert v["chunks"] > 2 * 64 and v["chain_steps"] > 2 * 64, "groups are chained"
    if sub_runs:
        assert di.run_probe(pexe, L, d)["sub_runs"] == sub_runs and sub_runs[0] % 1024 not in (0, 1023)


def test_block_with_ranks_is_a_block_of_kind_b(tools):
    """the sorted block the GPU test gives the stage: one sub-block of 20 000 runs whose flags stay open throughout"""
    L = ar.stretches_block()
    v = ar.probe_block(tools[0], tools[2], L)
    _check(v, "stretches_block()")
    assert v["und"] > 10_000 and v["chunks"] == 20


def test_realistic_block_has_a_handful_of_open_flags(tools, ref):
    """text followed by float32 noise, >= 1 MiB, two sub-blocks, <= 0.70 runs per byte: today's device model declines it for a handful of
    runs out of 670 000 (the paths probe: fail_mask == FAIL_AVG alone), and the resolve settles every one of them"""
    exe, pexe, d = tools
    T = ar.realistic_text()
    L, _, _ = ref.bwt_encode(T)
    p = di.run_probe(pexe, L, d)
    assert T.size >= 1 << 20 and p["nb"] >= 2 and p["runs"] <= 0.70 * T.size
    assert p["fail_mask"] == di.FAIL_AVG and 0 < p["avg_und"] <= 8, p["avg_und"]
    v = ar.probe_block(exe, d, L)
    _check(v, "realistic block")
    assert v["und"] == p["avg_und"]
