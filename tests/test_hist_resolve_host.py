"""The exact resolve of open run_hist brackets (BSCGPU_OPT_DC_HIST_EXACT) judged on the CPU: the bounds it rests on, and the host
restatement of its kernels (devcoder_model.h: hist_resolve_host, driven through tools/hist_resolve_probe.cpp) against the plain serial
walk of run_hist_next — every run's min(run_hist, 7).  Every case must leave brackets open: one that does not tests nothing.  The
block inputs are also pinned to the path they take today by the paths probe, so the GPU tests (test_gpu_hist_resolve.py), which hold
the device to the same counts, cannot pass for the wrong reason."""
import numpy as np
import pytest

import devcoder_inputs as di
import hist_resolve_inputs as hr


@pytest.fixture(scope="module")
def tools(tmp_path_factory):
    d = tmp_path_factory.mktemp("hist_resolve_probe")
    return hr.build_probe(d), di.build_probe(d), d


def _check(v, name):
    print(name, v)
    assert v["ext"] > 0, f"{name}: no open bracket, the case tests nothing"
    assert v["values_equal"], f"{name}: {v['values_differ']} values differ from the serial walk, first at element {v['first_differ']}"
    assert v["resolved"] == v["ext"], name
    assert 0 < v["chunks"] <= (v["runs"] + hr.CH - 1) // hr.CH


def test_bound(tools):
    """h' = (h + inc) >> 2: monotone, the width behind one step at most floor((d + 3) / 4) — 63 -> 16 -> 4 -> 1 —, [0, 63] invariant for
    every increment a run can give, and exactly the fixed points b and b + 1 for the classes 1 .. 6; every other class has one clamped value"""
    b = hr.probe_bound(tools[0])
    print(b)
    assert b["monotone"] and b["contracts_by_four"] and b["invariant_0_63"] and b["inc_is_next"]
    assert b["widths"] == [63, 16, 4, 1] and b["max_inc"] == 93 and b["max_image"] <= 63
    assert b["two_fixed_points_classes_1_to_6"] and b["other_classes_one_clamped_value"]
    assert b["fixed_points"][0] == [0] and b["fixed_points"][1] == [1, 2] and b["fixed_points"][6] == [6, 7]
    assert b["DC_HIST_NP"] == 9 and b["DC_HIST_NP"] >= 3, "behind three predecessors a bracket holds at most two neighbouring values"
    assert b["DC_HIST_CH"] == hr.CH and b["DC_HIST_CAND"] == 64 and b["DC_HIST_GROUP"] == hr.GROUP


@pytest.mark.parametrize("name", hr.HIST_EXT_GENERATORS + hr.FAIL_HIST_GENERATORS)
def test_generators_tagged_hist(tools, name):
    """every hist_ext and fail_hist generator: the path it takes today (the paths probe), the same count of open runs, every value exact"""
    exe, pexe, d = tools
    L = di.GENERATORS[name][2]()
    p = di.run_probe(pexe, L, d)
    di.check_tag(name, p)
    if name in hr.FAIL_HIST_GENERATORS:
        assert p["fail_mask"] == di.FAIL_HIST and p["hist_fail"] > 0
    v = hr.probe_block(exe, d, L)
    _check(v, name)
    assert v["ext"] == p["hist_ext"] and v["runs"] == p["runs"] and v["nb"] == p["nb"], "the bracket's count: the paths probe's"


def test_two_sub_blocks(tools):
    exe, pexe, d = tools
    L = di.GENERATORS["hist_two_sub_blocks_fail"][2]()
    p, v = di.run_probe(pexe, L, d), hr.probe_block(exe, d, L)
    _check(v, "hist_two_sub_blocks_fail")
    assert p["nb"] == v["nb"] == 2 and min(p["sub_runs"]) > 2 * 9216, "both sub-blocks hold a chain longer than today's look-back"


@pytest.mark.parametrize("period", [12, 50, 200, 1000, 5000])
def test_mixed_classes_close_on_the_data(tools, period):
    exe, pexe, d = tools
    L = di.hist_mixed(period)
    v = hr.probe_block(exe, d, L)
    _check(v, f"hist_mixed({period})")
    assert v["ext"] == di.run_probe(pexe, L, d)["hist_ext"]


@pytest.mark.parametrize("seed,m", hr.PLANTED_CASES)
def test_random_lengths_with_planted_stretches(tools, seed, m):
    chain, run = hr.planted(seed, m)
    _check(hr.probe_runs(tools[0], tools[2], chain, run), f"planted({seed}, {m})")


def test_stretch_across_a_chunk_border(tools):
    """a chain of 300 same-class runs from element 900 to 1199: it begins in chunk 0 and ends in chunk 1"""
    chain, run = hr.chains([900, 300, 848], fill=1)
    run[900:1200] = 5
    v = _probe(tools, chain, run, "stretch 900 .. 1199")
    assert v["chunks"] == 2 and v["ext"] == 300 - 9


def _probe(tools, chain, run, name):
    v = hr.probe_runs(tools[0], tools[2], chain, run)
    _check(v, name)
    return v


@pytest.mark.parametrize("at", [hr.CH, 2 * hr.CH - 1, 2 * hr.CH, 3 * hr.CH - 1])
def test_chain_start_on_the_first_and_on_the_last_element_of_a_chunk(tools, at):
    """two open chains, the second starting at element `at`: the first element of a chunk, or the last"""
    chain, run = hr.chains([at, 4 * hr.CH + 7 - at], fill=3)
    v = _probe(tools, chain, run, f"chain start at {at}")
    assert v["ext"] == 4 * hr.CH + 7 - 2 * 9 and v["chunks"] == 5


def test_more_than_64_chunks_in_one_chain(tools):
    chain, run = hr.chains([5, 100 * hr.CH + 300, 77], fill=100)
    v = _probe(tools, chain, run, "100 chunks in one chain")
    assert v["groups"] == 2 and v["chain_steps"] == 2 * hr.GROUP + 1 and v["chunks"] == 101


def test_more_than_64_groups_in_one_launch(tools):
    """one chain through 66 groups: the groups kernel takes a second round of 64"""
    m = 65 * hr.GROUP * hr.CH + 5000
    chain, run = hr.chains([m], fill=2)
    v = _probe(tools, chain, run, "66 groups")
    assert v["groups"] == 66 and v["chain_steps"] == 2 * hr.GROUP + 65 and v["ext"] == m - 9


def test_hist_chain_blocks_of_the_gpu_tests(tools):
    """hist_chain(140 000): more than 64 chunks in each chain"""
    exe, pexe, d = tools
    L = di.hist_chain(140_000)
    p, v = di.run_probe(pexe, L, d), hr.probe_block(exe, d, L)
    _check(v, "hist_chain(140000)")
    assert p["fail_mask"] == di.FAIL_HIST and v["ext"] == p["hist_ext"]
    assert p["nb"] == 2 and min(p["sub_runs"]) // 2 > hr.GROUP * hr.CH, "every other run of a sub-block belongs to the open chain"
    assert v["groups"] > 2 and v["chain_steps"] > 2 * hr.GROUP
