"""The CPU judge of "which path must this input take" for the device coder's rare exits (no GPU needed).

tools/devcoder_paths_probe.cpp walks a sorted block with the host coder's own decision walker and devcoder_model.h's formulas and
constants, and says which of the device coder's exits the block MUST take whatever the chain-major layout: undecided avg_rank flags,
run_hist brackets that enter the extended look-back (and where they close or fail), counter chains whose brackets stay open over
several evaluation chunks.  Every generator of tests/devcoder_inputs.py is tagged with the path it targets; here the probe has to
confirm every tag, so that the GPU tests (test_gpu_devcoder_paths.py) can never pass on an input that quietly missed its path."""
import numpy as np
import pytest

import devcoder_inputs as di


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    d = tmp_path_factory.mktemp("paths_probe")
    exe = di.build_probe(d)
    return lambda L: di.run_probe(exe, L, d)


def test_thresholds_follow_from_the_constants(probe):
    """replay / FAIL_REPLAY thresholds are derived from DC_EV and DC_REPLAY_MAX, not written down twice"""
    v = probe(np.arange(4000, dtype=np.uint8))
    c = v["constants"]
    assert v["ev"] == c["DC_EV"]                                    # a small block: the minimum chunk
    assert v["replay_min"] == 3 * v["ev"] and v["fail_min"] == (c["DC_REPLAY_MAX"] + 2) * v["ev"] and v["keep_max"] == c["DC_REPLAY_MAX"] * v["ev"]
    assert c["DC_AVG_WARM"] < c["DC_AVG_CH"]


def test_every_target_path_has_a_generator():
    tags = {t for t, _, _ in di.GENERATORS.values()}
    assert tags == {"avg_off", "avg_decides", "fail_avg", "hist_ext", "fail_hist", "replay_kept", "fail_replay"}
    # every widening step of the run_hist look-back closes somewhere, on the chain's start and on the data
    steps = sorted(e["step"] for t, e, _ in di.GENERATORS.values() if t == "hist_ext")
    assert set(steps) == {0, 1, 2, 3, 4}
    # replays in all three families
    assert {e["fam"] for t, e, _ in di.GENERATORS.values() if t == "replay_kept"} == set(di.FAMILIES)
    assert {e["fam"] for t, e, _ in di.GENERATORS.values() if t == "fail_replay"} == set(di.FAMILIES)


@pytest.mark.parametrize("name", list(di.GENERATORS))
def test_generator_takes_its_tagged_path(probe, name):
    L = di.GENERATORS[name][2]()
    assert L.dtype == np.uint8 and 0 < L.size <= 8 << 20
    di.check_tag(name, probe(L))


def test_generators_are_deterministic():
    for name in ("rank40_warm_1792", "alt_rm_state", "hist_mixed_p50"):
        assert np.array_equal(di.GENERATORS[name][2](), di.GENERATORS[name][2]())


def test_run_hist_look_back_counts_follow_the_chain_length(probe):
    """One symbol with q runs of one length class: the run with P predecessors enters the extended look-back iff P >= DC_HIST_NP and
    closes at the first widening K > P; none left at K = 9216 -> the probe's counts are those of the arithmetic."""
    v = probe(di.hist_chain(9217))
    assert v["hist_ext"] == 9217 - 9 and v["hist_closed"] == [36 - 9, 144 - 36, 576 - 144, 2304 - 576, 9216 - 2304] and v["hist_fail"] == 1


def test_avg_rank_bracket_ends_under_a_constant_rank(probe):
    """avg' = avg + floor((rank - avg) / 32): under a constant rank r the lower end settles at r - 31, the upper at r; they stay on
    opposite sides of 32 exactly for r in 32..62"""
    from_below = lambda r: [x := 0] and [x := (x * 124 + 4 * r) >> 7 for _ in range(2000)][-1]
    from_above = lambda r: [x := 255] and [x := (x * 124 + 4 * r) >> 7 for _ in range(2000)][-1]
    for r in range(32, 100):
        assert from_below(r) == r - 31 and from_above(r) == r
    und = {r: (from_below(r) >= 32) != (from_above(r) >= 32) for r in range(1, 100)}
    assert [r for r in und if und[r]] == list(range(32, 63))


@pytest.mark.parametrize("name", list(di.WHOLE_BLOCKS))
def test_whole_block_text_has_a_bwt_that_takes_the_path(probe, ref, name):
    """The texts of the whole-block GPU tests: the reference's BWT of the text must take the tagged path, and be a block bsc_compress
    gives to the device model at all (>= 1 MiB, several sub-blocks, at most 0.70 runs per byte)."""
    T = di.text_with_bwt_like(di.WHOLE_BLOCKS[name][2]())
    L, primary, _ = ref.bwt_encode(T)
    v = probe(L)
    assert v["n"] == T.size >= 1 << 20 and v["nb"] >= 2 and v["runs"] <= 0.70 * v["n"], (name, v)
    di.check_tag(name, v, di.WHOLE_BLOCKS)
