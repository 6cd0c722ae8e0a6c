"""The inputs of the combined-resolve tests judged on the CPU (no GPU needed): every block of resolve_combined_inputs.BLOCKS, the
whole-block text's BWT and the blocks of the batched pass are pinned to their reasons for leaving the device by the paths probe
(tools/devcoder_paths_probe.cpp), to the mask the stage must return under each of the eight sets of the three options, and the three
resolves' host restatements (avg_resolve_probe, hist_resolve_probe, replay_resolve_probe) must settle everything each of them leaves
open.  The GPU tests (test_gpu_resolve_combined.py) hold the device to the same verdicts, so none of them can pass on an input that
quietly missed a path."""
import numpy as np
import pytest

import devcoder_inputs as di
import resolve_combined_inputs as rc


@pytest.fixture(scope="module")
def t(tmp_path_factory):
    return rc.tools(tmp_path_factory.mktemp("combined_probes"))


def _check_resolves(t, key, L, p):
    """all three host restatements accept the block, and count what the paths probe counts"""
    a, h, r = rc.avg(t, key, L), rc.hist(t, key, L), rc.replay(t, key, L)
    print(key, "avg", a["und"], "hist", h["ext"], "replay off", r["off"], "on", r["on"])
    assert a["flags_equal"] and a["resolved"] == a["und"] == p["avg_und"] and a["left"] == 0 and a["sub_left"] == 0, (key, a)
    assert h["values_equal"] and h["resolved"] == h["ext"] == p["hist_ext"], (key, h)
    on, off = r["on"], r["off"]
    assert on["starts_equal"] and off["starts_equal"] and on["resolved"] == on["open"] == off["open"] and on["wide"] == 0 and on["replays"] == 0 and not on["fail_replay"], (key, r)
    assert off["fail_replay"] == (rc.REPLAY in rc.reasons(p)), "the restatement and the paths probe agree on FAIL_REPLAY"
    assert r["decisions"] == p["decisions"] and r["nb"] == p["nb"]
    return a, h, r


def test_option_sets_and_the_rule():
    assert len(rc.OPTION_SETS) == 8 and sorted(rc.set_index(o) for o in rc.OPTION_SETS) == list(range(8))
    assert set(rc.LATTICE) | {rc.KEPT_EITHER_WAY} == set(rc.BLOCKS)
    assert not set(rc.BLOCKS) & set(di.GENERATORS), "a table of its own"
    R = {rc.AVG, rc.HIST, rc.REPLAY}
    assert rc.mask_rule(R, ()) == 6 and rc.mask_rule(R, (rc.REPLAY,)) == 6 and rc.mask_rule(R, (rc.AVG,)) == 4 and rc.mask_rule(R, (rc.HIST,)) == 2
    assert rc.mask_rule(R, (rc.AVG, rc.HIST)) == 16 and rc.mask_rule(R, rc.ALL_ON) == 0


@pytest.mark.parametrize("name", list(rc.BLOCKS))
def test_block_has_its_reasons_and_its_mask_under_every_option_set(t, name):
    L = rc.block(name)
    m, p = rc.masks(t, name, L), rc.paths(t, name, L)
    R = rc.reasons(p)
    print(name, "n", L.size, "nb", p["nb"], "avg_und", p["avg_und"], "hist_ext", p["hist_ext"], "hist_fail", p["hist_fail"], "masks", m)
    assert R == (rc.LATTICE[name] if name in rc.LATTICE else {rc.AVG}), (name, R)
    assert len(R) >= 2 or name == rc.KEPT_EITHER_WAY, "more than one reason to leave the device"
    for o in rc.OPTION_SETS:
        assert m[rc.set_index(o)] == rc.mask_rule(R, o), (name, o, m)
        assert not (m[rc.set_index(o)] & di.FAIL_REPLAY and m[rc.set_index(o)] & (di.FAIL_AVG | di.FAIL_HIST)), "FAIL_REPLAY is never beside an exit of the first sync"
    assert m[0] == p["fail_mask"] and m[7] == 0
    if len(R) == 3 or R == {rc.AVG, rc.HIST}:
        assert m[0] == 6, "two bits"
    a, h, r = _check_resolves(t, name, L, p)
    if name == rc.KEPT_EITHER_WAY:
        # all three resolves have work to do on a block that only its avg flags keep off the device
        assert a["und"] > 0 and h["ext"] > 0 and p["hist_fail"] == 0 and r["off"]["replays"] > 0 and r["on"]["open"] > 0 and not r["off"]["fail_replay"]
    if name == "same_runs":
        assert p["nb"] == 2 and a["und"] > 0.9 * p["runs"] and p["hist_fail"] > 0 and r["on"]["open"] > 2 * 66, "open in all three ways, in both sub-blocks"


@pytest.mark.parametrize("name", ["avg_hist", "all_concat", "same_runs_small"])
def test_option_words_one_call_per_set(t, name):
    """the probe asked once per option set, words in either order: the mask of the one-walk table, the words echoed, every count the same"""
    L = rc.block(name)
    m, base = rc.masks(t, name, L), rc.paths(t, name, L)
    verdicts = ("fail_mask", "replay_certain", "no_replay_certain", "no_fail_replay_certain") + di.PROBE_OPTIONS
    for o in rc.OPTION_SETS:
        v = rc.paths(t, name, L, o)
        assert v["fail_mask"] == m[rc.set_index(o)], (name, o)
        assert {w for w in di.PROBE_OPTIONS if v.get(w)} == set(o)
        assert {k: x for k, x in v.items() if k not in verdicts} == {k: x for k, x in base.items() if k not in verdicts}
        if len(o) > 1:
            assert di.run_probe(t["paths"], L, t["dir"], o[::-1]) == v


def test_probe_refuses_an_unknown_word(t):
    import subprocess
    r = subprocess.run([t["paths"], "nothing.bin", "avg_exakt"], capture_output=True, text=True)
    assert r.returncode == 2 and "avg_exakt" in r.stderr


def test_whole_block_text(t, ref):
    """the text of the whole-block GPU test: the reference's BWT of it keeps all three reasons, and is a block bsc_compress gives to
    the device model at all (>= 1 MiB, several sub-blocks, at most 0.70 runs per byte)"""
    T = rc.whole_block_text()
    L, _, _ = ref.bwt_encode(T)
    src = rc.whole_block_source()
    assert L.size == src.size and 0 < np.count_nonzero(L != src) < 100, "the generated block up to a few swaps"
    m, p = rc.masks(t, "whole", L), rc.paths(t, "whole", L)
    print("whole block: n", T.size, "nb", p["nb"], "runs", p["runs"], "avg_und", p["avg_und"], "hist_ext", p["hist_ext"], "hist_fail", p["hist_fail"], "masks", m)
    assert p["n"] == T.size >= 1 << 20 and p["nb"] >= 2 and p["runs"] <= 0.70 * p["n"]
    R = rc.reasons(p)
    assert R == {rc.AVG, rc.HIST, rc.REPLAY}
    assert all(m[rc.set_index(o)] == rc.mask_rule(R, o) for o in rc.OPTION_SETS) and m[0] == 6
    # with any one option off again, that option's bit alone
    assert [m[rc.set_index(tuple(w for w in rc.ALL_ON if w != o))] for o in rc.ALL_ON] == [di.FAIL_AVG, di.FAIL_HIST, di.FAIL_REPLAY]
    _, _, r = _check_resolves(t, "whole", L, p)
    assert r["on"]["open"] > 2 * 66


def test_text_pass(t, ref):
    """the texts of the compress-batch test: the reference's BWT of each has the one reason it is there for, the neighbours none"""
    got = []
    for b, T in enumerate(rc.text_pass()):
        L, _, _ = ref.bwt_encode(T)
        m, p = rc.masks(t, f"text{b}", L), rc.paths(t, f"text{b}", L)
        R = rc.reasons(p)
        assert all(m[rc.set_index(o)] == rc.mask_rule(R, o) for o in rc.OPTION_SETS), (b, m)
        got.append(R)
    assert got == rc.TEXT_PASS_REASONS


def test_batched_pass(t):
    """every block under 1 MiB; three bad blocks with one reason each, a fourth that its avg flags keep off the device while all three
    resolves have work to do on it; the neighbours have no reason"""
    blocks, fb, _, _, _ = rc.pass_reference()
    assert fb.count == 6 and all(b.size < 1 << 20 for b in blocks)
    got = []
    for b, L in enumerate(blocks):
        m, p = rc.masks(t, f"pass{b}", L), rc.paths(t, f"pass{b}", L)
        R = rc.reasons(p)
        assert all(m[rc.set_index(o)] == rc.mask_rule(R, o) for o in rc.OPTION_SETS), (b, m)
        a, h, r = _check_resolves(t, f"pass{b}", L, p)
        got.append(R)
        if b == 4:
            assert a["und"] > 0 and h["ext"] > 0 and r["on"]["open"] > 0
    assert got == [set(), {rc.AVG}, {rc.HIST}, {rc.REPLAY}, {rc.AVG}, set()]
