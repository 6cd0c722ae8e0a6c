"""Inputs of the tests that switch the device model's three exact resolves on together (CPU: test_resolve_combined_host.py, GPU:
test_gpu_resolve_combined.py), on top of devcoder_inputs.py: sorted blocks with MORE THAN ONE reason to leave the device — open
avg_rank flags, run_hist brackets open behind the last widening, counter chains open over more than DC_REPLAY_MAX + 2 chunks — side
by side and in the same runs, the whole-block text and the batched pass made of them, and the four CPU judges behind one cache.

The inputs live in a table of their own (BLOCKS), not in di.GENERATORS: the existing parametrisations select from that table by tag
and every generator there carries exactly one tag.  What each block must do is not written down here: the tests take it from the
probes at run time (the paths probe: reasons and the mask under every option set; the three resolve probes: the counts)."""
import functools
import itertools
import json
import os
import subprocess

import numpy as np

import avg_resolve_inputs as ar
import devcoder_inputs as di
import hist_resolve_inputs as hr
import replay_resolve_inputs as ri

AVG, HIST, REPLAY = "avg_exact", "hist_exact", "replay_exact"      # the paths probe's option words (di.PROBE_OPTIONS)
OPTION_SETS = [tuple(o for o, on in zip(di.PROBE_OPTIONS, bits) if on) for bits in itertools.product((0, 1), repeat=3)]
ALL_ON = di.PROBE_OPTIONS


def set_index(options):
    """index of an option set in the probe's fail_mask_by_option_set: avg_exact + 2 hist_exact + 4 replay_exact"""
    return sum(1 << di.PROBE_OPTIONS.index(o) for o in options)


def set_id(options):
    return "+".join(o[:-len("_exact")] for o in options) or "none"


# ---- the blocks -------------------------------------------------------------------------------------------------------------------------
def _static_stretch():
    return di.periodic(di._W_RF_STATIC, [1], 1_200_000)                 # (alt_rf_static_2x73_chunks: the context-free RF chain never meets)


def same_runs(runs):
    """pair_swap(40, runs) — ranks alternate 40 and 38: every avg_rank flag behind the warm-up open, and the alternation holds the
    counter brackets of the state and the context-free family open — where the first four symbols' runs are 2 bytes long and all others
    1: those four symbols' chains of same-class runs never close their run_hist bracket.  All three kinds of open in the same runs"""
    s = di.pair_swap(40, runs)
    return di.runs_to_block(s, np.where(np.isin(s, di._symbols(40)[:4]), 2, 1))


BLOCKS = {
    "avg_hist": lambda: np.concatenate([di.const_rank(40, 100_000), di.hist_chain(12_000)]),
    "avg_replay": lambda: np.concatenate([di.const_rank(40, 60_000), _static_stretch()]),
    "hist_replay": lambda: np.concatenate([di.hist_chain(12_000), _static_stretch()]),
    "all_concat": lambda: np.concatenate([di.const_rank(40, 60_000), di.hist_chain(12_000), _static_stretch()]),
    "all_concat_reversed": lambda: np.concatenate([_static_stretch(), di.hist_chain(12_000), di.const_rank(40, 60_000)]),
    "same_runs": lambda: same_runs(1_200_000),
    "same_runs_small": lambda: same_runs(60_000),
}
# the blocks of the option lattice, and which of the three reasons each must have (the paths probe confirms: reasons() below)
LATTICE = {"avg_hist": {AVG, HIST}, "avg_replay": {AVG, REPLAY}, "hist_replay": {HIST, REPLAY}, "all_concat": {AVG, HIST, REPLAY},
           "all_concat_reversed": {AVG, HIST, REPLAY}, "same_runs": {AVG, HIST, REPLAY}}
KEPT_EITHER_WAY = "same_runs_small"                                     # only its avg flags keep it off the device; hist and replay have work


@functools.lru_cache(maxsize=None)
def block(name):
    """a block of BLOCKS, built once per process and shared; nobody writes to it"""
    L = BLOCKS[name]()
    L.setflags(write=False)
    return L


def whole_block_source():
    """the generated block the whole-block text is made from: the three whole-block constructions of di.WHOLE_BLOCKS side by side (run
    lengths 1 1 2 4 and 1 1 2 4 1 keep it at under 0.70 runs per byte, which is what bsc_compress gives the device model)"""
    return np.concatenate([di.runs_to_block(di.const_rank(40, 200_000), np.tile([1, 1, 2, 4], 50_000)), di.hist_chain(100_000),
                           di.periodic(di._W_RF_STATIC, [1, 1, 2, 4, 1], 1_400_000)])


@functools.lru_cache(maxsize=None)
def whole_block_text():
    """a text whose BWT is whole_block_source() up to a few swaps: built once per process (a few seconds).  (A text made from same_runs
    does not work: its BWT collapses to two runs.)"""
    T = di.text_with_bwt_like(whole_block_source())
    T.setflags(write=False)
    return T


def combined_pass():
    """a batched pass (every block under 1 MiB) with one block per reason, same_runs at 200 000 runs (its avg flags keep it off the device;
    its run_hist brackets and its chunk starts are open too, within what the look-back and the serial replay still settle), and two
    text-like neighbours as in model_batch_inputs' passes"""
    import model_batch_inputs as mb
    from front_inputs import KI, runs_block
    rng = np.random.default_rng(44)
    blocks = [runs_block(rng, 100 * KI, 33), mb.fail_avg_pass()[1], mb.fail_hist_pass()[1], ri.skewed_fail_replay_block(), same_runs(200_000),
              runs_block(rng, 64 * KI, 17)]
    assert all(b.size < 1 << 20 for b in blocks)
    return blocks


@functools.lru_cache(maxsize=None)
def pass_reference():
    """(blocks, layout, the pass's bytes, the stand-in's entries, its poff) as model_segment_inputs.reference gives them for a named pass"""
    import model_batch_inputs as mb
    blocks = combined_pass()
    fb, flat = mb.layout(blocks)
    ps, poff = mb.host_streams(fb)
    for a in (flat, ps, poff):
        a.setflags(write=False)
    return blocks, fb, flat, ps, poff


@functools.lru_cache(maxsize=None)
def text_pass():
    """inputs (texts, not sorted blocks) of the compress-batch test: texts whose BWT keeps one reason each — the constructions of
    test_gpu_avg_resolve / test_gpu_hist_resolve's compress-batch tests and ri.skewed_fail_replay_block() — between two synthetic
    texts, every one under 1 MiB.  (A text made from same_runs does not work: its BWT collapses to two runs.)"""
    from libbsc_amd.synth import synth_text_v1
    texts = [synth_text_v1(81, 700 * 1024), di.text_with_bwt_like(di.runs_to_block(di.const_rank(40, 200_000), np.tile([1, 1, 2, 4], 50_000))),
             di.text_with_bwt_like(di.hist_chain(200_000)), di.text_with_bwt_like(ri.skewed_fail_replay_block()), synth_text_v1(82, 300 * 1024)]
    for x in texts:
        assert x.size < 1 << 20
        x.setflags(write=False)
    return texts


TEXT_PASS_REASONS = [set(), {AVG}, {HIST}, {REPLAY}, set()]             # (the paths probe on the reference's BWT of each text confirms)


# ---- the four judges, each verdict computed once per process ------------------------------------------------------------------------------
_tools = {}
_cache = {}


def tools(dirname):
    """the four probes, compiled once per process (side by side) into the first directory asked for"""
    if not _tools:
        from concurrent.futures import ThreadPoolExecutor
        with ThreadPoolExecutor(4) as pool:
            exe = {k: pool.submit(m.build_probe, dirname) for k, m in (("paths", di), ("avg", ar), ("hist", hr), ("replay", ri))}
            _tools.update(dir=str(dirname), **{k: f.result() for k, f in exe.items()})
    return _tools


def _cached(kind, key, compute):
    if (kind, key) not in _cache:
        _cache[kind, key] = compute()
    return _cache[kind, key]


def paths(t, key, L, options=()):
    """the paths probe's verdict on L under an option set"""
    return _cached(("paths", tuple(options)), key, lambda: di.run_probe(t["paths"], L, t["dir"], options))


def masks(t, key, L):
    """the paths probe's mask under each of the eight option sets, from one walk of the block (index: set_index)"""
    def compute():
        path = os.path.join(t["dir"], "probe_input.bin")
        np.ascontiguousarray(L, dtype=np.uint8).tofile(path)
        r = subprocess.run([t["paths"], path, "option_sets"], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        v = json.loads(r.stdout)
        _cache.setdefault((("paths", ()), key), {k: x for k, x in v.items() if k != "fail_mask_by_option_set"})
        return v["fail_mask_by_option_set"]
    return _cached("masks", key, compute)


def avg(t, key, L):
    return _cached("avg", key, lambda: ar.probe_block(t["avg"], t["dir"], L))


def hist(t, key, L):
    return _cached("hist", key, lambda: hr.probe_block(t["hist"], t["dir"], L))


def replay(t, key, L):
    return _cached("replay", key, lambda: ri.probe_block(t["replay"], t["dir"], L))


def reasons(p):
    """the reasons a block has to leave the device, from the paths probe's counts (whatever the options)"""
    longest = max(f["stretch"] for f in p["families"].values())
    return {o for o, has in ((AVG, p["avg_und"] > 0), (HIST, p["hist_fail"] > 0), (REPLAY, longest > p["fail_min"])) if has}


def mask_rule(R, options):
    """the reasons of the first sync that no option takes away, alone; else FAIL_REPLAY; else 0"""
    first = (di.FAIL_AVG if AVG in R and AVG not in options else 0) | (di.FAIL_HIST if HIST in R and HIST not in options else 0)
    return first if first else di.FAIL_REPLAY if REPLAY in R and REPLAY not in options else 0
