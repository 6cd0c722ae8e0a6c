"""Inputs of the tests of the exact resolve of open chunk starts (CPU: test_replay_resolve_host.py, GPU: test_gpu_replay_resolve.py), on
top of devcoder_inputs.py: the CPU judge (tools/replay_resolve_probe.cpp: the host restatement of the kernels against the plain serial
walk), synthetic evaluations that put a stretch against each of its edges, and the block of under 1 MiB whose second sub-block holds a
chain long enough for FAIL_REPLAY (a batched pass takes only blocks below 1 MiB)."""
import json
import os
import subprocess

import numpy as np

import devcoder_inputs as di

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DC_EV, DC_EB, DC_RP_CAND, DC_REPLAY_MAX = 8192, 64, 384, 64       # devcoder_model.h (test_bound holds the probe's constants to these)
ROWMARK = 0x1000
FAM_STATE, FAM_CHAR, FAM_STATIC = 0, 1, 2
TAU_RF, TAU_RE, TAU_RM, TAU_NF = 0, 1, 8, 510                    # first decision type (row) of a class

KEPT = [k for k, (t, _, _) in di.GENERATORS.items() if t == "replay_kept"]
# ... and the second table's fail_replay: the block di.WHOLE_BLOCKS builds its text from, as a sorted block of its own
WHOLE_FAIL = "whole_blocks_fail_replay"
FAIL = [k for k, (t, _, _) in di.GENERATORS.items() if t == "fail_replay"] + [WHOLE_FAIL]


def block_of(name):
    """the sorted block of a name in KEPT or FAIL"""
    return di.WHOLE_BLOCKS["fail_replay"][2]() if name == WHOLE_FAIL else di.GENERATORS[name][2]()


# the guard: (generator, cap below its widest start bracket)
GUARD_KEPT = ("alt_rm_static", 64)
GUARD_FAIL = ("alt_rf_static_2x73_chunks", 2)


def build_probe(dirname):
    """compile tools/replay_resolve_probe.cpp into dirname (the command of devcoder_inputs.build_probe) -> path of the program"""
    exe = os.path.join(str(dirname), "replay_resolve_probe")
    subprocess.run(["g++", "-O2", "-std=c++17", "-march=x86-64-v3", "-I", os.path.join(ROOT, "libbsc_amd/csrc/host"), "-I", os.path.join(ROOT, "libbsc_amd/csrc/device"),
                    "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tools/replay_resolve_probe.cpp"), os.path.join(ROOT, "libbsc_amd/csrc/host/coder.cpp"),
                    "-o", exe, "-lpthread"], check=True)
    return exe


def _run(args):
    r = subprocess.run(args, capture_output=True, text=True)
    assert r.returncode == 0, (args, r.stderr)
    return json.loads(r.stdout)


def probe_bound(exe):
    return _run([exe, "bound"])


_cache = {}


def probe_block(exe, dirname, L, cand=None, key=None):
    """the probe's verdict on a sorted block (split into sub-blocks as the stage function splits it); key: computed once per process"""
    if key is not None and (key, cand) in _cache:
        return _cache[key, cand]
    path = os.path.join(str(dirname), "block.bin")
    np.ascontiguousarray(L, dtype=np.uint8).tofile(path)
    v = _run([exe, "block", path] + ([str(cand)] if cand is not None else []))
    if key is not None:
        _cache[key, cand] = v
    return v


def probe_events(exe, dirname, jobs, ev, coder=0, cand=DC_RP_CAND):
    """... on a synthetic evaluation: jobs = [(family, [(row, events of the row as uint16), ...]), ...], rows in increasing order"""
    ep, fp = os.path.join(str(dirname), "events.bin"), os.path.join(str(dirname), "events.txt")
    words = [f"{coder} {ev} {cand} {len(jobs)}"]
    parts = []
    for fam, rows in jobs:
        assert [r for r, _ in rows] == sorted({r for r, _ in rows})
        words.append(f"{fam} {sum(len(e) for _, e in rows)} {len(rows)}")
        for r, e in rows:
            words.append(f"{r} {len(e)}")
            parts.append(np.asarray(e, dtype=np.uint16))
    np.concatenate(parts).tofile(ep)
    with open(fp, "w") as f:
        f.write("\n".join(words))
    return _run([exe, "events", ep, fp])


# ---- synthetic evaluations ------------------------------------------------------------------------------------------------------------
def alternating(n, sig=0, phase=0):
    """n events of one chain (signature sig = X | sub-block << 8) whose bits alternate: under the static coder's slow counters (the state
    family, and the context-free family's RF) the two ends of the bracket settle on two orbits and never meet"""
    return (sig | (((np.arange(n) + phase) & 1) << 11)).astype(np.uint16)


def pattern(n, word, sig=0):
    return (sig | (np.asarray(word)[np.arange(n) % len(word)] << 11)).astype(np.uint16)


def random_with_stretches(seed, n, sig=0, stretch=3 * DC_EV):
    """random bits (the bracket meets within a few hundred events) with alternating stretches of 2/3 .. 1 `stretch` events planted at random
    places (one that spans two chunks and a bit leaves a chunk open wherever the boundaries fall)"""
    rng = np.random.default_rng(seed)
    bits = rng.integers(0, 2, n)
    for at in rng.integers(0, max(1, n - stretch), max(1, n // (4 * stretch))):
        k = int(rng.integers(2 * stretch // 3, stretch))
        bits[at:at + k] = (np.arange(k) & 1)[:n - at]
    return (sig | (bits << 11)).astype(np.uint16)


EVS = (DC_EV, DC_EV + 64, 2 * DC_EV)                              # chunk sizes eval_chunk_events gives: the minimum, a unit above it, twice it

# name -> (builder of the jobs for a chunk size, open chunks, stretches) where the counts follow from the layout alone.  A chunk that
# begins with a chain start walks exactly (both ends are reset at its first event), so the chunk behind it is never open: the first
# open chunk of a chain is the third it touches, and the head of a stretch is the second.
EDGE_CASES = {
    # chunks 2 and 3 are open; 3 is the job's last, partial chunk
    "partial_last_chunk": (lambda ev: [(FAM_STATIC, [(TAU_RF, alternating(3 * ev + ev // 2 + 8))])], 2, 1),
    # a row starts exactly at chunk 3: the bracket in front of it is open, the chunk does not continue
    "row_start_at_a_boundary": (lambda ev: [(FAM_STATE, [(TAU_RF, alternating(3 * ev)), (TAU_RM, alternating(3 * ev))])], 2, 2),
    # a row starts inside chunk 2: both ends are reset there and the bracket of chunk 2 meets
    "row_start_inside_a_chunk": (lambda ev: [(FAM_STATE, [(TAU_RF, alternating(2 * ev + ev // 2)), (TAU_RM, alternating(3 * ev + ev // 2))])], 3, 2),
    # the same signature throughout; the event at 3 ev carries the mark (another sub-block with the same signature modulo 8)
    "marked_event_at_a_boundary": (lambda ev: [(FAM_STATIC, [(TAU_RF, _marked(alternating(6 * ev), 3 * ev))])], 2, 2),
    "marked_event_inside_a_chunk": (lambda ev: [(FAM_STATIC, [(TAU_RF, _marked(alternating(6 * ev), 2 * ev + 100))])], 3, 2),
    # another sub-block in the signature, inside a chunk
    "signature_change": (lambda ev: [(FAM_STATIC, [(TAU_RF, np.concatenate([alternating(2 * ev + 64), alternating(3 * ev, sig=1 << 8)]))])], 3, 2),
    # two jobs with stretches (the later job's chunk slots start behind the earlier ones', padded to 64) and a short job between them; the
    # second stretch is 69 chunks long: without the resolve the unit is declined
    "two_jobs": (lambda ev: [(FAM_STATIC, [(TAU_RF, alternating(4 * ev))]), (FAM_CHAR, [(TAU_RF, alternating(100, sig=7))]), (FAM_STATIC, [(TAU_RF, alternating(70 * ev + 5))])], 2 + 69, 2),
}


def _marked(e, at):
    e = e.copy()
    e[at] |= ROWMARK
    return e


# ---- a block below 1 MiB that declines for FAIL_REPLAY ---------------------------------------------------------------------------------
def skewed_fail_replay_block(n_tail=31_000):
    """Under 1 MiB (what a batched pass takes) a block has two sub-blocks, and split evenly neither holds a chain of more than
    DC_REPLAY_MAX + 2 chunks.  The split samples every 32nd position and halves the sampled run starts: 8 KiB of single-byte runs
    (every sampled position starts a run), then groups of 32 bytes — a run of two bytes across the sampled position, thirty runs of
    one — with no sampled run start at all.  The cut falls inside the first 8 KiB and the second sub-block holds the rest: 31 runs
    per 32 bytes, whose ranks alternate (the word of alt_rf_static_*), about 118 chunks of the context-free RF chain."""
    head = 8192
    runs = head + 31 * n_tail
    w = np.asarray(di._W_RF_STATIC)
    sym = di._symbols(3)[w[np.arange(runs) % w.size]]
    length = np.concatenate([np.ones(head, np.int64), np.tile(np.array([2] + [1] * 30), n_tail)])
    return di.runs_to_block(sym, length)


def fail_replay_pass():
    """the block above between two text-like blocks (model_batch_inputs.fail_hist_pass's neighbours)"""
    from front_inputs import KI, runs_block
    rng = np.random.default_rng(43)
    return [runs_block(rng, 100 * KI, 33), skewed_fail_replay_block(), runs_block(rng, 64 * KI, 17)]
