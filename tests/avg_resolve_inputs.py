"""Inputs of the exact avg_rank resolve's tests (CPU: test_avg_resolve_host.py, GPU: test_gpu_avg_resolve.py), on top of
devcoder_inputs.py: rank sequences that leave flags open over many chunks, sorted blocks with such rank sequences, the realistic block
with a single open flag, and the CPU judge (tools/avg_resolve_probe.cpp: the host restatement of the kernels against the serial walk).
Every input here must leave flags open (`und > 0` from the probe): one that does not tests nothing."""
import json
import os
import subprocess

import numpy as np

import devcoder_inputs as di

KI = 1024
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAIL_AVG_GENERATORS = ("rank32", "rank62", "rank40_warm_front_255", "rank40_warm_1856")


def build_probe(dirname):
    """compile tools/avg_resolve_probe.cpp into dirname (the command of devcoder_inputs.build_probe) -> path of the program"""
    exe = os.path.join(str(dirname), "avg_resolve_probe")
    subprocess.run(["g++", "-O2", "-std=c++17", "-march=x86-64-v3", "-I", os.path.join(ROOT, "libbsc_amd/csrc/host"), "-I", os.path.join(ROOT, "libbsc_amd/csrc/device"),
                    "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tools/avg_resolve_probe.cpp"), os.path.join(ROOT, "libbsc_amd/csrc/host/coder.cpp"),
                    "-o", exe, "-lpthread"], check=True)
    return exe


def _run(args):
    r = subprocess.run(args, capture_output=True, text=True)
    assert r.returncode == 0, (args, r.stderr)
    return json.loads(r.stdout)


def probe_bound(exe):
    return _run([exe, "bound"])


def probe_ranks(exe, dirname, rank, first_run, top=255):
    """the probe's verdict on a rank sequence with sub-blocks starting at first_run (first_run[0] == 0; the end is appended)"""
    rp, fp = os.path.join(str(dirname), "ranks.bin"), os.path.join(str(dirname), "first.txt")
    np.ascontiguousarray(rank, dtype=np.uint8).tofile(rp)
    first = [int(x) for x in first_run] + [len(rank)]
    with open(fp, "w") as f:
        f.write(" ".join(str(x) for x in [len(first) - 1] + first + [top] * (len(first) - 1)))
    return _run([exe, "ranks", rp, fp])


def probe_block(exe, dirname, L):
    """... on a sorted block (split into sub-blocks as the stage function splits it)"""
    path = os.path.join(str(dirname), "block.bin")
    np.ascontiguousarray(L, dtype=np.uint8).tofile(path)
    return _run([exe, "block", path])


# ---- rank sequences ---------------------------------------------------------------------------------------------------------------
def stretches(seed, m, stretch=700):
    """(b) alternating stretches of about `stretch` runs: ranks drawn from {36, 40, 44, 52} in odd stretches and from {33, 60} in even
    ones — the average wanders between 33 and 60, where a warmed-up bracket's lower end stays below 32 and its upper end above, so
    it closes nowhere; two sub-block starts at random runs -> (rank, first_run)"""
    rng = np.random.default_rng(seed)
    rank = np.empty(m, np.uint8)
    j, odd = 0, False
    while j < m:
        n = int(rng.integers(stretch - 100, stretch + 101))
        rank[j:j + n] = rng.choice([36, 40, 44, 52] if odd else [33, 60], size=min(n, m - j))
        j, odd = j + n, not odd
    return rank, [0] + sorted(int(x) for x in rng.choice(np.arange(1, m), 2, replace=False))


def random_walk(seed, m):
    """(c) a +-1 random walk clipped to [20, 75], two sub-block starts at random runs -> (rank, first_run)"""
    rng = np.random.default_rng(seed)
    steps = rng.integers(0, 2, m) * 2 - 1
    r, out = 40, np.empty(m, np.uint8)
    for j in range(m):
        r = min(75, max(20, r + int(steps[j])))
        out[j] = r
    return out, [0] + sorted(int(x) for x in rng.choice(np.arange(1, m), 2, replace=False))


STRETCH_CASES = [(seed, m) for m in (3000, 9000, 20_000) for seed in (1, 2)]
# seeds for which the stand-in reports open flags (searched on the CPU over seeds 1..59: the walk has to cross 32 while its bracket
# is still open, which none of them does at m = 3000, one at 9000 and about one in seven at 20 000)
WALK_CASES = [(16, 9000), (16, 20_000), (30, 20_000), (39, 20_000)]


def block_with_ranks(rank, symbols=80):
    """a sorted block of runs of one byte whose QLFC ranks are `rank` almost everywhere: the rank of a run is the number of distinct
    symbols between it and the next run of its symbol, so the runs are laid from the last to the first out of a move-to-front list
    (the last occurrence of every symbol has whatever rank the front end gives it)"""
    a = [int(x) for x in di._symbols(symbols)]
    out = np.empty(len(rank), np.uint8)
    for j in range(len(rank) - 1, -1, -1):
        r = int(rank[j])
        assert 1 <= r < symbols
        s = a.pop(r)
        out[j] = s
        a.insert(0, s)
    return out


def stretches_block(seed=1, m=20_000):
    return block_with_ranks(stretches(seed, m)[0])


LONG_RUNS = 200_000              # constant rank 40: 196 chunks, four groups, one sub-block (under 256 KiB)
LONG_RUNS_TWO = 270_000          # ... 264 chunks in two sub-blocks of 134 977 and 135 023 runs: the second starts at run 833 of chunk 131
LONG_TWO_SUB_RUNS = [134_977, 135_023]


# ---- the realistic block: one open flag ---------------------------------------------------------------------------------------------
REALISTIC_SEED = 28             # searched on the CPU over seeds 1..39: 14, 18, 21 leave one flag open, 27 four, 28 five
REALISTIC_N = 1024 * KI


def realistic_text(seed=REALISTIC_SEED, n=REALISTIC_N):
    """five eighths bsc_synth_text_v1, three eighths float32 gaussian noise from a fixed numpy seed (half and half is 0.71 runs per
    byte, over the 0.70 up to which bsc_compress tries the device model; this mix is at 0.64): where the noise begins in the BWT the
    bracket's ends are a step apart as they cross 32, and for about one seed in seven a flag stays open"""
    from libbsc_amd.synth import synth_text_v1
    noise = np.random.default_rng(seed).standard_normal(3 * n // 32).astype(np.float32).view(np.uint8)
    return np.concatenate([synth_text_v1(seed, n - noise.size), noise])
