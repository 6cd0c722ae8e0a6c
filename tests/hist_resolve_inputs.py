"""Inputs of the exact run_hist resolve's tests (CPU: test_hist_resolve_host.py, GPU: test_gpu_hist_resolve.py), on top of
devcoder_inputs.py: run sequences in symbol-major order whose chains keep their bracket open across chunk and group borders, and the
CPU judge (tools/hist_resolve_probe.cpp: the host restatement of the kernels against the serial walk).  Every input here must leave
brackets open (`ext > 0` from the probe): one that does not tests nothing."""
import json
import os
import subprocess

import numpy as np

import devcoder_inputs as di

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CH, GROUP = 1024, 64                                  # DC_HIST_CH, DC_HIST_GROUP (the probe's `bound` reports them)
HIST_EXT_GENERATORS = tuple(k for k, v in di.GENERATORS.items() if v[0] == "hist_ext" and k.startswith("hist_"))
FAIL_HIST_GENERATORS = tuple(k for k, v in di.GENERATORS.items() if v[0] == "fail_hist")


def build_probe(dirname):
    """compile tools/hist_resolve_probe.cpp into dirname (the command of devcoder_inputs.build_probe) -> path of the program"""
    exe = os.path.join(str(dirname), "hist_resolve_probe")
    subprocess.run(["g++", "-O2", "-std=c++17", "-march=x86-64-v3", "-I", os.path.join(ROOT, "libbsc_amd/csrc/host"), "-I", os.path.join(ROOT, "libbsc_amd/csrc/device"),
                    "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tools/hist_resolve_probe.cpp"), os.path.join(ROOT, "libbsc_amd/csrc/host/coder.cpp"),
                    "-o", exe, "-lpthread"], check=True)
    return exe


def _run(args):
    r = subprocess.run(args, capture_output=True, text=True)
    assert r.returncode == 0, (args, r.stderr)
    return json.loads(r.stdout)


def probe_bound(exe):
    return _run([exe, "bound"])


def probe_runs(exe, dirname, chain, run):
    """the probe's verdict on runs in symbol-major order: chain[q] names the chain of element q, run[q] is its length"""
    path = os.path.join(str(dirname), "runs.bin")
    np.stack([np.asarray(chain, dtype=np.uint32), np.asarray(run, dtype=np.uint32)], axis=1).tofile(path)
    return _run([exe, "runs", path])


def probe_block(exe, dirname, L):
    """... on a sorted block (split into sub-blocks as the stage function splits it)"""
    path = os.path.join(str(dirname), "block.bin")
    np.ascontiguousarray(L, dtype=np.uint8).tofile(path)
    return _run([exe, "block", path])


# ---- run sequences in symbol-major order ----------------------------------------------------------------------------------------------
def chains(lengths, fill=2):
    """chains of the given numbers of elements, one after the other, every run `fill` bytes long -> (chain, run)"""
    chain = np.repeat(np.arange(len(lengths), dtype=np.uint32), lengths)
    return chain, np.full(chain.size, fill, dtype=np.uint32)


def planted(seed, m, stretches=12, nchains=5):
    """random run lengths of every class (1 .. 2^20 bytes) in `nchains` chains of random sizes, with `stretches` planted stretches of
    20 to 3000 runs of one class between 1 and 6 (two fixed points: the bracket stays open through them) -> (chain, run)"""
    rng = np.random.default_rng(seed)
    run = (1 << rng.integers(0, 21, m)).astype(np.uint32) + rng.integers(0, 2, m).astype(np.uint32)
    for _ in range(stretches):
        n = int(rng.integers(20, 3001))
        at = int(rng.integers(0, m - n))
        b = int(rng.integers(1, 7))
        run[at:at + n] = rng.integers(1 << b, 2 << b, n)
    cuts = np.sort(rng.choice(np.arange(1, m), nchains - 1, replace=False))
    chain = np.searchsorted(cuts, np.arange(m), side="right").astype(np.uint32)
    return chain, run


PLANTED_CASES = [(seed, m) for m in (3000, 20_000, 70_000) for seed in (1, 2)]
