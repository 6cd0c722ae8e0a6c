"""Inputs of the BWT driver's GPU tests that more than one test needs: the planted-phrase texts (long groups after the first sort), the
source-like and object-like blocks (prefix-doubling rounds with large groups), and the fixed list the round trace is taken over
(test_gpu_bwt_round_trace.py asserts it, make_bwt_round_trace.py records it).

Run as a program it is the round trace's child process: `python tests/bwt_inputs.py NAME...` transforms the named inputs in order with
one context, writes `== NAME` to stderr in front of each (the driver's `[bwt]` lines follow when BSCGPU_DEBUG is set) and checks every
block against libsais."""
import os
import re
import subprocess
import sys

import numpy as np

PHRASE = b"qzjxvkwpyfgmbqzjxvkwpyfgmbqzjxvkwpyfgmbhh"


def planted_phrase(rng, n, plen, times=3000):
    """synth text with the first plen characters of PHRASE planted `times` times, each time followed by different text"""
    from libbsc_amd import api
    T = api.synth_text_v1(31, n).copy()
    phrase = np.frombuffer(PHRASE[:plen], np.uint8)
    for p in rng.choice((n - 64) // 64, times, replace=False) * 64:
        T[p:p + plen] = phrase
    return T


def source_like(rng, n):
    from libbsc_amd import api
    T = api.synth_text_v1(5, n).copy()
    T[rng.integers(0, n, n // 300)] = rng.integers(128, 256, n // 300).astype(np.uint8)      # > 128 symbols: 8-bit codes, 8-character keys
    for p in rng.integers(0, n - 64, n // 40):                                                # indentation: runs of 4 .. 40 spaces
        T[p:p + int(rng.integers(4, 41))] = 32
    for _ in range(40):                                                                       # duplicated passages (LCPs up to 60 000)
        L = int(rng.integers(2000, 60000)); a, b = (int(x) for x in rng.integers(0, n - L, 2))
        T[b:b + L] = T[a:a + L]
    return T


def object_like(rng, n):
    T = rng.integers(0, 256, n).astype(np.uint8)
    for p in rng.integers(0, n - 5000, n // 2000):                                            # zero runs of 16 .. 4096 bytes
        T[p:p + int(rng.integers(16, 4097))] = 0
    tab = rng.integers(0, 256, 4096).astype(np.uint8)
    for p in rng.integers(0, n - 4096, 300):                                                  # the same table many times
        T[p:p + 4096] = tab
    return T


# ---- the round trace's inputs: name -> bytes; every input has a generator of its own, so one can grow without moving the others ----
MIB = 1 << 20
TRACE_SIZES = {"text": MIB, "phrase13": MIB, "phrase40": MIB, "source": MIB, "object": MIB, "period7": 256 << 10,
               "batch": [3001, 70_000, 200_000]}
TRACE_FIRST = ["text", "phrase13", "phrase40", "source", "object", "period7", "batch"]          # one child, one context, in this order
TRACE_RUNS = [("default", TRACE_FIRST, {}), ("hybrid-off", ["source"], {"BSC_BWT_HYBRID": "0"})]
# what the list as a whole must reach (asserted on the stored trace): a substring, or a pattern, per outcome
TRACE_OUTCOMES = {
    "a text round ran to its end": r"text round \d+ depth ",
    "long groups split and sorted": r"split by the top key bits -> sorted",
    "a split bucket still too long, or the round handed over": r"still too long|handing over",
    "long groups not split": r"not split",
    "a hybrid doubling round": r": hybrid,",
    "a doubling round through the segmented sort": r"\[bwt\] round \d+ h=.*\(passes 0\)",
    "a doubling round through the radix engine": r"\[bwt\] round \d+ h=.*\(passes [1-9]",
}


def trace_input(name):
    """-> one block, or the list of blocks of the batched pass"""
    from libbsc_amd import api
    n = TRACE_SIZES[name]
    if name == "text":
        return api.synth_text_v1(31, n)
    if name == "phrase13":
        return planted_phrase(np.random.default_rng(4), n, 13)
    if name == "phrase40":
        return planted_phrase(np.random.default_rng(5), n, 40)
    if name == "source":
        return source_like(np.random.default_rng(11), n)
    if name == "object":
        return object_like(np.random.default_rng(12), n)
    if name == "period7":
        return np.resize(np.frombuffer(b"abcabca", np.uint8), n).copy()
    if name == "batch":
        return [api.synth_text_v1(41 + b, m) for b, m in enumerate(n)]
    raise KeyError(name)


_MS = re.compile(r"\s*\(\d+\.\d+ ms\)")


def collect_trace(names, env):
    """One child process with the debug log on -> {name: the driver's [bwt] lines of that input, without their milliseconds}"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.abspath(__file__)] + list(names), capture_output=True, text=True,
                       env=dict(os.environ, BSCGPU_DEBUG="1", **env), cwd=root)
    assert r.returncode == 0 and all(f"{k} ok" in r.stdout for k in names), (r.stdout + r.stderr)[-3000:]
    out, cur = {}, None
    for line in r.stderr.splitlines():
        if line.startswith("== "):
            cur = out.setdefault(line[3:].strip(), [])
        elif line.startswith("[bwt]") and cur is not None:
            cur.append(_MS.sub("", line).rstrip())
    assert list(out) == list(names), list(out)
    return out


def collect_all():
    return {run: collect_trace(names, env) for run, names, env in TRACE_RUNS}


def _child(names):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    import torch
    from libbsc_amd import GpuContext
    from oracle.refbind import Ref
    ref = Ref()
    ctx = GpuContext(0, max_n=max(int(np.sum(TRACE_SIZES[k])) for k in names) + 4096)
    for name in names:
        T = trace_input(name)
        print("==", name, file=sys.stderr, flush=True)
        if isinstance(T, list):
            dT = torch.from_numpy(np.ascontiguousarray(np.concatenate(T))).cuda()
            got = ctx.bwt_batch(dT, [t.size for t in T], aux=False, dL=torch.empty_like(dT))
        else:
            L, idx, _ = ctx.bwt(T)
            got, T = [(L, idx, None)], [T]
        sys.stderr.flush()
        for b, (t, (L, idx, _)) in enumerate(zip(T, got)):
            wL, widx, _ = ref.bwt_encode(t, aux=False)
            assert idx == widx and np.array_equal(L, wL[:t.size]), (name, b)
        print(name, "ok", flush=True)
    ctx.close()


if __name__ == "__main__":
    _child(sys.argv[1:])
