"""Inputs of the tests of a single block in sub-block segments (tests/test_gpu_block_segments.py): the text blocks, the uneven block,
the arena's capacities as include/bscgpu.h states them, and the CPU stand-in's facts of a sorted block (tools/devcoder_paths_probe.cpp)."""
import functools

import numpy as np

import devcoder_inputs as di

MIB = 1 << 20
SIZES = {"1m+1": MIB + 1, "4m": 4 * MIB, "16m": 16 * MIB}         # 2, 4 and 8 sub-blocks
SEEDS = {"1m+1": 11, "4m": 12, "16m": 13}
DIVISORS = (2, 4, 8)


def capacity(max_n, k):
    """(Mcap, Dcap) of a context: runs — the bytes of ceil(max_n / k) plus 4096, rounded up to 4096 — and decisions, four per run plus 65536"""
    mcap = (-(-max_n // k) + 4096 + 4095) // 4096 * 4096
    return mcap, 4 * mcap + 65536


@functools.lru_cache(maxsize=None)
def text(name):
    """a synth_text_v1 block, built once per process and shared; nobody writes to it"""
    from libbsc_amd.synth import synth_text_v1
    T = synth_text_v1(SEEDS[name], SIZES[name])
    T.setflags(write=False)
    return T


@functools.lru_cache(maxsize=None)
def pipe_texts():
    from libbsc_amd.synth import synth_text_v1
    out = [synth_text_v1(20 + i, 4 * MIB) for i in range(4)]
    for T in out:
        T.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def uneven_block():
    """a sorted block of 4 MiB: the first half the look of a text's BWT (short runs over a skewed alphabet), the second half runs of
    nine to twelve thousand bytes — 64 consecutive ones hold more decisions than a wavefront of the stream kernel stages (30 each
    against 1792 in all), so the packed form of whatever unit holds them is void, and the sub-blocks differ widely in runs"""
    rng = np.random.default_rng(77)
    half = 2 * MIB
    p = 1.0 / np.arange(1, 61) ** 1.3
    sym = rng.choice(60, size=half, p=p / p.sum()).astype(np.uint8) + 32
    head = np.repeat(sym[: half // 2 + 1], rng.integers(1, 4, half // 2 + 1))[:half]
    lens = rng.integers(9000, 12000, 400)
    syms = (rng.permutation(400) % 23 + 100).astype(np.uint8)
    tail = np.repeat(syms, lens)[:half]
    assert tail.size == half
    L = np.concatenate([head, tail])
    L.setflags(write=False)
    return L


def stand_in_facts(exe, L, dirname):
    """the CPU stand-in's (sub_runs, sub_decisions for -e1, undecided avg_rank flags per sub-block) of the sorted block L"""
    v = di.run_probe(exe, L, dirname)
    return v["sub_runs"], v["sub_decisions"], v["avg_und_sb"]
