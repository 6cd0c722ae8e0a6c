"""Inputs of the tests of the LZP stage over a pass (test_lzp_batch_plan_host.py on the CPU, test_gpu_lzp_batch.py on the GPU): passes
made of lzp_device_inputs' blocks, the cut rule of lzp_staged.h restated, and the host encoder's and the stand-in's answers per block,
computed once (lzp_device_inputs.want)."""
import functools

import numpy as np

import lzp_device_inputs as I
from libbsc_amd import api, gpu

MAX_N = (4 << 20) + 4096
BATCH_MAX_N = 1 << 20
MAX_BLOCKS = 4096


# ---- lzp_staged.h: num_chunks / chunk_start / chunk_size, and the sizes the encoder refuses (lzp.cpp:531) ---------------------------------
def num_chunks(n):
    return 1 if n < 256 * 1024 else 2 if n < 4 << 20 else 4 if n < 16 << 20 else 8


def chunk_start(n, nc, b):
    return b * (n // nc)


def chunk_size(n, nc, b):
    return n // nc if b != nc - 1 else n - b * (n // nc)


def refused(n, min_len):
    return n - min_len < 32 or n - 2 < 16


def plan(sizes, min_len):
    """the chunk table the issue asks for: (block, start in the pass, size, cap) per chunk"""
    out, off = [], 0
    for b, n in enumerate(sizes):
        nc = num_chunks(n)
        if not (nc == 1 and refused(n, min_len)):
            for i in range(nc):
                out.append((b, off + chunk_start(n, nc, i), chunk_size(n, nc, i), n - 2 if nc == 1 else chunk_size(n, nc, i)))
        off += n
    return out


# ---- passes ---------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def corpora_pass():
    """the seven corpora as one pass (every one is below 1 MiB as it is): [(key, block)]"""
    return [(name, T[:BATCH_MAX_N - 1]) for name, T in I.corpora().items()]


@functools.lru_cache(maxsize=None)
def neighbours_pass():
    """one compressible block three times side by side, and a block of 300 000 bytes whose two chunks are the same bytes: a link that
    crossed a chunk would give the later copy matches at its first positions"""
    one = I.corpora()["repeat"][:100_000]
    half = I.corpora()["copied"][:150_000]
    return [("nb_one", one), ("nb_one", one), ("nb_one", one), ("nb_halves", np.concatenate([half, half]))]


def threshold_pass(min_len):
    """blocks at the chunk thresholds, tiny ones between them: refused sizes, the boundary of the refusal, an empty block"""
    big = I.threshold_block()
    out, at = [], 0
    for n_big, n_tiny in zip((256 * 1024 - 1, 256 * 1024, 256 * 1024 + 1, (1 << 20) - 1), ((1, 17), (18, min_len + 31), (min_len + 32, 0), ())):
        out.append((("thr", at, n_big), big[at:at + n_big]))
        at += 1000
        for n in n_tiny:
            out.append((("thr", at, n), big[at:at + n]))
            at += 1000
    return out


@functools.lru_cache(maxsize=None)
def second_chunk_raw():
    """first_chunk_raw mirrored: zeros, then random bytes — the first chunk is coded, the second kept raw"""
    return I.first_chunk_raw()[::-1].copy()


@functools.lru_cache(maxsize=None)
def raw_pass():
    return [("first_chunk_raw", I.first_chunk_raw()), ("second_chunk_raw", second_chunk_raw()), ("random", I.corpora()["random"])]


@functools.lru_cache(maxsize=None)
def many_small_pass():
    """700 blocks of 2 - 6 KiB cut from `copied` and `repeat_dense_f2`: more chunks than the device has CUs"""
    rng = np.random.default_rng(21)
    src = (I.corpora()["copied"], I.corpora()["repeat_dense_f2"])
    out = []
    for b in range(700):
        S = src[b % 2]
        n = int(rng.integers(2048, 6145))
        at = int(rng.integers(0, S.size - n))
        out.append((("small", b), S[at:at + n]))
    return out


@functools.lru_cache(maxsize=None)
def tiny_pass(count=MAX_BLOCKS):
    """`count` blocks of 40 - 300 bytes from the three generators of lzp_device_inputs.tiny_cases"""
    rng = np.random.default_rng(12)
    out = []
    for it in range(count):
        n = int(rng.integers(40, 301))
        T = [np.zeros(n, np.uint8), (rng.integers(0, 2, n) * 0xF2).astype(np.uint8),
             np.tile(rng.integers(0, 256, int(rng.integers(1, 7)), dtype=np.uint8), n)[:n].copy()][it % 3]
        out.append((("tinyb", it), T))
    return out


def path_pass(name):
    """the input of lzp_device_inputs.PATHS[name] between two other blocks"""
    make = I.PATHS[name][0]
    return [("zeros", I.corpora()["zeros"]), (("path", name), make()), ("text", I.corpora()["text"])]


def sizes_of(blocks):
    return [int(T.size) for _, T in blocks]


def joined(blocks):
    parts = [T for _, T in blocks if T.size]
    return np.ascontiguousarray(np.concatenate(parts)) if parts else np.zeros(0, np.uint8)


def wants(blocks, h, m, f):
    """api.bsc_lzp_compress per block (computed once per (key, h, m, f))"""
    return [I.want(key, T, h, m, f) for key, T in blocks]


_STAGED = {}


def staged_counters(blocks, h, m, f):
    """the sum of bscgpu_lzp_staged_host's counters over the blocks (each computed once)"""
    total = dict.fromkeys(gpu.LZP_COUNTERS, 0)
    for key, T in blocks:
        k = (key, h, m, f)
        if k not in _STAGED:
            got, cnt = gpu.lzp_staged_host(T, h, m, features=f)
            assert got == I.want(key, T, h, m, f), (k, "the stand-in against the host encoder")
            _STAGED[k] = cnt
        for name, v in _STAGED[k].items():
            total[name] += v
    return total
