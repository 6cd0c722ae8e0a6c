"""Inputs of the LZP stage's tests (test_lzp_staged_host.py on the CPU, test_gpu_lzp_device.py on the GPU): the corpora, the parameter
grid, the named inputs that pin each path of the staged encoder by its counter, and the host encoder's answers, computed once."""
import functools

import numpy as np

from libbsc_amd import api
from libbsc_amd.synth import synth_repeat_v1, synth_text_v1

# minLen -> the narrow variants: 4..7 <4, no verify>, 8..16 <8, no verify>, > 16 <8, verify>
MINLENS = (4, 5, 7, 8, 9, 15, 16, 17, 40, 128, 255)
HASHES = (10, 15)
FEATURES = (1, 3)


def copied_passages(seed, n, noise_every=97):
    """Passages copied from earlier places, with a changed byte now and then: the copies make matches, and the positions behind a
    match find their slot's last entry skipped — the look-ups that have to ask the real table."""
    rng = np.random.default_rng(seed)
    out = np.empty(n, np.uint8)
    have = min(n, 2000)
    out[:have] = rng.integers(0, 64, have, dtype=np.uint8)
    while have < n:
        if rng.random() < 0.8:
            src = int(rng.integers(0, have))
            ln = min(int(rng.integers(20, 700)), n - have, have - src)
            out[have:have + ln] = out[src:src + ln]
            noise = np.arange(int(rng.integers(1, noise_every)), ln, noise_every)
            out[have + noise] = rng.integers(0, 256, noise.size, dtype=np.uint8)
        else:
            ln = min(int(rng.integers(1, 60)), n - have)
            out[have:have + ln] = rng.integers(0, 64, ln, dtype=np.uint8)
        have += ln
    return out


@functools.lru_cache(maxsize=None)
def corpora():
    """test_host_lzp.py's six and the copied passages"""
    rng = np.random.default_rng(5)
    return {"zeros": np.zeros(70_000, np.uint8),
            "repeat": synth_repeat_v1(3, 300_000, 4000),
            "repeat_dense_f2": synth_repeat_v1(4, 200_000, 900, noise_every=40),
            "text": synth_text_v1(3, 150_000),
            "random": rng.integers(0, 256, 100_000, dtype=np.uint8),
            "f2_runs": (rng.integers(0, 3, 120_000) * 0x79).astype(np.uint8),      # bytes 0x00 0x79 0xF2
            "copied": copied_passages(7, 260_000)}


@functools.lru_cache(maxsize=None)
def first_chunk_raw():
    """two chunks, the first kept raw: 299 000 random bytes, then zeros (test_host_lzp.py)"""
    return np.concatenate([np.random.default_rng(6).integers(0, 256, 299_000, dtype=np.uint8), np.zeros(1000, np.uint8)])


@functools.lru_cache(maxsize=None)
def threshold_block():
    return synth_repeat_v1(8, (4 << 20) + 5, 50_000)


THRESHOLD_SIZES = (256 * 1024 - 1, 256 * 1024, (4 << 20) - 1, 4 << 20)

# name -> (input, hashSize, minLen, features, the counter that must move; None: the block as a whole is not compressible)
PATHS = {
    "matches":      (lambda: corpora()["repeat"], 15, 32, 3, "matches"),
    "dirty":        (lambda: corpora()["copied"], 15, 8, 3, "dirty"),
    "serial_zones": (lambda: corpora()["repeat_dense_f2"], 15, 40, 3, "serial_zones"),
    "serial_zones_128": (lambda: corpora()["repeat_dense_f2"], 10, 128, 3, "serial_zones"),
    "escapes":      (lambda: corpora()["repeat_dense_f2"], 15, 8, 3, "escapes"),
    "raw_chunks":   (first_chunk_raw, 15, 32, 3, "raw_chunks"),
    "block_not_compressible": (lambda: corpora()["random"], 15, 32, 3, None),
}


def tiny_cases():
    """the 1500 tiny inputs of test_lzp_tiny_and_boundary_sizes, with hashSize drawn from what the stage takes"""
    rng = np.random.default_rng(11)
    for it in range(1500):
        n = int(rng.integers(1, 300))
        T = [np.zeros(n, np.uint8), (rng.integers(0, 2, n) * 0xF2).astype(np.uint8),
             np.tile(rng.integers(0, 256, int(rng.integers(1, 7)), dtype=np.uint8), n)[:n].copy()][it % 3]
        yield T, int(rng.choice([10, 14, 15])), int(rng.choice(MINLENS)), int(rng.choice([0, 3]))


_WANT = {}


def want(key, T, h, m, f):
    """api.bsc_lzp_compress(T, h, m, f), computed once per (key, h, m, f)"""
    k = (key, h, m, f)
    if k not in _WANT:
        _WANT[k] = api.bsc_lzp_compress(T, h, m, features=f)
    return _WANT[k]
