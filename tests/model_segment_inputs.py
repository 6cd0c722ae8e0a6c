"""Inputs of the model segments' tests (CPU and GPU), on top of model_batch_inputs.py and fast_batch_inputs.py: the pass that is over the
small context's capacity as a whole while each of its blocks is under it, the stand-ins' per-sub-block decision counts and streams
for either coder, and what a segmented stage must deliver given which blocks it kept."""
import ctypes as C
import functools

import numpy as np

import fast_batch_inputs as fbi
import model_batch_inputs as mb
from front_inputs import KI, runs_block

MIB = 1 << 20
SMALL_CTX_N = 2 * MIB
# Decisions the device model holds in a context of SMALL_CTX_N bytes.  The CPU tests check the inputs' preconditions against this
# number; test_gpu_model_segments.py asserts that the context itself reports it (BSCGPU_CNT_DC_DCAP).
SMALL_CTX_DCAP = 8470528
STATIC, FAST = 1, 3                                            # LIBBSC_CODER_QLFC_STATIC, LIBBSC_CODER_QLFC_FAST


def over_capacity_pass():
    """32 blocks of 64 KiB over 70 symbols in runs of 1.5 bytes (the mix test_gpu_batch_front.py calls "seven decisions per byte"): 2 MiB,
    the small context exactly, at about 4.5 decisions per byte against the four its model holds"""
    rng = np.random.default_rng(71)
    return [runs_block(rng, 64 * KI, 70, mean_run=1.5) for _ in range(32)]


def noise_under_capacity_pass():
    """two 500 KiB blocks of uniform random bytes: about 13.8 decisions per byte with the fast coder, so each block alone is under the
    small context's capacity and the two together are over it.  (fast_batch_inputs.noise_pass(), two blocks of 700 KiB, is over it
    block by block — 9 685 312 and 9 686 356 decisions against 8 470 528 — and a segmented stage can only leave both to the host.)"""
    rng = np.random.default_rng(52)
    return [rng.integers(0, 256, 500 * KI, dtype=np.uint8) for _ in range(2)]


def sub_counts(fb, coder):
    """the stand-in's number of decisions of every sub-block of a layout (cap 0: counted, nothing written)"""
    from libbsc_amd import _native as N
    f = N.lib().bscgpu_fast_pstream_host if coder == FAST else N.lib().bscgpu_static_pstream_host
    out = np.array([int(f(C.byref(fb.lay), s, None, 0)) for s in range(fb.nsub)], np.int64)
    assert (out >= 0).all()
    return out


def block_counts(fb, counts):
    """decisions of every block: the sum over its sub-blocks"""
    return np.array([int(counts[fb.blk_sub[b]:fb.blk_sub[b + 1]].sum()) for b in range(fb.count)], np.int64)


@functools.lru_cache(maxsize=None)
def reference(name, coder):
    """(blocks, layout, the pass's bytes, the stand-in's entries, its poff) of a named pass — computed once per process and shared;
    nobody writes to any of it"""
    blocks = PASSES[name]()
    fb, flat = mb.layout(blocks)
    ps, poff = (fbi.host_streams if coder == FAST else mb.host_streams)(fb)
    for a in (flat, ps, poff):
        a.setflags(write=False)
    return blocks, fb, flat, ps, poff


PASSES = dict(over_capacity=over_capacity_pass, noise=fbi.noise_pass, noise_under=noise_under_capacity_pass, mixed=lambda: mb.mixed_batch(0), pass_of_4096=mb.pass_of_4096,
              chain_identity=mb.chain_identity_pass, long_chain=mb.long_chain_pass, fail_avg=mb.fail_avg_pass, fail_hist=mb.fail_hist_pass)


def expected(fb, want_ps, want_poff, state):
    """what the segmented stage must deliver when it kept the blocks with state 0: (entries of the kept sub-blocks back to back in
    sub-block order, poff with an empty range for every sub-block that was not modelled)"""
    keep = np.zeros(fb.nsub, bool)
    for b in range(fb.count):
        if state[b] == 0:
            keep[fb.blk_sub[b]:fb.blk_sub[b + 1]] = True
    lens = np.where(keep, np.diff(want_poff.astype(np.int64)), 0)
    poff = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)
    parts = [want_ps[int(want_poff[s]):int(want_poff[s + 1])] for s in range(fb.nsub) if keep[s]]
    return (np.concatenate(parts) if parts else np.zeros(0, np.uint16)), poff
