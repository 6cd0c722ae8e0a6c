"""Inputs of the tests of the adaptive coder's model (-e2) in segments (CPU and GPU), on top of adaptive_batch_inputs.py and
model_segment_inputs.py: the named passes with the CPU stand-in's streams (bscgpu_adaptive_pstream_host) and its third fact — the
longest mixer chain of every sub-block (bscgpu_adaptive_longest_chain_host) — and the pass whose blocks lie on both sides of the step
cap.

No pass built here may be declined by the device unless its name says so."""
import functools

import numpy as np

import adaptive_batch_inputs as ab
import model_batch_inputs as mb
import model_segment_inputs as ms

ADAPTIVE = 2                                                   # LIBBSC_CODER_QLFC_ADAPTIVE
MIX_CAP_DEFAULT = 1 << 18                                      # dev_common.h: DC_MIX_CHAIN_CAP
# A step cap between the block maxima of cap_sides_pass(): counted on the CPU (test_adaptive_segments_host.py), the blocks' longest
# chains are 283 948 / 476 792 / 791 884 above the default cap and 235 844 at most below it; this one bars two of the three.
MIX_CAP_BETWEEN = 400_000


def cap_sides_pass():
    """model_batch_inputs.whole_call_cases(101) taken as L (unsorted text: long chains): blocks on both sides of the step cap, an empty
    block and blocks of <= 28 bytes among them"""
    return mb.whole_call_cases(mb.WHOLE_SEEDS['host', 1])


PASSES = dict(over_capacity=ms.over_capacity_pass, mixed=lambda: mb.mixed_batch(0), pass_of_4096=mb.pass_of_4096,
              chain_identity=mb.chain_identity_pass, hist_above_clamp=ab.hist_above_clamp_pass, escape=ab.escape_pass,
              tiny_alphabets=ab.tiny_alphabets, cap_sides=cap_sides_pass)


def longest_chains(fb):
    """the stand-in's longest mixer chain of every sub-block of a layout"""
    from libbsc_amd.gpu import adaptive_longest_chain_host
    return np.array([adaptive_longest_chain_host(fb, s) for s in range(fb.nsub)], np.int64)


def block_max(fb, per_sub):
    """the maximum over every block's sub-blocks (0 for a block without any)"""
    return np.array([int(per_sub[fb.blk_sub[b]:fb.blk_sub[b + 1]].max()) if fb.blk_sub[b + 1] > fb.blk_sub[b] else 0 for b in range(fb.count)], np.int64)


@functools.lru_cache(maxsize=None)
def reference(name):
    """(blocks, layout, the pass's bytes, the stand-in's entries, its poff, the longest chain of every sub-block) of a named pass —
    computed once per process and shared; nobody writes to any of it"""
    blocks = PASSES[name]()
    fb, flat = mb.layout(blocks)
    ps, poff = ab.host_streams(fb)
    mix = longest_chains(fb)
    for a in (flat, ps, poff, mix):
        a.setflags(write=False)
    return blocks, fb, flat, ps, poff, mix


def three_pass_cases():
    """the call of three passes in the 2 MiB context (test_gpu_model_segments.py's): two texts of 700 KiB to a pass with blocks of 0, 1,
    20 and 29 bytes between them; sorted, every block's longest chain is under the default cap (counted on the CPU: 208 520 at most)"""
    from front_inputs import KI
    from libbsc_amd.synth import synth_text_v1
    return [synth_text_v1(90 + i, n) for i, n in enumerate([700 * KI, 20, 700 * KI, 0, 700 * KI, 29, 700 * KI, 700 * KI, 1, 700 * KI])]
