"""Inputs of the packed batch stream's tests (CPU and GPU), on top of model_batch_inputs.py / front_inputs.py: a pass whose sub-block
boundaries fall where the packed writer's cases are (boundary_pass), a pass whose packed form is void (void_pass), the packed
reference of a layout, and the numbers the CPU test proves about them before any GPU sees them."""
import functools

import numpy as np

import model_batch_inputs as mb
from front_inputs import KI, runs_block

WAVE_RUNS, WG_RUNS = 64, 256                           # runs a wavefront / a workgroup of dc_pstream_kernel holds (thread per run)
DC_PS_STAGE = 1792                                     # decisions a wavefront stages (devcoder.hip); a piece above it voids the packed form


def _alternating(nruns, a=5, b=9):
    """nruns runs of one byte each"""
    return np.where(np.arange(nruns) % 2 == 0, a, b).astype(np.uint8)


def boundary_pass():
    """A text-like block of 300 KiB, then blocks of 1 .. ~400 bytes: a filler that brings the run index to a multiple of the
    workgroup's 256 runs, a block of 64 runs (the next one starts at a multiple of 64 that is none of 256), a stretch of sixty blocks
    of 1 .. 3 bytes (dozens of sub-blocks inside one wavefront's 64 runs), single-run blocks of every length 1 .. 40, about 250 blocks
    of random sizes and alphabets, and a second text-like block of 300 KiB.  Alphabets stay at or below 32 symbols except in the two
    text blocks: no avg_rank flag can be left undecided by the small ones."""
    rng = np.random.default_rng(77)
    head = runs_block(rng, 300 * KI, 33, mean_run=4.0)
    fb, _ = mb.layout([head])
    blocks = [head, _alternating((-fb.m) % WG_RUNS or WG_RUNS), _alternating(WAVE_RUNS, 3, 4)]
    for i in range(60):
        n = 1 + i % 3
        blocks.append(runs_block(rng, n, 2, mean_run=1.2) if i % 4 else np.full(n, 10 + i, np.uint8))
    blocks += [np.full(n, 100 + n, np.uint8) for n in range(1, 41)]
    for i in range(250):
        n = int(rng.integers(1, 401))
        blocks.append(runs_block(rng, n, int(rng.integers(1, 25)), mean_run=float(rng.choice([1.3, 2.5, 6.0, 40.0]))))
    blocks.append(runs_block(rng, 300 * KI + 17, 40, mean_run=3.0))
    return blocks


def long_runs_block(nbytes=1000 * KI):
    """"runs of thousands" over six symbols, under 1 MiB: at 6000 .. 8190 bytes a run takes about 30 decisions, so the 64 runs of a
    wavefront hold more than it stages (1792) and the packed form of whatever holds this sorted block is void.  (At 2000 .. 9000
    bytes the average is 27.8 decisions a run, 1778 per wavefront: under 1 MiB there are too few wavefronts for one to be over.)"""
    rng = np.random.default_rng(1)
    a = np.repeat(rng.integers(0, 6, 200, dtype=np.uint8), rng.integers(6000, 8191, 200)).astype(np.uint8)
    assert a.size >= nbytes
    return a[:nbytes].copy()


def void_text():
    """the whole calls' void case, a TEXT whose transform is "runs of thousands": a word of 100 symbols over six, repeated to 1000 KiB.
    Every rotation class of the word is one run of about 10 240 bytes in the BWT (and in ST5: the word's 5-byte contexts are all
    different), about 30 decisions each, so the block's first 64 runs overflow a wavefront's staging buffer when the block comes
    first in its pass.  (long_runs_block() itself cannot serve as a text: the transforms break its runs up — 234 runs, at most 865
    decisions per wavefront under the BWT, 992 under ST5 — and the packed form of such a pass is not void.)"""
    rng = np.random.default_rng(5)
    return np.tile(rng.integers(0, 6, 100, dtype=np.uint8), 10300)[:1000 * KI].copy()


def void_pass():
    rng = np.random.default_rng(78)
    return [runs_block(rng, 100 * KI, 33), long_runs_block(), runs_block(rng, 64 * KI, 17)]


def run_decisions(fb, ps, poff):
    """decisions of every run of the pass, from the stand-in's run-start marks (bit 13 of a 16-bit entry)"""
    heads = np.flatnonzero(ps & (1 << 13))
    assert heads.size == fb.m
    return np.diff(np.concatenate([heads, [int(poff[-1])]]))


def max_wave_decisions(fb, ps, poff):
    """the most decisions any wavefront's 64 runs hold (wavefront w: runs 64 w .. 64 w + 63 of the pass)"""
    nd = run_decisions(fb, ps, poff)
    pad = (-nd.size) % WAVE_RUNS
    return int(np.concatenate([nd, np.zeros(pad, nd.dtype)]).reshape(-1, WAVE_RUNS).sum(axis=1).max())


def pbase_rule(poff):
    """the layout's rule, restated: pbase[0] = 0, pbase[s + 1] = pbase[s] + roundup64(poff[s + 1] - poff[s])"""
    lens = np.diff(np.asarray(poff, np.int64))
    return np.concatenate([[0], np.cumsum((lens + 63) // 64 * 64)]).astype(np.int64)


PASSES = dict(boundary=boundary_pass, void=void_pass, mixed=lambda: mb.mixed_batch(0), pass_of_4096=mb.pass_of_4096,
              chain_identity=mb.chain_identity_pass, fill=mb.fill_pass, long_chain=mb.long_chain_pass,
              raw_second=lambda: [mb.raw_second_sub_block()])


@functools.lru_cache(maxsize=None)
def reference(name):
    """(blocks, layout, the pass's bytes, the stand-in's 16-bit entries, poff, their packed form, pbase) of a named pass — computed once
    per process and shared; nobody writes to any of it"""
    from libbsc_amd.gpu import pstream_pack13_host
    blocks = PASSES[name]()
    fb, flat = mb.layout(blocks)
    ps, poff = mb.host_streams(fb)
    packed, pbase = pstream_pack13_host(ps, poff)
    for a in (flat, ps, poff, packed, pbase):
        a.setflags(write=False)
    return blocks, fb, flat, ps, poff, packed, pbase


def expected_packed(fb, want_ps, want_poff, state):
    """what the segmented packed stage must deliver when it kept the blocks with state 0: (bytes, poff, pbase), a sub-block that was
    not modelled empty in both offset tables"""
    import model_segment_inputs as ms
    from libbsc_amd.gpu import pstream_pack13_host
    e_ps, e_poff = ms.expected(fb, want_ps, want_poff, state)
    packed, pbase = pstream_pack13_host(e_ps, e_poff)
    return packed, e_poff, pbase
