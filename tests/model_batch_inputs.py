"""Inputs of the batch model's tests (CPU and GPU): passes of "sorted blocks" for the static coder's model over a sub-block table
(bscgpu_static_pstream_batch_device and its CPU stand-in).  Reuses front_inputs.py and devcoder_inputs.py.

No pass built here may be declined by the device unless its name says so; avg_undecided() restates, in numpy, the one exit that
depends on where a pass's run index space is cut into lanes (dc_avg_kernel's two-sided bracket) so that the CPU tests can check
that before any GPU sees the inputs."""
import numpy as np

import devcoder_inputs as di
from front_inputs import KI, mixed_batch, raw_second_sub_block, runs_block  # noqa: F401  (re-exported)

DC_AVG_CH, DC_AVG_WARM = 1024, 768                     # devcoder_model.h


def layout(blocks):
    """(FrontBatch built on the CPU, the pass's bytes)"""
    from libbsc_amd.gpu import front_batch_host
    sizes = [b.size for b in blocks]
    flat = np.concatenate(blocks) if sum(sizes) else np.zeros(1, np.uint8)
    return front_batch_host(flat, sizes), flat


def sub_bytes(fb, blocks, s):
    """the bytes of sub-block s of the layout of `blocks`"""
    b = int(np.searchsorted(fb.blk_sub, s, side="right")) - 1
    st, sz = int(fb.sub_start[s]), int(fb.sub_size[s])
    return blocks[b][st:st + sz]


def host_streams(fb):
    """the CPU stand-in's stream of every sub-block -> (entries back to back, poff[nsub + 1])"""
    from libbsc_amd.gpu import static_pstream_host
    parts = [static_pstream_host(fb, s) for s in range(fb.nsub)]
    poff = np.concatenate([[0], np.cumsum([p.size for p in parts])]).astype(np.uint32)
    return (np.concatenate(parts) if parts else np.zeros(0, np.uint16)), poff


def avg_undecided(fb):
    """runs whose avg_rank >= 32 flag the device's bracket would leave open: lanes of DC_AVG_CH runs of the pass's run index space,
    warmed up over DC_AVG_WARM runs (or from the sub-block's first run, then exact), upper end started at 2^(max_rank + 1) - 1,
    both ends reset at every sub-block start.  All lanes advance together, one run per step."""
    m = fb.m
    if m == 0:
        return 0
    rank = fb.rank.astype(np.int64)
    sub_run = fb.sub_run.astype(np.int64)
    is_first = np.zeros(m + 1, bool)
    is_first[sub_run[:-1]] = True
    top = (2 << np.array([max(int(n) - 1, 0).bit_length() - 1 if n > 1 else 0 for n in fb.nsym], np.int64)) - 1
    j0 = np.arange(0, m, DC_AVG_CH, dtype=np.int64)
    sb = np.searchsorted(sub_run, j0, side="right") - 1
    first = sub_run[sb]
    w0 = np.where(j0 > first + DC_AVG_WARM, j0 - DC_AVG_WARM, first)
    lo = np.zeros(j0.size, np.int64)
    hi = np.where(w0 == first, 0, top[sb])
    und = 0
    for t in range(DC_AVG_WARM + DC_AVG_CH):
        j = w0 + t
        live = j < np.minimum(j0 + DC_AVG_CH, m)
        jj = np.minimum(j, m - 1)
        counted = live & (j >= j0)
        reset = counted & is_first[jj] & (j > w0)
        lo = np.where(reset, 0, lo)
        hi = np.where(reset, 0, hi)
        und += int(np.count_nonzero(counted & ((lo >= 32) != (hi >= 32))))
        r = rank[jj]
        lo = np.where(live, (lo * 124 + r * 4) >> 7, lo)
        hi = np.where(live, (hi * 124 + r * 4) >> 7, hi)
    return und


def pass_of_4096():
    """the construction of test_gpu_batch_front.test_stage_pass_of_4096_blocks: 4096 blocks of 0..3000 bytes with a few of 300 KiB among
    them — sub-block starts inside every 64-run tile, every 1024-run avg lane and every evaluation chunk"""
    rng = np.random.default_rng(11)
    sizes = rng.integers(0, 3000, 4096)
    sizes[::512] = 300 * KI
    text = runs_block(rng, int(sizes.sum()), 40, mean_run=2.5)
    offs = np.concatenate([[0], np.cumsum(sizes)])
    return [text[offs[b]:offs[b + 1]] for b in range(4096)]


CHAIN_NINTH, CHAIN_LONG = (3, 11, 67, 131, 259), (3, 11, 67)


def chain_identity_pass():
    """300 blocks of 2 KiB over eight common symbols, one sub-block each (sub-block id = block index).  A ninth symbol appears, as
    about 50 short runs, only in blocks 3, 11, 67, 131 and 259, and one run of 5000 bytes only in blocks 3, 11 and 67 (those three
    are 5000 bytes longer): index gaps 8, 56, 64 and 128, so a sub-block id kept modulo 8, 64 or 128 walks two chains as one — the
    ninth symbol's in the char family, the long run's decision types in the context-free family."""
    rng = np.random.default_rng(21)
    blocks = []
    for b in range(300):
        a = runs_block(rng, 2 * KI, 8, mean_run=3.0)
        a = np.unique(a, return_inverse=True)[1].astype(np.uint8) + np.uint8(10)      # the same eight symbols (10..17) in every block
        if b in CHAIN_NINTH:
            at = np.sort(rng.choice(np.arange(10, 2 * KI - 10, 8), 50, replace=False))
            for p in at:
                a[p:p + int(rng.integers(1, 4))] = 99
        if b in CHAIN_LONG:
            a = np.concatenate([a[:1000], np.full(5000, 12, np.uint8), a[1000:]])
        blocks.append(a)
    return blocks


def long_chain_pass():
    """chains longer than one evaluation chunk inside batched blocks: 900 KiB blocks of devcoder_inputs.periodic (the context-free
    family's rank-first chain alternates with period two and its bracket stays open for the length of a sub-block: ~55 chunks of
    8192 events, under the replay limit of 64) next to text-like blocks"""
    rng = np.random.default_rng(31)
    n = 900 * KI
    return [runs_block(rng, 40 * KI, 33), di.periodic([0, 1, 0, 2], [1], n), runs_block(rng, 300 * KI, 65),
            di.periodic([0, 1, 0, 1, 2], [1], 300_000), runs_block(rng, 5000, 17)]


def fail_avg_pass():
    """one constant-rank-40 block among text-like ones: its avg_rank bracket never decides"""
    rng = np.random.default_rng(41)
    return [runs_block(rng, 100 * KI, 33), di.const_rank(40, 600_000), runs_block(rng, 64 * KI, 17)]


def fail_hist_pass():
    """one block with 40000 runs of length 2 of one symbol in one sub-block: more than 9216 same-class predecessors"""
    rng = np.random.default_rng(42)
    return [runs_block(rng, 100 * KI, 33), di.hist_chain(40000), runs_block(rng, 64 * KI, 17)]


FILL_SIZES = [700 * KI, 0, 700 * KI - 3, 2 * 1024 * KI - 1400 * KI + 3]      # test_stage_pass_that_fills_max_n: a 2 MiB context, exactly


def fill_pass():
    """text-like runs: about two decisions per byte, under the 2 MiB context's capacity of four (the front end's own test uses 70
    symbols in runs of 1.5 bytes: seven decisions per byte, a pass the model has to decline for capacity)"""
    rng = np.random.default_rng(12)
    return [runs_block(rng, n, 33, mean_run=5.0) for n in FILL_SIZES]


# seeds of the whole-call cases per (input kind, sorter).  The block of text followed by noise leaves one avg_rank flag undecided for
# about two seeds in five (where the noise begins the bracket's ends are a step apart as they cross 32), and the device then
# declines the pass: these seeds are the ones test_model_batch_host.py finds kept, for the BWT and for ST5.
WHOLE_SEEDS = {("host", 1): 101, ("host", 5): 105, ("device", 1): 201, ("device", 5): 215}


def whole_call_cases(seed):
    """inputs (texts, not sorted blocks) of the compress-batch tests: synthetic text of mixed sizes, two-sub-block sizes, text followed
    by noise, a 64 KiB noise block (stored), an empty block and blocks of <= 28 bytes.
    (front_inputs.raw_second_sub_block() is a SORTED block; given as a text, its BWT has no raw sub-block and leaves one or two
    avg_rank flags undecided, so the device would decline the pass: text followed by noise stands in for it, and the raw sub-block
    itself is covered by test_model_batch_host.py, which codes the sorted block from its streams.)"""
    from libbsc_amd.synth import synth_text_v1
    rng = np.random.default_rng(seed)
    cases = [synth_text_v1(61 + i, int(n)) for i, n in enumerate(rng.integers(1000, 200000, 6))]
    cases += [synth_text_v1(71, 300 * KI), synth_text_v1(72, 1024 * KI - 1)]
    cases += [np.concatenate([synth_text_v1(73, 500 * KI), rng.integers(0, 256, 120 * KI, dtype=np.uint8)]),
              rng.integers(0, 256, 64 * KI, dtype=np.uint8), np.zeros(0, np.uint8),
              np.frombuffer(bytes(range(40)), np.uint8)[:20].copy(), np.frombuffer(bytes(range(40)), np.uint8)[:28].copy()]
    return cases
