"""Inputs of the adaptive coder's batch model tests (CPU and GPU), on top of model_batch_inputs.py: the CPU stand-in's streams of a layout
(bscgpu_adaptive_pstream_host) with its debug planes, the passes that reach what only this coder has — run_hist above the static
model's clamp of 7, the escape mixers, alphabets too small for an exponent chain — and a numpy restatement of which mixer instance a
decision uses.

No pass built here may be declined by the device unless its name says so."""
import functools

import numpy as np

import fast_batch_inputs as fbi
import model_batch_inputs as mb
from front_inputs import KI, runs_block

CTX_N = fbi.CTX_N                                              # the GPU tests' module context
PS_BIT, PS_RUN = 1 << 12, 1 << 13                              # devcoder_model.h: the BSCGPU_RC_STATIC16 entry
# devcoder_model.h: mixer ids in the order of the reference's member arrays
MIX_RF, MIX_RE, MIX_RM, MIX_RP, MIX_NF, MIX_NE, MIX_NM, NUM_MIX = 0, 256, 320, 328, 584, 840, 1864, 1896
PLANES = ("state counter", "char counter", "static counter", "mixer id")


def host_streams(fb, dbg=False):
    """the CPU stand-in's adaptive stream of every sub-block -> (entries back to back, poff[nsub + 1]); dbg: and the four debug planes
    np.uint16[4][D]"""
    from libbsc_amd.gpu import adaptive_pstream_host
    parts = [adaptive_pstream_host(fb, s, dbg=True) for s in range(fb.nsub)]
    poff = np.concatenate([[0], np.cumsum([p[0].size for p in parts])]).astype(np.uint32)
    ps = np.concatenate([p[0] for p in parts]) if parts else np.zeros(0, np.uint16)
    if not dbg:
        return ps, poff
    return ps, poff, (np.concatenate([p[1] for p in parts], axis=1) if parts else np.zeros((4, 0), np.uint16))


def _runs(rng, symbols, lo, hi, n, spacer=None):
    """n bytes: runs of the symbols in turn, lengths uniform in [lo, hi], a single byte of `spacer` between two runs"""
    out, size, i = [], 0, 0
    while size < n:
        k = int(rng.integers(lo, hi + 1))
        out.append(np.full(k, symbols[i % len(symbols)], np.uint8))
        size += k
        if spacer is not None:
            out.append(np.full(1, spacer, np.uint8))
            size += 1
        i += 1
    return np.concatenate(out)[:n].copy()


def hist_above_clamp_pass():
    """a 300 KiB block of two symbols in runs of 2^10 .. 2^12 bytes with single bytes of a third symbol between them: run_hist of the two
    settles at 11 - 12, above the 7 the static model's state index is clamped to; and a twin with runs of 2^7 bytes (run_hist 6 - 7)"""
    rng = np.random.default_rng(61)
    return [_runs(rng, (20, 30), 1 << 10, 1 << 12, 300 * KI, spacer=40), _runs(rng, (20, 30), 1 << 7, 1 << 7, 300 * KI, spacer=40)]


def escape_pass():
    """64 KiB of uniform bytes over 256 symbols (avg_rank >= 32 from the first few runs on: the escape mixers), and text followed by
    noise followed by text, which crosses the threshold both ways"""
    rng = np.random.default_rng(62)
    mixed = np.concatenate([runs_block(rng, 40 * KI, 20, mean_run=4.0), rng.integers(0, 256, 24 * KI, dtype=np.uint8),
                            runs_block(rng, 40 * KI, 20, mean_run=4.0)])
    return [rng.integers(0, 256, 64 * KI, dtype=np.uint8), mixed]


def tiny_alphabets():
    """blocks of 1, 2, 3 and 5 symbols in sizes 1, 2, 29 and 4 KiB: max_rank 0 .. 2, empty exponent chains"""
    rng = np.random.default_rng(63)
    return [runs_block(rng, n, k, mean_run=2.0) for k in (1, 2, 3, 5) for n in (1, 2, 29, 4 * KI)]


PASSES = dict(mixed=lambda: mb.mixed_batch(0), pass_of_4096=mb.pass_of_4096, chain_identity=mb.chain_identity_pass,
              hist_above_clamp=hist_above_clamp_pass, escape=escape_pass, tiny_alphabets=tiny_alphabets, fill=mb.fill_pass)
# decisions the device model holds per context (four per byte of max_n), by the pass that runs in it
CAPACITY = {name: 4 * (2 * fbi.MIB if name == "fill" else CTX_N) for name in PASSES}


@functools.lru_cache(maxsize=None)
def reference(name):
    """(blocks, layout, stand-in entries, poff, debug planes) of a pass: computed once, shared by the tests, never written to"""
    blocks = PASSES[name]()
    fb, _ = mb.layout(blocks)
    ps, poff, dbg = host_streams(fb, dbg=True)
    for a in (ps, poff, dbg):
        a.setflags(write=False)
    return blocks, fb, ps, poff, dbg


def _bsr(x):
    return np.where(x > 0, np.floor(np.log2(np.maximum(x, 1))).astype(np.int64), 0)


def mixer_ids(fb, s):
    """the mixer id of every decision of sub-block s, from the run arrays alone (the table of devcoder_model.h, restated):
    RF rank[c] | RE rank_exp[max(hist, b)][b] | RM rank_mant[B] | RP rank_esc[node] | NF run[c] | NE run_exp[max(hist, b)][b], hist
    not clamped | NM run_mant[bits]"""
    r0, r1 = int(fb.sub_run[s]), int(fb.sub_run[s + 1])
    sym = fb.sym[r0:r1].astype(np.int64)
    rank = fb.rank[r0:r1].astype(np.int64)
    start = fb.start[r0:r1].astype(np.int64)
    end = int(fb.sub_start[s]) + int(fb.sub_size[s])
    run = np.diff(np.concatenate([start, [end]]))
    nsym = int(fb.nsym[s])
    max_rank = int(_bsr(np.array([nsym - 1]))[0]) if nsym > 1 else 0
    ids = []
    avg, rank_hist, run_hist = 0, [0] * 256, [0] * 256
    for c, rk, rn in zip(sym.tolist(), rank.tolist(), run.tolist()):
        h = rank_hist[c]
        if avg < 32:
            ids.append(MIX_RF + c)
            if rk != 1:
                B = rk.bit_length() - 1
                for b in range(1, B):
                    ids.append(MIX_RE + max(h, b) * 8 + b)
                if B < max_rank:
                    ids.append(MIX_RE + max(h, B) * 8 + B)
                ids += [MIX_RM + B] * B
            rank_hist[c] = 0 if rk == 1 else rk.bit_length() - 1
        else:
            ctx = 1
            for b in range(max_rank, -1, -1):
                ids.append(MIX_RP + ctx)
                ctx += ctx + ((rk >> b) & 1)
            rank_hist[c] = rk.bit_length() - 1
        avg = (avg * 124 + rk * 4) >> 7
        h = run_hist[c]
        ids.append(MIX_NF + c)
        if rn == 1:
            run_hist[c] = (h + 2) >> 2
        else:
            bits = rn.bit_length() - 1
            run_hist[c] = (h + 3 * bits + 3) >> 2
            for b in range(1, bits + 1):
                ids.append(MIX_NE + max(h, b) * 32 + b)
            ids += [MIX_NM + bits] * bits
    return np.array(ids, np.uint16)


# the construction's own claim, checked where it is made (CPU only): the stand-in's mixer ids of hist_above_clamp_pass contain
# run_exp[h][b] with h above the static model's clamp
def run_exp_rows(dbg_ids):
    ne = dbg_ids[(dbg_ids >= MIX_NE) & (dbg_ids < MIX_NM)].astype(np.int64) - MIX_NE
    return np.unique(ne // 32)


def first_difference(ps, want_ps, want_poff, dbg=None, want_dbg=None):
    """the message of a stream mismatch: the first differing entry, its sub-block and — with both sets of debug planes — whether a
    counter value, the mixer id or only the mixed probability differs first"""
    w = np.flatnonzero(ps != want_ps)
    if not w.size:
        return None
    i = int(w[0])
    s = int(np.searchsorted(want_poff, i, side="right")) - 1
    msg = (f"{w.size} of {ps.size} entries differ, first at {i} (sub-block {s}, its decision {i - int(want_poff[s])}): "
           f"{int(ps[i]):#x} != {int(want_ps[i]):#x}")
    if dbg is not None and want_dbg is not None:
        firsts = [(int(np.flatnonzero(dbg[p] != want_dbg[p])[0]), PLANES[p]) for p in range(4) if (dbg[p] != want_dbg[p]).any()]
        if firsts and min(firsts)[0] <= i:
            at, what = min(firsts)
            msg += f"; the {what} differs first, at {at}: {int(dbg[PLANES.index(what)][at])} != {int(want_dbg[PLANES.index(what)][at])}"
        else:
            msg += "; counter values and mixer ids agree up to there: the mixed probability differs first"
    return msg
