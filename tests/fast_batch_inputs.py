"""Inputs of the fast coder's batch model tests (CPU and GPU), on top of model_batch_inputs.py: the CPU stand-in's streams of a layout
(bscgpu_fast_pstream_host) and the one pass the device must decline — for capacity, the only exit a pass of ordinary data can take
with this coder (it has no avg_rank flags and no run_hist look-back)."""
import numpy as np

from front_inputs import KI

PSF_BIT, PSF_RUN, PSF_SIDE = 1 << 13, 1 << 14, 1 << 15        # devcoder_model.h: the BSCGPU_RC_FAST16 entry
MIB = 1 << 20
CTX_N = (16 << 20) + 4096                                      # the GPU tests' module context
# decisions the device model holds per context (devcoder_ensure: four per byte of max_n), by the pass that runs in it
CAPACITY = dict(mixed=4 * CTX_N, pass_of_4096=4 * CTX_N, chain_identity=4 * CTX_N, long_chain=4 * CTX_N, fill=4 * 2 * MIB)


def host_streams(fb):
    """the CPU stand-in's fast stream of every sub-block -> (entries back to back, poff[nsub + 1])"""
    from libbsc_amd.gpu import fast_pstream_host
    parts = [fast_pstream_host(fb, s) for s in range(fb.nsub)]
    poff = np.concatenate([[0], np.cumsum([p.size for p in parts])]).astype(np.uint32)
    return (np.concatenate(parts) if parts else np.zeros(0, np.uint16)), poff


def noise_pass():
    """two 700 KiB blocks of uniform random bytes: rank and run side together come to more than ten decisions per byte, against the four
    per byte of max_n that a 2 MiB context holds"""
    rng = np.random.default_rng(51)
    return [rng.integers(0, 256, 700 * KI, dtype=np.uint8) for _ in range(2)]


# ---- must a pass replay an evaluation chunk?  A CPU walk of the device's brackets ------------------------------------------------------
# The device walks a chain (sub-block, decision type, symbol) in chunks of DC_EV events; a chunk that begins inside a chain starts from
# the two ends of the counter's attainable range and the next chunk takes its end value if the two ends met, else the chunk is walked
# again serially from a known value (a replay).  The fast coder's update is v += ceil((target_bit - v) / 2^R).  Under a constant bit
# both ends land on the same value.  Under strictly alternating bits the two ends settle into two different orbits a few units apart
# and never meet, however long the chunk.  The chain looked for here is the first rank decision ("rank != 1") of a symbol whose ranks
# alternate between 1 and another value (bit 0, 1, 0, 1, ...): class RF, targets 8016 / 83, shift 4, start value 4096.
DC_EV = 8192                                                   # devcoder_model.h (passes of up to 8192 * 64000 events)
RF_T0, RF_T1, RF_SHIFT, RANK_INIT = 8016, 83, 4, 4096         # devcoder_model.h: model_params_fast


def _step(v, bit, t0=RF_T0, t1=RF_T1, shift=RF_SHIFT):
    return v + (((t1 if bit else t0) - v + (1 << shift) - 1) >> shift)


def _closure(init):
    lo = hi = init
    grown = True
    while grown:
        grown = False
        for s in range(lo, hi + 1):
            for b in (0, 1):
                w = _step(s, b)
                if w < lo or w > hi:
                    lo, hi, grown = min(lo, w), max(hi, w), True
    return lo, hi


def bracket_stays_open_under_alternating_bits():
    """the ends of the RF bracket after DC_EV alternating bits, for both phases: True if they never met"""
    vmin, vmax = _closure(RANK_INIT)
    for phase in (0, 1):
        lo, hi = vmin, vmax
        for i in range(DC_EV):
            lo, hi = _step(lo, (i + phase) & 1), _step(hi, (i + phase) & 1)
            if lo == hi:
                return False
    return True


def alternating_rank_first_chains(fb):
    """lengths of the chains (sub-block, RF, symbol) of a layout whose bits alternate strictly"""
    out = []
    for s in range(fb.nsub):
        r0, r1 = int(fb.sub_run[s]), int(fb.sub_run[s + 1])
        sym, rank = fb.sym[r0:r1], fb.rank[r0:r1]
        for c in np.unique(sym):
            r = rank[sym == c] != 1
            if r.size >= 2 and (r[1:] != r[:-1]).all():
                out.append(int(r.size))
    return out


def replay_must_happen(fb):
    """a chain of >= 3 DC_EV events holds a whole chunk and the start of the next one, wherever the chunk boundaries fall: if that
    chunk's bracket cannot close, the next chunk is replayed.  (It must also stay below the replay limit of 64 chunks.)"""
    chains = alternating_rank_first_chains(fb)
    long_enough = [n for n in chains if n >= 3 * DC_EV]
    assert all(n < 60 * DC_EV for n in chains), "a chain beyond the replay limit: the device would decline the pass"
    return bool(long_enough) and bracket_stays_open_under_alternating_bits()
