// dc_block_plan.h — the device model of a single block as plain host arithmetic without any HIP in it.  A block modelled in segments of
// whole sub-blocks (devcoder.hip: devcoder_block_begin / _segment; DESIGN §3.6, "A block in sub-block segments"): where the block is cut
// so that every segment fits the arena's capacity in runs and in decisions, the eight-entry run table of a segment rebased to its first
// run.  Where a sub-block's piece of the probability stream lies in the device buffer and lands in the block's one landing zone — of a
// block in segments and of one modelled in one go (DcBlockSchedule::whole) alike: block.cpp's sender copies by it and fills the job's
// poff / pbase from it, the stage functions of devcoder.hip lay their output out by it.  max_rank of a sub-block from its symbol count,
// and what the driver of one block (block.cpp: gpu_stage) decides.  tools/block_plan_probe.cpp reads the same from stdin, for
// tests/test_block_segment_plan_host.py.
#pragma once
#include <stdint.h>
#include "dc_segment_plan.h"                                            // the packed layout: dc_pack13_fields / dc_pack13_bytes

enum { DC_BLOCK_MAX_SUB = 8, DC_BLOCK_BAD_PARAMETER = -1 /* LIBBSC_BAD_PARAMETER */, DC_BLOCK_NOT_SUPPORTED = -4 /* LIBBSC_NOT_SUPPORTED */ };

// ---- the plan ------------------------------------------------------------------------------------------------------------------------
// Sub-blocks in order, sub_runs[s] runs and sub_dec[s] decisions each.  Consecutive sub-blocks join a segment while the runs stay within
// mcap and the decisions within dcap: greedy, which for contiguous ranges is the fewest segments (a cut that comes earlier than the
// greedy one never lets a later one come later).  seg_of[s]: the segment of sub-block s.  -> the number of segments;
// DC_BLOCK_NOT_SUPPORTED: a sub-block alone exceeds a capacity; DC_BLOCK_BAD_PARAMETER: a null pointer, nsub outside 1..8, a capacity
// <= 0 — nothing is written in either case.
static inline int dc_block_segment_plan(const uint32_t* sub_runs, const uint32_t* sub_dec, int nsub, int64_t mcap, int64_t dcap, int* seg_of)
{
    if (!sub_runs || !sub_dec || !seg_of || nsub < 1 || nsub > DC_BLOCK_MAX_SUB || mcap <= 0 || dcap <= 0) return DC_BLOCK_BAD_PARAMETER;
    for (int s = 0; s < nsub; ++s) if ((int64_t)sub_runs[s] > mcap || (int64_t)sub_dec[s] > dcap) return DC_BLOCK_NOT_SUPPORTED;
    int nseg = 0;
    int64_t runs = 0, dec = 0;
    for (int s = 0; s < nsub; ++s) {
        if (s == 0 || runs + sub_runs[s] > mcap || dec + sub_dec[s] > dcap) { ++nseg; runs = dec = 0; }
        runs += sub_runs[s]; dec += sub_dec[s];
        seg_of[s] = nseg - 1;
    }
    return nseg;
}

// ---- the schedule of a block ---------------------------------------------------------------------------------------------------------
// One segment: sub-blocks [s0, s1), runs [r0, r1) of the block, the decisions it must come to, its run table in the eight-entry form
// (first[b] relative to r0; first[s1 - s0 ..] = r1 - r0) and, per sub-block i of it, the bytes of its piece: at src[i] of the segment's
// device stream, at dst[i] of the landing zone, len[i] long (16-bit entries, or the groups of the packed form that hold a decision).
struct DcBlockSeg {
    int s0, s1;
    uint32_t r0, r1;
    int64_t expect;
    uint32_t first[DC_BLOCK_MAX_SUB + 1];
    int64_t src[DC_BLOCK_MAX_SUB], dst[DC_BLOCK_MAX_SUB], len[DC_BLOCK_MAX_SUB];
};

// Constructed from the facts of a block: run_first[0..nsub] (the sub-blocks' first runs, run_first[nsub] = m), dec[s] decisions of
// sub-block s.  packed: the block's stream is the 13-bit form — sub-block s at field pbase[s], a multiple of 64, as dc_pack13_host lays
// it out; else 16-bit entries, sub-block s at entry poff[s].  A segment's device stream has the same layout relative to its first
// sub-block, so joining is one offset: poff[s] - poff[s0], pbase[s] - pbase[s0].
class DcBlockSchedule {
public:
    DcBlockSchedule() : nsub(0), packed(false) {}                      // no plan: segments() < 0
    DcBlockSchedule(const uint32_t* run_first, const uint32_t* dec, int nsub, int64_t mcap, int64_t dcap, bool packed) : nsub(nsub), packed(packed)
    {
        uint32_t runs[DC_BLOCK_MAX_SUB];
        const bool sane = run_first && dec && nsub >= 1 && nsub <= DC_BLOCK_MAX_SUB;
        for (int s = 0; sane && s < nsub; ++s) runs[s] = run_first[s + 1] - run_first[s];
        nseg = dc_block_segment_plan(sane ? runs : nullptr, dec, nsub, mcap, dcap, seg_of);
        if (nseg < 0) return;
        poff[0] = 0; pbase[0] = 0;
        for (int s = 0; s < nsub; ++s) {
            first[s] = run_first[s]; sub_dec[s] = dec[s];
            poff[s + 1] = poff[s] + dec[s];
            pbase[s + 1] = pbase[s] + dc_pack13_fields(dec[s]);
        }
        first[nsub] = run_first[nsub];
    }
    // A block that was modelled in one go, from the poff[0..nsub] the model returned: one segment with src == dst, capacities no question
    // (its run fields are zero: nothing launches by it).
    static DcBlockSchedule whole(const uint32_t* poff, int nsub, bool packed)
    {
        uint32_t no_runs[DC_BLOCK_MAX_SUB + 1] = {}, dec[DC_BLOCK_MAX_SUB] = {};
        for (int s = 0; poff && s < nsub && s < DC_BLOCK_MAX_SUB; ++s) dec[s] = poff[s + 1] - poff[s];
        return DcBlockSchedule(poff ? no_runs : nullptr, dec, nsub, INT64_MAX, INT64_MAX, packed);
    }

    // the number of segments, or why there is no plan (DC_BLOCK_NOT_SUPPORTED, DC_BLOCK_BAD_PARAMETER)
    int segments() const { return nseg; }
    int segment_of(int s) const { return seg_of[s]; }
    // decisions of the block, and the bytes its stream takes of the landing zone
    int64_t decisions() const { return poff[nsub]; }
    int64_t zone_bytes() const { return packed ? dc_pack13_bytes(pbase[nsub]) : 2 * poff[nsub]; }
    int64_t poff_of(int s) const { return poff[s]; }
    int64_t pbase_of(int s) const { return pbase[s]; }

    DcBlockSeg segment(int i) const
    {
        DcBlockSeg g = {};
        g.s0 = 0; while (seg_of[g.s0] != i) ++g.s0;
        g.s1 = g.s0; while (g.s1 < nsub && seg_of[g.s1] == i) ++g.s1;
        g.r0 = first[g.s0]; g.r1 = first[g.s1];
        g.expect = poff[g.s1] - poff[g.s0];
        for (int b = 0; b <= DC_BLOCK_MAX_SUB; ++b) g.first[b] = (g.s0 + b < g.s1 ? first[g.s0 + b] : g.r1) - g.r0;
        for (int s = g.s0; s < g.s1; ++s) {
            const int k = s - g.s0;
            if (packed) {
                g.src[k] = dc_pack13_bytes(pbase[s] - pbase[g.s0]); g.dst[k] = dc_pack13_bytes(pbase[s]);
                g.len[k] = ((int64_t)sub_dec[s] + 7) / 8 * 13;
            } else {
                g.src[k] = 2 * (poff[s] - poff[g.s0]); g.dst[k] = 2 * poff[s]; g.len[k] = 2 * (int64_t)sub_dec[s];
            }
        }
        return g;
    }
    // what the model of segment g says of its sub-blocks' offsets (pseg[0 .. s1 - s0], relative to the segment) against the facts
    bool agrees(const DcBlockSeg& g, const uint32_t* pseg) const
    {
        for (int s = g.s0; s <= g.s1; ++s) if ((int64_t)pseg[s - g.s0] != poff[s] - poff[g.s0]) return false;
        return true;
    }
    // a segment whose packed form was void: its 16-bit entries (g.expect of them, as the device left them) packed into place in the
    // landing zone by the CPU stand-in of the layout -> false: the layout is not the plan's
    bool pack_void(const DcBlockSeg& g, const uint16_t* entries, uint8_t* zone) const
    {
        uint32_t pseg[DC_BLOCK_MAX_SUB + 1]; int64_t pb[DC_BLOCK_MAX_SUB + 1];
        for (int s = g.s0; s <= g.s1; ++s) pseg[s - g.s0] = (uint32_t)(poff[s] - poff[g.s0]);
        const int64_t need = dc_pack13_bytes(pbase[g.s1] - pbase[g.s0]);
        return packed && dc_pack13_host(entries, pseg, g.s1 - g.s0, zone + dc_pack13_bytes(pbase[g.s0]), need, pb) == need;
    }

private:
    int nsub, nseg = DC_BLOCK_BAD_PARAMETER;
    bool packed;
    int seg_of[DC_BLOCK_MAX_SUB] = {};
    uint32_t first[DC_BLOCK_MAX_SUB + 1] = {}, sub_dec[DC_BLOCK_MAX_SUB] = {};
    int64_t poff[DC_BLOCK_MAX_SUB + 1] = {}, pbase[DC_BLOCK_MAX_SUB + 1] = {};
};

// ---- max_rank ------------------------------------------------------------------------------------------------------------------------
// ... of a sub-block with nsym symbols: bsr(nsym - 1), 0 for nsym <= 2 (qlfc.cpp:888, encode_alphabet)
static inline int dc_max_rank(int nsym)
{
    int k = 0;
    for (int v = nsym - 1; v > 1; v >>= 1) ++k;
    return k;
}
// ... of sub-blocks 0 .. nb - 1 from the front end's table: first_run[256 b + c] = the first run of symbol c in sub-block b, 0xffffffff: none
static inline void dc_max_rank_table(const uint32_t* first_run, int nb, int* max_rank)
{
    for (int b = 0; b < nb; ++b) {
        int nsym = 0;
        for (int c = 0; c < 256; ++c) nsym += first_run[b * 256 + c] != 0xffffffffu;
        max_rank[b] = dc_max_rank(nsym);
    }
}

// ---- what the driver of one block decides ------------------------------------------------------------------------------------------
// Plain functions of integers and flags; the driver (block.cpp: gpu_stage) reads the environment and the context and asks.
// Whether the block tries the device model: the caller allows it (a redo does not), BSC_DEVICE_CODER, the static coder or the fast one
// with BSC_DEVICE_CODER_FAST, several sub-blocks, and at least BSC_DEVICE_CODER_MIN_N bytes.
static inline bool dc_block_tries_model(bool allowed, bool enabled, bool coder_static, bool coder_fast_enabled, int nsub, int64_t n, int64_t min_n)
{
    return allowed && enabled && (coder_static || coder_fast_enabled) && nsub > 1 && n >= min_n;
}
// Whether its m runs are too dense to bother: nearly one run per byte, the sub-blocks will be stored raw anyway
static inline bool dc_block_runs_too_dense(uint32_t m, int n) { return !((double)m <= 0.70 * (double)n); }
// What becomes of the block after the model returned code (a libbsc code).  sent: a block in several segments has issued its pieces;
// else NO_ERROR says that the whole stream lies in the device buffer — device_rc: the context codes it there (BSCGPU_OPT_DEVICE_RC);
// zone: the pinned landing zone could be had (not asked where device_rc is on).
enum DcBlockVerdict {
    DC_BLOCK_SENT,              // the pieces are on their way to the landing zone: the host codes from the stream
    DC_BLOCK_DEVICE_RC,         // range-coded on the device
    DC_BLOCK_LANDED,            // the whole stream goes down to the landing zone: the host codes from it
    DC_BLOCK_HOST_MODEL,        // declined, or no landing zone: the run arrays go down and the host models
    DC_BLOCK_ERROR              // code is the call's result
};
static inline DcBlockVerdict dc_block_verdict(int code, bool sent, bool device_rc, bool zone)
{
    if (code == 0 /* LIBBSC_NO_ERROR */) return sent ? DC_BLOCK_SENT : device_rc ? DC_BLOCK_DEVICE_RC : zone ? DC_BLOCK_LANDED : DC_BLOCK_HOST_MODEL;
    return code == DC_BLOCK_NOT_SUPPORTED ? DC_BLOCK_HOST_MODEL : DC_BLOCK_ERROR;
}
