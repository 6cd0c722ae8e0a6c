// dc_segment_plan.h — what the driver of a pass in model segments (devcoder.hip: devcoder_pstream_segments; DESIGN §2b, "Model
// segments") decides, as plain host arithmetic without any HIP in it: which blocks the plan leaves out and where it cuts, what a range
// takes of the landing buffer, whether it still fits, where a range that declined is split and how often, where the kept entries of a
// range land and how its sub-block offsets join the pass's — and the CPU stand-in of the packed layout.  The driver launches what
// DcSegSchedule hands out and tells it what came of it; tools/dc_segment_probe.cpp does the same with a rule in place of the model,
// for tests/test_dc_segment_plan_host.py.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <vector>

// ---- the packed 13-bit layout ("The packed stream of a pass") -----------------------------------------------------------
// a sub-block of `dec` decisions holds dc_pack13_fields(dec) 13-bit fields: whole groups of 64, 104 bytes each
static inline int64_t dc_pack13_fields(uint32_t dec) { return ((int64_t)dec + 63) / 64 * 64; }
static inline int64_t dc_pack13_bytes(int64_t fields) { return fields / 8 * 13; }

// The CPU stand-in for the layout: packs 16-bit static entries (sub-block s's at ps + poff[s]) into out, pbase[0..nsub] in fields.
// -> the bytes of the packed form (nothing is written when they exceed cap_bytes), -1: poff decreases, or ps / out is missing
static inline int64_t dc_pack13_host(const uint16_t* ps, const uint32_t* poff, int nsub, uint8_t* out, int64_t cap_bytes, int64_t* pbase)
{
    pbase[0] = 0;
    for (int s = 0; s < nsub; ++s) {
        if (poff[s + 1] < poff[s]) return -1;
        pbase[s + 1] = pbase[s] + dc_pack13_fields(poff[s + 1] - poff[s]);
    }
    const int64_t bytes = dc_pack13_bytes(pbase[nsub]);
    if (bytes > cap_bytes || bytes == 0) return bytes;
    if (!out || !ps) return -1;
    for (int s = 0; s < nsub; ++s) {
        const uint16_t* e = ps + poff[s];
        const int64_t len = (int64_t)(poff[s + 1] - poff[s]);
        uint8_t* g = out + dc_pack13_bytes(pbase[s]);
        for (int64_t k = 0; k < pbase[s + 1] - pbase[s]; k += 8, g += 13) {
            uint64_t lo = 0, hi = 0;                                   // fields 0..4 (the fifth's low 12 bits) | its top bit, fields 5..7
            for (int x = 0; x < 8; ++x) {
                const uint64_t f = k + x < len ? (uint64_t)(e[k + x] & 0x1fffu) : 0u;
                if (x < 4) lo |= f << (13 * x);
                else if (x == 4) { lo |= f << 52; hi |= f >> 12; }
                else hi |= f << (13 * (x - 5) + 1);
            }
            for (int i = 0; i < 8; ++i) g[i] = (uint8_t)(lo >> (8 * i));
            for (int i = 0; i < 5; ++i) g[8 + i] = (uint8_t)(hi >> (8 * i));
        }
    }
    return bytes;
}

// ---- the plan ------------------------------------------------------------------------------------------------------------------------
// Blocks in order; sub_dec[s] / sub_und[s]: decisions and undecided avg_rank flags of sub-block s, block b's sub-blocks are
// [blk_sub[b], blk_sub[b + 1]).  A block with an undecided flag or more than dcap decisions is left out (seg_of[b] = -1) and ends the
// segment before it; an empty block is in no segment and ends nothing; the others fill segments of at most min(dcap, target)
// decisions (target <= 0: dcap).  -> the number of segments.  blk_sub must not decrease (the exported wrapper checks).
// sub_mix (optional, the adaptive coder's third fact): the longest mixer chain of every sub-block, read only where sub_und[s] == 0; a
// block with a sub-block whose chain exceeds mix_cap is left out like an undecided one.  Null: no such rule.
static inline bool dc_segment_mix_barred(const uint32_t* sub_und, const uint32_t* sub_mix, int64_t mix_cap, int s0, int s1)
{
    if (!sub_mix) return false;
    for (int s = s0; s < s1; ++s) if (sub_und[s] == 0 && (int64_t)sub_mix[s] > mix_cap) return true;
    return false;
}
static inline int dc_segment_plan(const uint32_t* sub_dec, const uint32_t* sub_und, const int* blk_sub, int count, int64_t dcap, int64_t target, int* seg_of,
                                  const uint32_t* sub_mix = nullptr, int64_t mix_cap = 0)
{
    const int64_t limit = target > 0 && target < dcap ? target : dcap;
    int nseg = 0;
    bool open = false;              // a segment is being filled
    int64_t filled = 0;
    for (int b = 0; b < count; ++b) {
        if (blk_sub[b + 1] == blk_sub[b]) { seg_of[b] = -1; continue; }      // empty: ends nothing
        int64_t dec = 0; bool und = false;
        for (int s = blk_sub[b]; s < blk_sub[b + 1]; ++s) { dec += sub_dec[s]; und = und || sub_und[s] != 0; }
        if (und || dec > dcap || dc_segment_mix_barred(sub_und, sub_mix, mix_cap, blk_sub[b], blk_sub[b + 1])) { seg_of[b] = -1; open = false; continue; }
        if (!open || filled + dec > limit) { ++nseg; open = true; filled = 0; }
        filled += dec;
        seg_of[b] = nseg - 1;
    }
    return nseg;
}

// ---- the schedule of a pass ----------------------------------------------------------------------------------------------------------
// a range of blocks [b0, b1) to model as one small pass: its sub-blocks [s0, s1), the decisions it must come to, and what it takes of
// the landing buffer in the buffer's units (entries, or bytes of the packed form)
struct DcSegRange { int b0, b1, s0, s1; int64_t expect, need; };

enum DcSegNext {
    DC_SEG_RUN,          // the range is to be modelled; its outcome goes to declined() or kept()
    DC_SEG_GIVEN_UP,     // the range no longer fits behind the kept ones (per_segment_fit): its blocks are the host's, nothing to run
    DC_SEG_DONE,         // no range is left
};

struct DcSegTotals { int planned, kept, reruns, host_blocks, kept_packed, kept_void, fail; int64_t decisions; };

// Constructed from the facts of a pass; the caller's poff[0..nsub], pbase[0..nsub] (non-null: the packed form, cap and every need in
// bytes) and blk_state[0..count) are written as the pass goes.  After construction blk_state holds the blocks the plan left out
// (fail_avg where a sub-block has an undecided flag, else fail_cap where its decisions exceed dcap, else fail_mix — mix non-null only: a
// mixer chain above mix_cap; BSCGPU_DC_FAIL_*), planned_need() and copy_all() are known.  Every range with a member ends in exactly one
// of: next() -> DC_SEG_GIVEN_UP, declined() -> true, kept().
class DcSegSchedule {
public:
    DcSegSchedule(const uint32_t* dec, const uint32_t* und, const int* blk_sub, int count, int nsub, int64_t dcap, int64_t target, int64_t cap,
                  bool per_segment_fit, int fail_avg, int fail_cap, uint32_t* poff, int64_t* pbase, int* blk_state,
                  const uint32_t* mix = nullptr, int64_t mix_cap = 0, int fail_mix = 0)
        : dec(dec), blk_sub(blk_sub), count(count), nsub(nsub), cap(cap), per_segment_fit(per_segment_fit), fail_cap(fail_cap), poff(poff), pbase(pbase), blk_state(blk_state)
    {
        std::vector<int> seg_of((size_t)count);
        T.planned = dc_segment_plan(dec, und, blk_sub, count, dcap, target, seg_of.data(), mix, mix_cap);
        int nblk = 0;
        // the ranges are grown from the right (the stack then yields them in block order): an empty block between two members of a
        // segment lies inside its range, one at its left edge does not — either way it has no sub-block
        for (int b = count - 1; b >= 0; --b) {
            blk_state[b] = 0;
            if (!member(b)) continue;                                  // an empty block: nothing to model
            ++nblk;
            if (seg_of[b] < 0) {
                bool open = false; int64_t own = 0;
                for (int s = blk_sub[b]; s < blk_sub[b + 1]; ++s) { open = open || und[s] != 0; own += dec[s]; }
                blk_state[b] = open ? fail_avg : own > dcap || !mix ? fail_cap : fail_mix;
                continue;
            }
            need_all += span_need(blk_sub[b], blk_sub[b + 1]);
            if (!todo.empty() && seg_of[todo.back().b0] == seg_of[b]) todo.back().b0 = b; else todo.push_back(Seg{b, b + 1});
        }
        int lg = 0; while ((1 << lg) < nblk) ++lg;
        rerun_max = 2 * lg + 2;
        poff[0] = 0;
        if (pbase) pbase[0] = 0;
    }

    int64_t planned_need() const { return need_all; }
    // are kept entries copied out at all: always under per_segment_fit, else only when the whole plan fits (counted, not copied)
    bool copy_all() const { return per_segment_fit || need_all <= cap; }

    DcSegNext next(DcSegRange* g)
    {
        if (todo.empty()) return DC_SEG_DONE;
        const Seg t = todo.back(); todo.pop_back();
        g->b0 = t.b0; g->b1 = t.b1; g->s0 = blk_sub[t.b0]; g->s1 = blk_sub[t.b1];
        g->expect = 0;
        for (int s = g->s0; s < g->s1; ++s) g->expect += dec[s];
        g->need = span_need(g->s0, g->s1);
        if (per_segment_fit && base + g->need > cap) { give_up(*g, fail_cap); return DC_SEG_GIVEN_UP; }
        return DC_SEG_RUN;
    }

    // the range declined while it ran, with reason mask `why` -> true: it is given up (a single member, or the re-run budget is spent) and
    // its blocks carry the reason; false: its two halves are the next ranges
    bool declined(const DcSegRange& g, int why)
    {
        int members = 0; for (int b = g.b0; b < g.b1; ++b) members += member(b);
        if (members < 2 || T.reruns + 2 > rerun_max) { give_up(g, why); return true; }
        // the block boundary nearest half the decisions, with a member on either side
        int cut = -1; int64_t acc = 0, best = 0;
        int seen = 0;
        for (int b = g.b0; b < g.b1; ++b) {
            if (!member(b)) continue;
            for (int s = blk_sub[b]; s < blk_sub[b + 1]; ++s) acc += dec[s];
            if (++seen == members) break;
            const int64_t dist = acc * 2 > g.expect ? acc * 2 - g.expect : g.expect - acc * 2;
            if (cut < 0 || dist < best) { cut = b + 1; best = dist; }
        }
        todo.push_back(Seg{cut, g.b1}); todo.push_back(Seg{g.b0, cut});
        T.reruns += 2;
        return false;
    }

    // the range was modelled: D decisions, sub-block i's at pseg[i] .. pseg[i + 1] of its stream, and (packed form) either its fields
    // at pbseg[i] .. pbseg[i + 1] (packed) or the 2-byte form after all (void: pbseg is derived from pseg, as dc_pack13_host lays it out).
    // Joins them to the pass's poff / pbase -> where the range's stream lands in the buffer, in its units; -1: the packed layout is not
    // the one the plan counted on
    int64_t kept(const DcSegRange& g, uint32_t D, const uint32_t* pseg, const uint32_t* pbseg, bool packed)
    {
        fill_to(g.s0);
        for (int s = g.s0; s < g.s1; ++s) poff[s + 1] = poff[g.s0] + (pseg[s - g.s0 + 1] - pseg[0]);
        filled = g.s1;
        if (pbase) {
            int64_t at = 0;
            for (int s = g.s0; s < g.s1; ++s) {
                at = packed ? (int64_t)pbseg[s - g.s0 + 1] : at + dc_pack13_fields(pseg[s - g.s0 + 1] - pseg[s - g.s0]);
                pbase[s + 1] = pbase[g.s0] + at;
            }
            if (dc_pack13_bytes(at) != g.need) return -1;
            ++(packed ? T.kept_packed : T.kept_void);
        }
        const int64_t at = base;
        base += pbase ? g.need : (int64_t)D;
        T.decisions += D; ++T.kept;
        return at;
    }

    // after the last range: the sub-blocks behind the last kept one are empty -> what the pass came to
    DcSegTotals finish()
    {
        fill_to(nsub);
        T.fail = T.host_blocks = 0;
        for (int b = 0; b < count; ++b) if (blk_state[b]) { T.fail |= blk_state[b]; ++T.host_blocks; }
        return T;
    }

private:
    struct Seg { int b0, b1; };
    bool member(int b) const { return blk_sub[b + 1] > blk_sub[b]; }
    int64_t span_need(int s0, int s1) const
    {
        int64_t t = 0;
        for (int s = s0; s < s1; ++s) t += pbase ? dc_pack13_bytes(dc_pack13_fields(dec[s])) : (int64_t)dec[s];
        return t;
    }
    void give_up(const DcSegRange& g, int why) { for (int b = g.b0; b < g.b1; ++b) if (member(b)) blk_state[b] = why; }
    // poff / pbase are written as the ranges are kept (they come in block order): everything up to sub-block `filled` is final, and a
    // sub-block that was not modelled ends where it starts
    void fill_to(int s) { for (; filled < s; ++filled) { poff[filled + 1] = poff[filled]; if (pbase) pbase[filled + 1] = pbase[filled]; } }

    const uint32_t* dec; const int* blk_sub; int count, nsub; int64_t cap; bool per_segment_fit; int fail_cap;
    uint32_t* poff; int64_t* pbase; int* blk_state;
    std::vector<Seg> todo;                                            // a stack: depth first, in block order
    int64_t need_all = 0;                                             // what the planned blocks take of the landing buffer
    int rerun_max = 0;                                                // 2 ceil(log2(blocks)) + 2 re-runs a pass
    int filled = 0;
    int64_t base = 0;                                                 // where the next kept range lands
    DcSegTotals T = {};
};
