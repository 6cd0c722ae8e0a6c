// bwt_plan.h — what the BWT driver (bwt.hip) decides, as plain host arithmetic without any HIP in it: the layout of the first sort's
// keys, how key bits are cut into digit passes, which kind of refinement round an unsorted set gets, and whether a round on text
// keys paid.  The driver launches what these functions say; tools/bwt_plan_probe.cpp prints them for tests/test_bwt_plan_host.py.
#pragma once
#include <stdint.h>

struct RadixPass { int shift; int bits; };             // one digit pass of the radix engine (dev_common.h: radix_sort_passes)

// The driver's environment switches (bwt.hip: bwt_switches reads them once per process).  A/B and tests; the output is the same.
struct BwtSwitches {
    int wmax;           // BSC_BWT_W=<w>: at most w characters per first-sort key (>= 2; experiment: shorter first-sort keys), default 0 = no cap
    int text_rounds;    // BSC_BWT_TEXTROUNDS=0 keeps the round-1 flow (ISA built by the first seg, doubling from h = w)
    int hybrid;         // BSC_BWT_HYBRID=0: never a hybrid round (the whole round through the radix engine, as in round 3)
    int hybrid_pct;     // BSC_BWT_HYBRID_PCT=<p>: a hybrid round only while the groups of > HY_G records hold at most p % of the round's records
                        // (shared objects, first rounds: 48 of 57 M records are extracted; same box, 64 MiB: 40.4 ms without, 36.3 at 50 %, 34.8 at 100 % = the default)
    int isa_skip;       // BSC_BWT_ISASKIP=0 stores every rank of every round
};

static inline int bwt_bit_length(uint64_t x) { int b = 0; while (x) { ++b; x >>= 1; } return b; }

// Digits are 8 bits from shift s0 upwards over kbits key bits, the topmost with what is left.  -> number of passes
// (measured: 7- / 6-bit digits raise per-pass bandwidth (3.5 -> 3.8 / 4.0 TB/s) but the extra passes lose overall)
static inline int bwt_cut_passes(RadixPass* out, int s0, int kbits)
{
    int np = 0;
    for (int s = 0; s < kbits; s += 8) { out[np].shift = s0 + s; out[np].bits = (kbits - s < 8) ? kbits - s : 8; ++np; }
    return np;
}

// ---- key plan --------------------------------------------------------------------------------------------------------------------
struct BwtKeyPlan {
    uint32_t cb, w, tc, low_shift, pred_shift;          // PackParams (bwt.hip) is filled from these
    uint32_t batch_bb;                                  // bits of a batched pass's block field on top of the key
    uint32_t ta;                                        // characters a round on text keys takes
    uint32_t smask, tail_lo;
    uint32_t fold_r; int fold_np; bool fold;            // key packing sorts the leftover fold_r low bits itself, fold_np byte passes follow
    RadixPass passes[8]; int npass;                     // the first sort's digit passes
};

// K: distinct bytes of the text (of the whole pass for a batch); n: its length; batch_count: blocks of a batched pass, 0 = a single
// block; wmax: BwtSwitches::wmax; single_read: the single-read digit passes would take a sort of n records in fold_np passes and
// folding is on (the caller asks radix_onesweep_wanted: fold_np does not depend on the answer).
static inline BwtKeyPlan bwt_key_plan(uint32_t K, uint32_t n, uint32_t batch_count, int wmax, bool single_read)
{
    BwtKeyPlan p;
    const bool bt = batch_count != 0;
    // a batched pass: codes 1..K (0 = past the block's end) below the block field; no text rounds, no predecessor codes (see bwt_batch_pack_kernel)
    p.batch_bb = bt ? (uint32_t)bwt_bit_length(batch_count - 1) : 0u;
    p.cb = 1; while ((1u << p.cb) < K + (bt ? 1u : 0u)) ++p.cb;
    if (p.cb < 4) p.cb = 4;                                   // at most 16 characters per key
    p.w = 64 / p.cb;
    if (bt) { p.w = (64 - p.batch_bb) / p.cb; if (p.w > 16) p.w = 16; }
    else if (wmax >= 2 && (uint32_t)wmax < p.w) p.w = (uint32_t)wmax;
    // (Base-K keys — the w characters as one base-K number, 13 instead of 12 characters for 28 symbols — were measured and removed: fewer
    // unsorted suffixes after the first sort, but slower digit passes on their uniform bytes; profiles/r06/first_sort_keys.txt.)
    p.tc = n < p.w - 1 ? n : p.w - 1;
    p.low_shift = 64 - p.cb * p.w - p.batch_bb;
    // The sort's values have spare high bits when the block is not huge: carry the code of the character in FRONT of the
    // suffix there, so that the final L = T[SA - 1] needs no random gather from the text
    const int idx_bits = bwt_bit_length(n - 1);
    p.pred_shift = (!bt && idx_bits >= 1 && idx_bits + (int)p.cb <= 32) ? (uint32_t)idx_bits : 0u;
    p.smask = p.pred_shift ? ((1u << p.pred_shift) - 1u) : 0xffffffffu;
    p.tail_lo = bt ? 0xffffffffu : (n >= p.w) ? (n - (p.w - 1)) : 0;
    // Rounds on text keys (bwt_round_textsort_kernel) need a characters + 4 bits in 64: a = w where the first-sort key leaves
    // 4 bits spare, else w - 1.
    p.ta = (p.cb * p.w + 4 <= 64) ? p.w : p.w - 1;
    // Pass plan.  Where the key's width leaves r = (cb * w) mod 8 bits over, 1 <= r <= 4 (17..64 symbols: 60 key bits, r = 4), that half
    // digit costs a whole pass over all records; key packing writes every record once anyway, so it places them by these r bits itself
    // (bwt_pack_fold_kernel; r <= cb: the digit lies inside the key's last character) and the sort is (cb * w - r) / 8 byte passes
    // from low_shift + r.  A stable LSD sort gives the same arrays however the bits are cut into digits.  Only single blocks whose
    // sort takes the single-read passes go this way (so not the retry after a give-up, os_mode == 0); everything else keeps the plan
    // and the kernels it had.
    p.fold_r = (p.cb * p.w) & 7u;
    p.fold_np = (int)((p.cb * p.w - p.fold_r) / 8u);
    p.fold = !bt && p.fold_r >= 1 && p.fold_r <= 4 && p.fold_r <= p.cb && n >= p.w && single_read;
    p.npass = p.fold ? bwt_cut_passes(p.passes, (int)(p.low_shift + p.fold_r), 8 * p.fold_np)
                     : bwt_cut_passes(p.passes, (int)p.low_shift, 64 - (int)p.low_shift);
    return p;
}

// ---- round decision --------------------------------------------------------------------------------------------------------------
enum BwtRound {
    BWT_ROUND_TEXT,          // a round on text keys (bwt_round_textsort_kernel)
    BWT_ROUND_TEXT_SPLIT,    // ... with the groups too long for one workgroup split by the top bits of the round's key first
    BWT_ROUND_HAND_OVER,     // no text round: ISA from the current order, this round doubles
    BWT_ROUND_SEGSORT,       // prefix doubling: segmented sort of the grouped records
    BWT_ROUND_HYBRID,        // ... the large groups through the radix engine, the rest through the segmented sort
    BWT_ROUND_RADIX,         // ... the whole round through the radix engine
};

// What the seg that produced an unsorted set of U records counted (seg_apply): groups no segmented sort of this round can take
// (> RS_G records) with their records, and the same for groups of > HY_G records (hybrid rounds).
struct BwtRoundCounts { uint32_t U, n_long, n_long_rec, n_mid, n_mid_rec; };

// isa_valid: the rounds double (ISA exists); else they are rounds on text keys.  lg_max: long groups the split's tables hold (LG_MAX).
static inline BwtRound bwt_round_kind(bool isa_valid, const BwtRoundCounts& g, const BwtSwitches& sw, uint32_t lg_max)
{
    if (!isa_valid) {
        if (g.n_long == 0) return BWT_ROUND_TEXT;
        // Groups too long for one workgroup.  While they hold a small part of the round's records they — and only they — are
        // split by the top bits of this round's key and the segmented sort runs with the bucket starts as extra boundaries;
        // otherwise (long repeats: most unsorted suffixes sit in a few huge groups, and their records would all go through
        // global atomics — python sources, 64 MiB: 127 ms against 44 ms) the round is handed over to prefix doubling at once,
        // without first running a sort that gives up (9.5 ms on that block).
        return (g.n_long <= lg_max && g.n_long_rec <= g.U / 8u) ? BWT_ROUND_TEXT_SPLIT : BWT_ROUND_HAND_OVER;
    }
    // A round with a group of > RS_G records is a hybrid round, unless the switches say otherwise; without such a group the segmented
    // sort takes it (with one the kernel would only find out and give up), else the radix engine.
    if (sw.hybrid && g.n_long != 0 && g.n_mid != 0 && (uint64_t)g.n_mid_rec * 100ull <= (uint64_t)g.U * (uint64_t)sw.hybrid_pct) return BWT_ROUND_HYBRID;
    return g.n_long == 0 ? BWT_ROUND_SEGSORT : BWT_ROUND_RADIX;
}

// After a round on text keys that took U unsorted suffixes to U2, the text_rounds-th of the block: is the next round one too?
// (else it hands over to prefix doubling: the round did not pay)
static inline bool bwt_text_round_pays(uint32_t U, uint32_t U2, int text_rounds)
{
    return (U2 < 65536u || U2 <= U / 4) && text_rounds < 8;
}
