// devcoder_model.h — the static QLFC model (-e1) restated as data-parallel pieces, shared by the HIP kernels
// (devcoder.hip) and by host code (host range coder, CPU checks).  Plain integer functions, no HIP dependency.
//
// What the reference does per run, serially (libbsc/coder/qlfc/qlfc.cpp:896-1126, model slots qlfc_model.h:38-176):
// a short list of binary decisions, each predicted by THREE adaptive counters — one indexed by a context state, one by
// the run's symbol, one by nothing but the decision's place in the code tree — whose values are blended into a 12-bit
// probability and then updated with the coded bit (predictor.h:53-61).  Which three counters a decision touches is a pure
// function of the run data; each counter only ever sees its own decisions.  So the model is a set of independent CHAINS,
//      chain = (sub-block, decision type tau, family in {state, char, static}, X = state | symbol | nothing),
// every chain the recurrence v <- step(v, bit) over its decisions in stream order, starting from 2048.
//
// Decision types ("tau", 1080 of them) enumerate the code tree positions:
//   RF                 rank == 1 ?                                   1        class 0  (qlfc.cpp:904)
//   RE s               unary exponent of the rank, position s        7        class 1  (:919-:935)
//   RM (B, ctx)        mantissa of a B-bit rank, tree node ctx       247      class 2  (:938-:953)
//   RP ctx             escape coding of the rank (avg_rank >= 32)    255      class 3  (:960-:975)
//   NF                 run length == 1 ?                             1        class 4  (:990)
//   NE s               unary exponent of the run length              31       class 5  (:1003-:1019)
//   NM (bits, ctx)     mantissa of the run length                    538      class 6  (:1022-:1060)
// Inside one run every type occurs at most once, always in the order of the "canonical rounds" below, which is what lets a
// wavefront emit the decisions of 64 runs round by round and rank them stably with ballots.
#pragma once
#include <stdint.h>
#include <vector>

#if defined(__HIPCC__)
#define DC_HD __host__ __device__ __forceinline__
#else
#define DC_HD inline
#endif

namespace dcm {

// (CLS_NM2: run-length mantissas of more than 5 bits — one node per depth instead of a tree.  The static coder gives them the rates of
// CLS_NM; the fast coder, which runs on the same machinery, does not: qlfc.cpp:1316-1331)
enum : int { CLS_RF = 0, CLS_RE, CLS_RM, CLS_RP, CLS_NF, CLS_NE, CLS_NM, CLS_NM2, NUM_CLS };
enum : int { FAM_STATE = 0, FAM_CHAR = 1, FAM_STATIC = 2 };

// ---- type ids -------------------------------------------------------------------------------------------------------
constexpr int TAU_RF = 0, TAU_RE = 1, TAU_RM = 8, TAU_RP = 255, TAU_NF = 510, TAU_NE = 511, TAU_NM = 542, NUM_TAU = 1080;

DC_HD int bsr(uint32_t x) { return x ? 31 - __builtin_clz(x) : 0; }
// RM: B = 1..7, ctx in [1, 2^B): types of smaller B first
DC_HD int rm_off(int B) { return (1 << B) - 1 - B; }                       // sum_{b<B} (2^b - 1)
// NM: bits 1..5 are full trees (2^bits - 1 nodes), bits 6..31 are chains (ctx = 1..bits)
DC_HD int nm_off(int bits) { return bits <= 6 ? (1 << bits) - 1 - bits : 57 + (bits * (bits - 1)) / 2 - 15; }
constexpr int TAU_NM2 = TAU_NM + 57;                                         // = TAU_NM + nm_off(6): first type of the 6-bit chain
DC_HD int tau_class(int tau)
{
    return tau < TAU_RE ? CLS_RF : tau < TAU_RM ? CLS_RE : tau < TAU_RP ? CLS_RM : tau < TAU_NF ? CLS_RP
         : tau < TAU_NE ? CLS_NF : tau < TAU_NM ? CLS_NE : tau < TAU_NM2 ? CLS_NM : CLS_NM2;
}

// ---- canonical rounds ----------------------------------------------------------------------------------------------
// rank side: 0 RF | 1..7 RE s | 8..14 RM depth d | 15..22 RP depth d;   run side: 23 NF | 24..54 NE s | 55..85 NM depth d
constexpr int ROUND_RF = 0, ROUND_RE = 1, ROUND_RM = 8, ROUND_RP = 15, ROUND_NF = 23, ROUND_NE = 24, ROUND_NM = 55, NUM_ROUNDS = 86;
DC_HD int tau_round(int tau)
{
    if (tau < TAU_RE) return ROUND_RF;
    if (tau < TAU_RM) return ROUND_RE + (tau - TAU_RE);
    if (tau < TAU_RP) {                                        // depth of ctx inside its B-tree
        int t = tau - TAU_RM, B = 1;
        while (t >= (1 << B) - 1) { t -= (1 << B) - 1; ++B; }
        return ROUND_RM + bsr((uint32_t)t + 1);
    }
    if (tau < TAU_NF) return ROUND_RP + bsr((uint32_t)(tau - TAU_RP) + 1);
    if (tau < TAU_NE) return ROUND_NF;
    if (tau < TAU_NM) return ROUND_NE + (tau - TAU_NE);
    int t = tau - TAU_NM, bits = 1;
    for (;;) { const int cnt = bits <= 5 ? (1 << bits) - 1 : bits; if (t < cnt) break; t -= cnt; ++bits; }
    return ROUND_NM + (bits <= 5 ? bsr((uint32_t)t + 1) : t);
}

// ---- one run ("item") ----------------------------------------------------------------------------------------------
// packed item: [63:56] X (sort digit) | [55:53] sub-block | [52] avg_rank >= 32 | [51:44] rank | [43:13] run length
struct Item { uint32_t rank, run, sb, ge32; };
DC_HD uint64_t item_pack(uint32_t X, uint32_t sb, uint32_t ge32, uint32_t rank, uint32_t run)
{
    return ((uint64_t)X << 56) | ((uint64_t)sb << 53) | ((uint64_t)ge32 << 52) | ((uint64_t)rank << 44) | ((uint64_t)run << 13);
}
DC_HD Item item_unpack(uint64_t k)
{
    Item it;
    it.sb = (uint32_t)(k >> 53) & 7u; it.ge32 = (uint32_t)(k >> 52) & 1u; it.rank = (uint32_t)(k >> 44) & 0xffu; it.run = (uint32_t)(k >> 13) & 0x7fffffffu;
    return it;
}
DC_HD uint32_t item_X(uint64_t k) { return (uint32_t)(k >> 56); }
// packed item of a batched pass (up to 8192 sub-blocks, every block below 1 MiB):
//   [63:56] X | [55:43] sub-block | [42] avg_rank >= 32 | [41:34] rank | [33:31] max_rank of the sub-block | [30:10] run length
// The sub-block sits directly below X, as in the eight-entry form: "same chain" stays one shift (ITEMB_CHAIN_SHIFT) and one compare.
struct ItemB : Item { uint32_t maxr; };
constexpr int ITEM_CHAIN_SHIFT = 53, ITEMB_CHAIN_SHIFT = 43, ITEMB_SUB_BITS = 13, ITEMB_RUN_BITS = 21;
DC_HD uint64_t item_pack_b(uint32_t X, uint32_t sb, uint32_t ge32, uint32_t rank, uint32_t maxr, uint32_t run)
{
    return ((uint64_t)X << 56) | ((uint64_t)sb << 43) | ((uint64_t)ge32 << 42) | ((uint64_t)rank << 34) | ((uint64_t)maxr << 31) | ((uint64_t)run << 10);
}
DC_HD ItemB item_unpack_b(uint64_t k)
{
    ItemB it;
    it.sb = (uint32_t)(k >> 43) & 0x1fffu; it.ge32 = (uint32_t)(k >> 42) & 1u; it.rank = (uint32_t)(k >> 34) & 0xffu;
    it.maxr = (uint32_t)(k >> 31) & 7u; it.run = (uint32_t)(k >> 10) & 0x1fffffu;
    return it;
}

// number of decisions on each side (qlfc.cpp:904-975 / :990-1060)
DC_HD int count_rank_side(const Item& it, int max_rank)
{
    if (it.ge32) return max_rank + 1;
    if (it.rank == 1) return 1;
    const int B = bsr(it.rank);
    return 1 + (B - 1) + (B < max_rank ? 1 : 0) + B;
}
DC_HD int count_run_side(const Item& it)
{
    if (it.run == 1) return 1;
    const int bits = bsr(it.run);
    return 1 + bits + bits;
}

// The decision of canonical round r for this run, if it has one: returns tau (>= 0) and the coded bit, or -1.
DC_HD int decision(const Item& it, int max_rank, int r, uint32_t* bit)
{
    if (r < ROUND_NF) {
        const uint32_t rank = it.rank;
        if (r >= ROUND_RP) {                                   // escape coding: max_rank + 1 mantissa-like decisions
            const int d = r - ROUND_RP;
            if (!it.ge32 || d > max_rank) return -1;
            const uint32_t ctx = (1u << d) | ((rank >> (max_rank + 1 - d)) & ((1u << d) - 1u));
            *bit = (rank >> (max_rank - d)) & 1u;
            return TAU_RP + (int)ctx - 1;
        }
        if (it.ge32) return -1;
        if (r == ROUND_RF) { *bit = rank != 1u; return TAU_RF; }
        if (rank == 1u) return -1;
        const int B = bsr(rank);
        if (r < ROUND_RM) {
            const int s = r - ROUND_RE;                        // s = b - 1
            if (s <= B - 2) { *bit = 1u; return TAU_RE + s; }
            if (s == B - 1 && B < max_rank) { *bit = 0u; return TAU_RE + s; }
            return -1;
        }
        const int d = r - ROUND_RM;
        if (d >= B) return -1;
        const uint32_t ctx = rank >> (B - d);
        *bit = (rank >> (B - 1 - d)) & 1u;
        return TAU_RM + rm_off(B) + (int)ctx - 1;
    }
    const uint32_t run = it.run;
    if (r == ROUND_NF) { *bit = run != 1u; return TAU_NF; }
    if (run == 1u) return -1;
    const int bits = bsr(run);
    if (r < ROUND_NM) {
        const int s = r - ROUND_NE;
        if (s <= bits - 2) { *bit = 1u; return TAU_NE + s; }
        if (s == bits - 1) { *bit = 0u; return TAU_NE + s; }
        return -1;
    }
    const int d = r - ROUND_NM;
    if (d >= bits) return -1;
    const uint32_t ctx = bits <= 5 ? (run >> (bits - d)) : (uint32_t)(1 + d);
    *bit = (run >> (bits - 1 - d)) & 1u;
    return TAU_NM + nm_off(bits) + (int)ctx - 1;
}

// All decisions of a run in canonical (= stream) order: f(tau, bit, run_side).
template <class F>
DC_HD void enumerate(const Item& it, int max_rank, F&& f)
{
    const uint32_t rank = it.rank, run = it.run;
    if (it.ge32) {
        for (int d = 0; d <= max_rank; ++d) {
            const uint32_t ctx = (1u << d) | ((rank >> (max_rank + 1 - d)) & ((1u << d) - 1u));
            f(TAU_RP + (int)ctx - 1, (rank >> (max_rank - d)) & 1u, false);
        }
    } else {
        f(TAU_RF, rank != 1u ? 1u : 0u, false);
        if (rank != 1u) {
            const int B = bsr(rank);
            for (int s = 0; s <= B - 2; ++s) f(TAU_RE + s, 1u, false);
            if (B < max_rank) f(TAU_RE + B - 1, 0u, false);
            for (int d = 0; d < B; ++d) f(TAU_RM + rm_off(B) + (int)(rank >> (B - d)) - 1, (rank >> (B - 1 - d)) & 1u, false);
        }
    }
    f(TAU_NF, run != 1u ? 1u : 0u, true);
    if (run != 1u) {
        const int bits = bsr(run);
        for (int s = 0; s <= bits - 2; ++s) f(TAU_NE + s, 1u, true);
        f(TAU_NE + bits - 1, 0u, true);
        for (int d = 0; d < bits; ++d) {
            const uint32_t ctx = bits <= 5 ? (run >> (bits - d)) : (uint32_t)(1 + d);
            f(TAU_NM + nm_off(bits) + (int)ctx - 1, (run >> (bits - 1 - d)) & 1u, true);
        }
    }
}

// The k-th decision of a run (k counted over both sides, stream order), without walking the ones before it.
DC_HD int nth_decision(const Item& it, int max_rank, int n_rank, int k, uint32_t* bit, bool* run_side)
{
    if (k < n_rank) {
        const uint32_t rank = it.rank;
        *run_side = false;
        if (it.ge32) { return decision(it, max_rank, ROUND_RP + k, bit); }
        if (k == 0) { *bit = rank != 1u ? 1u : 0u; return TAU_RF; }
        const int B = bsr(rank);
        const int e = (B - 1) + (B < max_rank ? 1 : 0);
        if (k <= e) { const int sx = k - 1; *bit = sx + 1 < B ? 1u : 0u; return TAU_RE + sx; }
        const int d = k - 1 - e;
        *bit = (rank >> (B - 1 - d)) & 1u;
        return TAU_RM + rm_off(B) + (int)(rank >> (B - d)) - 1;
    }
    const int kk = k - n_rank;
    const uint32_t run = it.run;
    *run_side = true;
    if (kk == 0) { *bit = run != 1u ? 1u : 0u; return TAU_NF; }
    const int nb = bsr(run);
    if (kk <= nb) { const int sx = kk - 1; *bit = sx + 1 < nb ? 1u : 0u; return TAU_NE + sx; }
    const int d = kk - 1 - nb;
    const uint32_t ctx = nb <= 5 ? (run >> (nb - d)) : (uint32_t)(1 + d);
    *bit = (run >> (nb - 1 - d)) & 1u;
    return TAU_NM + nm_off(nb) + (int)ctx - 1;
}

// The CLASS (update rates, blend weights) and the coded bit of a run's k-th decision — what the probability stream needs; the type itself
// (which tree node) only matters to the partition.  Same case analysis as nth_decision without the node arithmetic
// (tools/devcoder_sim.cpp checks tau_class(nth_decision(...)) == nth_class(...) and the bits on every run it walks).
DC_HD int nth_class(const Item& it, int max_rank, int n_rank, int k, uint32_t* bit, bool* run_side)
{
    if (k < n_rank) {
        const uint32_t rank = it.rank;
        *run_side = false;
        if (it.ge32) { *bit = (rank >> (max_rank - k)) & 1u; return CLS_RP; }
        if (k == 0) { *bit = rank != 1u ? 1u : 0u; return CLS_RF; }
        const int B = bsr(rank);
        const int e = (B - 1) + (B < max_rank ? 1 : 0);
        if (k <= e) { *bit = k < B ? 1u : 0u; return CLS_RE; }
        *bit = (rank >> (B - 1 - (k - 1 - e))) & 1u;
        return CLS_RM;
    }
    const int kk = k - n_rank;
    const uint32_t run = it.run;
    *run_side = true;
    if (kk == 0) { *bit = run != 1u ? 1u : 0u; return CLS_NF; }
    const int nb = bsr(run);
    if (kk <= nb) { *bit = kk < nb ? 1u : 0u; return CLS_NE; }
    *bit = (run >> (nb - 1 - (kk - 1 - nb))) & 1u;
    return nb <= 5 ? CLS_NM : CLS_NM2;
}

// ---- counters --------------------------------------------------------------------------------------------------------
// predictor.h:53-61 with the family's tuned constants: bit 0 moves towards 4096 - th0, bit 1 towards th1 (arithmetic shifts)
// One form for both coders: v <- v + (((t_bit - v) * a_bit + r_bit) >> 12), arithmetic shift.
//   static coder (-e1): bit 0 moves towards t0 = 4096 - th0 with r0 = 0; bit 1 is v - (((v - t1) a1) >> 12), which is the same as
//                       v + (((t1 - v) a1 + 4095) >> 12) (minus the floor of a quotient = the ceiling of its negation): r1 = 4095;
//   fast coder (-e0):   p -= (p - target_bit) >> R (qlfc.cpp:1186-1331, shifts of 4..7) = v + ceil((target - v) / 2^R)
//                       = v + (((target - v) * 2^(12-R) + 4095) >> 12): a = 2^(12-R), r0 = r1 = 4095.
struct Rates { int t0, a0, t1, a1, r0, r1; };
DC_HD int step(int v, uint32_t bit, const Rates& R)
{
#if defined(__HIP_DEVICE_COMPILE__)
    // both directions with the full-rate 24-bit multiply (|t - v| < 2^14, rates < 2^11: exact), then one select: the plain form
    // compiles to two exec-masked branches around quarter-rate 32-bit multiplies, twice the cycles of this on the serial chains
    const int up = v + ((__mul24(R.t0 - v, R.a0) + R.r0) >> 12);
    const int dn = v + ((__mul24(R.t1 - v, R.a1) + R.r1) >> 12);
    return bit ? dn : up;
#else
    return bit ? v + (((R.t1 - v) * R.a1 + R.r1) >> 12) : v + (((R.t0 - v) * R.a0 + R.r0) >> 12);
#endif
}

// Everything the kernels need from the tuned tables (filled on the host from qlfc_data.inc, passed by value).
struct ModelParams {
    Rates   rates[NUM_CLS][3];                               // [class][family]
    short   lr[NUM_CLS][3];                                  // blend weights: p = (ch * lr[0] + st * lr[1] + static * lr[2]) >> 5
    short   vmin[NUM_CLS][3], vmax[NUM_CLS][3];              // attainable counter range from the start value (tight two-sided brackets)
    short   init[NUM_CLS];                                   // value a chain starts from (2048; fast coder: 4096 rank side, 1024 run side)
};
// attainable range: closure of {init} under both maps (monotone maps -> an interval)
inline void model_closure(const Rates& R, int init, short* vmin, short* vmax)
{
    int lo = init, hi = init;
    for (bool grown = true; grown;) {
        grown = false;
        for (int s = lo; s <= hi; ++s) for (uint32_t b = 0; b < 2; ++b) {
            const int w = step(s, b, R);
            if (w < lo) { lo = w; grown = true; }
            if (w > hi) { hi = w; grown = true; }
        }
    }
    *vmin = (short)lo; *vmax = (short)hi;
}
// kStaticParams row layout (tools/gen_qlfc_data.py): S{th0,ar0,th1,ar1} C{...} P{...} mixer{4} LR0 LR1 LR2
inline void model_params_from_table(const short (*P)[19], ModelParams& M)
{
    for (int c = 0; c < NUM_CLS; ++c) {
        const int pc = c == CLS_NM2 ? CLS_NM : c;             // the table has one row for all run-length mantissas
        for (int f = 0; f < 3; ++f) {
            Rates& R = M.rates[c][f];
            R.t0 = 4096 - P[pc][4 * f + 0]; R.a0 = P[pc][4 * f + 1]; R.t1 = P[pc][4 * f + 2]; R.a1 = P[pc][4 * f + 3];
            R.r0 = 0; R.r1 = 4095;
            model_closure(R, 2048, &M.vmin[c][f], &M.vmax[c][f]);
        }
        M.lr[c][0] = P[pc][16]; M.lr[c][1] = P[pc][17]; M.lr[c][2] = P[pc][18];
        M.init[c] = 2048;
    }
}
// The fast coder (-e0, qlfc.cpp:1135-1336): ONE counter per decision, indexed by the run's symbol — the chains of the char family
// with other update maps (shifts instead of multiplications, targets per class and bit, qlfc.cpp:1186-1331; initial values
// qlfc_model.cpp:74-75) and nothing to blend.  Only [class][FAM_CHAR] is used; RP (escape coding) does not exist in this coder.
inline void model_params_fast(ModelParams& M)
{
    //                           RF     RE     RM     RP     NF     NE     NM    NM2
    static const short T0[] = {8016,  8114,  7999,  7999,  2025,  1962,  1951,  1987};     // target of a coded 0
    static const short T1[] = {  83,   122,   235,   235,    42,   142,   147,    46};     // target of a coded 1
    static const short S0[] = {   4,     4,     7,     7,     5,     4,     6,     5};     // shift (RF / NF: both bits the same)
    for (int c = 0; c < NUM_CLS; ++c) {
        for (int f = 0; f < 3; ++f) {
            Rates& R = M.rates[c][f];
            R.t0 = T0[c]; R.t1 = T1[c]; R.a0 = R.a1 = 1 << (12 - S0[c]); R.r0 = R.r1 = 4095;
            M.init[c] = (short)(c < CLS_NF ? 4096 : 1024);
            model_closure(R, M.init[c], &M.vmin[c][f], &M.vmax[c][f]);
            M.lr[c][f] = 0;
        }
    }
}
// ---- the adaptive coder (-e2, qlfc.cpp:583-819) ------------------------------------------------------------------------------------
// Its decisions, contexts and three counter families are the static coder's, decision for decision, with the rates of kAdaptiveParams
// (same 19-column rows: model_params_from_table reads either table).  What differs is the probability: not a fixed blend of the three
// counter values but the output of a ProbabilityMixer (predictor.h:74-213), one of 1896 instances per sub-block.  Counters never depend
// on a mixer's output, so a mixer instance is one more independent chain, (sub-block, mixer id), over its decisions in stream order.
// (columns 16..18 of this table are the mixer's learning rates, not blend weights: the blend is left at zero, so that the static model's
// stream kernel writes the coded bit and the run-start mark of every decision around an empty probability field)
inline void model_params_adaptive(const short (*P)[19], ModelParams& M)
{
    model_params_from_table(P, M);
    for (int c = 0; c < NUM_CLS; ++c) M.lr[c][0] = M.lr[c][1] = M.lr[c][2] = 0;
}

// mixer ids in the order of the reference's member arrays (qlfc_model.h): which instance a decision uses is a pure function of the run
//   RF  rank[c]                              c: the run's symbol
//   RE  rank_exp[max(hist, b)][b]            b: 1-based position, hist: rank_hist[c] before this run (0..7)
//   RM  rank_mant[B]                         B = bsr(rank): one mixer for all nodes of the tree
//   RP  rank_esc[ctx]                        the tree node
//   NF  run[c]
//   NE  run_exp[max(hist, b)][b]             hist: run_hist[c] before this run, NOT clamped to 7 (0..31)
//   NM  run_mant[bits]                       bits = bsr(run)
constexpr int MIX_RF = 0, MIX_RE = 256, MIX_RM = 320, MIX_RP = 328, MIX_NF = 584, MIX_NE = 840, MIX_NM = 1864, NUM_MIX = 1896;
constexpr int MIX_BITS = 11;
static_assert(NUM_MIX <= (1 << MIX_BITS), "a mixer id fits 11 bits");
DC_HD int mix_re(int hist, int b) { return MIX_RE + ((hist > b ? hist : b) & 7) * 8 + b; }
DC_HD int mix_ne(int hist, int b) { return MIX_NE + ((hist > b ? hist : b) & 31) * 32 + b; }
DC_HD int mixer_class(int id)
{
    return id < MIX_RE ? CLS_RF : id < MIX_RM ? CLS_RE : id < MIX_RP ? CLS_RM : id < MIX_NF ? CLS_RP : id < MIX_NE ? CLS_NF : id < MIX_NM ? CLS_NE : CLS_NM;
}
// The mixer id of a run's k-th decision (the case analysis of nth_class): c the run's symbol, rank_hist / run_hist the symbol's
// histories in front of this run (run_hist unclamped).
DC_HD int nth_mixer(const Item& it, int max_rank, int n_rank, int k, int c, int rank_hist, int run_hist)
{
    if (k < n_rank) {
        const uint32_t rank = it.rank;
        if (it.ge32) return MIX_RP + (int)((1u << k) | ((rank >> (max_rank + 1 - k)) & ((1u << k) - 1u)));
        if (k == 0) return MIX_RF + c;
        const int B = bsr(rank);
        const int e = (B - 1) + (B < max_rank ? 1 : 0);
        return k <= e ? mix_re(rank_hist, k) : MIX_RM + B;
    }
    const int kk = k - n_rank;
    if (kk == 0) return MIX_NF + c;
    const int nb = bsr(it.run);
    return kk <= nb ? mix_ne(run_hist, kk) : MIX_NM + nb;
}

// One mixer instance and its step (predictor.h:121-183).  The reference's `int` arithmetic overflows on some inputs; what its binary
// computes is the two's-complement wrap, so the weighted sum and the weight updates are spelled in uint32_t with the same casts.
// P: the class's row of kAdaptiveParams — MixParams keeps its columns 12..18.
struct MixParams { short th0, ar0, th1, ar1, lr0, lr1, lr2, pad; };
inline void mix_params_from_table(const short (*P)[19], MixParams* out /* [NUM_CLS] */)
{
    for (int c = 0; c < NUM_CLS; ++c) {
        const short* r = P[c == CLS_NM2 ? CLS_NM : c];
        out[c] = MixParams{r[12], r[13], r[14], r[15], r[16], r[17], r[18], 0};
    }
}
struct MixerState { int32_t w0, w1, w2; short map[17]; };
DC_HD void mixer_init(MixerState& M, const short* squash)
{
    M.w0 = M.w1 = 2048 << 5; M.w2 = 0;
    for (int p = 0; p < 17; ++p) M.map[p] = squash[2048 + (p - 8) * 256];
}
DC_HD int mix_wmul(int a, int b) { return (int)((uint32_t)a * (uint32_t)b); }
DC_HD short mix_bump(short p, uint32_t bit, const MixParams& P)
{
    const int up = ((4096 - P.th0 - p) * P.ar0) >> 12, down = ((p - P.th1) * P.ar1) >> 12;
    return (short)(p + (bit ? -down : up));
}
// the stretched sum, clamped: the index of the squash table and of the interpolated map
DC_HD int mixer_dot(int s0, int s1, int s2, int w0, int w1, int w2)
{
    int d = (short)((int)((uint32_t)mix_wmul(s0, w0) + (uint32_t)mix_wmul(s1, w1) + (uint32_t)mix_wmul(s2, w2)) >> 17);
    return d < -2047 ? -2047 : d > 2047 ? 2047 : d;
}
// p_ch / p_st / p_sp: the char-, state- and position-indexed counter values BEFORE their update; returns the 12-bit probability.
// The weights and the 17-cell map wherever the caller keeps them (MixerState on the host, registers and an LDS row on the device).
template <class MapP, class TabP>
DC_HD int mixer_step_on(int32_t& w0, int32_t& w1, int32_t& w2, MapP map, const MixParams& P, TabP stretch, TabP squash, int p_ch, int p_st, int p_sp, uint32_t bit)
{
    const int s0 = stretch[p_ch], s1 = stretch[p_st], s2 = stretch[p_sp];
    const int d = mixer_dot(s0, s1, s2, w0, w1, w2);
    const int frac = d & 255, idx = (d + 2048) >> 8;
    const int m0 = map[idx], m1 = map[idx + 1];
    const int p = (3 * squash[2048 + d] + m0 + (((m1 - m0) * frac) >> 8)) >> 2;
    map[idx] = mix_bump((short)m0, bit, P); map[idx + 1] = mix_bump((short)m1, bit, P);
    const int eps = p - (bit ? 1 : 4095);
    w0 = (int32_t)((uint32_t)w0 - (uint32_t)(mix_wmul(mix_wmul(P.lr0, eps), s0) >> 16));
    w1 = (int32_t)((uint32_t)w1 - (uint32_t)(mix_wmul(mix_wmul(P.lr1, eps), s1) >> 16));
    w2 = (int32_t)((uint32_t)w2 - (uint32_t)(mix_wmul(mix_wmul(P.lr2, eps), s2) >> 16));
    return p;
}
DC_HD int mixer_step(MixerState& M, const MixParams& P, const short* stretch, const short* squash, int p_ch, int p_st, int p_sp, uint32_t bit)
{
    return mixer_step_on(M.w0, M.w1, M.w2, (short*)M.map, P, stretch, squash, p_ch, p_st, p_sp, bit);
}

DC_HD int blend(int v_char, int v_state, int v_static, const short* lr)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return (__mul24(v_char, lr[0]) + __mul24(v_state, lr[1]) + __mul24(v_static, lr[2])) >> 5;
#else
    return (v_char * lr[0] + v_state * lr[1] + v_static * lr[2]) >> 5;
#endif
}

// ---- contexts of a run (qlfc.cpp:896-903, :978-989, :1063-1068) -------------------------------------------------------
DC_HD uint32_t avg_rank_next(uint32_t avg, uint32_t rank) { return (avg * 124u + rank * 4u) >> 7; }
DC_HD uint32_t run_hist_next(uint32_t h, uint32_t run) { return run == 1u ? (h + 2u) >> 2 : (h + 3u * (uint32_t)bsr(run) + 3u) >> 2; }
// window contexts from the previous runs of the same sub-block (prev[0] = run j-1, ...; absent runs contribute zero bits)
DC_HD uint32_t rank_state_index(uint32_t ctx_run, uint32_t ctx_rank4, uint32_t rank_hist) { return (ctx_run << 11) | (ctx_rank4 << 3) | rank_hist; }
DC_HD uint32_t run_state_index(uint32_t ctx_rank0, uint32_t ctx_run, uint32_t rank, uint32_t run_hist)
{
    const uint32_t r1 = rank - 1u;
    return (ctx_rank0 << 10) | (ctx_run << 6) | ((r1 < 7u ? r1 : 7u) << 3) | (run_hist < 7u ? run_hist : 7u);
}

// ---- sizes of the device walk that decide which exit a block takes ------------------------------------------------------
// (devcoder.hip walks by them; tools/devcoder_paths_probe.cpp predicts from them, on the CPU, which exits a given block must take)
#ifndef DC_EV_N
#define DC_EV_N 8192
#endif
constexpr int DC_EV          = DC_EV_N;  // events per evaluation chunk: the minimum (see dc_eval: long enough for the brackets to meet)
constexpr int DC_EVAL_WAVES_TARGET = 1000;   // ... or as many as keep a block's evaluation at this many wavefronts of 64 chunks
constexpr int DC_EB          = 64;       // events per lane per batch of the evaluation walk (chunks are whole batches)
constexpr int DC_REPLAY_MAX  = 64;       // chunks a serial replay walks back before the block is declined (FAIL_REPLAY)
constexpr int DC_RP_CAND     = 384;      // exact resolve of open chunk starts: start values a chunk is walked from, six per lane of a wavefront (the
                                         // bracket behind DC_EV events is at most 373 wide for the static coder's slowest rate, 11 / 4096, and 128 for
                                         // the fast coder's: tools/replay_resolve_probe.cpp bound; a wider one is not walked)
constexpr uint32_t DC_SIGMASK = 0x7ffu;  // chain-major event = X | sub-block << 8 | bit << 11: the bits that name the chain inside a row
constexpr uint32_t DC_ROWMARK = 0x1000u; // ... and the mark of an event that starts a chain whatever its signature (dc_mark_rows_kernel, dc_mark_chains_kernel)
constexpr int DC_ROWS        = 1088;     // rows of the chain-major layout = decision types (NUM_TAU = 1080), padded to whole wavefronts
constexpr int DC_AVG_CH      = 1024;     // runs per avg_rank lane
constexpr int DC_AVG_WARM    = 768;      // warm-up runs in front of an avg_rank chunk
constexpr int DC_AVG_CAND    = 64;       // exact resolve: start values a lane's chunk is walked from, one per lane of a wavefront (the bracket
                                         // behind DC_AVG_WARM runs is at most 32 wide: 33 candidates; a wider one is not resolved)
constexpr int DC_AVG_GROUP   = 64;       // exact resolve: consecutive chunks whose transfer maps one wavefront composes
constexpr uint32_t DC_AVG_UNKNOWN = 0xffffu;   // exact resolve: a chunk's start value behind a bracket too wide to walk (the guard)
constexpr int DC_HIST_NP     = 9;        // predecessors of a run's symbol that the run_hist bracket always walks
constexpr int DC_HIST_KMAX   = 4096;     // the extended look-back quadruples from 4 DC_HIST_NP and gives up (FAIL_HIST) at the first K >= this
// events per evaluation chunk of a block with Etot events over all jobs
inline uint32_t eval_chunk_events(uint64_t Etot)
{
    uint64_t ev = (Etot + 64ull * DC_EVAL_WAVES_TARGET - 1) / (64ull * DC_EVAL_WAVES_TARGET);
    ev = (ev + DC_EB - 1) / DC_EB * DC_EB;
    return ev < (uint64_t)DC_EV ? (uint32_t)DC_EV : (uint32_t)ev;
}

// ---- avg_rank flags resolved exactly (devcoder.hip 1a': dc_avg_map_kernel .. dc_avg_fix_kernel), restated for the host -------------------
// rank[0 .. m): the ranks of the runs; first_run[0 .. nsub]: first run of every sub-block (strictly increasing, first_run[nsub] = m);
// top[s]: upper end a bracket inside sub-block s starts from (255, or 2^(max_rank + 1) - 1 for a table).  The same steps in the same
// order as the kernels: (1) every chunk of DC_AVG_CH runs walks its bracket from DC_AVG_WARM runs early, notes the bracket at its first
// run (lo0, hi0), writes the lower end's flags and counts the runs whose ends disagree; (2) a chunk whose successor starts open is
// walked from every value of its own start bracket: its transfer map; (3) the maps of DC_AVG_GROUP chunks are composed, the groups
// chained, every chunk handed its exact start (a closed bracket and a sub-block start inside a chunk restart the chain); (4) a chunk
// with open flags is walked again from its exact start.  A bracket of DC_AVG_CAND values or more is not walked: what follows it stays
// DC_AVG_UNKNOWN until the chain restarts, and the open flags of such chunks are `left`.
struct AvgResolve {
    uint64_t und = 0, resolved = 0, left = 0;      // flags the bracket left open; of those: settled exactly, not settled (the guard)
    uint32_t max_width = 0;                        // widest start bracket (hi0 - lo0) of any chunk
    uint32_t chain_steps = 0;                      // longest dependent path: steps inside a group + groups chained + steps inside a group
    std::vector<uint16_t> lo0, hi0, exact;         // per chunk
    std::vector<uint32_t> sub_left;                // per sub-block: flags left open
};
inline void avg_resolve_host(const uint8_t* rank, uint32_t m, const uint32_t* first_run, uint32_t nsub, const uint32_t* top, uint8_t* ge32, AvgResolve& R)
{
    const uint32_t nch = (m + DC_AVG_CH - 1) / DC_AVG_CH, ngr = (nch + DC_AVG_GROUP - 1) / DC_AVG_GROUP;
    R = AvgResolve();
    R.lo0.assign(nch, 0); R.hi0.assign(nch, 0); R.exact.assign(nch, 0); R.sub_left.assign(nsub, 0);
    std::vector<uint16_t> und(nch, 0);
    std::vector<uint8_t> has_start(nch, 0), map((size_t)nch * DC_AVG_CAND, 0);
    auto sb_of = [&](uint32_t j) { uint32_t s = 0; while (s + 1 < nsub && j >= first_run[s + 1]) ++s; return s; };
    auto open = [&](uint32_t c) { return R.lo0[c] != R.hi0[c]; };
    auto wide = [&](uint32_t c) { return (uint32_t)(R.hi0[c] - R.lo0[c]) >= (uint32_t)DC_AVG_CAND; };
    // (1) dc_avg_kernel
    for (uint32_t c = 0; c < nch; ++c) {
        const uint32_t j0 = c * DC_AVG_CH, j1 = j0 + DC_AVG_CH < m ? j0 + DC_AVG_CH : m;
        uint32_t sb = sb_of(j0);
        const uint32_t w0 = j0 > first_run[sb] + DC_AVG_WARM ? j0 - DC_AVG_WARM : first_run[sb];
        uint32_t lo = 0, hi = w0 == first_run[sb] ? 0u : top[sb];
        for (uint32_t j = w0; j < j0; ++j) { lo = avg_rank_next(lo, rank[j]); hi = avg_rank_next(hi, rank[j]); }
        R.lo0[c] = (uint16_t)lo; R.hi0[c] = (uint16_t)hi;
        if (hi - lo > R.max_width) R.max_width = hi - lo;
        for (uint32_t j = j0; j < j1; ++j) {
            if (sb + 1 < nsub && j == first_run[sb + 1]) { lo = hi = 0; ++sb; has_start[c] = 1; }
            und[c] += (lo >= 32u) != (hi >= 32u);
            ge32[j] = (uint8_t)(lo >= 32u);
            lo = avg_rank_next(lo, rank[j]); hi = avg_rank_next(hi, rank[j]);
        }
        R.und += und[c];
    }
    // (2) dc_avg_map_kernel
    for (uint32_t c = 0; c + 1 < nch; ++c) {
        if (!open(c + 1) || wide(c)) continue;
        const uint32_t j0 = c * DC_AVG_CH;
        for (uint32_t v = 0; v <= (uint32_t)(R.hi0[c] - R.lo0[c]); ++v) {
            uint32_t x = R.lo0[c] + v, sb = sb_of(j0);
            for (uint32_t j = j0; j < j0 + DC_AVG_CH; ++j) {
                if (sb + 1 < nsub && j == first_run[sb + 1]) { x = 0; ++sb; }
                x = avg_rank_next(x, rank[j]);
            }
            map[(size_t)c * DC_AVG_CAND + v] = (uint8_t)x;
        }
    }
    // the exact start of chunk c + 1 from that of chunk c (dc_avg_step)
    auto step = [&](uint32_t c, uint32_t x) -> uint32_t {
        if (!open(c + 1)) return R.lo0[c + 1];
        if (wide(c)) return DC_AVG_UNKNOWN;
        if (has_start[c]) return map[(size_t)c * DC_AVG_CAND];
        return x == DC_AVG_UNKNOWN ? DC_AVG_UNKNOWN : map[(size_t)c * DC_AVG_CAND + (x - R.lo0[c])];
    };
    // (3) dc_avg_chain_kernel<false>, dc_avg_groups_kernel, dc_avg_chain_kernel<true>
    std::vector<uint16_t> gmap((size_t)ngr * DC_AVG_CAND, 0), gstart(ngr, 0);
    uint32_t in_group = 0, across = 0, across_now = 0;
    for (uint32_t g = 0; g + 1 < ngr; ++g) {
        const uint32_t c0 = g * DC_AVG_GROUP;
        if (!open(c0 + DC_AVG_GROUP)) continue;
        for (uint32_t v = 0; v < (uint32_t)DC_AVG_CAND; ++v) {
            uint32_t x = (!wide(c0) && v <= (uint32_t)(R.hi0[c0] - R.lo0[c0])) ? R.lo0[c0] + v : DC_AVG_UNKNOWN;
            for (uint32_t c = c0; c < c0 + DC_AVG_GROUP; ++c) x = step(c, x);
            gmap[(size_t)g * DC_AVG_CAND + v] = (uint16_t)x;
        }
        in_group = DC_AVG_GROUP;
    }
    if (ngr) gstart[0] = R.lo0[0];
    for (uint32_t g = 0; g + 1 < ngr; ++g) {
        const uint32_t c0 = g * DC_AVG_GROUP, x = gstart[g];
        if (!open(c0 + DC_AVG_GROUP)) { gstart[g + 1] = R.lo0[c0 + DC_AVG_GROUP]; across_now = 0; continue; }
        gstart[g + 1] = (x == DC_AVG_UNKNOWN || wide(c0)) ? (uint16_t)DC_AVG_UNKNOWN : gmap[(size_t)g * DC_AVG_CAND + (x - R.lo0[c0])];
        if (++across_now > across) across = across_now;
    }
    for (uint32_t g = 0; g < ngr; ++g) {
        uint32_t x = gstart[g];
        for (uint32_t c = g * DC_AVG_GROUP; c < nch && c < (g + 1) * DC_AVG_GROUP; ++c) {
            R.exact[c] = (uint16_t)x;
            if (c + 1 == nch) break;
            if (open(c + 1) && c % DC_AVG_GROUP + 1 > in_group) in_group = c % DC_AVG_GROUP + 1;
            x = step(c, x);
        }
    }
    R.chain_steps = across ? 2 * DC_AVG_GROUP + across : in_group;
    // (4) dc_avg_fix_kernel
    for (uint32_t c = 0; c < nch; ++c) {
        if (!und[c]) continue;
        const uint32_t j0 = c * DC_AVG_CH, j1 = j0 + DC_AVG_CH < m ? j0 + DC_AVG_CH : m;
        const bool known = R.exact[c] != DC_AVG_UNKNOWN;
        uint32_t lo = R.lo0[c], hi = R.hi0[c], x = known ? R.exact[c] : lo, sb = sb_of(j0);
        for (uint32_t j = j0; j < j1; ++j) {
            if (sb + 1 < nsub && j == first_run[sb + 1]) { lo = hi = x = 0; ++sb; }
            if (!known && (lo >= 32u) != (hi >= 32u)) ++R.sub_left[sb];
            ge32[j] = (uint8_t)(x >= 32u);
            lo = avg_rank_next(lo, rank[j]); hi = avg_rank_next(hi, rank[j]); x = avg_rank_next(x, rank[j]);
        }
        (known ? R.resolved : R.left) += und[c];
    }
}

// ---- open run_hist brackets resolved exactly (devcoder.hip 1c': dc_ctx_kernel<SB, true>, dc_hist_map_kernel .. dc_hist_fix_kernel), restated
// for the host ----------------------------------------------------------------------------------------------------------------------
// The runs in symbol-major order, as the stable sort by symbol leaves them: chain[q] names the chain of element q (symbol and sub-block:
// the elements of one chain are consecutive), run[q] is its length.  run_hist of element q is h over the chain's elements in front of
// it, h' = (h + run_hist_inc(run)) >> 2 from 0.  h -> h' is monotone and [0, 63] is invariant (the largest increment, 3 * 29 + 3 for a
// run of 2^30 bytes, gives (63 + 90) >> 2 = 38), so 64 start values cover whatever a chunk can start from and nothing needs a guard.  The
// same steps in the same order as the kernels: (1) every run walks the bracket [0, 63] over its DC_HIST_NP nearest predecessors (from 0
// where the chain starts among them); its clamped ends differ: the run is OPEN and keeps the lower end for now; (2) if anything is open,
// every whole chunk of DC_HIST_CH elements is walked from each of the 64 values, reset to 0 at every chain start: its transfer map;
// (3) the maps of DC_HIST_GROUP chunks are composed, the groups chained from 0, every chunk handed its exact start; (4) a chunk that
// holds an open run is walked again from its exact start and every open run takes its min(h, 7).
constexpr int DC_HIST_CH     = 1024;     // exact resolve: symbol-major elements per chunk — 16 per lane of the wavefront that walks it
constexpr int DC_HIST_CAND   = 64;       // ... start values a chunk is walked from, one per lane: all of [0, 63]
constexpr int DC_HIST_GROUP  = 64;       // ... consecutive chunks whose transfer maps one wavefront composes
static_assert(DC_HIST_CH == DC_AVG_CH && DC_HIST_CAND == DC_AVG_CAND && DC_HIST_GROUP == DC_AVG_GROUP, "the two resolves share their chain and groups kernels");
DC_HD uint32_t run_hist_inc(uint32_t run) { return run == 1u ? 2u : 3u * (uint32_t)bsr(run) + 3u; }      // run_hist_next(h, run) = (h + run_hist_inc(run)) >> 2
struct HistResolve {
    uint64_t ext = 0, resolved = 0;                // runs whose bracket the nine predecessors left open; of those: settled by the resolve
    uint32_t chunks = 0, groups = 0;               // chunks that hold an open run; groups of chunks in the launch
    uint32_t chain_steps = 0;                      // longest dependent path: steps inside a group + groups chained + steps inside a group
    std::vector<uint8_t> hist, open;               // per element: min(run_hist, 7) as the stage leaves it; whether (1) left it open
};
inline void hist_resolve_host(const uint64_t* chain, const uint32_t* run, uint32_t m, HistResolve& R)
{
    const uint32_t nch = (m + DC_HIST_CH - 1) / DC_HIST_CH, ngr = (nch + DC_HIST_GROUP - 1) / DC_HIST_GROUP;
    R = HistResolve();
    R.hist.assign(m, 0); R.open.assign(m, 0); R.groups = ngr;
    std::vector<uint8_t> flag(nch, 0);
    auto starts = [&](uint32_t q) { return q == 0 || chain[q] != chain[q - 1]; };
    // (1) dc_ctx_kernel<SB, true>
    for (uint32_t q = 0; q < m; ++q) {
        uint32_t np = 0;
        while (np < (uint32_t)DC_HIST_NP && q > np && chain[q - np - 1] == chain[q]) ++np;
        uint32_t lo = 0, hi = np < (uint32_t)DC_HIST_NP ? 0u : 63u;
        for (uint32_t t = np; t >= 1; --t) { lo = run_hist_next(lo, run[q - t]); hi = run_hist_next(hi, run[q - t]); }
        const uint32_t cl = lo < 7u ? lo : 7u, ch = hi < 7u ? hi : 7u;
        R.hist[q] = (uint8_t)cl;
        if (cl != ch) { ++R.ext; R.open[q] = 1; flag[q / DC_HIST_CH] = 1; }
    }
    if (R.ext == 0) return;                                           // (every kernel behind the first leaves at once)
    // (2) dc_hist_map_kernel: whole chunks only — the last chunk has no successor
    std::vector<uint8_t> map((size_t)nch * DC_HIST_CAND, 0);
    for (uint32_t c = 0; c + 1 < nch; ++c)
        for (uint32_t v = 0; v < (uint32_t)DC_HIST_CAND; ++v) {
            uint32_t x = v;
            for (uint32_t q = c * DC_HIST_CH; q < (c + 1) * DC_HIST_CH; ++q) { if (starts(q)) x = 0; x = (x + run_hist_inc(run[q])) >> 2; }
            map[(size_t)c * DC_HIST_CAND + v] = (uint8_t)x;
        }
    // (3) dc_avg_chain_kernel<false, DcHistRec>, dc_avg_groups_kernel<DcHistRec>, dc_avg_chain_kernel<true, DcHistRec>
    std::vector<uint8_t> gmap((size_t)ngr * DC_HIST_CAND, 0), gstart(ngr, 0), ex(nch, 0);
    for (uint32_t g = 0; g + 1 < ngr; ++g)
        for (uint32_t v = 0; v < (uint32_t)DC_HIST_CAND; ++v) {
            uint32_t x = v;
            for (uint32_t c = g * DC_HIST_GROUP; c < (g + 1) * DC_HIST_GROUP; ++c) x = map[(size_t)c * DC_HIST_CAND + x];
            gmap[(size_t)g * DC_HIST_CAND + v] = (uint8_t)x;
        }
    for (uint32_t g = 0; g + 1 < ngr; ++g) gstart[g + 1] = gmap[(size_t)g * DC_HIST_CAND + gstart[g]];      // (element 0 starts a chain: from 0)
    for (uint32_t g = 0; g < ngr; ++g) {
        uint32_t x = gstart[g];
        for (uint32_t c = g * DC_HIST_GROUP; c < nch && c < (g + 1) * DC_HIST_GROUP; ++c) { ex[c] = (uint8_t)x; x = map[(size_t)c * DC_HIST_CAND + x]; }
    }
    R.chain_steps = ngr > 1 ? 2 * DC_HIST_GROUP + (ngr - 1) : nch - 1;
    // (4) dc_hist_fix_kernel
    for (uint32_t c = 0; c < nch; ++c) {
        if (!flag[c]) continue;
        ++R.chunks;
        uint32_t x = ex[c];
        for (uint32_t q = c * DC_HIST_CH; q < m && q < (c + 1) * DC_HIST_CH; ++q) {
            if (starts(q)) x = 0;
            if (R.open[q]) { R.hist[q] = (uint8_t)(x < 7u ? x : 7u); ++R.resolved; }
            x = (x + run_hist_inc(run[q])) >> 2;
        }
    }
}

// ---- open chunk starts resolved exactly (devcoder.hip 3': dc_rp_map_kernel, dc_rp_chain_kernel), restated for the host -------------------
// The evaluation of one unit as dc_eval has it: up to four jobs of chain-major events (row = decision type, rowstart[0 .. DC_ROWS]; the
// first event of every non-empty row and every other chain start the signature does not show carry DC_ROWMARK already), EV events per
// chunk, the chunks of job q in slots cstart[q] .. (padded to whole wavefronts, as on the device).  The same steps in the same order as
// the kernels: (1) dc_eval_wave_kernel<false>: every chunk walks the bracket [vmin, vmax] of its first row's class to its end
// (elo, ehi), both ends reset wherever a chain starts; (2) chunk c is OPEN iff it continues the chain of the event before it and the
// bracket of chunk c - 1 has not met; a STRETCH is a maximal run of open chunks c0 + 1 .. ck + 1, its HEAD c0 starts from a known value;
// (3) dc_rp_map_kernel: a chunk whose successor is open is walked — the head from its one start (head end), every other one from
// every value elo[p - 1] + v of its start bracket: map[p][v] = end - elo[p] — unless that bracket has more than `cand` values (the
// guard: state WIDE); (4) dc_rp_chain_kernel: per stretch the exact starts follow from the maps in order and close the brackets
// (elo[p] = ehi[p] = exact start of p + 1), up to the first WIDE chunk; (5) dc_eval_b_kernel: the start of every chunk — the chain's
// initial value, the closed bracket in front of it, or a serial replay from the nearest known start (`replays` chunks walked; more than
// DC_REPLAY_MAX back: fail_replay).  resolve false: steps 3 and 4 are left out — today's path.
enum : uint8_t { DC_RP_NONE = 0, DC_RP_HEAD = 1, DC_RP_MAP = 2, DC_RP_WIDE = 3 };      // per chunk: what dc_rp_map_kernel left for the chain
struct ReplayJob { const uint16_t* events; uint32_t E; const uint32_t* rowstart; int fam; };
struct ReplayResolve {
    uint32_t ev = 0, cstart[5] = {0, 0, 0, 0, 0};
    uint32_t open = 0;                             // chunks that start inside a chain behind a bracket that has not met
    uint32_t resolved = 0;                         // of those: start settled by the resolve (DM_REPLAY_RESOLVED)
    uint32_t replays = 0;                          // chunks walked again serially (DM_REPLAYS)
    bool     fail_replay = false;
    uint32_t stretches = 0, longest = 0;           // stretches, and the open chunks of the longest
    uint32_t max_width = 0;                        // widest start bracket (values) of an open chunk
    uint32_t wide = 0;                             // chunks the guard left unwalked
    std::vector<uint16_t> elo, ehi, start;         // per chunk slot: the bracket at its end (after step 4), the start value dc_eval_b_kernel hands it
    std::vector<uint8_t> known;                    // per chunk slot: start[] is set (a chunk behind a declined replay is not)
};
inline int class_first_row(int cls)
{
    return cls == CLS_RF ? TAU_RF : cls == CLS_RE ? TAU_RE : cls == CLS_RM ? TAU_RM : cls == CLS_RP ? TAU_RP : cls == CLS_NF ? TAU_NF
         : cls == CLS_NE ? TAU_NE : cls == CLS_NM ? TAU_NM : cls == CLS_NM2 ? TAU_NM2 : DC_ROWS;
}
inline uint32_t replay_find_row(const uint32_t* rowstart, uint32_t k)
{
    uint32_t lo = 0, hi = DC_ROWS;                                     // largest row with rowstart[row] <= k (dc_find_row)
    while (lo + 1 < hi) { const uint32_t mid = (lo + hi) >> 1; if (rowstart[mid] <= k) lo = mid; else hi = mid; }
    return lo;
}
inline bool replay_chunk_continues(const ReplayJob& J, uint32_t c, uint32_t EV)
{
    if (c == 0) return false;
    const uint32_t k0 = c * EV;
    if (J.rowstart[replay_find_row(J.rowstart, k0)] == k0) return false;
    const uint32_t e1 = J.events[k0];
    return ((((uint32_t)J.events[k0 - 1] ^ e1) & DC_SIGMASK) | (e1 & DC_ROWMARK)) == 0;
}
inline void replay_resolve_host(const ReplayJob* jobs /* [4] */, uint32_t EV, const ModelParams& M, uint32_t cand, bool resolve, ReplayResolve& R)
{
    R = ReplayResolve();
    R.ev = EV;
    for (int q = 0; q < 4; ++q) R.cstart[q + 1] = R.cstart[q] + ((jobs[q].E + EV - 1) / EV + 63) / 64 * 64;
    const uint32_t slots = R.cstart[4];
    R.elo.assign(slots, 0); R.ehi.assign(slots, 0); R.start.assign(slots, 0); R.known.assign(slots, 0);
    std::vector<uint8_t> st(slots, DC_RP_NONE);
    std::vector<uint16_t> head(slots, 0), map(resolve ? (size_t)slots * DC_RP_CAND : 0, 0);
    if (cand > (uint32_t)DC_RP_CAND) cand = DC_RP_CAND;
    for (int q = 0; q < 4; ++q) {
        const ReplayJob& J = jobs[q];
        if (J.E == 0) continue;
        const uint32_t nch = (J.E + EV - 1) / EV, s0 = R.cstart[q];
        uint16_t* elo = R.elo.data() + s0; uint16_t* ehi = R.ehi.data() + s0;
        auto cls_of = [&](uint32_t k) { return tau_class((int)replay_find_row(J.rowstart, k)); };
        auto is_open = [&](uint32_t c) { return c < nch && replay_chunk_continues(J, c, EV) && elo[c - 1] != ehi[c - 1]; };
        // a bare walk of n events from k: one chain, one set of rates (what the map kernel and the replay loop do)
        auto bare = [&](uint32_t k, uint32_t n, int v, const Rates& Rt) { for (uint32_t i = 0; i < n; ++i) v = step(v, ((uint32_t)J.events[k + i] >> 11) & 1u, Rt); return v; };
        // (1) dc_eval_wave_kernel<false>
        for (uint32_t c = 0; c < nch; ++c) {
            const uint32_t k0 = c * EV, k1 = k0 + EV < J.E ? k0 + EV : J.E;
            int cls = 0;
            while (cls + 1 < NUM_CLS && J.rowstart[class_first_row(cls + 1)] <= k0) ++cls;
            uint32_t clsend = J.rowstart[class_first_row(cls + 1)];
            uint32_t prev = k0 > 0 ? ((uint32_t)J.events[k0 - 1] & DC_SIGMASK) : 0xffffu;
            int lo = M.vmin[cls][J.fam], hi = M.vmax[cls][J.fam];
            for (uint32_t k = k0; k < k1; ++k) {
                while (k >= clsend && cls + 1 < NUM_CLS) { ++cls; clsend = J.rowstart[class_first_row(cls + 1)]; }
                const uint32_t e = J.events[k];
                if ((e & (DC_SIGMASK | DC_ROWMARK)) != prev) lo = hi = M.init[cls];
                prev = e & DC_SIGMASK;
                lo = step(lo, (e >> 11) & 1u, M.rates[cls][J.fam]); hi = step(hi, (e >> 11) & 1u, M.rates[cls][J.fam]);
            }
            elo[c] = (uint16_t)lo; ehi[c] = (uint16_t)hi;
        }
        // (2) the open chunks and their stretches
        for (uint32_t c = 1, run = 0; c <= nch; ++c) {
            if (is_open(c)) {
                ++R.open; ++run;
                const uint32_t w = (uint32_t)(ehi[c - 1] - elo[c - 1]) + 1u;
                if (w > R.max_width) R.max_width = w;
                if (run == 1) ++R.stretches;
                if (run > R.longest) R.longest = run;
            } else run = 0;
        }
        if (resolve) {
            // (3) dc_rp_map_kernel
            for (uint32_t p = 0; p + 1 < nch; ++p) {
                if (!is_open(p + 1)) continue;
                const Rates& Rt = M.rates[cls_of(p * EV)][J.fam];
                if (!is_open(p)) {                                     // (a head always continues a chain behind a closed bracket: see dc_rp_map_kernel)
                    const int s = replay_chunk_continues(J, p, EV) ? (int)elo[p - 1] : (int)M.init[cls_of(p * EV)];
                    head[s0 + p] = (uint16_t)bare(p * EV, EV, s, Rt);
                    st[s0 + p] = DC_RP_HEAD;
                    continue;
                }
                const uint32_t w = (uint32_t)(ehi[p - 1] - elo[p - 1]) + 1u;
                if (w > cand) { st[s0 + p] = DC_RP_WIDE; ++R.wide; continue; }
                for (uint32_t v = 0; v < w; ++v) map[(size_t)(s0 + p) * DC_RP_CAND + v] = (uint16_t)(bare(p * EV, EV, (int)elo[p - 1] + (int)v, Rt) - (int)elo[p]);
                st[s0 + p] = DC_RP_MAP;
            }
            // (4) dc_rp_chain_kernel: one walk per stretch, from its head
            for (uint32_t p0 = 0; p0 < nch; ++p0) {
                if (st[s0 + p0] != DC_RP_HEAD) continue;
                uint32_t x = head[s0 + p0], base = elo[p0];
                elo[p0] = ehi[p0] = (uint16_t)x; ++R.resolved;
                for (uint32_t p = p0 + 1; p < nch && st[s0 + p] == DC_RP_MAP; ++p) {
                    const uint32_t y = (uint32_t)elo[p] + map[(size_t)(s0 + p) * DC_RP_CAND + (x - base)];
                    base = elo[p];
                    elo[p] = ehi[p] = (uint16_t)y; ++R.resolved;
                    x = y;
                }
            }
        }
        // (5) dc_eval_b_kernel
        for (uint32_t c = 0; c < nch; ++c) {
            const int init_c = M.init[cls_of(c * EV)];
            R.known[s0 + c] = 1;
            if (!replay_chunk_continues(J, c, EV)) { R.start[s0 + c] = (uint16_t)init_c; continue; }
            if (elo[c - 1] == ehi[c - 1]) { R.start[s0 + c] = elo[c - 1]; continue; }
            uint32_t j = c - 1, depth = 1;
            int s = init_c;
            bool failed = false;
            for (;;) {
                if (!replay_chunk_continues(J, j, EV)) { s = init_c; break; }
                if (elo[j - 1] == ehi[j - 1]) { s = elo[j - 1]; break; }
                --j; ++depth;
                if (depth > (uint32_t)DC_REPLAY_MAX) { failed = true; break; }
            }
            if (failed) { R.fail_replay = true; R.known[s0 + c] = 0; continue; }
            R.replays += depth;
            R.start[s0 + c] = (uint16_t)bare(j * EV, (c - j) * EV, s, M.rates[cls_of(j * EV)][J.fam]);
        }
    }
}

// p-stream entry handed to the range coder: [11:0] probability, [12] bit, [13] first decision of a run
constexpr uint16_t PS_BIT = 1u << 12, PS_RUN = 1u << 13;
// ... of the fast coder: [12:0] probability (13 bits on the rank side, 11 on the run side), [13] bit, [14] first decision of a run,
// [15] run side (the range coder's precision follows it: qlfc.cpp:1186 / :1259)
constexpr uint16_t PSF_BIT = 1u << 13, PSF_RUN = 1u << 14, PSF_SIDE = 1u << 15;

}  // namespace dcm
