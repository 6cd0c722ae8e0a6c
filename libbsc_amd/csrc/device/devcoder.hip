// devcoder.hip — the adaptive model of the static QLFC coder (-e1) on MI355X: every probability the range coder will
// need, computed on the GPU, so that the host is left with the range coder's own carry chain and nothing else.
//
// The reference codes a sub-block as ONE serial loop (libbsc/coder/qlfc/qlfc.cpp:829-1129): per run ~7 binary decisions,
// each predicted from three adaptive counters and coded at once.  The counters, though, are independent chains (see
// devcoder_model.h): chain = (sub-block, decision type, family, X), v <- step(v, bit) over the chain's decisions in stream
// order.  This file lays the decisions of a whole block (8 sub-blocks, ~2e8 decisions for 64 MiB of text) out chain by
// chain and walks all chains in parallel (a batched pass of small blocks, up to 8192 sub-blocks, goes through the same kernels
// instantiated for a sub-block table: DcForm below, devcoder_pstream_batch):
//
//   1. contexts      avg_rank >= 32 flags (two-sided bracket walk with warm-up), per-run packed items; a stable 8-bit
//                    radix pass by symbol gives the symbol-major order in which "previous run of the same symbol"
//                    (rank_hist / run_hist, qlfc.cpp:900, :981-987) is the neighbouring element (run_hist: a bracket over the
//                    nine nearest such runs, then a longer look-back or, with BSCGPU_OPT_DC_HIST_EXACT, the exact resolve 1c'); context states from the
//                    reference's two state tables; two more radix passes order the runs by rank-state and by run-state.
//   2. partition     for each family (static: stream order; char: symbol-major; state: state-major) the decisions of the
//                    runs, generated on the fly round by round (64 runs per wavefront, ballot-match ranking, no atomics on
//                    the order-defining path), are scattered into chain-major order: row = decision type, inside a row
//                    X-major, inside that stream order.  Each decision also records where it went (pos).
//   3. evaluation    8192-event chunks, one lane each.  A chunk that starts inside a chain does not know the chain's value
//                    there, but the counter maps are monotone, so running them from the two ends of the attainable range
//                    brackets the truth, and once the two trajectories meet everything after is exact (chunks are long
//                    enough that they nearly always meet; a chunk whose predecessor did not coalesce replays it serially —
//                    exactness never depends on luck).  Second walk with the exact start values writes the counter value
//                    every decision sees.
//   4. p stream      back in stream order: gather the three values of every decision through pos, blend (predictor.h:121),
//                    emit 16 bits per decision: probability, coded bit, start-of-run mark.
//
// The host (qlfc.cpp: encode_from_pstream) then runs only the range coder.  Whenever something is outside what this path
// handles exactly (an avg_rank bracket that does not decide — unless BSCGPU_OPT_DC_AVG_EXACT has the open flags computed exactly,
// 1a' —, a run_hist bracket still open after 9216 predecessors — unless BSCGPU_OPT_DC_HIST_EXACT has the open brackets computed
// exactly, 1c', which leaves none —, a chain whose
// bracket stays open over more than 64 evaluation chunks — unless BSCGPU_OPT_DC_REPLAY_EXACT has the open chunk starts computed
// exactly, 3' —, capacity), a flag is raised and the caller falls back to the host model;
// nothing approximate is ever emitted.
//
// The host side drives the stages from ONE body per coder, a template over the form as the kernels are: dc_static_run (-e1) and
// dc_fast_run (-e0).  devcoder_pstream (a block), devcoder_pstream_batch (a pass) and devcoder_pstream_segments (a pass cut at
// capacity) hold what differs in front of a body: the sub-blocks' shape, the avg_rank flags, the table's max_rank, the rebased table.
// The adaptive coder (-e2) of a whole pass, or of a model segment of one, is dc_static_run with its own rates and, behind it, one walk
// per mixer chain (dc_mix_run); the segment plan of such a pass has a third fact, every sub-block's longest chain (dc_mix_facts_kernel).
#include "dev_common.h"
#include "dma_copy.h"
#include <thread>
#include <system_error>
#include "devcoder_model.h"
#include "dc_segment_plan.h"
#include "../host/qlfc.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <vector>
#include <type_traits>

using namespace dcm;

// Run-parallel kernels that gather (dc_ctx: the symbol-major neighbours; dc_pstream: the chain-major counter values) can give every
// XCD one contiguous eighth of the runs instead of every eighth workgroup (block b runs on XCD b % 8), so that a line of the gathered
// arrays is fetched by one XCD's L2 only.  Measured on the 64 MiB bench block (same box, round 3): dc_pstream 3.10 against 2.92 ms,
// dc_ctx 1.44 against 1.41 ms — no gain (the lines are mostly consumed by one workgroup or its neighbour in time, and eight
// separate streams per array cost more than the shared fetches save); kept as an A/B switch, off.
#ifndef DC_XCD_RANGES
#define DC_XCD_RANGES 0
#endif
__device__ __forceinline__ u32 dc_virtual_block() {
    if (!DC_XCD_RANGES) return blockIdx.x;
    return (blockIdx.x & 7u) * (gridDim.x >> 3) + (blockIdx.x >> 3);
}

constexpr int DC_WCH_MAX  = 4096;      // wave-chunks of a partition job (one wavefront walks one chunk of runs)
// (DC_EV, DC_AVG_CH, DC_AVG_WARM, DC_HIST_NP, DC_HIST_KMAX, DC_REPLAY_MAX: devcoder_model.h — the CPU probe of the exits shares them; so
// are DC_SIGMASK (event = X | sub-block << 8 | bit << 11), DC_ROWMARK and DC_ROWS, which the host restatement of the evaluation reads)

// meta scalars (device u32 array)
enum { DM_FAIL = 0, DM_NTYPES, DM_NROUNDS, DM_AVG_UND, DM_REPLAYS, DM_D0, DM_D1, DM_D2, DM_D3, DM_HIST_EXT /* runs that entered the extended run_hist look-back */, DM_P13_OVER /* a wavefront's piece did not fit the staging buffer: the packed stream is void */,
       DM_AVG_RESOLVED /* exact resolve: flags the bracket left open and the resolve settled */, DM_AVG_LEFT /* ... and did not (the guard) */,
       DM_REPLAY_RESOLVED /* open chunk starts the exact resolve settled (3') */,
       DM_HIST_RESOLVED /* runs whose open run_hist bracket the exact resolve settled (1c') */, DM_COUNT = 16 };
// (bit 0 is not in use: every decision type has a row of its own, DC_ROWS >= NUM_TAU, so no number of types is too many)
enum { FAIL_AVG = BSCGPU_DC_FAIL_AVG, FAIL_HIST = BSCGPU_DC_FAIL_HIST, FAIL_CAP = BSCGPU_DC_FAIL_CAP, FAIL_REPLAY = BSCGPU_DC_FAIL_REPLAY, FAIL_MIX = BSCGPU_DC_FAIL_MIX };
// the pinned host copy (DevCoder::hmeta, HM_WORDS words): the meta words in front, then what comes down beside them
enum { HM_POFF = 32 /* a block's poff[0..nb], 16 words */, HM_PBASE_END = 48 /* a table's pbase[nsub], the end of its packed layout */,
       HM_MIX = 50 /* the adaptive model's chains and the longest of them, 2 words */, HM_WORDS = 64 };
static_assert(DM_COUNT <= HM_POFF, "hmeta: the meta words end where the offsets begin");

struct DcSub { u32 nb; u32 first[9]; u32 maxr[8]; };           // run index range (first[nb] = m) and max_rank of each sub-block
struct DcRowBins { u16 lo1, hi1, lo2, hi2; };                   // counting pass: count(row) = P[hi1] - P[lo1] + P[hi2] - P[lo2] over bin prefix sums

// what the exact resolve of open avg_rank flags keeps per chunk of DC_AVG_CH runs and per group of DC_AVG_GROUP chunks (1a')
struct DcAvgRec {
    u16* brk;       // per chunk: lo0 | hi0 << 8, the bracket at the chunk's first run (equal where the warm-up reached the sub-block's first run)
    u16* und;       // per chunk: runs whose flag the bracket left open
    u8*  st;        // per chunk: DC_AVG_ST_*
    u16* ex;        // per chunk: the exact avg_rank at its first run, or DC_AVG_UNKNOWN
    u8*  map;       // per chunk, DC_AVG_CAND bytes: map[v] = avg_rank at the next chunk's first run, had this one started at lo0 + v
    u16* gmap;      // per group of DC_AVG_GROUP chunks, DC_AVG_CAND entries: the same across the group, from its first chunk's candidates
    u16* gstart;    // per group: the exact start of its first chunk
};

// what the exact resolve of open run_hist brackets keeps (1c'): per symbol-major element, per chunk of DC_HIST_CH elements and per group
// of DC_HIST_GROUP chunks; map, gmap, gstart and ex in the avg_rank resolve's format, whose chain and groups kernels walk them
struct DcHistRec {
    const u32* ext; // DM_HIST_EXT: runs the nine predecessors left open — zero: every kernel behind dc_ctx_kernel leaves at once
    u32* bits;      // per element: a bit, set where the run is open
    u8*  flag;      // per chunk: it holds an open run
    u64* scr;       // per open element: its run j << 13 | run_state_index with run_hist 0 (key_sn_s, which nobody writes before the
                    // run-state radix pass behind this stage)
    u16* ex;        // per chunk: run_hist in front of its first element
    u8*  map;       // per chunk, DC_HIST_CAND bytes: map[v] = run_hist in front of the next chunk's first element, had this one started at v
    u16* gmap;      // per group, DC_HIST_CAND entries: the same across the group
    u16* gstart;    // per group: the exact start of its first chunk
};

// what the exact resolve of open chunk starts keeps per chunk slot of the evaluation (3', in front of dc_rp_walk)
struct DcRpRec {
    u16* map;       // per chunk slot, DC_RP_CAND entries: map[v] = (value at the chunk's end, had it started at elo[p - 1] + v) - elo[p]
    u16* head;      // per chunk slot: the exact end of a stretch's head
    u8*  st;        // per chunk slot: DC_RP_*
    u32  cand;      // widest start bracket that is walked (values)
};

// One hipMalloc carved into 256-byte aligned pieces (dc_arena_alloc), made on the first use of what it serves.  failed: it did not
// fit, and is not tried again — what that means is its user's: see the five ensures.
struct DcArena { char* base = nullptr; size_t bytes = 0; bool failed = false; };

struct DevCoder {
    size_t Mcap = 0, Dcap = 0;                                 // runs and decisions a unit of model work may have (of max_n / BSCGPU_OPT_DC_ARENA_DIV)
    size_t Gcap = 0;                                           // runs of a whole block (of max_n): what ge32 holds
    DcArena arena;
    u64 *key_ch = nullptr, *key_ch_s = nullptr, *key_sr = nullptr, *key_sr_s = nullptr, *key_sn = nullptr, *key_sn_s = nullptr;
    u32 *inv_ch = nullptr, *inv_sr = nullptr, *inv_sn = nullptr;
    u8  *ge32 = nullptr;
    u32 *doff[4] = {nullptr, nullptr, nullptr, nullptr};       // per job: sp, ch, sr, sn
    u16 *events[4] = {nullptr, nullptr, nullptr, nullptr};     // per job, chain-major
    u32 *pos[4] = {nullptr, nullptr, nullptr, nullptr};        // per job: where each decision's event went
    u16 *V[4] = {nullptr, nullptr, nullptr, nullptr};          // per job: counter value seen by each event
    size_t nch_cap = 0;                                        // evaluation chunks per job (capacity)
    u16 *ps[2] = {nullptr, nullptr};                           // double buffer: block i's copy-out overlaps block i+1's kernels
    u32 *cnt = nullptr, *rowtot = nullptr, *rowstart = nullptr /*[4][257]*/, *wdec = nullptr, *wdecoff = nullptr;
    u16 *elo = nullptr, *ehi = nullptr, *S = nullptr;
    u32 *present = nullptr; u8 *rounds = nullptr; u32 *meta = nullptr; u32 *poff = nullptr;
    DcRowBins* rowbins = nullptr;                              // row -> bin ranges of the counting pass
    u16* sink = nullptr;                                       // where stores past the end of an array go (1 KB)
    u8  *tab_rank = nullptr, *tab_run = nullptr;
    ModelParams* mp = nullptr;                                 // device copy (static coder)
    ModelParams* mp_fast = nullptr;                            // device copy (fast coder: dcm::model_params_fast)
    struct DcFrag* frag = nullptr;                              // packed stream: two fragment records per wavefront of dc_pstream (DcP13)
    u32 *hmeta = nullptr;                                      // pinned, HM_WORDS: meta, poff (HM_POFF), the packed layout's end (HM_PBASE_END)
    // the model of a batched pass (devcoder_pstream_batch), allocated on its first use: the wider chain identity — every event's full
    // sub-block id, 2 bytes per decision and family (8 Dcap bytes) —, max_rank and stream offset of every sub-block
    DcArena batch_arena;
    u16 *esub[4] = {nullptr, nullptr, nullptr, nullptr};
    u8  *sub_maxr = nullptr; u32 *poff_tab = nullptr;
    // model segments (devcoder_pstream_segments): per sub-block the undecided avg_rank flags and the decisions of the coder at hand,
    // and the run table of the segment being modelled, rebased to its first run
    u32 *sub_und = nullptr, *sub_dec = nullptr, *seg_run = nullptr, *sub_mix = nullptr;   // (sub_mix: the adaptive coder's third fact, dc_mix_facts_kernel)
    // the packed stream of a pass or a segment (DcP13Tab): pad[s] and pbase[0 .. nsub] of the table at hand (dc_pbase_tab_kernel)
    u32 *pad_tab = nullptr, *pbase_tab = nullptr;
    hipEvent_t seg_ev[2] = {nullptr, nullptr};                 // behind the last copy out of ps[0 / 1] on the copy stream
    // the exact resolve of open avg_rank flags (BSCGPU_OPT_DC_AVG_EXACT), allocated on its first use: 71 bytes per chunk of DC_AVG_CH
    // runs, 130 per group of DC_AVG_GROUP chunks — under 0.1 byte per byte of max_n
    DcArena avg_arena;
    DcAvgRec avg = {};
    // the exact resolve of open chunk starts (BSCGPU_OPT_DC_REPLAY_EXACT), allocated on its first use: per chunk slot (4 nch_cap of them)
    // 2 DC_RP_CAND bytes of map, the head's end and a state byte — 771 bytes per slot, 1.5 bytes per byte of max_n (101 MB for 64 MiB)
    DcArena rp_arena;
    DcRpRec rp = {};
    // the exact resolve of open run_hist brackets (BSCGPU_OPT_DC_HIST_EXACT), allocated on its first use: a bit per run, 67 bytes per chunk
    // of DC_HIST_CH runs, 130 per group of DC_HIST_GROUP chunks — 0.2 byte per byte of max_n
    DcArena hist_arena;
    DcHistRec hist = {};
    // a block in sub-block segments (devcoder_block_begin), allocated on its first use: decisions and undecided flags of its eight sub-blocks
    DcArena blk_arena;
    u32 *blk_dec = nullptr, *blk_und = nullptr;
    // the adaptive coder's model of a pass (devcoder_adaptive_batch), allocated on its first use: two key buffers of the chain-major
    // sort (8 bytes per decision each) and the four debug planes (8) — 24 bytes per decision, 96 per byte of max_n — plus the tables
    // (stretch, squash, the mixers' parameters, the adaptive rates).  Everything else the stage needs lives in arrays of the main
    // arena that are dead behind the static model's stream kernel (pos[0..3], inv_sr).
    DcArena mix_arena;
    u64 *mix_key[2] = {nullptr, nullptr};
    u16 *mix_dbg = nullptr;                                    // [4][D]: state, char, static counter values, mixer id
    u32 *mix_meta = nullptr;                                   // MX_*
    short *mix_tab = nullptr;                                  // stretch[MX_TAB], squash[MX_TAB]
    MixParams *mix_mp = nullptr;                               // [NUM_CLS]
    ModelParams *mp_adapt = nullptr;                           // device copy (adaptive coder's counters)
};

__device__ __forceinline__ u32 dc_sb_of(u32 j, const DcSub& S)
{
    u32 sb = 0;
#pragma unroll
    for (int b = 1; b < 8; ++b) if ((u32)b < S.nb && j >= S.first[b]) sb = b;
    return sb;
}
// max_rank of an item's sub-block WITHOUT a memory access: indexing the by-value kernel argument with a per-lane index is a vector load
// from the argument segment (a select chain over S.maxr[b] is turned back into a load of a selected address), and inside the partition
// kernels' tile loops the wait for it (a vmcnt(0): the stores around it cannot be counted) also waited out the request for the next
// tile's items that had just gone out — round 6, from the ISA.  So: the eight values packed into one scalar word at the kernel's top.
__device__ __forceinline__ u32 dc_maxr_pack(const DcSub& S)
{
    u32 p = 0;
#pragma unroll
    for (u32 b = 0; b < 8; ++b) p |= (S.maxr[b] & 15u) << (4u * b);
    return (u32)__builtin_amdgcn_readfirstlane((int)p);
}
__device__ __forceinline__ int dc_maxr_of(u32 sb, u32 packed) { return (int)((packed >> (4u * sb)) & 15u); }
__device__ __forceinline__ u32 dc_run_len(const u32* __restrict__ start, u32 j, u32 m, u32 n) { return ((j + 1 < m) ? start[j + 1] : n) - start[j]; }

// ---- where the sub-block enters: the two shapes its boundaries come in (as qlfc_front.hip: QfRuns / QfRunTab) ------------------------------
// DcSub: one block's at most eight sub-blocks, by value.  DcSubTab: a batched pass's table in HBM (qlfc_front_batch leaves it: run[s] =
// first run of sub-block s, strictly increasing, run[nsub] = m; off[s] = its first byte in the pass, off[nsub] = the pass's bytes;
// base[s] = first byte of its block, which run starts are relative to) plus maxr[s] = max_rank of sub-block s (dc_tab_prep_kernel).
// The kernels below are templates over the shape; DcForm<SB> is everything that differs: the packed item (devcoder_model.h: Item /
// ItemB — the batch item carries 13 bits of sub-block and the sub-block's max_rank, so no kernel looks anything up by sub-block
// except a sub-block's first run), the shift that leaves (X, sub-block), and the index of the "kinds of run" bitmap (sub-block for the
// eight, max_rank for the table: 8 x 512 either way).
struct DcSubTab { u32 nsub; const u32* run; const u32* off; const u32* base; const u8* maxr; };
__device__ __forceinline__ u32 dc_sb_of(u32 j, const DcSubTab& S) { return batch_block_of(S.run, S.nsub, j); }
template <class SB> struct DcForm;
template <> struct DcForm<DcSub> {
    static constexpr bool TAB = false;
    static constexpr bool SUB_UND = false;                            // the avg_rank kernels count open flags for the block only
    static constexpr int CHAIN_SHIFT = ITEM_CHAIN_SHIFT;
    typedef Item It;
    static __device__ __forceinline__ It unpack(u64 k) { return item_unpack(k); }
    static __device__ __forceinline__ u32 maxr_word(const DcSub& S) { return dc_maxr_pack(S); }      // one scalar word at the kernel's top
    static __device__ __forceinline__ int maxr(const It& it, u32 w) { return dc_maxr_of(it.sb, w); }
    static __device__ __forceinline__ u32 first_run(const DcSub& S, u32 sb) { return S.first[sb]; }
    static __device__ __forceinline__ u32 next_first(const DcSub& S, u32 sb) { return (sb + 1 < S.nb) ? S.first[sb + 1] : 0xffffffffu; }
    static __device__ __forceinline__ u32 avg_top(const DcSub&, u32) { return 255u; }
    static __device__ __forceinline__ u32 kind(const It& it, int) { return it.sb; }
    static __device__ __forceinline__ int kind_maxr(u32 k, u32 w) { return dc_maxr_of(k, w); }
    static __device__ __forceinline__ u32 sig_sb(const It& it) { return it.sb; }
    static __device__ __forceinline__ u64 item(const DcSub& S, const u8* __restrict__ sym, const u8* __restrict__ rank, const u32* __restrict__ start,
                                               const u8* __restrict__ ge32, u32 j, u32 m, u32 n)
    { return item_pack(sym[j], dc_sb_of(j, S), ge32[j], rank[j], dc_run_len(start, j, m, n)); }
};
template <> struct DcForm<DcSubTab> {
    static constexpr bool TAB = true;
    static constexpr bool SUB_UND = true;                             // ... and per sub-block (sub_und)
    static constexpr int CHAIN_SHIFT = ITEMB_CHAIN_SHIFT;
    typedef ItemB It;
    static __device__ __forceinline__ It unpack(u64 k) { return item_unpack_b(k); }
    static __device__ __forceinline__ u32 maxr_word(const DcSubTab&) { return 0u; }
    static __device__ __forceinline__ int maxr(const It& it, u32) { return (int)it.maxr; }
    static __device__ __forceinline__ u32 first_run(const DcSubTab& S, u32 sb) { return S.run[sb]; }
    static __device__ __forceinline__ u32 next_first(const DcSubTab& S, u32 sb) { return (sb + 1 < S.nsub) ? S.run[sb + 1] : 0xffffffffu; }
    // avg' = (124 avg + 4 rank) >> 7 <= max(avg, rank) and rank < 2^(max_rank + 1): a tighter top for the bracket than 255, so that a
    // sub-block of at most 32 symbols in the middle of a pass can never leave a flag undecided (the eight-entry path does not even launch
    // the kernel for such a block)
    static __device__ __forceinline__ u32 avg_top(const DcSubTab& S, u32 sb) { return (2u << S.maxr[sb]) - 1u; }
    static __device__ __forceinline__ u32 kind(const It&, int maxr) { return (u32)maxr; }
    static __device__ __forceinline__ int kind_maxr(u32 k, u32) { return (int)k; }
    static __device__ __forceinline__ u32 sig_sb(const It& it) { return it.sb & 7u; }                // (the full id goes to the parallel array)
    static __device__ __forceinline__ u64 item(const DcSubTab& S, const u8* __restrict__ sym, const u8* __restrict__ rank, const u32* __restrict__ start,
                                               const u8* __restrict__ ge32, u32 j, u32, u32)
    {
        const u32 sb = dc_sb_of(j, S);
        const u32 end = (j + 1 < S.run[sb + 1]) ? start[j + 1] : S.off[sb + 1] - S.base[sb];      // the block's next run, or the sub-block's end
        return item_pack_b(sym[j], sb, ge32[j], rank[j], S.maxr[sb], end - start[j]);
    }
};
// The eight-entry form where the facts of a block in segments are taken (dc_block_facts): DcSub in everything, but the avg_rank kernels
// count the flags they leave open per sub-block as they do for a table.  A form of its own, so that the kernels of DcSub stay as they are.
struct DcSubU : DcSub {};
template <> struct DcForm<DcSubU> : DcForm<DcSub> { static constexpr bool SUB_UND = true; };

// ---------------------------------------------------------------------------------------------------------------------
// 1a. avg_rank >= 32 (qlfc.cpp:903 / :978): avg' = (avg * 124 + rank * 4) >> 7, reset per sub-block.  One lane per chunk,
// two-sided bracket [0, 255] started DC_AVG_WARM runs early; the flag of a run is decided when both ends agree.
// ---------------------------------------------------------------------------------------------------------------------
// REC (the exact resolve, 1a'): the lane also leaves what the kernels behind it start from (DcAvgRec) — its bracket at j0, its undecided
// count, whether a sub-block starts inside its chunk and whether the bracket is too wide to walk.  Off: the empty DcAvgNoRec, the
// kernel as it was.
struct DcAvgNoRec {};
enum : u32 { DC_AVG_ST_START = 1 /* a sub-block starts inside the chunk: whatever it started from, it ends the same */, DC_AVG_ST_WIDE = 2 /* DC_AVG_CAND values or more */ };
template <class SB, bool REC = false>
__global__ __launch_bounds__(WG) void dc_avg_kernel(const u8* __restrict__ rank, u32 m, SB S, u8* __restrict__ ge32, u32* __restrict__ meta,
                                                    u32* __restrict__ sub_und /* forms with SUB_UND only (may be null): undecided flags per sub-block */,
                                                    typename std::conditional<REC, DcAvgRec, DcAvgNoRec>::type R)
{
    typedef DcForm<SB> F;
    const u32 c = blockIdx.x * WG + threadIdx.x;
    const u64 j0 = (u64)c * DC_AVG_CH;
    if (j0 >= m) return;
    const u32 j1 = (u32)((j0 + DC_AVG_CH < m) ? j0 + DC_AVG_CH : m);
    u32 sb = dc_sb_of((u32)j0, S);
    const u32 sb_first = F::first_run(S, sb);
    u32 w0 = ((u32)j0 > sb_first + DC_AVG_WARM) ? (u32)j0 - DC_AVG_WARM : sb_first;
    u32 lo = 0, hi = (w0 == sb_first) ? 0u : F::avg_top(S, sb);
    for (u32 j = w0; j < (u32)j0; ++j) { const u32 r = rank[j]; lo = avg_rank_next(lo, r); hi = avg_rank_next(hi, r); }
    u32 next_first = F::next_first(S, sb);                            // (a chunk of a batched pass can hold dozens of sub-block starts)
    u32 und = 0, und_flushed = 0;                                     // (table: what of und has gone to sub_und)
    u32 st = 0;
    if constexpr (REC) { R.brk[c] = (u16)(lo | hi << 8); if (hi - lo >= (u32)DC_AVG_CAND) st = DC_AVG_ST_WIDE; }
    for (u32 j = (u32)j0; j < j1; ++j) {
        if (j == next_first) {
            if constexpr (F::SUB_UND) { if (sub_und && und != und_flushed) atomicAdd(&sub_und[sb], und - und_flushed); und_flushed = und; }
            lo = hi = 0; ++sb; next_first = F::next_first(S, sb);
            if constexpr (REC) st |= DC_AVG_ST_START;
        }
        const u32 f = lo >= 32u;
        und += (f != (u32)(hi >= 32u));
        ge32[j] = (u8)f;
        const u32 r = rank[j];
        lo = avg_rank_next(lo, r); hi = avg_rank_next(hi, r);
    }
    if constexpr (F::SUB_UND) { if (sub_und && und != und_flushed) atomicAdd(&sub_und[sb], und - und_flushed); }
    if (und) atomicAdd(&meta[DM_AVG_UND], und);
    if constexpr (REC) { R.und[c] = (u16)und; R.st[c] = (u8)st; }
}

// ---------------------------------------------------------------------------------------------------------------------
// 1a'. the open flags resolved exactly (BSCGPU_OPT_DC_AVG_EXACT; devcoder_model.h: avg_resolve_host restates these kernels).
// avg' is monotone in avg, so the exact value at a lane's first run lies in its bracket [lo0, hi0], and the bracket's width d obeys
// d' <= floor(124 d / 128) + 1: from 255 it is at most 32 after 128 runs, so behind DC_AVG_WARM runs a lane has at most 33 candidates.
// dc_avg_map_kernel walks a chunk once per candidate — its transfer map —, dc_avg_chain_kernel composes the maps of DC_AVG_GROUP
// chunks, dc_avg_groups_kernel chains the groups, dc_avg_chain_kernel<true> hands every chunk its exact start and dc_avg_fix_kernel
// walks the chunks with open flags again from theirs, one wavefront each.  All of them leave at once where nothing is open.
// ---------------------------------------------------------------------------------------------------------------------
// one wavefront per chunk whose successor starts open; lane v walks from lo0 + v.  The chunk has a successor, so it is whole:
// DC_AVG_CH runs, 16 rank bytes per lane, handed round the wavefront as scalars (every lane walks the same runs)
template <class SB>
__global__ __launch_bounds__(WG) void dc_avg_map_kernel(const u8* __restrict__ rank, u32 m, SB S, DcAvgRec R)
{
    typedef DcForm<SB> F;
    static_assert(DC_AVG_CAND == 64 && DC_AVG_CH == 64 * 16, "one candidate and 16 runs per lane");
    const u32 c = (u32)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * WAVES + (threadIdx.x >> 6)));
    const u32 lane = threadIdx.x & 63u;
    const u32 nch = (m + DC_AVG_CH - 1) / DC_AVG_CH;
    if (c + 1 >= nch) return;
    const u32 bn = R.brk[c + 1];
    if ((bn & 255u) == (bn >> 8)) return;                              // the successor starts exact: nobody reads this map
    const u32 b = R.brk[c], lo0 = b & 255u, w = (b >> 8) - lo0;
    if (w >= (u32)DC_AVG_CAND) return;                                 // the guard: not walked (DC_AVG_ST_WIDE says so to the chain)
    const u32 j0 = c * DC_AVG_CH;
    const u8* p = rank + j0 + 16u * lane;
    u32 q[4];
    if ((reinterpret_cast<uintptr_t>(rank) & 15u) == 0) {
        const uint4 t = *reinterpret_cast<const uint4*>(p);
        q[0] = t.x; q[1] = t.y; q[2] = t.z; q[3] = t.w;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) q[k] = (u32)p[4 * k] | (u32)p[4 * k + 1] << 8 | (u32)p[4 * k + 2] << 16 | (u32)p[4 * k + 3] << 24;
    }
    u32 x = lo0 + (lane <= w ? lane : 0u);
    u32 sb = 0, next_first = 0xffffffffu;
    if (R.st[c] & DC_AVG_ST_START) { sb = dc_sb_of(j0, S); next_first = F::next_first(S, sb); }
    for (u32 l = 0; l < 64u; ++l) {
        u32 r[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) r[k] = (u32)__builtin_amdgcn_readlane((int)q[k], (int)l);
        const u32 jb = j0 + 16u * l;
        if (next_first - jb < 16u) {                                   // a sub-block starts in these 16 runs (maybe several)
#pragma unroll
            for (u32 k = 0; k < 16u; ++k) {
                if (jb + k == next_first) { x = 0; ++sb; next_first = F::next_first(S, sb); }
                x = avg_rank_next(x, (r[k >> 2] >> (8u * (k & 3u))) & 255u);
            }
        } else {
#pragma unroll
            for (u32 k = 0; k < 16u; ++k) x = avg_rank_next(x, (r[k >> 2] >> (8u * (k & 3u))) & 255u);
        }
    }
    if (lane <= w) R.map[(size_t)c * DC_AVG_CAND + lane] = (u8)x;
}

// what the chain and groups kernels below read of a chunk, for the two resolves that share them: its start bracket (lo0 | hi0 << 8), its
// state, and whether there is anything to do at all
__device__ __forceinline__ u32 dc_rs_brk(const DcAvgRec& R, u32 c) { return R.brk[c]; }
__device__ __forceinline__ u32 dc_rs_st(const DcAvgRec& R, u32 c) { return R.st[c]; }
__device__ __forceinline__ bool dc_rs_idle(const DcAvgRec&) { return false; }
__device__ __forceinline__ u32 dc_rs_brk(const DcHistRec&, u32) { return (u32)(DC_HIST_CAND - 1) << 8; }      // [0, 63] everywhere: nothing restarts the chain but the maps
__device__ __forceinline__ u32 dc_rs_st(const DcHistRec&, u32) { return 0u; }
__device__ __forceinline__ bool dc_rs_idle(const DcHistRec& R) { return *R.ext == 0u; }
// the exact start of chunk c + 1 from the exact start x of chunk c; brk1 / brk0 / st0: of chunk c + 1 / c / c, map0: chunk c's map
__device__ __forceinline__ u32 dc_avg_step(u32 x, u32 brk1, u32 brk0, u32 st0, const u8* map0)
{
    if ((brk1 & 255u) == (brk1 >> 8)) return brk1 & 255u;             // a closed bracket restarts the chain
    if (st0 & DC_AVG_ST_WIDE) return DC_AVG_UNKNOWN;
    if (st0 & DC_AVG_ST_START) return map0[0];                         // ... and so does a sub-block start inside the chunk
    return x == DC_AVG_UNKNOWN ? DC_AVG_UNKNOWN : (u32)map0[x - (brk0 & 255u)];
}
// One wavefront per group of DC_AVG_GROUP chunks, their maps in LDS.  HAND = false: lane v follows candidate v of the group's first
// chunk through the group -> gmap[g][v], the start of the next group's first chunk (only where that one starts open).  HAND = true:
// every lane follows the group's exact start (gstart[g]) and lane k keeps what chunk k starts from -> ex.
// REC: whose maps they are.  DcAvgRec: the avg_rank resolve's; DcHistRec: the run_hist resolve's (1c') — the same map format, 64 byte
// entries from base 0, every chunk open over the whole range, no state, and nothing to do where no run is open (dc_rs_*)
template <bool HAND, class REC = DcAvgRec>
__global__ __launch_bounds__(64) void dc_avg_chain_kernel(u32 m, REC R)
{
    static_assert(DC_AVG_GROUP == 64 && DC_AVG_CAND == 64, "one chunk and one candidate per lane");
    __shared__ u32 brk_s[DC_AVG_GROUP + 1], st_s[DC_AVG_GROUP];
    __shared__ uint4 map_s[DC_AVG_GROUP * DC_AVG_CAND / 16];
    if (dc_rs_idle(R)) return;
    const u32 g = blockIdx.x, lane = threadIdx.x, c0 = g * DC_AVG_GROUP;
    const u32 nch = (m + DC_AVG_CH - 1) / DC_AVG_CH;
    const u32 cnt = nch - c0 < (u32)DC_AVG_GROUP ? nch - c0 : (u32)DC_AVG_GROUP;      // chunks of this group
    const u32 mine = lane < cnt ? dc_rs_brk(R, c0 + lane) : 0u;
    if constexpr (HAND) {
        if (__ballot(lane < cnt && (mine & 255u) != (mine >> 8)) == 0ull) {         // every chunk starts exact
            if (lane < cnt) R.ex[c0 + lane] = (u16)(mine & 255u);
            return;
        }
    } else {
        if (c0 + DC_AVG_GROUP >= nch) return;
        const u32 bn = dc_rs_brk(R, c0 + DC_AVG_GROUP);
        if ((bn & 255u) == (bn >> 8)) return;
    }
    brk_s[lane] = mine; st_s[lane] = lane < cnt ? dc_rs_st(R, c0 + lane) : 0u;
    if (lane == 0) brk_s[DC_AVG_GROUP] = c0 + DC_AVG_GROUP < nch ? dc_rs_brk(R, c0 + DC_AVG_GROUP) : 0u;
    const uint4* src = reinterpret_cast<const uint4*>(R.map + (size_t)c0 * DC_AVG_CAND);
#pragma unroll
    for (int k = 0; k < 4; ++k) map_s[k * 64 + lane] = src[k * 64 + lane];            // (the arrays are padded to whole groups)
    __syncthreads();
    const u8* maps = reinterpret_cast<const u8*>(map_s);
    u32 x, keep = 0;
    if constexpr (HAND) x = R.gstart[g];
    else x = (!(st_s[0] & DC_AVG_ST_WIDE) && lane <= (brk_s[0] >> 8) - (brk_s[0] & 255u)) ? (brk_s[0] & 255u) + lane : DC_AVG_UNKNOWN;
    for (u32 k = 0; k < cnt; ++k) {
        if (HAND && lane == k) keep = x;
        if (c0 + k + 1 >= nch) break;
        x = dc_avg_step(x, brk_s[k + 1], brk_s[k], st_s[k], maps + k * DC_AVG_CAND);
    }
    if constexpr (HAND) { if (lane < cnt) R.ex[c0 + lane] = (u16)keep; }
    else R.gmap[(size_t)g * DC_AVG_CAND + lane] = (u16)x;
}
// the groups chained: one wavefront, 64 groups' maps at a time in LDS, the walk itself on one value
template <class REC = DcAvgRec>
__global__ __launch_bounds__(64) void dc_avg_groups_kernel(u32 m, REC R)
{
    __shared__ u32 first_s[65], wide_s[64];
    __shared__ uint4 gmap_s[64 * DC_AVG_CAND * 2 / 16];
    if (dc_rs_idle(R)) return;
    const u32 lane = threadIdx.x;
    const u32 nch = (m + DC_AVG_CH - 1) / DC_AVG_CH, ngr = (nch + DC_AVG_GROUP - 1) / DC_AVG_GROUP;
    u32 x = dc_rs_brk(R, 0) & 255u;                                    // (chunk 0 starts a sub-block)
    for (u32 g0 = 0; g0 < ngr; g0 += 64u) {
        const u32 cnt = ngr - g0 < 64u ? ngr - g0 : 64u;
        // lane i: group g0 + i, and the first chunk of the group behind it
        const u32 nf = g0 + lane + 1 < ngr ? dc_rs_brk(R, (g0 + lane + 1) * DC_AVG_GROUP) : 0u;
        const bool any_open = __ballot((nf & 255u) != (nf >> 8)) != 0ull;
        __syncthreads();
        first_s[lane + 1] = nf;
        if (any_open) {
            if (lane == 0) first_s[0] = dc_rs_brk(R, g0 * DC_AVG_GROUP);
            wide_s[lane] = lane < cnt ? dc_rs_st(R, (g0 + lane) * DC_AVG_GROUP) & DC_AVG_ST_WIDE : 0u;
            const uint4* src = reinterpret_cast<const uint4*>(R.gmap + (size_t)g0 * DC_AVG_CAND);
#pragma unroll
            for (int k = 0; k < 8; ++k) gmap_s[k * 64 + lane] = src[k * 64 + lane];    // (padded to 64 groups)
        }
        __syncthreads();
        if (!any_open) {                                               // every group of the tile starts exact
            if (lane == 0) R.gstart[g0] = (u16)x;
            if (lane + 1 < cnt) R.gstart[g0 + lane + 1] = (u16)(nf & 255u);
            x = first_s[cnt] & 255u;                                   // (the tile behind starts from its own first chunk's bracket, if there is one)
            continue;
        }
        const u16* gm = reinterpret_cast<const u16*>(gmap_s);
        u32 keep = 0;
        for (u32 k = 0; k < cnt; ++k) {
            if (lane == k) keep = x;
            if (g0 + k + 1 >= ngr) break;
            const u32 b1 = first_s[k + 1], b0 = first_s[k];
            if ((b1 & 255u) == (b1 >> 8)) x = b1 & 255u;
            else x = (x == DC_AVG_UNKNOWN || wide_s[k]) ? DC_AVG_UNKNOWN : (u32)gm[k * DC_AVG_CAND + (x - (b0 & 255u))];
        }
        if (lane < cnt) R.gstart[g0 + lane] = (u16)keep;
    }
}
// one wavefront per chunk with open flags: again from its exact start, the ranks handed round as in dc_avg_map_kernel (a lane that
// walked alone would wait for every byte: 0.40 ms where every chunk of an 8 MiB block is open, against 0.18), every lane on the same values and lane l
// keeping the flags of runs 16 l ..  An unknown start (the guard) leaves the flags as they are and counts them: DM_AVG_LEFT, and per
// sub-block where the table form asks
template <class SB>
__global__ __launch_bounds__(WG) void dc_avg_fix_kernel(const u8* __restrict__ rank, u32 m, SB S, u8* __restrict__ ge32, u32* __restrict__ meta,
                                                        u32* __restrict__ sub_und, DcAvgRec R)
{
    typedef DcForm<SB> F;
    const u32 c = (u32)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * WAVES + (threadIdx.x >> 6)));
    const u32 lane = threadIdx.x & 63u;
    const u32 nch = (m + DC_AVG_CH - 1) / DC_AVG_CH;
    if (c >= nch) return;
    const u32 und = R.und[c];
    if (und == 0) return;
    const u32 j0 = c * DC_AVG_CH, j1 = (m - j0 > (u32)DC_AVG_CH) ? j0 + DC_AVG_CH : m;
    const u32 b = R.brk[c], e = R.ex[c];
    const bool known = e != DC_AVG_UNKNOWN;
    u32 lo = b & 255u, hi = b >> 8, x = known ? e : lo;
    const u32 at = j0 + 16u * lane;                                    // this lane's 16 runs (the last chunk may end inside or in front of them)
    u32 q[4];
    if (at + 16u <= j1 && (reinterpret_cast<uintptr_t>(rank) & 15u) == 0) {
        const uint4 t = *reinterpret_cast<const uint4*>(rank + at);
        q[0] = t.x; q[1] = t.y; q[2] = t.z; q[3] = t.w;
    } else {
#pragma unroll
        for (u32 k = 0; k < 4u; ++k) {
            q[k] = 0;
#pragma unroll
            for (u32 i = 0; i < 4u; ++i) if (at + 4u * k + i < j1) q[k] |= (u32)rank[at + 4u * k + i] << (8u * i);
        }
    }
    u32 sb = dc_sb_of(j0, S);
    u32 next_first = F::next_first(S, sb);
    u32 left = 0, mine = 0;
    const u32 pieces = (j1 - j0 + 15u) / 16u;
    for (u32 l = 0; l < pieces; ++l) {
        u32 r[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) r[k] = (u32)__builtin_amdgcn_readlane((int)q[k], (int)l);
        const u32 jb = j0 + 16u * l;
        u32 bits = 0;
#pragma unroll
        for (u32 k = 0; k < 16u; ++k) {
            if (jb + k < j1) {
                if (jb + k == next_first) {
                    if constexpr (F::SUB_UND) { if (sub_und && left && lane == 0) atomicAdd(&sub_und[sb], left); }
                    left = 0; lo = hi = x = 0; ++sb; next_first = F::next_first(S, sb);
                }
                left += (u32)(!known && (lo >= 32u) != (hi >= 32u));
                bits |= (u32)(x >= 32u) << k;
                const u32 rk = (r[k >> 2] >> (8u * (k & 3u))) & 255u;
                lo = avg_rank_next(lo, rk); hi = avg_rank_next(hi, rk); x = avg_rank_next(x, rk);
            }
        }
        if (lane == l) mine = bits;
    }
    if (lane == 0) {
        if constexpr (F::SUB_UND) { if (sub_und && left) atomicAdd(&sub_und[sb], left); }
        atomicAdd(&meta[known ? DM_AVG_RESOLVED : DM_AVG_LEFT], und);
    }
    if (!known) return;
    if (at + 16u <= j1 && (reinterpret_cast<uintptr_t>(ge32) & 15u) == 0) {
        uint4 t;
        t.x = (mine & 1u) | (mine & 2u) << 7 | (mine & 4u) << 14 | (mine & 8u) << 21;
        t.y = (mine >> 4 & 1u) | (mine >> 4 & 2u) << 7 | (mine >> 4 & 4u) << 14 | (mine >> 4 & 8u) << 21;
        t.z = (mine >> 8 & 1u) | (mine >> 8 & 2u) << 7 | (mine >> 8 & 4u) << 14 | (mine >> 8 & 8u) << 21;
        t.w = (mine >> 12 & 1u) | (mine >> 12 & 2u) << 7 | (mine >> 12 & 4u) << 14 | (mine >> 12 & 8u) << 21;
        *reinterpret_cast<uint4*>(ge32 + at) = t;
    } else {
        for (u32 k = 0; k < 16u; ++k) if (at + k < j1) ge32[at + k] = (u8)(mine >> k & 1u);
    }
}

// 1b. packed items in stream order: X = symbol (the char family's sort digit; the static family ignores it)
template <class SB>
__global__ __launch_bounds__(WG) void dc_items_kernel(const u8* __restrict__ sym, const u8* __restrict__ rank, const u32* __restrict__ start,
                                                      const u8* __restrict__ ge32, u32 m, u32 n, SB S, u64* __restrict__ key_ch)
{
    const u32 j = blockIdx.x * WG + threadIdx.x;
    if (j < m) key_ch[j] = DcForm<SB>::item(S, sym, rank, start, ge32, j, m, n);
}

// kinds of run for the "which decision types occur" bitmap: 8 sub-blocks (a batched pass: 8 values of max_rank — all the sub-block
// contributes to a run's decision types) x escape flag x 256 ranks, then 96 run-length classes
constexpr u32 DC_KIND_RUN = 8 * 512, DC_KIND_WORDS = (DC_KIND_RUN + 96 + 31) / 32;

// 1c. context states + the state family's items + which kinds of run occur.  Thread per run (stream order).
// REC (the exact resolve of open run_hist brackets, 1c'): a run whose bracket the nine predecessors leave open does not look further
// back — it keeps the lower end for now and leaves what dc_hist_fix_kernel rewrites its run-state from (DcHistRec).  Off: the empty
// DcHistNoRec, the kernel as it was.
struct DcHistNoRec {};
template <class SB, bool REC = false>
__global__ __launch_bounds__(WG) void dc_ctx_kernel(const u64* __restrict__ key_ch, const u64* __restrict__ key_ch_s, const u32* __restrict__ inv_ch,
                                                    u32 m, SB S, const u8* __restrict__ tab_rank, const u8* __restrict__ tab_run,
                                                    u64* __restrict__ key_sr, u64* __restrict__ key_sn, u32* __restrict__ present, u32* __restrict__ meta,
                                                    typename std::conditional<REC, DcHistRec, DcHistNoRec>::type R)
{
    __shared__ u32 bits[DC_KIND_WORDS];
    for (u32 i = threadIdx.x; i < DC_KIND_WORDS; i += WG) bits[i] = 0;
    __syncthreads();
    const u32 j = dc_virtual_block() * WG + threadIdx.x;
    if (j < m) {
        const u64 key = key_ch[j];
        typedef DcForm<SB> F;
        constexpr int CS = F::CHAIN_SHIFT;
        const typename F::It it = F::unpack(key);
        const u32 j0 = F::first_run(S, it.sb);                        // (a 64-run tile of a batched pass can hold dozens of sub-block starts)
        // window contexts: previous runs of the same sub-block (qlfc.cpp:1063-1068)
        u32 ctx_rank0 = 0, ctx_rank4 = 0, ctx_run = 0;
#pragma unroll
        for (u32 k = 1; k <= 4; ++k) {
            if (j >= j0 + k) {
                const typename F::It p = F::unpack(key_ch[j - k]);
                if (k <= 3) ctx_rank0 |= (p.rank == 1u ? 1u : 0u) << (k - 1);
                ctx_rank4 |= (p.rank - 1u < 3u ? p.rank - 1u : 3u) << (2 * (k - 1));
                ctx_run |= (p.run < 3u ? 1u : 0u) << (k - 1);
            }
        }
        // symbol-major neighbours: the previous runs of this symbol in this sub-block, nearest first (loaded once)
        const u32 q = inv_ch[j];
        const u64 chain_id = key >> CS;                               // X and sub-block
        // (all NP loads are issued at once — the index does not depend on what the nearer neighbours turn out to be — and NP is large
        // enough that the bracket below almost always closes: on the bench block 1.9 % of the runs — a lane in 38 % of the wavefronts —
        // stay open after five predecessors (a symbol whose recent runs all have length 2 or 3 has two fixed points, 1 and 2), 0.015 %
        // after nine)
        constexpr int NP = DC_HIST_NP;
        u64 pk[NP];
        if (q >= 10u) {
            // the nine predecessors are 72 consecutive bytes: five 16-byte loads instead of nine 8-byte ones (round 6: the kernel is bound by
            // the lines its gathers touch per instruction, and these nine touched the same one or two lines nine times)
            struct __attribute__((packed, aligned(8))) U2 { u64 a, b; };
            const U2* w = reinterpret_cast<const U2*>(key_ch_s + (q - 10u));
            const U2 w0 = w[0], w1 = w[1], w2 = w[2], w3 = w[3], w4 = w[4];            // elements q-10 .. q-1
            pk[8] = w0.b; pk[7] = w1.a; pk[6] = w1.b; pk[5] = w2.a; pk[4] = w2.b; pk[3] = w3.a; pk[2] = w3.b; pk[1] = w4.a; pk[0] = w4.b;
        } else {
#pragma unroll
            for (int t = 1; t <= NP; ++t) pk[t - 1] = key_ch_s[q >= (u32)t ? q - (u32)t : 0u];
        }
        u32 prun[NP], prank0 = 0; int np = 0; bool at_start = false;
#pragma unroll
        for (int t = 1; t <= NP; ++t) {
            bool have = false;
            if (!at_start && q >= (u32)t && (pk[t - 1] >> CS) == chain_id) {
                const typename F::It pi = F::unpack(pk[t - 1]); prun[t - 1] = pi.run; if (t == 1) prank0 = pi.rank; have = true; np = t;
            }
            if (!have) { at_start = true; prun[t - 1] = 1; }
        }
        const u32 rank_hist = np > 0 ? (u32)bsr(prank0) : 0u;
        // run_hist (qlfc.cpp:981-987): h' = (h + x) >> 2 over the symbol's earlier runs; only min(h, 7) is used.  Walk a two-sided
        // bracket forward over the loaded predecessors; the start is exact (0) when the chain begins inside the window.
        u32 run_hist = 0;
        {
            u32 lo = 0, hi = at_start ? 0u : 63u;
#pragma unroll
            for (int t = NP; t >= 1; --t) if (t <= np) { lo = run_hist_next(lo, prun[t - 1]); hi = run_hist_next(hi, prun[t - 1]); }
            u32 cl = lo < 7u ? lo : 7u, ch = hi < 7u ? hi : 7u;
            if constexpr (REC) {
                if (cl != ch) {                                       // open: the lower end for now, the rest is dc_hist_fix_kernel's
                    atomicAdd(&meta[DM_HIST_EXT], 1u);
                    R.scr[q] = (u64)j << 13 | run_state_index(ctx_rank0, ctx_run, it.rank, 0u);
                    atomicOr(&R.bits[q >> 5], 1u << (q & 31u));
                    R.flag[q / (u32)DC_HIST_CH] = 1;
                }
            } else if (cl != ch) {
                // rare: look further back (quadrupling) until the clamped values agree or the chain starts
                atomicAdd(&meta[DM_HIST_EXT], 1u);
                u32 K = 4 * NP;
                for (;;) {
                    lo = 0; hi = 63; u32 first = q; bool exact = false;
                    for (u32 t = 1; t <= K; ++t) {
                        if (q < t || (key_ch_s[q - t] >> CS) != chain_id) { exact = true; break; }
                        first = q - t;
                    }
                    if (exact) hi = 0;
                    for (u32 p = first; p < q; ++p) { const u32 r = F::unpack(key_ch_s[p]).run; lo = run_hist_next(lo, r); hi = run_hist_next(hi, r); }
                    cl = lo < 7u ? lo : 7u; ch = hi < 7u ? hi : 7u;
                    if (cl == ch) break;
                    if (K >= (u32)DC_HIST_KMAX) { atomicOr(&meta[DM_FAIL], (u32)FAIL_HIST); break; }
                    K *= 4;
                }
            }
            run_hist = cl;
        }
        const u32 state_rank = tab_rank[rank_state_index(ctx_run, ctx_rank4, rank_hist)];
        const u32 state_run = tab_run[run_state_index(ctx_rank0, ctx_run, it.rank, run_hist)];
        const u64 info = key & 0x00ffffffffffffffull;
        key_sr[j] = ((u64)state_rank << 56) | info;
        key_sn[j] = ((u64)state_run << 56) | info;

        // which kinds of run occur: the decision types of a run are a function of (sub-block, escape flag, rank) on the rank side
        // and of the run-length class on the run side (dc_setup_kernel expands the kinds that occur into types)
        auto mark = [&](u32 k) { const u32 w = k >> 5, b = 1u << (k & 31); if (!(bits[w] & b)) atomicOr(&bits[w], b); };
        mark((F::kind(it, F::maxr(it, 0u)) << 9) | (it.ge32 << 8) | it.rank);
        mark(DC_KIND_RUN + (it.run < 64u ? it.run : 64u + (u32)bsr(it.run)));
    }
    __syncthreads();
    // Bits are only ever set during the launch, so a plain look first is safe (a stale zero costs one atomic, a one is a one): without it
    // every workgroup — 110 K of them — sent ~20 atomics to the same few dozen words, and those serialise at ~11 ns apiece.
    for (u32 i = threadIdx.x; i < DC_KIND_WORDS; i += WG) {
        const u32 mine = bits[i];
        if (mine) { const u32 need = mine & ~__builtin_nontemporal_load(&present[i]); if (need) atomicOr(&present[i], need); }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// 1c'. the open run_hist brackets resolved exactly (BSCGPU_OPT_DC_HIST_EXACT; devcoder_model.h: hist_resolve_host restates these
// kernels).  h' = (h + inc) >> 2 is monotone in h and contracts by four — for a <= b the images are at most floor((b - a + 3) / 4)
// apart, so a bracket's width goes 63 -> 16 -> 4 -> 1 and stays at 1 wherever the class of the runs has two fixed points (runs of 2 to
// 127 bytes) — and [0, 63] is invariant: (63 + 93) >> 2 = 39.  So one wavefront walks a chunk of the symbol-major array from ALL 64
// values, one per lane: dc_hist_map_kernel.  The maps have the avg_rank resolve's format and are composed, chained and handed out by
// its kernels (dc_avg_chain_kernel<false>, dc_avg_groups_kernel, dc_avg_chain_kernel<true>, over DcHistRec); dc_hist_fix_kernel walks
// the chunks that hold an open run again from their exact start.  No guard: 64 candidates are the whole range, FAIL_HIST is never raised.
// All of them leave at once where no run is open.
// ---------------------------------------------------------------------------------------------------------------------
// a lane's 16 elements from `at` on, a byte each: the increment (at most 3 * 30 + 3) | 128 where the element starts a chain
template <class F>
__device__ __forceinline__ void dc_hist_load(const u64* __restrict__ key_ch_s, u32 at, u32 m, u32 q[4])
{
    u64 prev = (at > 0u && at <= m) ? key_ch_s[at - 1u] : 0ull;
#pragma unroll
    for (u32 k = 0; k < 4u; ++k) {
        q[k] = 0;
#pragma unroll
        for (u32 i = 0; i < 4u; ++i) {
            const u32 p = at + 4u * k + i;
            if (p < m) {
                const u64 key = key_ch_s[p];
                const u32 b = run_hist_inc(F::unpack(key).run) | ((p == 0u || (key >> F::CHAIN_SHIFT) != (prev >> F::CHAIN_SHIFT)) ? 128u : 0u);
                q[k] |= b << (8u * i);
                prev = key;
            }
        }
    }
}
__device__ __forceinline__ u32 dc_hist_step(u32 x, u32 b) { return (((b & 128u) ? 0u : x) + (b & 127u)) >> 2; }
// one wavefront per whole chunk (the last chunk has no successor); lane v walks from v.  The bytes are handed round the wavefront as
// scalars: every lane walks the same elements
template <class SB>
__global__ __launch_bounds__(WG) void dc_hist_map_kernel(const u64* __restrict__ key_ch_s, u32 m, DcHistRec R)
{
    static_assert(DC_HIST_CAND == 64 && DC_HIST_CH == 64 * 16, "one candidate and 16 elements per lane");
    if (*R.ext == 0u) return;
    const u32 c = (u32)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * WAVES + (threadIdx.x >> 6)));
    const u32 lane = threadIdx.x & 63u;
    const u32 nch = (m + DC_HIST_CH - 1) / DC_HIST_CH;
    if (c + 1 >= nch) return;
    u32 q[4];
    dc_hist_load<DcForm<SB>>(key_ch_s, c * DC_HIST_CH + 16u * lane, m, q);
    u32 x = lane;
    for (u32 l = 0; l < 64u; ++l) {
        u32 r[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) r[k] = (u32)__builtin_amdgcn_readlane((int)q[k], (int)l);
#pragma unroll
        for (u32 k = 0; k < 16u; ++k) x = dc_hist_step(x, (r[k >> 2] >> (8u * (k & 3u))) & 255u);
    }
    R.map[(size_t)c * DC_HIST_CAND + lane] = (u8)x;
}
// one wavefront per chunk that holds an open run: again from its exact start, every lane on the same values, lane l keeping min(h, 7)
// of elements 16 l ..; then every lane rewrites the run-state of its open elements (the state byte of key_sn[j]; key_sr does not
// depend on run_hist)
template <class SB>
__global__ __launch_bounds__(WG) void dc_hist_fix_kernel(const u64* __restrict__ key_ch_s, u32 m, const u8* __restrict__ tab_run, u64* __restrict__ key_sn,
                                                         u32* __restrict__ meta, DcHistRec R)
{
    if (*R.ext == 0u) return;
    const u32 c = (u32)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * WAVES + (threadIdx.x >> 6)));
    const u32 lane = threadIdx.x & 63u;
    const u32 nch = (m + DC_HIST_CH - 1) / DC_HIST_CH;
    if (c >= nch || R.flag[c] == 0) return;
    const u32 at = c * DC_HIST_CH + 16u * lane;                        // (the last chunk may end inside or in front of these: bytes of 0)
    u32 q[4];
    dc_hist_load<DcForm<SB>>(key_ch_s, at, m, q);
    u32 x = R.ex[c];
    u32 mine[2] = {0u, 0u};                                           // four bits per element
    for (u32 l = 0; l < 64u; ++l) {
        u32 r[4], v[2] = {0u, 0u};
#pragma unroll
        for (int k = 0; k < 4; ++k) r[k] = (u32)__builtin_amdgcn_readlane((int)q[k], (int)l);
#pragma unroll
        for (u32 k = 0; k < 16u; ++k) {
            const u32 b = (r[k >> 2] >> (8u * (k & 3u))) & 255u;
            if (b & 128u) x = 0;
            v[k >> 3] |= (x < 7u ? x : 7u) << (4u * (k & 7u));
            x = (x + (b & 127u)) >> 2;
        }
        if (lane == l) { mine[0] = v[0]; mine[1] = v[1]; }
    }
    const u32 open = (R.bits[at >> 5] >> (at & 31u)) & 0xffffu;        // (16 elements: half a word; no bit is set at or behind m)
    u32 n = 0;
#pragma unroll
    for (u32 k = 0; k < 16u; ++k) {
        bool done = false;
        if (open >> k & 1u) {
            const u64 s = R.scr[at + k];
            const u32 j = (u32)(s >> 13);
            if (j < m) {
                reinterpret_cast<u8*>(key_sn + j)[7] = tab_run[((u32)s & 8191u) | ((mine[k >> 3] >> (4u * (k & 7u))) & 7u)];
                done = true;
            }
        }
        n += (u32)__popcll(__ballot(done));
    }
    if (lane == 0 && n) atomicAdd(&meta[DM_HIST_RESOLVED], n);
}

// 1d. the canonical rounds that occur (and how many decision types: diagnostics).  One workgroup.
template <class SB>
__global__ __launch_bounds__(WG) void dc_setup_kernel(const u32* __restrict__ kinds, SB S, u8* __restrict__ rounds, u32* __restrict__ meta,
                                                      u32 avg_word /* DM_AVG_UND, or DM_AVG_LEFT behind the exact resolve */)
{
    typedef DcForm<SB> F;
    const u32 mrp = F::maxr_word(S);                                  // max_rank of the eight sub-blocks, one scalar word
    __shared__ u32 present[(NUM_TAU + 31) / 32];
    __shared__ u32 rbits[3];
    __shared__ u32 ntypes;
    for (u32 i = threadIdx.x; i < (NUM_TAU + 31) / 32; i += WG) present[i] = 0;
    if (threadIdx.x < 3) rbits[threadIdx.x] = 0;
    if (threadIdx.x == 0) ntypes = 0;
    __syncthreads();
    auto mark = [&](int tau) { atomicOr(&present[(u32)tau >> 5], 1u << (tau & 31)); };
    for (u32 k = threadIdx.x; k < DC_KIND_RUN + 96; k += WG) {
        if (!(kinds[k >> 5] & (1u << (k & 31)))) continue;
        Item it; it.sb = 0; it.ge32 = 0; it.rank = 1; it.run = 1;
        if (k < DC_KIND_RUN) {                                                    // the rank side of a run of this kind
            it.sb = k >> 9; it.ge32 = (k >> 8) & 1u; it.rank = k & 255u;
            const int maxr = F::kind_maxr(it.sb, mrp);                // (a batched pass: the kind IS the max_rank)
            if (it.ge32) { for (int d = 0; d <= maxr; ++d) { u32 bit; mark(decision(it, maxr, ROUND_RP + d, &bit)); } }
            else {
                mark(TAU_RF);
                if (it.rank != 1u) {
                    const int B = bsr(it.rank);
                    for (int s = 0; s <= B - 2; ++s) mark(TAU_RE + s);
                    if (B < maxr) mark(TAU_RE + B - 1);
                    for (int d = 0; d < B; ++d) { u32 bit; mark(decision(it, maxr, ROUND_RM + d, &bit)); }
                }
            }
        } else {                                                                  // the run side: a representative length of the class
            const u32 cls = k - DC_KIND_RUN;
            it.run = cls < 64u ? cls : 1u << (cls - 64u);
            mark(TAU_NF);
            if (it.run != 1u) {
                const int nb = bsr(it.run);
                for (int s = 0; s < nb; ++s) mark(TAU_NE + s);
                for (int d = 0; d < nb; ++d) { u32 bit; mark(decision(it, 0, ROUND_NM + d, &bit)); }
            }
        }
    }
    __syncthreads();
    for (int tau = threadIdx.x; tau < NUM_TAU; tau += WG) {
        if (present[(u32)tau >> 5] & (1u << (tau & 31))) {
            const int r = tau_round(tau);
            atomicOr(&rbits[r >> 5], 1u << (r & 31));
            atomicAdd(&ntypes, 1u);
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        u32 nr = 0;
        for (int r = 0; r < NUM_ROUNDS; ++r) if (rbits[r >> 5] & (1u << (r & 31))) rounds[nr++] = (u8)r;
        meta[DM_NTYPES] = ntypes; meta[DM_NROUNDS] = nr;
        if (meta[avg_word] != 0u) atomicOr(&meta[DM_FAIL], (u32)FAIL_AVG);
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// 2. partition: decisions of a job's items into chain-major order
// ---------------------------------------------------------------------------------------------------------------------
struct DcGeom { u32 m; u32 W; u32 per_wave; };                       // items, wave-chunks, items per wave-chunk (multiple of 64)
static DcGeom dc_geom(u32 m)
{
    DcGeom g; g.m = m;
    u32 W = (m + 63) / 64; if (W > DC_WCH_MAX) W = DC_WCH_MAX; if (W == 0) W = 1;
    u32 per = (m + W - 1) / W; per = (per + 63) / 64 * 64; if (per == 0) per = 64;
    g.per_wave = per; g.W = (m + per - 1) / per; if (g.W == 0) g.W = 1;
    return g;
}

typedef __attribute__((address_space(3))) volatile u32 dc_lds_vu32;

// Lanes among `on` whose NB-bit key equals this lane's: (lo, hi) halves of the peer mask.
template <int NB>
__device__ __forceinline__ void dc_peers(u32 key, bool on, u32& mlo, u32& mhi)
{
    const u64 act = __ballot(on);
    mlo = (u32)act; mhi = (u32)(act >> 32);
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        const int bitm = __builtin_amdgcn_sbfe((int)key, b, 1);              // 0 or -1
        const u64 bal = __ballot(bitm != 0);
        const u32 nbm = ~(u32)bitm;
        mlo &= (u32)bal ^ nbm;
        mhi &= (u32)(bal >> 32) ^ nbm;
    }
}
// One level down a code tree: of the peers keep those that coded the same bit (`keep` = all ones: no refinement for this lane).
__device__ __forceinline__ void dc_refine(u32 bit, u32 keep, u32& mlo, u32& mhi)
{
    const u64 bal = __ballot(bit != 0);
    const u32 nbm = bit ? 0u : ~0u;
    mlo &= ((u32)bal ^ nbm) | keep;
    mhi &= ((u32)(bal >> 32) ^ nbm) | keep;
}

// The decisions of 64 items, round by round in canonical order, with the case analysis done once per item instead of once per
// round: single-row rounds (RF, RE s, NF, NE s: one decision type, hence one row, per round) go to es(slot, on, bit) with
// slot = 0 | 1 + s | 8 | 9 + s; mantissa / escape rounds (several rows per round) go to em(tau, on, bit, peers) where peers is
// the mask of the lanes whose decision of this round has the same type.  The rows of such a round are the nodes of one level
// of a code tree: two lanes are peers at depth d + 1 iff they were peers at depth d and coded the same bit there, so the mask
// costs one ballot per round after a single match on the tree's id (rank length B / run-length bits).  Control flow is
// wave-uniform; every lane calls with its own `on`.
constexpr int DC_SLOTS = 40;
__device__ __forceinline__ int dc_slot_tau(int slot) { return slot == 0 ? TAU_RF : slot < 8 ? TAU_RE + slot - 1 : slot == 8 ? TAU_NF : TAU_NE + slot - 9; }

template <int SIDES, class ES, class EM>
__device__ __forceinline__ void dc_item_rounds(const Item& it, bool valid, int maxr, ES&& es, EM&& em)
{
    if (SIDES & 1) {
        const u32 rank = it.rank;
        const bool ge = valid && it.ge32 != 0u, ng = valid && it.ge32 == 0u;
        const int B = (ng && rank != 1u) ? bsr(rank) : 0;
        const int e = B ? (B - 1) + (B < maxr ? 1 : 0) : 0;
        if (__ballot(ng)) es(0, ng, rank != 1u ? 1u : 0u);
        for (int sx = 0; sx < 7; ++sx) { const bool on = sx < e; if (!__ballot(on)) break; es(1 + sx, on, sx + 1 < B ? 1u : 0u); }
        if (__ballot(B != 0)) {
            u32 mlo, mhi;
            dc_peers<3>((u32)B, B != 0, mlo, mhi);
            for (int d = 0; d < 7; ++d) {
                const bool on = d < B;
                const u64 act = __ballot(on);
                if (!act) break;
                const u32 ctx = on ? (rank >> (B - d)) : 1u;
                const u32 bit = on ? (rank >> (B - 1 - d)) & 1u : 0u;
                em(on ? TAU_RM + rm_off(B) + (int)ctx - 1 : 0, on, bit, mlo & (u32)act, mhi & (u32)(act >> 32));
                dc_refine(bit, 0u, mlo, mhi);
            }
        }
        if (__ballot(ge)) {
            u32 mlo = ~0u, mhi = ~0u;                                           // depth 0: one row (ctx = 1)
            for (int d = 0; d < 8; ++d) {
                const bool on = ge && d <= maxr;
                const u64 act = __ballot(on);
                if (!act) break;
                const u32 ctx = on ? ((1u << d) | ((rank >> (maxr + 1 - d)) & ((1u << d) - 1u))) : 1u;
                const u32 bit = on ? (rank >> (maxr - d)) & 1u : 0u;
                em(TAU_RP + (int)ctx - 1, on, bit, mlo & (u32)act, mhi & (u32)(act >> 32));
                dc_refine(bit, 0u, mlo, mhi);
            }
        }
    }
    if (SIDES & 2) {
        const u32 run = it.run;
        const int nb = (valid && run != 1u) ? bsr(run) : 0;
        if (__ballot(valid)) es(8, valid, run != 1u ? 1u : 0u);
        for (int sx = 0; sx < 31; ++sx) { const bool on = sx < nb; if (!__ballot(on)) break; es(9 + sx, on, sx + 1 < nb ? 1u : 0u); }
        if (__ballot(nb != 0)) {
            u32 mlo, mhi;
            dc_peers<5>((u32)nb, nb != 0, mlo, mhi);
            const u32 keep = nb > 5 ? ~0u : 0u;                                 // more than 5 bits: one row per depth, no tree
            for (int d = 0; d < 31; ++d) {
                const bool on = d < nb;
                const u64 act = __ballot(on);
                if (!act) break;
                const u32 ctx = on ? (nb <= 5 ? (run >> (nb - d)) : (u32)(1 + d)) : 1u;
                const u32 bit = on ? (run >> (nb - 1 - d)) & 1u : 0u;
                em(on ? TAU_NM + nm_off(nb) + (int)ctx - 1 : 0, on, bit, mlo & (u32)act, mhi & (u32)(act >> 32));
                dc_refine(bit, keep, mlo, mhi);
            }
        }
    }
}

// 2a. per wave-chunk: decisions per row and in total.  Which rows a run contributes to is a function of (rank, B < max_rank)
// on the rank side and of the run length's class on the run side, and every row collects a contiguous range of those values
// (a tree node = a prefix of the value): so the wavefront only histograms its runs into DC_BINS bins (two LDS atomics per run)
// and turns the prefix sums of the bins into row counts at the end through a table built on the host from the model itself
// (dc_build_rowbins).  Runs under escape coding (avg_rank >= 32; their rows depend on max_rank) are counted directly.
constexpr int DC_BIN_RUN = 512;        // bins [0, 256): rank, B >= max_rank or rank < 2; [256, 512): rank, B < max_rank; [512, 608): run classes
constexpr int DC_BINS = 640;           // padded to 10 per lane
__host__ __device__ __forceinline__ u32 dc_rank_bin(u32 rank, int maxr) { const int B = rank != 1u ? bsr(rank) : 0; return rank | ((B != 0 && B < maxr) ? 256u : 0u); }
__host__ __device__ __forceinline__ u32 dc_run_bin(u32 run) { return (u32)DC_BIN_RUN + (run < 64u ? run : 64u + (u32)bsr(run)); }

template <int SIDES, class SB>
__global__ __launch_bounds__(WG) void dc_part_count_kernel(const u64* __restrict__ items, DcGeom g, SB S, const DcRowBins* __restrict__ rowbins,
                                                           u32* __restrict__ cnt /*[DC_ROWS][W]*/, u32* __restrict__ wdec)
{
    typedef DcForm<SB> F;
    const u32 mrp = F::maxr_word(S);                                  // max_rank of the eight sub-blocks, one scalar word
    __shared__ u32 bins[WAVES][DC_BINS + 8];
    __shared__ u32 hrp[WAVES][256];                                             // escape rows (TAU_RP + ctx - 1), counted directly
    for (u32 i = threadIdx.x; i < WAVES * (DC_BINS + 8); i += WG) (&bins[0][0])[i] = 0;
    for (u32 i = threadIdx.x; i < WAVES * 256; i += WG) (&hrp[0][0])[i] = 0;
    __syncthreads();
    const u32 w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const u32 wc = blockIdx.x * WAVES + w;
    u32* bw = &bins[w][0];
    u32 total = 0;
    if (wc < g.W) {
        const u64 i0 = (u64)wc * g.per_wave;
        u64 i1 = i0 + g.per_wave; if (i1 > g.m) i1 = g.m;
        // four items per lane and trip, their loads issued together: with one load in flight per wavefront the ~108 trips of a wave-chunk
        // each waited out a full memory latency (0.17 ms per job for 225 MB: round 5 counters, 80 % of the wave cycles parked)
        // (round 6: the NEXT trip's four loads are in flight while this trip's items are counted — nothing but LDS atomics between them, so
        // the compiler waits with an exact vmcnt; before, every one of a wave-chunk's ~27 trips waited out a full memory round trip)
        u64 nx[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) { const u64 i = i0 + 64u * (u32)u + lane; nx[u] = items[i < i1 ? i : i0]; }
        for (u64 base = i0; base < i1; base += 256) {
            u64 kk[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) kk[u] = nx[u];
#pragma unroll
            for (int u = 0; u < 4; ++u) { const u64 i = base + 256u + 64u * (u32)u + lane; nx[u] = items[i < i1 ? i : i0]; }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                if (base + 64u * (u32)u + lane >= i1) continue;
                const typename F::It it = F::unpack(kk[u]);
                const int maxr = F::maxr(it, mrp);
                if (SIDES & 1) {
                    total += (u32)count_rank_side(it, maxr);
                    if (it.ge32) {
                        for (int d = 0; d <= maxr; ++d) atomicAdd(&hrp[w][((1u << d) | ((it.rank >> (maxr + 1 - d)) & ((1u << d) - 1u))) - 1u], 1u);
                    } else atomicAdd(&bw[dc_rank_bin(it.rank, maxr)], 1u);
                }
                if (SIDES & 2) { total += (u32)count_run_side(it); atomicAdd(&bw[dc_run_bin(it.run)], 1u); }
            }
        }
    }
    __syncthreads();
    {   // exclusive prefix sums of the wave's bins, 10 consecutive bins per lane
        u32 loc[DC_BINS / 64], sum = 0;
#pragma unroll
        for (int q = 0; q < DC_BINS / 64; ++q) { loc[q] = bw[lane * (DC_BINS / 64) + q]; sum += loc[q]; }
        u32 run = wave_incl_sum(sum) - sum;
#pragma unroll
        for (int q = 0; q < DC_BINS / 64; ++q) { bw[lane * (DC_BINS / 64) + q] = run; run += loc[q]; }
    }
    total = wave_incl_sum(total);
    __syncthreads();
    if (wc < g.W) {
        for (u32 h = lane; h < (u32)DC_ROWS; h += 64) {
            const DcRowBins rb = rowbins[h];
            u32 v = bw[rb.hi1] - bw[rb.lo1] + bw[rb.hi2] - bw[rb.lo2];
            if (h >= (u32)TAU_RP && h < (u32)TAU_NF) v += hrp[w][h - TAU_RP];
            cnt[(size_t)h * g.W + wc] = v;
        }
        if (lane == 63) wdec[wc] = total;
    }
}

// 2b. scans: rows over wave-chunks (one workgroup per row), then row bases and the wave-chunks' decision offsets
__global__ __launch_bounds__(WG) void dc_scan_rows_kernel(u32* __restrict__ cnt, u32 W, u32* __restrict__ rowtot)
{
    __shared__ u32 scr[8];
    u32* row = cnt + (size_t)blockIdx.x * W;
    u32 carry = 0;
    for (u32 base = 0; base < W; base += WG) {
        const u32 i = base + threadIdx.x;
        const u32 v = (i < W) ? row[i] : 0u;
        u32 tot;
        const u32 ex = block_excl_sum(v, scr, &tot);
        if (i < W) row[i] = carry + ex;
        carry += tot;
        __syncthreads();
    }
    if (threadIdx.x == 0) rowtot[blockIdx.x] = carry;
}
__global__ __launch_bounds__(WG) void dc_scan_misc_kernel(const u32* __restrict__ rowtot, u32* __restrict__ rowstart /*[DC_ROWS + 1]*/,
                                                          const u32* __restrict__ wdec, u32 W, u32* __restrict__ wdecoff /*[W+1]*/,
                                                          u32* __restrict__ meta, int job, u32 Dcap)
{
    __shared__ u32 scr[8];
    u32 rc = 0;
    for (u32 base = 0; base < (u32)DC_ROWS; base += WG) {
        const u32 i = base + threadIdx.x;
        const u32 v = (i < (u32)DC_ROWS) ? rowtot[i] : 0u;
        u32 t1;
        const u32 e1 = block_excl_sum(v, scr, &t1);
        if (i < (u32)DC_ROWS) rowstart[i] = rc + e1;
        rc += t1;
        __syncthreads();
    }
    if (threadIdx.x == 0) { rowstart[DC_ROWS] = rc; meta[DM_D0 + job] = rc; if (rc > Dcap) atomicOr(&meta[DM_FAIL], (u32)FAIL_CAP); }
    u32 carry = 0;
    for (u32 base = 0; base < W; base += WG) {
        const u32 i = base + threadIdx.x;
        const u32 v = (i < W) ? wdec[i] : 0u;
        u32 t2;
        const u32 e2 = block_excl_sum(v, scr, &t2);
        if (i < W) wdecoff[i] = carry + e2;
        carry += t2;
        __syncthreads();
    }
    if (threadIdx.x == 0) wdecoff[W] = carry;
}

// lane `lane` of v <- val, both wave-uniform (v_writelane takes one SGPR operand besides m0)
__device__ __forceinline__ int dc_writelane(int v, int val, int lane)
{
    asm volatile("s_mov_b32 m0, %2\n\tv_writelane_b32 %0, %1, m0" : "+v"(v) : "s"(val), "s"(lane) : "m0");
    return v;
}

// 2c. scatter.  One wavefront per wave-chunk walks its items 64 at a time; per canonical round the lanes that have a decision
// are ranked stably inside their row (same type -> same round, so rows never interleave across rounds) and write
//   events[row offset]            = X | sub-block << 8 | bit << 11
//   pos[decision index of item]   = that offset (index into the job's value array)
// The running offsets of the 40 single-row types live in one VGPR (lane = slot; v_readlane with a uniform slot), those of the
// mantissa / escape rows in LDS.  pos is item-major, i.e. every lane owns a short run of it and a direct store per round would
// touch ~20 lines per wavefront instruction (the address path, not the bytes, was the kernel's limit): the tile's entries are
// collected in LDS and leave as whole lines when the tile is done (a tile with more decisions than the stage holds stores directly).
#ifndef DC_POS_STAGE_N
#define DC_POS_STAGE_N 1280
#endif
constexpr u32 DC_POS_STAGE = DC_POS_STAGE_N;
struct __attribute__((packed, aligned(4))) DcPos4 { u32 a, b, c, d; };      // four positions, 4-byte aligned: one dwordx4 store
template <int SIDES, class SB>
__global__ __launch_bounds__(WG) void dc_part_scatter_kernel(const u64* __restrict__ items, DcGeom g, SB S, const u32* __restrict__ meta,
                                                             const u32* __restrict__ cnt, const u32* __restrict__ rowstart,
                                                             const u32* __restrict__ wdecoff, u32 ignoreX,
                                                             u16* __restrict__ events, u32* __restrict__ pos, u32* __restrict__ doff,
                                                             u16* __restrict__ esub /* batched pass: the sub-block of every event */)
{
    typedef DcForm<SB> F;
    const u32 mrp = F::maxr_word(S);                                  // max_rank of the eight sub-blocks, one scalar word
    __shared__ u32 goff[WAVES][DC_ROWS];
    __shared__ u32 spos[WAVES][DC_POS_STAGE];
    if (meta[DM_FAIL] != 0u) return;
    const u32 w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const u32 wc = blockIdx.x * WAVES + w;
    if (wc < g.W) for (u32 h = lane; h < (u32)DC_ROWS; h += 64) goff[w][h] = rowstart[h] + cnt[(size_t)h * g.W + wc];
    __syncthreads();
    if (wc >= g.W) return;
    dc_lds_vu32* vg = (dc_lds_vu32*)&goff[w][0];
    dc_lds_vu32* sp = (dc_lds_vu32*)&spos[w][0];
    int sreg = (lane < (u32)DC_SLOTS) ? (int)goff[w][dc_slot_tau((int)lane)] : 0;     // running offsets of the single-row types
    const u64 i0 = (u64)wc * g.per_wave;
    u64 i1 = i0 + g.per_wave; if (i1 > g.m) i1 = g.m;
    u32 running = wdecoff[wc];                                        // decision index of the tile's first item
    u64 knext = (i0 + lane < i1) ? items[i0 + lane] : 0ull;           // the next tile's items are requested one tile ahead
    for (u64 base = i0; base < i1; base += 64) {
        const u64 i = base + lane;
        const bool valid = i < i1;
        const u64 key = knext;
        // The request for the next tile's items goes out BEHIND the wait for this tile's.  (Round 6, from the ISA: the compiler cannot count the
        // stores of the rounds below — they sit in data-dependent loops — so the wait for `key` is a vmcnt(0); with the request in front of
        // it, as the source order had it, that wait covered the request itself: no prefetch at all, one full memory round trip per tile and
        // wavefront, 0.35 ms of every partition job whatever it had to scatter.)
        asm volatile("" :: "v"(key) : "memory");
        knext = (i + 64 < i1) ? items[i + 64] : 0ull;
        const typename F::It it = F::unpack(key);
        const int maxr = F::maxr(it, mrp);
        u32 nd = 0;
        if (valid) { if (SIDES & 1) nd += (u32)count_rank_side(it, maxr); if (SIDES & 2) nd += (u32)count_run_side(it); }
        const u32 incl = wave_incl_sum(nd);
        const u32 loc = incl - nd;                                    // first decision of this item inside the tile
        if (valid) doff[i] = running + loc;
        const u32 tile_total = (u32)__builtin_amdgcn_readlane((int)incl, 63);      // a scalar: `staged` below is then a scalar
        const bool staged = tile_total <= DC_POS_STAGE;               // branch around every round's position store, not an exec-mask dance
        const u32 sig = (ignoreX ? 0u : item_X(key)) | (F::sig_sb(it) << 8);
        const u16 sub16 = (u16)it.sb;
        u32* mypos = pos + running + loc;
        // (two copies of the rounds, chosen once per tile: with the test inside `put` every round carried a branch around its position store)
        auto rounds = [&](auto staged_tag) __attribute__((always_inline)) {
            constexpr bool STAGED = decltype(staged_tag)::value;
            u32 ord = 0;
            auto put = [&](u32 p) { if (STAGED) sp[loc + ord] = p; else mypos[ord] = p; ++ord; };
            dc_item_rounds<SIDES>(it, valid, maxr,
                [&](int slot, bool on, u32 bit) {
                    const u64 m = __ballot(on);
                    const u32 bs = (u32)__builtin_amdgcn_readlane(sreg, slot);
                    if (on) {
                        const u32 p = bs + __builtin_amdgcn_mbcnt_hi((u32)(m >> 32), __builtin_amdgcn_mbcnt_lo((u32)m, 0u));   // peers in lower lanes
                        events[p] = (u16)(sig | (bit << 11));
                        if (F::TAB) esub[p] = sub16;
                        put(p);
                    }
                    sreg = dc_writelane(sreg, (int)(bs + (u32)__popcll(m)), slot);                    // (was: compare, move, select)
                },
                [&](int tau, bool on, u32 bit, u32 mlo, u32 mhi) {
                    const u32 h = on ? (u32)tau : 0u;
                    const u32 before = vg[h];
                    const u32 rr = __builtin_amdgcn_mbcnt_hi(mhi, __builtin_amdgcn_mbcnt_lo(mlo, 0u));
                    const u32 cn = (u32)(__popc(mlo) + __popc(mhi));
                    if (on) {
                        const u32 p = before + rr;
                        vg[h] = before + cn;                                  // every peer writes the same value (was: the highest one, behind a compare and a branch)
                        events[p] = (u16)(sig | (bit << 11));
                        if (F::TAB) esub[p] = sub16;
                        put(p);
                    }
                });
        };
        if (staged) rounds(std::true_type()); else rounds(std::false_type());
        // the tile's positions leave as 16-byte stores (four entries per lane: two store instructions for an average tile instead of seven)
        if (staged) {
            for (u32 t = 4u * lane; t < tile_total; t += 256u) {
                if (t + 4u <= tile_total) {
                    DcPos4 v; v.a = sp[t]; v.b = sp[t + 1]; v.c = sp[t + 2]; v.d = sp[t + 3];
                    *reinterpret_cast<DcPos4*>(pos + running + t) = v;
                } else for (u32 x = t; x < tile_total; ++x) pos[running + x] = sp[x];
            }
        }
        running += tile_total;
    }
    if (wc == g.W - 1 && lane == 0) doff[g.m] = running;
}

// 2d. the fast coder (-e0) has ONE family, so the stream-order job has no chains to lay out — but the p stream still needs to know
// where every run's entries go: doff[i] = decision index of item i's first decision, exactly what dc_part_scatter leaves behind.
template <int SIDES, class SB>
__global__ __launch_bounds__(WG) void dc_doff_kernel(const u64* __restrict__ items, DcGeom g, SB S, const u32* __restrict__ meta,
                                                     const u32* __restrict__ wdecoff, u32* __restrict__ doff)
{
    typedef DcForm<SB> F;
    const u32 mrp = F::maxr_word(S);                                  // max_rank of the eight sub-blocks, one scalar word
    if (meta[DM_FAIL] != 0u) return;
    const u32 w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const u32 wc = blockIdx.x * WAVES + w;
    if (wc >= g.W) return;
    const u64 i0 = (u64)wc * g.per_wave;
    u64 i1 = i0 + g.per_wave; if (i1 > g.m) i1 = g.m;
    u32 running = wdecoff[wc];
    u64 knext = (i0 + lane < i1) ? items[i0 + lane] : 0ull;          // the next tile's items are requested one tile ahead
    for (u64 base = i0; base < i1; base += 64) {
        const u64 i = base + lane;
        const bool valid = i < i1;
        const u64 key = knext;
        asm volatile("" :: "v"(key) : "memory");                     // (wait for this tile's items, THEN request the next tile's: dc_part_scatter_kernel)
        const typename F::It it = F::unpack(key);
        knext = (i + 64 < i1) ? items[i + 64] : 0ull;
        const int maxr = F::maxr(it, mrp);
        u32 nd = 0;
        if (valid) { if (SIDES & 1) nd += (u32)count_rank_side(it, maxr); if (SIDES & 2) nd += (u32)count_run_side(it); }
        const u32 incl = wave_incl_sum(nd);
        if (valid) doff[i] = running + incl - nd;
        running += (u32)__builtin_amdgcn_readlane((int)incl, 63);
    }
    if (wc == g.W - 1 && lane == 0) doff[g.m] = running;
}

// ---------------------------------------------------------------------------------------------------------------------
// 3. chain evaluation over chain-major events
// ---------------------------------------------------------------------------------------------------------------------
struct DcEvalJob { const u16* events; u32 E; const u32* rowstart; int fam; };      // rowstart[DC_ROWS + 1]: row = decision type

template <class P>
__device__ __forceinline__ u32 dc_find_row(P rowstart, u32 k)
{
    u32 lo = 0, hi = DC_ROWS;                                          // largest row with rowstart[row] <= k
    while (lo + 1 < hi) { const u32 mid = (lo + hi) >> 1; if (rowstart[mid] <= k) lo = mid; else hi = mid; }
    return lo;
}

// Phases a and c as one wavefront per 64 chunks: the lanes own one chunk each (a serial chain), but memory is touched as
// full lines — for every batch of 64 events per lane the wavefront loads the 64 lanes' 128-byte pieces cooperatively
// (8 x 16 B per lane, eight rows per instruction), transposes them through LDS, and (phase c) writes the values back the same
// way.  The next batch is in flight while the current one is walked.
#ifndef DC_EVAL_TIMING
#define DC_EVAL_TIMING 0
#endif
constexpr int DC_EROW = DC_EB * 2 + 16;         // LDS row pitch in bytes (padded)
// all four jobs of a block in one launch (they are independent, and one job alone leaves most SIMDs idle: a lane is a serial chain)
struct DcEvalAll { DcEvalJob job[4]; u32 wstart[5]; u32 cstart[5]; u16* V[4]; u16* sink; u32 ev; };   // first wavefront / first chunk of each job; events per chunk

// First event of every non-empty row gets DC_ROWMARK: inside the rows of one class (same update rates) a walk then needs no row
// bookkeeping at all — a chain ends where the signature changes or a marked event begins.  (DC_ROWMARK: devcoder_model.h)
__global__ __launch_bounds__(WG) void dc_mark_rows_kernel(DcEvalAll A)
{
    const u32 g = blockIdx.x * WG + threadIdx.x;
    if (g >= 4u * DC_ROWS) return;
    const DcEvalJob J = A.job[g / DC_ROWS];
    if (J.E == 0) return;                                              // a job that does not run in this mode (its row table is not valid)
    const u32 r = g % DC_ROWS;
    const u32 rs = J.rowstart[r], re = J.rowstart[r + 1];
    if (re > rs) const_cast<u16*>(J.events)[rs] |= (u16)DC_ROWMARK;
}
// A batched pass (up to 8192 sub-blocks) keeps the 16-bit event: its signature holds the sub-block modulo 8, which alone would walk
// two chains as one wherever a symbol (or a decision type of the context-free family) occurs in sub-blocks s and s + 8 k and in none
// between — their chains are neighbours in the row.  The scatter therefore also writes every event's full sub-block id to a parallel
// array, and this pass turns it into the mark the walks already honour: an event whose id differs from its predecessor's starts a
// chain.  Inside a row the events of one X are in stream order, i.e. sub-block-major, so (signature change) or (id change) or (row
// start) is exactly "another chain" — the identity is exact, and the evaluation kernels read nothing new.  Thread per 8 events.
struct DcMarkAll { u16* events[4]; const u16* esub[4]; u32 E[4]; };
__global__ __launch_bounds__(WG) void dc_mark_chains_kernel(DcMarkAll A, const u32* __restrict__ meta)
{
    if (meta[DM_FAIL] != 0u) return;
    const u32 E = A.E[blockIdx.y];
    const u64 k0 = ((u64)blockIdx.x * WG + threadIdx.x) * 8u;
    if (k0 >= E) return;
    const u16* __restrict__ es = A.esub[blockIdx.y];
    u16* __restrict__ ev = A.events[blockIdx.y];
    const uint4 q = *reinterpret_cast<const uint4*>(es + k0);           // (the array has slack behind its last entry; entries past E are not used)
    const u32 w[4] = {q.x, q.y, q.z, q.w};
    u32 prev = k0 > 0 ? (u32)es[k0 - 1] : (w[0] & 0xffffu);
#pragma unroll
    for (u32 x = 0; x < 8; ++x) {
        const u32 id = (w[x >> 1] >> (16u * (x & 1u))) & 0xffffu;
        if (id != prev && k0 + x < E) ev[k0 + x] |= (u16)DC_ROWMARK;
        prev = id;
    }
}

// first row of each class, and one past the last
__device__ __forceinline__ int dc_class_first_row(int cls)
{
    return cls == CLS_RF ? TAU_RF : cls == CLS_RE ? TAU_RE : cls == CLS_RM ? TAU_RM : cls == CLS_RP ? TAU_RP : cls == CLS_NF ? TAU_NF
         : cls == CLS_NE ? TAU_NE : cls == CLS_NM ? TAU_NM : cls == CLS_NM2 ? TAU_NM2 : DC_ROWS;
}

// A wavefront is self-contained here (its own LDS slices, no workgroup barrier); four of them form a workgroup only so that the
// hardware puts them on the four SIMDs of one CU — launched as single-wave workgroups, a tenth of the ~1000 wavefronts ended up
// two to a SIMD while other SIMDs stayed empty, and the kernel took 1.6 x as long as its median wavefront.
constexpr int DC_EVAL_WAVES = 4;
constexpr int DC_EVAL_LDS_WAVE = 2 * 64 * DC_EROW;                                             // sin + sout
constexpr int DC_EVAL_LDS = DC_EVAL_WAVES * (DC_EVAL_LDS_WAVE + NUM_CLS * 4 + NUM_CLS * (int)sizeof(Rates));   // + class ends, rates
__device__ __forceinline__ void dc_wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");           // LDS operations of one wavefront execute in order: only the compiler has to be told
    __builtin_amdgcn_wave_barrier();
}

template <bool WRITE>
__global__ __launch_bounds__(64 * DC_EVAL_WAVES) void dc_eval_wave_kernel(DcEvalAll A, const ModelParams* __restrict__ mp, const u32* __restrict__ meta,
                                                          u16* __restrict__ elo_all, u16* __restrict__ ehi_all, const u16* __restrict__ Sv_all, u32* __restrict__ tdbg)
{
#if DC_EVAL_TIMING
    const u64 t_begin = wall_clock64();
    u32 slow_batches = 0;
#endif
    extern __shared__ __attribute__((aligned(16))) u8 dc_eval_lds[];
    const u32 wv = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    u8* const sin = dc_eval_lds + wv * DC_EVAL_LDS_WAVE;
    u8* const sout = sin + 64 * DC_EROW;
    // where each class's rows end (in events) and the family's rates per class: all a walk needs besides the events themselves
    u32* const sclsend = reinterpret_cast<u32*>(dc_eval_lds + DC_EVAL_WAVES * DC_EVAL_LDS_WAVE) + wv * NUM_CLS;
    Rates* const srate = reinterpret_cast<Rates*>(dc_eval_lds + DC_EVAL_WAVES * (DC_EVAL_LDS_WAVE + NUM_CLS * 4)) + wv * NUM_CLS;
    const u32 gw = blockIdx.x * DC_EVAL_WAVES + wv;                    // this wavefront among all of the launch
    if (meta[DM_FAIL] != 0u || gw >= A.wstart[4]) return;
    int jb = 0;
#pragma unroll
    for (int q = 1; q < 4; ++q) if (gw >= A.wstart[q]) jb = q;
    const DcEvalJob J = A.job[jb];
    if (lane < (u32)NUM_CLS) {
        srate[lane] = mp->rates[lane][J.fam];
        sclsend[lane] = J.rowstart[dc_class_first_row((int)lane + 1)];
    }
    dc_wave_sync();
    u16* const elo = elo_all + A.cstart[jb];
    u16* const ehi = ehi_all + A.cstart[jb];
    const u16* const Sv = Sv_all + A.cstart[jb];
    u16* const Vout = A.V[jb];
    const u32 wave = gw - A.wstart[jb];
    const u32 c = wave * 64 + lane;
    const u32 EV = A.ev;                                               // multiple of DC_EB
    const u64 k0 = (u64)c * EV;
    const bool mine = k0 < J.E;
    const u32 k1 = mine ? (u32)((k0 + EV < J.E) ? k0 + EV : J.E) : 0u;
    // cooperative mapping: instruction i moves 16 bytes of row 8 i + lane / 8, column lane % 8
    const u32 crow = lane >> 3, ccol = lane & 7u;
    const u64 wave_k0 = (u64)wave * 64 * EV;

    u32 cls = 0, clsend = 0, prev = 0xffffu;
    int init = mp->init[0];                                            // the value a chain of the current class starts from
    int lo = init, hi = init;
    Rates R = srate[0];
    if (mine) {
        while (cls + 1 < (u32)NUM_CLS && sclsend[cls] <= (u32)k0) ++cls;                     // class of the row that owns event k0
        clsend = sclsend[cls];
        R = srate[cls];
        init = mp->init[cls];
        // a chunk that starts a row starts with a marked event; otherwise the chain may continue from the event before
        prev = (k0 > 0) ? ((u32)J.events[k0 - 1] & DC_SIGMASK) : 0xffffu;
        if (WRITE) { lo = Sv[c]; hi = lo; } else { lo = mp->vmin[cls][J.fam]; hi = mp->vmax[cls][J.fam]; }
    }
    auto fetch = [&](u32 b, uint4* q) {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            // no branch around a global load or store in this kernel (past the end: a clamped address / a sink slot): the compiler
            // then knows how many are outstanding and waits for the prefetched batch with an exact vmcnt, not for the stores behind it
            const u64 kk = wave_k0 + (u64)(8 * i + crow) * EV + (u64)b * DC_EB + ccol * 8;
            const u64 ka = kk < J.E ? kk : 0ull;
            const uint4 val = *reinterpret_cast<const uint4*>(J.events + ka);
            q[i].x = val.x; q[i].y = val.y; q[i].z = val.z; q[i].w = val.w;          // (member-wise: a whole-vector copy through the select made the array live in scratch)
        }
    };
    auto store_out = [&](u32 b) {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const u64 kk = wave_k0 + (u64)(8 * i + crow) * EV + (u64)b * DC_EB + ccol * 8;
            *reinterpret_cast<uint4*>(kk < J.E ? Vout + kk : A.sink + lane * 8) = *reinterpret_cast<const uint4*>(sout + (8 * i + crow) * DC_EROW + ccol * 16);
        }
    };
    uint4 nxt[8];
    fetch(0, nxt);
    const u32 NB = EV / DC_EB;
    for (u32 b = 0; b < NB; ++b) {
#pragma unroll
        for (int i = 0; i < 8; ++i) *reinterpret_cast<uint4*>(sin + (8 * i + crow) * DC_EROW + ccol * 16) = nxt[i];
        dc_wave_sync();
        // the values of the batch before leave now, a whole walk ahead of the next wait on the memory counter (the loads below are
        // waited for at the top of the next iteration, and the counter is in order: stores issued after them would be waited for too)
        if (WRITE && b > 0) store_out(b - 1);
        fetch(b + 1 < NB ? b + 1 : b, nxt);                            // (the last batch is simply fetched again)
        const u32 kb = (u32)k0 + b * DC_EB;
        if (mine && kb < k1) {
            const u8* myrow = sin + lane * DC_EROW;
            u8* orow = sout + lane * DC_EROW;
            const u32 lim = k1 < clsend ? k1 : clsend;
            if (kb + DC_EB <= lim) {
                // whole batch inside one class (one set of rates): straight-line walk from registers
                const int c0 = R.t0 * R.a0 + R.r0, c1 = R.t1 * R.a1 + R.r1;
#pragma unroll
                for (int g8 = 0; g8 < 8; ++g8) {
                    const uint4 q = *reinterpret_cast<const uint4*>(myrow + g8 * 16);
                    const u32 wds[4] = {q.x, q.y, q.z, q.w};
                    u32 outw[4] = {0, 0, 0, 0};
#pragma unroll
                    for (int x = 0; x < 8; ++x) {
                        const u32 e = (wds[x >> 1] >> (16 * (x & 1))) & 0xffffu;
                        const u32 sigm = e & (DC_SIGMASK | DC_ROWMARK);                      // a marked event never equals prev
                        if (sigm != prev) { lo = init; hi = init; }
                        prev = e & DC_SIGMASK;
                        // dcm::step with the target, rate and rounding picked by the bit first, so that both ends of the bracket
                        // share the selects (static coder: bit 1 is v - (((v - t1) a1) >> 12) = v + (((t1 - v) a1 + 4095) >> 12) —
                        // floor of a negated quotient = minus its ceiling —, bit 0 is v + (((t0 - v) a0) >> 12); devcoder_model.h)
                        // (round 5: (t - v) a + r = (t a + r) - v a with c = t a + r fixed per class and bit — two selects and three operations
                        // per step instead of three and four; all products stay below 2^24: |v| < 2^13, a < 2^11, c < 2^24)
                        const bool b1 = (e & 0x800u) != 0u;
                        const int Cc = b1 ? c1 : c0, Aa = b1 ? R.a1 : R.a0;
                        if (WRITE) outw[x >> 1] |= (u32)lo << (16 * (x & 1));
                        lo += (Cc - __mul24(lo, Aa)) >> 12;
                        if (!WRITE) hi += (Cc - __mul24(hi, Aa)) >> 12;
                    }
                    if (WRITE) *reinterpret_cast<uint4*>(orow + g8 * 16) = make_uint4(outw[0], outw[1], outw[2], outw[3]);
                }
            } else {
                // a class boundary or the end of the chunk inside the batch (a handful of batches per launch)
#if DC_EVAL_TIMING
                ++slow_batches;
#endif
                const u32 cnt = (k1 - kb < (u32)DC_EB) ? k1 - kb : (u32)DC_EB;
                for (u32 x = 0; x < cnt; ++x) {
                    const u32 k = kb + x;
                    while (k >= clsend && cls + 1 < (u32)NUM_CLS) { ++cls; clsend = sclsend[cls]; R = srate[cls]; init = mp->init[cls]; }
                    const u32 e = *reinterpret_cast<const u16*>(myrow + 2 * x);
                    if ((e & (DC_SIGMASK | DC_ROWMARK)) != prev) { lo = init; hi = init; }
                    prev = e & DC_SIGMASK;
                    const u32 bt = (e >> 11) & 1u;
                    if (WRITE) *reinterpret_cast<u16*>(orow + 2 * x) = (u16)lo;
                    lo = step(lo, bt, R);
                    if (!WRITE) hi = step(hi, bt, R);
                }
            }
        }
        dc_wave_sync();
    }
    if (WRITE) store_out(NB - 1);
    if (!WRITE && mine) { elo[c] = (u16)lo; ehi[c] = (u16)hi; }
#if DC_EVAL_TIMING
    {
        u32 sb = slow_batches;
        for (int d = 32; d >= 1; d >>= 1) { const u32 o = (u32)__shfl_xor((int)sb, d, 64); sb = sb > o ? sb : o; }
        if (lane == 0) { tdbg[3 * gw] = (u32)(t_begin & 0xffffffffu); tdbg[3 * gw + 1] = (u32)(wall_clock64() - t_begin); tdbg[3 * gw + 2] = sb | ((u32)jb << 16); }
    }
#endif
}

__device__ __forceinline__ bool dc_chunk_continues(const DcEvalJob& J, u32 c, u32 EV)
{
    if (c == 0) return false;
    const u32 k0 = c * EV;
    u32 row = dc_find_row(J.rowstart, k0);
    if (J.rowstart[row] == k0) return false;                          // a row (hence a chain) starts exactly here
    // (an empty row cannot own k0: dc_find_row returns the last row starting at or before k0, which then is non-empty or k0 >= E)
    // (a marked event starts a chain: a row — tested above — or, in a batched pass, another sub-block with the same signature)
    const u32 e1 = J.events[k0];
    return ((((u32)J.events[k0 - 1] ^ e1) & DC_SIGMASK) | (e1 & DC_ROWMARK)) == 0;
}

// ---------------------------------------------------------------------------------------------------------------------
// 3'. open chunk starts resolved exactly (BSCGPU_OPT_DC_REPLAY_EXACT; devcoder_model.h: replay_resolve_host restates these kernels).
// Chunk c is OPEN iff it continues a chain and the bracket of chunk c - 1 has not met; today one lane of dc_eval_b_kernel then walks back
// to the nearest known start and replays everything in between, and gives the unit up (FAIL_REPLAY) behind DC_REPLAY_MAX chunks.  The
// maps are monotone, so the exact start of an open chunk lies inside the bracket in front of it, and a chunk can be walked from every
// value of that bracket at once: dc_rp_map_kernel, one wavefront per chunk whose successor is open — the head of a stretch (its own
// start is known) from that one value, every other chunk from all w = ehi - elo + 1 values of its start bracket, ceil(w / 64) per lane —,
// then dc_rp_chain_kernel, one lane per stretch, follows the maps from the head and CLOSES the brackets (elo = ehi = exact start of the
// next chunk), so that dc_eval_b_kernel, unchanged, finds nothing to replay.  A chunk whose end bracket is open holds no chain boundary
// (a boundary resets both ends to the same value) and is a full chunk (it has a successor): one row, one set of rates, a bare loop.
// The guard: a start bracket of more than `cand` values (DC_RP_CAND, which the contraction of the maps rules out — tools/
// replay_resolve_probe.cpp bound —, or what BSC_DC_REPLAY_CAND lowers it to) is not walked; the chain stops there and what lies behind
// it in the stretch is left to dc_eval_b_kernel's replay.
// ---------------------------------------------------------------------------------------------------------------------
static_assert(DC_RP_CAND % 64 == 0 && DC_RP_CAND / 64 == 6, "dc_rp_map_kernel: candidates per lane");

// N chains over the same nq x 8 events, interleaved (their dependent steps fill each other's issue gaps); the events 16 bytes per load
// with four loads in flight, as the replay loop of dc_eval_b_kernel; the step in the form of dc_eval_wave_kernel (c = t a + r per bit)
template <int N>
__device__ __forceinline__ void dc_rp_walk(const uint4* __restrict__ ev, u32 nq, const Rates& R, int (&v)[N])
{
    const int c0 = R.t0 * R.a0 + R.r0, c1 = R.t1 * R.a1 + R.r1;
    uint4 qb[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) qb[i] = ev[(u32)i < nq ? (u32)i : 0u];
    for (u32 i = 0; i < nq; ++i) {
        const uint4 q = qb[0];
        qb[0] = qb[1]; qb[1] = qb[2]; qb[2] = qb[3];
        qb[3] = ev[i + 4u < nq ? i + 4u : i];
        const u32 wds[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int x = 0; x < 8; ++x) {
            const bool b1 = ((wds[x >> 1] >> (16 * (x & 1) + 11)) & 1u) != 0u;
            const int Cc = b1 ? c1 : c0, Aa = b1 ? R.a1 : R.a0;
#pragma unroll
            for (int k = 0; k < N; ++k) v[k] += (Cc - __mul24(v[k], Aa)) >> 12;
        }
    }
}

// the candidates lane + 64 k of a start bracket of w values from lo0 (a lane past the bracket walks its last value again and stores nothing)
template <int N>
__device__ __forceinline__ void dc_rp_candidates(const uint4* __restrict__ ev, u32 nq, const Rates& R, u32 lane, u32 lo0, u32 w, u32 base, u16* __restrict__ map)
{
    int v[N];
#pragma unroll
    for (int k = 0; k < N; ++k) { const u32 cv = lane + 64u * (u32)k; v[k] = (int)(lo0 + (cv < w ? cv : w - 1u)); }
    dc_rp_walk<N>(ev, nq, R, v);
#pragma unroll
    for (int k = 0; k < N; ++k) { const u32 cv = lane + 64u * (u32)k; if (cv < w) map[cv] = (u16)((u32)v[k] - base); }
}

// one wavefront per chunk slot (all jobs in one launch); nearly all leave behind two loads: their bracket has met
__global__ __launch_bounds__(WG) void dc_rp_map_kernel(DcEvalAll A, const ModelParams* __restrict__ mp, const u32* __restrict__ meta,
                                                       const u16* __restrict__ elo_all, const u16* __restrict__ ehi_all, DcRpRec Q)
{
    if (meta[DM_FAIL] != 0u) return;
    const u32 lane = threadIdx.x & 63u;
    const u32 g = (u32)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * WAVES + (threadIdx.x >> 6)));
    if (g >= A.cstart[4]) return;
    int jb = 0;
#pragma unroll
    for (int q = 1; q < 4; ++q) if (g >= A.cstart[q]) jb = q;
    const DcEvalJob J = A.job[jb];
    const u16* elo = elo_all + A.cstart[jb]; const u16* ehi = ehi_all + A.cstart[jb];
    const u32 p = g - A.cstart[jb], EV = A.ev;
    u32 state = DC_RP_NONE;
    // (elo / ehi of a slot past the job's last chunk are not written: the test on E comes first)
    if ((u64)(p + 1u) * EV < J.E && elo[p] != ehi[p] && dc_chunk_continues(J, p + 1u, EV)) {
        const int cls = tau_class((int)dc_find_row(J.rowstart, p * EV));
        const Rates R = mp->rates[cls][J.fam];
        const uint4* ev = reinterpret_cast<const uint4*>(J.events + (size_t)p * EV);
        const u32 nq = EV / 8u;
        const bool cont = dc_chunk_continues(J, p, EV);
        // (!cont cannot be: a chunk that starts a chain resets both ends at its first event, so its end bracket would have met.  The arm
        // stays so that no index rests on that argument: p - 1 is read only where the chunk continues, i.e. p > 0.)
        if (!cont || elo[p - 1u] == ehi[p - 1u]) {
            int v[1] = {cont ? (int)elo[p - 1u] : (int)mp->init[cls]};
            dc_rp_walk<1>(ev, nq, R, v);
            if (lane == 0) Q.head[g] = (u16)v[0];
            state = DC_RP_HEAD;
        } else {
            const u32 lo0 = elo[p - 1u], w = (u32)ehi[p - 1u] - lo0 + 1u, base = elo[p];
            u16* map = Q.map + (size_t)g * DC_RP_CAND;
            if (w > Q.cand) state = DC_RP_WIDE;
            else {
                if (w <= 64u) dc_rp_candidates<1>(ev, nq, R, lane, lo0, w, base, map);
                else if (w <= 128u) dc_rp_candidates<2>(ev, nq, R, lane, lo0, w, base, map);
                else if (w <= 256u) dc_rp_candidates<4>(ev, nq, R, lane, lo0, w, base, map);
                else dc_rp_candidates<6>(ev, nq, R, lane, lo0, w, base, map);
                state = DC_RP_MAP;
            }
        }
    }
    if (lane == 0) Q.st[g] = (u8)state;
}

// One lane per stretch: from the head's exact end through the maps, closing every bracket on the way.  Stretches are disjoint, so
// the lane is the only writer of its entries; a bracket's lower end is read (the base of the next chunk's candidates) before it is
// overwritten.  One dependent load per chunk (the map entry; the next chunk's state and lower end are requested with it).
__global__ __launch_bounds__(WG) void dc_rp_chain_kernel(DcEvalAll A, u32* __restrict__ meta, u16* elo_all, u16* ehi_all, DcRpRec Q)
{
    if (meta[DM_FAIL] != 0u) return;
    const u32 g = blockIdx.x * WG + threadIdx.x;
    if (g >= A.cstart[4] || Q.st[g] != DC_RP_HEAD) return;
    u32 gend = A.cstart[4];
#pragma unroll
    for (int q = 3; q >= 1; --q) if (g < A.cstart[q]) gend = A.cstart[q];
    u32 x = Q.head[g], base = elo_all[g];
    elo_all[g] = (u16)x; ehi_all[g] = (u16)x;
    u32 n = 1, p = g + 1u;
    u32 st_n = p < gend ? (u32)Q.st[p] : (u32)DC_RP_NONE, lo_n = p < gend ? (u32)elo_all[p] : 0u;
    while (st_n == (u32)DC_RP_MAP) {
        const u32 lo = lo_n, idx = x - base;
        if (idx >= (u32)DC_RP_CAND) break;                              // (monotone maps: never; what follows then takes the serial replay)
        const u32 mv = Q.map[(size_t)p * DC_RP_CAND + idx];
        const u32 pn = p + 1u;
        st_n = pn < gend ? (u32)Q.st[pn] : (u32)DC_RP_NONE; lo_n = pn < gend ? (u32)elo_all[pn] : 0u;
        x = lo + mv; base = lo;
        elo_all[p] = (u16)x; ehi_all[p] = (u16)x;
        ++n; p = pn;
    }
    atomicAdd(&meta[DM_REPLAY_RESOLVED], n);
}

// exact value at the start of every chunk that begins inside a chain (all jobs in one launch; thread per chunk)
__global__ __launch_bounds__(WG) void dc_eval_b_kernel(DcEvalAll A, const ModelParams* __restrict__ mp, u32* __restrict__ meta,
                                                       const u16* __restrict__ elo_all, const u16* __restrict__ ehi_all, u16* __restrict__ Sv_all)
{
    if (meta[DM_FAIL] != 0u) return;
    const u32 g = blockIdx.x * WG + threadIdx.x;
    if (g >= A.cstart[4]) return;
    int jb = 0;
#pragma unroll
    for (int q = 1; q < 4; ++q) if (g >= A.cstart[q]) jb = q;
    const DcEvalJob J = A.job[jb];
    const u16* elo = elo_all + A.cstart[jb]; const u16* ehi = ehi_all + A.cstart[jb]; u16* Sv = Sv_all + A.cstart[jb];
    const u32 c = g - A.cstart[jb];
    const u32 EV = A.ev;
    const u64 k0 = (u64)c * EV;
    if (k0 >= J.E) return;
    const int init_c = mp->init[tau_class((int)dc_find_row(J.rowstart, (u32)k0))];     // what a chain of this chunk's first row starts from
    if (!dc_chunk_continues(J, c, EV)) { Sv[c] = (u16)init_c; return; }
    if (elo[c - 1] == ehi[c - 1]) { Sv[c] = elo[c - 1]; return; }
    // the predecessor did not coalesce: replay from the nearest chunk whose start value is known
    // (the chunks walked here hold no chain boundary — see below —, so they are all of this chunk's row and class)
    u32 j = c - 1;
    int start = init_c;
    u32 depth = 1;
    for (;;) {
        if (!dc_chunk_continues(J, j, EV)) { start = init_c; break; }
        if (elo[j - 1] == ehi[j - 1]) { start = elo[j - 1]; break; }
        --j; ++depth;
        if (depth > (u32)DC_REPLAY_MAX) { atomicOr(&meta[DM_FAIL], (u32)FAIL_REPLAY); Sv[c] = (u16)init_c; return; }
    }
    atomicAdd(&meta[DM_REPLAYS], depth);
    // Exact walk over chunks j .. c - 1.  None of them coalesced, so none contains a chain boundary (a boundary resets both ends of the
    // bracket to 2048 and they stay equal from there on): one chain, one row, one set of rates — a bare loop, eight events per 16-byte
    // load with four loads in flight (EV is a multiple of 8 and chunks start 16-byte aligned).  The GPU waits for this one lane:
    // 0.37 ms per replayed chunk with the general walk (row look-ups and signature tests per event), 0.32 ms like this (~80 cycles per
    // event: a lone wavefront issues the five dependent operations of a step ~8 cycles apart).  With several contexts on the GPU the
    // other blocks' kernels fill the machine meanwhile.
    const Rates R = mp->rates[tau_class((int)dc_find_row(J.rowstart, j * EV))][J.fam];
    int v = start;
    const uint4* ev = reinterpret_cast<const uint4*>(J.events + (size_t)j * EV);
    const u32 nq = (c - j) * (EV / 8u);
    uint4 qb[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) qb[i] = ev[(u32)i < nq ? (u32)i : 0u];
    for (u32 i = 0; i < nq; ++i) {
        const uint4 q = qb[0];
        qb[0] = qb[1]; qb[1] = qb[2]; qb[2] = qb[3];
        qb[3] = ev[i + 4u < nq ? i + 4u : i];
        const u32 wds[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int x = 0; x < 8; ++x) v = step(v, (wds[x >> 1] >> (16 * (x & 1) + 11)) & 1u, R);
    }
    Sv[c] = (u16)v;
}

// ---------------------------------------------------------------------------------------------------------------------
// 4. probability stream, stream order.  Thread per run.
// ---------------------------------------------------------------------------------------------------------------------
struct DcGather {
    const u64* key_ch; u32 m;
    const u32 *inv_ch, *inv_sr, *inv_sn;
    const u32 *doff_sp, *doff_ch, *doff_sr, *doff_sn;
    const u32 *pos_sp, *pos_ch, *pos_sr, *pos_sn;
    const u16 *V_sp, *V_ch, *V_sr, *V_sn;
};
// pos entries of one run are contiguous but only 4-byte aligned: a packed struct makes the compiler use one dwordx4 load
// (global memory takes dword-aligned multi-dword accesses) instead of four dword loads
struct __attribute__((packed, aligned(4))) DcU4 { u32 a, b, c, d; };

// The entries of a run are 2 bytes each and 1..~20 per run: written straight from the lanes, every store instruction of a wavefront
// touches ~13 lines with 2 bytes per lane, and the same lines again in the next iteration (PMC: WRITE_SIZE 2.66 GB for 0.37 GB of
// entries, and the read-modify-write traffic behind it).  The entries of a wavefront's 64 runs are contiguous in the stream, so
// they are collected in LDS and leave as whole 128-byte pieces (DC_PS_STAGE entries per wavefront; a wavefront with more — 64 runs of
// > 28 decisions on average — stores directly).
#ifndef DC_PS_STAGE_N
#define DC_PS_STAGE_N 1792
#endif
constexpr u32 DC_PS_STAGE = DC_PS_STAGE_N;
typedef __attribute__((address_space(3))) volatile u16 dc_lds_vu16;

// ---- the packed stream (round 6): 13 bits per decision ---------------------------------------------------------------------------
// What the host's range coder needs of a static-coder entry is the probability (12 bits) and the coded bit; the run-start mark only
// placed the reference's budget test (qlfc.cpp:894), and a stream that reaches its budget is redone from the run arrays anyway.
// P13: field = entry & 0x1fff, eight decisions in 13 bytes (field e of a group at bits [13 e, 13 e + 13), little endian); a sub-block's
// stream starts at a multiple of 64 decisions (104 bytes) and is zero-padded to a whole group: 366 -> 298 MB per 64 MiB block over PCIe
// and through the host's DRAM.  The entries of a wavefront's runs are contiguous in the stream, but its piece starts and ends anywhere,
// so a wavefront writes the groups that lie wholly inside its piece (13 bytes per lane and trip) and leaves the fragment of a group
// at either end of it as a 24-byte record; dc_p13_join_kernel then writes the group between every two neighbouring wavefronts from
// the tail record of the one and the head record of the other — no atomics, no zeroed buffer.
struct DcFrag { u32 gidx; u32 slot_count; u16 e[8]; };               // group index (decisions / 8), first slot | count << 8 (count 0: none), the entries
struct DcP13 { u32 pad[8]; u8* out; DcFrag* frag; };                 // pad[sb]: packed index of a decision = its index in the block's stream + pad[its sub-block]
// ... of a batched pass or a segment: up to FRONT_MAX_SUB offsets, a table in HBM indexed by the table's sub-block id (dc_pbase_tab_kernel
// writes it from poff, no host round trip); the index is wave-uniform wherever it is read, so the read is a scalar load
struct DcP13Tab { const u32* pad; u8* out; DcFrag* frag; };
template <class SB> struct DcP13Of;
template <> struct DcP13Of<DcSub> { typedef DcP13 T; };
template <> struct DcP13Of<DcSubTab> { typedef DcP13Tab T; };
struct __attribute__((packed)) DcGroup13 { u32 a, b, c; u8 d; };
__device__ __forceinline__ DcGroup13 dc_pack13(const u32 (&f)[8])
{
    const u64 lo = (u64)f[0] | ((u64)f[1] << 13) | ((u64)f[2] << 26) | ((u64)f[3] << 39) | ((u64)f[4] << 52);
    const u64 hi = (u64)(f[4] >> 12) | ((u64)f[5] << 1) | ((u64)f[6] << 14) | ((u64)f[7] << 27);
    DcGroup13 g; g.a = (u32)lo; g.b = (u32)(lo >> 32); g.c = (u32)hi; g.d = (u8)(hi >> 32);
    return g;
}
// The wavefront's staged entries sg[0 .. wtotal) are the decisions wbase .. of the block's stream; loc / nd / sb / valid: this lane's run.
// The same walk serves a table (P13Q = DcP13Tab), where a wavefront of 64 runs can hold dozens of whole sub-blocks (blocks of a handful
// of runs): every sub-block has at least one run, so the s2 loop trips once per sub-block present, each trip a piece that starts on its
// sub-block's first decision — a multiple of 64 in the packed space — except the first.  Hence only the first piece can leave a head
// record and only the last a tail record; every piece in between ends its sub-block and writes its own zero-padded last group.  The
// whole zero groups behind a short sub-block's last group (its extent is padded to 64 decisions) are nobody's piece: dc_p13_fill_tab_kernel.
// run_end: the run index behind the wavefront's last valid lane; sub_end(s): the run index behind sub-block s's last run.
// Returns false where the piece cannot be recorded (below): the caller voids the packed stream.
template <class P13Q, class SubEnd>
__device__ __forceinline__ bool dc_flush13(dc_lds_vu16* sg, const u32 wbase, const u32 lane, const u32 loc, const u32 nd, const u32 sb, const bool valid,
                                           const P13Q& Q, const u32 wave_global, const u32 run_end, SubEnd sub_end)
{
    bool ok = true;
    const u64 vmask = __ballot(valid);
    DcFrag head, tail; head.slot_count = 0; tail.slot_count = 0; head.gidx = 0; tail.gidx = 0;
#pragma unroll
    for (int x = 0; x < 8; ++x) { head.e[x] = 0; tail.e[x] = 0; }
    if (vmask != 0ull) {
        const u32 lastv = 63u - (u32)__builtin_clzll(vmask);
        const u32 sb_first = (u32)__builtin_amdgcn_readfirstlane((int)sb), sb_last = (u32)__builtin_amdgcn_readlane((int)sb, (int)lastv);
        for (u32 s2 = sb_first; s2 <= sb_last; ++s2) {                    // one trip, except where sub-blocks meet inside the wavefront
            const u64 mk = __ballot(valid && sb == s2);
            if (mk == 0ull) continue;
            const u32 l0 = (u32)__builtin_ctzll(mk), l1 = 63u - (u32)__builtin_clzll(mk);
            const u32 k0 = (u32)__builtin_amdgcn_readlane((int)loc, (int)l0), k1 = (u32)__builtin_amdgcn_readlane((int)(loc + nd), (int)l1);
            const u32 len = k1 - k0;
            if (len == 0u) continue;
            const u32 P0 = wbase + k0 + Q.pad[s2];
            const u32 g_full0 = (P0 + 7u) >> 3, g_full1 = (P0 + len) >> 3;         // groups [g_full0, g_full1) lie wholly inside
            for (u32 g = g_full0 + lane; g < g_full1; g += 64u) {
                const u32 k = k0 + (g * 8u - P0);
                u32 f[8];
#pragma unroll
                for (int x = 0; x < 8; ++x) f[x] = (u32)sg[k + (u32)x] & 0x1fffu;
                *reinterpret_cast<DcGroup13*>(Q.out + (size_t)g * 13u) = dc_pack13(f);
            }
            // the fragment before the first group boundary: only the wavefront's first piece can have one (a sub-block starts on a group)
            u32 hcount = 0;
            if ((P0 & 7u) != 0u) {
                hcount = 8u - (P0 & 7u); if (hcount > len) hcount = len;
                head.gidx = P0 >> 3; head.slot_count = (P0 & 7u) | (hcount << 8);
#pragma unroll
                for (int x = 0; x < 8; ++x) head.e[x] = (u32)x < hcount ? (u16)(sg[k0 + (u32)x] & 0x1fffu) : (u16)0;
                // A head-only piece: the whole piece lies inside one group and does not reach its end.  The join writes a group from ONE
                // tail and ONE head, so unless the sub-block ends here (the group's rest is padding) the next wavefront's head belongs to
                // the same group and two threads of the join would write it, each without the other's entries.  Not reachable while every
                // wavefront but a sub-block's last holds 64 runs of at least one decision each (8 < 64); kept so that it can never be silent.
                if (hcount == len && ((P0 + len) & 7u) != 0u && s2 == sb_last && run_end != sub_end(s2)) ok = false;
            }
            // the fragment behind the last one: the next wavefront completes it — unless the sub-block ends here, then it is a whole (padded) group
            if (((P0 + len) & 7u) != 0u && (g_full1 << 3) >= P0) {
                const u32 tcount = (P0 + len) & 7u, tk = k0 + ((g_full1 << 3) - P0);
                u32 f[8];
#pragma unroll
                for (int x = 0; x < 8; ++x) f[x] = (u32)x < tcount ? ((u32)sg[tk + (u32)x] & 0x1fffu) : 0u;
                if (s2 != sb_last) { if (lane == 0u) *reinterpret_cast<DcGroup13*>(Q.out + (size_t)g_full1 * 13u) = dc_pack13(f); }
                else {
                    tail.gidx = g_full1; tail.slot_count = tcount << 8;
#pragma unroll
                    for (int x = 0; x < 8; ++x) tail.e[x] = (u16)f[x];
                }
            }
        }
    }
    // both records (every lane holds the same two: they were read from LDS at wave-uniform addresses) as ONE 48-byte store: lane t writes word t
    if (lane < 12u) {
        const DcFrag& r = lane < 6u ? head : tail;
        const u32 q = lane < 6u ? lane : lane - 6u;
        const u32 w = q == 0u ? r.gidx : q == 1u ? r.slot_count
                    : q == 2u ? ((u32)r.e[0] | ((u32)r.e[1] << 16)) : q == 3u ? ((u32)r.e[2] | ((u32)r.e[3] << 16))
                    : q == 4u ? ((u32)r.e[4] | ((u32)r.e[5] << 16)) : ((u32)r.e[6] | ((u32)r.e[7] << 16));
        reinterpret_cast<u32*>(Q.frag + 2u * wave_global)[lane] = w;
    }
    return ok;
}
// thread w: the group between wavefront w and w + 1 (tail of w, head of w + 1), and a head nobody's tail belongs to (never on blocks whose
// wavefronts hold 64 runs; written for completeness)
__global__ __launch_bounds__(WG) void dc_p13_join_kernel(const DcFrag* __restrict__ frag, u32 nwaves, u8* __restrict__ out, const u32* __restrict__ meta)
{
    if (meta[DM_FAIL] != 0u) return;
    const u32 w = blockIdx.x * WG + threadIdx.x;
    if (w >= nwaves) return;
    const DcFrag T = frag[2u * w + 1u];
    DcFrag H; H.slot_count = 0; H.gidx = 0;
    if (w + 1u < nwaves) H = frag[2u * (w + 1u)];
    const u32 tc = T.slot_count >> 8, hc = H.slot_count >> 8, hs = H.slot_count & 0xffu;
    if (tc != 0u) {
        u32 f[8];
#pragma unroll
        for (int x = 0; x < 8; ++x) f[x] = (u32)x < tc ? (u32)T.e[x] : 0u;
        if (hc != 0u && H.gidx == T.gidx) {
#pragma unroll
            for (int x = 0; x < 8; ++x) if ((u32)x >= hs && (u32)x < hs + hc) f[x] = (u32)H.e[(u32)x - hs];
        }
        *reinterpret_cast<DcGroup13*>(out + (size_t)T.gidx * 13u) = dc_pack13(f);
    }
    if (hc != 0u && !(tc != 0u && H.gidx == T.gidx)) {
        u32 f[8];
#pragma unroll
        for (int x = 0; x < 8; ++x) f[x] = ((u32)x >= hs && (u32)x < hs + hc) ? (u32)H.e[(u32)x - hs] : 0u;
        *reinterpret_cast<DcGroup13*>(out + (size_t)H.gidx * 13u) = dc_pack13(f);
    }
}

// FAST: the fast coder's stream — one counter per decision (the char family's value IS the probability, 13 / 11 bits), entries
// {value, bit << 13, run start << 14, run side << 15} (devcoder_model.h PSF_*).
#ifndef DC_PS_MINW
#define DC_PS_MINW 1            // minimum waves per SIMD the register allocator must leave room for (A/B: 82 VGPRs = 5 waves by default)
#endif
template <bool FAST, bool P13, class SB>
__global__ __launch_bounds__(WG, DC_PS_MINW) void dc_pstream_kernel(DcGather G, SB S, const ModelParams* __restrict__ mp,
                                                        u32* __restrict__ meta, u16* __restrict__ out, u16* __restrict__ dbg /*[3][D] or null*/, u32 dbgD,
                                                        typename DcP13Of<SB>::T Q)
{
    typedef DcForm<SB> F;
    const u32 mrp = F::maxr_word(S);                                  // max_rank of the eight sub-blocks, one scalar word
    __shared__ u16 stage[WAVES][DC_PS_STAGE];
    __shared__ short s_lr[NUM_CLS][4];                                // blend weights per class: an LDS read per decision instead of global loads at a per-lane address
    if (meta[DM_FAIL] != 0u) return;
    if (!FAST) {
        if (threadIdx.x < (u32)NUM_CLS * 3u) s_lr[threadIdx.x / 3u][threadIdx.x % 3u] = mp->lr[threadIdx.x / 3u][threadIdx.x % 3u];
        __syncthreads();
    }
    const u32 j = dc_virtual_block() * WG + threadIdx.x;
    const u32 lane = threadIdx.x & 63u;
    const bool valid = j < G.m;                                       // (whole wavefronts past the end still take part in the shuffles below)
    const typename F::It it = F::unpack(valid ? G.key_ch[j] : 0ull);
    const int maxr = F::maxr(it, mrp);
    const int n_rank = valid ? count_rank_side(it, maxr) : 0, n_run = valid ? count_run_side(it) : 0, nd = n_rank + n_run;
    const u32 b_sp = valid ? G.doff_sp[j] : 0u;
    const u32 incl = wave_incl_sum((u32)nd);
    const u32 loc = incl - (u32)nd;                                   // this run's first entry inside the wavefront's piece of the stream
    const u32 wtotal = (u32)__builtin_amdgcn_readlane((int)incl, 63);
    const u32 wbase = (u32)__builtin_amdgcn_readfirstlane((int)b_sp);                  // lane 0 is valid whenever any lane is
    const bool staged = wtotal <= DC_PS_STAGE;                        // wave-uniform
    dc_lds_vu16* sg = (dc_lds_vu16*)&stage[threadIdx.x >> 6][0];
    const u32* p_sp = G.pos_sp + b_sp;
    const u32* p_ch = G.pos_ch + (valid ? G.doff_ch[G.inv_ch[j]] : 0u);
    const u32* p_sr = FAST ? G.pos_ch : G.pos_sr + (valid ? G.doff_sr[G.inv_sr[j]] : 0u);
    const u32* p_sn = FAST ? G.pos_ch : G.pos_sn + (valid ? G.doff_sn[G.inv_sn[j]] : 0u);
    u16* o = out + b_sp;
    auto emit = [&](int k, u32 q_sp, u32 q_ch, u32 q_st, bool run_side, int cls, u32 bit) {
        const int v_ch = G.V_ch[q_ch];
        u16 e;
        if (FAST) {
            e = (u16)((u32)v_ch | (bit << 13) | (k == 0 ? (u32)PSF_RUN : 0u) | (run_side ? (u32)PSF_SIDE : 0u));
        } else {
            const int v_sp = G.V_sp[q_sp];
            const int v_st = run_side ? G.V_sn[q_st] : G.V_sr[q_st];
            const int p = blend(v_ch, v_st, v_sp, s_lr[cls]);
            e = (u16)((u32)p | (bit << 12) | (k == 0 ? (u32)PS_RUN : 0u));
            if (dbg) { dbg[b_sp + k] = (u16)v_st; dbg[(size_t)dbgD + b_sp + k] = (u16)v_ch; dbg[2 * (size_t)dbgD + b_sp + k] = (u16)v_sp; }
        }
        if (staged) sg[loc + (u32)k] = e; else if (!P13) o[k] = e;
    };
    // first 8 decisions: positions by wide loads (the arrays have slack behind their last entry), static register indices
    u32 qsp[8], qch[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) { qsp[k] = 0; qch[k] = 0; }
    if (valid) {
        const DcU4 c0 = *reinterpret_cast<const DcU4*>(p_ch), c1 = *reinterpret_cast<const DcU4*>(p_ch + 4);
        qch[0] = c0.a; qch[1] = c0.b; qch[2] = c0.c; qch[3] = c0.d; qch[4] = c1.a; qch[5] = c1.b; qch[6] = c1.c; qch[7] = c1.d;
        if (!FAST) {
            const DcU4 a0 = *reinterpret_cast<const DcU4*>(p_sp), a1 = *reinterpret_cast<const DcU4*>(p_sp + 4);
            qsp[0] = a0.a; qsp[1] = a0.b; qsp[2] = a0.c; qsp[3] = a0.d; qsp[4] = a1.a; qsp[5] = a1.b; qsp[6] = a1.c; qsp[7] = a1.d;
        }
    }
    // the state family's positions: the first eight of each side by two wide loads each (was: one 4-byte load per decision); which of the
    // sixteen a decision takes is a select chain on (side, index inside the side)
    u32 sr8[8], sn8[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) { sr8[k] = 0; sn8[k] = 0; }
    if (!FAST && valid) {
        const DcU4 r0 = *reinterpret_cast<const DcU4*>(p_sr), r1 = *reinterpret_cast<const DcU4*>(p_sr + 4);
        const DcU4 n0 = *reinterpret_cast<const DcU4*>(p_sn), n1 = *reinterpret_cast<const DcU4*>(p_sn + 4);
        sr8[0] = r0.a; sr8[1] = r0.b; sr8[2] = r0.c; sr8[3] = r0.d; sr8[4] = r1.a; sr8[5] = r1.b; sr8[6] = r1.c; sr8[7] = r1.d;
        sn8[0] = n0.a; sn8[1] = n0.b; sn8[2] = n0.c; sn8[3] = n0.d; sn8[4] = n1.a; sn8[5] = n1.b; sn8[6] = n1.c; sn8[7] = n1.d;
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        if (k < nd) {
            u32 bit; bool rs;
            const int cls = nth_class(it, maxr, n_rank, k, &bit, &rs);
            u32 q_st = 0;
            if (!FAST) {
                // rank side: index k (static); run side: k - n_rank in 0 .. k
                u32 qn = sn8[0];
#pragma unroll
                for (int j = 1; j <= k; ++j) qn = (k - n_rank == j) ? sn8[j] : qn;
                q_st = rs ? qn : sr8[k];
            }
            emit(k, qsp[k], qch[k], q_st, rs, cls, bit);
        }
    }
    for (int k = 8; k < nd; ++k) {
        u32 bit; bool rs;
        const int cls = nth_class(it, maxr, n_rank, k, &bit, &rs);
        emit(k, FAST ? 0u : p_sp[k], p_ch[k], FAST ? 0u : (rs ? p_sn[k - n_rank] : p_sr[k]), rs, cls, bit);
    }
    if (P13) {
        // (a piece that does not fit the staging buffer voids the packed stream: the host launches the 2-byte form for this block)
        if (!staged) { if (lane == 0u) atomicOr(&meta[DM_P13_OVER], 1u); }
        __builtin_amdgcn_wave_barrier();
        if (staged) {
            const u32 j0 = j - lane, run_end = j0 + 64u < G.m ? j0 + 64u : G.m;
            const bool ok = dc_flush13(sg, wbase, lane, loc, (u32)nd, (u32)it.sb, valid, Q, j >> 6, run_end,
                                       [&](u32 s2) { const u32 nf = F::next_first(S, s2); return nf == 0xffffffffu ? G.m : nf; });
            if (!ok && lane == 0u) atomicOr(&meta[DM_P13_OVER], 1u);
        }
        else if (lane < 12u) reinterpret_cast<u32*>(Q.frag + 2u * (j >> 6))[lane] = 0u;
    } else if (staged) {
        // the wavefront's piece [wbase, wbase + wtotal) of the stream: 4-byte stores from the first even entry on, the odd ends singly
        __builtin_amdgcn_wave_barrier();
        u16* ow = out + wbase;
        const u32 head = wbase & 1u;                                  // 1: the piece starts on an odd entry
        if (head && lane == 0 && wtotal > 0) ow[0] = sg[0];
        const u32 body = (wtotal - (head < wtotal ? head : wtotal)) >> 1;     // whole 4-byte words after the head
        u32* ow32 = reinterpret_cast<u32*>(ow + head);
        for (u32 t = lane; t < body; t += 64) ow32[t] = (u32)sg[head + 2 * t] | ((u32)sg[head + 2 * t + 1] << 16);
        if (lane == 0 && wtotal > head && ((wtotal - head) & 1u)) ow[wtotal - 1] = sg[wtotal - 1];
    }
}

__global__ void dc_poff_kernel(const u32* __restrict__ doff_sp, DcSub S, u32 m, u32* __restrict__ poff)
{
    const u32 b = threadIdx.x;
    if (b <= S.nb) poff[b] = doff_sp[b < S.nb ? S.first[b] : m];
}
// ... of a batched pass: every sub-block of the table (run[nsub] = m, doff_sp[m] = the pass's decisions)
__global__ __launch_bounds__(WG) void dc_poff_tab_kernel(const u32* __restrict__ doff_sp, DcSubTab S, u32* __restrict__ poff)
{
    const u32 b = blockIdx.x * WG + threadIdx.x;
    if (b <= S.nsub) poff[b] = doff_sp[S.run[b]];
}
// ... and, for the packed stream of a pass (DcP13Tab), where every sub-block starts in the packed space: pbase[0] = 0, pbase[s + 1] =
// pbase[s] + (poff[s + 1] - poff[s] rounded up to 64), pad[s] = pbase[s] - poff[s].  One workgroup scans the at most FRONT_MAX_SUB + 1
// entries (a stretch per thread, the stretches' sums through LDS); behind dc_poff_tab_kernel on the stream, no host round trip.
__global__ __launch_bounds__(WG) void dc_pbase_tab_kernel(const u32* __restrict__ poff, u32 nsub, u32* __restrict__ pad, u32* __restrict__ pbase)
{
    __shared__ u32 s_sum[WG];
    const u32 t = threadIdx.x, per = (nsub + WG - 1) / WG;
    const u32 s0 = t * per, s1 = s0 + per < nsub ? s0 + per : nsub;
    u32 sum = 0;
    for (u32 s = s0; s < s1; ++s) sum += (poff[s + 1] - poff[s] + 63u) & ~63u;
    s_sum[t] = sum;
    __syncthreads();
    for (u32 d = 1; d < (u32)WG; d <<= 1) {
        const u32 v = t >= d ? s_sum[t - d] : 0u;
        __syncthreads();
        s_sum[t] += v;
        __syncthreads();
    }
    u32 base = s_sum[t] - sum;
    for (u32 s = s0; s < s1; ++s) { pbase[s] = base; pad[s] = base - poff[s]; base += (poff[s + 1] - poff[s] + 63u) & ~63u; }
    if (t == (u32)WG - 1u) pbase[nsub] = s_sum[t];
}
// The whole zero groups of a pass's packed stream: behind sub-block s's last (padded) group, up to its extent's end at pbase[s + 1] — at
// most seven groups, where the sub-block's decisions leave 57 .. 63 modulo 64 or fewer than 8 of them are there at all.  Thread per
// sub-block; with the stream kernel and the join every byte of [0, pbase[nsub] / 8 * 13) is written, the buffer is not cleared first.
__global__ __launch_bounds__(WG) void dc_p13_fill_tab_kernel(const u32* __restrict__ poff, const u32* __restrict__ pbase, u32 nsub, u8* __restrict__ out,
                                                             const u32* __restrict__ meta)
{
    if (meta[DM_FAIL] != 0u) return;
    const u32 s = blockIdx.x * WG + threadIdx.x;
    if (s >= nsub) return;
    const u32 g0 = (pbase[s] + (poff[s + 1] - poff[s]) + 7u) >> 3, g1 = pbase[s + 1] >> 3;
    DcGroup13 z; z.a = 0; z.b = 0; z.c = 0; z.d = 0;
    for (u32 g = g0; g < g1; ++g) *reinterpret_cast<DcGroup13*>(out + (size_t)g * 13u) = z;
}
// max_rank of every sub-block of a pass from its first-run table: bsr(nsym - 1), nsym = symbols with a first run.  One wavefront per
// sub-block.  Also closes the run table: run[nsub] = m.  fixed >= 0: that value for every sub-block instead (the fast coder closes
// the exponent below 7 bits whatever the alphabet: qlfc.cpp:1204).
__global__ __launch_bounds__(WG) void dc_tab_prep_kernel(const u32* __restrict__ first_run /*[nsub][256]*/, u32 nsub, u32 m, int fixed,
                                                         u8* __restrict__ maxr, u32* __restrict__ sub_run)
{
    const u32 s = blockIdx.x * WAVES + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (blockIdx.x == 0 && threadIdx.x == 0) sub_run[nsub] = m;
    if (s >= nsub) return;
    if (fixed >= 0) { if (lane == 0u) maxr[s] = (u8)fixed; return; }
    const uint4 q = reinterpret_cast<const uint4*>(first_run + (size_t)s * 256u)[lane];
    u32 cnt = (q.x != 0xffffffffu) + (q.y != 0xffffffffu) + (q.z != 0xffffffffu) + (q.w != 0xffffffffu);
    cnt = wave_incl_sum(cnt);
    if (lane == 63u) maxr[s] = (u8)bsr(cnt - 1u);
}

// ---- model segments: what the plan needs of every sub-block, before any sort or partition -------------------------------------
// Decisions of every sub-block of a pass for the coder at hand (maxr: the table's, 7 for the fast coder; ge32: the flags, zero for the
// fast coder): a run's count is the case analysis the partition walks (count_rank_side / count_run_side of the item the items kernel
// would pack).  Thread per run.  Runs are in stream order, so the sub-block id is non-decreasing across a wavefront: one inclusive scan
// of the counts, and the last lane of every sub-block's stretch adds (its prefix - the prefix in front of the stretch's first lane).
__global__ __launch_bounds__(WG) void dc_sub_dec_kernel(const u8* __restrict__ sym, const u8* __restrict__ rank, const u32* __restrict__ start,
                                                        const u8* __restrict__ ge32, u32 m, DcSubTab S, u32* __restrict__ sub_dec)
{
    typedef DcForm<DcSubTab> F;
    const u32 j = blockIdx.x * WG + threadIdx.x, lane = threadIdx.x & 63u;
    u32 nd = 0, sb = 0xffffffffu;                                     // (lanes past the end: a stretch of their own that adds nothing)
    if (j < m) {
        const ItemB it = F::unpack(F::item(S, sym, rank, start, ge32, j, m, 0u));
        sb = it.sb;
        nd = (u32)(count_rank_side(it, (int)it.maxr) + count_run_side(it));
    }
    const u32 incl = wave_incl_sum(nd);
    const u32 prev_sb = (u32)__shfl_up((int)sb, 1, 64);
    const u64 heads = __ballot(lane == 0u || prev_sb != sb);          // first lane of every stretch
    const bool tail = lane == 63u || ((heads >> (lane + 1u)) & 1ull) != 0ull;
    const u64 upto = heads & (~0ull >> (63u - lane));                 // heads at or below this lane: never empty (lane 0 is one)
    const u32 first = 63u - (u32)__builtin_clzll(upto);
    const u32 before = (u32)__shfl((int)(incl - nd), (int)first, 64); // the scan in front of the stretch
    if (tail && j < m && incl != before) atomicAdd(&sub_dec[sb], incl - before);
}
// ... of a single block (a block in sub-block segments, dc_block_facts): the eight-entry twin — Item, run lengths up to 2^31 (n: the
// block's bytes, the end of its last run), max_rank from the packed word.  A block has tens of millions of runs and eight counters: one
// atomic per wavefront of 64 runs (the table's way, where thousands of sub-blocks share them) would queue half a million atomics on
// eight addresses — 5 ms for the bench block.  So a wavefront walks tiles of 64 runs at the grid's stride and keeps the counts in
// registers, lane b the one of sub-block b (the sum of every stretch is handed to its lane: one or two stretches a tile), and adds them
// at the end: at most eight atomics per wavefront, a few thousand a block.
constexpr u32 DC_SUB_DEC8_GRID = 2048;
__global__ __launch_bounds__(WG) void dc_sub_dec8_kernel(const u8* __restrict__ sym, const u8* __restrict__ rank, const u32* __restrict__ start,
                                                         const u8* __restrict__ ge32, u32 m, u32 n, DcSub S, u32* __restrict__ sub_dec /*[8]*/)
{
    typedef DcForm<DcSub> F;
    const u32 maxr_w = F::maxr_word(S);
    const u32 lane = threadIdx.x & 63u;
    const u32 wave = blockIdx.x * WAVES + (threadIdx.x >> 6), nwaves = gridDim.x * WAVES;
    const u32 tiles = (m + 63u) / 64u;
    u32 acc = 0;                                                      // lane b < 8: decisions of sub-block b in this wavefront's tiles
    for (u32 t = wave; t < tiles; t += nwaves) {
        const u32 j = t * 64u + lane;
        u32 nd = 0, sb = 8u;                                          // (lanes past the end: a stretch of their own that no lane owns)
        if (j < m) {
            const Item it = F::unpack(F::item(S, sym, rank, start, ge32, j, m, n));
            sb = it.sb;
            nd = (u32)(count_rank_side(it, F::maxr(it, maxr_w)) + count_run_side(it));
        }
        const u32 incl = wave_incl_sum(nd);
        const u32 prev_sb = (u32)__shfl_up((int)sb, 1, 64);
        // runs are in stream order, so the sub-block id does not decrease across the tile: at most nine stretches, one loop trip each
        for (u64 h = __ballot(lane == 0u || prev_sb != sb); h != 0ull; h &= h - 1ull) {
            const u32 first = (u32)__builtin_ctzll(h);
            const u64 rest = h & (h - 1ull);
            const u32 last = rest ? (u32)__builtin_ctzll(rest) - 1u : 63u;
            const u32 before = first ? (u32)__shfl((int)incl, (int)first - 1, 64) : 0u;
            const u32 sum = (u32)__shfl((int)incl, (int)last, 64) - before;
            const u32 owner = (u32)__shfl((int)sb, (int)first, 64);
            if (lane == owner) acc += sum;
        }
    }
    if (lane < 8u && acc != 0u) atomicAdd(&sub_dec[lane], acc);
}
// The rebased run table of the segment [s0, s0 + nsub_seg) whose runs are [r0, r1): to every kernel instantiated for a table the
// segment then is a small pass of its own (sub_off / sub_base / maxr enter offset by s0, the run arrays and flags offset by r0).
__global__ __launch_bounds__(WG) void dc_seg_tab_kernel(const u32* __restrict__ sub_run, u32 s0, u32 nsub_seg, u32 r0, u32 r1, u32* __restrict__ seg_run)
{
    const u32 i = blockIdx.x * WG + threadIdx.x;
    if (i < nsub_seg) seg_run[i] = sub_run[s0 + i] - r0;
    else if (i == nsub_seg) seg_run[i] = r1 - r0;
}

// ---------------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------------
// Row -> bin ranges of the counting pass, derived from the model's own case analysis (the one dc_item_rounds walks): for every
// bin the rows a run of that bin contributes to, then per row the (at most two) ranges of consecutive bins.  Returns false if a
// row ever needed more — the layout of the bins would be wrong, and the device coder is then not offered at all.
static bool dc_build_rowbins(DcRowBins* T)
{
    static unsigned char member[DC_ROWS][DC_BINS];
    memset(member, 0, sizeof member);
    for (int lt = 0; lt < 2; ++lt) {
        for (u32 rank = 0; rank < 256; ++rank) {
            const int B = rank != 1u ? bsr(rank) : 0;
            if (lt && B == 0) continue;                                         // dc_rank_bin never produces these
            const u32 bin = rank | (lt ? 256u : 0u);
            const int e = B ? (B - 1) + lt : 0;
            member[TAU_RF][bin] = 1;
            for (int sx = 0; sx < e && sx < 7; ++sx) member[TAU_RE + sx][bin] = 1;
            for (int d = 0; d < B; ++d) member[TAU_RM + rm_off(B) + (int)(rank >> (B - d)) - 1][bin] = 1;
        }
    }
    for (u32 cls = 1; cls < 96; ++cls) {
        if (cls >= 64 && (cls < 70 || cls > 94)) continue;                      // run lengths below 64 have their own bin; 2^31 > run
        const u32 run = cls < 64 ? cls : 1u << (cls - 64);
        const u32 bin = dc_run_bin(run);
        if (bin != DC_BIN_RUN + cls) return false;
        const int nb = run != 1u ? bsr(run) : 0;
        member[TAU_NF][bin] = 1;
        for (int sx = 0; sx < nb; ++sx) member[TAU_NE + sx][bin] = 1;
        for (int d = 0; d < nb; ++d) member[TAU_NM + nm_off(nb) + (int)(nb <= 5 ? (run >> (nb - d)) : (u32)(1 + d)) - 1][bin] = 1;
    }
    for (int h = 0; h < DC_ROWS; ++h) {
        u16 r[4] = {0, 0, 0, 0}; int nr = 0;
        for (int b = 0; b < DC_BINS;) {
            if (!member[h][b]) { ++b; continue; }
            int e = b; while (e < DC_BINS && member[h][e]) ++e;
            if (nr == 2) return false;
            r[2 * nr] = (u16)b; r[2 * nr + 1] = (u16)e; ++nr;
            b = e;
        }
        T[h].lo1 = r[0]; T[h].hi1 = r[1]; T[h].lo2 = r[2]; T[h].hi2 = r[3];
    }
    return true;
}

static size_t dc_align(size_t x) { return (x + 255) / 256 * 256; }

// The arena's one allocation, and the pointers of the carve table into it.  false: it does not fit — or fail_env (may be null) is set
// in the environment, the tests' way to that exit —; the HIP error is cleared and the arena marked, so that nobody allocates again.
struct Carve { void** p; size_t bytes; };
template <size_t N>
static bool dc_arena_alloc(DcArena& a, const Carve (&carve)[N], const char* fail_env)
{
    size_t total = 0;
    for (const Carve& cv : carve) total += dc_align(cv.bytes);
    if ((fail_env && getenv(fail_env)) || hipMalloc((void**)&a.base, total) != hipSuccess) {
        (void)hipGetLastError(); a.base = nullptr; a.failed = true;
        return false;
    }
    a.bytes = total;
    size_t off = 0;
    for (const Carve& cv : carve) { *cv.p = a.base + off; off += dc_align(cv.bytes); }
    return true;
}

// Everything a DevCoder owns, whether it is the context's or one whose set-up did not get that far.
static void dc_free(DevCoder* d)
{
    for (DcArena* a : {&d->arena, &d->batch_arena, &d->avg_arena, &d->rp_arena, &d->hist_arena, &d->blk_arena, &d->mix_arena}) if (a->base) (void)hipFree(a->base);
    for (int k = 0; k < 2; ++k) if (d->seg_ev[k]) (void)hipEventDestroy(d->seg_ev[k]);
    if (d->hmeta) (void)hipHostFree(d->hmeta);
    delete d;
}
void devcoder_destroy(bscgpu_ctx* c)
{
    if (c->dc) dc_free(c->dc);
    c->dc = nullptr;
}


// The two parameter sets with their attainable-value closures: function-local statics, so whoever comes first computes them and
// everybody else waits for that.
static const ModelParams& dc_model_static()
{
    static const ModelParams mp = [] { ModelParams m; model_params_from_table(bschost::qlfc_static_params(), m); return m; }();
    return mp;
}
static const ModelParams& dc_model_fast()
{
    static const ModelParams mpf = [] { ModelParams m; model_params_fast(m); return m; }();
    return mpf;
}
// Called at the top of the process's first bscgpu_create: the ~60 ms of closure computation run beside the ~190 ms the HIP runtime
// takes to come up, instead of in front of the first block (a file of a few dozen blocks is done in about a second: bsc_mgpu, the CLI).
void devcoder_warm_tables()
{
    struct Warm {
        std::thread th;
        Warm() { try { th = std::thread([] { (void)dc_model_static(); (void)dc_model_fast(); }); } catch (const std::system_error&) {} }
        ~Warm() { if (th.joinable()) th.join(); }
    };
    static Warm warm;
}

// the arena's capacity: runs (bytes of max_n, padded) and decisions (four per byte of that)
static size_t dc_capacity_runs(int64_t max_n) { return ((size_t)max_n + 4096 + 4095) / 4096 * 4096; }
static size_t dc_capacity_decisions(int64_t max_n) { return 4 * dc_capacity_runs(max_n) + 65536; }
// ... of ceil(max_n / k) for the context's arena divisor k (BSCGPU_OPT_DC_ARENA_DIV; 1: max_n itself)
static int64_t dc_capacity_n(const bscgpu_ctx* c) { return (c->max_n + c->dc_arena_div - 1) / c->dc_arena_div; }
int64_t devcoder_dcap(const bscgpu_ctx* c) { return (int64_t)dc_capacity_decisions(dc_capacity_n(c)); }
int64_t devcoder_mcap(const bscgpu_ctx* c) { return (int64_t)dc_capacity_runs(dc_capacity_n(c)); }
// The divisor can change only while no arena was carved by another one.
int devcoder_arena_div_set(bscgpu_ctx* c, int value)
{
    if (value != 1 && value != 2 && value != 4 && value != 8) return BSC_BAD_PARAMETER;
    if (c->dc && value != c->dc_arena_div) return BSC_NOT_SUPPORTED;
    const int old = c->dc_arena_div;
    c->dc_arena_div = value;
    return old;
}

int devcoder_ensure(bscgpu_ctx* c)
{
    if (c->dc) return BSC_NO_ERROR;
    // An arena that does not fit (~220 bytes per block byte on top of the sorter's ~60) is a reason to DECLINE, not an error: the
    // block takes the host model, as it did before the device model existed, and the allocation is not retried for every block.
    if (c->dc_alloc_failed) return BSC_NOT_SUPPORTED;
    CtxTimer tm("devcoder_ensure (arena, tables)");
    DevCoder* d = new DevCoder();
    // (BSCGPU_OPT_DC_ARENA_DIV: the capacity of 1 / k of max_n; a block above it is modelled in sub-block segments.  ge32 alone keeps a
    // byte per run of the whole block: the facts the plan is made of are taken over all of it, once — k = 1: G == M, the carve as ever)
    const int64_t cap_n = dc_capacity_n(c);
    d->Mcap = dc_capacity_runs(cap_n); d->Dcap = dc_capacity_decisions(cap_n);
    const size_t M = d->Mcap + 64, D = d->Dcap + 64, NCH = d->Dcap / DC_EV + 16, G = dc_capacity_runs(c->max_n) + 64;
    d->Gcap = G - 64;
    const Carve carve[] = {
        {(void**)&d->key_ch, 8 * M}, {(void**)&d->key_ch_s, 8 * M}, {(void**)&d->key_sr, 8 * M}, {(void**)&d->key_sr_s, 8 * M},
        {(void**)&d->key_sn, 8 * M}, {(void**)&d->key_sn_s, 8 * M},
        {(void**)&d->inv_ch, 4 * M}, {(void**)&d->inv_sr, 4 * M}, {(void**)&d->inv_sn, 4 * M}, {(void**)&d->ge32, G},
        {(void**)&d->doff[0], 4 * M}, {(void**)&d->doff[1], 4 * M}, {(void**)&d->doff[2], 4 * M}, {(void**)&d->doff[3], 4 * M},
        {(void**)&d->events[0], 2 * D}, {(void**)&d->events[1], 2 * D}, {(void**)&d->events[2], 2 * D}, {(void**)&d->events[3], 2 * D},
        {(void**)&d->pos[0], 4 * D}, {(void**)&d->pos[1], 4 * D}, {(void**)&d->pos[2], 4 * D}, {(void**)&d->pos[3], 4 * D},
        {(void**)&d->V[0], 2 * D}, {(void**)&d->V[1], 2 * D}, {(void**)&d->V[2], 2 * D}, {(void**)&d->V[3], 2 * D},
        {(void**)&d->ps[0], 2 * D}, {(void**)&d->ps[1], 2 * D},
        {(void**)&d->cnt, (size_t)DC_ROWS * DC_WCH_MAX * 4}, {(void**)&d->rowtot, DC_ROWS * 4}, {(void**)&d->rowstart, 6 * (DC_ROWS + 8) * 4},
        {(void**)&d->wdec, (DC_WCH_MAX + 8) * 4}, {(void**)&d->wdecoff, (DC_WCH_MAX + 8) * 4},
        {(void**)&d->elo, 2 * 4 * NCH}, {(void**)&d->ehi, 2 * 4 * NCH}, {(void**)&d->S, 2 * 4 * NCH},
        {(void**)&d->present, (size_t)DC_KIND_WORDS * 4}, {(void**)&d->rounds, 256},
        {(void**)&d->meta, DM_COUNT * 4}, {(void**)&d->poff, 16 * 4}, {(void**)&d->frag, (M / 64 + 64) * 2 * sizeof(DcFrag)},
        {(void**)&d->tab_rank, 32768}, {(void**)&d->tab_run, 8192}, {(void**)&d->mp, sizeof(ModelParams)}, {(void**)&d->mp_fast, sizeof(ModelParams)},
        {(void**)&d->rowbins, DC_ROWS * sizeof(DcRowBins)}, {(void**)&d->sink, 4096},
    };
    d->nch_cap = NCH;
    if (!dc_arena_alloc(d->arena, carve, "BSC_DEVCODER_FAIL_ALLOC") || hipHostMalloc((void**)&d->hmeta, HM_WORDS * 4, hipHostMallocDefault) != hipSuccess) {
        (void)hipGetLastError(); d->hmeta = nullptr; dc_free(d);
        c->dc_alloc_failed = true;                                       // the policy above: the context keeps the host model
        return BSC_NOT_SUPPORTED;
    }
    // (once per process: the attainable-range closures behind the brackets take ~60 ms to compute, and every context needs the same tables;
    // devcoder_warm_tables starts them on a thread of their own while the first context is still being created)
    const ModelParams& mp = dc_model_static();
    const ModelParams& mpf = dc_model_fast();
    // more than 64 KB of dynamic LDS is a per-device attribute of the function: set for every context's device
    if (hipFuncSetAttribute((const void*)dc_eval_wave_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, DC_EVAL_LDS) != hipSuccess ||
        hipFuncSetAttribute((const void*)dc_eval_wave_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, DC_EVAL_LDS) != hipSuccess) {
        dc_free(d);
        return ctx_fail(c, BSC_GPU_ERROR, "device coder: LDS attribute", hipSuccess);
    }
    static DcRowBins rowbins[DC_ROWS];
    static const bool rowbins_ok = dc_build_rowbins(rowbins);
    if (!rowbins_ok) { dc_free(d); return ctx_fail(c, BSC_GPU_ERROR, "device coder: bin layout", hipSuccess); }
    const bschost::QlfcTables& QT = bschost::qlfc_tables();
    const uint8_t *rs = QT.rank_state, *ns = QT.run_state;
    const bool ok = hipMemcpyAsync(d->mp, &mp, sizeof mp, hipMemcpyHostToDevice, c->stream) == hipSuccess
                 && hipMemcpyAsync(d->mp_fast, &mpf, sizeof mpf, hipMemcpyHostToDevice, c->stream) == hipSuccess
                 && hipMemcpyAsync(d->tab_rank, rs, 32768, hipMemcpyHostToDevice, c->stream) == hipSuccess
                 && hipMemcpyAsync(d->tab_run, ns, 8192, hipMemcpyHostToDevice, c->stream) == hipSuccess
                 && hipMemcpyAsync(d->rowbins, rowbins, sizeof rowbins, hipMemcpyHostToDevice, c->stream) == hipSuccess
                 && ctx_sync(c) == hipSuccess;                      // mp is a stack object: the copies must have finished
    if (!ok) { dc_free(d); return ctx_fail(c, BSC_GPU_ERROR, "device coder tables", hipSuccess); }
    c->dc = d;
    return BSC_NO_ERROR;
}

int64_t devcoder_arena_bytes(const bscgpu_ctx* c) { return c->dc ? (int64_t)c->dc->arena.bytes : 0; }
int64_t devcoder_batch_bytes(const bscgpu_ctx* c) { return c->dc ? (int64_t)(c->dc->batch_arena.bytes + c->dc->avg_arena.bytes + c->dc->rp_arena.bytes + c->dc->hist_arena.bytes + c->dc->blk_arena.bytes + c->dc->mix_arena.bytes) : 0; }

// One partition job: counts, scans, scatter.  SCATTER = false: counts and scans only, then the runs' offsets in the stream
// (dc_doff_kernel) — all the fast coder needs of job 0, whose events nobody reads.
template <int SIDES, bool SCATTER = true, class SB>
static void dc_launch_partition(bscgpu_ctx* c, DevCoder* d, const u64* items, u32 m, const SB& S, int job, u32 ignoreX)
{
    const DcGeom g = dc_geom(m);
    const u32 grid = (g.W + WAVES - 1) / WAVES;
    u32* rowstart = d->rowstart + (DC_ROWS + 8) * job;
    prof_begin(c, BSCGPU_K_DC_PART, (u64)m * 8, m);
    hipLaunchKernelGGL((dc_part_count_kernel<SIDES, SB>), dim3(grid), dim3(WG), 0, c->stream, items, g, S, d->rowbins, d->cnt, d->wdec);
    hipLaunchKernelGGL(dc_scan_rows_kernel, dim3(DC_ROWS), dim3(WG), 0, c->stream, d->cnt, g.W, d->rowtot);
    hipLaunchKernelGGL(dc_scan_misc_kernel, dim3(1), dim3(WG), 0, c->stream, d->rowtot, rowstart, d->wdec, g.W, d->wdecoff, d->meta, job, (u32)d->Dcap);
    if constexpr (SCATTER)
        hipLaunchKernelGGL((dc_part_scatter_kernel<SIDES, SB>), dim3(grid), dim3(WG), 0, c->stream, items, g, S, d->meta, d->cnt, rowstart,
                           d->wdecoff, ignoreX, d->events[job], d->pos[job], d->doff[job], d->esub[job]);
    else
        hipLaunchKernelGGL((dc_doff_kernel<SIDES, SB>), dim3(grid), dim3(WG), 0, c->stream, items, g, S, d->meta, d->wdecoff, d->doff[job]);
    prof_end(c);
}

// what bscgpu_option_get reports about the context's last block, from the meta words just read back (declined or not)
static DcNote dc_note_from(const u32* hmeta)
{
    return DcNote{(int)hmeta[DM_FAIL], (int)hmeta[DM_REPLAYS], (int)hmeta[DM_AVG_UND], (int)hmeta[DM_AVG_RESOLVED], (int)hmeta[DM_REPLAY_RESOLVED],
                  (int)hmeta[DM_HIST_EXT], (int)hmeta[DM_HIST_RESOLVED]};
}

// ---- the avg_rank flags of m runs (1a), and with BSCGPU_OPT_DC_AVG_EXACT the exact resolve behind them (1a') ---------------------------
// The resolve's buffers, on the first call that asks for it; false: they do not fit.
static bool devcoder_avg_ensure(DevCoder* d)
{
    if (d->avg_arena.base || d->avg_arena.failed) return !d->avg_arena.failed;
    // chunks padded to whole groups, groups to the 64 that dc_avg_groups_kernel loads at a time (of Gcap: the facts of a block in
    // sub-block segments walk the flags of the whole block, whatever the arena's divisor; Gcap == Mcap without one)
    const size_t NC = (d->Gcap / DC_AVG_CH + 1 + DC_AVG_GROUP) / DC_AVG_GROUP * DC_AVG_GROUP + DC_AVG_GROUP, NG = (NC / DC_AVG_GROUP + 64) / 64 * 64 + 64;
    const Carve carve[] = {
        {(void**)&d->avg.brk, 2 * NC}, {(void**)&d->avg.und, 2 * NC}, {(void**)&d->avg.st, NC}, {(void**)&d->avg.ex, 2 * NC},
        {(void**)&d->avg.map, (size_t)DC_AVG_CAND * NC}, {(void**)&d->avg.gmap, 2 * (size_t)DC_AVG_CAND * NG}, {(void**)&d->avg.gstart, 2 * NG},
    };
    return dc_arena_alloc(d->avg_arena, carve, "BSC_DC_AVG_FAIL_ALLOC");
}
// No sync: the resolve's kernels are launched whether or not a flag is open, and leave at once where none is.
template <class SB>
static int dc_launch_avg(bscgpu_ctx* c, DevCoder* d, const u8* drank, u32 m, const SB& S, u32* sub_und)
{
    const u32 nch = (m + DC_AVG_CH - 1) / DC_AVG_CH, ngr = (nch + DC_AVG_GROUP - 1) / DC_AVG_GROUP;
    if (!c->dc_avg_exact) {
        hipLaunchKernelGGL(dc_avg_kernel<SB>, dim3((nch + WG - 1) / WG), dim3(WG), 0, c->stream, drank, m, S, d->ge32, d->meta, sub_und, DcAvgNoRec{});
        return BSC_NO_ERROR;
    }
    if (!devcoder_avg_ensure(d)) return BSC_NOT_SUPPORTED;             // do not fit: the unit is declined, as for the batch arena (no reason bit)
    hipLaunchKernelGGL((dc_avg_kernel<SB, true>), dim3((nch + WG - 1) / WG), dim3(WG), 0, c->stream, drank, m, S, d->ge32, d->meta, (u32*)nullptr, d->avg);
    if (nch > 1) hipLaunchKernelGGL(dc_avg_map_kernel<SB>, dim3((nch - 1 + WAVES - 1) / WAVES), dim3(WG), 0, c->stream, drank, m, S, d->avg);
    if (ngr > 1) hipLaunchKernelGGL(dc_avg_chain_kernel<false>, dim3(ngr - 1), dim3(64), 0, c->stream, m, d->avg);
    hipLaunchKernelGGL(dc_avg_groups_kernel<>, dim3(1), dim3(64), 0, c->stream, m, d->avg);
    hipLaunchKernelGGL(dc_avg_chain_kernel<true>, dim3(ngr), dim3(64), 0, c->stream, m, d->avg);
    hipLaunchKernelGGL(dc_avg_fix_kernel<SB>, dim3((nch + WAVES - 1) / WAVES), dim3(WG), 0, c->stream, drank, m, S, d->ge32, d->meta, sub_und, d->avg);
    return BSC_NO_ERROR;
}

// ---- the exact resolve of open run_hist brackets (1c') ---------------------------------------------------------------------------------
// Its buffers, on the first static model that asks for it; false: they do not fit.
static bool devcoder_hist_ensure(DevCoder* d)
{
    if (d->hist_arena.base || d->hist_arena.failed) return !d->hist_arena.failed;
    // chunks padded to whole groups, groups to the 64 that dc_avg_groups_kernel loads at a time; a bit per element of the padded chunks
    const size_t NC = (d->Mcap / DC_HIST_CH + 1 + DC_HIST_GROUP) / DC_HIST_GROUP * DC_HIST_GROUP + DC_HIST_GROUP, NG = (NC / DC_HIST_GROUP + 64) / 64 * 64 + 64;
    const Carve carve[] = {
        {(void**)&d->hist.bits, NC * DC_HIST_CH / 8}, {(void**)&d->hist.flag, NC}, {(void**)&d->hist.ex, 2 * NC},
        {(void**)&d->hist.map, (size_t)DC_HIST_CAND * NC}, {(void**)&d->hist.gmap, 2 * (size_t)DC_HIST_CAND * NG}, {(void**)&d->hist.gstart, 2 * NG},
    };
    if (!dc_arena_alloc(d->hist_arena, carve, "BSC_DC_HIST_FAIL_ALLOC")) return false;
    d->hist.ext = d->meta + DM_HIST_EXT; d->hist.scr = d->key_sn_s;
    return true;
}
// The context states of m runs (1c), and with the resolve behind them (1c').  No sync: the resolve's kernels are launched whether or
// not a run is open, and leave at once where none is.
template <class SB>
static int dc_launch_ctx(bscgpu_ctx* c, DevCoder* d, u32 m, const SB& S, bool always_exact = false)
{
    const u32 gm8 = ((m + WG - 1) / WG + 7u) / 8u * 8u;                // (dc_virtual_block())
    // (buffers that do not fit: the option stays without effect — dc_ctx_kernel<SB> with its look-back, as with the option off; not an error)
    if (!((c->dc_hist_exact || always_exact) && devcoder_hist_ensure(d))) {
        hipLaunchKernelGGL(dc_ctx_kernel<SB>, dim3(gm8), dim3(WG), 0, c->stream, d->key_ch, d->key_ch_s, d->inv_ch, m, S, d->tab_rank, d->tab_run,
                           d->key_sr, d->key_sn, d->present, d->meta, DcHistNoRec{});
        return BSC_NO_ERROR;
    }
    const u32 nch = (m + DC_HIST_CH - 1) / DC_HIST_CH, ngr = (nch + DC_HIST_GROUP - 1) / DC_HIST_GROUP;
    HIP_TRY(c, hipMemsetAsync(d->hist.bits, 0, (size_t)nch * DC_HIST_CH / 8, c->stream));
    HIP_TRY(c, hipMemsetAsync(d->hist.flag, 0, nch, c->stream));
    hipLaunchKernelGGL((dc_ctx_kernel<SB, true>), dim3(gm8), dim3(WG), 0, c->stream, d->key_ch, d->key_ch_s, d->inv_ch, m, S, d->tab_rank, d->tab_run,
                       d->key_sr, d->key_sn, d->present, d->meta, d->hist);
    if (nch > 1) hipLaunchKernelGGL(dc_hist_map_kernel<SB>, dim3((nch - 1 + WAVES - 1) / WAVES), dim3(WG), 0, c->stream, d->key_ch_s, m, d->hist);
    if (ngr > 1) hipLaunchKernelGGL((dc_avg_chain_kernel<false, DcHistRec>), dim3(ngr - 1), dim3(64), 0, c->stream, m, d->hist);
    hipLaunchKernelGGL(dc_avg_groups_kernel<DcHistRec>, dim3(1), dim3(64), 0, c->stream, m, d->hist);
    hipLaunchKernelGGL((dc_avg_chain_kernel<true, DcHistRec>), dim3(ngr), dim3(64), 0, c->stream, m, d->hist);
    hipLaunchKernelGGL(dc_hist_fix_kernel<SB>, dim3((nch + WAVES - 1) / WAVES), dim3(WG), 0, c->stream, d->key_ch_s, m, d->tab_run, d->key_sn, d->meta, d->hist);
    return BSC_NO_ERROR;
}

// One of the bodies' two syncs: meta comes down (and whatever rides with it: DcDown), the finished brackets are folded, the context
// notes what the flags say.  BSC_NOT_SUPPORTED: a flag is raised — the block (the pass, the segment) is declined.
struct DcDown { void* dst; const void* src; size_t bytes; };
static int dc_meta_down(bscgpu_ctx* c, DevCoder* d, const DcDown& also)
{
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(d->hmeta, d->meta, DM_COUNT * 4, hipMemcpyDeviceToHost, c->stream));
    if (also.dst) HIP_TRY(c, hipMemcpyAsync(also.dst, also.src, also.bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, ctx_sync(c));
    prof_collect(c);
    c->dc_note = dc_note_from(d->hmeta);
    return d->hmeta[DM_FAIL] != 0 ? BSC_NOT_SUPPORTED : BSC_NO_ERROR;
}

// Before the stream kernel writes ps[psbuf]: the buffer's previous copy-out — an event on the copy stream, or, when it went through the
// DMA engine directly, the signals of its pieces (two blocks ago: long landed; a piece that FAILED to land ends the call).
static int dc_ps_wait(bscgpu_ctx* c, int psbuf)
{
    if (c->ps_guard[psbuf & 1]) HIP_TRY(c, hipStreamWaitEvent(c->stream, c->ps_guard[psbuf & 1], 0));
    for (int b = 0; b < 8; ++b)
        if (c->ps_guard_sig[psbuf & 1][b] && dma_wait(c->ps_guard_sig[psbuf & 1][b]) != 0)
            return ctx_fail(c, BSC_GPU_ERROR, "device coder: the stream buffer's previous copy-out failed", hipSuccess);
    return BSC_NO_ERROR;
}

// Where the form enters on the host (the kernels: DcForm): the sub-blocks' offsets in the stream, from job 0's doff.  The eight go to
// d->poff and come down with meta at the FIRST sync (hmeta[HM_POFF..]: the packed stream's layout is made of them); a table's go to
// d->poff_tab and come down at the LAST sync, where the caller asks for them (poff_host).
static void dc_launch_poff(bscgpu_ctx* c, DevCoder* d, const DcSub& S, u32 m)
{
    hipLaunchKernelGGL(dc_poff_kernel, dim3(1), dim3(16), 0, c->stream, d->doff[0], S, m, d->poff);
}
static void dc_launch_poff(bscgpu_ctx* c, DevCoder* d, const DcSubTab& S, u32)
{
    hipLaunchKernelGGL(dc_poff_tab_kernel, dim3((S.nsub + 1 + WG - 1) / WG), dim3(WG), 0, c->stream, d->doff[0], S, d->poff_tab);
}
static DcDown dc_poff_down(DevCoder* d, const DcSub&, bool last, u32*) { return last ? DcDown{} : DcDown{d->hmeta + HM_POFF, d->poff, 16 * 4}; }
static DcDown dc_poff_down(DevCoder* d, const DcSubTab& S, bool last, u32* poff_host) { return last ? DcDown{poff_host, d->poff_tab, ((size_t)S.nsub + 1) * 4} : DcDown{}; }

// The buffers of the exact resolve of open chunk starts (3'), on the first evaluation that asks for it; false: they do not fit.
static bool devcoder_rp_ensure(bscgpu_ctx* c, DevCoder* d)
{
    if (d->rp_arena.base || d->rp_arena.failed) return !d->rp_arena.failed;
    const size_t slots = 4 * d->nch_cap;
    const Carve carve[] = {{(void**)&d->rp.map, 2 * (size_t)DC_RP_CAND * slots}, {(void**)&d->rp.head, 2 * slots}, {(void**)&d->rp.st, slots}};
    if (!dc_arena_alloc(d->rp_arena, carve, "BSC_DC_REPLAY_FAIL_ALLOC")) return false;
    // (a lane of dc_rp_map_kernel holds at most DC_RP_CAND / 64 candidates and a slot's map DC_RP_CAND entries: the cap can only be lowered)
    d->rp.cand = (c->dc_replay_cand == 0 || c->dc_replay_cand > (u32)DC_RP_CAND) ? (u32)DC_RP_CAND : c->dc_replay_cand;
    return true;
}

// All chains of a block (or of a batched pass: tab) in one set of launches: E[job] events of family fam[job] per job, values to
// d->V[job], counters by mp.  The fast coder's one family is job 1 alone: E = {0, E, 0, 0}, mp_fast.
static int dc_eval(bscgpu_ctx* c, DevCoder* d, const u32 E[4], const int fam[4], const ModelParams* mp, bool tab)
{
    DcEvalAll A;
    A.wstart[0] = 0; A.cstart[0] = 0; A.sink = d->sink;
    // One lane is one serial chain, so the walks are VALU-issue bound with ONE wavefront per SIMD (1024 of them); a few
    // wavefronts more than that and some SIMDs get two, which doubles the kernel's time.  Chunks are therefore DC_EV events
    // (what the brackets need to meet) or as many as it takes to stay at <= 1000 wavefronts (+ <= 4 of padding) per launch.
    A.ev = eval_chunk_events((u64)E[0] + E[1] + E[2] + E[3]);
    for (int job = 0; job < 4; ++job) {
        A.job[job].events = d->events[job]; A.job[job].E = E[job]; A.job[job].rowstart = d->rowstart + (DC_ROWS + 8) * job;
        A.job[job].fam = fam[job];
        A.V[job] = d->V[job];
        const u32 nch = (E[job] + A.ev - 1) / A.ev;
        A.wstart[job + 1] = A.wstart[job] + (nch + 63) / 64;
        A.cstart[job + 1] = A.cstart[job] + (nch + 63) / 64 * 64;           // chunk slots padded to whole wavefronts
    }
    if (A.cstart[4] > 4 * d->nch_cap) return ctx_fail(c, BSC_GPU_ERROR, "device coder: chunk table too small", hipSuccess);
    // (buffers that do not fit: the option stays without effect — the evaluation is what it is with the option off; not an error)
    const bool resolve = c->dc_replay_exact && A.wstart[4] > 0 && devcoder_rp_ensure(c, d);
    prof_begin(c, BSCGPU_K_DC_EVAL, (u64)(E[0] + E[1] + E[2] + E[3]) * 6, (u64)E[0] + E[1] + E[2] + E[3]);
    if (A.wstart[4] > 0) {
        hipLaunchKernelGGL(dc_mark_rows_kernel, dim3((4 * DC_ROWS + WG - 1) / WG), dim3(WG), 0, c->stream, A);
        if (tab) {                                                        // a batched pass: chain starts from the events' full sub-block ids
            DcMarkAll K; u32 emax = 0;
            for (int job = 0; job < 4; ++job) { K.events[job] = d->events[job]; K.esub[job] = d->esub[job]; K.E[job] = E[job]; if (E[job] > emax) emax = E[job]; }
            hipLaunchKernelGGL(dc_mark_chains_kernel, dim3((emax + 8 * WG - 1) / (8 * WG), 4), dim3(WG), 0, c->stream, K, d->meta);
        }
        hipLaunchKernelGGL(dc_eval_wave_kernel<false>, dim3((A.wstart[4] + DC_EVAL_WAVES - 1) / DC_EVAL_WAVES), dim3(64 * DC_EVAL_WAVES), DC_EVAL_LDS, c->stream, A, mp, d->meta, d->elo, d->ehi, (const u16*)nullptr, d->cnt);
        if (resolve) {                                                    // 3': a class of its own in the profile
            prof_end(c);
            prof_begin(c, BSCGPU_K_DC_REPLAY, (u64)A.cstart[4] * 5, A.cstart[4]);
            hipLaunchKernelGGL(dc_rp_map_kernel, dim3((A.cstart[4] + WAVES - 1) / WAVES), dim3(WG), 0, c->stream, A, mp, d->meta, d->elo, d->ehi, d->rp);
            hipLaunchKernelGGL(dc_rp_chain_kernel, dim3((A.cstart[4] + WG - 1) / WG), dim3(WG), 0, c->stream, A, d->meta, d->elo, d->ehi, d->rp);
            prof_end(c);
            prof_begin(c, BSCGPU_K_DC_EVAL, 0, 0);
        }
        hipLaunchKernelGGL(dc_eval_b_kernel, dim3((A.cstart[4] + WG - 1) / WG), dim3(WG), 0, c->stream, A, mp, d->meta, d->elo, d->ehi, d->S);
        hipLaunchKernelGGL(dc_eval_wave_kernel<true>, dim3((A.wstart[4] + DC_EVAL_WAVES - 1) / DC_EVAL_WAVES), dim3(64 * DC_EVAL_WAVES), DC_EVAL_LDS, c->stream, A, mp, d->meta, (u16*)nullptr, (u16*)nullptr, d->S, d->cnt + 3 * 4096);
    }
    prof_end(c);
    return BSC_NO_ERROR;
}

#if DC_EVAL_TIMING
// the per-wavefront timing words dc_eval_wave_kernel left in d->cnt (both of its passes), one line per wavefront on stderr
static void dc_eval_timing_dump(const DevCoder* d)
{
    std::vector<u32> h(6 * 4096);
    (void)hipMemcpy(h.data(), d->cnt, h.size() * 4, hipMemcpyDeviceToHost);
    const u32 nw = 1100;
    for (int pass = 0; pass < 2; ++pass) {
        const u32* t = h.data() + pass * 3 * 4096;
        u32 t0 = 0xffffffffu; for (u32 i = 0; i < nw && i < 4096; ++i) if (t[3 * i + 1] && t[3 * i] < t0) t0 = t[3 * i];
        fprintf(stderr, "[eval timing pass %d] wave: start(us) dur(us) maxslowbatches job\n", pass);
        for (u32 i = 0; i < nw && i < 4096; ++i) if (t[3 * i + 1]) fprintf(stderr, "  %u %.1f %.1f %u %u\n", i, (t[3 * i] - t0) / 100.0, t[3 * i + 1] / 100.0, t[3 * i + 2] & 0xffff, t[3 * i + 2] >> 16);
    }
}
#endif

// ---- the two coders' models, each ONE body for both forms (SB: DcSub, one block's eight sub-blocks; DcSubTab, a pass's or a
// segment's table) -------------------------------------------------------------------------------------------------------------------
// Both take a unit (DcUnit) with its sub-blocks S and write O.D decisions to the device p stream ps[U.psbuf], the sub-blocks' decision
// offsets where dc_poff_down says.  The caller has cleared meta (the static coder: present too), and launched what its form needs in
// front of the items.  Every guarded exit declines the whole unit (BSC_NOT_SUPPORTED, c->dc_note.fail says why).  Two syncs: the
// families' sizes after the partition, the flags after the stream.
//
// The unit: the front end's run arrays on the device with the avg_rank flags, and how it runs.
struct DcUnit {
    const u8 *sym, *rank; const u32* start; const u8* ge32;      // m runs
    u32 m, n;                   // n: the block's bytes, 0 for a table, which carries its own ends
    int psbuf;                  // the device p stream written: ps[psbuf & 1]
    int64_t expect;             // >= 0: the decisions the plan counted for these sub-blocks — the families' totals must equal it
    bool ctx_open;              // the caller's contexts bracket of the profile is still open and takes the items as well (a single block)
    const ModelParams* mp = nullptr;   // the adaptive coder's counters (device copy): dc_static_run with these rates, the run_hist resolve always on
};
// What comes back, and where what comes down to the host goes.  Written on success only.
struct DcOut {
    u32  D = 0;                 // decisions written
    bool take_packed = false;   // in (static coder): the caller can take the stream at 13 bits per decision (DcP13 / DcP13Tab) ...
    bool packed = false;        // ... and that is what was written
    u32* poff_host = nullptr;   // a table: poff[0..nsub] (the eight of a block: hmeta[HM_POFF..])
    u32* pbase_host = nullptr;  // a table, packed: pbase[0..nsub], where the caller keeps the offsets (its end: hmeta[HM_PBASE_END], always)
    u16* dbg = nullptr;         // the static coder's debug planes (device)
};

// The static coder (-e1), the four stages of the file header.
template <class SB>
static int dc_static_run(bscgpu_ctx* c, DevCoder* d, const SB& S, const DcUnit& U, DcOut& O)
{
    constexpr bool TAB = DcForm<SB>::TAB;
    const u32 m = U.m;
    const int psbuf = U.psbuf; u16* const dbg = O.dbg;
    const ModelParams* const mp = U.mp ? U.mp : d->mp;
    const u32 gm = (m + WG - 1) / WG;
    const u32 gm8 = (gm + 7u) / 8u * 8u;            // kernels that use dc_virtual_block()
    if (!U.ctx_open) prof_begin(c, BSCGPU_K_DC_CTX, (u64)m * 40, m);
    hipLaunchKernelGGL(dc_items_kernel<SB>, dim3(gm), dim3(WG), 0, c->stream, U.sym, U.rank, U.start, U.ge32, m, U.n, S, d->key_ch);
    prof_end(c);
    RadixPass top; top.shift = 56; top.bits = 8;
    int in_alt = 0;
    // one pass: the engine reads `keys` (left intact) and writes the sorted copy to the alt array
    int rc = radix_sort_passes(c, d->key_ch, d->key_ch_s, nullptr, nullptr, m, &top, 1, &in_alt, d->inv_ch);
    if (rc < 0) return rc;
    prof_begin(c, BSCGPU_K_DC_CTX, (u64)m * 40, m);
    rc = dc_launch_ctx(c, d, m, S, U.mp != nullptr);   // (with BSCGPU_OPT_DC_HIST_EXACT: and the resolve of the open run_hist brackets, 1c')
    if (rc < 0) { prof_end(c); return rc; }
    hipLaunchKernelGGL(dc_setup_kernel<SB>, dim3(1), dim3(WG), 0, c->stream, d->present, S, d->rounds, d->meta,
                       (u32)(c->dc_avg_exact ? DM_AVG_LEFT : DM_AVG_UND));
    prof_end(c);
    rc = radix_sort_passes(c, d->key_sr, d->key_sr_s, nullptr, nullptr, m, &top, 1, &in_alt, d->inv_sr);
    if (rc < 0) return rc;
    rc = radix_sort_passes(c, d->key_sn, d->key_sn_s, nullptr, nullptr, m, &top, 1, &in_alt, d->inv_sn);
    if (rc < 0) return rc;

    // families: static (stream order, X ignored), char (symbol-major), state (rank side by rank-state, run side by run-state):
    // four independent partition jobs, then ONE read-back of their sizes, then all chains of the block in one set of launches
    dc_launch_partition<3>(c, d, d->key_ch, m, S, 0, 1u);
    dc_launch_partition<3>(c, d, d->key_ch_s, m, S, 1, 0u);
    dc_launch_partition<1>(c, d, d->key_sr_s, m, S, 2, 0u);
    dc_launch_partition<2>(c, d, d->key_sn_s, m, S, 3, 0u);
    dc_launch_poff(c, d, S, m);                     // (the sub-blocks' offsets in the stream are known from here on)
    if constexpr (TAB) {                            // ... and where they start in the packed space, if that is what the caller takes
        if (O.take_packed) hipLaunchKernelGGL(dc_pbase_tab_kernel, dim3(1), dim3(WG), 0, c->stream, d->poff_tab, S.nsub, d->pad_tab, d->pbase_tab);
    }
    rc = dc_meta_down(c, d, dc_poff_down(d, S, false, O.poff_host));
    if (rc < 0) return rc;
    u32 E[4];
    for (int job = 0; job < 4; ++job) E[job] = d->hmeta[DM_D0 + job];
    const u32 Efull = E[0];                                           // decisions of the block
    if (Efull != E[1] || Efull != E[2] + E[3]) return ctx_fail(c, BSC_GPU_ERROR, "device coder: decision counts of the families differ", hipSuccess);
    if (U.expect >= 0 && (int64_t)Efull != U.expect) return ctx_fail(c, BSC_GPU_ERROR, "device coder: a segment's decisions differ from the plan's count", hipSuccess);
    const int fam[4] = {FAM_STATIC, FAM_CHAR, FAM_STATE, FAM_STATE};
    rc = dc_eval(c, d, E, fam, mp, DcForm<SB>::TAB);
    if (rc < 0) return rc;

    DcGather G;
    G.key_ch = d->key_ch; G.m = m; G.inv_ch = d->inv_ch; G.inv_sr = d->inv_sr; G.inv_sn = d->inv_sn;
    G.doff_sp = d->doff[0]; G.doff_ch = d->doff[1]; G.doff_sr = d->doff[2]; G.doff_sn = d->doff[3];
    G.pos_sp = d->pos[0]; G.pos_ch = d->pos[1]; G.pos_sr = d->pos[2]; G.pos_sn = d->pos[3];
    G.V_sp = d->V[0]; G.V_ch = d->V[1]; G.V_sr = d->V[2]; G.V_sn = d->V[3];
    prof_begin(c, BSCGPU_K_DC_PSTREAM, (u64)Efull * 26, Efull);
    rc = dc_ps_wait(c, psbuf);
    if (rc < 0) return rc;
    bool packed = false;
    typename DcP13Of<SB>::T Q{};
    if constexpr (TAB) {
        // a pass's or a segment's: the offsets are on the device (dc_pbase_tab_kernel), the host knows only their bound — every sub-block
        // pads by at most 63 decisions.  13 / 8 of that against the 2 Dcap bytes of the buffer: fits whenever Dcap >= 2.2 M decisions
        // (contexts from ~0.5 MiB up), whatever the pass; a pass that does not takes the 2-byte form like a void one
        packed = O.take_packed && ((u64)Efull + 63ull * S.nsub + 7ull) / 8ull * 13ull <= 2ull * (u64)(d->Dcap + 64);
        if (packed) { Q.pad = d->pad_tab; Q.out = reinterpret_cast<u8*>(d->ps[psbuf & 1]); Q.frag = d->frag; }
    } else {
        // 13 bits per decision (DcP13) when the caller can take it: not with the debug planes
        packed = O.take_packed && c->dc_p13 != 0 && dbg == nullptr;
        if (packed) {
            const u32* poff_h = d->hmeta + HM_POFF;
            u32 pbase = 0;
            for (u32 b = 0; b < S.nb; ++b) { Q.pad[b] = pbase - poff_h[b]; pbase += (poff_h[b + 1] - poff_h[b] + 63u) / 64u * 64u; }
            Q.out = reinterpret_cast<u8*>(d->ps[psbuf & 1]); Q.frag = d->frag;
            if ((u64)pbase / 8u * 13u > 2ull * (u64)(d->Dcap + 64)) packed = false;        // (cannot happen: 13 / 8 of D + 8 x 64 decisions of padding against 2 D)
        }
    }
    if (packed) {
        // (d->frag holds two records for each of the gm8 * WAVES <= m / 64 + 32 wavefronts: (Mcap + 64) / 64 + 64 pairs, m <= Mcap)
        hipLaunchKernelGGL((dc_pstream_kernel<false, true, SB>), dim3(gm8), dim3(WG), 0, c->stream, G, S, mp, d->meta, d->ps[psbuf & 1], dbg, Efull, Q);
        hipLaunchKernelGGL(dc_p13_join_kernel, dim3((gm8 * WAVES + WG - 1) / WG), dim3(WG), 0, c->stream, d->frag, gm8 * WAVES, Q.out, d->meta);
        if constexpr (TAB) {
            hipLaunchKernelGGL(dc_p13_fill_tab_kernel, dim3((S.nsub + WG - 1) / WG), dim3(WG), 0, c->stream, d->poff_tab, d->pbase_tab, S.nsub, Q.out, d->meta);
            // the layout comes down with the flags: its end for every caller (hmeta[HM_PBASE_END]), all of it where the caller keeps the offsets
            HIP_TRY(c, hipMemcpyAsync(d->hmeta + HM_PBASE_END, d->pbase_tab + S.nsub, 4, hipMemcpyDeviceToHost, c->stream));
            if (O.pbase_host) HIP_TRY(c, hipMemcpyAsync(O.pbase_host, d->pbase_tab, ((size_t)S.nsub + 1) * 4, hipMemcpyDeviceToHost, c->stream));
        }
    }
    if (!packed) hipLaunchKernelGGL((dc_pstream_kernel<false, false, SB>), dim3(gm8), dim3(WG), 0, c->stream, G, S, mp, d->meta, d->ps[psbuf & 1], dbg, Efull, Q);
    prof_end(c);
    rc = dc_meta_down(c, d, dc_poff_down(d, S, true, O.poff_host));
    if (rc < 0) return rc;
    if (packed && d->hmeta[DM_P13_OVER] != 0) {
        // 64 consecutive runs with more decisions than a wavefront's staging buffer holds (runs of thousands): this block's (pass's,
        // segment's) stream in the 2-byte form
        packed = false;
        prof_begin(c, BSCGPU_K_DC_PSTREAM, (u64)Efull * 26, Efull);
        hipLaunchKernelGGL((dc_pstream_kernel<false, false, SB>), dim3(gm8), dim3(WG), 0, c->stream, G, S, mp, d->meta, d->ps[psbuf & 1], dbg, Efull, Q);
        prof_end(c);
        HIP_TRY(c, hipGetLastError());
        HIP_TRY(c, ctx_sync(c));
    }
#if DC_EVAL_TIMING
    dc_eval_timing_dump(d);
#endif
    if (getenv("BSCGPU_DEBUG")) fprintf(stderr, "[devcoder] runs %u, decisions %u, types %u, rounds %u, chunks replayed %u\n", m, Efull, d->hmeta[DM_NTYPES], d->hmeta[DM_NROUNDS], d->hmeta[DM_REPLAYS]);
    O.D = Efull; O.packed = packed;
    return BSC_NO_ERROR;
}

// The fast coder (-e0, qlfc.cpp:1135-1336) on the same machinery: its one counter per decision is indexed by the run's symbol, i.e. its
// chains ARE the char family's — (sub-block, decision type, symbol) — with shift updates and per-class targets (dcm::model_params_fast),
// no escape coding and the exponent always closed below 7 bits (max_rank = 7 in the static coder's terms).  So: items, ONE radix pass
// (symbol-major order), the stream offsets of the runs (job 0: counts and scans only), ONE partition job (job 1; for a table its
// scatter writes every event's full sub-block id to esub[1], which dc_mark_chains_kernel folds into the chain-start mark), evaluation
// of that one job with mp_fast, and a p stream whose entries are the counter values themselves (dcm::PSF_*).  No contexts, no state
// tables, no blend: about a third of the static coder's device work.  No avg_rank flags, no run_hist look-back: FAIL_CAP and
// FAIL_REPLAY are the only flags that can be raised.  The caller has cleared ge32 as well.
template <class SB>
static int dc_fast_run(bscgpu_ctx* c, DevCoder* d, const SB& S, const DcUnit& U, DcOut& O)
{
    const u32 m = U.m;
    const u32 gm = (m + WG - 1) / WG;
    const u32 gm8 = (gm + 7u) / 8u * 8u;            // kernels that use dc_virtual_block()
    if (!U.ctx_open) prof_begin(c, BSCGPU_K_DC_CTX, (u64)m * 14, m);
    hipLaunchKernelGGL(dc_items_kernel<SB>, dim3(gm), dim3(WG), 0, c->stream, U.sym, U.rank, U.start, U.ge32, m, U.n, S, d->key_ch);
    prof_end(c);
    RadixPass top; top.shift = 56; top.bits = 8;
    int in_alt = 0;
    int rc = radix_sort_passes(c, d->key_ch, d->key_ch_s, nullptr, nullptr, m, &top, 1, &in_alt, d->inv_ch);
    if (rc < 0) return rc;
    dc_launch_partition<3, false>(c, d, d->key_ch, m, S, 0, 0u);
    dc_launch_partition<3>(c, d, d->key_ch_s, m, S, 1, 0u);
    dc_launch_poff(c, d, S, m);
    rc = dc_meta_down(c, d, dc_poff_down(d, S, false, O.poff_host));
    if (rc < 0) return rc;
    const u32 E[4] = {0u, d->hmeta[DM_D0 + 1], 0u, 0u};
    if (d->hmeta[DM_D0 + 0] != E[1]) return ctx_fail(c, BSC_GPU_ERROR, "device coder (fast): decision counts of stream and chain order differ", hipSuccess);
    if (U.expect >= 0 && (int64_t)E[1] != U.expect) return ctx_fail(c, BSC_GPU_ERROR, "device coder (fast): a segment's decisions differ from the plan's count", hipSuccess);
    const int fam[4] = {FAM_CHAR, FAM_CHAR, FAM_CHAR, FAM_CHAR};
    rc = dc_eval(c, d, E, fam, d->mp_fast, DcForm<SB>::TAB);
    if (rc < 0) return rc;

    DcGather G;                                     // (everything is job 1's: the stream kernel reads one value per decision)
    G.key_ch = d->key_ch; G.m = m; G.inv_ch = d->inv_ch; G.inv_sr = d->inv_ch; G.inv_sn = d->inv_ch;
    G.doff_sp = d->doff[0]; G.doff_ch = d->doff[1]; G.doff_sr = d->doff[1]; G.doff_sn = d->doff[1];
    G.pos_sp = d->pos[1]; G.pos_ch = d->pos[1]; G.pos_sr = d->pos[1]; G.pos_sn = d->pos[1];
    G.V_sp = d->V[1]; G.V_ch = d->V[1]; G.V_sr = d->V[1]; G.V_sn = d->V[1];
    prof_begin(c, BSCGPU_K_DC_PSTREAM, (u64)E[1] * 10, E[1]);
    rc = dc_ps_wait(c, U.psbuf);
    if (rc < 0) return rc;
    hipLaunchKernelGGL((dc_pstream_kernel<true, false, SB>), dim3(gm8), dim3(WG), 0, c->stream, G, S, d->mp_fast, d->meta, d->ps[U.psbuf & 1], (u16*)nullptr, E[1], typename DcP13Of<SB>::T{});
    prof_end(c);
    rc = dc_meta_down(c, d, dc_poff_down(d, S, true, O.poff_host));
    if (rc < 0) return rc;
    if (getenv("BSCGPU_DEBUG")) fprintf(stderr, "[devcoder fast] runs %u, decisions %u, chunks replayed %u\n", m, E[1], d->hmeta[DM_REPLAYS]);
    O.D = E[1];
    return BSC_NO_ERROR;
}

// What every unit of model work (a block, a pass, a pass's facts, a segment) starts from: the meta words cleared and, where the static
// coder's model follows, the context kinds it has seen.
static int dc_unit_clear(bscgpu_ctx* c, DevCoder* d, bool kinds_seen)
{
    HIP_TRY(c, hipMemsetAsync(d->meta, 0, DM_COUNT * 4, c->stream));
    if (kinds_seen) HIP_TRY(c, hipMemsetAsync(d->present, 0, (size_t)DC_KIND_WORDS * 4, c->stream));
    return BSC_NO_ERROR;
}

// Probability stream of a whole block.  Inputs: the QLFC front end's run arrays on the device (sym / rank / start, m runs of
// the n-byte sorted block), the sub-blocks' run ranges and max_rank values; coder 1: dc_static_run, 3: dc_fast_run.  On success
// *D_out decisions were written to the device p stream (d->ps) and poff[0..nb] (decision offsets of the sub-blocks) to hmeta[HM_POFF..];
// returns BSC_NOT_SUPPORTED when the block has to go through the host model instead.
int devcoder_pstream(bscgpu_ctx* c, const u8* dsym, const u8* drank, const u32* dstart, u32 m, u32 n, int nb, const u32* run_first,
                     const int* max_rank, u32* D_out, u32* poff_out, u16* dbg, int psbuf, int coder, int* packed_out)
{
    if (packed_out) *packed_out = 0;
    int rc = devcoder_ensure(c);
    if (rc < 0) return rc;
    DevCoder* d = c->dc;
    c->dc_note.clear(m > d->Mcap ? (int)FAIL_CAP : 0);                 // (more runs than the arena holds: capacity, as too many decisions are)
    if (m == 0 || m > d->Mcap || nb < 1 || nb > 8) return BSC_NOT_SUPPORTED;
    const bool fast = coder == 3;
    DcSub S; S.nb = (u32)nb;
    for (int b = 0; b < 9; ++b) S.first[b] = (b <= nb) ? run_first[b] : m;
    // (the fast coder: `if (bits < 7)` closes the exponent (qlfc.cpp:1204), whatever the alphabet)
    for (int b = 0; b < 8; ++b) S.maxr[b] = fast ? 7u : (b < nb) ? (u32)max_rank[b] : 0u;

    rc = dc_unit_clear(c, d, !fast);
    if (rc < 0) return rc;
    prof_begin(c, BSCGPU_K_DC_CTX, (u64)m * (fast ? 14 : 40), m);
    // avg' = (124 avg + 4 rank) >> 7 <= max(avg, rank) and rank < nsym <= 2^(max_rank + 1): with at most 32 symbols in every
    // sub-block the average never reaches 32 and the escape coding (qlfc.cpp:960) cannot occur; the fast coder has none
    bool may_escape = false;
    for (int b = 0; b < nb && !fast; ++b) may_escape |= max_rank[b] > 4;
    if (may_escape) {
        rc = dc_launch_avg(c, d, drank, m, S, (u32*)nullptr);
        if (rc < 0) { prof_end(c); return rc; }
    } else
        HIP_TRY(c, hipMemsetAsync(d->ge32, 0, m, c->stream));
    DcUnit U;
    U.sym = dsym; U.rank = drank; U.start = dstart; U.ge32 = d->ge32; U.m = m; U.n = n;
    U.psbuf = psbuf; U.expect = -1; U.ctx_open = true;
    DcOut O;
    O.take_packed = packed_out != nullptr; O.dbg = dbg;
    rc = fast ? dc_fast_run(c, d, S, U, O) : dc_static_run(c, d, S, U, O);
    if (rc < 0) return rc;
    *D_out = O.D;
    if (packed_out) *packed_out = O.packed ? 1 : 0;
    for (int b = 0; b <= nb; ++b) poff_out[b] = d->hmeta[HM_POFF + b];
    return BSC_NO_ERROR;
}

// ---- a block in sub-block segments ("A block in sub-block segments") ----------------------------------------------------
// Sub-blocks are independent chains, so the model can run over any contiguous range of a block's sub-blocks and write the same entries
// — what the batched path does with a pass (below), here in the eight-entry form, which takes run lengths up to 2^31: to every kernel
// the range is a block of its own (S.first rebased to its first run, the run arrays and the flags offset by it, n = the end of its last
// sub-block).  What is needed of the whole block comes first, once: the avg_rank flags of all its runs (ge32 holds a byte per run of
// max_n) and, for the plan (dc_block_plan.h), every sub-block's decisions and the flags left open.
static bool devcoder_block_ensure(DevCoder* d)
{
    if (d->blk_arena.base || d->blk_arena.failed) return !d->blk_arena.failed;
    const Carve carve[] = {{(void**)&d->blk_dec, 8 * 4}, {(void**)&d->blk_und, 8 * 4}};
    return dc_arena_alloc(d->blk_arena, carve, nullptr);
}
static DcSub dc_block_sub(int nb, const u32* first, const u32* maxr, u32 m)
{
    DcSub S; S.nb = (u32)nb;
    for (int b = 0; b < 9; ++b) S.first[b] = (b <= nb) ? first[b] : m;
    for (int b = 0; b < 8; ++b) S.maxr[b] = (b < nb) ? maxr[b] : 0u;
    return S;
}
// The facts: flags behind dc_launch_avg over the whole block (the fast coder and a block that cannot escape: zero, as devcoder_pstream),
// then dc_sub_dec8_kernel.  One sync.  B->sum: the avg values of the block, as a pass's in segments.
static int dc_block_facts(bscgpu_ctx* c, DevCoder* d, DcBlock* B, const u32* run_first)
{
    u32 first[9];
    for (int b = 0; b < 9; ++b) first[b] = b <= B->nb ? run_first[b] : B->m;
    DcSubU S; static_cast<DcSub&>(S) = dc_block_sub(B->nb, first, B->maxr, B->m);
    int rc = dc_unit_clear(c, d, /* kinds_seen: no model runs here */ false);
    if (rc < 0) return rc;
    HIP_TRY(c, hipMemsetAsync(d->blk_dec, 0, 8 * 4, c->stream));
    HIP_TRY(c, hipMemsetAsync(d->blk_und, 0, 8 * 4, c->stream));
    prof_begin(c, BSCGPU_K_DC_FACTS, (u64)B->m * 6, B->m);
    bool may_escape = false;
    for (int b = 0; b < B->nb && !B->fast; ++b) may_escape |= B->maxr[b] > 4u;
    if (may_escape) {
        rc = dc_launch_avg(c, d, B->rank, B->m, S, d->blk_und);
        if (rc < 0) { prof_end(c); return rc; }
    } else
        HIP_TRY(c, hipMemsetAsync(d->ge32, 0, B->m, c->stream));
    const u32 dec_grid = ((B->m + 63u) / 64u + WAVES - 1) / WAVES;
    hipLaunchKernelGGL(dc_sub_dec8_kernel, dim3(dec_grid < DC_SUB_DEC8_GRID ? dec_grid : DC_SUB_DEC8_GRID), dim3(WG), 0, c->stream, B->sym, B->rank, B->start, d->ge32, B->m, B->n,
                       static_cast<const DcSub&>(S), d->blk_dec);
    prof_end(c);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(d->hmeta, d->meta, DM_COUNT * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(d->hmeta + HM_POFF, d->blk_dec, 8 * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(d->hmeta + HM_POFF + 8, d->blk_und, 8 * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, ctx_sync(c));
    prof_collect(c);
    for (int b = 0; b < 8; ++b) { B->dec[b] = b < B->nb ? d->hmeta[HM_POFF + b] : 0u; B->und[b] = b < B->nb ? d->hmeta[HM_POFF + 8 + b] : 0u; }
    B->sum.avg_und = (int)d->hmeta[DM_AVG_UND]; B->sum.avg_resolved = (int)d->hmeta[DM_AVG_RESOLVED];
    return BSC_NO_ERROR;
}
static int dc_block_open(bscgpu_ctx* c, const u8* dsym, const u8* drank, const u32* dstart, u32 m, u32 n, int nb, const int* sub_start,
                         const int* sub_size, const int* max_rank, int coder, DcBlock* B)
{
    int rc = devcoder_ensure(c);
    if (rc < 0) return rc;
    DevCoder* d = c->dc;
    c->cnt_block_segments = 0;
    c->dc_note.clear(m > d->Gcap ? (int)FAIL_CAP : 0);
    if (m == 0 || m > d->Gcap || nb < 1 || nb > 8) return BSC_NOT_SUPPORTED;
    if (!devcoder_block_ensure(d)) return BSC_NOT_SUPPORTED;            // does not fit: declined, no reason bit (as the batch arena)
    *B = DcBlock();
    B->sym = dsym; B->rank = drank; B->start = dstart; B->m = m; B->n = n; B->nb = nb; B->fast = coder == 3;
    // (the fast coder: `if (bits < 7)` closes the exponent (qlfc.cpp:1204), whatever the alphabet)
    for (int b = 0; b < nb; ++b) { B->maxr[b] = B->fast ? 7u : (u32)max_rank[b]; B->end[b] = (u32)(sub_start[b] + sub_size[b]); }
    return BSC_NO_ERROR;
}
int devcoder_block_begin(bscgpu_ctx* c, const u8* dsym, const u8* drank, const u32* dstart, u32 m, u32 n, int nb, const int* sub_start,
                         const int* sub_size, const u32* run_first, const int* max_rank, int coder, bool take_packed, DcBlock* B)
{
    int rc = dc_block_open(c, dsym, drank, dstart, m, n, nb, sub_start, sub_size, max_rank, coder, B);
    if (rc < 0) return rc;
    DevCoder* d = c->dc;
    rc = dc_block_facts(c, d, B, run_first);
    if (rc < 0) return rc;
    c->dc_note = B->sum;
    int64_t open = 0;
    for (int b = 0; b < nb; ++b) open += B->und[b];
    if (open) { c->dc_note.fail = (int)FAIL_AVG; return BSC_NOT_SUPPORTED; }       // (what dc_setup_kernel raises for a block run whole)
    B->packed = take_packed && !B->fast && c->dc_p13 != 0;
    B->plan = DcBlockSchedule(run_first, B->dec, nb, (int64_t)d->Mcap, (int64_t)d->Dcap, B->packed);
    if (B->plan.segments() == DC_BLOCK_NOT_SUPPORTED) { c->dc_note.fail = (int)FAIL_CAP; return BSC_NOT_SUPPORTED; }
    if (B->plan.segments() < 0) return ctx_fail(c, BSC_GPU_ERROR, "device coder: no plan for the block's segments", hipSuccess);
    return BSC_NO_ERROR;
}
int devcoder_block_facts(bscgpu_ctx* c, const u8* dsym, const u8* drank, const u32* dstart, u32 m, u32 n, int nb, const int* sub_start,
                         const int* sub_size, const u32* run_first, const int* max_rank, int coder, DcBlock* B)
{
    const int rc = dc_block_open(c, dsym, drank, dstart, m, n, nb, sub_start, sub_size, max_rank, coder, B);
    return rc < 0 ? rc : dc_block_facts(c, c->dc, B, run_first);
}
int devcoder_block_segment(bscgpu_ctx* c, DcBlock* B, const DcBlockSeg& g, int psbuf, bool* host_packed)
{
    DevCoder* d = c->dc;
    *host_packed = false;
    int rc = dc_unit_clear(c, d, !B->fast);
    if (rc < 0) return rc;
    const DcSub S = dc_block_sub(g.s1 - g.s0, g.first, B->maxr + g.s0, g.r1 - g.r0);
    DcUnit U;
    U.sym = B->sym + g.r0; U.rank = B->rank + g.r0; U.start = B->start + g.r0; U.ge32 = d->ge32 + g.r0; U.m = g.r1 - g.r0;
    U.n = B->end[g.s1 - 1];                                            // (the last run of the range ends with its sub-block)
    U.psbuf = psbuf; U.expect = g.expect; U.ctx_open = false;
    DcOut O;
    O.take_packed = B->packed;
    rc = B->fast ? dc_fast_run(c, d, S, U, O) : dc_static_run(c, d, S, U, O);
    const DcNote& run = c->dc_note;
    B->sum.fail |= run.fail; B->sum.replays += run.replays; B->sum.hist_ext += run.hist_ext;
    B->sum.replay_resolved += run.replay_resolved; B->sum.hist_resolved += run.hist_resolved;
    c->dc_note = B->sum;
    if (rc < 0) return rc;
    if (!B->plan.agrees(g, d->hmeta + HM_POFF)) return ctx_fail(c, BSC_GPU_ERROR, "device coder: a segment's sub-block offsets differ from the plan's", hipSuccess);
    *host_packed = B->packed && !O.packed;
    ++c->cnt_block_segments;
    if (B->packed) ++(O.packed ? c->cnt_packed_passes : c->cnt_packed_void);
    return BSC_NO_ERROR;
}

// ---- the model of a whole batched pass ------------------------------------------------------------------------------
// What the wider chain identity needs on top of the arena, on the first pass that takes this route: every event's full sub-block
// id (2 bytes per decision and family = 8 Dcap bytes, ~32 bytes per byte of max_n), max_rank and stream offset per sub-block.
// false: it does not fit.
static bool devcoder_batch_ensure(DevCoder* d)
{
    if (d->batch_arena.base || d->batch_arena.failed) return !d->batch_arena.failed;
    CtxTimer tm("devcoder_batch_ensure (sub-block ids of the events)");
    const size_t D = d->Dcap + 64;
    const Carve carve[] = {
        {(void**)&d->esub[0], 2 * D}, {(void**)&d->esub[1], 2 * D}, {(void**)&d->esub[2], 2 * D}, {(void**)&d->esub[3], 2 * D},
        {(void**)&d->sub_maxr, (size_t)FRONT_MAX_SUB + 64}, {(void**)&d->poff_tab, 4 * ((size_t)FRONT_MAX_SUB + 64)},
        {(void**)&d->sub_und, 4 * ((size_t)FRONT_MAX_SUB + 64)}, {(void**)&d->sub_dec, 4 * ((size_t)FRONT_MAX_SUB + 64)},
        {(void**)&d->seg_run, 4 * ((size_t)FRONT_MAX_SUB + 64)}, {(void**)&d->sub_mix, 4 * ((size_t)FRONT_MAX_SUB + 64)},
        {(void**)&d->pad_tab, 4 * ((size_t)FRONT_MAX_SUB + 64)}, {(void**)&d->pbase_tab, 4 * ((size_t)FRONT_MAX_SUB + 64)},
    };
    return dc_arena_alloc(d->batch_arena, carve, nullptr);
}

// What the entry points of a pass share: the arenas, the pass as qlfc_front_batch left it — the run arrays (FrontBufs: the buffers
// the single path reads) and its table in front_tab, with max_rank per sub-block where dc_tab_prep_kernel will put it.
// over_fail >= 0: the call is a model run, which clears what the context says about its last block; over_fail is what dc_note.fail
// then says about a pass of more runs than the arena holds (a whole pass: FAIL_CAP, as devcoder_pstream; segments: 0).
struct DcPass { DevCoder* d; FrontTab T; DcSubTab S; const u8 *dsym, *drank; const u32* dstart; };
static int dc_pass_begin(bscgpu_ctx* c, u32 m, int nsub, int over_fail, DcPass* P)
{
    int rc = devcoder_ensure(c);
    if (rc < 0) return rc;
    DevCoder* d = c->dc;
    if (over_fail >= 0) c->dc_note.clear(m > d->Mcap ? over_fail : 0);
    if (m == 0 || m > d->Mcap || nsub < 1 || nsub > FRONT_MAX_SUB || !c->front_tab) return BSC_NOT_SUPPORTED;
    if (!devcoder_batch_ensure(d)) return BSC_NOT_SUPPORTED;             // does not fit: the pass is declined (its blocks take the host model), not an error
    P->d = d; P->T = qlfc_front_tab(c, nsub);
    { const FrontBufs fb = front_bufs(c); P->dsym = fb.sym; P->drank = fb.rank; P->dstart = fb.start; }
    P->S.nsub = (u32)nsub; P->S.run = P->T.sub_run; P->S.off = P->T.sub_off; P->S.base = P->T.sub_base; P->S.maxr = d->sub_maxr;
    return BSC_NO_ERROR;
}
// Runs [r0, r1) of the pass as a unit of their own (all of it: [0, m)): the run arrays and the flags offset to its first run
static DcUnit dc_pass_range(const DcPass& P, u32 r0, u32 r1, int psbuf, int64_t expect)
{
    DcUnit U;
    U.sym = P.dsym + r0; U.rank = P.drank + r0; U.start = P.dstart + r0; U.ge32 = P.d->ge32 + r0; U.m = r1 - r0; U.n = 0u;
    U.psbuf = psbuf; U.expect = expect; U.ctx_open = false;
    return U;
}
// ... and what every model of the pass reads: max_rank per sub-block and the rebased run table, then the avg_rank >= 32 flags.  The
// static coder walks them always (which sub-blocks can escape is not known on the host here; one of at most 32 symbols never leaves a
// flag open — avg_top), sub_und non-null: with the flags left open counted per sub-block; the fast coder has no escape coding.
// Inside the caller's profile bracket.
static int dc_pass_tables(bscgpu_ctx* c, const DcPass& P, u32 m, bool fast, u32* sub_und)
{
    DevCoder* d = P.d;
    hipLaunchKernelGGL(dc_tab_prep_kernel, dim3((P.S.nsub + WAVES - 1) / WAVES), dim3(WG), 0, c->stream, P.T.first_run, P.S.nsub, m, fast ? 7 : -1, d->sub_maxr, P.T.sub_run);
    if (!fast) return dc_launch_avg(c, d, P.drank, m, P.S, sub_und);
    HIP_TRY(c, hipMemsetAsync(d->ge32, 0, m, c->stream));
    return BSC_NO_ERROR;
}

// ---- the adaptive coder's model of a pass (-e2; DESIGN §2b, "The adaptive coder's model of a pass") -------------------------------
// dc_static_run with the adaptive rates leaves, per decision in stream order, the three counter values (the debug planes) and the
// coded bit with the run-start mark (the stream's entries; their blended probability is not used).  What is left is the mixer: one of
// NUM_MIX instances per sub-block picks the probability, and an instance only ever sees its own decisions — a chain (sub-block,
// mixer id).  A pass of small blocks has ~10^5 such chains, the longest a few 10^4 steps:
//   (a) dc_mix_hist_kernel   rank_hist and the UNCLAMPED run_hist of every run (run_exp is indexed by the full value; the static
//                            model's contexts keep min(run_hist, 7)): a workgroup per sub-block, a thread per symbol, the sub-block's
//                            runs through LDS — exact by construction, no bracket
//       dc_mix_key_kernel    thread per run: key = (sub-block << 11 | mixer id) << 32 | stream position of every decision
//   (b) radix passes         stable, keys only, on the 11 + log2(nsub) key bits above bit 32: chain-major order, the permutation in the
//                            keys' low words
//   (c) dc_mix_gather_kernel thread per decision in chain-major order: its 8-byte record (counter values, bit, run-start mark) next
//                            to its key; the last decision of a chain finds the chain's first by bisection and notes (start, length)
//       dc_mix_place_kernel  the chains by descending bsr(length), so that the 64 lanes of a wavefront walk chains of similar length
//   (d) dc_mix_walk_kernel   one lane per chain: weights in registers, the 17-cell map in an LDS row of its own, stretch / squash
//                            shared in LDS; the probabilities in chain-major order
//       dc_mix_scatter_kernel  thread per decision: the entry {p, bit, run start} to the decision's stream position
// Guard: the longest chain above the context's step cap (BSC_DC_MIX_CHAIN_CAP) declines the pass, FAIL_MIX.
enum { MX_CNT = 0 /* chains per bsr(length), 32 */, MX_OFF = 32 /* first slot of each, 32 */, MX_FILL = 64 /* 32 */, MX_CHAINS = 96, MX_LONGEST = 97, MX_WORDS = 128 };
constexpr int MX_TAB = 4104;                                          // shorts per table (4097, padded to 16 bytes)
constexpr int MX_MAP_STRIDE = 18;                                     // shorts per lane's map row: 9 words, odd against bank conflicts

__global__ __launch_bounds__(WG) void dc_mix_hist_kernel(const u64* __restrict__ key_ch, DcSubTab S, u16* __restrict__ hist)
{
    static_assert(WG == 256, "a thread per symbol");
    __shared__ u32 s_it[WG], s_run[WG];
    const u32 s = blockIdx.x, t = threadIdx.x;
    const u32 r0 = S.run[s], r1 = S.run[s + 1];
    u32 rh = 0, nh = 0;
    for (u32 base = r0; base < r1; base += WG) {
        const u32 n = r1 - base < (u32)WG ? r1 - base : (u32)WG;
        if (t < n) {
            const u64 k = key_ch[base + t];
            const ItemB it = item_unpack_b(k);
            s_it[t] = item_X(k) | (u32)bsr(it.rank) << 8; s_run[t] = it.run;
        }
        __syncthreads();
        for (u32 i = 0; i < n; ++i) {
            const u32 v = s_it[i];
            if ((v & 0xffu) == t) { hist[base + i] = (u16)(rh | nh << 8); rh = v >> 8; nh = run_hist_next(nh, s_run[i]); }
        }
        __syncthreads();
    }
}

// The adaptive coder's fact for the segment plan (dc_segment_plan.h): the longest mixer chain of every sub-block, exactly, before any
// sort or partition — the chains of a sub-block are its decisions by mixer id, so the longest is the maximum of their histogram.
// dc_mix_hist_kernel's shape: a workgroup per sub-block, its runs through LDS in tiles of WG; the thread that owns a run's symbol carries
// rank_hist and the unclamped run_hist and leaves them beside the run, then the thread that owns the run builds the item
// dc_sub_dec_kernel builds (ge32: behind dc_avg_kernel, and behind the exact resolve where that is on) and counts the mixer id of each
// of its decisions in an LDS histogram.  No global atomics, no scratch.  sub_mix[s] means something only where sub_und[s] == 0.
constexpr int MX_HIST = 1 << MIX_BITS;                                // counters of the histogram (NUM_MIX of them used): 8 KB
__global__ __launch_bounds__(WG) void dc_mix_facts_kernel(const u8* __restrict__ sym, const u8* __restrict__ rank, const u32* __restrict__ start,
                                                          const u8* __restrict__ ge32, u32 m, DcSubTab S, u32* __restrict__ sub_mix)
{
    typedef DcForm<DcSubTab> F;
    static_assert(WG == 256 && NUM_MIX <= MX_HIST, "a thread per symbol");
    __shared__ u32 s_it[WG], s_run[WG], s_hist[WG], s_cnt[MX_HIST], s_max[WAVES];
    const u32 s = blockIdx.x, t = threadIdx.x;
    for (u32 x = t; x < (u32)MX_HIST; x += WG) s_cnt[x] = 0u;
    const u32 r0 = S.run[s], r1 = S.run[s + 1] < m ? S.run[s + 1] : m;
    u32 rh = 0, nh = 0;
    for (u32 base = r0; base < r1; base += WG) {
        const u32 n = r1 - base < (u32)WG ? r1 - base : (u32)WG;
        u64 k = 0;
        if (t < n) {
            k = F::item(S, sym, rank, start, ge32, base + t, m, 0u);
            const ItemB it = item_unpack_b(k);
            s_it[t] = item_X(k) | (u32)bsr(it.rank) << 8; s_run[t] = it.run;
        }
        __syncthreads();
        for (u32 i = 0; i < n; ++i) {
            const u32 v = s_it[i];
            if ((v & 0xffu) == t) { s_hist[i] = rh | nh << 8; rh = v >> 8; nh = run_hist_next(nh, s_run[i]); }
        }
        __syncthreads();
        if (t < n) {
            const ItemB it = item_unpack_b(k);
            const int maxr = (int)it.maxr, c = (int)item_X(k);
            const int n_rank = count_rank_side(it, maxr), nd = n_rank + count_run_side(it);
            const u32 h = s_hist[t];
            for (int q = 0; q < nd; ++q) {
                const u32 id = (u32)nth_mixer(it, maxr, n_rank, q, c, (int)(h & 0xffu), (int)(h >> 8));
                atomicAdd(&s_cnt[id & (u32)(MX_HIST - 1)], 1u);
            }
        }
        __syncthreads();
    }
    __syncthreads();
    u32 mx = 0;
    for (u32 x = t; x < (u32)MX_HIST; x += WG) mx = s_cnt[x] > mx ? s_cnt[x] : mx;
    for (int o = 32; o > 0; o >>= 1) { const u32 y = (u32)__shfl_xor((int)mx, o, 64); mx = y > mx ? y : mx; }
    if ((t & 63u) == 0u) s_max[t >> 6] = mx;
    __syncthreads();
    if (t == 0) { for (u32 w = 1; w < (u32)WAVES; ++w) mx = s_max[w] > mx ? s_max[w] : mx; sub_mix[s] = mx; }
}

__global__ __launch_bounds__(WG) void dc_mix_key_kernel(const u64* __restrict__ key_ch, const u32* __restrict__ doff_sp, const u16* __restrict__ hist,
                                                        u32 m, u32 D, u64* __restrict__ key, u16* __restrict__ dbg_id)
{
    const u32 j = blockIdx.x * WG + threadIdx.x;
    if (j >= m) return;
    const u64 k = key_ch[j];
    const ItemB it = item_unpack_b(k);
    const int maxr = (int)it.maxr, c = (int)item_X(k);
    const int n_rank = count_rank_side(it, maxr), nd = n_rank + count_run_side(it);
    const u32 b = doff_sp[j], h = hist[j];
    if ((u64)b + (u32)nd > (u64)D) return;                            // (never: the offsets are sums of the same counts)
    for (int q = 0; q < nd; ++q) {
        const u32 id = (u32)nth_mixer(it, maxr, n_rank, q, c, (int)(h & 0xffu), (int)(h >> 8));
        key[b + q] = (u64)(it.sb << MIX_BITS | id) << 32 | (u64)(b + (u32)q);
        dbg_id[b + q] = (u16)id;
    }
}

// record of a decision in chain-major order: [12:0] state, [25:13] char, [38:26] static counter value, [39] coded bit, [40] run start
constexpr int MX_PF = 8;                                              // records a lane has in flight ahead of the step that uses them
__global__ __launch_bounds__(WG) void dc_mix_gather_kernel(const u64* __restrict__ key, u32 D, const u16* __restrict__ dbg, const u16* __restrict__ ps,
                                                           u64* __restrict__ rec, u32* __restrict__ tmp_start, u32* __restrict__ tmp_len, u32* __restrict__ meta)
{
    const u32 i = blockIdx.x * WG + threadIdx.x;
    if (i >= D) return;
    const u64 k = key[i];
    const u32 ck = (u32)(k >> 32), pos = (u32)k < D ? (u32)k : 0u;     // (never clipped: the keys are a permutation of [0, D))
    const u32 e = ps[pos];
    rec[i] = (u64)(dbg[pos] & 0x1fffu) | (u64)(dbg[(size_t)D + pos] & 0x1fffu) << 13 | (u64)(dbg[2 * (size_t)D + pos] & 0x1fffu) << 26
           | (u64)((e >> 12) & 3u) << 39;
    if (i + 1 < D && (u32)(key[i + 1] >> 32) == ck) return;
    u32 lo = 0, hi = i;                                               // the first decision of the chain that ends here
    while (lo < hi) { const u32 mid = (lo + hi) >> 1; if ((u32)(key[mid] >> 32) < ck) lo = mid + 1; else hi = mid; }
    const u32 len = i + 1 - lo;
    const u32 slot = atomicAdd(&meta[MX_CHAINS], 1u);
    tmp_start[slot] = lo; tmp_len[slot] = len;
    atomicAdd(&meta[MX_CNT + bsr(len)], 1u);
    atomicMax(&meta[MX_LONGEST], len);
}
__global__ void dc_mix_offsets_kernel(u32* __restrict__ meta)
{
    if (threadIdx.x != 0) return;
    u32 off = 0;
    for (int b = 31; b >= 0; --b) { meta[MX_OFF + b] = off; off += meta[MX_CNT + b]; }
}
__global__ __launch_bounds__(WG) void dc_mix_place_kernel(const u32* __restrict__ tmp_start, const u32* __restrict__ tmp_len, u32 nchains, u32* __restrict__ meta,
                                                          u32* __restrict__ chain_start, u32* __restrict__ chain_len)
{
    const u32 q = blockIdx.x * WG + threadIdx.x;
    if (q >= nchains) return;
    const u32 len = tmp_len[q], b = (u32)bsr(len);
    const u32 slot = meta[MX_OFF + b] + atomicAdd(&meta[MX_FILL + b], 1u);
    if (slot >= nchains) return;                                      // (never: the offsets are sums of the same counts)
    chain_start[slot] = tmp_start[q]; chain_len[slot] = len;
}

// A lane's step waits for nothing but its own previous step, and a wavefront's memory instructions touch 64 lines each (every lane is in
// a chain of its own), so they are kept few: the records of the next MX_PF steps are requested before the current MX_PF are walked, two
// records per load, and the probabilities of MX_PF steps leave as two 16-byte stores in chain-major order (pout, 4 bytes per decision);
// dc_mix_scatter_kernel, a thread per decision, then puts every entry at its stream position.  (One step ahead with a store per step,
// the walk ran at about 1.3 us per step, a load's latency; with eight steps ahead but two loads and a store per step, at 0.7 - 0.9 us.)
struct __attribute__((packed, aligned(4))) DcMixRec2 { u64 a, b; };
struct __attribute__((packed, aligned(4))) DcMixOut4 { u32 a, b, c, d; };
__global__ __launch_bounds__(WG) void dc_mix_walk_kernel(const u64* __restrict__ key, const u64* __restrict__ rec, u32 D,
                                                         const u32* __restrict__ chain_start, const u32* __restrict__ chain_len, u32 nchains,
                                                         const short* __restrict__ tab, const MixParams* __restrict__ mixp, u32* __restrict__ pout)
{
    static_assert(MX_PF == 8, "two records per load, four probabilities per store");
    __shared__ short s_stretch[MX_TAB], s_squash[MX_TAB];
    __shared__ short s_map[WG * MX_MAP_STRIDE];
    for (u32 x = threadIdx.x; x < (u32)MX_TAB; x += WG) { s_stretch[x] = tab[x]; s_squash[x] = tab[MX_TAB + x]; }
    __syncthreads();
    const u32 q = blockIdx.x * WG + threadIdx.x;
    if (q >= nchains) return;
    const u32 lo = chain_start[q];
    u32 len = chain_len[q];
    if (lo >= D || len == 0u) return;
    if (len > D - lo) len = D - lo;                                   // (never: a chain lies inside the pass)
    // (records are read up to 2 MX_PF - 1 past the chain's last, inside the buffer's slack behind D, and not used)
    u64 rc[MX_PF], rn[MX_PF];
    auto fetch = [&](u32 at, u64* r) {
#pragma unroll
        for (int x = 0; x < MX_PF; x += 2) { const DcMixRec2 v = *reinterpret_cast<const DcMixRec2*>(rec + at + x); r[x] = v.a; r[x + 1] = v.b; }
    };
    fetch(lo, rc);
    const MixParams P = mixp[mixer_class((int)((u32)(key[lo] >> 32) & ((1u << MIX_BITS) - 1u)))];
    short* map = s_map + threadIdx.x * MX_MAP_STRIDE;
    int32_t w0 = 2048 << 5, w1 = 2048 << 5, w2 = 0;
    for (int p = 0; p < 17; ++p) map[p] = s_squash[2048 + (p - 8) * 256];
    for (u32 i = 0; i < len; i += MX_PF) {
        fetch(lo + i + MX_PF, rn);
        u32 out[MX_PF];
#pragma unroll
        for (int x = 0; x < MX_PF; ++x) {
            const u64 r = rc[x];
            out[x] = 0;
            if (i + (u32)x < len)
                out[x] = (u32)mixer_step_on(w0, w1, w2, map, P, (const short*)s_stretch, (const short*)s_squash, (int)((u32)(r >> 13) & 0x1fffu), (int)((u32)r & 0x1fffu),
                                            (int)((u32)(r >> 26) & 0x1fffu), (u32)(r >> 39) & 1u);
        }
        u32* o = pout + lo + i;
        if (i + MX_PF <= len) {
            *reinterpret_cast<DcMixOut4*>(o) = DcMixOut4{out[0], out[1], out[2], out[3]};
            *reinterpret_cast<DcMixOut4*>(o + 4) = DcMixOut4{out[4], out[5], out[6], out[7]};
        } else {
#pragma unroll
            for (int x = 0; x < MX_PF; ++x) if (i + (u32)x < len) o[x] = out[x];
        }
#pragma unroll
        for (int x = 0; x < MX_PF; ++x) rc[x] = rn[x];
    }
}
// thread per decision in chain-major order: the mixed probability with the record's bit and run-start mark, to its stream position
__global__ __launch_bounds__(WG) void dc_mix_scatter_kernel(const u64* __restrict__ key, const u64* __restrict__ rec, const u32* __restrict__ pout, u32 D, u16* __restrict__ ps)
{
    const u32 i = blockIdx.x * WG + threadIdx.x;
    if (i >= D) return;
    const u32 pos = (u32)key[i];
    if (pos < D) ps[pos] = (u16)((pout[i] & 0xfffu) | ((u32)(rec[i] >> 39) & 3u) << 12);
}

// The adaptive stage's buffers and tables, on the first -e2 pass; false: they do not fit (the pass is declined, reason 0).
static bool devcoder_mix_ensure(bscgpu_ctx* c, DevCoder* d)
{
    if (d->mix_arena.base || d->mix_arena.failed) return !d->mix_arena.failed;
    CtxTimer tm("devcoder_mix_ensure (adaptive model: keys, planes, tables)");
    const size_t D = d->Dcap + 64;
    const Carve carve[] = {
        {(void**)&d->mix_key[0], 8 * D + 65536}, {(void**)&d->mix_key[1], 8 * D + 65536}, {(void**)&d->mix_dbg, 8 * D},
        {(void**)&d->mix_meta, MX_WORDS * 4}, {(void**)&d->mix_tab, 2 * MX_TAB * sizeof(short)}, {(void**)&d->mix_mp, NUM_CLS * sizeof(MixParams)},
        {(void**)&d->mp_adapt, sizeof(ModelParams)},
    };
    if (!dc_arena_alloc(d->mix_arena, carve, "BSC_DC_MIX_FAIL_ALLOC")) return false;
    static const ModelParams mpa = [] { ModelParams m; model_params_adaptive(bschost::qlfc_adaptive_params(), m); return m; }();
    const bschost::QlfcTables& QT = bschost::qlfc_tables();
    std::vector<short> tab(2 * MX_TAB, 0);
    memcpy(tab.data(), QT.stretch, sizeof QT.stretch); memcpy(tab.data() + MX_TAB, QT.squash, sizeof QT.squash);
    MixParams mixp[NUM_CLS];
    mix_params_from_table(bschost::qlfc_adaptive_params(), mixp);
    const bool ok = hipMemcpyAsync(d->mp_adapt, &mpa, sizeof mpa, hipMemcpyHostToDevice, c->stream) == hipSuccess
                 && hipMemcpyAsync(d->mix_tab, tab.data(), tab.size() * sizeof(short), hipMemcpyHostToDevice, c->stream) == hipSuccess
                 && hipMemcpyAsync(d->mix_mp, mixp, sizeof mixp, hipMemcpyHostToDevice, c->stream) == hipSuccess
                 && ctx_sync(c) == hipSuccess;                        // (stack objects: the copies must have finished)
    if (!ok) { (void)hipGetLastError(); (void)hipFree(d->mix_arena.base); d->mix_arena.base = nullptr; d->mix_arena.bytes = 0; d->mix_arena.failed = true; }
    return ok;
}

// Behind dc_static_run with the adaptive rates and the debug planes (D decisions in ps, their counter values in mix_dbg): the
// mixers.  One sync of its own: the chains' number and the longest of them.  expect_longest >= 0 (a segment): what the plan's facts
// say the longest chain is — the chain table must agree, as the families' totals must with the plan's decisions.
static int dc_mix_run(bscgpu_ctx* c, DevCoder* d, const DcSubTab& S, u32 m, u32 D, u16* ps, int64_t expect_longest = -1)
{
    static_assert(HM_MIX + 2 <= HM_WORDS && sizeof(short) == 2, "hmeta holds the two words");
    if (D == 0) return BSC_NO_ERROR;
    u16* const hist = reinterpret_cast<u16*>(d->inv_sr);              // dead behind the stream kernel, as pos[0..3] below
    u32 *tmp_start = d->pos[0], *tmp_len = d->pos[1], *chain_start = d->pos[2], *chain_len = d->pos[3];
    u32* pout = d->pos[0];                                            // (the walk's output, behind the placement's last read of tmp_start)
    HIP_TRY(c, hipMemsetAsync(d->mix_meta, 0, MX_WORDS * 4, c->stream));
    prof_begin(c, BSCGPU_K_DC_EVAL, (u64)m * 10 + (u64)D * 10, D);
    hipLaunchKernelGGL(dc_mix_hist_kernel, dim3(S.nsub), dim3(WG), 0, c->stream, d->key_ch, S, hist);
    hipLaunchKernelGGL(dc_mix_key_kernel, dim3((m + WG - 1) / WG), dim3(WG), 0, c->stream, d->key_ch, d->doff[0], hist, m, D, d->mix_key[0], d->mix_dbg + 3 * (size_t)D);
    prof_end(c);
    HIP_TRY(c, hipGetLastError());
    // (b) the sub-block bits that are set at all and the mixer id: two or three 8-bit passes
    int sbits = 0;
    while ((1u << sbits) < S.nsub) ++sbits;
    const int kbits = MIX_BITS + sbits, npass = (kbits + 7) / 8;
    RadixPass passes[3];
    for (int p = 0; p < npass; ++p) { passes[p].shift = 32 + 8 * p; passes[p].bits = kbits - 8 * p < 8 ? kbits - 8 * p : 8; }
    int in_alt = 0;
    int rc = radix_sort_passes(c, d->mix_key[0], d->mix_key[1], nullptr, nullptr, D, passes, npass, &in_alt, nullptr, /* aux */ true);
    if (rc < 0) return rc;
    const u64* key = d->mix_key[in_alt];
    u64* rec = d->mix_key[in_alt ^ 1];                                // (the sort's other buffer: dead behind its last pass)
    prof_begin(c, BSCGPU_K_DC_EVAL, (u64)D * 26, D);
    hipLaunchKernelGGL(dc_mix_gather_kernel, dim3((D + WG - 1) / WG), dim3(WG), 0, c->stream, key, D, d->mix_dbg, ps, rec, tmp_start, tmp_len, d->mix_meta);
    hipLaunchKernelGGL(dc_mix_offsets_kernel, dim3(1), dim3(64), 0, c->stream, d->mix_meta);
    prof_end(c);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(d->hmeta + HM_MIX, d->mix_meta + MX_CHAINS, 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, ctx_sync(c));
    prof_collect(c);
    const u32 nchains = d->hmeta[HM_MIX], longest = d->hmeta[HM_MIX + 1];
    c->dc_mix_chains = nchains; c->dc_mix_longest = longest;
    if (nchains == 0 || nchains > D) return ctx_fail(c, BSC_GPU_ERROR, "device coder (adaptive): chain table", hipSuccess);
    if (expect_longest >= 0 && (int64_t)longest != expect_longest)
        return ctx_fail(c, BSC_GPU_ERROR, "device coder (adaptive): a segment's longest chain differs from the plan's", hipSuccess);
    if (longest > c->dc_mix_cap) { c->dc_note.fail |= (int)FAIL_MIX; return BSC_NOT_SUPPORTED; }
    const auto walk_t0 = std::chrono::steady_clock::now();             // (the stream is idle: the sync above)
    prof_begin(c, BSCGPU_K_DC_EVAL, (u64)D * 18, D);
    hipLaunchKernelGGL(dc_mix_place_kernel, dim3((nchains + WG - 1) / WG), dim3(WG), 0, c->stream, tmp_start, tmp_len, nchains, d->mix_meta, chain_start, chain_len);
    hipLaunchKernelGGL(dc_mix_walk_kernel, dim3((nchains + WG - 1) / WG), dim3(WG), 0, c->stream, key, rec, D, chain_start, chain_len, nchains,
                       d->mix_tab, d->mix_mp, pout);
    hipLaunchKernelGGL(dc_mix_scatter_kernel, dim3((D + WG - 1) / WG), dim3(WG), 0, c->stream, key, rec, pout, D, ps);
    prof_end(c);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, ctx_sync(c));
    c->dc_mix_walk_us = (u32)std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - walk_t0).count();
    prof_collect(c);
    if (getenv("BSCGPU_DEBUG")) fprintf(stderr, "[devcoder adaptive] decisions %u, chains %u, longest %u\n", D, nchains, longest);
    return BSC_NO_ERROR;
}
const u16* devcoder_mix_dbg_ptr(const bscgpu_ctx* c) { return c->dc ? c->dc->mix_dbg : nullptr; }

// Probability stream of a whole pass, coder 1 (dc_static_run), 2 (dc_static_run with the adaptive rates, then dc_mix_run) or 3
// (dc_fast_run) -> every sub-block's entries back to back in stream
// order in the device p stream (buffer 0), poff[0..nsub] in d->poff_tab.  The same stages, the same kernels as a single block's,
// instantiated for the table (DcSubTab); every guarded exit keeps its meaning with the PASS as the unit: a raised flag declines the
// whole pass (BSC_NOT_SUPPORTED, c->dc_note.fail says why).  The arena of devcoder_batch_ensure serves both coders (the fast one uses
// one esub plane of its four, and max_rank 7 for every sub-block).
// packed_out non-null (coder 1 only): the caller can take the stream at 13 bits per decision (DcP13Tab); *packed_out says whether that
// is what lies in the buffer — pbase[0..nsub] in d->pbase_tab, its end in *pbytes_out as bytes — or the 2-byte form after all (void).
int devcoder_pstream_batch(bscgpu_ctx* c, u32 m, int nsub, int coder, u32* D_out, int* packed_out, int64_t* pbytes_out)
{
    if (packed_out) *packed_out = 0;
    DcPass P;
    int rc = dc_pass_begin(c, m, nsub, (int)FAIL_CAP, &P);
    if (rc < 0) return rc;
    DevCoder* d = P.d;
    const bool fast = coder == 3;                                      // LIBBSC_CODER_QLFC_FAST
    const bool adaptive = coder == 2;                                  // LIBBSC_CODER_QLFC_ADAPTIVE
    if (adaptive && !devcoder_mix_ensure(c, d)) return BSC_NOT_SUPPORTED;   // does not fit: declined, no reason bit (as the batch arena)
    rc = dc_unit_clear(c, d, !fast);
    if (rc < 0) return rc;
    prof_begin(c, BSCGPU_K_DC_CTX, (u64)m * (fast ? 14 : 40), m);
    rc = dc_pass_tables(c, P, m, fast, nullptr);
    prof_end(c);
    if (rc < 0) return rc;
    DcUnit U = dc_pass_range(P, 0u, m, 0, -1);
    DcOut O;
    O.take_packed = coder == 1 && packed_out != nullptr;
    if (adaptive) { U.mp = d->mp_adapt; O.dbg = d->mix_dbg; }
    rc = fast ? dc_fast_run(c, d, P.S, U, O) : dc_static_run(c, d, P.S, U, O);
    if (rc < 0) return rc;
    if (adaptive) {
        rc = dc_mix_run(c, d, P.S, m, O.D, d->ps[0]);
        if (rc < 0) return rc;
    }
    *D_out = O.D;
    if (packed_out) *packed_out = O.packed ? 1 : 0;
    if (O.packed && pbytes_out) *pbytes_out = (int64_t)d->hmeta[HM_PBASE_END] / 8 * 13;
    return rc;
}
const u32* devcoder_batch_poff_ptr(const bscgpu_ctx* c) { return c->dc ? c->dc->poff_tab : nullptr; }
const u32* devcoder_batch_pbase_ptr(const bscgpu_ctx* c) { return c->dc ? c->dc->pbase_tab : nullptr; }

// ---- a pass in model segments ("Model segments") --------------------------------------------------------------------
// Sub-blocks are independent chains by construction (the chain identity carries the sub-block), so the model of a pass can run over
// any contiguous range of its sub-blocks and write the same entries.  Facts first, once per pass and before any sort: every
// sub-block's undecided avg_rank flags (dc_avg_kernel) and its decisions for this coder (dc_sub_dec_kernel).  The plan
// (dc_segment_plan.h: dc_segment_plan) excludes a block with an undecided flag or more decisions than the arena holds and cuts the rest into
// segments of at most min(Dcap, target) decisions; each segment then is a small pass of its own to dc_static_run / dc_fast_run (its
// rebased run table: dc_seg_tab_kernel).  The device stream is double-buffered over ps[0 / 1]: segment k + 1 is modelled while
// segment k's entries leave on the copy stream.  A segment that declines while it runs (FAIL_HIST, FAIL_REPLAY) is split at the block
// boundary nearest half its decisions and both halves run again, depth first; a single block that declines is marked with the reason.
// out / cap: where the kept entries go back to back (host); per_segment_fit: a segment that no longer fits behind the ones before
// it is left to the host (FAIL_CAP) — else a total above cap is counted, not copied.
// coder 2 (the adaptive coder): a third fact, the longest mixer chain of every sub-block (dc_mix_facts_kernel), lets the plan leave out
// a block whose chain exceeds the context's step cap (FAIL_MIX, per BLOCK on this route) before anything runs; every segment is
// dc_static_run with the adaptive rates and dc_mix_run over the same rebased table, into the segment's ps buffer.  A segment's chain
// table must report the longest chain its facts promise (BSC_GPU_ERROR otherwise), so FAIL_MIX cannot arise while a segment runs.
// pbase non-null (coder 1 only): the packed form (DcP13Tab).  out / cap are BYTES then; every kept segment's packed stream lands behind
// the one before it (a segment's bytes are a whole number of 104-byte sub-block extents), pbase[0..nsub] runs on across the segments in
// kept order and a sub-block that was not modelled has pbase[s + 1] == pbase[s].  A segment's bytes are known with the plan
// (sub_dec rounded up to 64 per sub-block), so "fits" is tested before it runs.  A segment whose packed form is void (DM_P13_OVER)
// has been re-launched in the 2-byte form by dc_static_run: its entries come down to a scratch vector and dc_pack13_host
// packs them into place — the caller sees one form, the blocks keep the device's model; counted in cnt_packed_void.
// Every decision of the above that is arithmetic — what runs next, whether it fits, where a declined range is cut and when it is
// given up, where kept entries land, poff / pbase — is DcSegSchedule's (dc_segment_plan.h); the driver below launches, copies and tells.
// the facts of a pass (after qlfc_front_batch): dec[s] / und[s] of every sub-block on the host; ge32 and sub_maxr stay for the segments
// note non-null: its avg_und and avg_resolved are the pass's — the flags the bracket left open, and what the exact resolve settled of them
// mix non-null (the adaptive coder; dec and und are the static coder's: same decisions, same flags): the longest mixer chain of every
// sub-block (dc_mix_facts_kernel), down in the same sync
static int dc_segment_facts(bscgpu_ctx* c, const DcPass& P, u32 m, bool fast, u32* dec, u32* und, DcNote* note = nullptr, u32* mix = nullptr)
{
    DevCoder* d = P.d;
    const int nsub = (int)P.S.nsub;
    const int crc = dc_unit_clear(c, d, /* kinds_seen: no model runs here */ false);
    if (crc < 0) return crc;
    HIP_TRY(c, hipMemsetAsync(d->sub_und, 0, (size_t)nsub * 4, c->stream));
    HIP_TRY(c, hipMemsetAsync(d->sub_dec, 0, (size_t)nsub * 4, c->stream));
    prof_begin(c, BSCGPU_K_DC_FACTS, (u64)m * 6, m);
    const int arc = dc_pass_tables(c, P, m, fast, d->sub_und);             // (with the exact resolve: what is left behind it)
    if (arc < 0) { prof_end(c); return arc; }
    hipLaunchKernelGGL(dc_sub_dec_kernel, dim3((m + WG - 1) / WG), dim3(WG), 0, c->stream, P.dsym, P.drank, P.dstart, d->ge32, m, P.S, d->sub_dec);
    prof_end(c);
    if (mix) {
        prof_begin(c, BSCGPU_K_DC_FACTS, (u64)m * 10, m);
        hipLaunchKernelGGL(dc_mix_facts_kernel, dim3((u32)nsub), dim3(WG), 0, c->stream, P.dsym, P.drank, P.dstart, d->ge32, m, P.S, d->sub_mix);
        prof_end(c);
        HIP_TRY(c, hipMemcpyAsync(mix, d->sub_mix, (size_t)nsub * 4, hipMemcpyDeviceToHost, c->stream));
    }
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(und, d->sub_und, (size_t)nsub * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(dec, d->sub_dec, (size_t)nsub * 4, hipMemcpyDeviceToHost, c->stream));
    // (behind the exact resolve und[] is what it left: what the bracket had left open, and what was settled, are meta words)
    if (c->dc_avg_exact && note) HIP_TRY(c, hipMemcpyAsync(d->hmeta, d->meta, DM_COUNT * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, ctx_sync(c));
    prof_collect(c);
    if (note && c->dc_avg_exact) { note->avg_und = (int)d->hmeta[DM_AVG_UND]; note->avg_resolved = (int)d->hmeta[DM_AVG_RESOLVED]; }
    else if (note) {
        int64_t und_total = 0;
        for (int s = 0; s < nsub; ++s) und_total += und[s];
        note->avg_und = (int)und_total; note->avg_resolved = 0;
    }
    return BSC_NO_ERROR;
}
int devcoder_segment_facts(bscgpu_ctx* c, u32 m, int nsub, int coder, u32* dec, u32* und, u32* mix)
{
    if ((coder == 2) != (mix != nullptr)) return BSC_BAD_PARAMETER;
    DcPass P;
    const int rc = dc_pass_begin(c, m, nsub, -1, &P);
    if (rc < 0) return rc;
    return dc_segment_facts(c, P, m, coder == 3, dec, und, nullptr, mix);
}

// The copy-outs of kept segments in flight on the copy stream, oldest first: at most one per ps buffer, its end marked by seg_ev[k].
struct DcCopyRing {
    hipEvent_t* ev; hipStream_t copy_stream; const DcSegNote* note;
    struct Pend { int b0, b1, k; };
    std::deque<Pend> pend;
    void settle(const DcSegRange& g) const { if (note) note->settled(note->user, g.b0, g.b1); }
    // a copy out of ps[k] with the entries of range g has been queued on the copy stream
    hipError_t started(int k, const DcSegRange& g)
    {
        const hipError_t e = hipEventRecord(ev[k], copy_stream);
        if (e == hipSuccess) pend.push_back(Pend{g.b0, g.b1, k});
        return e;
    }
    // tell what has landed: the copies up to the one out of buffer `upto` (0 / 1) or all of them (2) are waited for, the ones behind
    // them are told if they are found landed; nothing is told out of order
    hipError_t landed(int upto)
    {
        int must = 0;                                                  // how many of the oldest to wait for
        for (size_t k = 0; k < pend.size(); ++k) if (upto == 2 || pend[k].k == upto) must = (int)k + 1;
        while (!pend.empty()) {
            const Pend q = pend.front();
            if (must <= 0 && hipEventQuery(ev[q.k]) != hipSuccess) break;
            const hipError_t e = hipEventSynchronize(ev[q.k]);
            if (e != hipSuccess) return e;
            pend.pop_front(); --must;
            if (note) note->settled(note->user, q.b0, q.b1);
        }
        return hipSuccess;
    }
};

// The ranges of the schedule one after the other, launch by launch; out: the landing buffer (host), 2-byte entries or the packed
// form's bytes (pk).  sum: what the kept and the declined runs counted together (replays, hist_ext and what the two resolves settled).
// sub_mix non-null: the adaptive coder — dc_static_run with its rates and the debug planes, then the mixers over the same table (the
// sub-block ids in the mixer key are the segment's own: chains never cross a segment, which is made of whole sub-blocks); mixsum: the
// chains (sum), the longest (maximum) and the walk's microseconds (sum) of the kept segments.
struct DcMixSum { u64 chains = 0; u32 longest = 0; u64 walk_us = 0; };
static int dc_segments_loop(bscgpu_ctx* c, const DcPass& P, bool fast, bool pk, const u32* sub_run, DcSegSchedule& sch, DcCopyRing& ring, u8* out,
                            DcNote& sum, const u32* sub_mix = nullptr, DcMixSum* mixsum = nullptr)
{
    DevCoder* d = P.d;
    std::vector<u32> pseg((size_t)P.S.nsub + 1), pbseg(pk ? (size_t)P.S.nsub + 1 : 0);
    std::vector<u16> void_entries;                                    // (packed: the 2-byte entries of a void segment on their way to the host's packer)
    std::vector<int64_t> void_pbase;
    int launched = 0;
    DcSegRange g;
    for (DcSegNext nx; (nx = sch.next(&g)) != DC_SEG_DONE; ) {
        if (nx == DC_SEG_GIVEN_UP) { ring.settle(g); continue; }
        const int s0 = g.s0, s1 = g.s1;
        const u32 r0 = sub_run[s0], r1 = sub_run[s1];
        const int psbuf = launched++ & 1;
        int rc = dc_unit_clear(c, d, !fast);
        if (rc < 0) return rc;
        prof_begin(c, BSCGPU_K_DC_FACTS, (u64)(s1 - s0) * 8, (u64)(s1 - s0));
        hipLaunchKernelGGL(dc_seg_tab_kernel, dim3(((u32)(s1 - s0) + 1 + WG - 1) / WG), dim3(WG), 0, c->stream, P.T.sub_run, (u32)s0, (u32)(s1 - s0), r0, r1, d->seg_run);
        prof_end(c);
        HIP_TRY(c, hipStreamWaitEvent(c->stream, d->seg_ev[psbuf], 0));          // this buffer's copy-out of two segments ago
        // (the segment's rebased table; its runs as a unit)
        DcSubTab G; G.nsub = (u32)(s1 - s0); G.run = d->seg_run; G.off = P.T.sub_off + s0; G.base = P.T.sub_base + s0; G.maxr = d->sub_maxr + s0;
        DcUnit U = dc_pass_range(P, r0, r1, psbuf, g.expect);
        DcOut O;
        O.take_packed = pk; O.poff_host = pseg.data(); O.pbase_host = pk ? pbseg.data() : nullptr;
        if (sub_mix) { U.mp = d->mp_adapt; O.dbg = d->mix_dbg; }
        rc = fast ? dc_fast_run(c, d, G, U, O) : dc_static_run(c, d, G, U, O);
        if (sub_mix && rc >= 0) {
            u32 longest = 0;
            for (int s = s0; s < s1; ++s) longest = sub_mix[s] > longest ? sub_mix[s] : longest;
            rc = dc_mix_run(c, d, G, r1 - r0, O.D, d->ps[psbuf & 1], (int64_t)longest);
            if (rc >= 0 && mixsum && O.D > 0) { mixsum->chains += c->dc_mix_chains; mixsum->longest = c->dc_mix_longest > mixsum->longest ? c->dc_mix_longest : mixsum->longest; mixsum->walk_us += c->dc_mix_walk_us; }
        }
        const DcNote& run = c->dc_note;
        sum.replays += run.replays; sum.hist_ext += run.hist_ext; sum.replay_resolved += run.replay_resolved; sum.hist_resolved += run.hist_resolved;
        if (rc == BSC_NOT_SUPPORTED) { if (sch.declined(g, run.fail)) ring.settle(g); continue; }
        if (rc < 0) return rc;
        const u32 D = O.D;
        // this buffer's earlier copy-out has landed (the stream kernel waited for it), maybe the other one's too
        HIP_TRY(c, ring.landed(psbuf));
        const int64_t at = sch.kept(g, D, pseg.data(), O.packed ? pbseg.data() : nullptr, O.packed);
        if (at < 0) return ctx_fail(c, BSC_GPU_ERROR, "device coder: a segment's packed layout differs from the plan's", hipSuccess);
        if (!sch.copy_all() || D == 0) ring.settle(g);
        else if (pk && !O.packed) {
            // void: the 2-byte form lies in ps[psbuf] (dc_static_run re-launched it); down, and packed into place on the host
            void_entries.resize((size_t)D); void_pbase.resize((size_t)(s1 - s0) + 1);
            HIP_TRY(c, hipMemcpyAsync(void_entries.data(), d->ps[psbuf], (size_t)D * 2, hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(c, ctx_sync(c));
            if (dc_pack13_host(void_entries.data(), pseg.data(), s1 - s0, out + at, g.need, void_pbase.data()) != g.need)
                return ctx_fail(c, BSC_GPU_ERROR, "device coder: packing a void segment", hipSuccess);
            ring.settle(g);
        } else {
            HIP_TRY(c, hipMemcpyAsync(out + (pk ? at : 2 * at), d->ps[psbuf], pk ? (size_t)g.need : (size_t)D * 2, hipMemcpyDeviceToHost, c->copy_stream));
            HIP_TRY(c, ring.started(psbuf, g));
        }
    }
    HIP_TRY(c, ring.landed(2));
    return BSC_NO_ERROR;
}

int devcoder_pstream_segments(bscgpu_ctx* c, u32 m, int nsub, const int* blk_sub, int count, const u32* sub_run, int coder, int64_t target,
                              void* out, int64_t cap, bool per_segment_fit, u32* poff, int* blk_state, int64_t* D_out, const DcSegNote* note,
                              int64_t* pbase)
{
    const bool pk = pbase != nullptr;
    if (pk && coder != 1) return BSC_BAD_PARAMETER;
    DcPass P;
    int rc = dc_pass_begin(c, m, nsub, 0, &P);
    if (rc < 0) return rc;
    DevCoder* d = P.d;
    for (int k = 0; k < 2; ++k)
        if (!d->seg_ev[k]) HIP_TRY(c, hipEventCreateWithFlags(&d->seg_ev[k], hipEventDisableTiming));
    const bool fast = coder == 3;                                      // LIBBSC_CODER_QLFC_FAST
    const bool adaptive = coder == 2;                                  // LIBBSC_CODER_QLFC_ADAPTIVE
    if (adaptive && !devcoder_mix_ensure(c, d)) return BSC_NOT_SUPPORTED;   // does not fit: declined, no reason bit (as the whole-pass stage)

    std::vector<u32> und((size_t)nsub), dec((size_t)nsub), mix(adaptive ? (size_t)nsub : 0);
    DcNote sum;                                                        // the pass's: avg values from the facts, the rest summed over its segments
    rc = dc_segment_facts(c, P, m, fast, dec.data(), und.data(), &sum, adaptive ? mix.data() : nullptr);
    if (rc < 0) return rc;

    // (the adaptive coder: the step cap reads per BLOCK here — a block with a chain above it is left out, FAIL_MIX, before anything runs)
    DcSegSchedule sch(dec.data(), und.data(), blk_sub, count, nsub, (int64_t)d->Dcap, target, cap, per_segment_fit, (int)FAIL_AVG, (int)FAIL_CAP, poff, pbase, blk_state,
                      adaptive ? mix.data() : nullptr, (int64_t)c->dc_mix_cap, (int)FAIL_MIX);
    if (note) note->planned(note->user);
    DcCopyRing ring{d->seg_ev, c->copy_stream, note, {}};
    DcMixSum mixsum;
    rc = dc_segments_loop(c, P, fast, pk, sub_run, sch, ring, static_cast<u8*>(out), sum, adaptive ? mix.data() : nullptr, &mixsum);
    // (no copy into the caller's buffer may outlive the call, whichever way it ends)
    if (hipStreamSynchronize(c->copy_stream) != hipSuccess && rc >= 0) rc = ctx_fail(c, BSC_GPU_ERROR, "device coder: segment copy-out", hipSuccess);
    if (rc < 0) return rc;
    const DcSegTotals T = sch.finish();
    sum.fail = T.fail;
    c->dc_note = sum;
    if (adaptive) { c->dc_mix_chains = (u32)mixsum.chains; c->dc_mix_longest = mixsum.longest; c->dc_mix_walk_us = (u32)mixsum.walk_us; }
    c->cnt_seg += T.kept; c->cnt_seg_reruns += T.reruns; c->cnt_seg_host_blocks += T.host_blocks;
    c->cnt_packed_passes += T.kept_packed; c->cnt_packed_void += T.kept_void;
    if (getenv("BSCGPU_DEBUG")) fprintf(stderr, "[devcoder segments] sub-blocks %d, planned %d, kept %d, re-runs %d, blocks left to the host %d, decisions %lld\n", nsub, T.planned, T.kept, T.reruns, T.host_blocks, (long long)T.decisions);
    *D_out = T.decisions;
    return BSC_NO_ERROR;
}

const u16* devcoder_pstream_ptr(const bscgpu_ctx* c, int psbuf) { return c->dc ? c->dc->ps[psbuf & 1] : nullptr; }

// ---- C ABI: the stage on its own (host block in, probability stream out) ---------------------------------------------
// What a maintainer would call next to bsc_qlfc_transform-style stage functions, and what the parity tests compare with the
// oracle's trace of the reference model: sub-block split (coder.cpp:70-109), run / rank front end and the model on the GPU.
// Returns the number of decisions (their 16-bit entries are in out[0..)), BSC_NOT_SUPPORTED when the block needs the host
// model (bscgpu_last_error tells why), or another negative libbsc code.
// ... of a context with a divided arena (BSCGPU_OPT_DC_ARENA_DIV > 1): facts, plan, and the segments one after the other, each one's
// pieces copied to where the plan puts them in out — the same out, poff and pbase as the whole block's (the bytes between a sub-block's
// last group of eight and its padded extent are nobody's in either; a void segment is packed into place, where the whole block would
// have been void).  The debug planes are the whole block's only.
static int64_t qlfc_static_pstream_segments(bscgpu_ctx* c, int n, int nb, const int* sub_start, const int* sub_size, u32 m, const u32* run_first,
                                            const int* max_rank, uint16_t* out, int64_t cap, int* nblocks_out, int64_t* poff_out, bool dbg,
                                            bool want_packed, int64_t* pbase_out)
{
    if (dbg) { c->err = "the debug planes need the whole block in the arena (BSCGPU_OPT_DC_ARENA_DIV 1)"; return BSC_NOT_SUPPORTED; }
    DcBlock B;
    const FrontBufs fb = front_bufs(c);
    int rc = devcoder_block_begin(c, fb.sym, fb.rank, fb.start, m, (u32)n, nb, sub_start, sub_size,
                                  run_first, max_rank, 1, want_packed, &B);
    if (rc == BSC_NO_ERROR && want_packed && !B.packed) { c->err = "the packed stream was not produced (option off)"; return BSC_NOT_SUPPORTED; }
    std::vector<u16> void_entries;
    const bool fits = B.plan.segments() > 0 && B.plan.zone_bytes() <= (want_packed ? cap : 2 * cap);
    for (int i = 0; rc == BSC_NO_ERROR && i < B.plan.segments(); ++i) {
        const DcBlockSeg g = B.plan.segment(i);
        bool host_packed = false;
        rc = devcoder_block_segment(c, &B, g, i & 1, &host_packed);
        if (rc < 0 || !fits) continue;
        const u8* dps = reinterpret_cast<const u8*>(devcoder_pstream_ptr(c, i & 1));
        if (host_packed) {
            void_entries.resize((size_t)g.expect);
            HIP_TRY(c, hipMemcpyAsync(void_entries.data(), dps, (size_t)g.expect * 2, hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(c, ctx_sync(c));
            if (!B.plan.pack_void(g, void_entries.data(), reinterpret_cast<u8*>(out))) return ctx_fail(c, BSC_GPU_ERROR, "device coder: packing a void segment", hipSuccess);
        } else
            for (int k = 0; k < g.s1 - g.s0; ++k)
                if (g.len[k]) HIP_TRY(c, hipMemcpyAsync(reinterpret_cast<u8*>(out) + g.dst[k], dps + g.src[k], (size_t)g.len[k], hipMemcpyDeviceToHost, c->stream));
    }
    if (rc == BSC_NOT_SUPPORTED) {
        char buf[96]; snprintf(buf, sizeof buf, "device coder declined the block (reason mask %d)", c->dc_note.fail);
        c->err = buf;
    }
    HIP_TRY(c, ctx_sync(c));                                           // (no copy into the caller's buffer outlives the call)
    prof_collect(c);
    if (rc < 0) return rc;
    *nblocks_out = nb;
    for (int b = 0; b <= nb; ++b) { poff_out[b] = B.plan.poff_of(b); if (want_packed) pbase_out[b] = B.plan.pbase_of(b); }
    return B.plan.decisions();
}
// What the stage functions below start with: the arguments they share checked, the block up into dL, its sub-block split and runs
// (qlfc_front.hip; the run arrays stay in HBM) and every sub-block's max_rank.
struct StageFront { int nb = 0; u32 m = 0, run_first[9] = {}; int max_rank[8] = {}; };
static int qlfc_stage_front(bscgpu_ctx* c, const uint8_t* L, int n, int* nblocks_out, int* sub_start /*[8]*/, int* sub_size /*[8]*/, StageFront* F)
{
    if (!c || !L || n <= 0 || !nblocks_out || !sub_start || !sub_size) return BSC_BAD_PARAMETER;
    if (n > c->max_n) return BSC_GPU_NOT_ENOUGH_MEMORY;
    if (hipSetDevice(c->device) != hipSuccess) return BSC_GPU_ERROR;
    HIP_TRY(c, hipMemcpyAsync(c->dL, L, (size_t)n, hipMemcpyHostToDevice, c->stream));
    F->nb = bschost::coder_num_blocks(n);
    int rc = qlfc_front_split(c, c->dL, (u32)n, F->nb, sub_start, sub_size);
    if (rc < 0) return rc;
    static thread_local u32 first_run[8 * 256];
    rc = qlfc_front_runs(c, c->dL, (u32)n, F->nb, sub_start, &F->m, F->run_first, first_run, c->slots[0]);
    if (rc < 0) return rc;
    dc_max_rank_table(first_run, F->nb, F->max_rank);
    return BSC_NO_ERROR;
}
static int64_t qlfc_static_pstream_stage(bscgpu_ctx* c, const uint8_t* L, int n, uint16_t* out, int64_t cap, int* nblocks_out,
                                         int* sub_start /*[8]*/, int* sub_size /*[8]*/, int64_t* poff_out /*[9]*/, uint16_t* dbg_out /*[3][cap] or NULL*/,
                                         bool want_packed, int64_t* pbase_out /*[9], packed only*/)
{
    if (!out || !poff_out) return BSC_BAD_PARAMETER;
    StageFront F;
    int rc = qlfc_stage_front(c, L, n, nblocks_out, sub_start, sub_size, &F);
    if (rc < 0) return rc;
    const int nb = F.nb;
    if (c->dc_arena_div > 1)
        return qlfc_static_pstream_segments(c, n, nb, sub_start, sub_size, F.m, F.run_first, F.max_rank, out, cap, nblocks_out, poff_out, dbg_out != nullptr, want_packed, pbase_out);
    u16* ddbg = nullptr;
    if (dbg_out) { rc = devcoder_ensure(c); if (rc < 0) return rc; if (hipMalloc((void**)&ddbg, (size_t)c->dc->Dcap * 6) != hipSuccess) return BSC_GPU_NOT_ENOUGH_MEMORY; }
    u32 D = 0, poff[9];
    int packed = 0;
    const FrontBufs fb = front_bufs(c);
    rc = devcoder_pstream(c, fb.sym, fb.rank, fb.start, F.m, (u32)n, nb, F.run_first, F.max_rank, &D, poff, ddbg, 0, 1,
                          want_packed ? &packed : nullptr);
    if (rc == BSC_NO_ERROR && want_packed && !packed) { c->err = "the packed stream was not produced (option off, or a wavefront's piece beyond the staging buffer)"; rc = BSC_NOT_SUPPORTED; }
    else if (rc == BSC_NOT_SUPPORTED) {
        char buf[96]; snprintf(buf, sizeof buf, "device coder declined the block (reason mask %d)", c->dc_note.fail);
        c->err = buf;
    }
    if (rc < 0) { if (ddbg) hipFree(ddbg); return rc; }
    *nblocks_out = nb;
    const DcBlockSchedule lay = DcBlockSchedule::whole(poff, nb, want_packed);
    for (int b = 0; b <= nb; ++b) { poff_out[b] = lay.poff_of(b); if (want_packed) pbase_out[b] = lay.pbase_of(b); }
    if (want_packed) {
        if (lay.zone_bytes() <= cap) { HIP_TRY(c, hipMemcpyAsync(out, devcoder_pstream_ptr(c), (size_t)lay.zone_bytes(), hipMemcpyDeviceToHost, c->stream)); HIP_TRY(c, ctx_sync(c)); }
    } else if ((int64_t)D <= cap) {
        HIP_TRY(c, hipMemcpyAsync(out, devcoder_pstream_ptr(c), (size_t)D * 2, hipMemcpyDeviceToHost, c->stream));
        if (dbg_out) for (int f = 0; f < 3; ++f) HIP_TRY(c, hipMemcpyAsync(dbg_out + (size_t)f * cap, ddbg + (size_t)f * D, (size_t)D * 2, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, ctx_sync(c));
    }
    if (ddbg) hipFree(ddbg);
    prof_collect(c);
    return (int64_t)D;
}
extern "C" int64_t bscgpu_qlfc_static_pstream(bscgpu_ctx* c, const uint8_t* L, int n, uint16_t* out, int64_t cap, int* nblocks_out,
                                              int* sub_start /*[8]*/, int* sub_size /*[8]*/, int64_t* poff_out /*[9]*/, uint16_t* dbg_out /*[3][cap] or NULL*/)
{
    return qlfc_static_pstream_stage(c, L, n, out, cap, nblocks_out, sub_start, sub_size, poff_out, dbg_out, false, nullptr);
}
// The same stage with the stream as it crosses PCIe since round 6 (DcP13): out[0 .. pbase[nb] / 8 * 13) bytes (cap in BYTES), sub-block b's
// fields from decision pbase[b] of the packed space on (13 bits each, eight in 13 bytes); poff as above.  BSC_NOT_SUPPORTED also when the
// packed form was not produced for this block (BSCGPU_OPT_DC_PACKED_STREAM off, or 64 consecutive runs with more decisions than a
// wavefront stages: bsc_compress then takes the 16-bit form for that block).
extern "C" int64_t bscgpu_qlfc_static_pstream_packed(bscgpu_ctx* c, const uint8_t* L, int n, uint8_t* out, int64_t cap_bytes, int* nblocks_out,
                                                     int* sub_start /*[8]*/, int* sub_size /*[8]*/, int64_t* poff_out /*[9]*/, int64_t* pbase_out /*[9]*/)
{
    if (!pbase_out) return BSC_BAD_PARAMETER;
    return qlfc_static_pstream_stage(c, L, n, reinterpret_cast<uint16_t*>(out), cap_bytes, nblocks_out, sub_start, sub_size, poff_out, nullptr, true, pbase_out);
}

// The facts of a block alone (include/bscgpu.h): the front end as above, then the flags, every sub-block's runs, its decisions for the
// coder at hand and the flags left open.
extern "C" int bscgpu_qlfc_pstream_facts(bscgpu_ctx* c, const uint8_t* L, int n, int coder, int* nblocks_out, int* sub_start /*[8]*/, int* sub_size /*[8]*/,
                                         uint32_t* sub_runs /*[8]*/, uint32_t* sub_dec /*[8]*/, uint32_t* sub_und /*[8]*/)
{
    if ((coder != 1 && coder != 3) || !sub_runs || !sub_dec || !sub_und) return BSC_BAD_PARAMETER;
    StageFront F;
    int rc = qlfc_stage_front(c, L, n, nblocks_out, sub_start, sub_size, &F);
    if (rc < 0) return rc;
    DcBlock B;
    const FrontBufs fb = front_bufs(c);
    rc = devcoder_block_facts(c, fb.sym, fb.rank, fb.start, F.m, (u32)n, F.nb, sub_start, sub_size, F.run_first,
                              F.max_rank, coder, &B);
    if (rc < 0) return rc;
    *nblocks_out = F.nb;
    for (int b = 0; b < F.nb; ++b) { sub_runs[b] = F.run_first[b + 1] - F.run_first[b]; sub_dec[b] = B.dec[b]; sub_und[b] = B.und[b]; }
    return BSC_NO_ERROR;
}
