// batch_pass_plan.h — what the driver of a batched-compress call (block.cpp: compress_batch_impl) decides, as plain host
// arithmetic without any HIP in it: which blocks ride in which pass and the range of the input a pass covers, which route the call
// takes, what becomes of a block after its preparation, where every block lies in the pass, which model step a pass takes and whether
// its stream is kept, which counters that moves, what a sorted block is coded from, and how a block left over is compressed.  The
// driver does what these rules say and tells them what came back from the device; tools/batch_pass_probe.cpp does the same with the
// device's answers read from its input, for tests/test_batch_pass_plan_host.py.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <vector>

#include "../../../include/libbsc.h"
#include "../../../include/bscgpu.h"
#include "container.h"          // aux_rate

constexpr int BATCH_PASS_MAX_BLOCKS = BSCGPU_ST_BATCH_MAX_BLOCKS;      // blocks of a pass, empty ones included: BWT and ST alike

// ---- pass membership and ranges ---------------------------------------------------------------------------------------------------
// Consecutive members (member(n): a block of n > 0 bytes that the pass's sorter takes) fill passes of at most cap bytes and
// BATCH_PASS_MAX_BLOCKS blocks; pass_of[b] = -1 for the others.  -> the number of passes; LIBBSC_BAD_PARAMETER at a negative size
template <class Member>
static inline int batch_pass_plan(const int* sizes, int count, int64_t cap, Member member, int* pass_of)
{
    int passes = 0, cur = -1, span = 0;
    int64_t bytes = 0;
    for (int b = 0; b < count; ++b) {
        const int n = sizes[b];
        if (n < 0) return LIBBSC_BAD_PARAMETER;
        if (!(n > 0 && (int64_t)n <= cap && member(n))) {
            pass_of[b] = -1;
            if (n > 0) cur = -1;                     // a pass is one contiguous range of the input: a block of its own ends it
            else if (cur >= 0) ++span;               // (an empty block inside a pass is an empty entry of its table)
            continue;
        }
        if (cur < 0 || bytes + n > cap || span + 1 > BATCH_PASS_MAX_BLOCKS) { cur = passes++; bytes = 0; span = 0; }
        pass_of[b] = cur; bytes += n; ++span;
    }
    return passes;
}
// the BWT takes blocks below BSCGPU_BATCH_MAX_N (another sorter: none), ST3..ST8 below BSCGPU_ST_BATCH_MAX_N (a block of one byte too:
// its record sorts like any other)
static inline int batch_pass_plan_bwt(const int* sizes, int count, int blockSorter, int64_t cap, int* pass_of)
{
    return batch_pass_plan(sizes, count, cap, [=](int n) { return blockSorter == LIBBSC_BLOCKSORTER_BWT && n < BSCGPU_BATCH_MAX_N; }, pass_of);
}
static inline int batch_pass_plan_st(const int* sizes, int count, int64_t cap, int* pass_of)
{
    return batch_pass_plan(sizes, count, cap, [](int n) { return n < BSCGPU_ST_BATCH_MAX_N; }, pass_of);
}

// the pass that starts at member b covers [b, e): its members and the empty blocks between them, one contiguous range of the input
static inline int batch_pass_end(const int* pass_of, const int* sizes, int count, int b)
{
    int e = b;
    for (int q = b; q < count && (pass_of[q] == pass_of[b] || (pass_of[q] < 0 && sizes[q] == 0)); ++q) if (pass_of[q] == pass_of[b]) e = q + 1;
    return e;
}

// ---- the call's route --------------------------------------------------------------------------------------------------------------
struct BatchOptions { int front, model, model_fast, segments, packed, device_rc, model_adaptive, adaptive_segments; };      // the context's BSCGPU_OPT_* values

struct BatchRoute {
    bool front;          // the front end of every pass on the GPU (BSCGPU_OPT_BATCH_FRONT): its run arrays come down instead of its L
    bool model;          // ... and the coder's model behind it: the static coder's (BSCGPU_OPT_BATCH_MODEL) or the fast coder's
    bool fast_model;     // (BSCGPU_OPT_BATCH_MODEL_FAST: an option and counters of its own) or the adaptive coder's (adaptive_model, below)
    bool segments;       // ... in model segments (BSCGPU_OPT_BATCH_MODEL_SEGMENTS; the adaptive coder's: BSCGPU_OPT_BATCH_ADAPTIVE_SEGMENTS alone); with the
                         // device's range coder on, a pass of -e1 / -e0 takes the whole-pass route
    bool packed;         // ... with the stream in the packed 13-bit form (BSCGPU_OPT_BATCH_MODEL_PACKED): -e1 only, whole passes and segments alike
    bool device_rc;      // a whole pass's streams stay in HBM: one launch of the device's range coder codes them (BSCGPU_OPT_DEVICE_RC)
    int64_t min_pass;    // smallest pass (bytes of L) that is given to the device model
    int64_t segment_target;
    bool adaptive_model; // the model is the adaptive coder's (BSCGPU_OPT_BATCH_MODEL_ADAPTIVE, -e2: an option and counters of its own): whole passes of
                         // 16-bit entries that the host codes — no packed form, no device range coder, and segments only by its own option
                         // (BSCGPU_OPT_BATCH_ADAPTIVE_SEGMENTS), whatever the other coders' options say
};

// the front end needs its two pinned run buffers: they are asked for (front_host) only where this holds
static inline bool batch_wants_front(int npass, const BatchOptions& o) { return npass > 0 && o.front != 0; }

// min_pass_static / _fast: the smallest modelled pass of either coder; front_host: the pinned run buffers are there
static inline BatchRoute batch_route(int npass, const BatchOptions& o, int coder, bool front_host, int64_t min_pass_static, int64_t min_pass_fast,
                                     int64_t segment_target)
{
    BatchRoute R;
    R.front = batch_wants_front(npass, o) && front_host;
    R.fast_model = R.front && o.model_fast != 0 && coder == LIBBSC_CODER_QLFC_FAST;
    R.adaptive_model = R.front && o.model_adaptive != 0 && coder == LIBBSC_CODER_QLFC_ADAPTIVE;
    R.model = R.fast_model || R.adaptive_model || (R.front && o.model != 0 && coder == LIBBSC_CODER_QLFC_STATIC);
    R.min_pass = R.fast_model ? min_pass_fast : min_pass_static;         // (-e2: the static coder's until its own sweep is measured)
    R.segments = R.adaptive_model ? o.adaptive_segments != 0 : R.model && o.segments != 0 && o.device_rc == 0;
    R.segment_target = R.segments ? segment_target : 0;
    R.packed = R.model && !R.fast_model && !R.adaptive_model && o.packed != 0;
    R.device_rc = R.model && !R.adaptive_model && o.device_rc != 0;
    return R;
}

// ---- a block's class after its preparation --------------------------------------------------------------------------------------------
enum BatchClass {
    BATCH_EMPTY,         // an empty block between members: an empty entry of the pass's table
    BATCH_STORED,        // host input of <= LIBBSC_HEADER_SIZE bytes: stored at once
    BATCH_RIDES,         // device input of that size: its bytes come back with the pass (rate -1: L = T) and are stored from there
    BATCH_SINGLE,        // after LZP: the single-block path decides (a sorter input too short for the aux indexes)
    BATCH_SORTED,        // in the pass's sort
};
// n: the block's size, lz: what LZP left of it (n where there is no LZP, or before it ran: a block of more than LIBBSC_HEADER_SIZE
// bytes is then never BATCH_SINGLE); st: a sort transform (no aux indexes); dev: input in HBM; member: of the pass (else it is empty)
static inline BatchClass batch_block_class(int n, int lz, bool st, bool dev, bool member)
{
    if (!member) return BATCH_EMPTY;
    if (n <= LIBBSC_HEADER_SIZE) return dev ? BATCH_RIDES : BATCH_STORED;
    if (!st && aux_rate(lz) < 2) return BATCH_SINGLE;
    return BATCH_SORTED;
}

// ---- a pass's geometry ------------------------------------------------------------------------------------------------------------------
// psz[i] / prate[i]: size and aux rate (0: a sort transform, -1: not sorted, L = T) of entry i of the pass's table; at[i]: where its L
// lies in the pass; pos: the bytes of the pass.  Device input: the pass is the caller's own range of HBM, every block in place; host
// input: the sorted blocks back to back, what LZP left of them.  packed_rides (a pass whose LZP ran on the device, whatever its input:
// dev is then false): laid out as host input, and a block that rides along keeps riding, with its sizes[i] raw bytes.
struct BatchGeometry { std::vector<int> psz, prate; std::vector<int64_t> at; int64_t pos; };
static inline void batch_pass_geometry(const BatchClass* cls, const int* sizes, const int* lz, int count, bool st, bool dev, BatchGeometry* G,
                                       bool packed_rides = false)
{
    G->psz.assign((size_t)count, 0); G->prate.assign((size_t)count, -1); G->at.assign((size_t)count, 0);
    G->pos = 0;
    for (int i = 0; i < count; ++i) {
        const bool sorted = cls[i] == BATCH_SORTED;
        G->at[i] = G->pos;
        G->prate[i] = sorted ? (st ? 0 : aux_rate(lz[i])) : -1;
        G->psz[i] = dev ? sizes[i] : sorted ? lz[i] : packed_rides && cls[i] == BATCH_RIDES ? sizes[i] : 0;
        G->pos += G->psz[i];
    }
}

// ---- a pass's model step --------------------------------------------------------------------------------------------------------------
enum BatchModelStep { BATCH_MODEL_NONE, BATCH_MODEL_WHOLE, BATCH_MODEL_SEGMENTS };
// nsub: sub-blocks of the pass's layout; pos: its bytes; model_host: the two pinned stream buffers are there (they are allocated by the
// first pass that qualifies — ask with true first — and without them the passes keep the host model)
static inline BatchModelStep batch_model_step(const BatchRoute& R, int nsub, int64_t pos, bool model_host)
{
    if (!R.model || nsub <= 0 || pos < R.min_pass || !model_host) return BATCH_MODEL_NONE;
    return R.segments ? BATCH_MODEL_SEGMENTS : BATCH_MODEL_WHOLE;
}

// what a pass adds to the context's counters (BSCGPU_CNT_BATCH_*, BSCGPU_CNT_DEVICE_RC_BLOCKS; the segments' own are the model's)
struct BatchCounters { int front_passes, l_passes, model_passes, model_declined, fast_passes, fast_declined, packed_passes, packed_void, device_rc,
                       adaptive_passes, adaptive_declined; };

enum BatchVerdict { BATCH_PASS_KEPT, BATCH_PASS_HOST, BATCH_PASS_DECLINED, BATCH_PASS_ERROR };
// A whole-pass model returned mrc with D decisions; pk: what it left is the packed 13-bit form, pbytes of it (else 16-bit entries);
// entries: what a pinned stream buffer holds in 16-bit entries.  The stream is kept where it has landing room (packed: less the few
// bytes a packed entry's 4-byte read may reach past a stream); a pass without is the host model's, and counts nowhere
static inline BatchVerdict batch_whole_verdict(int mrc, uint32_t D, int pk, int64_t pbytes, size_t entries)
{
    if (mrc == LIBBSC_NOT_SUPPORTED) return BATCH_PASS_DECLINED;
    if (mrc < 0) return BATCH_PASS_ERROR;
    return (pk ? (size_t)pbytes + 8 <= entries * 2 : (size_t)D <= entries) ? BATCH_PASS_KEPT : BATCH_PASS_HOST;
}
// A segmented model returned mrc and left blk_state[i] != 0 where block i takes the host model: kept where the device's stream serves
// any block with a sub-block (an arena that did not fit, LIBBSC_NOT_SUPPORTED: none does)
static inline BatchVerdict batch_segments_verdict(int mrc, const int* blk_sub, const int* blk_state, int count)
{
    if (mrc < 0 && mrc != LIBBSC_NOT_SUPPORTED) return BATCH_PASS_ERROR;
    for (int i = 0; i < count && mrc >= 0; ++i) if (blk_sub[i + 1] > blk_sub[i] && blk_state[i] == 0) return BATCH_PASS_KEPT;
    return BATCH_PASS_DECLINED;
}
// the counters a model step moves (the front end's own pass counter aside); pk as above, whole passes only
static inline BatchCounters batch_model_counters(const BatchRoute& R, BatchModelStep step, BatchVerdict v, int pk)
{
    BatchCounters d = {};
    if (v == BATCH_PASS_KEPT) {
        ++(R.fast_model ? d.fast_passes : R.adaptive_model ? d.adaptive_passes : d.model_passes);
        if (step == BATCH_MODEL_WHOLE && R.packed) ++(pk ? d.packed_passes : d.packed_void);
        if (step == BATCH_MODEL_WHOLE && R.device_rc) ++d.device_rc;
    }
    if (v == BATCH_PASS_DECLINED) ++(R.fast_model ? d.fast_declined : R.adaptive_model ? d.adaptive_declined : d.model_declined);
    return d;
}

// ---- what a sorted block is coded from ------------------------------------------------------------------------------------------------
enum BatchSource {
    BATCH_FROM_L,        // its L, by the host coder
    BATCH_FROM_RUNS,     // its run arrays in the pass's layout, by the host model
    BATCH_FROM_PS16,     // the device model's 16-bit stream of the static coder, or the adaptive coder's in the same form: the range coder alone
    BATCH_FROM_PS13,     // ... in the packed 13-bit form
    BATCH_FROM_FAST,     // the fast coder's stream
    BATCH_FROM_DEVICE_RC // the bytes the device's range coder left
};
// layout: the pass took the front end; stream: the pass kept a stream of the device model; coded: the device's range coder has coded
// it; host_block: this block of a segmented pass takes the host model (blk_state != 0); packed: the stream is the 13-bit form
static inline BatchSource batch_block_source(bool layout, bool stream, bool coded, bool host_block, bool fast, bool packed)
{
    if (!layout) return BATCH_FROM_L;
    if (coded) return BATCH_FROM_DEVICE_RC;
    if (!stream || host_block) return BATCH_FROM_RUNS;
    return fast ? BATCH_FROM_FAST : packed ? BATCH_FROM_PS13 : BATCH_FROM_PS16;
}

// ---- the blocks left over ----------------------------------------------------------------------------------------------------------------
enum BatchLeftover {
    BATCH_LEFT_NONE,
    BATCH_LEFT_ONE_BY_ONE,   // before the pipe: larger than the context, a too short sorter input, host input that is stored
    BATCH_LEFT_PIPE,         // through a pipe on the context: the GPU stage of one overlaps the host coding of the ones before it
};
// single: the block is in no pass, or its pass left it to the single path (BATCH_SINGLE); member: of a pass
static inline BatchLeftover batch_leftover(bool single, bool member, int n, int64_t cap, bool dev)
{
    if (!single) return BATCH_LEFT_NONE;
    return !member && (int64_t)n <= cap && (dev || n > LIBBSC_HEADER_SIZE) ? BATCH_LEFT_PIPE : BATCH_LEFT_ONE_BY_ONE;
}
