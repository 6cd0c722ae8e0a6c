// dev_common.h — shared declarations for the gfx950 device layer (internal).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>
#include <functional>
#include <string>
#include <vector>

#include "../../../include/bscgpu.h"
#include "bwt_plan.h"      // RadixPass; the BWT driver's plan (host arithmetic, no HIP)
#include "dc_block_plan.h" // DcBlockSchedule: a single block in sub-block segments (host arithmetic, no HIP)
#include "qlfc_front_plan.h" // the QLFC front end's cuts, alphabets, pass plan and table layout (host arithmetic, no HIP)

typedef unsigned long long u64;
typedef unsigned int       u32;
typedef unsigned short     u16;
typedef unsigned char      u8;

// libbsc error codes (libbsc.h:41-51)
#define BSC_NO_ERROR                0
#define BSC_BAD_PARAMETER          -1
#define BSC_NOT_ENOUGH_MEMORY      -2
#define BSC_NOT_COMPRESSIBLE       -3
#define BSC_NOT_SUPPORTED          -4
#define BSC_DATA_CORRUPT           -6
#define BSC_GPU_ERROR              -7
#define BSC_GPU_NOT_SUPPORTED      -8
#define BSC_GPU_NOT_ENOUGH_MEMORY  -9

// ---------------------------------------------------------------------------------------------
// Work decomposition shared by all "chunked" kernels: the input is cut into at most MAX_CHUNKS
// contiguous chunks, one workgroup per chunk, each chunk a whole number of tiles.  ~1024 chunks
// = 4 workgroups of 256 threads on each of the 256 CUs (all resident at once, b % 8 -> XCD so
// every XCD streams an equal share).
// ---------------------------------------------------------------------------------------------
constexpr int   WG          = 256;      // threads per workgroup (4 wave64)
constexpr int   WAVES       = WG / 64;
#ifndef BSC_MAX_CHUNKS
#define BSC_MAX_CHUNKS 1024
#endif
constexpr int   MAX_CHUNKS  = BSC_MAX_CHUNKS;

struct Chunking {
    u32 num_tiles;     // total tiles
    u32 chunk_tiles;   // tiles per chunk
    u32 num_chunks;    // workgroups to launch
};
static inline Chunking make_chunking(u64 n, u32 tile) {
    Chunking c;
    c.num_tiles   = (u32)((n + tile - 1) / tile);
    if (c.num_tiles == 0) c.num_tiles = 1;
    c.chunk_tiles = (c.num_tiles + MAX_CHUNKS - 1) / MAX_CHUNKS;
    c.num_chunks  = (c.num_tiles + c.chunk_tiles - 1) / c.chunk_tiles;
    return c;
}

// ---------------------------------------------------------------------------------------------
// The scalar area of a context: dscal (HBM) and hscal (pinned), SCAL_WORDS u32 each, hscal[i] mirroring dscal[i]; dscal64, SCAL64_WORDS
// u64 in HBM.  This is the one map of both: every user indexes them by these names.  A context runs one call at a time, so words of
// stages that never run inside one another may coincide; those are the aliases below, each written as one.  Ranges that can be live
// together are held apart by the static_asserts.
// ---------------------------------------------------------------------------------------------
constexpr int SCAL_WORDS = 1024, SCAL64_WORDS = 16;
constexpr int DS_TOTAL     = 0;     // seg_scan_kernel's total: the unsorted records of a BWT round
constexpr int DS_PRIMARY   = 1;     // bwt_find_kernel: the primary index (the emit kernels read it)
constexpr int DS_GIVEUP    = 2;     // a BWT round's segmented sort met a group it could not hold
constexpr int DS_NMID      = 3;     // seg_apply: groups of more than HY_G records in the new unsorted set (hybrid doubling rounds) ...
constexpr int DS_MIDEXCESS = 4;     // ... and their records past the first HY_G
constexpr int DS_NLONG     = 5;     // the same two counts for groups of more than RS_G records
constexpr int DS_EXCESS    = 6;
constexpr int DS_LRTOTAL   = 7;     // what a hybrid round's extraction really found (must equal the host's count)
constexpr int DS_ROUND_WORDS = DS_LRTOTAL + 1;      // a BWT round reads words [0, DS_ROUND_WORDS) back in one copy
constexpr int DS_AUX       = 8,   DS_AUX_LEN = 256;        // bwt_find_kernel: aux index t at DS_AUX + t; bwt_finish reads [0, DS_AUX + DS_AUX_LEN) back
constexpr int DS_BYTEHIST  = 300, DS_BYTEHIST_LEN = 256;   // BWT first sort: the text's byte histogram
constexpr int DS_CODES     = 560, DS_CODES_LEN = 64;       // ... its code table, byte -> code (256 bytes)
constexpr int DS_FRONT_LUT = 640, DS_FRONT_LUT_LEN = 64;   // QLFC front end: the alphabet's renumbering (256 bytes), up from hscal
constexpr int DS_DECODE    = 720, DS_DECODE_LEN = 64;      // BWT first sort: code -> byte (256 bytes), read by the emit kernel
constexpr int OS_ERR_SLOT  = 1000;  // sticky error word of the single-read digit passes (cleared by radix_onesweep_check only)
// Aliases: a word one stage leaves free, taken by a stage that never runs inside it.
constexpr int DS_FRONT_RUNS = DS_TOTAL;       // the front end scans its run heads with seg_scan_kernel after the sort: the total is its run count m
constexpr int DS_ST_INDEX   = DS_GIVEUP;      // a sort transform's index; a context sorts a block by BWT or by ST
constexpr int DS_ST_WORDS   = 4;              // ... st_device reads words [0, DS_ST_WORDS) back for it
constexpr int DS_UB_GUARD   = DS_MIDEXCESS;   // the inverse BWT's guard word: decoding runs no BWT round
constexpr int DS64_ST_KEY0  = 0;              // dscal64: the sort transform's key of position 0

static_assert(DS_ROUND_WORDS <= DS_AUX && DS_AUX + DS_AUX_LEN <= DS_BYTEHIST && DS_BYTEHIST + DS_BYTEHIST_LEN <= DS_CODES
              && DS_CODES + DS_CODES_LEN <= DS_FRONT_LUT && DS_FRONT_LUT + DS_FRONT_LUT_LEN <= DS_DECODE && DS_DECODE + DS_DECODE_LEN <= OS_ERR_SLOT
              && OS_ERR_SLOT + 1 <= SCAL_WORDS, "the ranges of the scalar area lie in this order, apart, inside it");
static_assert(DS_TOTAL < DS_PRIMARY && DS_PRIMARY < DS_GIVEUP && DS_GIVEUP < DS_NMID && DS_NMID < DS_MIDEXCESS && DS_MIDEXCESS < DS_NLONG
              && DS_NLONG < DS_EXCESS && DS_EXCESS < DS_LRTOTAL, "the words of a BWT round are distinct");
static_assert(DS_ST_INDEX < DS_ST_WORDS && DS_ST_WORDS <= DS_AUX && DS64_ST_KEY0 < SCAL64_WORDS, "the sort transform's words");
static_assert(DS_FRONT_RUNS < DS_ROUND_WORDS && DS_ST_INDEX < DS_ROUND_WORDS && DS_UB_GUARD < DS_ROUND_WORDS,
              "every alias names a word of a BWT round: none reaches a table, the histogram or the sticky error word");

// ---------------------------------------------------------------------------------------------
// Context
// ---------------------------------------------------------------------------------------------
struct ScatterLaunch { double ms; u64 records; };

// Pinned host buffers one block's QLFC front-end output lands in (sized for max_n).
struct HostSlot {
    u8*  hsym   = nullptr;   // run symbols
    u8*  hrank  = nullptr;   // QLFC ranks
    u32* hstart = nullptr;   // run start positions
    u8*  run_base = nullptr; size_t run_bytes = 0;   // the one pinned mapping behind hsym / hrank / hstart
    u16* hps    = nullptr;   // probability stream of the device coder (allocated when that path is first used)
    size_t hps_cap = 0;      // entries
    hipEvent_t copy_ev = nullptr;   // recorded on the copy stream behind the block's p-stream copy (its last piece); guards the device buffer's reuse
    hipEvent_t part_ev[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};   // behind the piece of each sub-block: a coder task waits
                                    // for its own sub-blocks only (the stream leaves sub-block by sub-block, 366 MB in all for a 64 MiB text block)
    // the same pieces through the DMA engine directly (dma_copy.h): one HSA signal per piece, the landing zone's device address
    uint64_t part_sig[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    void* hps_dev = nullptr;
};
constexpr int MAX_SLOTS = 8;

struct DevCoder;                  // device-side static coder state (devcoder.hip), created on first use
// What a unit of the device coder's model work (a block, a pass, a pass in segments) says about itself (bscgpu_option_get: BSCGPU_CNT_DC_*)
struct DcNote {
    int fail = 0;            // why it left the device coder (bit mask, devcoder.hip FAIL_* = BSCGPU_DC_FAIL_*), 0 = it did not
    int replays = 0;         // evaluation chunks replayed serially
    int avg_und = 0;         // runs whose avg_rank >= 32 flag the two-sided bracket left undecided (any: FAIL_AVG)
    int avg_resolved = 0;    // ... of those, the runs the exact resolve settled (BSCGPU_OPT_DC_AVG_EXACT)
    int replay_resolved = 0; // chunks whose start the exact resolve settled (BSCGPU_OPT_DC_REPLAY_EXACT)
    int hist_ext = 0;        // runs whose run_hist bracket was still open after nine predecessors (the extended look-back)
    int hist_resolved = 0;   // ... of those, the runs the exact resolve settled (BSCGPU_OPT_DC_HIST_EXACT)
    void clear(int why = 0) { *this = DcNote(); fail = why; }
};

constexpr u32 DC_MIX_CHAIN_CAP = 1u << 18;  // devcoder.hip: steps of the longest mixer chain of an -e2 pass (bscgpu_ctx::dc_mix_cap).  Measured (DESIGN §2b,
                                            // "The adaptive coder's model of a pass"): the walk takes 274 - 293 ns per step of the longest chain, the host
                                            // coder 108 - 122 ms for a 64 MiB pass on 16 threads: 371 - 423 thousand steps, rounded down to a power of two
constexpr u32 UB_STEP_CAP = 1u << 22;       // unbwt.hip: steps a walk may take between two marked rows (bscgpu_ctx::ub_step_cap)

struct bscgpu_ctx {
    int          device      = 0;
    hipStream_t  stream      = nullptr;
    hipStream_t  copy_stream = nullptr;   // D2H of the device coder's p stream, overlapped with the next block's GPU stage
    hipEvent_t   ps_guard[2] = {nullptr, nullptr};   // last copy out of each device p-stream buffer (not owned: a slot's copy_ev)
    uint64_t     ps_guard_sig[2][8] = {{0, 0, 0, 0, 0, 0, 0, 0}, {0, 0, 0, 0, 0, 0, 0, 0}};   // ... or, when the copy went through dma_copy.h, the signals of its pieces (host-side wait)
    int          ps_toggle   = 0;
    hipEvent_t   sync_ev     = nullptr;   // blocking-sync event: waiting threads sleep instead of spinning (host CPUs are the scarce resource)
    int64_t      max_n       = 0;
    char*        arena       = nullptr;
    size_t       arena_bytes = 0;

    // carved device buffers (sized for max_n)
    u8*  dT     = nullptr;   // text with 64 B zero/cyclic padding on both sides (points at T[0])
    u8*  dL     = nullptr;   // output bytes
    u64* kA     = nullptr;  u64* kB = nullptr;   // sort keys ping/pong
    u32* vA     = nullptr;  u32* vB = nullptr;   // sort values ping/pong
    u32* SA     = nullptr;
    u32* ISA    = nullptr;
    u32* cpos[2] = {nullptr, nullptr};
    u32* csa [2] = {nullptr, nullptr};
    u32* cgrp[2] = {nullptr, nullptr};
    u8*  flags  = nullptr;
    u32* counts = nullptr;   // [256][MAX_CHUNKS] radix per-chunk digit counts -> offsets
    u32* rowtot = nullptr;   // [256]
    u32* segsum = nullptr;   // [2][MAX_CHUNKS] per-chunk (unsorted count, last head+1)
    u32* segoff = nullptr;   // [2][MAX_CHUNKS] scanned
    u32* dscal  = nullptr;   // small device scalars (SCAL_WORDS u32, mirrored slot by slot in hscal; the slot map is above)
    u64* dscal64 = nullptr;  // small device u64 scalars (SCAL64_WORDS)
    u64* adler_part = nullptr; // [MAX_CHUNKS][2]
    u32* tile_counts = nullptr; size_t tile_counts_cap = 0;   // [256][tiles of 8192 records]: rs_scatter_tiled's offsets, allocated on first use
    u32* long_tables = nullptr;   // BWT text rounds: counting-sort tables of the long-group split (bwt.hip LongTables), allocated on first use
    u32* batch_tab = nullptr;     // batched BWT / ST pass: block table + per-block results (bwt.hip BwtBatch, st.hip st_batch_device), allocated on first use
    size_t batch_bytes = 0;       // HBM of batch_tab (bscgpu_arena_bytes counts it once allocated)
    u8*  batch_host[2] = {nullptr, nullptr};   // pinned: a batched pass's text going up and its L coming back (two: coding overlaps the next pass)
    // the QLFC front end of a whole pass (qlfc_front.hip: qlfc_front_batch), allocated on first use
    u32* front_tab = nullptr;     // sub-block table of the pass (offsets, block starts, first runs), split-flag table, first run of every symbol per sub-block
    size_t front_bytes = 0;       // HBM of front_tab (bscgpu_arena_bytes counts it once allocated)
    u8*  front_host[2] = {nullptr, nullptr};   // pinned: a pass's run arrays coming back (sym, rank, start for max_n runs + the first-run table); two: coding overlaps the next pass
    size_t front_host_bytes = 0;
    int  batch_front = 1;         // BSCGPU_OPT_BATCH_FRONT (default: DESIGN §2b, "The QLFC front end of a pass")
    int  cnt_front_passes = 0, cnt_l_passes = 0;   // BSCGPU_CNT_BATCH_FRONT_PASSES / _L_PASSES
    // the range coder stage (rangecoder.hip): stream table, prefix entries and results of one launch; grows on demand
    u8*  rc_tab = nullptr;
    size_t rc_tab_bytes = 0;      // HBM of rc_tab (bscgpu_arena_bytes counts it once allocated)
    int  device_rc = 0;           // BSCGPU_OPT_DEVICE_RC: a device-model block's streams are range-coded on the device (default off)
    int  cnt_device_rc = 0;       // BSCGPU_CNT_DEVICE_RC_BLOCKS
    // the static coder's model of a whole pass (devcoder.hip: devcoder_pstream_batch)
    int  batch_model = 0;         // BSCGPU_OPT_BATCH_MODEL (default 0: DESIGN §2b, "The static coder's model of a pass")
    int  cnt_model_passes = 0, cnt_model_declined = 0;   // BSCGPU_CNT_BATCH_MODEL_PASSES / _DECLINED
    // the fast coder's (the same entry with coder 3); it shares the pinned stream buffers below
    int  batch_model_fast = 0;    // BSCGPU_OPT_BATCH_MODEL_FAST (default 0: DESIGN §2b, "The fast coder's model of a pass")
    int  cnt_model_fast_passes = 0, cnt_model_fast_declined = 0;   // BSCGPU_CNT_BATCH_FAST_PASSES / _DECLINED
    // the adaptive coder's (coder 2: the static model with the adaptive rates, then the mixer chains)
    int  batch_model_adaptive = 0;   // BSCGPU_OPT_BATCH_MODEL_ADAPTIVE (default 0: DESIGN §2b, "The adaptive coder's model of a pass")
    int  batch_adaptive_segments = 0;   // BSCGPU_OPT_BATCH_ADAPTIVE_SEGMENTS (default 0: DESIGN §2b, "The adaptive coder's model in segments")
    int  cnt_model_adaptive_passes = 0, cnt_model_adaptive_declined = 0;   // BSCGPU_CNT_BATCH_ADAPTIVE_PASSES / _DECLINED
    u32  dc_mix_cap = DC_MIX_CHAIN_CAP;   // steps the longest mixer chain of a pass may have (BSC_DC_MIX_CHAIN_CAP, a test knob): above it FAIL_MIX
    u32  dc_mix_chains = 0, dc_mix_longest = 0;   // BSCGPU_CNT_DC_MIX_CHAINS / _LONGEST: the last -e2 pass given to the device model
    u32  dc_mix_walk_us = 0;                      // BSCGPU_CNT_DC_MIX_WALK_US: ... and the host's wall time of its walk (placement and walk kernels, one sync)
    // model segments (devcoder.hip: devcoder_pstream_segments; DESIGN §2b, "Model segments")
    int  batch_model_segments = 0;   // BSCGPU_OPT_BATCH_MODEL_SEGMENTS (default 0)
    int  cnt_seg = 0, cnt_seg_reruns = 0, cnt_seg_host_blocks = 0;   // BSCGPU_CNT_BATCH_SEGMENTS / _SEG_RERUNS / _SEG_HOST_BLOCKS
    // the packed 13-bit stream of a pass ("The packed stream of a pass")
    int  batch_model_packed = 0;     // BSCGPU_OPT_BATCH_MODEL_PACKED (default 0)
    int  cnt_packed_passes = 0, cnt_packed_void = 0;                 // BSCGPU_CNT_BATCH_PACKED_PASSES / _VOID
    u16* model_host[2] = {nullptr, nullptr};   // pinned: a pass's probability stream coming down (two: coding overlaps the next pass), allocated on first use
    size_t model_host_entries = 0;
    bool model_host_failed = false;            // they could not be pinned: the route is off for this context
    u64* wc_sink = nullptr;  // [512 * 1024] scratch of the digit passes: phase stamps under RS_PHASE_TIMING (rs_scatter, the single-read passes)
    // single-read digit passes (radix_onesweep.hip), allocated on first use
    int  num_cus = 256;           // hipDeviceAttributeMultiprocessorCount of the context's device
    int  os_mode = 0;             // BSC_RS_ONESWEEP: 0 = off, 1 = large (key, value) sorts only, 2 = every sort of >= 4 tiles (tests), 3 = large sorts, keys-only too (default)
    u32* os_agg = nullptr;        // [tiles][256] tile rows {launch tag, digit count}
    u32* os_zero = nullptr;       // [8 passes] x {control block, digit totals, batch rows}: cleared per sort
    u32  os_tiles_cap = 0;
    u32  os_pass_stride = 0;      // words
    u32  os_batch_words = 0;      // words of the batch rows inside a pass's block (the group rows follow)
    u32  os_epoch = 0;            // launches so far (launch tag = epoch % 255 + 1)
    bool os_check_pending = false;   // hscal[OS_ERR_SLOT] has not been looked at since the last single-read sort
    bool os_available = true;        // the single-read kernels could be set up on this device (radix_onesweep_setup)
    int  os_retries = 0;             // transforms redone through the three-kernel passes after a give-up (bscgpu_debug_counter)
    int  dc_avg_exact = 0;           // BSCGPU_OPT_DC_AVG_EXACT: open avg_rank flags are resolved exactly on the device (BSC_DC_AVG_EXACT=1)
    int  dc_replay_exact = 0;        // BSCGPU_OPT_DC_REPLAY_EXACT: open chunk starts of the evaluation are resolved exactly (BSC_DC_REPLAY_EXACT=1)
    int  dc_hist_exact = 0;          // BSCGPU_OPT_DC_HIST_EXACT: open run_hist brackets are resolved exactly on the device (BSC_DC_HIST_EXACT=1)
    u32  dc_replay_cand = 0;        // ... the widest start bracket that resolve walks, if BSC_DC_REPLAY_CAND sets one (a test knob); 0: DC_RP_CAND.  devcoder_rp_ensure clamps it to DC_RP_CAND
    int  dc_arena_div = 1;           // BSCGPU_OPT_DC_ARENA_DIV: the device coder's arena holds ceil(max_n / this) bytes' worth of runs and decisions (BSC_DC_ARENA_DIV)
    int  cnt_block_segments = 0;     // BSCGPU_CNT_DC_BLOCK_SEGMENTS: segments the last single block given to the device model ran in
    int  dc_p13 = 1;                 // BSCGPU_OPT_DC_PACKED_STREAM: the static coder's p stream leaves as 13 bits per decision (BSC_PS13=0: 16-bit entries)
    bool os_gave_up = false;         // radix_onesweep_check found a give-up: the caller may redo its sorts through the three-kernel passes
    // BWT first sort: the leftover low digit of the key is sorted by key packing (bwt.hip: bwt_pack_fold_kernel)
    int  bwt_fold = 1;               // BSCGPU_OPT_BWT_FOLD: 0 off, 1 packing also counts the remaining digits, 2 it leaves that to rs_hist_all
    int  cnt_bwt_folded = 0;         // BSCGPU_CNT_BWT_FOLDED
    bool fold_lds_set = false;       // the packing kernels' dynamic-LDS limit has been raised on this context's device
    // the LZP stage (lzp.hip)
    int  device_lzp = 0;             // BSCGPU_OPT_DEVICE_LZP: a host block with LZP goes up raw and is preprocessed on the device (BSC_DEVICE_LZP=1)
    int  cnt_lzp_blocks = 0, cnt_lzp_declined = 0;   // BSCGPU_CNT_LZP_BLOCKS / _DECLINED: blocks the route gave to the stage / that it declined
    int64_t lzp_last[5] = {0, 0, 0, 0, 0};           // BSCGPU_CNT_LZP_MATCHES .. _RAW_CHUNKS of the last block given to the stage (lzp_staged.h: CNT_*)
    int  batch_device_lzp = 0;       // BSCGPU_OPT_BATCH_DEVICE_LZP: the members of a host-input pass with LZP go up raw, one run of the stage per pass (BSC_BATCH_DEVICE_LZP=1)
    int  cnt_batch_lzp_passes = 0, cnt_batch_lzp_blocks = 0;   // BSCGPU_CNT_BATCH_LZP_PASSES / _BLOCKS: passes given to the stage over a pass, and their sorted blocks
    int  lzp_lds_set = 0;            // sweep variants whose dynamic-LDS limit has been raised on this context's device (bit mask)
    u8*  lzp_tab = nullptr;          // the stage's tables, for a block as for a pass (lzp.hip: lzp_stage): chunk table, result records, piece list, table bytes; allocated on first use
    u8*  lzp_tab_host = nullptr;     // ... and its pinned mirror
    size_t lzp_tab_bytes = 0;        // HBM of lzp_tab (bscgpu_arena_bytes counts it once allocated)
    u32  ub_step_cap = UB_STEP_CAP;  // inverse BWT: a walk longer than this between two marked rows is declined (BSC_UNBWT_STEP_CAP, a test knob)
    // pinned host
    u32* hscal  = nullptr;   // SCAL_WORDS u32 (the slot map is above)
    u64* hadler = nullptr;
    u64* hsplit = nullptr;   // pinned: split-flag words (max_n / 256 + 64 bytes)
    HostSlot slots[MAX_SLOTS];   // pinned landing zones for the QLFC front end; >1 when blocks are pipelined
    int      nslots = 0;
    DevCoder* dc = nullptr;
    bool     dc_alloc_failed = false;   // the device coder's arena did not fit: this context keeps the host model (not retried per block)
    DcNote   dc_note;            // the last block (pass) that went to the device coder, set whether it stayed there or not

    // profiling
    bool         prof        = false;
    bscgpu_kstat kstat[BSCGPU_K_COUNT];
    std::vector<ScatterLaunch> scatter_log;
    struct Pending { hipEvent_t a, b; int kind; u64 bytes; u64 records; };
    std::vector<Pending> pending;
    std::vector<hipEvent_t> event_pool;
    double       stage_ms[6] = {0, 0, 0, 0, 0, 0};

    std::string  err;
};

int  ctx_fail(bscgpu_ctx* c, int code, const char* what, hipError_t e);
// BSCGPU_TIMING=1: one line on stderr per set-up step (context creation, arenas, landing zones) with its wall time — where a short
// job's start-up goes
bool ctx_timing_on();
struct CtxTimer {
    const char* what; double t0; bool on;
    explicit CtxTimer(const char* w);
    ~CtxTimer();
};
hipError_t ctx_sync(bscgpu_ctx* c);   // wait for everything queued on c->stream without burning a CPU
#define HIP_TRY(ctx, expr)                                                         \
    do { hipError_t _e = (expr);                                                   \
         if (_e != hipSuccess) return ctx_fail((ctx), BSC_GPU_ERROR, #expr, _e);   \
    } while (0)
#define RC_TRY(expr) do { const int _rc = (expr); if (_rc < 0) return _rc; } while (0)     // an internal call's error code goes up as it is

// profiling brackets: PROF_BEGIN/END record events on ctx->stream around a launch.
void prof_begin(bscgpu_ctx* c, int kind, u64 bytes, u64 records);
void prof_end(bscgpu_ctx* c);
void prof_collect(bscgpu_ctx* c);   // after a stream sync: fold pending events into kstat

// ---- internal device-layer entry points (all asynchronous on ctx->stream) ---------------------
// Sort n records; passes applied in order (LSD).  Result lands in (keys, vals) if the number of
// passes is even, else in (keys_alt, vals_alt); *in_alt tells which.
// emit_pos (optional; one keys-only pass): emit_pos[i] = index in the output of input record i.
int radix_sort_passes(bscgpu_ctx* c, u64* keys, u64* keys_alt, u32* vals, u32* vals_alt, u64 n,
                      const RadixPass* passes, int npasses, int* in_alt, u32* emit_pos = nullptr, bool aux = false);

int  radix_onesweep_setup(bscgpu_ctx* c);
bool radix_onesweep_wanted(const bscgpu_ctx* c, u64 n, int npasses, bool has_val);
// totals_ready: radix_onesweep_prepare ran for this sort and the caller has added every digit's totals to the tables it returned (the
// counters of pass p, digit d at totals[p * stride + d]); the sort then launches its digit passes only.
int  radix_onesweep_prepare(bscgpu_ctx* c, u64 n, int npasses, u32** totals = nullptr, u32* stride = nullptr);
int  radix_onesweep_sort(bscgpu_ctx* c, u64* keys, u64* keys_alt, u32* vals, u32* vals_alt, u64 n, const RadixPass* passes, int npasses,
                         bool totals_ready = false);
int  radix_onesweep_check(bscgpu_ctx* c);   // after the next stream sync: did a pass of the last such sort give up a wait?
// A single-read digit pass that gave up a wait (radix_onesweep.hip: bounded polls; pre-emption, a debugger, a hogged CU) fails the
// sort, not the block: the transform is redone once with the three-kernel passes, which have no cross-workgroup protocol at all.
// once(second_attempt) runs the transform; every sort in it is checked (radix_onesweep_check) before anything is written to the
// caller's buffer.  The BWT does NOT rely on its private copy of the text for the second attempt (it may have been clobbered by
// kernels that ran behind the failed sort — kernels that consume a failed sort's output run before the check, on stale keys and
// values: see seg_apply_kernel — while the caller's buffer is untouched until the last kernel of a transform): it copies the text
// again.  The ST's caller's buffer may already hold the failed attempt's bytes when it is also the output: it reuses its copy.
template <class Once>
static inline int with_onesweep_retry(bscgpu_ctx* c, Once once)
{
    c->os_gave_up = false;
    int rc = once(false);
    if (rc == BSC_GPU_ERROR && c->os_gave_up) {
        const int mode = c->os_mode;
        c->os_mode = 0; c->os_gave_up = false; ++c->os_retries;
        rc = once(true);
        c->os_mode = mode;
    }
    return rc;
}
int radix_engine_setup(bscgpu_ctx* c);     // per-device kernel attributes; bscgpu_create calls it with c->device current

int bwt_device(bscgpu_ctx* c, const u8* dT_user, u8* dL_user, int64_t n, int64_t r, u32* I_host,
               int64_t* primary_out);
int bwt_first_sort_device(bscgpu_ctx* c, const u8* dT_user, int64_t n, u64* keys_out, u32* vals_out);   // (tests) the sorted arrays of the first sort
int st_device(bscgpu_ctx* c, const u8* dT_user, u8* dOut_user, int n, int k, int* index_out);
// Batched BWT pass (bwt.hip): `count` blocks of sizes[b] laid out back to back in dT_user, sum <= max_n, count <= BATCH_MAX_BLOCKS.
// rates[b] > 0: the block's aux rate, 0: primary index only, < 0: not transformed (L = T).  res[16 b + t] = I[t] of block b as bwt_device
// returns it (I[0] = the primary index), for t < (n_b - 1) / rates[b] + 1.
constexpr int BATCH_MAX_BLOCKS = 4096;
// adler_host != nullptr: also every block's Adler-32 of dT_user (st.hip: adler_batch_kernel, one launch), back with the same sync.
int bwt_batch_device(bscgpu_ctx* c, const u8* dT_user, u8* dL_user, const int* sizes, int count, const int* rates, u32* res,
                     u32* adler_host = nullptr);
// Batched ST pass (st.hip): the same layout and limits, order k = 3..8.  rates (optional): < 0 = the block is not transformed (out = T,
// index 0).  index_out[b] = what st_device returns for block b alone (0 for n_b <= 1); dOut_user may be dT_user.  adler_host as above.
int st_batch_device(bscgpu_ctx* c, const u8* dT_user, u8* dOut_user, const int* sizes, int count, int k, const int* rates, int* index_out,
                    u32* adler_host = nullptr);
// (stride 2: doff holds a (start, end) pair per block, blocks anywhere in d)
void launch_adler_batch(bscgpu_ctx* c, const u8* d, const u32* doff, u32 count, u32* dout, u32 stride = 1);     // st.hip (asynchronous)
int batch_tab_ensure(bscgpu_ctx* c);       // bwt.hip: batch_tab on first use
// The set-up of a batched BWT / ST pass (bwt.hip): count and total checked, the block table built and uploaded, every block's Adler-32
// launched where asked for.  total == 0: nothing to do.  index_out (ST only): zeroed, and rates may then be null (all blocks transformed).
struct BatchTab { u32 total; const u32* off; const int* rate; u32* res; };      // device: offsets [count + 1], rates [count], results
int batch_pass_setup(bscgpu_ctx* c, const u8* dT_user, const int* sizes, int count, const int* rates, int* index_out, u32* adler_host, BatchTab* bt);
// Batched inverse-BWT pass (unbwt.hip): `count` <= unbwt_batch_max_blocks(max_n) blocks, L of sizes[b] bytes back to back at
// dL (sum <= max_n); idx[b] = the block's primary index (1..n_b), 0 = not decoded (nothing written).  Block b's T goes to out + dst[b]
// (dst[b] + n_b < 2^32; out may be dL).  res[b] = 0, LIBBSC_DATA_CORRUPT or LIBBSC_NOT_SUPPORTED (0 for a block not decoded).
// adler != nullptr: adler[b] = Adler-32 of out[dst[b], dst[b] + n_b); t_host != nullptr: out[0, max(dst[b] + n_b)) also comes down
// there.  Both with the pass's last sync.
int unbwt_batch_max_blocks(int64_t cap);
int unbwt_batch_pass(bscgpu_ctx* c, const u8* dL, u8* out, const int* sizes, const int* idx, int count, const u32* dst, int* res,
                     u32* adler, u8* t_host);
int adler32_device(bscgpu_ctx* c, const u8* d, int64_t n, u32* out);
// The LZP encoder stage (lzp.hip): dIn (HBM, n bytes; may be c->dT or dOut) -> what lzp_compress returns, with the same
// bytes in dOut (HBM, n bytes; may be c->dL, not c->dT); hashSize 10..15, else BSC_NOT_SUPPORTED before anything is launched.  The
// block is copied to c->dT unless it lies there and runs as a pass of one block through the routine below.  One sync; the frame
// kernel that writes dOut is queued behind it, final_sync waits for it too.  c->lzp_last: the paths taken.
int lzp_device(bscgpu_ctx* c, const u8* dIn, u8* dOut, int n, int hashSize, int minLen, int features, bool final_sync);
// ... for `count` blocks back to back at dIn (bscgpu_lzp_batch_device without the pointer checks): results[b] = what lzp_compress returns
// for block b, the bytes at the block's own offset in dOut (dIn's layout; may be c->dL, not dIn, not c->dT).  dIn is read in place.
// The same kernels and the same driver as lzp_device's; the limits of the public batch call (include/bscgpu.h: block size, count, sum)
// are checked here.  c->lzp_last: the sums over the pass.  final_sync as above.
// place (or null): the caller packs the pass.  Called once, behind the stage's sync, with the results: it fills dst[b], where block b
// goes in dOut (preset to lzp::BATCH_NOWHERE: the block gets nothing), and as_it_is[b] != 0 where the block's raw bytes go there
// instead of a stream; the frame kernel then writes the pass as the caller laid it out (dOut: as many bytes as that takes).
typedef std::function<void(const int* results, uint32_t* dst, unsigned char* as_it_is)> LzpBatchPlace;
int lzp_batch_device(bscgpu_ctx* c, const u8* dIn, u8* dOut, const int* sizes, int count, int hashSize, int minLen, int features, int* results,
                     bool final_sync, const LzpBatchPlace* place = nullptr);
void launch_seg_scan(bscgpu_ctx* c, u32 num_chunks);
// The QLFC front end's view of the sort buffers (qlfc_front.hip).  Once a block's (a pass's) L has been emitted nothing of the sorter
// is live until the next sorter starts, and the front end and whoever reads its run arrays — the copy down, the device model — take
// these roles from here:
struct FrontBufs {
    u8*  sym;        // vA: symbol of every run (m <= n bytes of 4 n; the sort values were last read when SA was made)
    u8*  rank;       // vB: QLFC rank of every run (the values' other half)
    u32* start;      // SA: start of every run (L has been emitted from it)
    u32* first;      // ISA: a single block's first-run rows [8][256] (a pass keeps its rows in front_tab)
    u64* mask;       // kB: the symbol set of every 256 runs (the sort keys went with the values)
    u64* super;      // cpos[0]: ... of every 65536 runs (the BWT rounds' positions)
    u64* flags;      // kA: the split-flag words, read back before the run arrays are made
};
static inline FrontBufs front_bufs(const bscgpu_ctx* c)
{
    return {reinterpret_cast<u8*>(c->vA), reinterpret_cast<u8*>(c->vB), c->SA, c->ISA, c->kB, reinterpret_cast<u64*>(c->cpos[0]), c->kA};
}
int qlfc_front_split(bscgpu_ctx* c, const u8* dL, u32 n, int nblocks, int* start, int* size);
int qlfc_front_runs(bscgpu_ctx* c, const u8* dL, u32 n, int nblocks, const int* start, u32* m_out, u32* run_first, u32* first_run_host,
                    HostSlot& slot, bool copy_runs = true);
int qlfc_front_copy_runs(bscgpu_ctx* c, u32 m, HostSlot& slot);
// The front end of a whole pass: L of `count` blocks back to back at dL (16-byte aligned; sum <= max_n, every block
// below 1 MiB) -> the layout of include/bscgpu.h, without nsym / first_seen: first_run_host[256 s + c] = first run of symbol c in
// sub-block s (0xffffffff: none), which qlfc_front_first_seen turns into a sub-block's alphabet.  scratch_host: front_scratch_bytes()
// bytes, the split-flag words land there and then the first-run table (first_run_host may point into it).  Synchronous.
static_assert(FRONT_MAX_BLOCKS == BATCH_MAX_BLOCKS, "qlfc_front_plan.h plans passes of as many blocks as the sorters take");
int  qlfc_front_batch(bscgpu_ctx* c, const u8* dL, const int* sizes, int count, bscgpu_front_layout* out, void* scratch_host);
// the table qlfc_front_batch left in HBM for its last pass of nsub sub-blocks (qlfc_front_plan.h: the FT_* words)
struct FrontTab { const u32* sub_off; const u32* sub_base; u32* sub_run; const u32* first_run; };
FrontTab qlfc_front_tab(const bscgpu_ctx* c, int nsub);
int  ctx_ensure_model_host(bscgpu_ctx* c);        // both pinned stream buffers of the batch model; < 0: not to be had (the pass takes the host model)
int  ctx_ensure_front_host(bscgpu_ctx* c);        // both pinned run buffers of the batch front end; < 0: not to be had (the pass takes the L route)
int ctx_ensure_slots(bscgpu_ctx* c, int count);
int ctx_ensure_pstream_slot(bscgpu_ctx* c, HostSlot& slot, size_t entries);     // pinned landing zone for a block's p stream
int ctx_ensure_run_slot(bscgpu_ctx* c, HostSlot& slot);                           // pinned landing zone for a block's run arrays
// device-side model of the QLFC coders (devcoder.hip: dc_static_run / dc_fast_run): probability stream of a whole block from the front
// end's run arrays
int  devcoder_pstream(bscgpu_ctx* c, const u8* dsym, const u8* drank, const u32* dstart, u32 m, u32 n, int nb, const u32* run_first,
                      const int* max_rank, u32* D_out, u32* poff_out, u16* dbg, int psbuf = 0, int coder = 1 /* 1 static (-e1), 3 fast (-e0) */,
                      int* packed_out = nullptr /* non-null: the caller takes the 13-bit packed stream (devcoder.hip DcP13); *packed_out = 1 if that is what was written */);
const u16* devcoder_pstream_ptr(const bscgpu_ctx* c, int psbuf = 0);
// ... of a block in segments of whole sub-blocks ("A block in sub-block segments"), for a context whose arena is divided
// (BSCGPU_OPT_DC_ARENA_DIV > 1).  devcoder_block_begin: the facts of the block — the avg_rank flags of all its runs, every sub-block's
// decisions and undecided flags, one sync — and the plan made of them (B->plan, dc_block_plan.h); take_packed: the block's stream is
// the 13-bit form (coder 1 with BSCGPU_OPT_DC_PACKED_STREAM), else 16-bit entries.  BSC_NOT_SUPPORTED: the block is declined before any
// segment ran (c->dc_note.fail: FAIL_AVG an open flag, FAIL_CAP a sub-block alone above the capacity, 0 an arena did not fit).
// devcoder_block_segment: the model of segment g of the plan into the device p stream psbuf, laid out as g says; *host_packed: its
// packed form was void, the 16-bit entries lie there instead and the caller packs them into place (dc_pack13_host).
// BSC_NOT_SUPPORTED: the segment, and with it the block, is declined.  Either way c->dc_note is the sum over the segments run so far
// and BSCGPU_CNT_DC_BLOCK_SEGMENTS counts the ones that stayed.
struct DcBlock {
    const u8 *sym = nullptr, *rank = nullptr; const u32* start = nullptr; u32 m = 0, n = 0; int nb = 0; bool fast = false, packed = false;
    u32 maxr[8] = {}, end[8] = {} /* the byte behind each sub-block */, dec[8] = {}, und[8] = {};
    DcBlockSchedule plan;
    DcNote sum;
};
int  devcoder_block_begin(bscgpu_ctx* c, const u8* dsym, const u8* drank, const u32* dstart, u32 m, u32 n, int nb, const int* sub_start,
                          const int* sub_size, const u32* run_first, const int* max_rank, int coder, bool take_packed, DcBlock* B);
// ... the facts alone (bscgpu_qlfc_pstream_facts): B->dec / B->und, whatever the divisor; no plan, nothing declined for an open flag
int  devcoder_block_facts(bscgpu_ctx* c, const u8* dsym, const u8* drank, const u32* dstart, u32 m, u32 n, int nb, const int* sub_start,
                          const int* sub_size, const u32* run_first, const int* max_rank, int coder, DcBlock* B);
int  devcoder_block_segment(bscgpu_ctx* c, DcBlock* B, const DcBlockSeg& g, int psbuf, bool* host_packed);
int  devcoder_arena_div_set(bscgpu_ctx* c, int value);     // BSCGPU_OPT_DC_ARENA_DIV: the previous value, or a negative libbsc code
int64_t devcoder_mcap(const bscgpu_ctx* c);             // runs the device model's arena holds for this context
// ... of a whole batched pass ("The static coder's model of a pass"): after qlfc_front_batch, from the run arrays and the
// table it left in HBM -> *D_out decisions in devcoder_pstream_ptr(c, 0), sub-block s's at [poff[s], poff[s + 1]) with poff[0..nsub] at
// devcoder_batch_poff_ptr (device).  BSC_NOT_SUPPORTED: the pass is declined (c->dc_note.fail: BSCGPU_DC_FAIL_*; 0: an arena did not
// fit).  Synchronous.  coder 3: the fast coder's (-e0) model of the pass — same inputs, same outputs with entries in the dcm::PSF_*
// form, same exits (only FAIL_CAP and FAIL_REPLAY can be raised: this coder has no avg_rank flags and no run_hist look-back)
// packed_out non-null (coder 1): the stream may be left in the packed 13-bit form of a pass ("The packed stream of a pass");
// *packed_out = 1: it was — pbase[0..nsub] at devcoder_batch_pbase_ptr (device), *pbytes_out = pbase[nsub] / 8 * 13 bytes in the
// stream buffer; 0: the packed form was void and the 2-byte entries are there instead
// coder 2: the adaptive coder's (-e2) — the static model with the adaptive rates (the run_hist resolve always on: never FAIL_HIST),
// then one walk per mixer chain; entries in the static coder's form; FAIL_MIX when the longest chain exceeds c->dc_mix_cap; the four
// debug planes [4][*D_out] (state / char / static counter values, mixer id) stay at devcoder_mix_dbg_ptr (device)
int  devcoder_pstream_batch(bscgpu_ctx* c, u32 m, int nsub, int coder /* 1 static (-e1), 2 adaptive (-e2), 3 fast (-e0) */, u32* D_out,
                            int* packed_out = nullptr, int64_t* pbytes_out = nullptr);
const u16* devcoder_mix_dbg_ptr(const bscgpu_ctx* c);
const u32* devcoder_batch_poff_ptr(const bscgpu_ctx* c);
const u32* devcoder_batch_pbase_ptr(const bscgpu_ctx* c);
// ... of a pass in model segments ("Model segments"): the same inputs plus the layout's blk_sub[count + 1] and
// sub_run[nsub + 1] (host), coder 1, 2 or 3, target decisions per segment (<= 0: the arena's capacity).  out[0 .. cap) (host): the kept
// sub-blocks' entries back to back in sub-block order, poff[0..nsub] (host; a sub-block that was not modelled is empty), blk_state[b] =
// 0 or the BSCGPU_DC_FAIL_* mask that leaves block b to the host model.  per_segment_fit: a segment that no longer fits behind the
// ones before it is left to the host; else a total above cap is counted, not copied.  *D_out: decisions kept.  BSC_NOT_SUPPORTED: an
// arena did not fit.  Moves the segment counters of the context.  Synchronous.
// coder 2: every segment is the static model with the adaptive rates and then the mixers' walk; a block with a mixer chain above
// c->dc_mix_cap is left out by the plan (FAIL_MIX per BLOCK), c->dc_mix_chains / _longest / _walk_us say sum / maximum / sum of the kept segments.
// note (or null): told as the pass settles, on the calling thread, so that coding can start before the last segment.  planned(): the
// plan is known, blk_state holds the excluded blocks.  settled(b0, b1): the blocks of [b0, b1) with a sub-block are final — their
// entries have landed in out and their poff entries are written, or blk_state gives them to the host.  Every planned block is settled
// exactly once before a return >= 0; after planned(), blk_state and poff of settled blocks are not written again.
struct DcSegNote {
    void (*planned)(void* user);
    void (*settled)(void* user, int b0, int b1);
    void* user;
};
int  devcoder_pstream_segments(bscgpu_ctx* c, u32 m, int nsub, const int* blk_sub, int count, const u32* sub_run, int coder, int64_t target,
                               void* out, int64_t cap, bool per_segment_fit, u32* poff, int* blk_state, int64_t* D_out,
                               const DcSegNote* note = nullptr, int64_t* pbase = nullptr /* non-null: the packed form, out / cap in bytes */);
// ... the facts the plan is made of alone: dec[s] / und[s] (host, nsub entries each) of the pass qlfc_front_batch just laid out
int  devcoder_segment_facts(bscgpu_ctx* c, u32 m, int nsub, int coder, u32* dec, u32* und, u32* mix = nullptr);   // (mix: coder 2, and only then)
int64_t devcoder_dcap(const bscgpu_ctx* c);             // decisions the device model's arena holds for this context
int64_t devcoder_batch_bytes(const bscgpu_ctx* c);      // HBM the batch model added on its first use
void devcoder_destroy(bscgpu_ctx* c);
// the range coder stage on c->stream (rangecoder.hip): bscgpu_rc_encode_device without the argument check; synchronous
int  rc_encode_device(bscgpu_ctx* c, int form, const void* dBody, const u32* prefix, int nprefix_total, const bscgpu_rc_stream* streams,
                      int count, void* dOut, int* res, int streams_per_wave);
int64_t devcoder_arena_bytes(const bscgpu_ctx* c);
void devcoder_warm_tables();               // starts the model tables' computation on a background thread (first context of the process)

// ---------------------------------------------------------------------------------------------
// Device helpers (wave64)
// ---------------------------------------------------------------------------------------------
#ifdef __HIPCC__
__device__ __forceinline__ u32 lane_id() { return __lane_id(); }

// Block of position i in a batch's offset table off[0..count] (bwt.hip, st.hip): the largest b in [lo, hi) with off[b] <= i, given
// off[lo] <= i.  Empty blocks share an offset: the last such block wins, so the block found holds i.
__device__ __forceinline__ u32 batch_block_of(const u32* __restrict__ off, u32 lo, u32 hi, u32 i)
{
    while (hi - lo > 1) { const u32 mid = (lo + hi) >> 1; if (off[mid] <= i) lo = mid; else hi = mid; }
    return lo;
}
__device__ __forceinline__ u32 batch_block_of(const u32* __restrict__ off, u32 count, u32 i) { return batch_block_of(off, 0u, count, i); }

__device__ __forceinline__ u64 lanemask_lt() {
    u32 l = lane_id();
    return (l == 0) ? 0ull : (~0ull >> (64 - l));
}

// Inclusive wave64 scans on the DPP network (row shifts inside the rows of 16, then the two row broadcasts): six dependent VALU operations.
// ALL 64 LANES MUST BE ACTIVE (every caller scans whole wavefronts).  Round 6: the ds_bpermute form these replace (kept below as *_bperm)
// is six LDS round trips, each waited for — ~700 cycles per scan on the critical path of every tile of the device coder's partition kernels
// (four wavefronts per SIMD: nothing to hide it behind) and of every block scan of the chunked kernels.
__device__ __forceinline__ u32 wave_incl_sum(u32 v) {
    v += (u32)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, true);      // row_shr:1
    v += (u32)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, true);      // row_shr:2
    v += (u32)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, true);      // row_shr:4
    v += (u32)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, true);      // row_shr:8
    v += (u32)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xa, 0xf, false);     // row_bcast:15 -> rows 1 and 3
    v += (u32)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xc, 0xf, false);     // row_bcast:31 -> rows 2 and 3
    return v;
}
__device__ __forceinline__ u32 wave_incl_max(u32 v) {
    auto mx = [](u32 a, u32 b) { return a > b ? a : b; };                         // (lanes without a source read 0: the identity of an unsigned max)
    v = mx(v, (u32)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, true));
    v = mx(v, (u32)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, true));
    v = mx(v, (u32)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, true));
    v = mx(v, (u32)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, true));
    v = mx(v, (u32)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xa, 0xf, false));
    v = mx(v, (u32)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xc, 0xf, false));
    return v;
}
__device__ __forceinline__ u32 wave_incl_sum_bperm(u32 v) {
    u32 l = lane_id();
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        u32 t = __shfl_up(v, d, 64);
        if (l >= (u32)d) v += t;
    }
    return v;
}

// Block (256 threads) exclusive sum scan.  lds must hold >= 8 u32.  Returns exclusive prefix of v;
// *total receives the block total.  Contains __syncthreads(); all threads must call.
__device__ __forceinline__ u32 block_excl_sum(u32 v, u32* lds, u32* total) {
    u32 incl = wave_incl_sum(v);
    u32 w = threadIdx.x >> 6, l = lane_id();
    __syncthreads();                 // protect lds reuse from a previous call
    if (l == 63) lds[w] = incl;
    __syncthreads();
    u32 base = 0, tot = 0;
#pragma unroll
    for (int i = 0; i < WAVES; ++i) { u32 t = lds[i]; if ((u32)i < w) base += t; tot += t; }
    *total = tot;
    return base + incl - v;
}
// Block inclusive max scan.
__device__ __forceinline__ u32 block_incl_max(u32 v, u32* lds, u32* total) {
    u32 incl = wave_incl_max(v);
    u32 w = threadIdx.x >> 6, l = lane_id();
    __syncthreads();
    if (l == 63) lds[w] = incl;
    __syncthreads();
    u32 base = 0, tot = 0;
#pragma unroll
    for (int i = 0; i < WAVES; ++i) { u32 t = lds[i]; if ((u32)i < w) base = (t > base) ? t : base; tot = (t > tot) ? t : tot; }
    *total = tot;
    return (base > incl) ? base : incl;
}
#endif
