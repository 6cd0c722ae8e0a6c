/*
 * bscgpu.h — thin C ABI between libbsc-style host code and the MI355X (gfx950) HIP kernels.
 *
 * This is the drop-in boundary for the reference's GPU plug points.  Each entry point names the
 * reference interface it replaces (paths relative to the reference tree, libbsc 3.3.5):
 *
 *   bscgpu_create / bscgpu_destroy   <->  libcubwt_allocate_device_storage / libcubwt_free_device_storage
 *                                         (libbsc/bwt/libcubwt/libcubwt.cuh:60-71; called from bwt.cpp:92-115)
 *   bscgpu_bwt                       <->  libcubwt_bwt      (libcubwt.cuh:73-80,  bwt.cpp:148-162)
 *   bscgpu_bwt_aux                   <->  libcubwt_bwt_aux  (libcubwt.cuh:82-89,  bwt.cpp:104-118)
 *   bscgpu_st_encode                 <->  bsc_st_encode_cuda (libbsc/st/st.cuh:57, st.cpp:998-1002)
 *
 * Like the reference hooks these take HOST pointers, do their own H2D/D2H and are synchronous on
 * return.  The *_device variants take DEVICE pointers (input already resident in HBM) and are what
 * bench.py times; they have no counterpart in the reference (its coder never leaves the CPU).
 *
 * Plain C, plain pointers and sizes.  Return values follow libbsc.h:41-51 (>= 0 ok, < 0 error code;
 * -7 GPU_ERROR, -8 GPU_NOT_SUPPORTED, -9 GPU_NOT_ENOUGH_MEMORY, -1 BAD_PARAMETER).
 */
#ifndef BSCGPU_H
#define BSCGPU_H

#include <stddef.h>
#include <stdint.h>

#if defined(__GNUC__)
#define BSCGPU_API __attribute__((visibility("default")))
#else
#define BSCGPU_API
#endif

#ifdef __cplusplus
extern "C" {
#endif

typedef struct bscgpu_ctx bscgpu_ctx;

/* Number of visible HIP devices (0 when there is no usable GPU). */
BSCGPU_API int bscgpu_device_count(void);

/* Create a per-device context with an HBM arena large enough for blocks of up to max_n bytes.
 * One context per GPU (one process per GPU in the multi-GPU driver); a context is not re-entrant:
 * serialise calls on it (the reference serialises on one global lock, bwt.cpp:50-52). */
BSCGPU_API int  bscgpu_create(bscgpu_ctx** ctx, int device, int64_t max_n);
BSCGPU_API void bscgpu_destroy(bscgpu_ctx* ctx);

/* Bytes of device memory held by the context's arena. */
BSCGPU_API int64_t bscgpu_arena_bytes(const bscgpu_ctx* ctx);
/* Bytes of the device model's own arena (carved on the first -e1 / -e0 block or pass that takes the device model, for
 * ceil(max_n / BSCGPU_OPT_DC_ARENA_DIV); 0 before that).  bscgpu_arena_bytes does not count it. */
BSCGPU_API int64_t bscgpu_model_arena_bytes(const bscgpu_ctx* ctx);

/* ---- forward BWT ------------------------------------------------------------------------- */
/* L may alias T.  Returns the primary index (1..n) like libcubwt_bwt, or a negative error. */
BSCGPU_API int64_t bscgpu_bwt(bscgpu_ctx* ctx, const uint8_t* T, uint8_t* L, int64_t n);
/* As above plus auxiliary indexes: r is a power of two, I[0..(n-1)/r] receives 1-based ranks
 * (I[0] = primary index), exactly libsais_bwt_aux / libcubwt_bwt_aux semantics.  Returns 0. */
BSCGPU_API int64_t bscgpu_bwt_aux(bscgpu_ctx* ctx, const uint8_t* T, uint8_t* L, int64_t n, int64_t r, uint32_t* I);
/* Device-resident variant: dT, dL are device pointers (may alias); I is a HOST array or NULL
 * (r ignored when I is NULL).  Returns the primary index. */
BSCGPU_API int64_t bscgpu_bwt_device(bscgpu_ctx* ctx, const void* dT, void* dL, int64_t n, int64_t r, uint32_t* I);
/* The first sort of that transform alone (tests): byte histogram, key packing and the radix sort on the packed prefix keys exactly as
 * bscgpu_bwt_device runs them for this block, the n sorted (u64 key, u32 value) records copied to d_keys_out / d_vals_out (device
 * pointers).  Returns 0 or a negative libbsc code. */
BSCGPU_API int bscgpu_bwt_first_sort_device(bscgpu_ctx* ctx, const void* dT, int64_t n, void* d_keys_out, void* d_vals_out);

/* ---- inverse BWT (libcubwt_unbwt's role, libcubwt.cuh:91-104; reached from bsc_bwt_decode, bwt.cpp:233-281) ---------- */
/* L[0..n) and the 1-based primary index as bsc_bwt_encode writes them -> T[0..n); host pointers, may alias; synchronous.
 * Returns 0, LIBBSC_DATA_CORRUPT (-6) when the rows 0..n do not form one cycle through the sentinel row (T is then not written; the
 * same verdict, and on 0 the same text, as bsc_bwt_decode's host walk), LIBBSC_NOT_SUPPORTED (-4) when a piece of the cycle between two
 * marked rows is longer than the step cap (T not written: use the host walk), or another libbsc code.
 * BSC_UNBWT_STEP_CAP in the environment (read when a context is created; values below 16 are ignored): the step cap, 1 << 22 by
 * default.  A test knob: no constructible input reaches the default, so a small cap is what drives the LIBBSC_NOT_SUPPORTED exits. */
BSCGPU_API int bscgpu_unbwt(bscgpu_ctx* ctx, const uint8_t* L, uint8_t* T, int64_t n, int64_t index);

/* ---- Sort Transform (order k = 3..8) ----------------------------------------------------- */
/* In place on host T[0..n).  Returns the 0-based primary index like bsc_st_encode (st.cpp:990). */
BSCGPU_API int bscgpu_st_encode(bscgpu_ctx* ctx, uint8_t* T, int n, int k);
BSCGPU_API int bscgpu_st_encode_device(bscgpu_ctx* ctx, const void* dT, void* dOut, int n, int k);

/* ---- Adler-32 of a device buffer (adler32.cpp:82) ---------------------------------------- */
BSCGPU_API int bscgpu_adler32_device(bscgpu_ctx* ctx, const void* dT, int64_t n, uint32_t* out);

/* ---- LSD radix sort primitive (the kernel the roofline is measured on) -------------------- */
/* Stable sort of n (u64 key, u32 value) records on key bits [begin_bit, end_bit), 8-bit digits.
 * All pointers are device pointers; *_alt are same-sized scratch (ping-pong).  vals may be NULL
 * (keys-only).  On return *result_in_alt is 1 when the sorted data lives in the *_alt buffers. */
BSCGPU_API int bscgpu_radix_sort_u64(bscgpu_ctx* ctx, void* keys, void* keys_alt, void* vals, void* vals_alt,
                          int64_t n, int begin_bit, int end_bit, int* result_in_alt);

/* ---- QLFC static coder (-e1): the adaptive model on the GPU --------------------------------- */
/* Stage function: sorted host block L[0..n) -> sub-block split (coder.cpp:70-109) + run/rank front end (qlfc.cpp:398-455)
 * + every probability of the static model (qlfc.cpp:896-1126, predictor.h:53-61,121) as a stream of 16-bit entries
 * {[11:0] probability, [12] coded bit, [13] first decision of a run}, stream order, all sub-blocks back to back
 * (poff[b]..poff[b+1] = sub-block b).  Returns the number of decisions, LIBBSC_NOT_SUPPORTED (-4) when the block has to take
 * the host model (a context bracket that does not close, a chain that would be replayed over more than 64 chunks, capacity;
 * bscgpu_last_error and BSCGPU_CNT_DC_LAST_FAIL say which), or a negative libbsc code.
 * dbg (optional, [3][cap]): the state- / char- / static-counter value behind every decision. */
BSCGPU_API int64_t bscgpu_qlfc_static_pstream(bscgpu_ctx* ctx, const uint8_t* L, int n, uint16_t* out, int64_t cap, int* nblocks,
                                   int* sub_start /*[8]*/, int* sub_size /*[8]*/, int64_t* poff /*[9]*/, uint16_t* dbg);
/* The same stage with the stream in the form that crosses PCIe since round 6 (BSCGPU_OPT_DC_PACKED_STREAM): 13 bits per decision
 * {[11:0] probability, [12] coded bit}, eight decisions in 13 bytes (field e of a group at bits [13 e, 13 e + 13), little endian); sub-block
 * b's fields start at decision pbase[b] of the packed space — a multiple of 64, i.e. at byte pbase[b] / 8 * 13 — and its last group is
 * zero-padded.  out takes pbase[nblocks] / 8 * 13 bytes (cap_bytes).  Returns the number of decisions; LIBBSC_NOT_SUPPORTED also when
 * the packed form was not produced for this block (option off; 64 consecutive runs with more decisions than a wavefront stages —
 * bsc_compress then moves that block's stream as 16-bit entries). */
BSCGPU_API int64_t bscgpu_qlfc_static_pstream_packed(bscgpu_ctx* ctx, const uint8_t* L, int n, uint8_t* out, int64_t cap_bytes, int* nblocks,
                                   int* sub_start /*[8]*/, int* sub_size /*[8]*/, int64_t* poff /*[9]*/, int64_t* pbase /*[9]*/);

/* ---- range coder: many probability streams in one launch -------------------------
 * The back half of the static / fast coders as a stage of its own: a stream is a prefix (the header word and the alphabet, as plain
 * entries) followed by a body in one of the three forms the device model writes.  One lane codes one stream; the bytes are those of
 * the host coders of the same form (rangecoder.h:38-271: 32-bit range, 64-bit low with the carry in bit 32, 16-bit little-endian
 * units, finish = one conditional and three unconditional shifts).
 *   prefix entry (u32)   [15:0] multiplier p, [20:16] precision, [24] coded bit: range' = (range >> precision) * p for a 0 bit
 *   bscgpu_rc_prefix     pure function: the decisions qlfc_encode_pstream (the static forms for coder 1, the fast form for coder 3)
 *                        issue before the body — EncodeWord(in_size) at precision 12, p 2048, then the alphabet (csrc/host/qlfc.cpp: encode_alphabet) at
 *                        precision 12, p 2048 (static) or precision 1, p 1 (fast).  Returns the count (at most BSCGPU_RC_PREFIX_MAX; entries
 *                        may be NULL to ask for it) or LIBBSC_BAD_PARAMETER (cap too small included).
 * Stopping rule of a stream, per form (full = bytes written >= out_size - 16, rangecoder.h:127): STATIC16 gives up at a run-start
 *   mark once full, STATIC13 at any body decision once full, FAST16 at a run-start mark once full — what the host coder of the same
 *   form does.  On top of that no stream ever stores outside out[out_off, out_off + out_size + 64): a renormalisation (and the
 *   finish) that finds bytes written + 2 * pending units + 10 > out_size + 64 ends the stream instead.  Either way res = LIBBSC_NOT_COMPRESSIBLE.
 * res[i] = bytes written, or LIBBSC_NOT_COMPRESSIBLE.  The calls return 0, LIBBSC_BAD_PARAMETER (nothing launched) or a GPU error.
 * bscgpu_rc_encode_host   the CPU stand-in (no GPU, no context): the same streams through the scalar range encoder of the host coders.
 * bscgpu_rc_encode_device dBody / dOut device pointers (dOut 2-byte aligned), prefix / streams / res host arrays; streams_per_wave =
 *                        64, 8 or 1 streams per wavefront (same bytes; 1 keeps a chain wave-uniform).  Synchronous.  A body is read
 *                        in aligned 16-byte pieces: at most 15 bytes before its first and after its last byte are touched.
 * bscgpu_rc_encode       the same with host pointers for body (body_bytes of it) and out (out_bytes): copies up and down. */
#define BSCGPU_RC_STATIC16 0  /* dcm::PS_*: [11:0] p, [12] bit, [13] run start, precision 12 */
#define BSCGPU_RC_STATIC13 1  /* DcP13: 13 bits per decision {[11:0] p, [12] bit}, eight in 13 bytes */
#define BSCGPU_RC_FAST16   2  /* dcm::PSF_*: [12:0] p, [13] bit, [14] run start, [15] side: precision 11, else 13 */
#define BSCGPU_RC_REFILL   128   /* decisions a wavefront stages per stream and refill (a multiple of 8) */
#define BSCGPU_RC_PREFIX_MAX (32 + 256 * 8)
typedef struct bscgpu_rc_stream {
    int64_t  body;      /* first body entry (16-bit forms: entry index; packed: decision index in the packed space, multiple of 8) */
    uint32_t count;     /* body decisions, may be 0 */
    uint32_t prefix, nprefix;   /* range in the call's prefix array */
    uint32_t out_off;   /* even; the stream owns out[out_off .. out_off + out_size + 64) */
    int32_t  out_size;  /* the reference's outputSize; budget = out_size - 16 (rangecoder.h:127) */
} bscgpu_rc_stream;
BSCGPU_API int bscgpu_rc_prefix(const unsigned char* first_seen, int nsym, int in_size, int coder, uint32_t* entries, int cap);
BSCGPU_API int bscgpu_rc_encode_host(int form, const void* body, const uint32_t* prefix, int nprefix_total,
                                     const bscgpu_rc_stream* streams, int count, void* out, int* res);
BSCGPU_API int bscgpu_rc_encode_device(bscgpu_ctx* ctx, int form, const void* dBody, const uint32_t* prefix, int nprefix_total,
                                       const bscgpu_rc_stream* streams, int count, void* dOut, int* res, int streams_per_wave);
BSCGPU_API int bscgpu_rc_encode(bscgpu_ctx* ctx, int form, const void* body, int64_t body_bytes, const uint32_t* prefix, int nprefix_total,
                                const bscgpu_rc_stream* streams, int count, void* out, int64_t out_bytes, int* res, int streams_per_wave);
/* The argument check of the three calls as a pure function: 0 or LIBBSC_BAD_PARAMETER (a form or stream shape outside the above;
 * body_bytes / out_bytes < 0: that extent is not checked). */
BSCGPU_API int bscgpu_rc_check(int form, int nprefix_total, const bscgpu_rc_stream* streams, int count, int64_t body_bytes, int64_t out_bytes);

/* ---- full block compression with the BWT/ST + coder split across GPU and host ------------- */
/* bsc_compress semantics (libbsc.cpp:213) for input already in HBM: Adler-32 + sort transform on
 * the GPU, QLFC coder on host threads.  output is a HOST buffer of n + 28 bytes. */
BSCGPU_API int bscgpu_compress_device(bscgpu_ctx* ctx, const void* dInput, uint8_t* output, int n,
                           int blockSorter, int coder, int features);

/* bscgpu_compress_device with the LZP stage in front (bsc_compress's full parameter list for input in HBM): the Adler-32 of the original
 * comes from the device kernel, bscgpu_lzp_compress_device's stage writes the sorter's input.  A chunk-level or block-level
 * LIBBSC_NOT_COMPRESSIBLE lets the block go on without LZP (libbsc.cpp:266-269); LIBBSC_NOT_SUPPORTED where the stage declines
 * (lzpHashSize >= 16).  lzpHashSize == 0 and lzpMinLen == 0: bscgpu_compress_device.  Same bytes as bsc_compress of the same input. */
BSCGPU_API int bscgpu_compress_device_lzp(bscgpu_ctx* ctx, const void* dInput, uint8_t* output, int n, int lzpHashSize, int lzpMinLen,
                           int blockSorter, int coder, int features);

/* ---- the LZP encoder stage on the GPU ------------------------------------------
 * bscgpu_lzp_compress_device: what bsc_lzp_compress returns for the n bytes at dIn (HBM), with the same bytes in dOut (HBM, n bytes; may
 *   be dIn) — or LIBBSC_NOT_SUPPORTED, before anything is launched, for hashSize >= 16: the stage holds a chunk's table in LDS and covers
 *   the narrow scanners only.  Both framings (features & LIBBSC_FEATURE_MULTITHREADING) are exact.  BSCGPU_CNT_LZP_MATCHES.. say which
 *   paths the block took.  n <= the context's max_n.  Memory: the stage's tables, as for bscgpu_lzp_batch_device below — the same
 *   allocation, made by whichever call comes first.
 * bscgpu_lzp_compress: the same with host pointers (out: n bytes).
 * bscgpu_lzp_staged_host: the CPU stand-in — the stage's three steps (links, flags, the sweep with its dirty marks and the real table:
 *   written for every visited position, read by dirty positions only) as the device runs them, on the calling thread; no GPU, no context.  counters (or NULL): five values in the order of
 *   BSCGPU_CNT_LZP_MATCHES .. _RAW_CHUNKS. */
BSCGPU_API int bscgpu_lzp_compress_device(bscgpu_ctx* ctx, const void* dIn, void* dOut, int n, int hashSize, int minLen, int features);
BSCGPU_API int bscgpu_lzp_compress(bscgpu_ctx* ctx, const uint8_t* in, uint8_t* out, int n, int hashSize, int minLen, int features);
BSCGPU_API int bscgpu_lzp_staged_host(const uint8_t* in, uint8_t* out, int n, int hashSize, int minLen, int features, int64_t* counters);

/* ---- the LZP stage for all blocks of a pass ("A pass of small blocks") ----------
 * bscgpu_lzp_batch_device: `count` blocks back to back at dIn (HBM), as in the other batch calls.  results[b] = what
 *   bsc_lzp_compress(block b, hashSize, minLen, features) returns, a size or LIBBSC_NOT_COMPRESSIBLE; where it is a size the same bytes
 *   lie in dOut (HBM, dIn's layout, sizes[b] bytes per block) at the block's own offset.  One key kernel, one sort, one link and one
 *   flag kernel and one sweep with a workgroup per chunk for the whole pass; one copy of the chunks' results down, one sync, one gather
 *   kernel for all frames.  dIn and dOut must not overlap; dIn is not modified.  Limits: count <= BSCGPU_ST_BATCH_MAX_BLOCKS, every
 *   sizes[b] < BSCGPU_BATCH_MAX_N, the sum <= the context's max_n, hashSize 10..15 — hashSize >= 16: LIBBSC_NOT_SUPPORTED before
 *   anything is launched; every other violation: LIBBSC_BAD_PARAMETER, nothing written.  Returns 0 or such a batch-level error.
 *   BSCGPU_CNT_LZP_MATCHES .. _RAW_CHUNKS are the sums over the call's blocks.  Memory: on first use a context allocates the stage's
 *   tables (709 KB of HBM, counted by bscgpu_arena_bytes from then on, and as much pinned host memory).
 * bscgpu_lzp_batch_plan: the chunk table of such a pass as a pure function, one entry per chunk in pass order (arrays of 8192): its
 *   block, its first byte in the pass, its size, and the bytes its sweep may write (sizes[b] - 2 for a block that is one chunk).  An
 *   empty block, or one the encoder refuses by size (n - minLen < 32 or n - 2 < 16), owns no chunk.  Returns the number of chunks, or
 *   LIBBSC_BAD_PARAMETER (count above 4096, a size negative or not below BSCGPU_BATCH_MAX_N, a sum of 2^31 - 1 or more, minLen outside
 *   4..255) with nothing written.
 * bscgpu_lzp_batch_frame: the frames of the pass from its chunks' own results own[k] (chunk k of the plan: its sweep's size or a
 *   negative code), both framings: results[b] as above, and the list of pieces one gather kernel moves (arrays of 3 * 4096): source
 *   (0 the sweep's staging area, 1 the raw input, 2 the table bytes), offset in the source (staging and input: in the pass), offset in
 *   the output, length.  table: count * 17 bytes, the blocks' tables one behind the other.  raw_chunks (or NULL): chunks kept raw.
 *   Returns the number of pieces.
 * bscgpu_lzp_chunk_staged_host: the CPU stand-in's sweep of ONE chunk of n bytes under a budget of cap bytes -> its size (the bytes in
 *   out, n bytes) or LIBBSC_NOT_COMPRESSIBLE: own[k] of the two calls above.  counters as bscgpu_lzp_staged_host's. */
BSCGPU_API int bscgpu_lzp_batch_device(bscgpu_ctx* ctx, const void* dIn, void* dOut, const int* sizes, int count, int hashSize, int minLen,
                                       int features, int* results);
BSCGPU_API int bscgpu_lzp_batch_plan(const int* sizes, int count, int minLen, int* chunk_block, int* chunk_start, int* chunk_size, int* chunk_cap);
BSCGPU_API int bscgpu_lzp_batch_frame(const int* sizes, int count, int minLen, int features, const int* own, int* results, int* piece_src,
                                      int* piece_src_off, int* piece_dst_off, int* piece_len, unsigned char* table, int64_t* raw_chunks);
BSCGPU_API int bscgpu_lzp_chunk_staged_host(const uint8_t* in, uint8_t* out, int n, int cap, int hashSize, int minLen, int64_t* counters);

/* ---- batches of small blocks: one suffix sort for many blocks ------------------------------
 * Blocks are laid out back to back: block b starts at off_b = sizes[0] + ... + sizes[b-1].  Blocks below
 * BSCGPU_BATCH_MAX_N that the BWT sorts share one suffix sort per pass (at most max_n bytes and 4096 blocks,
 * consecutive blocks), blocks below BSCGPU_ST_BATCH_MAX_N that ST3..ST8 sort share one sort transform per pass
 * (the same limits); every other block takes the single-block path inside the same call.  Output is
 * byte-identical to the single-block calls.  The context stays non-re-entrant.
 *
 * bscgpu_bwt_batch_device: dT / dL device pointers (may alias, dL in dT's layout).  primary[b] = what
 *   bsc_bwt_encode returns for block b alone (error codes included); with num_indexes != NULL, num_indexes[b]
 *   and indexes[16 b ..] are its aux indexes (at most 15).  Returns 0 or a batch-level error (bad arguments, GPU).
 * bscgpu_compress_batch: host input; block b's output region starts at off_b + 28 b and holds sizes[b] + 28
 *   bytes; results[b] = what bsc_compress(block b, ...) returns, with the same bytes — except for a block larger
 *   than the context's max_n, which gets LIBBSC_GPU_NOT_ENOUGH_MEMORY (the call does not resize its context).
 *   input and output must not overlap.  Returns 0 or a batch-level error (bad arguments: nothing written; a GPU failure).
 * bscgpu_compress_batch_device: the same for input in HBM, without LZP, results as bscgpu_compress_device's (a block
 *   larger than max_n: LIBBSC_BAD_PARAMETER).  Passes are sorted straight from dInput; checksums come from one
 *   segmented Adler-32 launch per pass; only L (and a stored block's own bytes) crosses PCIe.
 * bscgpu_compress_batch_device_lzp: the same with bsc_compress's full parameter list.  Per pass one run of bscgpu_lzp_batch_device's
 *   stage writes the sorter's input, the blocks' LZP streams back to back as the host route lays them out; a block the
 *   stage finds not compressible goes on without LZP (libbsc.cpp:266-269); blocks outside a pass go one by one through
 *   bscgpu_compress_device_lzp.  lzpHashSize == 0 and lzpMinLen == 0: bscgpu_compress_batch_device.  lzpHashSize >= 16:
 *   LIBBSC_NOT_SUPPORTED at batch level, nothing written.  Same bytes as bsc_compress of every block.
 * Memory: on first use a context allocates the batch table (311 KB of HBM, counted by bscgpu_arena_bytes from then
 *   on) and two pinned host buffers of max_n bytes each (not HBM; kept until bscgpu_destroy).
 * bscgpu_batch_plan: the routing rule as a pure function: pass_of[b] = the pass of block b, or -1 for the
 *   single-block path; returns the number of passes (cap = the context's max_n). */
#define BSCGPU_BATCH_MAX_N (1 << 20)       /* = the device-model threshold; the batched route beats the call's per-block route below it */
BSCGPU_API int bscgpu_batch_plan(const int* sizes, int count, int blockSorter, int64_t cap, int* pass_of);
/* The sort transform's batch: one sort of the records of many blocks per pass, block-cyclic contexts.
 * bscgpu_st_batch_plan: the ST routing rule as a pure function (bscgpu_batch_plan keeps answering for the BWT only): blocks of
 *   1 .. BSCGPU_ST_BATCH_MAX_N - 1 bytes and at most cap bytes join passes of consecutive blocks, at most cap bytes and
 *   BSCGPU_ST_BATCH_MAX_BLOCKS blocks each (every k the same); pass_of[b] = -1 for larger blocks (they end a pass) and for empty
 *   ones (an empty entry inside a pass).  Returns the number of passes; k outside 3..8 or a negative size: LIBBSC_BAD_PARAMETER,
 *   nothing written.
 * bscgpu_st_batch_device: dT / dOut device pointers, blocks back to back, may alias (dOut in dT's layout).  index[b] = what
 *   bsc_st_encode returns for block b alone (0 for n_b <= 1, bytes unchanged; a block larger than max_n: LIBBSC_BAD_PARAMETER as
 *   bscgpu_st_encode_device, its bytes not written).  Returns 0 or a batch-level error (bad arguments: nothing written; GPU). */
#define BSCGPU_ST_BATCH_MAX_N BSCGPU_BATCH_MAX_N
#define BSCGPU_ST_BATCH_MAX_BLOCKS 4096
BSCGPU_API int bscgpu_st_batch_plan(const int* sizes, int count, int k, int64_t cap, int* pass_of);
BSCGPU_API int bscgpu_st_batch_device(bscgpu_ctx* ctx, const void* dT, void* dOut, const int* sizes, int count, int k, int* index);
BSCGPU_API int bscgpu_bwt_batch_device(bscgpu_ctx* ctx, const void* dT, void* dL, const int* sizes, int count, int* primary,
                                       unsigned char* num_indexes, int* indexes);
BSCGPU_API int bscgpu_compress_batch(bscgpu_ctx* ctx, const unsigned char* input, const int* sizes, int count, unsigned char* output,
                                     int* results, int lzpHashSize, int lzpMinLen, int blockSorter, int coder, int features);
BSCGPU_API int bscgpu_compress_batch_device(bscgpu_ctx* ctx, const void* dInput, const int* sizes, int count, unsigned char* output,
                                            int* results, int blockSorter, int coder, int features);
BSCGPU_API int bscgpu_compress_batch_device_lzp(bscgpu_ctx* ctx, const void* dInput, const int* sizes, int count, unsigned char* output,
                                                int* results, int lzpHashSize, int lzpMinLen, int blockSorter, int coder, int features);

/* ---- the QLFC front end of a whole pass ---------------------------------------
 * What bsc_coder_compress does to a sorted block before any entropy coding — the sub-block split (coder.cpp:70-109), the run scan
 * and the backward move-to-front rank (qlfc.cpp:398-455) — for every block of a pass at once, as flat arrays in ONE run index space.
 * The caller owns every array of the layout and sets the pointers before the call; N = Σ sizes[b]:
 *   blk_sub   [count + 1]   first sub-block of block b; block b has blk_sub[b + 1] - blk_sub[b] sub-blocks (0 for an empty block,
 *                           else coder_num_blocks(n_b): 1 below 256 KiB, 2 from there on); blk_sub[count] = nsub
 *   sub_start [2 count]     sub-block s: its first byte, relative to ITS BLOCK's first byte ...
 *   sub_size  [2 count]     ... and its length
 *   sub_run   [2 count + 1] runs sub_run[s] .. sub_run[s + 1] - 1 are sub-block s's; sub_run[nsub] = m
 *   nsym      [2 count]     distinct symbols of sub-block s ...
 *   first_seen[2 count][256] ... and those symbols in order of first appearance (the stream's alphabet header): entries [256 s, 256 s + nsym[s])
 *   sym, rank [N]           run j: its symbol and its QLFC rank (the last run of every sub-block has rank 1)
 *   start     [N]           run j: its first byte, relative to its block's first byte (a run ends where the next one starts, the
 *                           last run of a sub-block at sub_start + sub_size); a head is forced at every sub-block start
 * nsub and m are written by the call.  This is the layout the compress-batch calls use internally.
 * bscgpu_qlfc_front_batch_device: dL = L of `count` sorted blocks back to back in HBM, under a pass's limits (count <= 4096, every
 *   block below BSCGPU_BATCH_MAX_N, N <= max_n).  Synchronous.  Returns 0, LIBBSC_BAD_PARAMETER, or a GPU error.
 * bscgpu_front_batch_host: the same layout built on the CPU from the reference's own rules (no GPU, no context) — the stand-in
 *   the tests compare the device stage against.
 * bscgpu_front_batch_code: codes block `block` of a layout into out (sizes[block] + 4096 bytes): what bsc_coder_compress(L_b, out,
 *   n_b, coder, features) returns and writes; a sub-block that has to be stored raw is rebuilt from its runs.  Thread-safe for
 *   different blocks of one layout. */
typedef struct bscgpu_front_layout {
    int count, nsub;
    int64_t m;
    const int* sizes;
    int* blk_sub;
    int* sub_start;
    int* sub_size;
    uint32_t* sub_run;
    int* nsym;
    uint8_t* first_seen;
    uint8_t* sym;
    uint8_t* rank;
    uint32_t* start;
} bscgpu_front_layout;
BSCGPU_API int bscgpu_qlfc_front_batch_device(bscgpu_ctx* ctx, const void* dL, const int* sizes, int count, bscgpu_front_layout* out);
BSCGPU_API int bscgpu_front_batch_host(const unsigned char* L, const int* sizes, int count, bscgpu_front_layout* out);
BSCGPU_API int bscgpu_front_batch_code(const bscgpu_front_layout* layout, int block, unsigned char* out, int coder, int features);

/* ---- the static coder's model (-e1) of a whole pass ("The static coder's model of a pass") --------------------------
 * The device model of bscgpu_qlfc_static_pstream over a pass's sub-block table: up to 4096 blocks and 8192 sub-blocks in one run
 * index space, one set of launches.  Entries are 16 bits, {[11:0] probability, [12] coded bit, [13] first decision of a run}.
 * bscgpu_static_pstream_batch_device: front end and model of `count` sorted blocks back to back in HBM (limits and layout as
 *   bscgpu_qlfc_front_batch_device, which it includes).  out[0 .. cap): every sub-block's entries back to back in stream order,
 *   sub-block s's at [poff[s], poff[s + 1]); poff has nsub + 1 <= 2 count + 1 entries.  Returns the number of decisions (nothing is
 *   copied when it exceeds cap); LIBBSC_NOT_SUPPORTED when the device declines the PASS — BSCGPU_CNT_DC_LAST_FAIL says why (0: an
 *   arena did not fit), the layout is filled and bscgpu_front_batch_code still codes every block; LIBBSC_BAD_PARAMETER; or a GPU
 *   error.  Synchronous.  Memory: the first call adds 8 bytes per decision of capacity (32 bytes per byte of max_n, + 48 KB) to the
 *   device model's arena, counted by bscgpu_arena_bytes from then on.
 * bscgpu_static_pstream_host: the CPU stand-in (no GPU, no context): the host model's own walk over sub-block s of a layout,
 *   recording instead of coding.  Returns the sub-block's number of decisions; entries past cap are counted, not written.
 * bscgpu_front_batch_code_ps: bscgpu_front_batch_code for the static coder from the sub-blocks' streams (ps / poff as above) — the
 *   host runs the range coder only.  A sub-block whose stream runs out of its budget is stored raw, rebuilt from its runs, as the
 *   reference stores it.  Thread-safe for different blocks of one layout. */
BSCGPU_API int64_t bscgpu_static_pstream_batch_device(bscgpu_ctx* ctx, const void* dL, const int* sizes, int count, bscgpu_front_layout* layout,
                                                      uint16_t* out, int64_t cap, uint32_t* poff);
BSCGPU_API int64_t bscgpu_static_pstream_host(const bscgpu_front_layout* layout, int s, uint16_t* out, int64_t cap);
BSCGPU_API int bscgpu_front_batch_code_ps(const bscgpu_front_layout* layout, int block, const uint16_t* ps, const uint32_t* poff,
                                          unsigned char* out, int features);

/* ---- the fast coder's model (-e0) of a whole pass ("The fast coder's model of a pass") ------------------------------
 * The three calls above for the fast coder; every limit, return value and rule is theirs word for word ("counted, not copied" above
 * cap, a declined pass still fills the layout, the memory of the first call).  Entries are in the BSCGPU_RC_FAST16 form:
 * {[12:0] the counter's value before its update, [13] coded bit, [14] first decision of a run, [15] run side of the run = 11-bit
 * precision, else 13}.  The fast model has no avg_rank flags and no run_hist look-back: the device declines a pass only for capacity
 * (BSCGPU_DC_FAIL_CAP) or a chain whose bracket stays open too long (BSCGPU_DC_FAIL_REPLAY).
 * bscgpu_fast_pstream_host is the host fast coder's own walk, recording instead of coding; bscgpu_front_batch_code_psf codes a block
 * from its sub-blocks' fast streams (framing, stored-raw rule and LIBBSC_NOT_COMPRESSIBLE points as bscgpu_front_batch_code_ps). */
BSCGPU_API int64_t bscgpu_fast_pstream_batch_device(bscgpu_ctx* ctx, const void* dL, const int* sizes, int count, bscgpu_front_layout* layout,
                                                    uint16_t* out, int64_t cap, uint32_t* poff);
BSCGPU_API int64_t bscgpu_fast_pstream_host(const bscgpu_front_layout* layout, int s, uint16_t* out, int64_t cap);
BSCGPU_API int bscgpu_front_batch_code_psf(const bscgpu_front_layout* layout, int block, const uint16_t* ps, const uint32_t* poff,
                                           unsigned char* out, int features);

/* ---- the adaptive coder's model (-e2) of a whole pass ("The adaptive coder's model of a pass") ----------------------
 * The adaptive coder's decisions, contexts and counters are the static coder's with other rates; its probability comes from one of
 * 1896 mixer instances per sub-block instead of a fixed blend.  The stage runs the static coder's device model with the adaptive
 * rates, then walks every mixer chain (sub-block, mixer id) of the pass, one lane per chain.  Entries are in the static coder's
 * 16-bit form, {[11:0] probability, [12] coded bit, [13] first decision of a run}: an -e2 sub-block stream is a BSCGPU_RC_STATIC16
 * body behind the prefix that bscgpu_rc_prefix returns for coder 1 (header word, alphabet and stop rule are the static coder's;
 * bscgpu_rc_prefix itself keeps refusing coder 2).  There is no block coder of its own: bscgpu_front_batch_code_ps codes a block
 * from -e2 streams, bscgpu_rc_encode_host / _device take a sub-block's stream unchanged.
 * bscgpu_adaptive_pstream_batch_device: limits, return values, "counted, not copied" above cap and "a declined pass still fills
 *   the layout" are bscgpu_static_pstream_batch_device's word for word.  dbg (optional, [4][cap] uint16): the state-, char- and
 *   position-indexed counter values before their update and the mixer id behind every decision, to localise a mismatch.  Declines:
 *   those of the static model (the run_hist resolve always runs, so never BSCGPU_DC_FAIL_HIST), and BSCGPU_DC_FAIL_MIX when the
 *   longest mixer chain of the pass exceeds the step cap (BSC_DC_MIX_CHAIN_CAP in the environment, read when a context is created;
 *   values below 16 are ignored; default 1 << 18: the steps the walk does in the time the host coder takes for a 64 MiB pass on 16
 *   threads, measured).  Memory: the first call adds 24 bytes per decision of capacity (96 bytes per byte of max_n) to
 *   the device model's arena, on top of the batch model's 8, counted by bscgpu_arena_bytes from then on; where that does not fit
 *   the pass is declined with BSCGPU_CNT_DC_LAST_FAIL = 0.
 * bscgpu_adaptive_pstream_host: the CPU stand-in (no GPU, no context): the host model's own walk over sub-block s of a layout with
 *   the mixer step the device uses, recording instead of coding; dbg as above.  Returns the sub-block's number of decisions; entries
 *   past cap are counted, not written. */
BSCGPU_API int64_t bscgpu_adaptive_pstream_batch_device(bscgpu_ctx* ctx, const void* dL, const int* sizes, int count, bscgpu_front_layout* layout,
                                                        uint16_t* out, int64_t cap, uint32_t* poff, uint16_t* dbg);
BSCGPU_API int64_t bscgpu_adaptive_pstream_host(const bscgpu_front_layout* layout, int s, uint16_t* out, int64_t cap, uint16_t* dbg);
/* bscgpu_adaptive_longest_chain_host: the same walk, counting: the decisions of every mixer of sub-block s (per_mixer, optional, 1896
 *   entries) — a sub-block's mixer chains — and, returned, the longest of them.  LIBBSC_BAD_PARAMETER as above. */
BSCGPU_API int64_t bscgpu_adaptive_longest_chain_host(const bscgpu_front_layout* layout, int s, uint32_t* per_mixer);

/* ---- a pass's model in segments ("Model segments") ------------------------------------------------------------------
 * Sub-blocks are independent chains, so the model of a pass can run over any contiguous range of its sub-blocks and write the same
 * entries.  A model segment is such a range, made of whole blocks.
 * bscgpu_model_segment_plan: the rule as a pure function.  sub_dec[s] / sub_und[s]: decisions and undecided avg_rank flags of
 *   sub-block s; blk_sub[count + 1]: first sub-block of every block (the layout's).  Blocks are taken in order.  A block is excluded
 *   (seg_of[b] = -1) when one of its sub-blocks has sub_und > 0 or its own decisions exceed dcap; an excluded block ends the current
 *   segment.  A block without sub-blocks gets -1 and ends nothing.  The others join the current segment while its decisions stay
 *   <= min(dcap, target) (target <= 0: dcap); a single block above target but <= dcap is a segment of its own.  Returns the number of
 *   segments, or LIBBSC_BAD_PARAMETER (null pointers with count > 0, count < 0, dcap <= 0, blk_sub not non-decreasing from >= 0) with
 *   nothing written.
 * bscgpu_model_segment_facts_device (a stage on its own for tests and tools, as the _pstream_ stages are; no caller needs it to
 *   compress): front end (as bscgpu_static_pstream_batch_device) and what the plan is made of, for `coder`:
 *   sub_dec[s] = decisions of sub-block s (what the CPU stand-in of that coder returns for it), sub_und[s] = its undecided avg_rank
 *   flags (0 for the fast coder); nsub <= 2 count entries each.  Two kernels over the run arrays, before any sort.  Returns 0,
 *   LIBBSC_NOT_SUPPORTED (an arena did not fit), LIBBSC_BAD_PARAMETER or a GPU error.  Synchronous.
 * bscgpu_pstream_batch_segments_device: front end (as bscgpu_static_pstream_batch_device) and the model of `coder`
 *   (LIBBSC_CODER_QLFC_STATIC or _FAST) segment by segment, target decisions per segment.  out[0 .. cap): the kept sub-blocks' entries
 *   back to back in sub-block order; poff[nsub + 1]: a sub-block that was not modelled has poff[s + 1] == poff[s]; blk_state[count]:
 *   0 when block b's streams are there, else the mask of BSCGPU_DC_FAIL_* that leaves it to the host model (the layout is always
 *   filled: bscgpu_front_batch_code codes such a block, bscgpu_front_batch_code_ps / _psf the others from out / poff).  A segment that
 *   declines while it runs is split at the block boundary nearest half its decisions and both halves run again, at most
 *   2 ceil(log2(blocks)) + 2 re-runs per pass.  Returns the decisions written (above cap: counted, not copied; poff and blk_state are
 *   filled all the same); LIBBSC_NOT_SUPPORTED only when an arena did not fit; LIBBSC_BAD_PARAMETER; or a GPU error.  Moves
 *   BSCGPU_CNT_BATCH_SEGMENTS / _SEG_RERUNS / _SEG_HOST_BLOCKS.  Synchronous.  Memory: as the whole-pass stage, + 100 KB of tables. */
BSCGPU_API int bscgpu_model_segment_plan(const uint32_t* sub_dec, const uint32_t* sub_und, const int* blk_sub, int count, int64_t dcap,
                                         int64_t target, int* seg_of);
BSCGPU_API int bscgpu_model_segment_facts_device(bscgpu_ctx* ctx, const void* dL, const int* sizes, int count, bscgpu_front_layout* layout,
                                                 int coder, uint32_t* sub_dec, uint32_t* sub_und);
BSCGPU_API int64_t bscgpu_pstream_batch_segments_device(bscgpu_ctx* ctx, const void* dL, const int* sizes, int count, bscgpu_front_layout* layout,
                                                        int coder, int64_t target, uint16_t* out, int64_t cap, uint32_t* poff, int* blk_state);
/* ... for the adaptive coder (-e2; DESIGN §2b, "The adaptive coder's model in segments"); the two above keep refusing coder 2.
 * bscgpu_adaptive_segment_facts_device: sub_dec and sub_und are the static coder's (same decisions, same flags); sub_mix[s] = the
 *   longest mixer chain of sub-block s (what bscgpu_adaptive_longest_chain_host returns for it), exact, from one more kernel over the
 *   run arrays; it means something only where sub_und[s] == 0.  Returns as bscgpu_model_segment_facts_device.
 * bscgpu_adaptive_pstream_batch_segments_device: bscgpu_pstream_batch_segments_device with the adaptive coder's model: every segment is
 *   the static model with the adaptive rates and then the mixers' walk over the segment's chains.  The plan has a third rule: a block
 *   with a sub-block whose longest chain exceeds the step cap (BSC_DC_MIX_CHAIN_CAP) is excluded with BSCGPU_DC_FAIL_MIX and ends the
 *   segment before it — the cap reads per BLOCK here, per pass in bscgpu_adaptive_pstream_batch_device.  Entries are the 16-bit static
 *   form; out, poff, blk_state, the re-runs (BSCGPU_DC_FAIL_REPLAY only), the return values and the segment counters are the above's.
 *   A segment whose chain table disagrees with its sub_mix is LIBBSC_GPU_ERROR.  BSCGPU_CNT_DC_MIX_CHAINS / _LONGEST / _WALK_US then say
 *   sum / maximum / sum over the pass's kept segments.  Memory: as bscgpu_adaptive_pstream_batch_device; where the mixers' arena does not
 *   fit, LIBBSC_NOT_SUPPORTED with BSCGPU_CNT_DC_LAST_FAIL = 0. */
BSCGPU_API int bscgpu_adaptive_segment_facts_device(bscgpu_ctx* ctx, const void* dL, const int* sizes, int count, bscgpu_front_layout* layout,
                                                    uint32_t* sub_dec, uint32_t* sub_und, uint32_t* sub_mix);
BSCGPU_API int64_t bscgpu_adaptive_pstream_batch_segments_device(bscgpu_ctx* ctx, const void* dL, const int* sizes, int count, bscgpu_front_layout* layout,
                                                                 int64_t target, uint16_t* out, int64_t cap, uint32_t* poff, int* blk_state);

/* ---- the packed 13-bit stream of a pass (-e1; DESIGN §2b, "The packed stream of a pass") ------------------------------------------
 * The static coder's stream of a pass in the form bscgpu_qlfc_static_pstream_packed writes for a block, over up to 8192 sub-blocks:
 * 13 bits per decision, {[11:0] probability, [12] coded bit}, eight decisions in 13 bytes (field e of a group at bits
 * [13 e, 13 e + 13), little endian).  Sub-block s starts at decision pbase[s] of the packed space: pbase[0] = 0, pbase[s + 1] =
 * pbase[s] + (poff[s + 1] - poff[s] rounded up to a multiple of 64), i.e. at byte pbase[s] / 8 * 13; behind a sub-block's last
 * decision its extent is zero.  The stream is pbase[nsub] / 8 * 13 bytes, every one of them written.  A sub-block is a
 * BSCGPU_RC_STATIC13 body at pbase[s] (bscgpu_rc_stream::body) for every range coder of this library.
 * bscgpu_static_pstream_batch_packed_device: bscgpu_static_pstream_batch_device with the stream in this form.  out[0 .. cap_bytes);
 *   poff[nsub + 1] as there, pbase[nsub + 1].  Returns the number of decisions; nothing is copied when pbase[nsub] / 8 * 13 >
 *   cap_bytes (poff and pbase are filled all the same).  LIBBSC_NOT_SUPPORTED when the device declines the pass
 *   (BSCGPU_CNT_DC_LAST_FAIL says why) and also, with BSCGPU_CNT_DC_LAST_FAIL = 0, when the packed form was void: 64 consecutive runs
 *   with more decisions than a wavefront stages (runs of thousands) — the 16-bit stage still serves such a pass.  Synchronous.
 *   Memory: as the 16-bit stage, + 66 KB of tables.
 * bscgpu_pstream_pack13_host: the CPU stand-in for the layout, a pure function: packs 16-bit static entries (ps, sub-block s's at
 *   [poff[s], poff[s + 1])) into out and fills pbase[nsub + 1].  Returns the byte count pbase[nsub] / 8 * 13; above cap_bytes nothing
 *   is written but pbase.  LIBBSC_BAD_PARAMETER: null pointers, nsub < 0, poff not non-decreasing.
 * bscgpu_front_batch_code_ps13: bscgpu_front_batch_code_ps reading BSCGPU_RC_STATIC13 bodies (packed / poff / pbase as above).  One
 *   difference: the packed coder gives up at ANY decision once its output is full, the reference at a run start, so a sub-block
 *   whose packed stream ends LIBBSC_NOT_COMPRESSIBLE is coded again by the host model from its runs, and the reference's own answer
 *   decides between "compressed" and "stored raw" — never the packed coder's word alone.  Output byte-equal to
 *   bscgpu_front_batch_code.  Thread-safe for different blocks of one layout.
 * bscgpu_pstream_batch_segments_packed_device: bscgpu_pstream_batch_segments_device for -e1 in this form (any other coder:
 *   LIBBSC_BAD_PARAMETER).  out[0 .. cap_bytes): the kept segments' packed streams back to back; pbase runs on across segments in
 *   kept order and a sub-block that was not modelled has pbase[s + 1] == pbase[s] (and poff[s + 1] == poff[s]).  Above cap_bytes:
 *   counted, not copied.  A segment whose packed form is void is re-run in the 16-bit form internally and packed into place on the
 *   host (bscgpu_pstream_pack13_host): the caller sees one form, the blocks keep the device's model, BSCGPU_CNT_BATCH_PACKED_VOID
 *   counts it.  Returns the decisions written.  Everything else as the 16-bit stage. */
BSCGPU_API int64_t bscgpu_static_pstream_batch_packed_device(bscgpu_ctx* ctx, const void* dL, const int* sizes, int count, bscgpu_front_layout* layout,
                                                             uint8_t* out, int64_t cap_bytes, uint32_t* poff, int64_t* pbase);
BSCGPU_API int64_t bscgpu_pstream_pack13_host(const uint16_t* ps, const uint32_t* poff, int nsub, uint8_t* out, int64_t cap_bytes, int64_t* pbase);
BSCGPU_API int bscgpu_front_batch_code_ps13(const bscgpu_front_layout* layout, int block, const uint8_t* packed, const uint32_t* poff,
                                            const int64_t* pbase, unsigned char* out, int features);
BSCGPU_API int64_t bscgpu_pstream_batch_segments_packed_device(bscgpu_ctx* ctx, const void* dL, const int* sizes, int count, bscgpu_front_layout* layout,
                                                               int coder, int64_t target, uint8_t* out, int64_t cap_bytes, uint32_t* poff,
                                                               int64_t* pbase, int* blk_state);

/* ---- batched decompression: one inverse-BWT pass for many blocks -------------
 * bscgpu_unbwt_batch_device: L of `count` blocks back to back in HBM (block b at Σ sizes[0..b), primary[b] its 1-based
 *   primary index) -> T in the same layout; dT may be dL.  Passes of consecutive blocks, at most max_n bytes and
 *   min(4096, max_n / 256 + 16) blocks each.  results[b] = what bscgpu_unbwt returns for block b alone (0, LIBBSC_DATA_CORRUPT,
 *   LIBBSC_NOT_SUPPORTED: the step cap, use a host walk; LIBBSC_BAD_PARAMETER: primary out of 1..n_b; LIBBSC_GPU_NOT_ENOUGH_MEMORY:
 *   n_b > max_n).  A failed block's T range is not written; the other blocks decode as if alone.  Returns 0 or a batch-level error.
 * bscgpu_decompress_batch_sizes: reads the headers only.  data_sizes[b] = the block's dataSize, 0 where its header cannot be
 *   read; returns the decoded total (Σ data_sizes) or LIBBSC_BAD_PARAMETER.
 * bscgpu_decompress_batch: compressed blocks back to back in host memory (block b: in_sizes[b] bytes).  Block b decodes to
 *   output + Σ data_sizes[0..b) (the layout bscgpu_compress_batch took its input in); out_cap must hold the total.
 *   results[b] = what bsc_decompress(block b, in_sizes[b], ..., dataSize, features) returns, error codes included.  (Aux indexes
 *   are a shortcut, not data: the GPU walk never reads them, and bsc_decompress falls back to the single walk from row 0 where
 *   they are inconsistent, so a block with valid checksums and damaged aux indexes decodes on both routes.)
 *   BWT blocks of 2 .. max_n bytes share one GPU inverse BWT per pass (QLFC decoding on the host threads, pass k + 1's
 *   overlapping pass k's GPU work; Adler-32 of the output on the GPU); stored, ST3..ST8, larger and damaged blocks go
 *   through bsc_decompress itself.  input and output must not overlap.
 * bscgpu_decompress_batch_device: the same with output in HBM (dOutput): without LZP the walk writes each block straight
 *   to its place; LZP blocks are undone on the host and copied up.
 * Both return 0 or a batch-level error: LIBBSC_BAD_PARAMETER (null pointers, count < 0, in_sizes[b] < 0, out_cap below
 *   the total) with nothing written, or a GPU failure.  Memory: the batch table and the pinned pass buffers of the
 *   compress batch.
 * bscgpu_unbwt_batch_plan: the routing rule as a pure function.  sizes[b] = block b's BWT length (a bound: its dataSize),
 *   or -1 for a block no pass takes (stored, ST3..ST8, a header that fails).  pass_of[b] = its pass, or -1 when
 *   sizes[b] < 2 or > cap; passes take consecutive such blocks (other blocks between them do not end a pass), at most
 *   cap bytes and min(4096, cap / 256 + 16) blocks each.  Returns the number of passes (cap = the context's max_n). */
BSCGPU_API int bscgpu_unbwt_batch_plan(const int* sizes, int count, int64_t cap, int* pass_of);
BSCGPU_API int bscgpu_unbwt_batch_device(bscgpu_ctx* ctx, const void* dL, void* dT, const int* sizes, int count, const int* primary,
                                         int* results);
BSCGPU_API int64_t bscgpu_decompress_batch_sizes(const unsigned char* input, const int* in_sizes, int count, int* data_sizes);
BSCGPU_API int bscgpu_decompress_batch(bscgpu_ctx* ctx, const unsigned char* input, const int* in_sizes, int count, unsigned char* output,
                                       int64_t out_cap, int* results, int features);
BSCGPU_API int bscgpu_decompress_batch_device(bscgpu_ctx* ctx, const unsigned char* input, const int* in_sizes, int count, void* dOutput,
                                              int64_t out_cap, int* results, int features);

/* Pipelined variant: up to `depth` (<= 8) blocks in flight on one GPU.  submit() runs the GPU stage of a block
 * (Adler-32, sort transform, QLFC front end, D2H of the run arrays) on the calling thread and hands the host stage
 * (QLFC modelling + range coding, one task per sub-block; container) to the process's coder threads, so block i+1 sorts
 * while blocks i, i-1, ... are coded.
 * dInput and output must stay valid until wait() returns for that ticket.  wait() returns what
 * bscgpu_compress_device would have returned.  One submitting thread per pipe.  The host work is queued as tasks for the
 * process's pool of coder threads, shared by all pipes (default: the CPUs the process may use — affinity and cgroup quota —
 * clamped to 4..64; BSCGPU_HOST_THREADS overrides the thread count, BSCGPU_HOST_CPUS the CPU budget idle CPUs are counted
 * against), so a depth of 3-4 keeps those threads and the GPU busy.  A device-model block is one eight-lane SIMD task (half the
 * CPU time, ~100 ms) when the pool is busy and four tasks of two interleaved sub-blocks (~50 ms) while at least four CPUs of
 * the budget are idle if BSC_RC_ADAPTIVE=1 (round 5: off by default — every block that is not marked low-latency is the former;
 * BSC_RC_SIMD=8 / 0 forces one of the two). */
typedef struct bscgpu_pipe bscgpu_pipe;
/* Extra `features` bit for bscgpu_pipe_submit*: code this block's sub-blocks as several short host tasks (two interleaved scalar range
 * coders per task, ~50 ms for a 64 MiB block; one coder per task, ~35 ms, when eight CPUs of the pool are idle) instead of one
 * eight-lane SIMD task (~100 ms, half the CPU time).  For the LAST blocks
 * of a job, where latency — the drain of the pipeline — counts and the coder threads are running dry anyway.  Output is identical. */
#define BSCGPU_FEATURE_LOW_LATENCY 0x10000
/* ... and with this bit as well: one coder per task (eight tasks) whatever the pool's load — for the very last block(s) of a job, whose
 * coding time is the job's last 35 ms whatever else is still running. */
#define BSCGPU_FEATURE_URGENT 0x20000
BSCGPU_API int  bscgpu_pipe_create(bscgpu_ctx* ctx, int depth, bscgpu_pipe** out);
/* How the pool has coded the pipes' blocks so far: out[0] blocks as eight scalar tasks, [1] as four pair tasks, [2] as one eight-lane
 * task, [3] blocks on the host model (one task per sub-block).  reset != 0 clears the counts.  (bench.py reports them.) */
BSCGPU_API void bscgpu_coder_pool_stats(uint64_t out[4], int reset);
/* Where a job ends: `blocks` more blocks will be submitted to the pipes of this process (all pipes together), which drive `gpus` GPUs.
 * The blocks whose GPU stages END last are then coded as short tasks — per GPU the last one as eight single-stream tasks, the few
 * before it as pairs (two fewer than the contexts that interleave on a GPU) (BSC_TAIL_SINGLES / BSC_TAIL_PAIRS) — whatever their order of submission (several contexts interleave on a GPU,
 * so the two orders differ by up to 100 ms), everything earlier as one eight-lane task.  For callers that know the total, instead of
 * marking blocks BSCGPU_FEATURE_LOW_LATENCY at submission; blocks < 0 withdraws the announcement.  Output is identical either way. */
BSCGPU_API int  bscgpu_coder_pool_expect(long long blocks, int gpus);
/* The pool's own record of its tasks (recorded when BSCGPU_POOL_TRACE=1 is in the environment): up to cap rows of six doubles — start, end
 * (seconds on the clock bscgpu_steady_now reads), the block's id inside its pipe, first sub-block, sub-blocks per task (1, 2, 8), the
 * block's features.  Returns the number of rows; reset != 0 clears the record.  (bench.py prints it with
 * BSC_BENCH_TRACE=1: where a short job's last 100 ms go.) */
BSCGPU_API int    bscgpu_coder_pool_trace(double* out, int cap, int reset);
BSCGPU_API double bscgpu_steady_now(void);
/* 1 when a block's probability stream leaves the device through the HSA runtime's DMA copy (csrc/device/dma_copy.h) in this process,
 * 0 when it goes through hipMemcpyAsync (BSC_D2H_DMA=0, or no usable HSA runtime in the process).  Which engine that is depends on the
 * HIP runtime: a DMA engine on ROCm 7.2's, a 256-workgroup copy kernel on the one torch 2.10 carries (profiles/r06/d2h_copy_path.txt). */
BSCGPU_API int  bscgpu_d2h_dma_available(void);
/* The rule behind those shapes as a pure function (unit-tested on CPU): sub-blocks per coder task — 8 (one SIMD task), 2 or 1 — from
 * forced (-1 none, 8 or 0: BSC_RC_SIMD), low_latency (synchronous call or BSCGPU_FEATURE_LOW_LATENCY), pool_free (idle CPUs of the
 * pool's budget; -1: a synchronous call), sync_cpus (CPUs / synchronous callers running), wide_simd (AVX-512VL), adaptive. */
BSCGPU_API int bscgpu_coder_task_shape(int forced, int low_latency, int pool_free, int sync_cpus, int wide_simd, int adaptive);
BSCGPU_API void bscgpu_pipe_destroy(bscgpu_pipe* pipe);
BSCGPU_API int  bscgpu_pipe_submit(bscgpu_pipe* pipe, const void* dInput, uint8_t* output, int n,
                                   int blockSorter, int coder, int features);       /* ticket >= 0 or error */
/* Host-resident block with bsc_compress's full parameter list (libbsc.cpp:213), LZP included: LZP runs on the calling
 * thread (+ up to 8 chunk threads), then one H2D copy feeds the same GPU stage.  input must stay valid until wait(). */
BSCGPU_API int  bscgpu_pipe_submit_host(bscgpu_pipe* pipe, const uint8_t* input, uint8_t* output, int n,
                                        int lzpHashSize, int lzpMinLen, int blockSorter, int coder, int features);
BSCGPU_API int  bscgpu_pipe_wait(bscgpu_pipe* pipe, int ticket);
/* From ANY thread: block until the host stage of `ticket` is over; 1 and *result (what bscgpu_pipe_wait will return) when the block is
 * complete — its output buffer is final —, 0 when it needs its submitting thread after all (redo on the host model) or has been retired
 * already.  Does not retire the ticket.  For in-order collectors running beside the submitting thread (the job driver). */
BSCGPU_API int  bscgpu_pipe_peek(bscgpu_pipe* pipe, int ticket, int* result);

/* ---- multi-GPU job: every GPU of a node from one process, C/C++ callers ----------------------------------------------------
 * The reference parallelises over blocks with the CLI's OpenMP team (bsc.cpp:182-199: next block under critical(input),
 * bsc_compress, write under critical(output)) and knows one GPU behind one lock (bwt.cpp:50-52).  A job is that loop for N GPUs:
 * `contexts_per_device` pipes per device (their kernels interleave on the GPU), `depth` blocks in flight per pipe, one worker thread
 * per pipe pulling the next block from ONE queue (blocks are independent, so block b -> whichever GPU is free next: on equal GPUs one
 * block per GPU per round, with load balancing for free), host coding on the process-wide coder pool.  The caller adds blocks in
 * order and collects them in order: bscgpu_job_wait(b) returns what bsc_compress would have returned for block b, and the bytes
 * are in that block's output buffer — the ordered host gather of the multi-GPU run (inside one process nothing has to travel
 * between GPUs; the RCCL concatenation belongs to the one-process-per-GPU layout, libbsc_amd/multigpu.py).
 *   devices / ndevices   device ordinals; ndevices = 0: every visible device
 *   input / output       host buffers, n and n + 28 bytes, valid until the block has been waited for
 * add() returns the block's number (0, 1, 2, ... in call order) or a negative code; it never blocks on the GPU.  One thread adds;
 * wait() may be called from another thread (for blocks that have been added); destroy() finishes what is queued, then frees every
 * context.  */
typedef struct bscgpu_job bscgpu_job;
BSCGPU_API int  bscgpu_job_create(bscgpu_job** job, const int* devices, int ndevices, int contexts_per_device, int depth, int64_t max_block_bytes);
BSCGPU_API int  bscgpu_job_add(bscgpu_job* job, const uint8_t* input, uint8_t* output, int n, int lzpHashSize, int lzpMinLen,
                               int blockSorter, int coder, int features);
/* Optional: how many blocks the job will have in all (a file's block count).  With the total known the job's LAST blocks are handled
 * for latency instead of throughput — the drain of the pipeline is the caller's time: the k-th context of a device takes a block only
 * while more than k x devices are left (the GPU stages of the tail end one after the other and their host coding overlaps the GPU work
 * still to come, instead of all contexts finishing one last block each in a burst), and the last (devices x contexts) blocks are
 * submitted with BSCGPU_FEATURE_LOW_LATENCY.  Adding more blocks than announced is allowed (the rule is dropped).  Independently of
 * this call the START of a job (and of every later burst, when the caller had let the job run dry) is tapered: a first context begins,
 * the k-th context of a device joins once k GPU stages of the burst have finished there. */
BSCGPU_API int  bscgpu_job_expect(bscgpu_job* job, int total_blocks);
/* (bscgpu_job_wait looks at the worker's pipe while it waits: it must have RETURNED before bscgpu_job_destroy is called on the same
 * job — destroy finishes the queued blocks, then frees the pipes a concurrent wait would still be peeking into) */
BSCGPU_API int  bscgpu_job_wait(bscgpu_job* job, int block);
/* which worker (= pipe; return value) on which device took the block — known once a worker has claimed it */
BSCGPU_API int  bscgpu_job_block_worker(bscgpu_job* job, int block, int* device);
BSCGPU_API void bscgpu_job_destroy(bscgpu_job* job);
/* The executor behind a job's pipes as a table of functions (default: bscgpu_create / bscgpu_pipe_* of this library).  Tests drive
 * the scheduler with a CPU stand-in (tests/test_job_driver.py); semantics of every entry = the bscgpu_* function it stands for. */
typedef struct bscgpu_job_backend {
    void* user;
    int  (*ctx_create)(void* user, void** ctx, int device, int64_t max_n);
    void (*ctx_destroy)(void* user, void* ctx);
    int  (*pipe_create)(void* user, void* ctx, int depth, void** pipe);
    void (*pipe_destroy)(void* user, void* pipe);
    int  (*pipe_submit_host)(void* user, void* pipe, const uint8_t* input, uint8_t* output, int n, int lzpHashSize, int lzpMinLen,
                             int blockSorter, int coder, int features);          /* ticket >= 0 or error */
    int  (*pipe_wait)(void* user, void* pipe, int ticket);
} bscgpu_job_backend;
BSCGPU_API int  bscgpu_job_create_ex(bscgpu_job** job, const int* devices, int ndevices, int contexts_per_device, int depth,
                                     int64_t max_block_bytes, const bscgpu_job_backend* backend /* NULL = this library */);

/* ---- profiling --------------------------------------------------------------------------- */
/* When enabled every kernel launch is bracketed by HIP events on the context's stream (the stream
 * the kernels run on) and accumulated per kernel class. */
enum {
    BSCGPU_K_RADIX_SCATTER = 0, /* the graded kernel: one LSD digit pass (read + scatter) */
    BSCGPU_K_RADIX_HIST    = 1, /* per-chunk digit histogram of the next pass */
    BSCGPU_K_RADIX_SCAN    = 2,
    BSCGPU_K_PACK          = 3, /* key packing (BWT prefix keys / ST context keys) */
    BSCGPU_K_SEG           = 4, /* head flags, rank scans, compaction */
    BSCGPU_K_GATHER        = 5, /* ISA[SA+h] gathers */
    BSCGPU_K_EMIT          = 6, /* BWT / ST output byte emit */
    BSCGPU_K_MISC          = 7,
    BSCGPU_K_DC_CTX        = 8,  /* device coder: contexts, items, setup */
    BSCGPU_K_DC_PART       = 9,  /* device coder: decisions into chain-major order */
    BSCGPU_K_DC_EVAL       = 10, /* device coder: counter chains */
    BSCGPU_K_DC_PSTREAM    = 11, /* device coder: probability stream */
    BSCGPU_K_RADIX_HISTALL = 12, /* single-read sorts: the one histogram read per sort (all digits at once) */
    BSCGPU_K_RADIX_AUX     = 13, /* keys-only passes that also emit the permutation (device coder's orders, inverse BWT): not the graded kernel */
    BSCGPU_K_RC            = 14, /* range coder: many probability streams in one launch (rangecoder.hip) */
    BSCGPU_K_DC_FACTS      = 15, /* device coder, a pass in model segments: per-sub-block facts (flags, decision counts) and segment tables */
    BSCGPU_K_DC_REPLAY     = 16, /* device coder: open chunk starts resolved exactly (BSCGPU_OPT_DC_REPLAY_EXACT): candidate walks and chaining */
    BSCGPU_K_LZP           = 17, /* LZP encoder stage (lzp.hip): keys, links, flags, the sweep; its sort passes are booked under _RADIX_AUX */
    BSCGPU_K_COUNT         = 18
};
typedef struct bscgpu_kstat {
    double   ms;        /* accumulated HIP-event time */
    uint64_t launches;
    uint64_t bytes;     /* algorithmic bytes moved (per kernel) */
    uint64_t records;   /* records processed (radix kernels) */
} bscgpu_kstat;
BSCGPU_API void bscgpu_profile_enable(bscgpu_ctx* ctx, int on);
BSCGPU_API void bscgpu_profile_reset(bscgpu_ctx* ctx);
BSCGPU_API int  bscgpu_profile_get(bscgpu_ctx* ctx, bscgpu_kstat* stats /* [BSCGPU_K_COUNT] */);
/* Per-launch durations (ms) of the most recent radix scatter launches, newest last; returns count. */
BSCGPU_API int  bscgpu_profile_scatter_launches(bscgpu_ctx* ctx, double* ms, uint64_t* records, int max);
/* Stage wall times (ms) of the last bscgpu_compress_device call: [0] adler, [1] sort transform,
 * [2] D2H, [3] host coder, [4] total; plus doubling rounds in [5]. */
BSCGPU_API int  bscgpu_last_stage_ms(bscgpu_ctx* ctx, double* out6);

BSCGPU_API const char* bscgpu_last_error(const bscgpu_ctx* ctx);

/* ---- measurement / test knobs of one context ------------------------------------------------
 * BSCGPU_OPT_RS_ONESWEEP   which large (key, value) sorts take the single-read digit passes: 0 none (three-kernel passes: histogram,
 *                          scan and a scatter whose offsets are all known before it starts — what bench.py times as the digit pass's
 *                          `pattern_ceiling`), 1 large (key, value) sorts only, 2 every sort of >= 4 tiles (tests), 3 large sorts including keys-only ones (the
 *                          sort transform; the default).
 *                          Results are identical.
 * BSCGPU_CNT_OS_RETRIES    (get only) transforms this context has redone through the three-kernel passes because a single-read pass
 *                          gave up a wait (bounded polls; the block still comes out right).
 * BSCGPU_OPT_DC_PACKED_STREAM  1 (default; BSC_PS13=0 in the environment turns it off): the static coder's probability stream crosses
 *                          PCIe as 13 bits per decision — 12-bit probability + coded bit, eight decisions in 13 bytes — instead of
 *                          16-bit entries (298 instead of 366 MB per 64 MiB text block).  The run-start mark of the 16-bit entry only
 *                          placed the reference's output-budget test; a stream that reaches its budget is redone on the host model
 *                          either way.  Same output.
 * BSCGPU_CNT_DC_*          (get only) the last block this context gave to the device model of the static / fast coder, whether it
 *                          stayed there or was declined (the block is then coded through the host model, same bytes):
 *     _REPLAYS             evaluation chunks whose start value had to be replayed serially (the predecessor's bracket had not met);
 *                          0 where BSCGPU_OPT_DC_REPLAY_EXACT settled every such start
 *     _REPLAY_RESOLVED     evaluation chunks whose start value the exact resolve settled (BSCGPU_OPT_DC_REPLAY_EXACT; 0 with the option off)
 *     _LAST_FAIL           why the block was declined: a mask of BSCGPU_DC_FAIL_*, 0 when it stayed on the device
 *     _AVG_UNDECIDED       runs whose avg_rank >= 32 flag the warmed-up bracket left open (any such run declines: _FAIL_AVG — unless BSCGPU_OPT_DC_AVG_EXACT settles it)
 *     _AVG_RESOLVED        of those, the runs whose flag the exact resolve then settled (BSCGPU_OPT_DC_AVG_EXACT; 0 with the option off)
 *     _HIST_EXTENDED       runs whose run_hist bracket was still open after nine predecessors of their symbol and went on to the
 *                          extended look-back (36 .. 9216 predecessors; still open after that: _FAIL_HIST) — or, with
 *                          BSCGPU_OPT_DC_HIST_EXACT, to the exact resolve (the same runs are counted in both modes)
 *     _HIST_RESOLVED       of those, the runs whose run_hist the exact resolve settled (BSCGPU_OPT_DC_HIST_EXACT: all of them; 0 with the option off)
 * BSCGPU_OPT_DC_AVG_EXACT  0 (default; BSC_DC_AVG_EXACT=1 in the environment turns it on for contexts created after that) / 1: the
 *                          avg_rank flags the bracket leaves open are computed exactly on the device — every chunk of runs is walked
 *                          from each of the at most 33 values its start can have, the chunks' maps are chained, the open chunks walked
 *                          again from their exact start; no sync, nothing approximate — so such a block, pass or segment is not declined
 *                          for them: _FAIL_AVG is raised only where a start bracket is 64 values wide or more, which the contraction
 *                          of avg_rank rules out.  Batched passes in model segments: no block is excluded for its avg flags.  -e0 has
 *                          no such flags and is not affected.  Same output.
 * BSCGPU_OPT_DC_REPLAY_EXACT  0 (default; BSC_DC_REPLAY_EXACT=1 in the environment turns it on for contexts created after that) / 1:
 *                          an evaluation chunk that starts inside a counter chain whose bracket has not met (periodic ranks or run
 *                          lengths: tables, records, bitmaps) gets its start value exactly and in parallel — the chunk before it is
 *                          walked from every value of its own start bracket (at most 373 for -e1, 128 for -e0; up to six per lane of
 *                          one wavefront), the chunks' maps are followed from the last known start — instead of one lane replaying up to
 *                          64 chunks serially; such a block, pass or segment is then not declined for it: _FAIL_REPLAY is raised only
 *                          behind a start bracket of more than 384 values, which the contraction of the counter maps rules out
 *                          (BSC_DC_REPLAY_CAND in the environment, read when a context is created: a lower cap, a test knob).  Both
 *                          coders, single blocks, passes and model segments.  Buffers on first use (1.5 bytes per byte of max_n, counted
 *                          by bscgpu_arena_bytes from then on); if they do not fit the option has no effect.  Same output.
 * BSCGPU_OPT_DC_HIST_EXACT  0 (default; BSC_DC_HIST_EXACT=1 in the environment turns it on for contexts created after that) / 1:
 *                          a run whose run_hist bracket is still open after nine predecessors of its symbol (a symbol whose runs stay
 *                          in one length class of 2 to 127 bytes: tables, records, bitmaps, padding) gets its value exactly and in
 *                          parallel instead of looking back over up to 9216 predecessors in its own lane — every chunk of 1024 runs
 *                          in symbol-major order is walked from all 64 values run_hist can have, one per lane of a wavefront, the
 *                          chunks' maps are chained as the avg_rank resolve's are, the chunks with open runs walked again from their
 *                          exact start; no sync, nothing approximate, and no guard: _FAIL_HIST is never raised.  -e1 single blocks,
 *                          passes and model segments; -e0 has no run_hist and is not affected.  Buffers on first use (0.2 byte per byte
 *                          of max_n, counted by bscgpu_arena_bytes from then on); if they do not fit the option has no effect.  Same output.
 * BSCGPU_OPT_BATCH_FRONT    1: the passes of bscgpu_compress_batch / _batch_device run the QLFC front end of the whole pass on the GPU and
 *                          bring down its run arrays (sym, rank, start) instead of L; 0: L comes down and every block goes through
 *                          bsc_coder_compress on the host.  Same output.  Default 1 (measured: DESIGN §2b).
 * BSCGPU_CNT_BATCH_FRONT_PASSES, BSCGPU_CNT_BATCH_L_PASSES  (get only) passes of this context's compress-batch calls that took each
 *                          of the two routes (a pass whose pinned run buffers cannot be had takes the L route).
 * BSCGPU_OPT_DEVICE_RC     1: a block that took the device model (-e1 16-bit or packed, -e0) has its sub-block streams range-coded by one launch
 *                          on the context's stream, straight from the device's probability stream (rangecoder.hip); only the compressed
 *                          bytes come down and the host frames them.  A sub-block that ends LIBBSC_NOT_COMPRESSIBLE sends the block through
 *                          the host model again, as on the host route.  0 (default): the stream crosses PCIe and host threads code it.  Same
 *                          output.  -e2 and blocks the model declines are not affected.  A batched pass that took the device model
 *                          (BSCGPU_OPT_BATCH_MODEL, BSCGPU_OPT_BATCH_MODEL_FAST) has all its sub-block streams coded by one launch, eight streams per wavefront;
 *                          only the coded bytes come down.  The counter below then counts the pass.
 * BSCGPU_CNT_DEVICE_RC_BLOCKS  (get only) blocks of this context whose streams were coded that way.
 * BSCGPU_OPT_BATCH_MODEL    1: a pass of the compress-batch calls that takes the front-end route with the static coder (-e1) also runs the
 *                          coder's adaptive model on the GPU (bscgpu_static_pstream_batch_device's stage) and brings the probability
 *                          stream down; the coder threads run the range coder only (bscgpu_front_batch_code_ps).  A pass the device
 *                          declines, a pass below 16 MiB (BSC_BATCH_MODEL_MIN_PASS in the environment: another minimum, in bytes), and
 *                          every pass with -e2 or without the front end, takes the host model (-e0: the option below).  Same output.  Default 0: it halves
 *                          the host's CPU time per MB and wins on calls of several passes, but not on the one-pass workloads.
 * BSCGPU_CNT_BATCH_MODEL_PASSES, BSCGPU_CNT_BATCH_MODEL_DECLINED  (get only) passes that were coded from the device model's stream, and
 *                          passes given to it that it declined (BSCGPU_CNT_DC_LAST_FAIL: why the last one was).
 * BSCGPU_OPT_BATCH_MODEL_FAST  1: the same for the fast coder (-e0), an option of its own: a pass of the compress-batch calls that takes
 *                          the front-end route with -e0 also runs the fast coder's model on the GPU (bscgpu_fast_pstream_batch_device's
 *                          stage); the coder threads run the range coder only (bscgpu_front_batch_code_psf), or, with
 *                          BSCGPU_OPT_DEVICE_RC, one launch of the device's range coder codes the pass.  A pass the device declines
 *                          (capacity, or a chain open over too many evaluation chunks) and a pass below 32 MiB
 *                          (BSC_BATCH_MODEL_MIN_PASS in the environment: another minimum for both routes) take the host model.  -e1 and
 *                          -e2 are not affected, and BSCGPU_OPT_BATCH_MODEL and its counters are not moved by -e0 calls.  Same output.
 *                          Default 0: measured, it gains on calls of several full passes (4 % from host input, 10 % from HBM, a quarter
 *                          less CPU per MB) and loses 9 - 19 % on one-pass calls.
 * BSCGPU_CNT_BATCH_FAST_PASSES, BSCGPU_CNT_BATCH_FAST_DECLINED  (get only) its passes coded from the device's stream, and declined.
 * BSCGPU_OPT_BATCH_MODEL_ADAPTIVE  1: the same for the adaptive coder (-e2), an option of its own: a pass of the compress-batch calls that
 *                          takes the front-end route with -e2 also runs the adaptive coder's model on the GPU
 *                          (bscgpu_adaptive_pstream_batch_device's stage); the 16-bit stream comes down and the coder threads run the
 *                          range coder only (bscgpu_front_batch_code_ps).  A pass the device declines (the static model's reasons, or
 *                          BSCGPU_DC_FAIL_MIX) and a pass below BSC_BATCH_MODEL_MIN_PASS (default 16 MiB, -e1's, until measured) take
 *                          the host model.  BSCGPU_OPT_BATCH_MODEL_SEGMENTS, the packed form and BSCGPU_OPT_DEVICE_RC do not apply to -e2:
 *                          with them on such a pass takes the whole-pass 16-bit host-coded route (segments for -e2 have an option of
 *                          their own, BSCGPU_OPT_BATCH_ADAPTIVE_SEGMENTS).  -e1 and -e0 and their counters are not affected.  Same
 *                          output.  Default 0 (DESIGN §2b has the stage's and the whole calls' figures).
 * BSCGPU_CNT_BATCH_ADAPTIVE_PASSES, BSCGPU_CNT_BATCH_ADAPTIVE_DECLINED  (get only) its passes coded from the device's stream, and declined.
 * BSCGPU_CNT_DC_MIX_CHAINS, BSCGPU_CNT_DC_MIX_LONGEST  (get only) mixer chains of the last -e2 pass given to the device model, and the
 *                          steps of the longest (what BSC_DC_MIX_CHAIN_CAP is compared with); a pass in segments: the sum and the
 *                          maximum over its kept segments (and _WALK_US below their sum).
 * BSCGPU_CNT_DC_MIX_WALK_US  (get only) the host's wall time, in microseconds, of that pass's walk (chain placement and walk kernels up to
 *                          their sync): divided by the longest chain, the walk's time per dependent step (tools/batch_bench.py).
 * BSCGPU_OPT_BATCH_ADAPTIVE_SEGMENTS  0 (default) / 1: with BSCGPU_OPT_BATCH_MODEL_ADAPTIVE on and -e2, a pass that takes the model route
 *                          takes it in model segments (bscgpu_adaptive_pstream_batch_segments_device's stage): a pass above the arena's
 *                          capacity is cut, not declined, and a block with a mixer chain above the step cap (BSCGPU_DC_FAIL_MIX, per
 *                          block here) or another of the model's reasons takes the host model alone.  Moves
 *                          BSCGPU_CNT_BATCH_ADAPTIVE_PASSES / _DECLINED (kept: the device's stream serves any block) and
 *                          BSCGPU_CNT_BATCH_SEGMENTS / _SEG_RERUNS / _SEG_HOST_BLOCKS.  BSC_BATCH_MODEL_SEGMENT applies.  -e1 and -e0 are
 *                          not affected, nor is -e2 without BSCGPU_OPT_BATCH_MODEL_ADAPTIVE.  Same output.
 * BSCGPU_OPT_BWT_FOLD      1 (default; BSC_BWT_FOLD=0 in the environment turns it off): where the first-sort key of a single block leaves
 *                          1..4 bits over a whole number of bytes (17..64 symbols) and the sort takes the single-read passes, key
 *                          packing places the records by those bits and counts the byte digits, and the sort is one pass shorter
 *                          and reads no histogram.  2: packing places the records, rs_hist_all still counts (measurements).  Same output.
 * BSCGPU_CNT_BWT_FOLDED    (get only) first sorts of this context that took that route.
 * BSCGPU_OPT_BATCH_MODEL_SEGMENTS  0 (default) / 1: with the coder's own model option on (BSCGPU_OPT_BATCH_MODEL for -e1, _FAST for -e0), a
 *                          pass that takes the model route takes it in model segments (bscgpu_pstream_batch_segments_device's stage):
 *                          a pass above the arena's capacity in decisions is cut, not declined, and a block the device cannot model
 *                          takes the host model alone instead of taking its pass with it.  BSC_BATCH_MODEL_SEGMENT in the environment:
 *                          decisions per segment (default: the capacity).  Not with BSCGPU_OPT_DEVICE_RC: such a pass takes the
 *                          whole-pass route.  Same output.
 * BSCGPU_CNT_BATCH_SEGMENTS  (get only) model segments this context modelled and kept.
 * BSCGPU_CNT_BATCH_SEG_RERUNS  (get only) segments run again as halves of one that declined while it ran.
 * BSCGPU_CNT_BATCH_SEG_HOST_BLOCKS  (get only) blocks given to the segmented model that ended on the host model.  After a segmented
 *                          pass BSCGPU_CNT_DC_LAST_FAIL is the OR of those blocks' reasons.
 *                          (Counted per block of the layout: with HBM input a block that rides along untransformed — stored, or left to
 *                          the single path — is planned like any other and counts here if the device leaves it out.)
 * BSCGPU_CNT_DC_DCAP       (get only) decisions the device model's arena holds for this context (a pass or segment above it cannot be modelled):
 *                          4 Mcap + 65536, where Mcap — the runs it holds — is ceil(max_n / BSCGPU_OPT_DC_ARENA_DIV) + 4096 rounded up to 4096.
 * BSCGPU_OPT_BATCH_MODEL_PACKED  0 (default) / 1: with BSCGPU_OPT_BATCH_MODEL on (with or without _SEGMENTS) and -e1, a pass's or a
 *                          segment's stream is written and brought down in the packed 13-bit form (13 bytes per eight decisions instead
 *                          of 16: the pinned landing buffers hold 16 / 13 as many decisions) and coded by bscgpu_front_batch_code_ps13;
 *                          with BSCGPU_OPT_DEVICE_RC the device's range coder reads it as BSCGPU_RC_STATIC13.  A pass whose packed form
 *                          is void goes down as 16-bit entries.  -e0, -e2, the L route and single blocks are not affected.  Same output.
 * BSCGPU_CNT_BATCH_PACKED_PASSES, BSCGPU_CNT_BATCH_PACKED_VOID  (get only) passes or segments of this context that went down packed, and
 *                          those whose packed form was void and went down as 16-bit entries.
 * BSCGPU_OPT_DC_ARENA_DIV  1 (default) / 2 / 4 / 8 (BSC_DC_ARENA_DIV in the environment, read when a context is created, sets the same): the
 *                          device model's arena is carved for the runs and decisions of ceil(max_n / k) bytes instead of max_n — about
 *                          221 / k + 1 bytes per byte of max_n (the avg_rank flags keep their byte per run of the whole block).  A single
 *                          -e1 / -e0 block above that capacity is modelled in segments of whole sub-blocks, one after the other through
 *                          the same two stream buffers, each segment's pieces landing where the whole block's would
 *                          (bscgpu_block_segment_plan cuts; DESIGN §3.6, "A block in sub-block segments"); a block one of whose
 *                          sub-blocks alone exceeds the capacity takes the host model (BSCGPU_DC_FAIL_CAP).  Not combined with
 *                          BSCGPU_OPT_DEVICE_RC: the stream of a block in more than one segment goes down and the host codes it.  Batched
 *                          passes see the smaller capacity (BSCGPU_CNT_DC_DCAP): the segments route cuts finer, a whole-pass model above it
 *                          declines with BSCGPU_DC_FAIL_CAP.  Set while the context's arena exists with another value:
 *                          LIBBSC_NOT_SUPPORTED, nothing changes; other values: LIBBSC_BAD_PARAMETER.  Same output.
 * BSCGPU_CNT_DC_BLOCK_SEGMENTS  (get only) segments the last single block given to the device model of a context with a divided arena ran
 *                          in: 1 = whole, 0 = declined before any ran (or the arena is not divided: such a block takes the whole-block
 *                          route without the plan's facts).  Segments of a packed block count in BSCGPU_CNT_BATCH_PACKED_PASSES, one
 *                          whose packed form was void — re-run as 16-bit entries and packed into place by the host — in _PACKED_VOID.
 * BSCGPU_OPT_DEVICE_LZP    0 (default) / 1 (BSC_DEVICE_LZP=1 in the environment, read when a context is created, sets the same): in
 *                          bscgpu_pipe_submit_host (and so the job driver's blocks) and in the single-block path of bscgpu_compress_batch a
 *                          host block with LZP whose parameters the device stage takes (hashSize 10..15) goes up raw and
 *                          is preprocessed by bscgpu_lzp_compress_device's stage in front of the sorter, instead of by lzp_compress on the
 *                          submitting thread.  A block the stage declines takes the host route.  Same output.  The batched passes of
 *                          bscgpu_compress_batch have an option of their own (BSCGPU_OPT_BATCH_DEVICE_LZP).  bsc_compress runs on default contexts that no caller can set options on and
 *                          decides, before it has one, whether LZP runs on the host: it takes the route from BSC_DEVICE_LZP=1 in the
 *                          environment AS IT STANDS AT THE CALL, not from the option of the context it then gets.
 * BSCGPU_CNT_LZP_BLOCKS    (get only) blocks that route gave to the stage; _LZP_DECLINED: blocks with LZP it left to the host because the
 *                          stage does not take their parameters.
 * BSCGPU_OPT_BATCH_DEVICE_LZP  0 (default) / 1 (BSC_BATCH_DEVICE_LZP=1 in the environment, read when a context is created, sets the same): in
 *                          bscgpu_compress_batch the members of a pass with LZP whose parameters the device stage takes (hashSize 10..15) go
 *                          up raw, and one run of bscgpu_lzp_batch_device's stage per pass makes the sorter's input of them, as
 *                          bscgpu_compress_batch_device_lzp does for input in HBM.  With hashSize >= 16 the pass keeps host LZP and
 *                          BSCGPU_CNT_LZP_DECLINED counts it.  Same output.
 * BSCGPU_CNT_BATCH_LZP_PASSES  (get only) passes, of either call, whose LZP ran as one stage on the device; _BATCH_LZP_BLOCKS: the blocks of
 *                          those passes that went to the sorter.
 * BSCGPU_CNT_LZP_MATCHES   (get only, as the four that follow: of the LAST block — or the last pass — given to the stage, by a route or by
 *                          bscgpu_lzp_compress* / bscgpu_lzp_batch_device, summed over its chunks, saturating) matches taken; _LZP_DIRTY: positions visited whose predecessor a match had
 *                          skipped (they read the real table); _LZP_SERIAL_ZONES: failed verifies (minLen > 16), each followed by a stretch
 *                          run group by group; _LZP_ESCAPES: escaped literals (0xF2 0xFF); _LZP_RAW_CHUNKS: chunks kept raw by the framing.
 * Environment only, no option key: BSC_UNBWT_STEP_CAP (read when a context is created, like BSC_PS13; values below 16 are ignored) is the
 *                          inverse BWT's step cap, 1 << 22 by default — a test knob for the LIBBSC_NOT_SUPPORTED exits (see bscgpu_unbwt).
 * set returns the previous value or a negative libbsc error code; get the value or a negative error code. */
enum { BSCGPU_OPT_RS_ONESWEEP = 1, BSCGPU_CNT_OS_RETRIES = 2, BSCGPU_OPT_DC_PACKED_STREAM = 4,
       BSCGPU_CNT_DC_REPLAYS = 5, BSCGPU_CNT_DC_LAST_FAIL = 6, BSCGPU_CNT_DC_AVG_UNDECIDED = 7, BSCGPU_CNT_DC_HIST_EXTENDED = 8,
       BSCGPU_OPT_BATCH_FRONT = 9, BSCGPU_CNT_BATCH_FRONT_PASSES = 10, BSCGPU_CNT_BATCH_L_PASSES = 11,
       BSCGPU_OPT_DEVICE_RC = 12, BSCGPU_CNT_DEVICE_RC_BLOCKS = 13,
       BSCGPU_OPT_BATCH_MODEL = 14, BSCGPU_CNT_BATCH_MODEL_PASSES = 15, BSCGPU_CNT_BATCH_MODEL_DECLINED = 16,
       BSCGPU_OPT_BATCH_MODEL_FAST = 17, BSCGPU_CNT_BATCH_FAST_PASSES = 18, BSCGPU_CNT_BATCH_FAST_DECLINED = 19,
       BSCGPU_OPT_BWT_FOLD = 20, BSCGPU_CNT_BWT_FOLDED = 21,
       BSCGPU_OPT_BATCH_MODEL_SEGMENTS = 22, BSCGPU_CNT_BATCH_SEGMENTS = 23, BSCGPU_CNT_BATCH_SEG_RERUNS = 24,
       BSCGPU_CNT_BATCH_SEG_HOST_BLOCKS = 25, BSCGPU_CNT_DC_DCAP = 26,
       BSCGPU_OPT_BATCH_MODEL_PACKED = 27, BSCGPU_CNT_BATCH_PACKED_PASSES = 28, BSCGPU_CNT_BATCH_PACKED_VOID = 29,
       BSCGPU_OPT_DC_AVG_EXACT = 30, BSCGPU_CNT_DC_AVG_RESOLVED = 31,
       BSCGPU_OPT_DC_REPLAY_EXACT = 32, BSCGPU_CNT_DC_REPLAY_RESOLVED = 33,
       BSCGPU_OPT_DC_HIST_EXACT = 34, BSCGPU_CNT_DC_HIST_RESOLVED = 35,
       BSCGPU_OPT_DC_ARENA_DIV = 36, BSCGPU_CNT_DC_BLOCK_SEGMENTS = 37,
       BSCGPU_OPT_BATCH_MODEL_ADAPTIVE = 38, BSCGPU_CNT_BATCH_ADAPTIVE_PASSES = 39, BSCGPU_CNT_BATCH_ADAPTIVE_DECLINED = 40,
       BSCGPU_CNT_DC_MIX_CHAINS = 41, BSCGPU_CNT_DC_MIX_LONGEST = 42, BSCGPU_CNT_DC_MIX_WALK_US = 43,
       BSCGPU_OPT_BATCH_ADAPTIVE_SEGMENTS = 44,
       BSCGPU_OPT_DEVICE_LZP = 45, BSCGPU_CNT_LZP_BLOCKS = 46, BSCGPU_CNT_LZP_DECLINED = 47,
       BSCGPU_CNT_LZP_MATCHES = 48, BSCGPU_CNT_LZP_DIRTY = 49, BSCGPU_CNT_LZP_SERIAL_ZONES = 50, BSCGPU_CNT_LZP_ESCAPES = 51,
       BSCGPU_CNT_LZP_RAW_CHUNKS = 52,
       BSCGPU_OPT_BATCH_DEVICE_LZP = 53, BSCGPU_CNT_BATCH_LZP_PASSES = 54, BSCGPU_CNT_BATCH_LZP_BLOCKS = 55 };
/* _FAIL_AVG: undecided avg_rank flags; _FAIL_HIST: a run_hist bracket open after 9216 predecessors (never with
 * BSCGPU_OPT_DC_HIST_EXACT); _FAIL_CAP: more runs or decisions
 * than the context's arena holds; _FAIL_REPLAY: a chain whose bracket stayed open over more than 64 evaluation chunks (with
 * BSCGPU_OPT_DC_REPLAY_EXACT: only behind the resolve's guard); _FAIL_MIX (the adaptive coder's model of a pass only): the longest
 * mixer chain exceeds the step cap. */
enum { BSCGPU_DC_FAIL_AVG = 2, BSCGPU_DC_FAIL_HIST = 4, BSCGPU_DC_FAIL_CAP = 8, BSCGPU_DC_FAIL_REPLAY = 16, BSCGPU_DC_FAIL_MIX = 32 };
BSCGPU_API int bscgpu_option_set(bscgpu_ctx* ctx, int key, int value);
/* Where a single block is cut when the device model's arena holds less than the block (BSCGPU_OPT_DC_ARENA_DIV): pure host arithmetic,
 * no GPU needed.  Sub-blocks in order (nsub in 1..8), sub_runs[s] runs and sub_dec[s] decisions each; consecutive sub-blocks join a
 * segment while the runs stay within mcap and the decisions within dcap (greedy: the fewest contiguous segments).  seg_of[s]: the
 * segment of sub-block s.  Returns the number of segments; LIBBSC_NOT_SUPPORTED when one sub-block alone exceeds a capacity,
 * LIBBSC_BAD_PARAMETER for null pointers, nsub outside 1..8 or a capacity <= 0 — nothing is written then. */
BSCGPU_API int bscgpu_block_segment_plan(const uint32_t* sub_runs, const uint32_t* sub_dec, int nsub, int64_t mcap, int64_t dcap, int* seg_of);
/* The facts that plan is made of, as a stage on its own (tests, tools; like bscgpu_model_segment_facts_device for a pass): the sorted
 * block L[0..n) through the sub-block split and the run / rank front end, then per sub-block its runs, its decisions for `coder`
 * (1: -e1, 3: -e0) and the avg_rank flags the bracket (with BSCGPU_OPT_DC_AVG_EXACT: the resolve) left open (-e0: none).  Arrays of 8. */
BSCGPU_API int bscgpu_qlfc_pstream_facts(bscgpu_ctx* ctx, const uint8_t* L, int n, int coder, int* nblocks, int* sub_start, int* sub_size,
                                         uint32_t* sub_runs, uint32_t* sub_dec, uint32_t* sub_und);
BSCGPU_API int bscgpu_option_get(bscgpu_ctx* ctx, int key);
/* Process-wide counts since start (tests, reports): blocks whose static model ran on the GPU, how many of those were LZP-preprocessed,
 * and blocks that took the device model first and were redone with the model on the host (a sub-block that does not compress has to
 * be stored raw from the run arrays, which the device path never copies); _DEVICE_LZP_BLOCKS: runs of the device's LZP stage in front
 * of a sorter (BSCGPU_OPT_DEVICE_LZP, BSC_DEVICE_LZP=1 for bsc_compress, bscgpu_compress_device_lzp), a redo's second run included. */
enum { BSCGPU_PCNT_DEVICE_MODEL_BLOCKS = 1, BSCGPU_PCNT_REDONE_ON_HOST_MODEL = 2, BSCGPU_PCNT_DEVICE_MODEL_LZP_BLOCKS = 3,
       BSCGPU_PCNT_DEVICE_LZP_BLOCKS = 4 };
BSCGPU_API long long bscgpu_process_counter(int key);

/* ---- how the libbsc.h entry points spread concurrent callers over the GPUs of a node (pure functions, no GPU needed) -------------
 * The host-pointer API keeps ctx_per_dev default contexts per physical device = nphys * ctx_per_dev logical slots; slot s lives
 * on device s % nphys, so every GPU's first context comes before anybody's second one.  A call takes the usable slot whose GPU has
 * the fewest calls in flight (then the slot with the fewest, then a slot marked usable = 2 — its context exists and is large
 * enough — before one that would have to be created; remaining ties in round-robin order from `start`).  The reference has one
 * lock and one device (bwt.cpp:50-52, st.cu:56); its parallelism is the CLI's OpenMP team of concurrent bsc_compress calls
 * (bsc.cpp:184-199), which this rule maps to one block per GPU.  Returns the slot, -1 when no slot is usable. */
BSCGPU_API int bscgpu_dispatch_device(int slot, int nphys);
BSCGPU_API int bscgpu_dispatch_pick(int nphys, int ctx_per_dev, const int* users, const unsigned char* usable, unsigned start);

#ifdef __cplusplus
}
#endif
#endif /* BSCGPU_H */
