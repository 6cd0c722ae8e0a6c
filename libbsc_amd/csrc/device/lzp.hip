// lzp.hip — the LZP encoder on the device, bit-exact with host/lzp.cpp's narrow scanners (hashSize 10..15), in the three stages of
// DESIGN §3.9.  host/lzp_staged.cpp is the same algorithm on the CPU; the tests hold both to lzp_compress.
//
// One implementation serves a single block (lzp_device) and all blocks of a batched pass (lzp_batch_device): both hand lzp_stage the
// chunk table of host/lzp_batch_plan.h — a single block is a pass of one block with 1, 2, 4 or 8 chunks — and every kernel is
// launched once for all chunks of the table.
//
//   A  lzp_key_kernel     thread per byte: key = slot of the position's context << 45 | chunk << 32 | position in the chunk; a
//                         position outside every chunk, or 0..3 of a chunk, which the scanner never enters, gets the slot 2^hashSize.
//      radix_sort_passes  stable, keys only, on the slot bits alone: two 8-bit passes (booked BSCGPU_K_RADIX_AUX)
//      lzp_link_kernel    thread per sorted key: neighbours with the same (slot, chunk) are predecessor and successor — prev0 / next0,
//                         the table's content "as if every position were visited"
//   B  lzp_flag_kernel    thread per byte: occupied0 = prev0 > 0, cand0 = the scanner's two-word probe against prev0, is_flag; one
//                         byte per position.  Also clears the position's dirty byte.
//   C  lzp_sweep_kernel   one workgroup per chunk, the chunk's real table in LDS.  Windows of SWEEP_WINDOW positions, four per thread:
//                         a position whose predecessor a match skipped (dirty) reads the table and probes for itself, every other one
//                         takes its flags; the first candidate of the window ends it, escaped literals in front of it move the output
//                         offset (a prefix sum) and the group phase (a window without a match ends where a group starts).  The
//                         candidate is measured by one wavefront, 512 bytes a step; an accepted match marks dirty[next0[x]] for every
//                         position x it skips.  Where the phase decides — behind a failed verify up to retry_after, and the last
//                         SWEEP_SERIAL_TAIL positions in front of `limit` — thread 0 runs the scanner's own group loop.
//
//      lzp_frame_kernel   the frames: every block's table bytes and payloads (coded from the staging area, raw from the input) moved
//                         into the output from the piece list the host makes of the chunks' results (lzp_batch_plan.h: batch_frame).
//
// Every store of the sweep is to out[0, cap) of its chunk: a window is written only after its last byte is known to lie below
// eob = cap - 8, a group adds at most 6 bytes to an o < eob, a match's length bytes are checked before they are written.  Once o >= eob
// the chunk is NOT_COMPRESSIBLE whatever follows (o only grows), so the sweep stops there.  All loops are bounded by the chunk's length;
// no workgroup waits for another, and global memory sees no atomics.
#include "dev_common.h"
#include "../host/lzp_staged.h"
#include "../host/lzp_batch_plan.h"

using namespace bschost::lzp;

namespace {

static_assert(SWEEP_WINDOW == 4 * WG, "four positions per thread");

__device__ __forceinline__ u32 d_ld32(const u8* p) { u32 v; __builtin_memcpy(&v, p, 4); return v; }
__device__ __forceinline__ u64 d_ld64(const u8* p) { u64 v; __builtin_memcpy(&v, p, 8); return v; }
template <int W>
__device__ __forceinline__ bool d_same(const u8* T, u32 q, u32 ref, int minLen)
{
    const int far = minLen - W;
    if (W == 4) return d_ld32(T + q + far) == d_ld32(T + ref + far) && d_ld32(T + q) == d_ld32(T + ref);
    return d_ld64(T + q + far) == d_ld64(T + ref + far) && d_ld64(T + q) == d_ld64(T + ref);
}

// ---- A --------------------------------------------------------------------------------------------------------------------------------
// Keys are slot << 45 | chunk << 32 | position in the chunk, sorted (stable) on the slot bits alone: chunks ascend in the table, so inside
// a slot the positions stay grouped by chunk and ascending, and neighbours with the same upper word are predecessor and successor.  A
// position that belongs to no chunk (a block refused by size) or that the scanner never enters gets the slot 2^hashSize, behind all.
constexpr int BK_SLOT_SHIFT = 45, BK_CHUNK_SHIFT = 32;
static_assert(BATCH_LZP_MAX_CHUNKS <= 1 << (BK_SLOT_SHIFT - BK_CHUNK_SHIFT), "a chunk's number fits below the slot");

// The chunk that holds position g, from the chunk of a position g0 <= g found before (or -1): the last chunk that starts at or before
// g, if g lies inside it; else -1.  Advances by at most the chunks that start in (g0, g].
__device__ __forceinline__ int chunk_first(const BatchChunk* __restrict__ chunks, int nchunks, u32 g0)
{
    if (nchunks == 0 || chunks[0].start > g0) return -1;
    int lo = 0, hi = nchunks;
    while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (chunks[mid].start <= g0) lo = mid; else hi = mid; }
    return lo;
}
__device__ __forceinline__ int chunk_of(const BatchChunk* __restrict__ chunks, int nchunks, int from, u32 g)
{
    int k = from;
    while (k + 1 < nchunks && chunks[k + 1].start <= g) ++k;
    return k >= 0 && g - chunks[k].start < chunks[k].size ? k : -1;
}

__global__ __launch_bounds__(WG) void lzp_key_kernel(const u8* __restrict__ T, u32 n, const BatchChunk* __restrict__ chunks, int nchunks,
                                                      int hashSize, u64* __restrict__ keys)
{
    const u32 g = blockIdx.x * WG + threadIdx.x;
    if (g >= n) return;
    const int k = chunk_of(chunks, nchunks, chunk_first(chunks, nchunks, blockIdx.x * WG), g);
    u64 key = (u64)(1u << hashSize) << BK_SLOT_SHIFT;
    if (k >= 0) {
        const u32 q = g - chunks[k].start;
        key |= q;
        if (q >= 4) key = (u64)slot_of(ctx_of(T, g), (1u << hashSize) - 1) << BK_SLOT_SHIFT | (u64)k << BK_CHUNK_SHIFT | q;
    }
    keys[g] = key;
}

__global__ __launch_bounds__(WG) void lzp_link_kernel(const u64* __restrict__ keys, u32 n, const BatchChunk* __restrict__ chunks, int nchunks,
                                                       int hashSize, u32* __restrict__ prev0, u32* __restrict__ next0)
{
    const u32 i = blockIdx.x * WG + threadIdx.x;
    if (i >= n) return;
    const u64 key = keys[i];
    const u32 hi = (u32)(key >> 32), q = (u32)key;
    if (hi >> (BK_SLOT_SHIFT - 32 + hashSize)) return;
    const u32 k = hi & ((1u << (BK_SLOT_SHIFT - BK_CHUNK_SHIFT)) - 1);
    if (k >= (u32)nchunks || q >= chunks[k].size) return;      // (cannot be: the key kernel made it from a position of chunk k)
    const u32 g = chunks[k].start + q;
    const u64 kp = i > 0 ? keys[i - 1] : ~0ull, kn = i + 1 < n ? keys[i + 1] : ~0ull;
    prev0[g] = (u32)(kp >> 32) == hi ? (u32)kp : 0u;
    next0[g] = (u32)(kn >> 32) == hi ? (u32)kn : 0u;
}

// ---- B --------------------------------------------------------------------------------------------------------------------------------
template <int W>
__global__ __launch_bounds__(WG) void lzp_flag_kernel(const u8* __restrict__ T, u32 n, const BatchChunk* __restrict__ chunks, int nchunks,
                                                       int minLen, const u32* __restrict__ prev0, u8* __restrict__ flags, u8* __restrict__ dirty)
{
    const u32 g = blockIdx.x * WG + threadIdx.x;
    if (g >= n) return;
    const int k = chunk_of(chunks, nchunks, chunk_first(chunks, nchunks, blockIdx.x * WG), g);
    u8 f = 0;
    if (k >= 0) {
        const u32 start = chunks[k].start, q = g - start;
        const int limit = (int)chunks[k].size - narrow_guard(minLen);
        if (q >= 4) {
            const u32 pv = prev0[g];
            f = (pv > 0 ? F_OCC : 0) | (T[g] == FLAG ? F_FLAG : 0);
            // q + minLen <= limit + 2 + minLen < size: the probe stays inside the chunk
            if (pv > 0 && (int)q < limit + 3 && d_same<W>(T + start, q, pv, minLen)) f |= F_CAND;
        }
    }
    flags[g] = f;
    dirty[g] = 0;
}

// ---- C --------------------------------------------------------------------------------------------------------------------------------
struct SweepState { int p, o, retry, cand; u32 seen; int len, win_m, win_e; u32 cnt[CR_WORDS]; u32 scan[8]; };

// The sweep of one chunk by one workgroup: T, the links, the flag and dirty bytes and out are the chunk's own (its first byte at 0), res its
// result record, table 2^hashSize words of LDS.
template <int W, bool VERIFY>
__device__ __forceinline__ void lzp_sweep_chunk(const u8* const T, const int size, const int cap, int hashSize, int minLen,
                                                const u32* const prev0, const u32* const next0, const u8* const flags, u8* const dirty,
                                                u8* const out, u32* const res, u32* const table, SweepState& S)
{
    const int tid = (int)threadIdx.x;
    const int eob = cap - 8, limit = size - narrow_guard(minLen);
    const u32 mask = (1u << hashSize) - 1;

    for (u32 i = (u32)tid; i <= mask; i += WG) table[i] = 0;
    if (tid < 4) out[tid] = T[tid];
    if (tid < CR_WORDS) S.cnt[tid] = 0;
    int p = 4, o = 4, retry = 0;                               // the scanner's state, the same in every thread
    bool spent = false;
    __syncthreads();

    while (true) {
        const bool tail = p >= limit;                          // finish_tail: no probing, no phase
        if (tail && p >= size) break;
        if (o >= eob) { spent = true; break; }
        int cand = -1; u32 seen = 0;                           // a candidate found at `cand` whose slot held `seen`

        if (!tail && ((VERIFY && p <= retry) || limit - p < SWEEP_SERIAL_TAIL)) {
            // ---- the scanner's group loop (lzp.cpp:63), one thread.  q <= p + 3 < limit + 3: flags, links and the probe are in range
            if (tid == 0) {
                u32 sn = 0, ndirty = 0, nesc = 0;
                while (p < limit && o < eob && ((VERIFY && p <= retry) || limit - p < SWEEP_SERIAL_TAIL)) {
                    const bool probing = !VERIFY || p > retry;
                    int j = 0, kind = 0;
                    for (; j < 4; ++j) {
                        const u32 q = (u32)(p + j);
                        const u8 f = flags[q];
                        const u32 s = slot_of(ctx_of(T, q), mask);
                        bool cd;
                        if (dirty[q]) { sn = table[s]; ++ndirty; cd = probing && sn > 0 && d_same<W>(T, q, sn, minLen); }
                        else          { sn = (f & F_OCC) ? prev0[q] : 0u; cd = probing && (f & F_CAND); }
                        if (q > table[s]) table[s] = q;
                        if (sn > 0) {
                            if (cd) { kind = 1; break; }
                            if (f & F_FLAG) { kind = 2; break; }
                        }
                    }
                    const int lit = kind == 0 ? 4 : j;
                    for (int t = 0; t < lit; ++t) out[o + t] = T[p + t];
                    o += lit; p += lit;
                    if (kind == 2) { out[o] = FLAG; out[o + 1] = 255; o += 2; ++p; ++nesc; }
                    if (kind == 1) { cand = p; break; }
                }
                S.p = p; S.o = o; S.cand = cand; S.seen = sn;
                S.cnt[CR_DIRTY] += ndirty; S.cnt[CR_ESCAPES] += nesc;
            }
            __syncthreads();
            p = S.p; o = S.o; cand = S.cand; seen = S.seen;
        } else {
            // ---- a window: nw positions from p, all in front of `limit` (or all in the tail)
            const int nw = tail ? (size - p < SWEEP_WINDOW ? size - p : SWEEP_WINDOW) : (limit - p < SWEEP_WINDOW ? limit - p : SWEEP_WINDOW);
            if (tid == 0) { S.win_m = nw; S.win_e = -1; }
            __syncthreads();
            const int i0 = 4 * tid;
            u32 sn[4]; int ev[4]; bool dt[4]; u32 sl[4]; u8 by[4];    // per position: slot content, 0 literal / 1 candidate / 2 escaped literal
            int first = nw;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int i = i0 + j;
                sn[j] = 0; ev[j] = 0; dt[j] = false; sl[j] = 0; by[j] = 0;
                if (i < nw) {
                    const u32 q = (u32)(p + i);
                    const u8 f = flags[q];
                    by[j] = T[q];
                    sl[j] = slot_of(ctx_of(T, q), mask);
                    dt[j] = dirty[q] != 0;
                    bool cd;
                    if (dt[j]) { sn[j] = table[sl[j]]; cd = !tail && sn[j] > 0 && d_same<W>(T, q, sn[j], minLen); }   // the table as the window found it
                    else       { sn[j] = (f & F_OCC) ? 1u : 0u; cd = !tail && (f & F_CAND); }
                    if (sn[j] > 0) ev[j] = cd ? 1 : ((f & F_FLAG) ? 2 : 0);
                    if (ev[j] == 1 && i < first) first = i;
                }
            }
            if (first < nw) atomicMin(&S.win_m, first);
            __syncthreads();                                   // (every dirty position has read the table: the window may write it)
            const int m = S.win_m;
            u32 my_esc = 0; int my_last = -1;
#pragma unroll
            for (int j = 0; j < 4; ++j) if (i0 + j < m && ev[j] == 2) { ++my_esc; my_last = i0 + j; }
            if (my_last >= 0) atomicMax(&S.win_e, my_last);
            u32 nesc = 0;
            const u32 esc_before = block_excl_sum(my_esc, S.scan, &nesc);      // (two barriers: win_e is complete behind them)
            const int e = S.win_e;
            // without a match the window ends where a group starts: groups restart behind an escaped literal
            const int end = (m == nw && !tail) ? e + 1 + ((nw - (e + 1)) & ~3) : m;
            if (o + end + (int)nesc >= eob) { spent = true; break; }
            int off = o + i0 + (int)esc_before;
            u32 ndirty = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int i = i0 + j;
                if (i < end) {
                    out[off++] = by[j];
                    if (ev[j] == 2) out[off++] = 255;
                }
                if (i < end || (i == m && m < nw)) {           // visited: the candidate's position too
                    atomicMax(&table[sl[j]], (u32)(p + i));
                    ndirty += dt[j];
                    if (i == m) S.seen = dt[j] ? sn[j] : prev0[p + i];
                }
            }
            if (ndirty) atomicAdd(&S.cnt[CR_DIRTY], ndirty);
            if (tid == 0) S.cnt[CR_ESCAPES] += nesc;
            __syncthreads();
            p += end; o += end + (int)nesc;
            if (m < nw) { cand = p; seen = S.seen; }
        }

        if (cand >= 0) {
            // ---- measure the candidate (lzp.cpp:103-110): one wavefront, lane l compares the stride at len + 8 l
            if (tid < 64) {
                int len = VERIFY ? 8 : minLen;
                while (true) {
                    const int L = len + 8 * tid;
                    const bool active = cand + L < limit;      // a stride that starts before `limit` is compared in full: it ends below size
                    u64 x = 0;
                    if (active) x = d_ld64(T + cand + L) ^ d_ld64(T + seen + L);
                    const u64 stop = __ballot(!active || x != 0);
                    if (stop) {
                        if (tid == (int)__builtin_ctzll(stop)) S.len = active ? L + (int)(__builtin_ctzll(x) >> 3) : L;
                        break;
                    }
                    len += 512;
                }
            }
            __syncthreads();
            const int len = S.len;
            if (VERIFY && len < minLen) {                      // not a match after all: a literal, and no probing up to the failure
                const u8 bb = T[cand];
                if (tid == 0) {
                    out[o] = bb;
                    if (bb == FLAG) { out[o + 1] = 255; ++S.cnt[CR_ESCAPES]; }
                    ++S.cnt[CR_ZONES];
                }
                retry = cand + len; o += 1 + (bb == FLAG); p = cand + 1;
            } else {
                const int excess = len - minLen, k = excess / 254;
                if (k >= 1 && o + 1 + k >= eob) { spent = true; break; }       // put_match's check behind every 254
                if (tid == 0) { out[o] = FLAG; out[o + 1 + k] = (u8)(excess - 254 * k); ++S.cnt[CR_MATCHES]; }
                for (int i = tid; i < k; i += WG) out[o + 1 + i] = 254;
                // the positions the match skips never enter the table: whoever has one of them as predecessor must ask the table
                for (int x = cand + 1 + tid; x < cand + len; x += WG) { const u32 d = next0[x]; if (d) dirty[d] = 1; }
                o += k + 2; p = cand + len;
            }
            __syncthreads();                                   // the marks and S.len's next writer
        }
    }
    __syncthreads();
    if (tid == 0) {
        res[CR_RES] = (spent || o >= eob) ? (u32)BSC_NOT_COMPRESSIBLE : (u32)o;
        for (int t = 1; t < CR_WORDS; ++t) res[t] = S.cnt[t];
    }
}

template <int W, bool VERIFY>
__global__ __launch_bounds__(WG) void lzp_sweep_kernel(const u8* __restrict__ Tall, const BatchChunk* __restrict__ chunks, int hashSize,
                                                        int minLen, const u32* __restrict__ prev0_all, const u32* __restrict__ next0_all,
                                                        const u8* __restrict__ flags_all, u8* dirty_all, u8* out_all, u32* __restrict__ res)
{
    extern __shared__ u32 table[];                             // 2^hashSize words: the last VISITED position of every slot, 0 = none
    __shared__ SweepState S;
    const BatchChunk C = chunks[blockIdx.x];
    lzp_sweep_chunk<W, VERIFY>(Tall + C.start, (int)C.size, (int)C.cap, hashSize, minLen, prev0_all + C.start, next0_all + C.start,
                               flags_all + C.start, dirty_all + C.start, out_all + C.start, res + blockIdx.x * CR_WORDS, table, S);
}

// ---- the frames -----------------------------------------------------------------------------------------------------------------------
// All pieces in one launch: piece p is moved by the workgroups wg_first[p] .. wg_first[p + 1] - 1, FRAME_SPAN bytes each, as aligned
// words of the output with the bytes in front of and behind them one by one.
constexpr u32 FRAME_SPAN = 16384;
__global__ __launch_bounds__(WG) void lzp_frame_kernel(const BatchPiece* __restrict__ pieces, const u32* __restrict__ wg_first, u32 npieces,
                                                        const u8* __restrict__ staging, const u8* __restrict__ raw,
                                                        const u8* __restrict__ tab, u8* __restrict__ out)
{
    const u32 tid = threadIdx.x;
    u32 lo = 0, hi = npieces;
    while (hi - lo > 1) { const u32 mid = (lo + hi) >> 1; if (wg_first[mid] <= blockIdx.x) lo = mid; else hi = mid; }
    const BatchPiece P = pieces[lo];
    const u32 from = (blockIdx.x - wg_first[lo]) * FRAME_SPAN;
    if (from >= P.len) return;
    const u32 len = P.len - from < FRAME_SPAN ? P.len - from : FRAME_SPAN;
    const u8* const src = (P.src == PIECE_STAGING ? staging : P.src == PIECE_RAW ? raw : tab) + P.src_off + from;
    u8* const dst = out + P.dst_off + from;
    u32 head = (u32)(0 - (size_t)dst) & 3u; if (head > len) head = len;
    const u32 words = (len - head) >> 2, behind = head + 4 * words;
    if (tid < head) dst[tid] = src[tid];
    for (u32 w = tid; w < words; w += WG) *reinterpret_cast<u32*>(dst + head + 4 * w) = d_ld32(src + head + 4 * w);
    if (tid < len - behind) dst[behind + tid] = src[behind + tid];
}

// ---- the stage ------------------------------------------------------------------------------------------------------------------------
// c->lzp_tab (HBM) and c->lzp_tab_host (pinned), the same map: nothing of it is an arena buffer, so the sort in the middle of the stage
// and whatever follows the stage leave it alone.  Allocated by the first call of either entry point.
constexpr size_t LT_CHUNKS = 0;                                                              // BatchChunk [BATCH_LZP_MAX_CHUNKS]
constexpr size_t LT_RES    = LT_CHUNKS + sizeof(BatchChunk) * BATCH_LZP_MAX_CHUNKS;          // u32 [BATCH_LZP_MAX_CHUNKS][CR_WORDS]
constexpr size_t LT_PIECES = LT_RES + (size_t)4 * CR_WORDS * BATCH_LZP_MAX_CHUNKS;           // BatchPiece [BATCH_LZP_MAX_PIECES]
constexpr size_t LT_WG     = LT_PIECES + sizeof(BatchPiece) * BATCH_LZP_MAX_PIECES;          // u32 [BATCH_LZP_MAX_PIECES + 1]
constexpr size_t LT_TABLE  = LT_WG + (((size_t)4 * (BATCH_LZP_MAX_PIECES + 1) + 255) & ~(size_t)255);   // the blocks' table bytes
constexpr size_t LT_BYTES  = LT_TABLE + (size_t)BATCH_LZP_TABLE_BYTES * BATCH_LZP_MAX_BLOCKS;
static_assert(sizeof(BatchChunk) == 16 && sizeof(BatchPiece) == 16, "the kernels read the host's records as they stand");
// a single block has up to eight chunks whatever its size: 8 entries, a table of 1 + 8 * 8 bytes and eight payloads
static_assert(BATCH_LZP_MAX_CHUNKS >= 8 && BATCH_LZP_MAX_PIECES >= 1 + 8, "a single block's chunks and pieces fit LT_CHUNKS / LT_RES and LT_PIECES / LT_WG");
static_assert((size_t)BATCH_LZP_TABLE_BYTES * BATCH_LZP_MAX_BLOCKS >= 1 + 8 * 8, "a single block's table fits LT_TABLE");

int lzp_tab_ensure(bscgpu_ctx* c)
{
    if (c->lzp_tab && c->lzp_tab_host) return BSC_NO_ERROR;
    if (!c->lzp_tab_host && hipHostMalloc((void**)&c->lzp_tab_host, LT_BYTES, hipHostMallocDefault) != hipSuccess) {
        (void)hipGetLastError(); c->lzp_tab_host = nullptr;
        return ctx_fail(c, BSC_NOT_ENOUGH_MEMORY, "LZP stage: pinned tables", hipSuccess);
    }
    if (!c->lzp_tab && hipMalloc((void**)&c->lzp_tab, LT_BYTES) != hipSuccess) {
        (void)hipGetLastError(); c->lzp_tab = nullptr;
        return ctx_fail(c, BSC_GPU_NOT_ENOUGH_MEMORY, "LZP stage: tables", hipSuccess);
    }
    c->lzp_tab_bytes = LT_BYTES;
    return BSC_NO_ERROR;
}

template <int W, bool VERIFY>
int launch_sweep(bscgpu_ctx* c, int nchunks, size_t lds, const u8* T, const BatchChunk* chunks, int hashSize, int minLen, const u32* prev0,
                 const u32* next0, const u8* flags, u8* dirty, u8* out, u32* res)
{
    const int bit = 1 << ((W == 8) + VERIFY);                  // the limit is a per-device attribute of the function: once per context
    if (!(c->lzp_lds_set & bit)) {
        HIP_TRY(c, hipFuncSetAttribute((const void*)lzp_sweep_kernel<W, VERIFY>, hipFuncAttributeMaxDynamicSharedMemorySize, 4 << STAGED_MAX_HASH));
        c->lzp_lds_set |= bit;
    }
    hipLaunchKernelGGL((lzp_sweep_kernel<W, VERIFY>), dim3(nchunks), dim3(WG), lds, c->stream, T, chunks, hashSize, minLen,
                       prev0, next0, flags, dirty, out, res);
    return BSC_NO_ERROR;
}

// Stages A, B and C over the chunk table the caller left in the pinned mirror: the table goes up, the chunks' result records come down, one
// sync.  Arena roles, all dead between two blocks and sized by max_n, serving a pass as they serve a block: kA / kB the sort's keys,
// vA / vB the links, flags and SA the flag and dirty bytes, ISA the chunks' staging.  The input is read where it lies.
int lzp_sweeps(bscgpu_ctx* c, const u8* dIn, u32 N, int nchunks, int hashSize, int minLen)
{
    const u32 grid = (N + WG - 1) / WG;
    unsigned char* const H = c->lzp_tab_host;
    u64 *keys = c->kA, *keys_alt = c->kB;
    u32 *prev0 = c->vA, *next0 = c->vB;
    u8 *flags = c->flags, *dirty = reinterpret_cast<u8*>(c->SA), *staging = reinterpret_cast<u8*>(c->ISA);
    const BatchChunk* dchunks = reinterpret_cast<const BatchChunk*>(c->lzp_tab + LT_CHUNKS);
    u32* res = reinterpret_cast<u32*>(c->lzp_tab + LT_RES);
    HIP_TRY(c, hipMemcpyAsync(c->lzp_tab + LT_CHUNKS, H + LT_CHUNKS, sizeof(BatchChunk) * (size_t)nchunks, hipMemcpyHostToDevice, c->stream));

    prof_begin(c, BSCGPU_K_LZP, (u64)N * 9, N);
    hipLaunchKernelGGL(lzp_key_kernel, dim3(grid), dim3(WG), 0, c->stream, dIn, N, dchunks, nchunks, hashSize, keys);
    prof_end(c);
    HIP_TRY(c, hipGetLastError());
    const int kbits = hashSize + 1;                            // the slot and the bit of the positions behind all slots: two passes
    const RadixPass passes[2] = {{BK_SLOT_SHIFT, 8}, {BK_SLOT_SHIFT + 8, kbits - 8}};
    int in_alt = 0;
    RC_TRY(radix_sort_passes(c, keys, keys_alt, nullptr, nullptr, N, passes, 2, &in_alt, nullptr, /* aux */ true));
    const u64* sorted = in_alt ? keys_alt : keys;

    const int W = narrow_word(minLen);
    const bool verify = narrow_verify(minLen);
    prof_begin(c, BSCGPU_K_LZP, (u64)N * 30, N);
    hipLaunchKernelGGL(lzp_link_kernel, dim3(grid), dim3(WG), 0, c->stream, sorted, N, dchunks, nchunks, hashSize, prev0, next0);
    if (W == 4) hipLaunchKernelGGL(lzp_flag_kernel<4>, dim3(grid), dim3(WG), 0, c->stream, dIn, N, dchunks, nchunks, minLen, prev0, flags, dirty);
    else        hipLaunchKernelGGL(lzp_flag_kernel<8>, dim3(grid), dim3(WG), 0, c->stream, dIn, N, dchunks, nchunks, minLen, prev0, flags, dirty);
    prof_end(c);
    HIP_TRY(c, hipGetLastError());

    const size_t lds = (size_t)4 << hashSize;
    prof_begin(c, BSCGPU_K_LZP, (u64)N * 4, N);
    if (verify)      RC_TRY((launch_sweep<8, true >(c, nchunks, lds, dIn, dchunks, hashSize, minLen, prev0, next0, flags, dirty, staging, res)));
    else if (W == 8) RC_TRY((launch_sweep<8, false>(c, nchunks, lds, dIn, dchunks, hashSize, minLen, prev0, next0, flags, dirty, staging, res)));
    else             RC_TRY((launch_sweep<4, false>(c, nchunks, lds, dIn, dchunks, hashSize, minLen, prev0, next0, flags, dirty, staging, res)));
    prof_end(c);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(H + LT_RES, res, (size_t)nchunks * CR_WORDS * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, ctx_sync(c));
    prof_collect(c);
    return BSC_NO_ERROR;
}

// The stage on c->stream for `count` blocks back to back at dIn, N bytes in all, whose chunk table (nchunks entries) the caller has
// planned into the pinned mirror: the sweeps, then on the host the results and the piece list (batch_frame), then the frame kernel
// into dOut.  results[b] = what lzp_compress returns for block b; c->lzp_last: the paths taken, summed.  One sync for the chunks'
// results; final_sync: a second one behind the frame kernel (a caller that goes on in c->stream does not need it).  place: dev_common.h.
int lzp_stage(bscgpu_ctx* c, const u8* dIn, u8* dOut, const int* sizes, int count, u32 N, int nchunks, int hashSize, int minLen, int features,
              int* results, bool final_sync, const LzpBatchPlace* place)
{
    unsigned char* const H = c->lzp_tab_host;
    const BatchChunk* const hchunks = reinterpret_cast<const BatchChunk*>(H + LT_CHUNKS);
    BatchPiece* const hpieces = reinterpret_cast<BatchPiece*>(H + LT_PIECES);
    const u32* hres = reinterpret_cast<const u32*>(H + LT_RES);
    if (nchunks > 0) RC_TRY(lzp_sweeps(c, dIn, N, nchunks, hashSize, minLen));
    else if (place) HIP_TRY(c, ctx_sync(c));                   // (no block reaches the encoder; the piece list of the call before may still be going up)

    std::vector<int> own((size_t)nchunks);
    for (int k = 0; k < nchunks; ++k) {
        const u32* r = hres + (size_t)k * CR_WORDS;
        own[(size_t)k] = (int)r[CR_RES];
        if (own[(size_t)k] >= 0 && (u32)own[(size_t)k] > hchunks[k].cap)
            return ctx_fail(c, BSC_GPU_ERROR, "LZP stage: a chunk's size is out of range", hipSuccess);
        count_chunk(c->lzp_last, r);
    }
    std::vector<u32> dst;
    std::vector<unsigned char> as_it_is;
    if (place) {                                               // the caller packs the pass: it says where every block goes once it knows the results
        batch_results(sizes, count, minLen, features, own.data(), results);
        dst.assign((size_t)count + 1, BATCH_NOWHERE); as_it_is.assign((size_t)count + 1, 0);
        (*place)(results, dst.data(), as_it_is.data());
    }
    const int np = batch_frame(sizes, count, minLen, features, own.data(), results, hpieces, H + LT_TABLE, &c->lzp_last[CNT_RAW_CHUNKS],
                               place ? dst.data() : nullptr, place ? as_it_is.data() : nullptr);
    if (np > 0) {
        u32* const hwg = reinterpret_cast<u32*>(H + LT_WG);
        u32 wgs = 0, tab_bytes = 0;
        for (int p = 0; p < np; ++p) {
            hwg[p] = wgs; wgs += (hpieces[p].len + FRAME_SPAN - 1) / FRAME_SPAN;
            if (hpieces[p].src == PIECE_TABLE) tab_bytes = hpieces[p].src_off + hpieces[p].len;
        }
        hwg[np] = wgs;
        HIP_TRY(c, hipMemcpyAsync(c->lzp_tab + LT_PIECES, hpieces, sizeof(BatchPiece) * (size_t)np, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, hipMemcpyAsync(c->lzp_tab + LT_WG, hwg, (size_t)4 * (np + 1), hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, hipMemcpyAsync(c->lzp_tab + LT_TABLE, H + LT_TABLE, tab_bytes, hipMemcpyHostToDevice, c->stream));
        prof_begin(c, BSCGPU_K_LZP, (u64)N * 2, N);
        hipLaunchKernelGGL(lzp_frame_kernel, dim3(wgs), dim3(WG), 0, c->stream, reinterpret_cast<const BatchPiece*>(c->lzp_tab + LT_PIECES),
                           reinterpret_cast<const u32*>(c->lzp_tab + LT_WG), (u32)np, reinterpret_cast<const u8*>(c->ISA), dIn,
                           c->lzp_tab + LT_TABLE, dOut);
        prof_end(c);
        HIP_TRY(c, hipGetLastError());
    }
    if (final_sync) { HIP_TRY(c, ctx_sync(c)); prof_collect(c); }
    return BSC_NO_ERROR;
}

}  // namespace

// A single block: a pass of one block, read from c->dT.
int lzp_device(bscgpu_ctx* c, const u8* dIn, u8* dOut, int n, int hashSize, int minLen, int features, bool final_sync)
{
    for (auto& v : c->lzp_last) v = 0;
    if (hashSize > STAGED_MAX_HASH) return BSC_NOT_SUPPORTED;           // the table of a chunk would not fit LDS; the wide scanner is another algorithm
    if (n > c->max_n) return BSC_GPU_NOT_ENOUGH_MEMORY;
    if (num_chunks(n) == 1 && batch_refused_by_size(n, minLen)) return BSC_NOT_COMPRESSIBLE;       // (chunks of a larger block are 128 KiB and more)
    RC_TRY(lzp_tab_ensure(c));
    const int nchunks = plan_block(n, minLen, 0, 0, reinterpret_cast<BatchChunk*>(c->lzp_tab_host + LT_CHUNKS));
    // dOut may be dIn, and the frame kernel reads raw chunks while dOut is being written: the stage reads the block in dT
    if (dIn != c->dT) HIP_TRY(c, hipMemcpyAsync(c->dT, dIn, (size_t)n, hipMemcpyDeviceToDevice, c->stream));
    int result = 0;
    RC_TRY(lzp_stage(c, c->dT, dOut, &n, 1, (u32)n, nchunks, hashSize, minLen, features, &result, final_sync, nullptr));
    return result;
}

// A pass: the public batch call's limits (batch_plan), then the stage where the pass lies.
int lzp_batch_device(bscgpu_ctx* c, const u8* dIn, u8* dOut, const int* sizes, int count, int hashSize, int minLen, int features, int* results,
                     bool final_sync, const LzpBatchPlace* place)
{
    for (auto& v : c->lzp_last) v = 0;
    if (hashSize > STAGED_MAX_HASH) return BSC_NOT_SUPPORTED;
    if (count < 0 || count > BATCH_LZP_MAX_BLOCKS) return BSC_BAD_PARAMETER;
    RC_TRY(lzp_tab_ensure(c));
    const int nchunks = batch_plan(sizes, count, minLen, reinterpret_cast<BatchChunk*>(c->lzp_tab_host + LT_CHUNKS));
    if (nchunks < 0) return nchunks;
    int64_t total = 0;
    for (int b = 0; b < count; ++b) total += sizes[b];
    if (total > c->max_n) return BSC_BAD_PARAMETER;
    return lzp_stage(c, dIn, dOut, sizes, count, (u32)total, nchunks, hashSize, minLen, features, results, final_sync, place);
}

extern "C" int bscgpu_lzp_batch_device(bscgpu_ctx* c, const void* dIn, void* dOut, const int* sizes, int count, int hashSize, int minLen,
                                       int features, int* results)
{
    if (!c || !dIn || !dOut || count < 0 || (count > 0 && (!sizes || !results)) || minLen < 4 || minLen > 255 || hashSize < 10 || hashSize > 28)
        return BSC_BAD_PARAMETER;
    if (hipSetDevice(c->device) != hipSuccess) return BSC_GPU_ERROR;
    return lzp_batch_device(c, (const u8*)dIn, (u8*)dOut, sizes, count, hashSize, minLen, features, results, true, nullptr);
}

static int lzp_args(const bscgpu_ctx* c, const void* in, const void* out, int n, int hashSize, int minLen)
{
    if (!c || !in || !out || n < 0 || minLen < 4 || minLen > 255 || hashSize < 10 || hashSize > 28) return BSC_BAD_PARAMETER;
    return BSC_NO_ERROR;
}

extern "C" int bscgpu_lzp_compress_device(bscgpu_ctx* c, const void* dIn, void* dOut, int n, int hashSize, int minLen, int features)
{
    RC_TRY(lzp_args(c, dIn, dOut, n, hashSize, minLen));
    if (hipSetDevice(c->device) != hipSuccess) return BSC_GPU_ERROR;
    return lzp_device(c, (const u8*)dIn, (u8*)dOut, n, hashSize, minLen, features, true);
}

extern "C" int bscgpu_lzp_compress(bscgpu_ctx* c, const uint8_t* in, uint8_t* out, int n, int hashSize, int minLen, int features)
{
    RC_TRY(lzp_args(c, in, out, n, hashSize, minLen));
    if (hashSize > STAGED_MAX_HASH) return BSC_NOT_SUPPORTED;
    if (n > c->max_n) return BSC_GPU_NOT_ENOUGH_MEMORY;
    if (hipSetDevice(c->device) != hipSuccess) return BSC_GPU_ERROR;
    if (n > 0) HIP_TRY(c, hipMemcpyAsync(c->dT, in, (size_t)n, hipMemcpyHostToDevice, c->stream));
    const int r = lzp_device(c, c->dT, c->dL, n, hashSize, minLen, features, false);
    if (r < 0) { (void)ctx_sync(c); return r; }               // (the upload reads the caller's buffer)
    HIP_TRY(c, hipMemcpyAsync(out, c->dL, (size_t)r, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, ctx_sync(c));
    prof_collect(c);                                           // (the frame kernel's range)
    return r;
}
