// lzp.hip — the LZP encoder on the device, bit-exact with host/lzp.cpp's narrow scanners (hashSize 10..15), in the three stages of
// DESIGN §3.9.  host/lzp_staged.cpp is the same algorithm on the CPU; the tests hold both to lzp_compress.
//
//   A  lzp_key_kernel     thread per byte: key = (chunk << hashSize | slot of the position's context) << 32 | position in the chunk;
//                         positions 0..3 of a chunk, which the scanner never enters, get a chunk number past the last.
//      radix_sort_passes  stable, keys only, on the (chunk, slot) bits: two or three 8-bit passes (booked BSCGPU_K_RADIX_AUX)
//      lzp_link_kernel    thread per sorted key: neighbours with the same (chunk, slot) are predecessor and successor — prev0 / next0,
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
// Every store of the sweep is to out[0, cap) of its chunk: a window is written only after its last byte is known to lie below
// eob = cap - 8, a group adds at most 6 bytes to an o < eob, a match's length bytes are checked before they are written.  Once o >= eob
// the chunk is NOT_COMPRESSIBLE whatever follows (o only grows), so the sweep stops there.  All loops are bounded by the chunk's length;
// no workgroup waits for another, and global memory sees no atomics.
#include "dev_common.h"
#include "../host/lzp_staged.h"

using namespace bschost::lzp;

namespace {

constexpr int DS_LZP = DS_AUX;                                 // dscal / hscal: CR_WORDS per chunk; a context runs no BWT round inside this stage
constexpr int DS_LZP_TABLE = DS_LZP + 8 * CR_WORDS;            // hscal only: the frame's table on its way up
static_assert(DS_LZP_TABLE * 4 + 1 + 8 * 8 <= (DS_AUX + DS_AUX_LEN) * 4, "results and table fit the words of the aux indexes");
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
__global__ __launch_bounds__(WG) void lzp_key_kernel(const u8* __restrict__ T, u32 n, int nc, int hashSize, u64* __restrict__ keys)
{
    const u32 g = blockIdx.x * WG + threadIdx.x;
    if (g >= n) return;
    const u32 per = n / (u32)nc;
    u32 b = g / per; if (b >= (u32)nc) b = (u32)nc - 1;
    const u32 q = g - b * per;
    u32 hi = 8u << hashSize;                                   // not a position the scanner enters: behind every chunk's keys
    if (q >= 4) hi = (b << hashSize) | slot_of(ctx_of(T, g), (1u << hashSize) - 1);
    keys[g] = ((u64)hi << 32) | q;
}

__global__ __launch_bounds__(WG) void lzp_link_kernel(const u64* __restrict__ keys, u32 n, int nc, int hashSize,
                                                       u32* __restrict__ prev0, u32* __restrict__ next0)
{
    const u32 i = blockIdx.x * WG + threadIdx.x;
    if (i >= n) return;
    const u64 k = keys[i];
    const u32 hi = (u32)(k >> 32), q = (u32)k;
    if (hi >= (8u << hashSize)) return;
    const u32 g = (hi >> hashSize) * (n / (u32)nc) + q;
    if (g >= n) return;                                        // (cannot be: the key kernel made it from a position below n)
    const u64 kp = i > 0 ? keys[i - 1] : ~0ull, kn = i + 1 < n ? keys[i + 1] : ~0ull;
    prev0[g] = (u32)(kp >> 32) == hi ? (u32)kp : 0u;
    next0[g] = (u32)(kn >> 32) == hi ? (u32)kn : 0u;
}

// ---- B --------------------------------------------------------------------------------------------------------------------------------
template <int W>
__global__ __launch_bounds__(WG) void lzp_flag_kernel(const u8* __restrict__ T, u32 n, int nc, int minLen, const u32* __restrict__ prev0,
                                                       u8* __restrict__ flags, u8* __restrict__ dirty)
{
    const u32 g = blockIdx.x * WG + threadIdx.x;
    if (g >= n) return;
    const u32 per = n / (u32)nc;
    u32 b = g / per; if (b >= (u32)nc) b = (u32)nc - 1;
    const u32 start = b * per, q = g - start;
    const int size = (int)(b != (u32)nc - 1 ? per : n - start), limit = size - narrow_guard(minLen);
    u8 f = 0;
    if (q >= 4) {
        const u32 pv = prev0[g];
        f = (pv > 0 ? F_OCC : 0) | (T[g] == FLAG ? F_FLAG : 0);
        // q + minLen <= limit + 2 + minLen < size: the probe stays inside the chunk
        if (pv > 0 && (int)q < limit + 3 && d_same<W>(T + start, q, pv, minLen)) f |= F_CAND;
    }
    flags[g] = f;
    dirty[g] = 0;
}

// ---- C --------------------------------------------------------------------------------------------------------------------------------
struct SweepState { int p, o, retry, cand; u32 seen; int len, win_m, win_e; u32 cnt[CR_WORDS]; u32 scan[8]; };

template <int W, bool VERIFY>
__global__ __launch_bounds__(WG) void lzp_sweep_kernel(const u8* __restrict__ Tall, u32 n, int nc, int hashSize, int minLen, int single_cap,
                                                        const u32* __restrict__ prev0_all, const u32* __restrict__ next0_all,
                                                        const u8* __restrict__ flags_all, u8* dirty_all, u8* out_all, u32* __restrict__ res)
{
    extern __shared__ u32 table[];                             // 2^hashSize words: the last VISITED position of every slot, 0 = none
    __shared__ SweepState S;
    const int tid = (int)threadIdx.x, b = (int)blockIdx.x;
    const u32 start = (u32)b * (n / (u32)nc);
    const int size = (int)(b != nc - 1 ? n / (u32)nc : n - start);
    const u8* const T = Tall + start;
    const u32* const prev0 = prev0_all + start; const u32* const next0 = next0_all + start;
    const u8* const flags = flags_all + start;
    u8* const dirty = dirty_all + start; u8* const out = out_all + start;
    const int cap = nc == 1 ? single_cap : size, eob = cap - 8, limit = size - narrow_guard(minLen);
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
        res[b * CR_WORDS + CR_RES] = (spent || o >= eob) ? (u32)BSC_NOT_COMPRESSIBLE : (u32)o;
        for (int t = 1; t < CR_WORDS; ++t) res[b * CR_WORDS + t] = S.cnt[t];
    }
}

template <int W, bool VERIFY>
int launch_sweep(bscgpu_ctx* c, int nc, size_t lds, const u8* T, u32 n, int hashSize, int minLen, const u32* prev0, const u32* next0,
                 const u8* flags, u8* dirty, u8* out, u32* res)
{
    const int bit = 1 << ((W == 8) + VERIFY);                  // the limit is a per-device attribute of the function: once per context
    if (!(c->lzp_lds_set & bit)) {
        HIP_TRY(c, hipFuncSetAttribute((const void*)lzp_sweep_kernel<W, VERIFY>, hipFuncAttributeMaxDynamicSharedMemorySize, 4 << STAGED_MAX_HASH));
        c->lzp_lds_set |= bit;
    }
    hipLaunchKernelGGL((lzp_sweep_kernel<W, VERIFY>), dim3(nc), dim3(WG), lds, c->stream, T, n, nc, hashSize, minLen, (int)n - 2,
                       prev0, next0, flags, dirty, out, res);
    return BSC_NO_ERROR;
}

}  // namespace

// The stage on c->stream: dIn (HBM, n bytes; may be c->dT, may be dOut) -> what lzp_compress returns, the same bytes in dOut (HBM, n
// bytes; may be c->dL).  Arena roles, all dead between two blocks: dT the raw input, kA / kB the sort's keys, vA / vB the links, flags
// and SA the flag and dirty bytes, ISA the chunks' staging.  One sync for the chunks' results; final_sync: a second one behind the
// frame's copies (a caller that goes on in c->stream does not need it).
int lzp_device(bscgpu_ctx* c, const u8* dIn, u8* dOut, int n, int hashSize, int minLen, int features, bool final_sync)
{
    for (auto& v : c->lzp_last) v = 0;
    if (hashSize > STAGED_MAX_HASH) return BSC_NOT_SUPPORTED;           // the table of a chunk would not fit LDS; the wide scanner is another algorithm
    if (n > c->max_n) return BSC_GPU_NOT_ENOUGH_MEMORY;
    const int nc = num_chunks(n);
    if (nc == 1 && ((int64_t)n - minLen < 32 || n - 2 < 16)) return BSC_NOT_COMPRESSIBLE;      // lzp.cpp:531 (chunks of a larger block are 128 KiB and more)
    const u32 N = (u32)n, grid = (N + WG - 1) / WG;
    u64 *keys = c->kA, *keys_alt = c->kB;
    u32 *prev0 = c->vA, *next0 = c->vB;
    u8 *flags = c->flags, *dirty = reinterpret_cast<u8*>(c->SA), *staging = reinterpret_cast<u8*>(c->ISA);
    u32* res = c->dscal + DS_LZP;
    if (dIn != c->dT) HIP_TRY(c, hipMemcpyAsync(c->dT, dIn, (size_t)n, hipMemcpyDeviceToDevice, c->stream));

    prof_begin(c, BSCGPU_K_LZP, (u64)n * 9, N);
    hipLaunchKernelGGL(lzp_key_kernel, dim3(grid), dim3(WG), 0, c->stream, c->dT, N, nc, hashSize, keys);
    prof_end(c);
    HIP_TRY(c, hipGetLastError());
    const int kbits = hashSize + 4, npass = (kbits + 7) / 8;
    RadixPass passes[3];
    for (int p = 0; p < npass; ++p) { passes[p].shift = 32 + 8 * p; passes[p].bits = kbits - 8 * p < 8 ? kbits - 8 * p : 8; }
    int in_alt = 0;
    RC_TRY(radix_sort_passes(c, keys, keys_alt, nullptr, nullptr, N, passes, npass, &in_alt, nullptr, /* aux */ true));
    const u64* sorted = in_alt ? keys_alt : keys;

    const int W = narrow_word(minLen);
    const bool verify = narrow_verify(minLen);
    prof_begin(c, BSCGPU_K_LZP, (u64)n * 30, N);
    hipLaunchKernelGGL(lzp_link_kernel, dim3(grid), dim3(WG), 0, c->stream, sorted, N, nc, hashSize, prev0, next0);
    if (W == 4) hipLaunchKernelGGL(lzp_flag_kernel<4>, dim3(grid), dim3(WG), 0, c->stream, c->dT, N, nc, minLen, prev0, flags, dirty);
    else        hipLaunchKernelGGL(lzp_flag_kernel<8>, dim3(grid), dim3(WG), 0, c->stream, c->dT, N, nc, minLen, prev0, flags, dirty);
    prof_end(c);
    HIP_TRY(c, hipGetLastError());

    const size_t lds = (size_t)4 << hashSize;
    prof_begin(c, BSCGPU_K_LZP, (u64)n * 4, N);
    if (verify)      RC_TRY((launch_sweep<8, true >(c, nc, lds, c->dT, N, hashSize, minLen, prev0, next0, flags, dirty, staging, res)));
    else if (W == 8) RC_TRY((launch_sweep<8, false>(c, nc, lds, c->dT, N, hashSize, minLen, prev0, next0, flags, dirty, staging, res)));
    else             RC_TRY((launch_sweep<4, false>(c, nc, lds, c->dT, N, hashSize, minLen, prev0, next0, flags, dirty, staging, res)));
    prof_end(c);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(c->hscal + DS_LZP, res, (size_t)nc * CR_WORDS * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, ctx_sync(c));
    prof_collect(c);

    int own[8];
    for (int b = 0; b < nc; ++b) {
        const u32* r = c->hscal + DS_LZP + b * CR_WORDS;
        own[b] = (int)r[CR_RES];
        if (own[b] >= 0 && own[b] > chunk_size(n, nc, b)) return ctx_fail(c, BSC_GPU_ERROR, "LZP stage: a chunk's size is out of range", hipSuccess);
        c->lzp_last[CNT_MATCHES] += r[CR_MATCHES]; c->lzp_last[CNT_DIRTY] += r[CR_DIRTY];
        c->lzp_last[CNT_ZONES] += r[CR_ZONES]; c->lzp_last[CNT_ESCAPES] += r[CR_ESCAPES];
    }
    Frame F;
    const int total = frame_from_own(n, features, own, &F);
    c->lzp_last[CNT_RAW_CHUNKS] = F.raw_chunks;
    if (total < 0) return total;
    unsigned char* tab = reinterpret_cast<unsigned char*>(c->hscal + DS_LZP_TABLE);     // pinned: it goes up behind this call's return
    const int tab_bytes = frame_table(F, tab);
    HIP_TRY(c, hipMemcpyAsync(dOut, tab, (size_t)tab_bytes, hipMemcpyHostToDevice, c->stream));
    for (int b = 0; b < nc; ++b) {
        const u8* src = (nc > 1 && F.res[b] == F.size[b] ? c->dT : staging) + F.start[b];
        if (F.res[b] > 0) HIP_TRY(c, hipMemcpyAsync(dOut + F.off[b], src, (size_t)F.res[b], hipMemcpyDeviceToDevice, c->stream));
    }
    if (final_sync) HIP_TRY(c, ctx_sync(c));
    return total;
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
    return r;
}
