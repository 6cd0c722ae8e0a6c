// unbwt.hip — inverse Burrows-Wheeler transform on MI355X (the reference's GPU hook: libcubwt_unbwt, libcubwt.cu:2953,
// reached from bsc_bwt_decode, bwt.cpp:233-281).
//
// Contract (bwt.cpp:283-334 via libsais_unbwt_aux): L[0..n) and the 1-based primary index `idx` as bsc_bwt_encode writes them;
// rows 0..n, row `idx` is the sentinel row; sym(row) = L[row] below idx, L[row-1] above; the text is read off backwards by
// row <- LF(row) from row 0 and the walk must close on row idx after n steps.
//
// The walk is one serial chain of n dependent random accesses — hopeless on one lane.  As the reference's GPU path does, it is
// cut into many independent pieces (this implementation is our own):
//   1. LF      the stable counting-sort position of every row's symbol = ONE keys-only pass of the radix engine with
//              destination positions (rs_scatter<EMIT_POS>): LF(row) = pos + 1; packed with the symbol into P[row] (8 B), so
//              a step is one random 8-byte load.
//   2. marks   S ~ n/128 rows are marked (one per stratum, hashed offset; row 0 and the sentinel row included); their P entry
//              is replaced by {MARK, segment id}, the original kept in the segment table.
//   3. survey  one lane per segment walks until it arrives at a marked row: length and successor segment.
//   4. order   the host follows the S successor links from segment 0 (row 0 = text end) and turns lengths into offsets
//              (a 4 MB table; 512 K dependent steps in L2 ~ 2 ms) — and checks that the links form ONE chain of n steps that
//              ends on the sentinel row: anything else is a corrupt block, reported, never walked blindly.
//   5. decode  the same walks again, every lane writing its bytes straight to their final place.
// Latency is hidden by the number of concurrent walks (S lanes, mean length 128), not by any single one being fast.
#include "dev_common.h"
#include <cstring>
#include <vector>

constexpr u64 UB_MARK = 1ull << 63;
constexpr u32 UB_END  = 0xffffffffu;            // successor of the segment that runs into the sentinel row (as a start: not walked)
constexpr u32 UB_CAP  = 0xfffffffeu;            // successor of a segment whose walk hit the step cap
// The step cap (bscgpu_ctx::ub_step_cap: UB_STEP_CAP, dev_common.h, unless BSC_UNBWT_STEP_CAP says otherwise): a walk longer than
// this is declined.  ub_walk_kernel takes it as an argument; with the default it is compiled in (ARG_CAP = false), because the
// compiler unrolls the decode walk four times only when it knows the bound (the argument form measured 2 % slower on a whole call).

struct UbSeg { u64 orig; u32 row; u32 pad; };   // original P entry of the marked row, and the row

__device__ __forceinline__ u32 ub_hash(u32 x)
{
    x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
    return x;
}

// keys for the LF pass: one u64 per non-sentinel row, in row order
__global__ __launch_bounds__(WG) void ub_keys_kernel(const u8* __restrict__ L, u32 n, u64* __restrict__ keys)
{
    const u32 i = blockIdx.x * WG + threadIdx.x;
    if (i < n) keys[i] = (u64)L[i];
}

// P[row] = LF(row) | sym(row) << 32; the sentinel row gets LF 0 and an END mark
__global__ __launch_bounds__(WG) void ub_pack_kernel(const u8* __restrict__ L, const u32* __restrict__ pos, u32 n, u32 idx, u64* __restrict__ P)
{
    const u32 row = blockIdx.x * WG + threadIdx.x;
    if (row > n) return;
    if (row == idx) { P[row] = UB_MARK | (u64)UB_END; return; }
    const u32 i = row < idx ? row : row - 1;
    P[row] = (u64)(pos[i] + 1u) | ((u64)L[i] << 32);
}

__device__ __forceinline__ u32 ub_seg_row(u32 s, u32 S, u32 rows)
{
    // stratum s of the rows 0..rows-1; segment 0 starts at row 0 (the walk's start)
    const u32 q = rows / S, r = rows % S;
    const u32 lo = s * q + (s < r ? s : r), len = q + (s < r ? 1u : 0u);
    return s == 0 ? 0u : lo + ub_hash(s * 2654435761u + rows) % len;
}

__global__ __launch_bounds__(WG) void ub_mark_kernel(u64* __restrict__ P, u32 S, u32 rows, UbSeg* __restrict__ seg)
{
    const u32 s = blockIdx.x * WG + threadIdx.x;
    if (s >= S) return;
    const u32 row = ub_seg_row(s, S, rows);
    const u64 p = P[row];
    seg[s].orig = p; seg[s].row = row; seg[s].pad = 0;
    if (!(p & UB_MARK)) P[row] = UB_MARK | (u64)s;                    // the sentinel row keeps its END mark
}

// one lane per segment: DECODE = false: length + successor; true: bytes to out[k], k descending from `start`
template <bool DECODE, bool ARG_CAP>
__global__ __launch_bounds__(WG) void ub_walk_kernel(const u64* __restrict__ P, const UbSeg* __restrict__ seg, u32 S,
                                                     u32* __restrict__ seg_len, u32* __restrict__ seg_next,
                                                     const u32* __restrict__ seg_start, u8* __restrict__ out, u32* __restrict__ bad,
                                                     u32 step_cap)
{
    const u32 s = blockIdx.x * WG + threadIdx.x;
    if (s >= S) return;
    u64 p = seg[s].orig;
    if (p & UB_MARK) {                                                // the segment placed on the sentinel row: empty
        if (!DECODE) { seg_len[s] = 0; seg_next[s] = UB_END; }
        return;
    }
    if (DECODE && seg_start[s] == UB_END) return;                     // a batched pass's block that failed its chain check
    long long k = DECODE ? (long long)seg_start[s] : 0;
    u32 len = 0, nxt = UB_END;
    const u32 cap = ARG_CAP ? step_cap : UB_STEP_CAP;
    for (;;) {
        if (DECODE) { if (k < 0) { atomicOr(bad, 1u); break; } out[k--] = (u8)(p >> 32); }
        ++len;
        const u64 q = P[(u32)p];
        if (q & UB_MARK) { nxt = (u32)q; break; }
        p = q;
        if (len >= cap) { atomicOr(bad, 2u); nxt = UB_CAP; break; }
    }
    if (!DECODE) { seg_len[s] = len; seg_next[s] = nxt; }
}

template <bool DECODE>
static void ub_launch_walk(bscgpu_ctx* c, const u64* P, const UbSeg* seg, u32 S, u32* seg_len, u32* seg_next, const u32* seg_start, u8* out)
{
    const dim3 grid((S + WG - 1) / WG), block(WG);
    if (c->ub_step_cap == UB_STEP_CAP)
        hipLaunchKernelGGL((ub_walk_kernel<DECODE, false>), grid, block, 0, c->stream, P, seg, S, seg_len, seg_next, seg_start, out, c->dscal + DS_UB_GUARD, UB_STEP_CAP);
    else
        hipLaunchKernelGGL((ub_walk_kernel<DECODE, true>), grid, block, 0, c->stream, P, seg, S, seg_len, seg_next, seg_start, out, c->dscal + DS_UB_GUARD, c->ub_step_cap);
}

// Host-pointer entry: L (n bytes) -> T (n bytes), both host memory; returns BSC_NO_ERROR, a libbsc error code,
// LIBBSC_DATA_CORRUPT (-6) when the rows do not form one cycle through the sentinel row, or LIBBSC_NOT_SUPPORTED (-4) when a
// piece of the cycle is longer than the walk kernel's step cap (T untouched: use the host walk).
extern "C" int bscgpu_unbwt(bscgpu_ctx* c, const uint8_t* L, uint8_t* T, int64_t n64, int64_t index)
{
    if (!c || !L || !T || n64 < 0 || index <= 0 || index > n64) return BSC_BAD_PARAMETER;
    if (n64 > c->max_n || n64 >= 0x7ffffff0ll) return BSC_GPU_NOT_ENOUGH_MEMORY;
    if (hipSetDevice(c->device) != hipSuccess) return BSC_GPU_ERROR;
    if (n64 == 0) return BSC_NO_ERROR;
    const u32 n = (u32)n64, idx = (u32)index, rows = n + 1;
    u8* dL = c->dT;                                 // input bytes
    u64* keys = c->kA; u64* P = c->kB;              // the pass's sorted keys land in kB and are overwritten by P afterwards
    u32* pos = c->vA;
    u32 S = rows / 128; if (S > (1u << 19)) S = 1u << 19; if (S < 1) S = 1;
    UbSeg* seg = reinterpret_cast<UbSeg*>(c->cpos[0]);             // 16 B x S <= 8 MB (cpos holds 4N bytes)
    u32* seg_len = c->csa[0]; u32* seg_next = c->csa[1]; u32* seg_start = c->cgrp[0];
    if ((size_t)S * 16 > (size_t)c->max_n * 4 + 4096 * 4) { S = (u32)(((size_t)c->max_n * 4) / 16); if (S < 1) S = 1; }

    HIP_TRY(c, hipMemcpyAsync(dL, L, n, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemsetAsync(c->dscal + DS_UB_GUARD, 0, 4, c->stream));
    prof_begin(c, BSCGPU_K_PACK, (u64)n * 9, n);
    hipLaunchKernelGGL(ub_keys_kernel, dim3((n + WG - 1) / WG), dim3(WG), 0, c->stream, dL, n, keys);
    prof_end(c);
    RadixPass low; low.shift = 0; low.bits = 8;
    int in_alt = 0;
    int rc = radix_sort_passes(c, keys, P, nullptr, nullptr, n, &low, 1, &in_alt, pos);
    if (rc < 0) return rc;
    prof_begin(c, BSCGPU_K_PACK, (u64)rows * 13, rows);
    hipLaunchKernelGGL(ub_pack_kernel, dim3((rows + WG - 1) / WG), dim3(WG), 0, c->stream, dL, pos, n, idx, P);
    hipLaunchKernelGGL(ub_mark_kernel, dim3((S + WG - 1) / WG), dim3(WG), 0, c->stream, P, S, rows, seg);
    prof_end(c);
    prof_begin(c, BSCGPU_K_GATHER, (u64)n * 8, n);
    ub_launch_walk<false>(c, P, seg, S, seg_len, seg_next, nullptr, nullptr);
    prof_end(c);
    HIP_TRY(c, hipGetLastError());
    std::vector<u32> hlen(S), hnext(S), hstart(S, 0u);
    HIP_TRY(c, hipMemcpyAsync(hlen.data(), seg_len, (size_t)S * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(hnext.data(), seg_next, (size_t)S * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(c->hscal + DS_UB_GUARD, c->dscal + DS_UB_GUARD, 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, ctx_sync(c));
    prof_collect(c);
    // A walk longer than the step cap is not proof of corruption — the marked rows are a fixed hash of the row number, and a valid
    // but adversarial block can put more than the cap between two of them —, so it is "not handled here" (the caller's host walk
    // decides, T is still untouched); LIBBSC_DATA_CORRUPT is reserved for the chain-closure checks below.
    if (c->hscal[DS_UB_GUARD] & 2u) return BSC_NOT_SUPPORTED;
    if (c->hscal[DS_UB_GUARD] != 0) return -6;
    // order of the segments: from segment 0 (row 0 = the text's end) along the successor links; every non-empty segment must
    // be met exactly once, the lengths must add up to n and the last link must be the sentinel row
    {
        u64 done = 0; u32 s = 0, met = 0;
        std::vector<u8> seen(S, 0);
        for (;;) {
            if (seen[s]) return -6;
            seen[s] = 1; ++met;
            if (done + hlen[s] > n) return -6;
            hstart[s] = (u32)(n - 1 - done);                           // first byte this segment writes (descending)
            done += hlen[s];
            const u32 nx = hnext[s];
            if (nx == UB_END) break;
            if (nx >= S) return -6;
            s = nx;
        }
        if (done != n) return -6;
        (void)met;
    }
    HIP_TRY(c, hipMemcpyAsync(seg_start, hstart.data(), (size_t)S * 4, hipMemcpyHostToDevice, c->stream));
    prof_begin(c, BSCGPU_K_GATHER, (u64)n * 9, n);
    ub_launch_walk<true>(c, P, seg, S, nullptr, nullptr, seg_start, c->dL);
    prof_end(c);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(T, c->dL, n, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(c->hscal + DS_UB_GUARD, c->dscal + DS_UB_GUARD, 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, ctx_sync(c));
    prof_collect(c);
    return c->hscal[DS_UB_GUARD] != 0 ? -6 : BSC_NO_ERROR;
}

// ---- batched passes (bscgpu_unbwt_batch_device; the decompress batch, batch_decode.cpp) ------------------------------
// A pass holds `count` blocks with their L back to back (block b at off[b], n_b bytes).  Block b owns the rows base_b .. base_b + n_b,
// base_b = off[b] + b: contiguous, in block order.  LF without a wider sort: the one 8-bit keys-only pass over the whole pass's symbols
// gives every record its global stable position pos_g, and records of one symbol are in block order there.  With H[b][c] the block x
// symbol histogram, G[c] the global count of smaller symbols, P_b[c] = sum of H[b'][c] over b' < b and C_b[c] = sum of H[b][c'] over
// c' < c, the rank inside the block is r = pos_g - G[c] - P_b[c] and LF = base_b + 1 + C_b[c] + r = pos_g + D[b][c]: one table, built
// from H by two scans.  Walks then never leave their block (every LF of block b lands in its rows), and ub_walk_kernel runs unchanged on
// global rows.  Segments are global too: block b owns soff[b] .. soff[b+1] - 1, the first starting at its row 0 (its text's end).
constexpr u32 UB_TILE = WG * 16;

__device__ __forceinline__ u32 ub_find(const u32* __restrict__ tab, u32 count, u32 i)
{
    u32 lo = 0, hi = count;                     // the last b with tab[b] <= i (entries that share a value: the last one)
    while (hi - lo > 1) { const u32 mid = (lo + hi) >> 1; if (tab[mid] <= i) lo = mid; else hi = mid; }
    return lo;
}

// keys of the LF pass and H (zeroed before): a tile's bytes of the block its first byte lies in are counted in LDS, those of any later
// block (a tile that crosses a block end) straight in H
__global__ __launch_bounds__(WG) void ub_keys_batch_kernel(const u8* __restrict__ L, u32 n, const u32* __restrict__ off, u32 count,
                                                          u64* __restrict__ keys, u32* __restrict__ H)
{
    __shared__ u32 h[256];
    h[threadIdx.x] = 0;
    __syncthreads();
    const u32 t0 = blockIdx.x * UB_TILE;
    const u32 b0 = ub_find(off, count, t0), e0 = off[b0 + 1];
    for (u32 j = 0; j < 16; ++j) {
        const u32 i = t0 + j * WG + threadIdx.x;
        if (i >= n) break;
        const u32 c = L[i];
        keys[i] = (u64)c;
        if (i < e0) atomicAdd(&h[c], 1u);
        else atomicAdd(&H[(size_t)ub_find(off, count, i) * 256 + c], 1u);
    }
    __syncthreads();
    if (h[threadIdx.x]) atomicAdd(&H[(size_t)b0 * 256 + threadIdx.x], h[threadIdx.x]);
}

// PD[b][c] = P_b[c] (one workgroup per symbol c), tot[c] = the symbol's count in the pass
__global__ __launch_bounds__(WG) void ub_scan_blocks_kernel(const u32* __restrict__ H, u32 count, u32* __restrict__ PD, u32* __restrict__ tot)
{
    __shared__ u32 lds[8];
    const u32 c = blockIdx.x;
    u32 carry = 0;
    for (u32 b0 = 0; b0 < count; b0 += WG) {
        const u32 b = b0 + threadIdx.x;
        const u32 v = b < count ? H[(size_t)b * 256 + c] : 0u;
        u32 sum;
        const u32 ex = block_excl_sum(v, lds, &sum);
        if (b < count) PD[(size_t)b * 256 + c] = carry + ex;
        carry += sum;
    }
    if (threadIdx.x == 0) tot[c] = carry;
}

// PD[b][c] <- D[b][c] = base_b + 1 + C_b[c] - G[c] - P_b[c] (one workgroup per block, one lane per symbol; modulo 2^32)
__global__ __launch_bounds__(WG) void ub_lf_base_kernel(const u32* __restrict__ H, const u32* __restrict__ tot, const u32* __restrict__ off,
                                                       u32* __restrict__ PD)
{
    __shared__ u32 lds[8];
    const u32 b = blockIdx.x, c = threadIdx.x;
    u32 sum;
    const u32 G = block_excl_sum(tot[c], lds, &sum);
    const size_t k = (size_t)b * 256 + c;
    const u32 C = block_excl_sum(H[k], lds, &sum);
    PD[k] = off[b] + b + 1u + C - G - PD[k];
}

// P[row] for every row of the pass; idx[b] = 0: the block is not decoded (every row an END mark, no segment)
__global__ __launch_bounds__(WG) void ub_pack_batch_kernel(const u8* __restrict__ L, const u32* __restrict__ pos, const u32* __restrict__ off,
                                                          const u32* __restrict__ idx, const u32* __restrict__ D, u32 count, u32 rows,
                                                          u64* __restrict__ P)
{
    const u32 row = blockIdx.x * WG + threadIdx.x;
    if (row >= rows) return;
    u32 lo = 0, hi = count;                     // the block: the last b with base_b <= row (bases grow strictly: every block has a row)
    while (hi - lo > 1) { const u32 mid = (lo + hi) >> 1; if (off[mid] + mid <= row) lo = mid; else hi = mid; }
    const u32 r = row - (off[lo] + lo), id = idx[lo];
    if (id == 0 || r == id) { P[row] = UB_MARK | (u64)UB_END; return; }
    const u32 i = off[lo] + (r < id ? r : r - 1);
    const u32 c = L[i];
    P[row] = (u64)(pos[i] + D[(size_t)lo * 256 + c]) | ((u64)c << 32);
}

__global__ __launch_bounds__(WG) void ub_mark_batch_kernel(u64* __restrict__ P, const u32* __restrict__ off, const u32* __restrict__ soff,
                                                          u32 count, u32 S, UbSeg* __restrict__ seg)
{
    const u32 s = blockIdx.x * WG + threadIdx.x;
    if (s >= S) return;
    const u32 b = ub_find(soff, count, s);     // (blocks without segments share their successor's offset)
    const u32 rows = off[b + 1] - off[b] + 1u;
    const u32 row = off[b] + b + ub_seg_row(s - soff[b], soff[b + 1] - soff[b], rows);
    const u64 p = P[row];
    seg[s].orig = p; seg[s].row = row; seg[s].pad = 0;
    if (!(p & UB_MARK)) P[row] = UB_MARK | (u64)s;
}

int unbwt_batch_max_blocks(int64_t cap)
{
    const int64_t m = cap / 256 + 16;           // H: 256 counters per block in vB (4N bytes, N >= max_n + 4096)
    return m < BATCH_MAX_BLOCKS ? (int)m : BATCH_MAX_BLOCKS;
}

int unbwt_batch_pass(bscgpu_ctx* c, const u8* dL, u8* out, const int* sizes, const int* idx, int count, const u32* dst, int* res,
                     u32* adler, u8* t_host)
{
    if (count <= 0 || count > unbwt_batch_max_blocks(c->max_n)) return BSC_BAD_PARAMETER;
    const int trc = batch_tab_ensure(c);
    if (trc < 0) return trc;
    // batch_tab words: offsets [count + 1], primary indexes [count], segment offsets [count + 1], (dst, dst + n) pairs [2 count],
    // checksums [count], symbol totals [256]
    constexpr size_t A_IDX = BATCH_MAX_BLOCKS + 1, A_SOFF = 2 * BATCH_MAX_BLOCKS + 1, A_PAIR = 3 * BATCH_MAX_BLOCKS + 2,
                     A_ADLER = 5 * BATCH_MAX_BLOCKS + 2, A_TOT = 6 * BATCH_MAX_BLOCKS + 2;
    std::vector<u32> tab(A_ADLER, 0u);
    u64 total = 0, span = 0;
    for (int b = 0; b < count; ++b) {
        if (sizes[b] < 0 || idx[b] < 0 || idx[b] > sizes[b]) return BSC_BAD_PARAMETER;
        tab[b] = (u32)total; total += (u64)sizes[b];
        tab[A_IDX + b] = (u32)idx[b];
        const u64 end = (u64)dst[b] + (u64)sizes[b];
        if (end > 0xffffffffull) return BSC_BAD_PARAMETER;
        tab[A_PAIR + 2 * b] = dst[b]; tab[A_PAIR + 2 * b + 1] = (u32)end;
        if (end > span) span = end;
        res[b] = BSC_NO_ERROR;
    }
    tab[count] = (u32)total;
    if (total > (u64)c->max_n) return BSC_BAD_PARAMETER;
    const u32 n = (u32)total, rows = n + (u32)count;
    // segments: at least one per decoded block, ~rows_b / stride each, under the single-block path's global cap
    u64 smax = ((u64)c->max_n * 4 + 4096 * 4) / 16;
    if (smax > (1u << 19)) smax = 1u << 19;
    u32 stride = 128;
    u64 S = 0;
    for (;;) {
        S = 0;
        for (int b = 0; b < count; ++b) if (idx[b]) { const u32 k = (u32)(sizes[b] + 1) / stride; S += k ? k : 1; }
        if (S <= smax || stride >= (1u << 30)) break;
        stride *= 2;
    }
    {
        u32 s = 0;
        for (int b = 0; b < count; ++b) {
            tab[A_SOFF + b] = s;
            if (idx[b]) { const u32 k = (u32)(sizes[b] + 1) / stride; s += k ? k : 1; }
        }
        tab[A_SOFF + count] = s;
    }
    if (S == 0) return BSC_NO_ERROR;
    if (hipSetDevice(c->device) != hipSuccess) return BSC_GPU_ERROR;
    u32* const dtab = c->batch_tab;
    const u32* doff = dtab; const u32* didx = dtab + A_IDX; const u32* dsoff = dtab + A_SOFF;
    u64* keys = c->kA; u64* P = c->kB;          // as bscgpu_unbwt: the sorted keys land in kB and are overwritten by P
    u32* pos = c->vA; u32* H = c->vB; u32* PD = c->SA;
    UbSeg* seg = reinterpret_cast<UbSeg*>(c->cpos[0]);
    u32* seg_len = c->csa[0]; u32* seg_next = c->csa[1]; u32* seg_start = c->cgrp[0];
    const u32 nseg = (u32)S;

    HIP_TRY(c, hipMemcpyAsync(dtab, tab.data(), tab.size() * 4, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemsetAsync(H, 0, (size_t)count * 256 * 4, c->stream));
    HIP_TRY(c, hipMemsetAsync(c->dscal + DS_UB_GUARD, 0, 4, c->stream));
    prof_begin(c, BSCGPU_K_PACK, (u64)n * 9, n);
    if (n > 0) hipLaunchKernelGGL(ub_keys_batch_kernel, dim3((n + UB_TILE - 1) / UB_TILE), dim3(WG), 0, c->stream, dL, n, doff, (u32)count, keys, H);
    prof_end(c);
    RadixPass low; low.shift = 0; low.bits = 8;
    int in_alt = 0;
    int rc = radix_sort_passes(c, keys, P, nullptr, nullptr, n, &low, 1, &in_alt, pos);
    if (rc < 0) return rc;
    prof_begin(c, BSCGPU_K_PACK, (u64)rows * 13, rows);
    hipLaunchKernelGGL(ub_scan_blocks_kernel, dim3(256), dim3(WG), 0, c->stream, H, (u32)count, PD, dtab + A_TOT);
    hipLaunchKernelGGL(ub_lf_base_kernel, dim3(count), dim3(WG), 0, c->stream, H, dtab + A_TOT, doff, PD);
    hipLaunchKernelGGL(ub_pack_batch_kernel, dim3((rows + WG - 1) / WG), dim3(WG), 0, c->stream, dL, pos, doff, didx, PD, (u32)count, rows, P);
    hipLaunchKernelGGL(ub_mark_batch_kernel, dim3((nseg + WG - 1) / WG), dim3(WG), 0, c->stream, P, doff, dsoff, (u32)count, nseg, seg);
    prof_end(c);
    prof_begin(c, BSCGPU_K_GATHER, (u64)n * 8, n);
    ub_launch_walk<false>(c, P, seg, nseg, seg_len, seg_next, nullptr, nullptr);
    prof_end(c);
    HIP_TRY(c, hipGetLastError());
    std::vector<u32> hlen(nseg), hnext(nseg), hstart(nseg, 0u);
    HIP_TRY(c, hipMemcpyAsync(hlen.data(), seg_len, (size_t)nseg * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(hnext.data(), seg_next, (size_t)nseg * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, ctx_sync(c));
    prof_collect(c);
    // every block's chain, from its first segment: each segment met once and the block's own, the lengths adding up to n_b, the last
    // link on the block's sentinel row.  A block whose pieces hit the step cap is "not handled here" (as bscgpu_unbwt says it).
    std::vector<u8> seen(nseg, 0);
    for (int b = 0; b < count; ++b) {
        if (!idx[b]) continue;
        const u32 s0 = tab[A_SOFF + b], s1 = tab[A_SOFF + b + 1], nb = (u32)sizes[b];
        int r = BSC_NO_ERROR;
        for (u32 s = s0; s < s1; ++s) if (hnext[s] == UB_CAP) r = BSC_NOT_SUPPORTED;
        if (r == BSC_NO_ERROR) {
            u64 done = 0;
            for (u32 s = s0;;) {
                if (seen[s] || done + hlen[s] > nb) { r = BSC_DATA_CORRUPT; break; }
                seen[s] = 1;
                hstart[s] = (u32)(dst[b] + nb - 1 - done);             // first byte this segment writes (descending)
                done += hlen[s];
                const u32 nx = hnext[s];
                if (nx == UB_END) { if (done != nb) r = BSC_DATA_CORRUPT; break; }
                if (nx < s0 || nx >= s1) { r = BSC_DATA_CORRUPT; break; }
                s = nx;
            }
        }
        if (r != BSC_NO_ERROR) { res[b] = r; for (u32 s = s0; s < s1; ++s) hstart[s] = UB_END; }     // its segments are not walked
    }
    HIP_TRY(c, hipMemcpyAsync(seg_start, hstart.data(), (size_t)nseg * 4, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemsetAsync(c->dscal + DS_UB_GUARD, 0, 4, c->stream));
    prof_begin(c, BSCGPU_K_GATHER, (u64)n * 9, n);
    ub_launch_walk<true>(c, P, seg, nseg, nullptr, nullptr, seg_start, out);
    prof_end(c);
    if (adler) {
        launch_adler_batch(c, out, dtab + A_PAIR, (u32)count, dtab + A_ADLER, 2);
        HIP_TRY(c, hipMemcpyAsync(adler, dtab + A_ADLER, (size_t)count * 4, hipMemcpyDeviceToHost, c->stream));
    }
    HIP_TRY(c, hipGetLastError());
    if (t_host && span > 0) HIP_TRY(c, hipMemcpyAsync(t_host, out, (size_t)span, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(c->hscal + DS_UB_GUARD, c->dscal + DS_UB_GUARD, 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, ctx_sync(c));
    prof_collect(c);
    if (c->hscal[DS_UB_GUARD] != 0)                       // a guard of the decode walk fired (the chain checks rule it out): trust no block of the pass
        for (int b = 0; b < count; ++b) if (idx[b] && res[b] == BSC_NO_ERROR) res[b] = BSC_DATA_CORRUPT;
    return BSC_NO_ERROR;
}

// L of many blocks back to back in HBM -> T in the same layout (dT may be dL).  Passes: consecutive blocks, at most max_n bytes and
// unbwt_batch_max_blocks(max_n) blocks each; results[b] = what bscgpu_unbwt returns for block b alone.
extern "C" int bscgpu_unbwt_batch_device(bscgpu_ctx* c, const void* dL, void* dT, const int* sizes, int count, const int* primary, int* results)
{
    if (!c || count < 0 || (count > 0 && (!sizes || !primary || !results))) return BSC_BAD_PARAMETER;
    int64_t total = 0;
    for (int b = 0; b < count; ++b) { if (sizes[b] < 0) return BSC_BAD_PARAMETER; total += sizes[b]; }
    if (total > 0 && (!dL || !dT)) return BSC_BAD_PARAMETER;
    if (count == 0) return BSC_NO_ERROR;
    if (hipSetDevice(c->device) != hipSuccess) return BSC_GPU_ERROR;
    const u8* L = (const u8*)dL; u8* T = (u8*)dT;
    const int lim = unbwt_batch_max_blocks(c->max_n);
    std::vector<int> idx, res;
    std::vector<u32> dst;
    int64_t o = 0;
    for (int b = 0; b < count;) {
        if (sizes[b] > c->max_n) { results[b] = primary[b] <= 0 || primary[b] > sizes[b] ? BSC_BAD_PARAMETER : BSC_GPU_NOT_ENOUGH_MEMORY; o += sizes[b]; ++b; continue; }
        int e = b; int64_t bytes = 0;
        while (e < count && e - b < lim && sizes[e] <= c->max_n && bytes + sizes[e] <= c->max_n) bytes += sizes[e++];
        idx.assign((size_t)(e - b), 0); res.assign((size_t)(e - b), 0); dst.assign((size_t)(e - b), 0u);
        bool any = false;
        for (int q = b, p = 0; q < e; ++q) {
            const int i = q - b, n = sizes[q];
            dst[i] = (u32)p; p += n;
            if (primary[q] <= 0 || primary[q] > n) { results[q] = BSC_BAD_PARAMETER; continue; }
            results[q] = BSC_NO_ERROR;
            if (n == 1) {                           // T = L
                if (T != L) HIP_TRY(c, hipMemcpyAsync(T + o + dst[i], L + o + dst[i], 1, hipMemcpyDeviceToDevice, c->stream));
                continue;
            }
            idx[i] = primary[q]; any = true;
        }
        if (any) {
            const int rc = unbwt_batch_pass(c, L + o, T + o, sizes + b, idx.data(), e - b, dst.data(), res.data(), nullptr, nullptr);
            if (rc < 0) return rc;
            for (int q = b; q < e; ++q) if (idx[q - b]) results[q] = res[q - b];
        } else HIP_TRY(c, ctx_sync(c));
        o += bytes; b = e;
    }
    return BSC_NO_ERROR;
}
