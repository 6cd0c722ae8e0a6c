// st.hip — Sort Transform of order k = 3..8 on MI355X, plus the device Adler-32.
//
// Result contract (bsc_st_encode, st.cpp:990; verified against the compiled reference):
// stable-sort the positions i in [0,n) by the k cyclic bytes T[i..i+k-1]; output byte T[i-1] (cyclic) in
// that order; return the 0-based sorted rank of position 0.  The reference's GPU path (st.cu:100-217)
// builds the same keys and calls cub::DeviceRadixSort; here the keys go through our own LSD engine:
//   k <= 7 : key = T[i-1] | T[i] .. T[i+6]  (output byte rides in the top byte, never sorted on),
//            keys-only passes over bits [(7-k)*8, 56)  -> k passes of 16 B/record;
//   k == 8 : key = T[i..i+7], value = T[i-1] | (i == 0) << 8, 8 passes of 24 B/record.
// Many small blocks go through one sort per pass with the block id as the top digits: st_batch_device, further down.
#include "dev_common.h"
#include <cstring>
#include <vector>

// cyclic padding around the private text copy: dT[-1] = T[n-1], dT[n+j] = T[j mod n] (j < 32)
__global__ void st_pad_kernel(u8* __restrict__ dT, u32 n)
{
    const u32 j = threadIdx.x;
    if (j < 32) dT[n + j] = dT[j % n];
    if (j == 32) dT[-1] = dT[n - 1];
}

template <bool K8>
__global__ __launch_bounds__(WG) void st_pack_kernel(const u8* __restrict__ T, u32 n, u64* __restrict__ keys,
                                                     u32* __restrict__ vals, u64* __restrict__ key0)
{
    const u32 i0 = 4u * (blockIdx.x * WG + threadIdx.x);
    if (i0 >= n) return;
    const u32* T32 = reinterpret_cast<const u32*>(T + i0) - 1;         // bytes i0-4 .. i0+11
    const u64 w0 = ((u64)__builtin_bswap32(T32[0]) << 32) | __builtin_bswap32(T32[1]);
    const u64 w1 = ((u64)__builtin_bswap32(T32[2]) << 32) | __builtin_bswap32(T32[3]);
#pragma unroll
    for (u32 j = 0; j < 4; ++j) {
        const u32 i = i0 + j;
        if (i < n) {
            if (!K8) {
                const u32 s = 8 * (3 + j);                               // window starts at byte i-1
                const u64 key = (w0 << s) | (w1 >> (64 - s));
                keys[i] = key;
                if (i == 0) *key0 = key;
            } else {
                const u32 s = 8 * (4 + j);                               // window starts at byte i
                const u64 key = (s == 32) ? ((w0 << 32) | (w1 >> 32)) : ((w0 << s) | (w1 >> (64 - s)));
                keys[i] = key;
                const u32 prev = (u32)(w0 >> (8 * (4 - j))) & 0xffu;     // byte i-1
                vals[i] = prev | ((i == 0) ? 0x100u : 0u);
            }
        }
    }
}

template <bool K8>
__global__ __launch_bounds__(WG) void st_post_kernel(const u64* __restrict__ keys, const u32* __restrict__ vals,
                                                     u32 n, const u64* __restrict__ key0, u8* __restrict__ out,
                                                     u32* __restrict__ index)
{
    const u32 j0 = 4u * (blockIdx.x * WG + threadIdx.x);
    if (j0 >= n) return;
    const u64 k0 = K8 ? 0 : *key0;
    u32 word = 0;
#pragma unroll
    for (u32 q = 0; q < 4; ++q) {
        const u32 j = j0 + q;
        if (j < n) {
            if (!K8) {
                const u64 key = keys[j];
                word |= (u32)(key >> 56) << (8 * q);
                if (key == k0) atomicMin(index, j);
            } else {
                const u32 v = vals[j];
                word |= (v & 0xffu) << (8 * q);
                if (v & 0x100u) atomicMin(index, j);
            }
        }
    }
    if (j0 + 4 <= n) *reinterpret_cast<u32*>(out + j0) = word;
    else for (u32 q = 0; j0 + q < n; ++q) out[j0 + q] = (u8)(word >> (8 * q));
}

static int st_device_once(bscgpu_ctx* c, const u8* dT_user, u8* dOut_user, int n_, int k, int* index_out, bool reuse_text);

// as bwt_device: a single-read pass that gave up fails the sort, and the transform is redone once with the three-kernel passes from
// the private copy of the text (the caller's buffer may already hold the failed attempt's bytes when it is also the output)
int st_device(bscgpu_ctx* c, const u8* dT_user, u8* dOut_user, int n_, int k, int* index_out)
{
    return with_onesweep_retry(c, [&](bool reuse_text) { return st_device_once(c, dT_user, dOut_user, n_, k, index_out, reuse_text); });
}

static int st_device_once(bscgpu_ctx* c, const u8* dT_user, u8* dOut_user, int n_, int k, int* index_out, bool reuse_text)
{
    if (n_ < 0 || n_ > c->max_n) return BSC_BAD_PARAMETER;
    if (k < 3 || k > 8) return BSC_BAD_PARAMETER;
    const u32 n = (u32)n_;
    if (n <= 1) {                                   // st.cpp:994
        if (n == 1 && dOut_user != dT_user) HIP_TRY(c, hipMemcpyAsync(dOut_user, dT_user, 1, hipMemcpyDeviceToDevice, c->stream));
        HIP_TRY(c, ctx_sync(c));
        *index_out = 0;
        return BSC_NO_ERROR;
    }
    if (!reuse_text) HIP_TRY(c, hipMemcpyAsync(c->dT, dT_user, n, hipMemcpyDeviceToDevice, c->stream));
    hipLaunchKernelGGL(st_pad_kernel, dim3(1), dim3(64), 0, c->stream, c->dT, n);
    HIP_TRY(c, hipMemsetAsync(c->dscal + DS_ST_INDEX, 0xff, 4, c->stream));

    const dim3 grid((n + 4 * WG - 1) / (4 * WG));
    int in_alt = 0, rc;
    RadixPass passes[8];
    if (k < 8) {
        prof_begin(c, BSCGPU_K_PACK, (u64)n * 9, n);
        hipLaunchKernelGGL(st_pack_kernel<false>, grid, dim3(WG), 0, c->stream, c->dT, n, c->kA, (u32*)nullptr, c->dscal64 + DS64_ST_KEY0);
        prof_end(c);
        bwt_cut_passes(passes, (7 - k) * 8, 8 * k);
        rc = radix_sort_passes(c, c->kA, c->kB, nullptr, nullptr, n, passes, k, &in_alt);
        if (rc < 0) return rc;
        prof_begin(c, BSCGPU_K_EMIT, (u64)n * 9, n);
        hipLaunchKernelGGL(st_post_kernel<false>, grid, dim3(WG), 0, c->stream, in_alt ? c->kB : c->kA, (const u32*)nullptr,
                           n, c->dscal64 + DS64_ST_KEY0, dOut_user, c->dscal + DS_ST_INDEX);
        prof_end(c);
    } else {
        prof_begin(c, BSCGPU_K_PACK, (u64)n * 13, n);
        hipLaunchKernelGGL(st_pack_kernel<true>, grid, dim3(WG), 0, c->stream, c->dT, n, c->kA, c->vA, c->dscal64 + DS64_ST_KEY0);
        prof_end(c);
        bwt_cut_passes(passes, 0, 64);
        rc = radix_sort_passes(c, c->kA, c->kB, c->vA, c->vB, n, passes, 8, &in_alt);
        if (rc < 0) return rc;
        prof_begin(c, BSCGPU_K_EMIT, (u64)n * 5, n);
        hipLaunchKernelGGL(st_post_kernel<true>, grid, dim3(WG), 0, c->stream, in_alt ? c->kB : c->kA, in_alt ? c->vB : c->vA,
                           n, c->dscal64 + DS64_ST_KEY0, dOut_user, c->dscal + DS_ST_INDEX);
        prof_end(c);
    }
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(c->hscal, c->dscal, DS_ST_WORDS * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, ctx_sync(c));
    prof_collect(c);
    *index_out = (int)c->hscal[DS_ST_INDEX];
    return radix_onesweep_check(c);
}

// ---------------------------------------------------------------------------------------------
// Batched pass: the records of many blocks, laid out back to back, in one sort (st_batch_device).  A record's context is
// BLOCK-CYCLIC (T_b[(i + j) mod n_b]: the blocks touch, so there is no padding to read) and the block id is the sort's most
// significant digits: the engine is LSD and stable, so the block digits simply run last, and slot j of the sorted pass belongs to the
// block that owns text position j.  Position 0 of a block is flagged, which gives the block's index without a comparison.
//   k <= 5 : keys only, key = out byte [63:56] | block [55:44] | T[i .. i+4] [43:4] | (i == 0) [0];
//            k context passes from bit 4 + 8 (5 - k), then the block digits from bit 44 (8 bits, then the rest): 16 B/record per pass;
//   k >= 6 : key = T[i .. i+7], value = out byte | (i == 0) << 8 | block << 9; k context passes from bit 8 (8 - k), the key is
//            rewritten as the block id (st_batch_rekey_kernel: 12 B/record), then the block digits: 24 B/record per pass.
// A block with rate < 0 is not transformed: its records carry their own byte and an all-zero context, so the stable sort returns them
// in text order (out = T, index 0).
constexpr u32 STB_BLOCK_SHIFT = 44, STB_CTX_SHIFT = 4, STB_VAL_BLOCK_SHIFT = 9, STB_BLOCK_MASK = BATCH_MAX_BLOCKS - 1;

template <bool KV>
__device__ __forceinline__ void st_batch_put(u64* __restrict__ keys, u32* __restrict__ vals, u32 g, u32 b, bool first, u32 prev, u64 ctx)
{
    if (KV) {
        keys[g] = ctx;
        vals[g] = prev | (first ? 0x100u : 0u) | (b << STB_VAL_BLOCK_SHIFT);
    } else {
        keys[g] = ((u64)prev << 56) | ((u64)b << STB_BLOCK_SHIFT) | ((ctx >> 24) << STB_CTX_SHIFT) | (first ? 1ull : 0ull);
    }
}

// Four consecutive positions of the pass per thread.  Interior of a block (the thread's bytes g0 - 1 .. g0 + 10 all inside it): the
// single-block kernel's four aligned 4-byte loads.  Within eleven bytes of a block's ends, blocks shorter than that included: byte
// reads that wrap at the block's ends.  The block of a workgroup's first and last position is found once per workgroup; a thread
// searches the table only where its workgroup spans several blocks, and then only between those two.
template <bool KV>
__global__ __launch_bounds__(WG) void st_batch_pack_kernel(const u8* __restrict__ T, u32 N, const u32* __restrict__ off,
                                                           const int* __restrict__ rate, u32 count, u64* __restrict__ keys,
                                                           u32* __restrict__ vals)
{
    __shared__ u32 span[2];
    const u32 p0 = 4u * WG * blockIdx.x;
    if (threadIdx.x < 2) {
        u32 p = p0 + threadIdx.x * (4u * WG - 1u);
        if (p >= N) p = N - 1u;
        span[threadIdx.x] = batch_block_of(off, count, p);
    }
    __syncthreads();
    const u32 g0 = p0 + 4u * threadIdx.x;
    if (g0 >= N) return;
    u32 b = span[0];
    if (span[1] != b) b = batch_block_of(off, b, span[1] + 1u, g0);
    u32 o0 = off[b], end = off[b + 1];
    if (g0 > o0 && g0 + 11u <= end && rate[b] >= 0) {
        const u32* T32 = reinterpret_cast<const u32*>(T + g0) - 1;         // bytes g0-4 .. g0+11
        const u64 w0 = ((u64)__builtin_bswap32(T32[0]) << 32) | __builtin_bswap32(T32[1]);
        const u64 w1 = ((u64)__builtin_bswap32(T32[2]) << 32) | __builtin_bswap32(T32[3]);
#pragma unroll
        for (u32 j = 0; j < 4; ++j) {
            const u32 s = 8 * (4 + j);                                   // window starts at byte g0 + j
            st_batch_put<KV>(keys, vals, g0 + j, b, false, (u32)(w0 >> (8 * (4 - j))) & 0xffu, (w0 << s) | (w1 >> (64 - s)));
        }
        return;
    }
    for (u32 j = 0; j < 4; ++j) {
        const u32 g = g0 + j;
        if (g >= N) break;
        while (g >= end) { ++b; o0 = off[b]; end = off[b + 1]; }         // (g < N = off[count]: ends; empty blocks are stepped over)
        const u32 n = end - o0, i = g - o0;
        u32 prev = T[g];
        u64 ctx = 0;
        if (rate[b] >= 0) {
            prev = T[i ? g - 1u : end - 1u];
            u32 p = i;
            for (u32 t = 0; t < 8; ++t) { ctx = (ctx << 8) | T[o0 + p]; if (++p == n) p = 0; }
        }
        st_batch_put<KV>(keys, vals, g, b, i == 0, prev, ctx);
    }
}

__global__ __launch_bounds__(WG) void st_batch_rekey_kernel(const u32* __restrict__ vals, u64* __restrict__ keys, u32 N)
{
    const u32 j = blockIdx.x * WG + threadIdx.x;
    if (j < N) keys[j] = vals[j] >> STB_VAL_BLOCK_SHIFT;
}

// Slot j of the sorted pass is output byte j.  `out` is the caller's pointer rounded down to 4 bytes and `lead` what was cut off,
// so that the 4-byte stores are aligned wherever the pass starts in the caller's buffer.  (The block id is masked to the table's
// size: the records of a sort that gave up a wait are not to be trusted, and the retry writes everything again.)
template <bool KV>
__global__ __launch_bounds__(WG) void st_batch_post_kernel(const u64* __restrict__ keys, const u32* __restrict__ vals, u32 N, u32 lead,
                                                           const u32* __restrict__ off, u8* __restrict__ out, u32* __restrict__ index)
{
    const u32 q0 = 4u * (blockIdx.x * WG + threadIdx.x);
    if (q0 >= N + lead) return;
    u32 word = 0, have = 0;
#pragma unroll
    for (u32 q = 0; q < 4; ++q) {
        const u32 j = q0 + q - lead;
        if (q0 + q >= lead && j < N) {
            u32 byte, b; bool first;
            if (KV) { const u32 v = vals[j]; byte = v & 0xffu; first = (v & 0x100u) != 0; b = (v >> STB_VAL_BLOCK_SHIFT) & STB_BLOCK_MASK; }
            else { const u64 key = keys[j]; byte = (u32)(key >> 56); first = (key & 1ull) != 0; b = (u32)(key >> STB_BLOCK_SHIFT) & STB_BLOCK_MASK; }
            word |= byte << (8 * q);
            have |= 1u << q;
            if (first) index[b] = j - off[b];
        }
    }
    if (have == 0xfu) *reinterpret_cast<u32*>(out + q0) = word;
    else for (u32 q = 0; q < 4; ++q) if (have & (1u << q)) out[q0 + q] = (u8)(word >> (8 * q));
}

static int st_batch_once(bscgpu_ctx* c, const u8* dT_user, u8* dOut_user, u32 N, u32 count, int k, const u32* doff, const int* drate,
                         u32* dindex, int* index_out, bool reuse_text)
{
    if (!reuse_text) HIP_TRY(c, hipMemcpyAsync(c->dT, dT_user, N, hipMemcpyDeviceToDevice, c->stream));
    HIP_TRY(c, hipMemsetAsync(dindex, 0, (size_t)count * 4, c->stream));
    int bb = 0;
    while ((1u << bb) < count) ++bb;                                       // bits of the block id
    const bool kv = k >= 6;
    const dim3 grid((N + 4 * WG - 1) / (4 * WG));
    int in_alt = 0, rc, np = 0;
    RadixPass passes[8];
    u64 *kcur = c->kA, *kalt = c->kB;
    u32 *vcur = kv ? c->vA : nullptr, *valt = kv ? c->vB : nullptr;
    prof_begin(c, BSCGPU_K_PACK, (u64)N * (kv ? 13 : 9), N);
    if (kv) hipLaunchKernelGGL(st_batch_pack_kernel<true>, grid, dim3(WG), 0, c->stream, c->dT, N, doff, drate, count, kcur, vcur);
    else hipLaunchKernelGGL(st_batch_pack_kernel<false>, grid, dim3(WG), 0, c->stream, c->dT, N, doff, drate, count, kcur, vcur);
    prof_end(c);
    np = bwt_cut_passes(passes, kv ? 8 * (8 - k) : (int)STB_CTX_SHIFT + 8 * (5 - k), 8 * k);
    const int block_shift = kv ? 0 : (int)STB_BLOCK_SHIFT;
    if (kv && bb > 0) {
        rc = radix_sort_passes(c, kcur, kalt, vcur, valt, N, passes, np, &in_alt);
        if (rc < 0) return rc;
        if (in_alt) { u64* tk = kcur; kcur = kalt; kalt = tk; u32* tv = vcur; vcur = valt; valt = tv; }
        prof_begin(c, BSCGPU_K_MISC, (u64)N * 12, N);
        hipLaunchKernelGGL(st_batch_rekey_kernel, dim3((N + WG - 1) / WG), dim3(WG), 0, c->stream, vcur, kcur, N);
        prof_end(c);
        np = 0;
    }
    np += bwt_cut_passes(passes + np, block_shift, bb);
    rc = radix_sort_passes(c, kcur, kalt, vcur, valt, N, passes, np, &in_alt);
    if (rc < 0) return rc;
    if (in_alt) { u64* tk = kcur; kcur = kalt; kalt = tk; u32* tv = vcur; vcur = valt; valt = tv; }
    const u32 lead = (u32)((uintptr_t)dOut_user & 3u);
    const dim3 pgrid((N + lead + 4 * WG - 1) / (4 * WG));
    prof_begin(c, BSCGPU_K_EMIT, (u64)N * (kv ? 5 : 9), N);
    if (kv) hipLaunchKernelGGL(st_batch_post_kernel<true>, pgrid, dim3(WG), 0, c->stream, kcur, vcur, N, lead, doff, dOut_user - lead, dindex);
    else hipLaunchKernelGGL(st_batch_post_kernel<false>, pgrid, dim3(WG), 0, c->stream, kcur, vcur, N, lead, doff, dOut_user - lead, dindex);
    prof_end(c);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(index_out, dindex, (size_t)count * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, ctx_sync(c));
    prof_collect(c);
    return radix_onesweep_check(c);
}

// One batched pass.  As st_device: the pass is sorted from a private copy of the text (the caller's output may be its input), and a
// single-read digit pass that gave up is answered by one more attempt through the three-kernel passes from that copy.
int st_batch_device(bscgpu_ctx* c, const u8* dT_user, u8* dOut_user, const int* sizes, int count, int k, const int* rates, int* index_out,
                    u32* adler_host)
{
    if (k < 3 || k > 8) return BSC_BAD_PARAMETER;
    BatchTab tab;                               // (the Adler launch reads the caller's text before the post kernel may overwrite it; the pass's last sync covers the copy)
    const int src = batch_pass_setup(c, dT_user, sizes, count, rates, index_out, adler_host, &tab);
    if (src < 0 || tab.total == 0) return src;
    return with_onesweep_retry(c, [&](bool reuse_text) {
        return st_batch_once(c, dT_user, dOut_user, tab.total, (u32)count, k, tab.off, tab.rate, tab.res, index_out, reuse_text);
    });
}

// ---------------------------------------------------------------------------------------------
// Adler-32 (adler32.cpp:82-204): s1 = 1 + sum d, s2 = sum of running s1, both mod 65521.
// Each workgroup reduces one contiguous chunk to (a = sum d, b = sum (len - pos) * d); the host
// folds the <= 1024 partials in order: s2 += len * s1 + b ; s1 += a.
// ---------------------------------------------------------------------------------------------
constexpr u32 ADLER_TILE = 16 * WG;   // 4096 bytes per iteration (16-B load per lane)

__device__ __forceinline__ u64 wave_sum_u64(u64 v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

__global__ __launch_bounds__(WG) void adler_kernel(const u8* __restrict__ T, u64 n, u32 chunk_tiles,
                                                   u64* __restrict__ part /*[chunks][2]*/)
{
    __shared__ u64 red[2 * WAVES];
    const u64 start = (u64)blockIdx.x * chunk_tiles * ADLER_TILE;
    u64 end = start + (u64)chunk_tiles * ADLER_TILE; if (end > n) end = n;
    u64 a = 0, b = 0;
    for (u64 i = start + 16ull * threadIdx.x; i < end; i += ADLER_TILE) {
        if (i + 16 <= end) {
            const uint4 q = *reinterpret_cast<const uint4*>(T + i);
            const u32 w[4] = {q.x, q.y, q.z, q.w};
            u32 s = 0, ws = 0;                       // ws = sum (15 - pos) * d  within the 16 bytes
#pragma unroll
            for (int x = 0; x < 4; ++x) {
#pragma unroll
                for (int y = 0; y < 4; ++y) {
                    const u32 d = (w[x] >> (8 * y)) & 0xffu;
                    s += d; ws += (u32)(15 - (4 * x + y)) * d;
                }
            }
            a += s;
            b += (u64)s * (end - i - 15) + ws;       // weight of byte at i+p is end - (i+p)
        } else {
            for (u64 p = i; p < end; ++p) { const u32 d = T[p]; a += d; b += (u64)d * (end - p); }
        }
    }
    a = wave_sum_u64(a); b = wave_sum_u64(b);
    const u32 w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { red[w] = a; red[WAVES + w] = b; }
    __syncthreads();
    if (threadIdx.x == 0) {
        u64 sa = 0, sb = 0;
        for (int i = 0; i < WAVES; ++i) { sa += red[i]; sb += red[WAVES + i]; }
        part[2 * blockIdx.x]     = sa % 65521ull;
        part[2 * blockIdx.x + 1] = sb % 65521ull;
    }
}

// Segmented Adler-32: one workgroup per block of a batch (blocks back to back, off[0..count]), every block's checksum in one launch.
// Lanes read consecutive bytes (blocks start anywhere, so no 16-byte loads); per lane a = sum d, b = sum (end - p) d, folded as adler_kernel's
// chunks are: s1 = 1 + a, s2 = n + b (mod 65521).
// (stride 2: off holds a (start, end) pair per block)
__global__ __launch_bounds__(WG) void adler_batch_kernel(const u8* __restrict__ T, const u32* __restrict__ off, u32* __restrict__ out, u32 stride)
{
    __shared__ u64 red[2 * WAVES];
    const u32 start = off[stride * blockIdx.x], end = off[stride * blockIdx.x + 1];
    u64 a = 0, b = 0;
    for (u32 p = start + threadIdx.x; p < end; p += WG) { const u32 d = T[p]; a += d; b += (u64)d * (end - p); }
    a = wave_sum_u64(a); b = wave_sum_u64(b);
    const u32 w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { red[w] = a; red[WAVES + w] = b; }
    __syncthreads();
    if (threadIdx.x == 0) {
        u64 sa = 0, sb = 0;
        for (int i = 0; i < WAVES; ++i) { sa += red[i]; sb += red[WAVES + i]; }
        const u64 s1 = (1ull + sa) % 65521ull, s2 = ((u64)(end - start) + sb) % 65521ull;
        out[blockIdx.x] = (u32)(s1 | (s2 << 16));
    }
}

void launch_adler_batch(bscgpu_ctx* c, const u8* d, const u32* doff, u32 count, u32* dout, u32 stride)
{
    prof_begin(c, BSCGPU_K_MISC, 0, 0);
    hipLaunchKernelGGL(adler_batch_kernel, dim3(count), dim3(WG), 0, c->stream, d, doff, dout, stride);
    prof_end(c);
}

int adler32_device(bscgpu_ctx* c, const u8* d, int64_t n, u32* out)
{
    if (n < 0) return BSC_BAD_PARAMETER;
    if (n == 0) { *out = 1; return BSC_NO_ERROR; }
    if (((uintptr_t)d) & 15) {
        // the kernel reads 16 bytes per lane: an unaligned input (a slice of a caller's tensor) goes through the context's
        // aligned text buffer first (the sorters copy the block there anyway, after this call)
        if (n > c->max_n) return ctx_fail(c, BSC_BAD_PARAMETER, "adler32: unaligned input larger than the context", hipSuccess);
        HIP_TRY(c, hipMemcpyAsync(c->dT, d, (size_t)n, hipMemcpyDeviceToDevice, c->stream));
        d = c->dT;
    }
    const Chunking ch = make_chunking((u64)n, ADLER_TILE);
    prof_begin(c, BSCGPU_K_MISC, (u64)n, 0);
    hipLaunchKernelGGL(adler_kernel, dim3(ch.num_chunks), dim3(WG), 0, c->stream, d, (u64)n, ch.chunk_tiles, c->adler_part);
    prof_end(c);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(c->hadler, c->adler_part, (size_t)ch.num_chunks * 16, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, ctx_sync(c));
    prof_collect(c);
    u64 s1 = 1, s2 = 0;
    const u64 chunk_bytes = (u64)ch.chunk_tiles * ADLER_TILE;
    for (u32 k = 0; k < ch.num_chunks; ++k) {
        const u64 start = (u64)k * chunk_bytes;
        u64 len = (u64)n - start; if (len > chunk_bytes) len = chunk_bytes;
        s2 = (s2 + (len % 65521ull) * s1 + c->hadler[2 * k + 1]) % 65521ull;
        s1 = (s1 + c->hadler[2 * k]) % 65521ull;
    }
    *out = (u32)(s1 | (s2 << 16));
    return BSC_NO_ERROR;
}
