// bwt.hip — forward Burrows-Wheeler transform of one block on MI355X: suffix sort = one LSD radix sort on packed prefix
// keys (radix_sort.hip), refinement rounds as segmented sorts on text keys, prefix doubling only for blocks with long repeats;
// then the BWT byte emit.
//
// Result contract (what bsc_bwt_encode returns, bwt.cpp:178-231, via libsais_bwt_aux, libsais.c:6704):
//   SA  = suffixes of T[0..n) in lexicographic order, a proper prefix sorting first;
//   L   = [T[n-1]] ++ [T[SA[j]-1] for j = 0..n-1 if SA[j] != 0];  primary index = ISA[0] + 1;
//   aux = I[t] = ISA[t*r] + 1 for t = 0..(n-1)/r  (I[0] is the primary index).
// The reference GPU path (libcubwt.cu:2031-2223: DC3 2/3 sample + 64-bit prefix sort + segmented sort
// + merge) is NOT followed; this is a different algorithm with the same result:
//
//   1. bwt_pack:   key[s] = the first w characters of suffix i as dense alphabet codes (w = 8..16), value = i (+ the code of
//                  the character in front of it in the spare high bits).  The < w "tail" suffixes whose window crosses the
//                  block end are placed FIRST in input order, shortest first; the LSD sort is stable, so inside a group of
//                  equal padded keys they come out first and already in final order ("proper prefix is smaller"), and seg
//                  marks each of them as a finished singleton.
//   2. <= 8 radix passes over (u64 key, u32 suffix) -> order by w-character prefix.
//   3. seg (reduce / scan / apply): group heads, rank = position of the group head (so ranks are valid SA slots and only
//      ever grow under refinement), stream compaction of every suffix still sharing its rank ("unsorted").
//   4. rounds on text keys (bwt_round_textsort_kernel): the groups are refined by the next a characters of the text behind
//      the h characters they share — no inverse suffix array; h += a.  Blocks that converge this way (text: two rounds)
//      never build ISA.
//   5. otherwise ISA is built once from the current order and the rounds double h (bwt_round_segsort_kernel on ISA[sa+h],
//      radix fallback for groups longer than a workgroup sorts).  One 4-byte D2H + stream sync per round for the loop
//      test (libcubwt does the same, libcubwt.cu:1383).
//   6. bwt_find / bwt_emit: primary and aux indexes from a scan of SA, L from SA (predecessor codes) or SA/T.
#include "dev_common.h"
#include "radix_dev.h"
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

constexpr int SEG_ITEMS = 8;
constexpr int SEG_TILE  = WG * SEG_ITEMS;      // 2048 records per tile, 8 consecutive per thread

// ---------------------------------------------------------------------------------------------
// Byte histogram of the block (replicated LDS bins against skew) -> alphabet size K and dense codes.
__global__ __launch_bounds__(WG) void bwt_bytehist_kernel(const u8* __restrict__ T, u32 n, u32 chunk_bytes, u32* __restrict__ hist)
{
    __shared__ u32 h[8 * 256];
    for (u32 i = threadIdx.x; i < 8 * 256; i += WG) h[i] = 0;
    __syncthreads();
    u32* hw = h + (threadIdx.x & 7) * 256;
    const u64 start = (u64)blockIdx.x * chunk_bytes;
    u64 end = start + chunk_bytes; if (end > n) end = n;
    for (u64 i = start + 16ull * threadIdx.x; i < end; i += 16ull * WG) {
        if (i + 16 <= end) {
            const uint4 q = *reinterpret_cast<const uint4*>(T + i);
            const u32 w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
            for (int x = 0; x < 4; ++x) {
                atomicAdd(&hw[w[x] & 255u], 1u); atomicAdd(&hw[(w[x] >> 8) & 255u], 1u);
                atomicAdd(&hw[(w[x] >> 16) & 255u], 1u); atomicAdd(&hw[w[x] >> 24], 1u);
            }
        } else for (u64 p = i; p < end; ++p) atomicAdd(&hw[T[p]], 1u);
    }
    __syncthreads();
    u32 sum = 0;
#pragma unroll
    for (int r = 0; r < 8; ++r) sum += h[r * 256 + threadIdx.x];
    if (sum) atomicAdd(&hist[threadIdx.x], sum);
}

// Alphabet-compacted prefix keys.  codes[c] = order-preserving dense code of byte c (bits per code = cb), a key
// holds the first w = min(16, 64 / cb) characters of the suffix, most significant first, zero (= smallest code)
// padded past the block end.  Text with <= 32 distinct bytes thus sorts on 12-16 characters in the same 8 passes
// that raw bytes spend on 8, which removes most of the first doubling round's work.
// Suffixes whose window crosses the end ("tails", i + w > n, at most w-1 of them) go FIRST in input order, shortest
// first: the stable sort then leaves them first inside any group of equal padded keys, already in final order.
struct PackParams { u32 cb; u32 w; u32 tc; u32 low_shift; u32 pred_shift; };   // pred_shift: 0 = values are plain suffix indexes,
                                                                               // else value = index | code(T[i-1]) << pred_shift

__global__ __launch_bounds__(WG) void bwt_pack_kernel(const u8* __restrict__ T, u32 n, PackParams pp,
                                                      const u8* __restrict__ codes, u64* __restrict__ keys, u32* __restrict__ vals)
{
    // A thread builds the keys of four consecutive suffixes (their windows share all but three characters); written from there the
    // stores of a wavefront have a 32-byte lane pitch — every line of the output is touched by four instructions.  The workgroup's
    // 1024 records therefore go through LDS and leave lane-contiguous (the few tail suffixes, whose slots are elsewhere, directly).
    __shared__ u8 lut[256];
    __shared__ u64 skey[4 * WG];
    __shared__ u32 sval[4 * WG];
    lut[threadIdx.x] = codes[threadIdx.x];
    __syncthreads();
    const u32 b0 = 4u * blockIdx.x * WG;                                 // first suffix of the workgroup
    const u32 i0 = b0 + 4u * threadIdx.x;
    if (i0 < n) {
        // characters i0 .. i0 + w + 2 (<= 19 bytes; T is 16-B aligned at T[0] and zero padded for 32 bytes past n)
        const u32* T32 = reinterpret_cast<const u32*>(T + i0);
        u32 wds[5];
#pragma unroll
        for (int x = 0; x < 5; ++x) wds[x] = T32[x];
        u32 pcode = (pp.pred_shift && i0 > 0) ? (u32)lut[T[i0 - 1]] : 0u;        // code of the character in front of suffix i0
        u64 cd[19];                                     // codes of characters i0 .. i0+18 (0 past the end)
#pragma unroll
        for (u32 t = 0; t < 19; ++t) {
            const u32 c = (wds[t >> 2] >> (8 * (t & 3))) & 0xffu;
            cd[t] = (i0 + t < n) ? (u64)lut[c] : 0ull;
        }
#pragma unroll
        for (u32 j = 0; j < 4; ++j) {
            const u32 i = i0 + j;
            if (i < n) {
                u64 key = 0;
#pragma unroll
                for (u32 t = 0; t < 16; ++t) if (t < pp.w) key |= cd[j + t] << (64 - pp.cb * (t + 1));
                const u32 val = pp.pred_shift ? (i | (pcode << pp.pred_shift)) : i;
                const bool tail = (u64)i + pp.w > (u64)n;
                if (tail) { keys[n - 1 - i] = key; vals[n - 1 - i] = val; }
                else { skey[4u * threadIdx.x + j] = key; sval[4u * threadIdx.x + j] = val; }
                pcode = (u32)cd[j];                                                 // this suffix's first character precedes the next one
            }
        }
    }
    __syncthreads();
#pragma unroll
    for (u32 k = 0; k < 4; ++k) {
        const u32 li = k * WG + threadIdx.x, i = b0 + li;
        if (i < n && (u64)i + pp.w <= (u64)n) { keys[i + pp.tc] = skey[li]; vals[i + pp.tc] = sval[li]; }
    }
}

// ---------------------------------------------------------------------------------------------
// Folded packing: the key's lowest r = (cb * w) mod 8 bits (1..4 of them, all inside its last character) are sorted HERE, while every
// record is written anyway, and the digit passes that follow are whole bytes — one pass fewer (bwt_device_once has the plan).
//   bwt_fold_count_kernel   one read of the text: digit of suffix i = codes[T[i + w - 1]] & (2^r - 1), counted per packing tile
//                           (FOLD_TILE consecutive suffixes); tails are not counted — their last character is padding, digit 0, and they
//                           keep their slots [0, tc), the head of bucket 0.
//   bwt_fold_scan_kernel    per bucket d and scan segment s (64 per bucket): off[d][tile] = records of d in the segment's tiles below,
//                           segtot[d][s] = all of the segment's.  Packing sums the 1024 totals itself (bucket-major: tails, buckets below,
//                           segments below), so the tile's first record of digit d has its slot and nothing waits for another workgroup.
//   bwt_pack_fold_kernel    keys and values exactly as bwt_pack_kernel forms them; the tile's records are ranked inside their digit in
//                           suffix order (wave-striped, ballot match, per-wave counters, one scan over digit x wave), reordered in LDS so
//                           that every digit leaves as one run, and written at the scanned offsets.  Stable: bucket order = tile order,
//                           then suffix order, and bucket 0 starts with the tails — the input order the tails-first rule above needs.
//                           HIST: also the 256-bin totals of the np byte digits above the folded one, all n keys (tails included), in
//                           replicated LDS counters that a workgroup — the grid is persistent — adds to the digit passes' tables once.
// ---------------------------------------------------------------------------------------------
#ifndef FOLD_REPL_N
#define FOLD_REPL_N 1           // replicas of the fused digit counters (a power of two; by lane)
#endif
#ifndef FOLD_WGS_PER_CU
#define FOLD_WGS_PER_CU 6       // persistent workgroups per CU: what the LDS of FOLD_REPL_N replicas (and 80 VGPRs) leaves room for
#endif
constexpr int FOLD_WAVES = WG / 64, FOLD_TILE = 4 * WG /* 1024 suffixes, four consecutive ones per thread */, FOLD_NB = 16 /* buckets at most */,
              FOLD_BINS = 32 /* counter stride of a wave */, FOLD_REPL = FOLD_REPL_N, FOLD_MAXP = 7, FOLD_SEGS = 64 /* scan segments of a bucket */;
static_assert(FOLD_NB * FOLD_SEGS == 4 * WG, "packing scans the segment totals four per thread");
static_assert(FOLD_NB * FOLD_WAVES == 64, "the tile scan is one wavefront's: a (digit, wave) pair per lane");
static size_t fold_lds_bytes(u32 np) { return (size_t)FOLD_REPL * np * 256 * 4; }

// one wavefront per tile: a lane reads 16 of its 1024 characters, lane 0 also the w - 1 that follow
__global__ __launch_bounds__(WG) void bwt_fold_count_kernel(const u8* __restrict__ T, u32 n, u32 w, u32 dmask, const u8* __restrict__ codes,
                                                            u32 ntiles, u32* __restrict__ cnt /*[FOLD_NB][ntiles]*/)
{
    __shared__ u8 lut[256];
    __shared__ u32 h[FOLD_WAVES][16 * 17];                               // per wave: 16 replicas (by lane), 17 words apart
    const u32 t = threadIdx.x, wv = t >> 6, lane = t & 63u;
    const u32 tile = blockIdx.x * (u32)FOLD_WAVES + wv;
    lut[t] = codes[t] & (u8)dmask;
    for (u32 i = lane; i < 16 * 17; i += 64) h[wv][i] = 0;
    __syncthreads();
    // last characters of the tile's suffixes that are no tails: positions [base + w - 1, base + FOLD_TILE + w - 1) below n
    const u64 base = (u64)tile * FOLD_TILE, lo = base + w - 1;
    u64 hi = base + FOLD_TILE + w - 1; if (hi > n) hi = n;
    u32* hr = h[wv] + (lane & 15u) * 17;
    if (tile < ntiles) {
        for (u32 ch = lane; ch < FOLD_TILE / 16 + 1; ch += 64) {
            const u64 a = base + 16ull * ch;                             // (a < hi <= n: the 16 bytes end inside the text's zero padding)
            if (a < hi) {
                const uint4 q = *reinterpret_cast<const uint4*>(T + a);
                const u32 wd[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
                for (u32 x = 0; x < 16; ++x) {
                    const u64 p = a + x;
                    if (p >= lo && p < hi) atomicAdd(&hr[lut[(wd[x >> 2] >> (8 * (x & 3))) & 0xffu]], 1u);
                }
            }
        }
    }
    __syncthreads();
    if (tile < ntiles && lane < (u32)FOLD_NB) {
        u32 sum = 0;
#pragma unroll
        for (int r = 0; r < 16; ++r) sum += h[wv][r * 17 + lane];
        cnt[(size_t)lane * ntiles + tile] = sum;
    }
}

// one workgroup per digit and segment (FOLD_SEGS segments of seg_tiles tiles): off[d][tile] = records of digit d in the tiles of the
// segment below this one, segtot[d][s] = all of the segment's
__global__ __launch_bounds__(WG) void bwt_fold_scan_kernel(const u32* __restrict__ cnt, u32 ntiles, u32 seg_tiles, u32* __restrict__ off, u32* __restrict__ segtot)
{
    __shared__ u32 scr[8];
    const u32 t = threadIdx.x, sg = blockIdx.x, d = blockIdx.y;
    const u32 s0 = sg * seg_tiles;
    const u32 s1 = (s0 + seg_tiles < ntiles) ? s0 + seg_tiles : ntiles;           // (s0 may lie past the end: an empty segment)
    const u32 per = (seg_tiles + WG - 1) / WG;
    const u32 b = s0 + t * per, e = (b + per < s1) ? b + per : s1;
    const u32* row = cnt + (size_t)d * ntiles;
    u32 own = 0;
    for (u32 i = b; i < e; ++i) own += row[i];
    u32 tot;
    u32 run = block_excl_sum(own, scr, &tot);
    for (u32 i = b; i < e; ++i) { off[(size_t)d * ntiles + i] = run; run += row[i]; }
    if (t == 0) segtot[d * (u32)FOLD_SEGS + sg] = tot;
}

template <bool HIST>
__global__ __launch_bounds__(WG) void bwt_pack_fold_kernel(const u8* __restrict__ T, u32 n, PackParams pp, u32 rbits,
                                                           const u8* __restrict__ codes, const u32* __restrict__ off, const u32* __restrict__ segtot,
                                                           u32 ntiles, u32 seg_tiles, u64* __restrict__ keys, u32* __restrict__ vals,
                                                           u32 np, u32* __restrict__ totals, u32 pass_stride)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char fold_smem[];
    u32* hh = reinterpret_cast<u32*>(fold_smem);                         // [FOLD_REPL][np][256]
    __shared__ u64 skey[FOLD_TILE];                                      // the tile in suffix order, then bucket by bucket
    __shared__ u32 sval[FOLD_TILE];
    __shared__ u8 lut[256];
    __shared__ u32 wh[FOLD_WAVES * FOLD_BINS];                           // per wave: digit counters, then the tile-local start of its records of each digit
    __shared__ u32 sbase[FOLD_NB * FOLD_SEGS];                           // first slot of every (bucket, segment): the tails, the buckets below, the bucket's segments below
    __shared__ u32 scr[8];
    __shared__ u32 adj[FOLD_NB];                                         // output slot of tile-local slot q of digit d = adj[d] + q
    lds_vu32* vwh = (lds_vu32*)wh;
    const u32 t = threadIdx.x, w = t >> 6, lane = t & 63u;
    lut[t] = codes[t];
    {
        // bucket-major, so one exclusive sum over the table is the layout of the output
        const uint4 q = *reinterpret_cast<const uint4*>(segtot + 4u * t);
        u32 tot;
        const u32 ex = pp.tc + block_excl_sum(q.x + q.y + q.z + q.w, scr, &tot);
        sbase[4u * t] = ex; sbase[4u * t + 1] = ex + q.x; sbase[4u * t + 2] = ex + q.x + q.y; sbase[4u * t + 3] = ex + q.x + q.y + q.z;
    }
    if (HIST) for (u32 i = t; i < (u32)FOLD_REPL * np * 256u; i += WG) hh[i] = 0;
    __syncthreads();
    const u32 dmask = (1u << rbits) - 1u;
    const u32 nt_end = n >= pp.w ? n - pp.w + 1 : 0;                     // suffixes below this index are no tails
    u32* hr = hh + (lane & (u32)(FOLD_REPL - 1)) * np * 256u;
    const u64 lt = lanemask_lt();

    for (u32 tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const u32 b0 = tile * (u32)FOLD_TILE;                            // first suffix of the tile
        const u32 i0 = b0 + 4u * t;
        if (lane < (u32)FOLD_BINS) wh[w * FOLD_BINS + lane] = 0;
        if (i0 < n) {
            // bwt_pack_kernel's keys and values.  The kernel is bound by its VALU work, so the four keys are not built character by
            // character: the first is, and each next one is the one before shifted up by a character (its first character leaves
            // through the top) with the next character put in at low_shift.
            const u32* T32 = reinterpret_cast<const u32*>(T + i0);
            u32 wds[5];
#pragma unroll
            for (int x = 0; x < 5; ++x) wds[x] = T32[x];
            u32 pcode = (pp.pred_shift && i0 > 0) ? (u32)lut[T[i0 - 1]] : 0u;
            u32 cd[19];                                     // codes of characters i0 .. i0+18 (0 past the end)
#pragma unroll
            for (u32 x = 0; x < 19; ++x) {
                const u32 ch = (wds[x >> 2] >> (8 * (x & 3))) & 0xffu;
                cd[x] = (i0 + x < n) ? (u32)lut[ch] : 0u;
            }
            u64 key = 0;
            u32 ext = 0;                                    // characters w, w + 1, w + 2, the first of them on top
#pragma unroll
            for (u32 x = 0; x < 19; ++x) {
                if (x < pp.w) { if (x < 16) key |= (u64)cd[x] << (64 - pp.cb * (x + 1)); }
                else if (x < pp.w + 3) ext |= cd[x] << (pp.cb * (pp.w + 2 - x));
            }
            const u32 cmask = (1u << pp.cb) - 1u;
#pragma unroll
            for (u32 j = 0; j < 4; ++j) {
                const u32 i = i0 + j;
                if (i < n) {
                    const u32 val = pp.pred_shift ? (i | (pcode << pp.pred_shift)) : i;
                    if (HIST) {
                        // (the digits are whole bytes of the key: its top np)
                        const u32 klo = (u32)key, khi = (u32)(key >> 32);
#pragma unroll
                        for (u32 bb = 1; bb < 8; ++bb)
                            if (bb >= 8u - np) atomicAdd(&hr[(bb - (8u - np)) * 256u + (((bb < 4 ? klo : khi) >> (8 * (bb & 3))) & 0xffu)], 1u);
                    }
                    if (i >= nt_end) { keys[n - 1 - i] = key; vals[n - 1 - i] = val; }
                    else { skey[4u * t + j] = key; sval[4u * t + j] = val; }
                    pcode = cd[j];
                }
                if (j < 3) key = (key << pp.cb) | ((u64)((ext >> (pp.cb * (2 - j))) & cmask) << pp.low_shift);
            }
        }
        __syncthreads();
        // the tile's records that are no tails are its first nv; a wave ranks 256 consecutive ones, item-major
        const u32 nv = nt_end > b0 ? ((nt_end - b0 < (u32)FOLD_TILE) ? nt_end - b0 : (u32)FOLD_TILE) : 0u;
        u64 k[4]; u32 v[4], dg[4], rk[4];
#pragma unroll
        for (u32 j = 0; j < 4; ++j) {
            const u32 q = w * 256u + j * 64u + lane;
            const bool valid = q < nv;
            k[j] = valid ? skey[q] : 0ull;
            v[j] = valid ? sval[q] : 0u;
            dg[j] = valid ? ((u32)(k[j] >> pp.low_shift) & dmask) : (u32)FOLD_NB;       // slots past the end: a bucket of their own, never written
        }
#pragma unroll
        for (u32 j = 0; j < 4; ++j) {
            u64 m = ~0ull;
#pragma unroll
            for (u32 b = 0; b < 5; ++b) {
                const bool bit = (dg[j] >> b) & 1u;
                const u64 bal = __ballot(bit);
                m &= bit ? bal : ~bal;
            }
            const u32 before = vwh[w * FOLD_BINS + dg[j]];
            const u32 r = (u32)__popcll(m & lt), cnt = (u32)__popcll(m);
            rk[j] = before + r;
            if (r == cnt - 1) vwh[w * FOLD_BINS + dg[j]] = before + cnt;                 // highest peer lane publishes
        }
        __syncthreads();
        if (w == 0) {
            const u32 sd = lane >> 2, sw = lane & 3u;                    // digit-major, then wave: the scan is the tile's bucket layout
            const u32 c = wh[sw * FOLD_BINS + sd];
            const u32 ex = wave_incl_sum(c) - c;
            wh[sw * FOLD_BINS + sd] = ex;
            if (sw == 0) adj[sd] = sbase[sd * (u32)FOLD_SEGS + tile / seg_tiles] + off[(size_t)sd * ntiles + tile] - ex;
        }
        __syncthreads();
#pragma unroll
        for (u32 j = 0; j < 4; ++j) {
            if (dg[j] < (u32)FOLD_NB) {
                const u32 pos = wh[w * FOLD_BINS + dg[j]] + rk[j];
                skey[pos] = k[j]; sval[pos] = v[j];
            }
        }
        __syncthreads();
#pragma unroll
        for (u32 j = 0; j < 4; ++j) {
            const u32 q = j * (u32)WG + t;
            if (q < nv) {
                const u64 key = skey[q];
                const u32 o = adj[(u32)(key >> pp.low_shift) & dmask] + q;
                if (o < n) { keys[o] = key; vals[o] = sval[q]; }         // (always, when the counts are those of this text: the test keeps a store inside the arrays whatever it is given)
            }
        }
        __syncthreads();
    }
    if (HIST) {
        for (u32 i = t; i < np * 256u; i += WG) {
            u32 sum = 0;
#pragma unroll
            for (u32 r = 0; r < (u32)FOLD_REPL; ++r) sum += hh[r * np * 256u + i];
            if (sum) atomicAdd(&totals[(size_t)(i >> 8) * pass_stride + (i & 255u)], sum);
        }
    }
}

// ---------------------------------------------------------------------------------------------
// seg phase A: head / unsorted flags + per-chunk summaries.
//   head(x)  = x == 0 || key[x] != key[x-1] || (INITIAL && (tail(sa[x]) || tail(sa[x-1])))
//   uns(x)   = !(head(x) && head(x+1)), head(m) = 1
//   flags[x] = head | uns << 1 | oldhead << 2
//   oldhead (doubling rounds, grp_shift = the width of the key's next-rank field): x is also the first record of a group of the round's
//   INPUT — the group rank in the key's high bits changes there.  Records of a new group that starts at an old head keep their rank, and
//   seg_apply skips their (random, 4-byte) ISA stores: most of them while the unsorted set shrinks slowly.
// ---------------------------------------------------------------------------------------------
//   grp (rounds on text keys, see bwt_round_textsort_kernel): the group rank of every record is a separate array and a head is
//   also where it changes: head(x) |= grp[x] != grp[x-1]
template <bool INITIAL>
__global__ __launch_bounds__(WG) void seg_reduce_kernel(const u64* __restrict__ keys, const u32* __restrict__ sa,
                                                        u32 m, u32 tail_lo, u32 smask, u32 chunk_tiles, u32 num_tiles,
                                                        u8* __restrict__ flags, u32* __restrict__ segsum /*[2][MAX_CHUNKS]*/,
                                                        const u32* __restrict__ grp = nullptr, int grp_shift = 0)
{
    __shared__ u32 scr[8];
    const u32 t = threadIdx.x;
    const u32 tile0 = blockIdx.x * chunk_tiles;
    u32 tile1 = tile0 + chunk_tiles; if (tile1 > num_tiles) tile1 = num_tiles;
    // suffix i is a tail (window crosses the block end) iff i >= tail_lo

    u32 cnt = 0, last1 = 0;
    for (u32 tile = tile0; tile < tile1; ++tile) {
        const u32 j = tile * SEG_TILE + t * SEG_ITEMS;
        if (j >= m) continue;
        u64 k[SEG_ITEMS + 2];          // keys j-1 .. j+8
        u32 s[SEG_ITEMS + 2];
        const bool full = (j + SEG_ITEMS <= m);
        if (full) {
#pragma unroll
            for (int q = 0; q < SEG_ITEMS; q += 2) {
                const ulonglong2 kk = *reinterpret_cast<const ulonglong2*>(keys + j + q);
                k[1 + q] = kk.x; k[2 + q] = kk.y;
            }
        } else {
#pragma unroll
            for (int q = 0; q < SEG_ITEMS; ++q) k[1 + q] = (j + q < m) ? keys[j + q] : 0;
        }
        k[0] = (j > 0) ? keys[j - 1] : 0;
        k[SEG_ITEMS + 1] = (j + SEG_ITEMS < m) ? keys[j + SEG_ITEMS] : 0;
        if (INITIAL || grp != nullptr) {
            // suffix numbers (first seg) / group ranks (text rounds) j-1 .. j+8: the thread's own eight as two 16-byte loads (ten
            // 4-byte loads at a 32-byte lane pitch put every line through the address path eight times)
            const u32* src = INITIAL ? sa : grp;
            const u32 msk = INITIAL ? smask : 0xffffffffu;
            if (full && SEG_ITEMS == 8) {
                const uint4 a = *reinterpret_cast<const uint4*>(src + j), b = *reinterpret_cast<const uint4*>(src + j + 4);
                s[1] = a.x & msk; s[2] = a.y & msk; s[3] = a.z & msk; s[4] = a.w & msk;
                s[5] = b.x & msk; s[6] = b.y & msk; s[7] = b.z & msk; s[8] = b.w & msk;
                s[0] = (j > 0) ? (src[j - 1] & msk) : 0;
                s[9] = (j + 8 < m) ? (src[j + 8] & msk) : 0;
            } else {
#pragma unroll
                for (int q = 0; q < SEG_ITEMS + 2; ++q) {
                    const long long x = (long long)j - 1 + q;
                    s[q] = (x >= 0 && x < (long long)m) ? (src[x] & msk) : 0;
                }
            }
        }
        u32 h[SEG_ITEMS + 1], oh[SEG_ITEMS + 1];
#pragma unroll
        for (int q = 0; q <= SEG_ITEMS; ++q) {
            const u32 x = j + q;
            bool hd, od = false;
            if (x == 0 || x >= m) { hd = true; od = grp_shift > 0; }
            else {
                hd = (k[q + 1] != k[q]);
                if (INITIAL) hd = hd || (s[q + 1] >= tail_lo) || (s[q] >= tail_lo);
                else if (grp != nullptr) hd = hd || (s[q + 1] != s[q]);
                else if (grp_shift > 0) od = (k[q + 1] >> grp_shift) != (k[q] >> grp_shift);
            }
            h[q] = hd ? 1u : 0u; oh[q] = od ? 1u : 0u;
        }
        u64 packed = 0;
#pragma unroll
        for (int q = 0; q < SEG_ITEMS; ++q) {
            const u32 x = j + q;
            if (x < m) {
                const u32 uns = (h[q] & h[q + 1]) ^ 1u;
                packed |= (u64)(h[q] | (uns << 1) | (oh[q] << 2)) << (8 * q);
                cnt += uns;
                if (h[q]) last1 = x + 1;
            }
        }
        if (full) *reinterpret_cast<u64*>(flags + j) = packed;
        else {
#pragma unroll
            for (int q = 0; q < SEG_ITEMS; ++q) if (j + q < m) flags[j + q] = (u8)(packed >> (8 * q));
        }
    }
    u32 tot, mx;
    block_excl_sum(cnt, scr, &tot);
    block_incl_max(last1, scr, &mx);
    if (t == 0) { segsum[blockIdx.x] = tot; segsum[MAX_CHUNKS + blockIdx.x] = mx; }
}

// Geometry of the segmented sorts of the refinement rounds (bwt_round_segsort_kernel / bwt_round_textsort_kernel below): a workgroup owns
// the groups whose head lies in its tile of RS_T records and sees RS_G records past the tile, so a group of up to RS_G + 1 records always
// fits; seg_apply counts the groups that do not (see there).
constexpr int RS_T = 2048, RS_G = 1024, RS_E = RS_T + RS_G;       // 24 KB of LDS per workgroup: 6 workgroups per CU hide the ISA gather
// seg_apply counts the groups of > RS_G records in the new unsorted set and their records past the first RS_G (dev_common.h: DS_NLONG, DS_EXCESS),
// and the same for groups of more than HY_G records (DS_NMID, DS_MIDEXCESS; hybrid doubling rounds, bwt_longrec_kernel): the segmented sort ranks a
// record by counting inside its group — s comparisons per record of a group of s —, the radix engine costs ~50 ps per record whatever the group.
constexpr int HY_G = 256;

// seg phase B: one workgroup scans the <= 1024 chunk summaries.
//   segoff[c]            = exclusive sum of unsorted counts
//   segoff[MAX_CHUNKS+c] = max(last head + 1) over chunks < c
//   dscal[DS_TOTAL]      = total unsorted
__global__ __launch_bounds__(WG) void seg_scan_kernel(const u32* __restrict__ segsum, u32 num_chunks,
                                                      u32* __restrict__ segoff, u32* __restrict__ dscal)
{
    __shared__ u32 scr[8];
    __shared__ u32 smax[WG];
    u32 carry = 0, carrymax = 0;
    for (u32 base = 0; base < num_chunks; base += WG) {
        const u32 i = base + threadIdx.x;
        const u32 v  = (i < num_chunks) ? segsum[i] : 0u;
        const u32 mx = (i < num_chunks) ? segsum[MAX_CHUNKS + i] : 0u;
        u32 tot, totmax;
        const u32 ex = block_excl_sum(v, scr, &tot);
        const u32 im = block_incl_max(mx, scr, &totmax);
        __syncthreads();
        smax[threadIdx.x] = im;
        __syncthreads();
        const u32 exmax = (threadIdx.x > 0) ? smax[threadIdx.x - 1] : 0u;
        if (i < num_chunks) {
            segoff[i] = carry + ex;
            segoff[MAX_CHUNKS + i] = (carrymax > exmax) ? carrymax : exmax;
        }
        carry += tot;
        carrymax = (carrymax > totmax) ? carrymax : totmax;
        __syncthreads();
    }
    if (threadIdx.x == 0) { dscal[DS_TOTAL] = carry; dscal[DS_NLONG] = 0; dscal[DS_EXCESS] = 0; dscal[DS_NMID] = 0; dscal[DS_MIDEXCESS] = 0; }   // (seg_apply, the next launch, adds to the counters)
}

// seg phase C: ranks (position of the group head), SA / ISA write-back, compaction of unsorted records.
// WRITE_ISA = false (rounds on text keys): nobody reads ISA, the random 4-byte scatter is skipped.
// Also counts, for free, what the next round's segmented sort cannot take: an unsorted record knows its SA slot and its group's rank (the
// slot of the group's head), and members of a group are contiguous in SA — the record RS_G places behind its head proves a group of more
// than RS_G records (one such record per long group: dscal[DS_NLONG]), every record at or beyond that distance is counted in
// dscal[DS_EXCESS].  The host reads both with the size of the unsorted set and never launches a segmented sort that would give up.
template <bool INITIAL, bool WRITE_ISA>
__global__ __launch_bounds__(WG) void seg_apply_kernel(const u8* __restrict__ flags, const u32* sa_sorted,
                                                       const u32* __restrict__ cpos_in, u32 m, u32 smask,
                                                       u32 chunk_tiles, u32 num_tiles, const u32* __restrict__ segoff,
                                                       u32* SA, u32* __restrict__ ISA,
                                                       u32* __restrict__ cpos_out, u32* __restrict__ csa_out,
                                                       u32* __restrict__ cgrp_out, u32* __restrict__ dscal)
{
    __shared__ u32 scr[8];
    __shared__ u32 sprev[WG];
    __shared__ u32 cstage[3 * SEG_TILE];            // SA slot, suffix, group rank of the tile's unsorted records
    __shared__ u32 slong[4];
    const u32 t = threadIdx.x;
    // A single-read digit pass in front of this seg gave up a wait (radix_onesweep.hip): its output is in bounds but not sorted, and the
    // workgroups that stopped claiming tiles left stale records behind — suffix numbers that, masked, can exceed n.  Nothing of that may
    // be scattered into SA / ISA (the host finds the word raised right after this launch and redoes the transform).
    // (this relies on the word being STICKY: only radix_onesweep_check, on the host behind this launch, clears it — dev_common.h)
    if (dscal[OS_ERR_SLOT] != 0u) return;
    if (t < 4) slong[t] = 0;
    u32 n_long = 0, n_excess = 0, n_mid = 0, n_midx = 0;
    const u32 tile0 = blockIdx.x * chunk_tiles;
    u32 tile1 = tile0 + chunk_tiles; if (tile1 > num_tiles) tile1 = num_tiles;
    u32 off   = segoff[blockIdx.x];                 // next compacted slot
    // heads travel as (SA slot + 1) << 1 | oldhead: monotone in the slot, so the running maximum is still "the last head", and its low bit
    // says whether the group it opens keeps the rank its records already have in ISA (seg_reduce: oldhead)
    u32 carry = segoff[MAX_CHUNKS + blockIdx.x];    // (head index + 1) carried in from the left
    if (carry) carry = INITIAL ? carry << 1 : (((cpos_in[carry - 1] + 1) << 1) | ((flags[carry - 1] >> 2) & 1u));   // compacted index -> SA slot of that head

    for (u32 tile = tile0; tile < tile1; ++tile) {
        const u32 j = tile * SEG_TILE + t * SEG_ITEMS;
        u32 f[SEG_ITEMS], pos[SEG_ITEMS], s[SEG_ITEMS];
        u32 lmax = 0, lcnt = 0;
        if (SEG_ITEMS == 8 && j + SEG_ITEMS <= m) {
            // a thread's eight records: flags as one 8-byte load, suffixes (and SA slots) as two 16-byte loads each — not 8 + 8 (+ 8) narrow ones
            const u64 fw = *reinterpret_cast<const u64*>(flags + j);
            const uint4 s0 = *reinterpret_cast<const uint4*>(sa_sorted + j), s1 = *reinterpret_cast<const uint4*>(sa_sorted + j + 4);
            s[0] = s0.x; s[1] = s0.y; s[2] = s0.z; s[3] = s0.w; s[4] = s1.x; s[5] = s1.y; s[6] = s1.z; s[7] = s1.w;
            if (INITIAL) {
#pragma unroll
                for (int q = 0; q < 8; ++q) pos[q] = j + q;
            } else {
                const uint4 p0 = *reinterpret_cast<const uint4*>(cpos_in + j), p1 = *reinterpret_cast<const uint4*>(cpos_in + j + 4);
                pos[0] = p0.x; pos[1] = p0.y; pos[2] = p0.z; pos[3] = p0.w; pos[4] = p1.x; pos[5] = p1.y; pos[6] = p1.z; pos[7] = p1.w;
            }
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                f[q] = (u32)(fw >> (8 * q)) & 0xffu;
                if (f[q] & 1u) lmax = ((pos[q] + 1) << 1) | ((f[q] >> 2) & 1u);
                lcnt += (f[q] >> 1) & 1u;
            }
        } else {
#pragma unroll
            for (int q = 0; q < SEG_ITEMS; ++q) {
                const u32 x = j + q;
                if (x < m) {
                    f[q]   = flags[x];
                    pos[q] = INITIAL ? x : cpos_in[x];
                    s[q]   = sa_sorted[x];
                    if (f[q] & 1u) lmax = ((pos[q] + 1) << 1) | ((f[q] >> 2) & 1u);
                    lcnt += (f[q] >> 1) & 1u;
                } else { f[q] = 0; pos[q] = 0; s[q] = 0; }
            }
        }
        u32 totmax, totcnt;
        const u32 imax = block_incl_max(lmax, scr, &totmax);
        __syncthreads();
        sprev[t] = imax;
        __syncthreads();
        u32 run = (t > 0) ? sprev[t - 1] : 0u;       // exclusive max over lower threads
        if (carry > run) run = carry;
        u32 kslot = block_excl_sum(lcnt, scr, &totcnt);          // compacted index inside the tile
#pragma unroll
        for (int q = 0; q < SEG_ITEMS; ++q) {
            const u32 x = j + q;
            if (x < m) {
                if (f[q] & 1u) run = ((pos[q] + 1) << 1) | ((f[q] >> 2) & 1u);
                const u32 rank = (run >> 1) - 1;
                if (!INITIAL || SA != sa_sorted) SA[pos[q]] = s[q];          // the first seg may run in place: SA = the sort's value array
                if (WRITE_ISA && (INITIAL || !(run & 1u))) ISA[s[q] & smask] = rank;   // SA / csa keep the predecessor code in their high bits
                if (f[q] & 2u) {
                    cstage[kslot] = pos[q]; cstage[SEG_TILE + kslot] = s[q]; cstage[2 * SEG_TILE + kslot] = rank; ++kslot;
                    const u32 dist = pos[q] - rank;
                    n_long += (u32)(dist == (u32)RS_G); n_excess += (u32)(dist >= (u32)RS_G);
                    n_mid += (u32)(dist == (u32)HY_G); n_midx += (u32)(dist >= (u32)HY_G);
                }
            }
        }
        __syncthreads();
        // the tile's unsorted records leave through LDS: consecutive lanes write consecutive slots of the three arrays
        for (u32 i = t; i < totcnt; i += WG) {
            cpos_out[off + i] = cstage[i];
            csa_out[off + i]  = cstage[SEG_TILE + i];
            cgrp_out[off + i] = cstage[2 * SEG_TILE + i];
        }
        carry = (carry > totmax) ? carry : totmax;
        off += totcnt;
        __syncthreads();
    }
    if (n_midx) {
        atomicAdd(&slong[3], n_midx); if (n_mid) atomicAdd(&slong[2], n_mid);
        if (n_excess) { atomicAdd(&slong[1], n_excess); if (n_long) atomicAdd(&slong[0], n_long); }
    }
    __syncthreads();
    if (t == 0 && slong[3]) {
        atomicAdd(&dscal[DS_MIDEXCESS], slong[3]); if (slong[2]) atomicAdd(&dscal[DS_NMID], slong[2]);
        if (slong[1]) { atomicAdd(&dscal[DS_EXCESS], slong[1]); if (slong[0]) atomicAdd(&dscal[DS_NLONG], slong[0]); }
    }
}

// ---------------------------------------------------------------------------------------------
// doubling round key build: key = rank << 32 | (ISA[sa + h] + 1, 0 when sa + h == n)
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(WG) void bwt_gather_kernel(const u32* __restrict__ csa, const u32* __restrict__ cgrp,
                                                        const u32* __restrict__ ISA, u32 U, u64 h, u64 n, int lo_bits, u32 smask,
                                                        u64* __restrict__ keys, u32* __restrict__ vals)
{
    const u32 stride = gridDim.x * WG;
    for (u32 k = blockIdx.x * WG + threadIdx.x; k < U; k += stride) {
        const u32 s = csa[k];
        const u64 p = (u64)(s & smask) + h;
        const u32 nxt = (p < n) ? (ISA[p] + 1u) : 0u;
        keys[k] = ((u64)cgrp[k] << lo_bits) | nxt;
        vals[k] = s;
    }
}


// ---------------------------------------------------------------------------------------------
// Doubling round as a SEGMENTED sort (what libcubwt does with cub::DeviceSegmentedSort, libcubwt.cu:1691): the compacted
// records arrive grouped (equal group rank = contiguous, in SA order), so ordering them by (group, next rank) only has to
// reorder each group internally.  One workgroup takes the groups whose head lies in its tile of RS_T records (plus the tail of
// the last one, up to RS_G records past the tile), fetches next = ISA[sa + h] + 1 for them (the gather of the round), and
// ranks every record inside its group by counting (groups are small: 99.9 % of the records of a text block sit in groups of
// <= 1024, three quarters in groups of <= 8; sum of squares ~ 23 comparisons per record).  Output = the same (key, value)
// arrays the radix path produced.  A group longer than RS_G raises `fallback` and the round is redone by the radix engine.
// ---------------------------------------------------------------------------------------------

__global__ __launch_bounds__(WG) void bwt_round_segsort_kernel(const u32* __restrict__ csa, const u32* __restrict__ cgrp, const u32* __restrict__ ISA,
                                                               u32 U, u64 h, u64 n, int lo_bits, u32 smask,
                                                               u64* __restrict__ keys_out, u32* __restrict__ vals_out, u32* __restrict__ fallback,
                                                               u32 skip_long = 0u)
{
    __shared__ u32 snext[RS_E];                  // first the group ranks (for the head flags), then the gathered next ranks
    __shared__ short sgs[RS_E];                  // start of the record's group inside the window, -1: it started before the window
    __shared__ short sge[RS_E];                  // indexed by a group's start: one past its last record
    __shared__ u32 scr[8];
    __shared__ u32 sincl[WG];
    const u32 t = threadIdx.x;
    const u64 base = (u64)blockIdx.x * RS_T;
    const u32 ext = (u32)((base + RS_E <= U) ? (u64)RS_E : (U - base));     // records visible to this workgroup
    const u32 own = ext < (u32)RS_T ? ext : (u32)RS_T;                      // groups whose head is below `own` are ours
    const u32 prevg = (base > 0) ? cgrp[base - 1] : 0xffffffffu;            // group ranks are SA slots < n: never 0xffffffff
    for (u32 i = t; i < ext; i += WG) { snext[i] = cgrp[base + i]; sge[i] = (short)ext; }
    __syncthreads();
    // group start of every record = running maximum of head positions; each thread owns PER consecutive records
    constexpr int PER = RS_E / WG;
    const u32 i0 = t * PER;
    u32 hmask = 0;                               // head flags of this thread's records
    int last_head = -1;
#pragma unroll
    for (int q = 0; q < PER; ++q) {
        const u32 i = i0 + q;
        if (i < ext) { const bool head = (i == 0) ? (snext[0] != prevg) : (snext[i] != snext[i - 1]); if (head) { last_head = (int)i; hmask |= 1u << q; } }
    }
    u32 totmax;
    const u32 incl = block_incl_max((u32)(last_head + 1), scr, &totmax);    // 0 = no head so far
    sincl[t] = incl;
    __syncthreads();
    int run = (t > 0) ? (int)sincl[t - 1] - 1 : -1;
#pragma unroll
    for (int q = 0; q < PER; ++q) {
        const u32 i = i0 + q;
        if (i < ext) {
            if (hmask & (1u << q)) { if (run >= 0) sge[run] = (short)i; run = (int)i; }      // a head closes the group before it
            sgs[i] = (short)run;
        }
    }
    __syncthreads();
    // a group of ours that is still open at the end of the window (and continues behind it) is too long for this kernel.
    // skip_long (hybrid rounds, bwt_longrec_kernel): groups of more than HY_G records are somebody else's — the radix engine sorts them and
    // bwt_longrec_place_kernel puts them into the same output arrays; this kernel leaves their slots alone.  (An open group of ours has
    // its head below `own` and RS_G records of the window behind the tile: more than RS_G >= HY_G records, skipped like any closed one.)
    if (!skip_long && t == 0 && base + ext < U) {
        const int gs = sgs[ext - 1];
        if (gs >= 0 && (u32)gs < own && cgrp[base + ext] == snext[ext - 1]) atomicOr(fallback, 1u);
    }
    __syncthreads();
    // the round's gather, for the records we own (overwrites the group ranks in LDS; they are re-read from memory at the end)
    for (u32 i = t; i < ext; i += WG) {
        const int gs = sgs[i];
        u32 nx = 0;
        if (gs >= 0 && (u32)gs < own && !(skip_long && (u32)sge[gs] - (u32)gs > (u32)HY_G)) {
            const u64 p = (u64)(csa[base + i] & smask) + h;
            nx = (p < n) ? (ISA[p] + 1u) : 0u;
        }
        snext[i] = nx;
    }
    __syncthreads();
    // rank inside the group by counting (ties keep their order), write to the sorted position
    for (u32 i = t; i < ext; i += WG) {
        const int gs = sgs[i];
        if (gs < 0 || (u32)gs >= own) continue;
        const u32 mine = snext[i];
        const u32 ge = (u32)sge[gs];
        if (skip_long && ge - (u32)gs > (u32)HY_G) continue;
        u32 r = 0;
        for (u32 k = (u32)gs; k < ge; ++k) { const u32 o = snext[k]; r += (u32)((o < mine) || (o == mine && k < i)); }
        const u64 dst = base + (u32)gs + r;
        keys_out[dst] = ((u64)cgrp[base + i] << lo_bits) | mine;
        vals_out[dst] = csa[base + i];
    }
}

// ---------------------------------------------------------------------------------------------
// Hybrid doubling round (round 4): groups of more than HY_G records through the radix engine, everything else through the segmented sort.
// Rounds with a group of more than RS_G records used to send ALL unsorted records through seven radix passes on (group rank, next rank) —
// python sources, 64 MiB: 62 M records in the first doubling round, 18 M of them in 3783 such groups; the four rounds that have them cost
// 17.6 of the block's 25 ms (profiles/r04/bwt_rounds_python-source.txt).  The large groups' records are pulled out in order (count / scan
// / write: a stream compaction), keyed by (head index >> 8, next rank) — heads of groups of more than 256 records lie more than 256
// apart, so the shifted head index still tells the groups apart and keeps their order, in 18 bits instead of 26 —, sorted by the radix
// engine and put back: the j-th sorted record belongs into the slot the j-th extracted record came from (same groups, same sizes, same
// order).  The threshold is HY_G, not RS_G: the segmented sort ranks by counting inside the group, and with the first version's 1024
// the rounds of a block of shared objects (many groups of hundreds of records) got slower, not faster.  "More than HY_G" is what
// seg_apply counted for this unsorted set (the record HY_G places behind the head exists), so the host knows the number of extracted
// records without another round trip: dscal[DS_MIDEXCESS] + dscal[DS_NMID] * HY_G.
// ---------------------------------------------------------------------------------------------
constexpr int LR_ITEMS = 16, LR_TILE = WG * LR_ITEMS;
constexpr int LR_HEAD_SHIFT = 8;                                  // 2^8 <= HY_G
static_assert((1 << LR_HEAD_SHIFT) <= HY_G && HY_G <= RS_G, "heads of the extracted groups must differ after the shift; the segmented sort must be able to take the rest");
// i = index among the unsorted records (a group is contiguous there and in SA: head index = i - (SA slot - group rank))
__device__ __forceinline__ bool bwt_rec_is_long(const u32* __restrict__ cgrp, u32 i, u32 pos, u32 grp, u32 U)
{
    const u32 dist = pos - grp;
    if (dist >= (u32)HY_G) return true;
    const u64 far = (u64)(i - dist) + (u64)HY_G;
    return far < (u64)U && cgrp[far] == grp;
}

// WRITE = false: cnt[chunk] = extracted records of the chunk.  WRITE = true: off[chunk] = where the chunk's extracted records go; writes
// their index (lidx), key and suffix.  Lane-strided records (record = tile base + q * WG + t): loads are coalesced, a wavefront's
// extracted records of one q leave to consecutive slots (ballot prefix), and the 16 x 4 (q, wavefront) counts of a tile are scanned in
// LDS.  (The first version gave every thread 16 consecutive records and let it write its own run of slots: 64 lines per store
// instruction and sixteen dependent csa -> ISA loads in a row per thread; a block of shared objects lost 1.4 ms in its first round.)
template <bool WRITE>
__global__ __launch_bounds__(WG) void bwt_longrec_kernel(const u32* __restrict__ cpos, const u32* __restrict__ csa, const u32* __restrict__ cgrp,
                                                         const u32* __restrict__ ISA, u32 U, u64 h, u64 n, int lo_bits, u32 smask,
                                                         u32 chunk_tiles, u32 num_tiles, u32* __restrict__ cnt_or_off,
                                                         u32* __restrict__ lidx, u64* __restrict__ keys, u32* __restrict__ vals)
{
    __shared__ u32 scr[8];
    __shared__ u32 swc[LR_ITEMS * WAVES];            // extracted records per (q, wavefront) of the tile, then their exclusive sums
    __shared__ u32 stot;
    const u32 t = threadIdx.x, lane = t & 63u, wave = t >> 6;
    const u32 tile0 = blockIdx.x * chunk_tiles;
    u32 tile1 = tile0 + chunk_tiles; if (tile1 > num_tiles) tile1 = num_tiles;
    u32 off = WRITE ? cnt_or_off[blockIdx.x] : 0u;
    u32 mine_total = 0;
    for (u32 tile = tile0; tile < tile1; ++tile) {
        const u32 base = tile * (u32)LR_TILE;
        u32 pp[LR_ITEMS], gg[LR_ITEMS];
#pragma unroll
        for (int q = 0; q < LR_ITEMS; ++q) {
            const u32 i = base + (u32)q * WG + t;
            const bool in = i < U;
            pp[q] = in ? cpos[i] : 0u; gg[q] = in ? cgrp[i] : 0u;
        }
        u32 mask = 0, pre[LR_ITEMS];
#pragma unroll
        for (int q = 0; q < LR_ITEMS; ++q) {
            const u32 i = base + (u32)q * WG + t;
            const bool lg = i < U && bwt_rec_is_long(cgrp, i, pp[q], gg[q], U);
            const u64 bal = __ballot(lg);
            if (lg) mask |= 1u << q;
            if (WRITE) {
                pre[q] = (u32)__popcll(bal & ((1ull << lane) - 1ull));
                if (lane == 0) swc[q * WAVES + wave] = (u32)__popcll(bal);
            }
        }
        if (!WRITE) { mine_total += (u32)__popc(mask); continue; }
        __syncthreads();
        if (t < 64) {                                   // LR_ITEMS * WAVES = 64 counts: one wavefront scans them
            const u32 v = swc[t];
            const u32 incl = wave_incl_sum(v);
            swc[t] = incl - v;
            if (t == 63) stot = incl;
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < LR_ITEMS; ++q) {
            if (mask & (1u << q)) {
                const u32 i = base + (u32)q * WG + t;
                const u32 o = off + swc[q * WAVES + wave] + pre[q];
                const u32 s = csa[i];
                const u64 p = (u64)(s & smask) + h;
                const u32 nxt = (p < n) ? (ISA[p] + 1u) : 0u;
                const u32 head = i - (pp[q] - gg[q]);
                keys[o] = ((u64)(head >> LR_HEAD_SHIFT) << lo_bits) | nxt;
                vals[o] = s;
                lidx[o] = i;
            }
        }
        off += stot;
        __syncthreads();                                // swc / stot are rewritten by the next tile
    }
    if (!WRITE) {
        u32 tot;
        (void)block_excl_sum(mine_total, scr, &tot);
        if (t == 0) cnt_or_off[blockIdx.x] = tot;
    }
}

// one workgroup: off[c] = exclusive sum of cnt[0..c); *total = their sum (the host sized the round's radix sort from seg_apply's counts:
// the two numbers are compared after the round, a difference fails the transform instead of leaving a wrong order behind)
__global__ __launch_bounds__(WG) void bwt_longrec_scan_kernel(const u32* __restrict__ cnt, u32 num_chunks, u32* __restrict__ off, u32* __restrict__ total)
{
    __shared__ u32 scr[8];
    u32 carry = 0;
    for (u32 base = 0; base < num_chunks; base += WG) {
        const u32 i = base + threadIdx.x;
        const u32 v = (i < num_chunks) ? cnt[i] : 0u;
        u32 tot;
        const u32 ex = block_excl_sum(v, scr, &tot);
        if (i < num_chunks) off[i] = carry + ex;
        carry += tot;
    }
    if (threadIdx.x == 0) *total = carry;
}

// the j-th sorted long record goes where the j-th extracted one came from, with the key format of the round's other records
__global__ __launch_bounds__(WG) void bwt_longrec_place_kernel(const u64* __restrict__ ks, const u32* __restrict__ vs, const u32* __restrict__ lidx,
                                                               const u32* __restrict__ cgrp, u32 UL, int lo_bits,
                                                               u64* __restrict__ keys_out, u32* __restrict__ vals_out)
{
    const u32 stride = gridDim.x * WG;
    const u64 lomask = (1ull << lo_bits) - 1ull;
    for (u32 j = blockIdx.x * WG + threadIdx.x; j < UL; j += stride) {
        const u32 i = lidx[j];
        keys_out[i] = ((u64)cgrp[i] << lo_bits) | (ks[j] & lomask);
        vals_out[i] = vs[j];
    }
}

// The key of a refinement round on text keys: the packed codes of T[p .. p + a) (zero past the end) and, in the low 4 bits,
// min(n - p, a) — "a proper prefix sorts first" among equal padded keys, 0 for the empty suffix.  lut: byte -> code (LDS or global).
// (two halves so that a caller can have the loads of several records in flight before it packs the first key)
struct TextWin { u32 d[5]; };
__device__ __forceinline__ TextWin bwt_text_window(const u32* __restrict__ T32, u64 p64, u32 n, u32 a = 16)
{
    TextWin w;
    const u32 p = p64 < n ? (u32)p64 : 0u;                // (past the end: any valid address, the key is 0 anyway)
    const u32* q = T32 + (p >> 2);                         // T is 4-byte aligned at T[0] and zero padded for 32 bytes past n
#pragma unroll
    for (int i = 0; i < 4; ++i) w.d[i] = q[i];
    // the fifth word only holds characters 13.. of the window (a <= 12, any text: characters 0..11 + an offset of <= 3 bytes end inside
    // the fourth): one gather in five saved per record; `a` is a kernel argument, the branch is scalar
    w.d[4] = a > 12u ? q[4] : 0u;
    return w;
}
template <class LUT>
__device__ __forceinline__ u64 bwt_text_key_of(const TextWin& w, LUT lut, u64 p64, u32 n, u32 cb, u32 a)
{
    u64 key = 0;
    if (p64 < n) {
        const u32 p = (u32)p64, off = p & 3u;
        const u32 x[4] = { __builtin_amdgcn_alignbyte(w.d[1], w.d[0], off), __builtin_amdgcn_alignbyte(w.d[2], w.d[1], off),
                           __builtin_amdgcn_alignbyte(w.d[3], w.d[2], off), __builtin_amdgcn_alignbyte(w.d[4], w.d[3], off) };
        const u32 left = n - p;                          // characters the suffix has
#pragma unroll
        for (u32 c = 0; c < 15; ++c) {
            if (c < a) {
                const u32 byte = (x[c >> 2] >> (8 * (c & 3))) & 0xffu;
                const u64 code = (c < left) ? (u64)lut[byte] : 0ull;
                key |= code << (64 - cb * (c + 1));
            }
        }
        key |= (u64)(left < a ? left : a);
    }
    return key;
}
template <class LUT>
__device__ __forceinline__ u64 bwt_text_round_key(const u32* __restrict__ T32, LUT lut, u64 p64, u32 n, u32 cb, u32 a)
{
    if (p64 >= n) return 0;
    const TextWin w = bwt_text_window(T32, p64, n, a);
    return bwt_text_key_of(w, lut, p64, n, cb, a);
}

// ---------------------------------------------------------------------------------------------
// A refinement round WITHOUT the inverse suffix array.  Prefix doubling orders the suffixes of a group (equal first h
// characters) by the rank of suffix s + h, which needs ISA — a random 4-byte scatter of n entries after the first sort
// (1.7 ms per 64 MiB block, 5.6 GB of HBM writes for 0.27 GB of payload: the second-largest kernel of the sorter) and a random
// 4-byte gather per unsorted suffix.  But right after the first sort the rank of suffix s + h is just the order of ITS first
// a characters, and those can be read from the text: the round's key is the packed codes of T[s+h .. s+h+a) (zero padded
// past the end) with, in the low 4 bits, min(n - (s+h), a) — "a proper prefix sorts first" among equal padded keys, 0 for the
// empty suffix.  The text is 1/4 of ISA's size and the 16 bytes a record needs are one or two cache lines.  Such a round
// advances the sorted depth by a characters instead of doubling it, so it is used while it pays: text blocks are done after
// two of them (27.8 M unsorted -> 7 155 -> 0 on the bench block) and never build ISA at all; a block that does not converge
// (long repeats) or has a group too long for one workgroup builds ISA once from the current order (bwt_isa_fill / _fix) and
// continues with the doubling rounds below.  Same structure as bwt_round_segsort_kernel; the group rank of a record is not
// part of the output key (cgrp stays valid: records only move inside their group), seg_reduce takes it as a second array.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(WG) void bwt_round_textsort_kernel(const u8* __restrict__ T, const u8* __restrict__ codes,
                                                                const u32* __restrict__ csa, const u32* __restrict__ cgrp,
                                                                u32 U, u64 h, u32 n, u32 smask, u32 cb, u32 a,
                                                                u64* __restrict__ keys_out, u32* __restrict__ vals_out, u32* __restrict__ fallback,
                                                                const u8* __restrict__ subhead = nullptr)
{
    // subhead (optional): extra group boundaries inside long groups that bwt_long_* have split by the first characters of this round's
    // key (see there): a record with subhead[k] != 0 starts a group of its own although its group rank equals its left neighbour's
    __shared__ u64 snext[RS_E];                  // first (as u32) the group ranks for the head flags, then the round keys
    __shared__ short sgs[RS_E];
    __shared__ short sge[RS_E];
    __shared__ u32 scr[8];
    __shared__ u32 sincl[WG];
    __shared__ u8 lut[256];
    u32* sgrp = reinterpret_cast<u32*>(snext);
    const u32 t = threadIdx.x;
    lut[t] = codes[t];
    const u64 base = (u64)blockIdx.x * RS_T;
    const u32 ext = (u32)((base + RS_E <= U) ? (u64)RS_E : (U - base));
    const u32 own = ext < (u32)RS_T ? ext : (u32)RS_T;
    const u32 prevg = (base > 0) ? cgrp[base - 1] : 0xffffffffu;
    for (u32 i = t; i < ext; i += WG) { sgrp[i] = cgrp[base + i]; sge[i] = (short)ext; }
    __syncthreads();
    constexpr int PER = RS_E / WG;
    const u32 i0 = t * PER;
    u32 hmask = 0;
    int last_head = -1;
#pragma unroll
    for (int q = 0; q < PER; ++q) {
        const u32 i = i0 + q;
        if (i < ext) {
            bool head = (i == 0) ? (sgrp[0] != prevg) : (sgrp[i] != sgrp[i - 1]);
            if (subhead != nullptr && subhead[base + i]) head = true;
            if (head) { last_head = (int)i; hmask |= 1u << q; }
        }
    }
    u32 totmax;
    const u32 incl = block_incl_max((u32)(last_head + 1), scr, &totmax);
    sincl[t] = incl;
    __syncthreads();
    int run = (t > 0) ? (int)sincl[t - 1] - 1 : -1;
#pragma unroll
    for (int q = 0; q < PER; ++q) {
        const u32 i = i0 + q;
        if (i < ext) {
            if (hmask & (1u << q)) { if (run >= 0) sge[run] = (short)i; run = (int)i; }
            sgs[i] = (short)run;
        }
    }
    __syncthreads();
    if (t == 0 && base + ext < U) {
        const int gs = sgs[ext - 1];
        if (gs >= 0 && (u32)gs < own && cgrp[base + ext] == sgrp[ext - 1] && !(subhead != nullptr && subhead[base + ext])) atomicOr(fallback, 1u);
    }
    __syncthreads();
    // the round's keys, from the text (overwrites the group ranks in LDS)
    const u32* T32 = reinterpret_cast<const u32*>(T);
    // (issuing the text loads of four records at a time — 20 loads in flight per lane — was measured: 1.02 ms against 1.00, no gain; the
    // kernel waits on the gathers' sector traffic, 2 GB for 28 M records, not on their latency)
    for (u32 i = t; i < ext; i += WG) {
        const int gs = sgs[i];
        u64 key = 0;
        if (gs >= 0 && (u32)gs < own) key = bwt_text_round_key(T32, lut, (u64)(csa[base + i] & smask) + h, n, cb, a);
        snext[i] = key;
    }
    __syncthreads();
    for (u32 i = t; i < ext; i += WG) {
        const int gs = sgs[i];
        if (gs < 0 || (u32)gs >= own) continue;
        const u64 mine = snext[i];
        const u32 ge = (u32)sge[gs];
        u32 r = 0;
        for (u32 k = (u32)gs; k < ge; ++k) { const u64 o = snext[k]; r += (u32)((o < mine) || (o == mine && k < i)); }
        const u64 dst = base + (u32)gs + r;
        keys_out[dst] = mine;
        vals_out[dst] = csa[base + i];
    }
}

// ---------------------------------------------------------------------------------------------
// Groups longer than one workgroup sorts (RS_G records).  cub::DeviceSegmentedSort (libcubwt.cu:1691) takes segments of any
// length; bwt_round_textsort_kernel does not, and used to hand the WHOLE round over to prefix doubling as soon as one such group
// existed (w = 11 characters on the bench text: 318 long groups, BWT 6.7 -> 14.3 ms).  Now the long groups — and only they — are
// first split by the top LG_BITS bits of this round's key (the first two characters of a text) with a counting sort per group:
//   bwt_long_heads    every record knows where its group starts (its SA slot minus its group rank) and whether the group is long
//                     (the record RS_G places behind the head still has the head's rank); heads of long groups draw a dense id
//   bwt_long_count    histogram of the key's top bits per long group (global atomics: the long groups' records are few)
//   bwt_long_scan     one workgroup per long group: exclusive scan of its 1024 counts, sub-group heads marked at bucket starts
//   bwt_long_scatter  records of long groups move to their bucket (any order inside a bucket: they are about to be sorted by
//                     the full key), all others are copied through
// and the round's segmented sort runs again with the bucket starts as additional group boundaries.  Buckets are almost always short
// enough; if one is not (a long repeat: thousands of suffixes that agree far beyond the key), or there are more than LG_MAX long
// groups, the round is handed over to prefix doubling as before — the right tool for that shape.
// ---------------------------------------------------------------------------------------------
constexpr u32 LG_BITS = 10, LG_BUCKETS = 1u << LG_BITS, LG_MAX = 4096;
struct LongTables { u32* nlong; u32* khead; u32* cnt; };        // [1], [LG_MAX], [LG_MAX][LG_BUCKETS]

__device__ __forceinline__ bool bwt_group_is_long(const u32* __restrict__ cpos, const u32* __restrict__ cgrp, u32 U, u32 k, u32* kh_out)
{
    const u32 g = cgrp[k], kh = k - (cpos[k] - g);                                  // members of a group are contiguous, in SA order
    *kh_out = kh;
    return kh + (u32)RS_G < U && cgrp[kh + RS_G] == g;
}

__global__ __launch_bounds__(WG) void bwt_long_heads_kernel(const u32* __restrict__ cpos, const u32* __restrict__ cgrp, u32 U, LongTables L, u32* __restrict__ lgid)
{
    // heads of long groups draw a dense id (one atomic per long group; how many long groups and records there are the host already knows
    // from seg_apply — a count per wavefront here was 285 K atomics on one address, 3.3 ms on a block with 18 M such records)
    const u32 stride = gridDim.x * WG;
    for (u32 k = blockIdx.x * WG + threadIdx.x; k < U; k += stride) {
        u32 kh = 0;
        if (bwt_group_is_long(cpos, cgrp, U, k, &kh) && kh == k) {
            const u32 id = atomicAdd(L.nlong, 1u);
            lgid[k] = id;
            if (id < LG_MAX) L.khead[id] = k;
        }
    }
}
// The split pays only while the long groups hold a small part of the round's records: their records go through global atomics
// (counting sort per group), and on inputs with long repeats — where most unsorted suffixes sit in a few huge groups — that costs
// far more than the hand-over to prefix doubling it tries to avoid (python sources, 64 MiB: 127 ms against 44 ms).
__device__ __forceinline__ bool bwt_long_split_pays(const LongTables& L, u32 U) { (void)U; return L.nlong[0] != 0u && L.nlong[0] <= LG_MAX; }     // (the host decides; this only guards the tables)

__global__ __launch_bounds__(WG) void bwt_long_count_kernel(const u8* __restrict__ T, const u8* __restrict__ codes, const u32* __restrict__ csa,
                                                            const u32* __restrict__ cpos, const u32* __restrict__ cgrp, u32 U, u64 h, u32 n, u32 smask, u32 cb, u32 a,
                                                            LongTables L, const u32* __restrict__ lgid)
{
    if (!bwt_long_split_pays(L, U)) return;
    const u32* T32 = reinterpret_cast<const u32*>(T);
    const u32 stride = gridDim.x * WG;
    for (u32 k = blockIdx.x * WG + threadIdx.x; k < U; k += stride) {
        u32 kh;
        if (!bwt_group_is_long(cpos, cgrp, U, k, &kh)) continue;
        const u64 key = bwt_text_round_key(T32, codes, (u64)(csa[k] & smask) + h, n, cb, a);
        atomicAdd(&L.cnt[(size_t)lgid[kh] * LG_BUCKETS + (u32)(key >> (64 - LG_BITS))], 1u);
    }
}

__global__ __launch_bounds__(WG) void bwt_long_scan_kernel(LongTables L, u32 U, u8* __restrict__ subhead)
{
    __shared__ u32 scr[8];
    const u32 nl = *L.nlong;
    if (!bwt_long_split_pays(L, U) || blockIdx.x >= nl) return;
    u32* row = L.cnt + (size_t)blockIdx.x * LG_BUCKETS;
    const u32 kh = L.khead[blockIdx.x];
    u32 c[LG_BUCKETS / WG], sum = 0;
#pragma unroll
    for (u32 q = 0; q < LG_BUCKETS / WG; ++q) { c[q] = row[threadIdx.x * (LG_BUCKETS / WG) + q]; sum += c[q]; }
    u32 tot;
    u32 run = block_excl_sum(sum, scr, &tot);
#pragma unroll
    for (u32 q = 0; q < LG_BUCKETS / WG; ++q) {
        row[threadIdx.x * (LG_BUCKETS / WG) + q] = run;                           // becomes the bucket's cursor
        if (c[q]) subhead[kh + run] = 1;
        run += c[q];
    }
}

__global__ __launch_bounds__(WG) void bwt_long_scatter_kernel(const u8* __restrict__ T, const u8* __restrict__ codes, const u32* __restrict__ csa,
                                                              const u32* __restrict__ cpos, const u32* __restrict__ cgrp, u32 U, u64 h, u32 n, u32 smask, u32 cb, u32 a,
                                                              LongTables L, const u32* __restrict__ lgid, u32* __restrict__ csa_out)
{
    if (!bwt_long_split_pays(L, U)) return;
    const u32* T32 = reinterpret_cast<const u32*>(T);
    const u32 stride = gridDim.x * WG;
    for (u32 k = blockIdx.x * WG + threadIdx.x; k < U; k += stride) {
        u32 kh;
        const u32 s = csa[k];
        if (!bwt_group_is_long(cpos, cgrp, U, k, &kh)) { csa_out[k] = s; continue; }
        const u64 key = bwt_text_round_key(T32, codes, (u64)(s & smask) + h, n, cb, a);
        const u32 slot = atomicAdd(&L.cnt[(size_t)lgid[kh] * LG_BUCKETS + (u32)(key >> (64 - LG_BITS))], 1u);
        csa_out[kh + slot] = s;
    }
}

// ISA from the current order (when the text rounds hand over to prefix doubling): every suffix gets its SA slot, then the
// still unsorted ones the rank of their group (the slot of the group's head).
// (uns: the first seg's flags, while they are still there — a slot whose suffix is unsorted is left to bwt_isa_fix_kernel instead of being
// stored twice: with long repeats nearly every slot, and a random 4-byte store costs a whole line of HBM traffic)
__global__ __launch_bounds__(WG) void bwt_isa_fill_kernel(const u32* __restrict__ SA, u32 n, u32 smask, u32* __restrict__ ISA, const u8* __restrict__ uns)
{
    const u32 stride = gridDim.x * WG;
    for (u32 x = blockIdx.x * WG + threadIdx.x; x < n; x += stride) {
        if (uns != nullptr && (uns[x] & 2u)) continue;
        ISA[SA[x] & smask] = x;
    }
}
__global__ __launch_bounds__(WG) void bwt_isa_fix_kernel(const u32* __restrict__ csa, const u32* __restrict__ cgrp, u32 U, u32 smask, u32* __restrict__ ISA)
{
    const u32 stride = gridDim.x * WG;
    for (u32 k = blockIdx.x * WG + threadIdx.x; k < U; k += stride) ISA[csa[k] & smask] = cgrp[k];
}

// Primary index and aux indexes straight from SA (no ISA needed): dscal[DS_PRIMARY] = j + 1 where SA[j] = 0,
// dscal[DS_AUX + t] = j + 1 where SA[j] = t * r (libsais_bwt_aux semantics: I[t] = ISA[t * r] + 1).
__global__ __launch_bounds__(WG) void bwt_find_kernel(const u32* __restrict__ SA, u32 n, u32 smask, u32 rmask, u32 rshift, u32 cnt, u32* __restrict__ dscal)
{
    const u32 j0 = 4u * (blockIdx.x * WG + threadIdx.x);
    if (j0 >= n) return;
    u32 sv[4];
    if (j0 + 4 <= n) { const uint4 q = *reinterpret_cast<const uint4*>(SA + j0); sv[0] = q.x; sv[1] = q.y; sv[2] = q.z; sv[3] = q.w; }
    else { for (u32 q = 0; q < 4; ++q) sv[q] = (j0 + q < n) ? SA[j0 + q] : 0xffffffffu; }
#pragma unroll
    for (u32 q = 0; q < 4; ++q) {
        if (j0 + q >= n) continue;
        const u32 sfx = sv[q] & smask;
        if (sfx == 0) dscal[DS_PRIMARY] = j0 + q + 1;
        if (cnt != 0 && (sfx & rmask) == 0 && (sfx >> rshift) < cnt) dscal[DS_AUX + (sfx >> rshift)] = j0 + q + 1;
    }
}

// ---------------------------------------------------------------------------------------------
// L[0] = T[n-1]; L[o] = T[SA[j]-1] with j = o-1 for o <= ISA[0], j = o for o > ISA[0].
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(WG) void bwt_emit_kernel(const u8* __restrict__ T, const u32* __restrict__ SA,
                                                      u32 n, u8* __restrict__ L, const u32* __restrict__ dscal)
{
    const u32 o0 = 4u * (blockIdx.x * WG + threadIdx.x);
    if (o0 >= n) return;
    const u32 p = dscal[DS_PRIMARY] - 1;                  // ISA[0], from bwt_find_kernel
    u32 word = 0;
#pragma unroll
    for (u32 q = 0; q < 4; ++q) {
        const u32 o = o0 + q;
        u32 byte = 0;
        if (o < n) {
            if (o == 0) byte = T[n - 1];
            else {
                const u32 j = (o <= p) ? (o - 1) : o;
                byte = T[SA[j] - 1];
            }
        }
        word |= byte << (8 * q);
    }
    if (o0 + 4 <= n) *reinterpret_cast<u32*>(L + o0) = word;
    else for (u32 q = 0; o0 + q < n; ++q) L[o0 + q] = (u8)(word >> (8 * q));
}

// The same from values that carry the predecessor's code (SA[j] = index | code(T[index-1]) << pred_shift): no access to T at
// all, SA is read in order.  decode[code] = byte.
__global__ __launch_bounds__(WG) void bwt_emit_pred_kernel(const u8* __restrict__ T, const u32* __restrict__ SA, u32 n,
                                                           u32 pred_shift, const u8* __restrict__ decode, u8* __restrict__ L, const u32* __restrict__ dscal)
{
    __shared__ u8 dec[256];
    dec[threadIdx.x] = decode[threadIdx.x];
    __syncthreads();
    const u32 o0 = 4u * (blockIdx.x * WG + threadIdx.x);
    if (o0 >= n) return;
    const u32 p = dscal[DS_PRIMARY] - 1;                  // ISA[0], from bwt_find_kernel
    u32 word = 0;
#pragma unroll
    for (u32 q = 0; q < 4; ++q) {
        const u32 o = o0 + q;
        u32 byte = 0;
        if (o < n) {
            if (o == 0) byte = T[n - 1];
            else { const u32 j = (o <= p) ? (o - 1) : o; byte = dec[SA[j] >> pred_shift]; }
        }
        word |= byte << (8 * q);
    }
    if (o0 + 4 <= n) *reinterpret_cast<u32*>(L + o0) = word;
    else for (u32 q = 0; o0 + q < n; ++q) L[o0 + q] = (u8)(word >> (8 * q));
}

// ---------------------------------------------------------------------------------------------
// Batched pass: many blocks back to back in one suffix sort (bwt_batch_device).  The block table `off` (count + 1 offsets) lives in a
// small device array; a position finds its block by a binary search in it.  Block-major order is DESCENDING: block count - 1 takes the
// lowest SA slots, block 0 the highest (block b: slots [N - off[b+1], N - off[b])).  The first-sort key carries count - 1 - b in its top
// bits and the dense codes + 1 below (0 = past the block's own end: "shorter, hence smaller", no tail trick needed).  The doubling rounds
// then need no block table at all: for a suffix s of block b, s + h past the block's end lies in a later block, whose ranks are all
// below block b's slots, so next = ISA[s + h] + 1 orders it before every same-block next rank — exactly what 0 does at the block end.
// (Only one suffix per group can reach the end: the members of a group share h characters and differ in length.)
// (batch_block_of: dev_common.h)
__global__ __launch_bounds__(WG) void bwt_batch_pack_kernel(const u8* __restrict__ T, u32 N, const u32* __restrict__ off, u32 count,
                                                            u32 bb, u32 cb, u32 w, const u8* __restrict__ codes,
                                                            u64* __restrict__ keys, u32* __restrict__ vals)
{
    __shared__ u8 lut[256];
    lut[threadIdx.x] = codes[threadIdx.x];
    __syncthreads();
    const u32 i = blockIdx.x * WG + threadIdx.x;
    if (i >= N) return;
    const u32 b = batch_block_of(off, count, i), end = off[b + 1];
    u64 key = bb ? (u64)(count - 1 - b) << (64 - bb) : 0ull;
#pragma unroll
    for (u32 t = 0; t < 16; ++t) {
        if (t < w) {
            const u32 p = i + t;
            const u64 cd = (p < end) ? (u64)lut[T[p]] + 1ull : 0ull;
            key |= cd << (64 - bb - cb * (t + 1));
        }
    }
    keys[i] = key;
    vals[i] = i;
}

// per block: I[t] = (row of suffix off_b + t * r_b inside the block) + 1, from the final ISA (slots)
__global__ __launch_bounds__(WG) void bwt_batch_find_kernel(const u32* __restrict__ ISA, u32 N, const u32* __restrict__ off,
                                                            const int* __restrict__ rate, u32 count, u32* __restrict__ res)
{
    const u32 b = blockIdx.x * WG + threadIdx.x;
    if (b >= count) return;
    const u32 o0 = off[b], end = off[b + 1], nb = end - o0;
    const int r = rate[b];
    if (nb == 0 || r < 0) return;
    const u32 base = N - end;
    res[16u * b] = ISA[o0] - base + 1u;
    if (r > 0) {
        u32 cnt = (nb - 1u) / (u32)r + 1u; if (cnt > 16u) cnt = 16u;
        for (u32 t = 1; t < cnt; ++t) res[16u * b + t] = ISA[o0 + t * (u32)r] - base + 1u;
    }
}

// L of block b at the block's own place: L[0] = T[end - 1]; L[j] = T[SA[base + row] - 1], row = j - 1 up to the primary row, j after it
__global__ __launch_bounds__(WG) void bwt_batch_emit_kernel(const u8* __restrict__ T, const u32* __restrict__ SA, const u32* __restrict__ ISA,
                                                            u32 N, const u32* __restrict__ off, const int* __restrict__ rate, u32 count,
                                                            u8* __restrict__ L)
{
    const u32 o = blockIdx.x * WG + threadIdx.x;
    if (o >= N) return;
    const u32 b = batch_block_of(off, count, o), o0 = off[b], end = off[b + 1];
    if (rate[b] < 0) { L[o] = T[o]; return; }
    const u32 base = N - end, p = ISA[o0] - base, j = o - o0;
    u8 byte;
    if (j == 0) byte = T[end - 1];
    else byte = T[SA[base + ((j <= p) ? j - 1 : j)] - 1u];
    L[o] = byte;
}

struct BwtBatch { u32 count; const u32* off; const int* rate; u32* res; u32* res_host; };

void launch_seg_scan(bscgpu_ctx* c, u32 num_chunks)
{
    hipLaunchKernelGGL(seg_scan_kernel, dim3(1), dim3(WG), 0, c->stream, c->segsum, num_chunks, c->segoff, c->dscal);
}

// ---------------------------------------------------------------------------------------------
// The driver.  What it decides — key layout, digit passes, the kind of every round — is bwt_plan.h's arithmetic; here are the launches.
// ---------------------------------------------------------------------------------------------
// The driver's environment switches, read once per process (bwt_plan.h: BwtSwitches says what each does).
static const BwtSwitches& bwt_switches()
{
    static const BwtSwitches sw = [] {
        auto env = [](const char* name, int dflt) { const char* e = getenv(name); return e ? atoi(e) : dflt; };
        return BwtSwitches{env("BSC_BWT_W", 0), env("BSC_BWT_TEXTROUNDS", 1), env("BSC_BWT_HYBRID", 1), env("BSC_BWT_HYBRID_PCT", 100), env("BSC_BWT_ISASKIP", 1)};
    }();
    return sw;
}

// workgroups of a grid-stride kernel over x items
static inline u32 capped_grid(u32 x, u32 cap = 8192) { const u32 blocks = (x + WG - 1) / WG; return blocks > cap ? cap : blocks; }

template <bool INITIAL, bool WRITE_ISA>
static int run_seg(bscgpu_ctx* c, const u64* keys, const u32* sa_sorted, const u32* cpos_in, u32 m, u32 tail_lo, u32 smask,
                   u32* cpos_out, u32* csa_out, u32* cgrp_out, u32* U_out, u32* SA, const u32* grp_in = nullptr, int grp_shift = 0)
{
    const Chunking ch = make_chunking(m, SEG_TILE);
    prof_begin(c, BSCGPU_K_SEG, (u64)m * (8 + (INITIAL ? 4 : 0) + 1), m);
    hipLaunchKernelGGL(seg_reduce_kernel<INITIAL>, dim3(ch.num_chunks), dim3(WG), 0, c->stream,
                       keys, sa_sorted, m, tail_lo, smask, ch.chunk_tiles, ch.num_tiles, c->flags, c->segsum, grp_in, grp_shift);
    prof_end(c);
    prof_begin(c, BSCGPU_K_SEG, 0, 0);
    hipLaunchKernelGGL(seg_scan_kernel, dim3(1), dim3(WG), 0, c->stream, c->segsum, ch.num_chunks, c->segoff, c->dscal);
    prof_end(c);
    prof_begin(c, BSCGPU_K_SEG, (u64)m * (1 + 4 + (INITIAL ? 0 : 4) + 4 + 4), m);
    hipLaunchKernelGGL((seg_apply_kernel<INITIAL, WRITE_ISA>), dim3(ch.num_chunks), dim3(WG), 0, c->stream,
                       c->flags, sa_sorted, cpos_in, m, smask, ch.chunk_tiles, ch.num_tiles, c->segoff,
                       SA, c->ISA, cpos_out, csa_out, cgrp_out, c->dscal);
    prof_end(c);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(c->hscal, c->dscal, DS_ROUND_WORDS * 4, hipMemcpyDeviceToHost, c->stream));  // U, (slots of other kernels), group counts, a hybrid round's extracted records
    HIP_TRY(c, ctx_sync(c));
    prof_collect(c);
    *U_out = c->hscal[DS_TOTAL];
    return radix_onesweep_check(c);            // the sort in front of this seg, if it used the single-read passes
}

static int bwt_device_once(bscgpu_ctx* c, const u8* dT_user, u8* dL_user, int64_t n64, int64_t r, u32* I_host, int64_t* primary_out,
                           const BwtBatch* bt = nullptr);

// Retry rule: with_onesweep_retry (dev_common.h); the second attempt copies the text again, as the first.
int bwt_device(bscgpu_ctx* c, const u8* dT_user, u8* dL_user, int64_t n64, int64_t r, u32* I_host, int64_t* primary_out)
{
    return with_onesweep_retry(c, [&](bool) { return bwt_device_once(c, dT_user, dL_user, n64, r, I_host, primary_out); });
}

// One batched pass (see bwt_batch_pack_kernel): the block table goes up, one transform of the whole pass runs, the per-block indexes come
// back with the pass's last sync.  Same retry rule as bwt_device.
int batch_tab_ensure(bscgpu_ctx* c)
{
    constexpr size_t TAB_WORDS = (size_t)(BATCH_MAX_BLOCKS + 1) + BATCH_MAX_BLOCKS + 16 * (size_t)BATCH_MAX_BLOCKS + BATCH_MAX_BLOCKS;   // offsets, rates, indexes, checksums
    if (!c->batch_tab && hipMalloc((void**)&c->batch_tab, TAB_WORDS * 4) != hipSuccess) {
        (void)hipGetLastError(); c->batch_tab = nullptr;
        return ctx_fail(c, BSC_GPU_NOT_ENOUGH_MEMORY, "batched BWT: block table", hipSuccess);
    }
    c->batch_bytes = TAB_WORDS * 4;
    return BSC_NO_ERROR;
}

int batch_pass_setup(bscgpu_ctx* c, const u8* dT_user, const int* sizes, int count, const int* rates, int* index_out, u32* adler_host, BatchTab* bt)
{
    if (count <= 0 || count > BATCH_MAX_BLOCKS) return BSC_BAD_PARAMETER;
    RC_TRY(batch_tab_ensure(c));
    std::vector<u32> tab((size_t)2 * count + 1, 0u);
    u64 total = 0;
    for (int b = 0; b < count; ++b) { tab[b] = (u32)total; total += (u64)sizes[b]; if (index_out) index_out[b] = 0; }
    tab[count] = (u32)total;
    if (rates) memcpy(&tab[count + 1], rates, (size_t)count * 4);
    bt->total = 0;
    if (total == 0) return BSC_NO_ERROR;
    if (total > (u64)c->max_n || total >= 0x7fffffffull) return BSC_BAD_PARAMETER;
    bt->total = (u32)total; bt->off = c->batch_tab; bt->rate = reinterpret_cast<const int*>(c->batch_tab + count + 1);
    bt->res = c->batch_tab + 2 * BATCH_MAX_BLOCKS + 1;
    HIP_TRY(c, hipMemcpyAsync(c->batch_tab, tab.data(), tab.size() * 4, hipMemcpyHostToDevice, c->stream));
    if (adler_host) {                           // (reads the caller's text before the transform may overwrite it; the transform's last sync covers the copy)
        u32* dadler = c->batch_tab + 18 * BATCH_MAX_BLOCKS + 1;
        launch_adler_batch(c, dT_user, c->batch_tab, (u32)count, dadler);
        HIP_TRY(c, hipMemcpyAsync(adler_host, dadler, (size_t)count * 4, hipMemcpyDeviceToHost, c->stream));
    }
    return BSC_NO_ERROR;
}

int bwt_batch_device(bscgpu_ctx* c, const u8* dT_user, u8* dL_user, const int* sizes, int count, const int* rates, u32* res, u32* adler_host)
{
    BatchTab tab;
    const int src = batch_pass_setup(c, dT_user, sizes, count, rates, nullptr, adler_host, &tab);
    if (src < 0 || tab.total == 0) return src;
    const BwtBatch bt = {(u32)count, tab.off, tab.rate, tab.res, res};
    int64_t unused = 0;
    return with_onesweep_retry(c, [&](bool) { return bwt_device_once(c, dT_user, dL_user, (int64_t)tab.total, 0, nullptr, &unused, &bt); });
}

// The front of a transform: private copy of the text, alphabet, key packing and the first sort (asynchronous behind the alphabet's sync;
// run_seg checks the sort).  Also what bscgpu_bwt_first_sort_device runs.
struct FirstSort { BwtKeyPlan kp; PackParams pp; u8* dcodes; u8* ddecode; const u64* ks; const u32* vs; };
static int bwt_first_sort(bscgpu_ctx* c, const u8* dT_user, u32 n, const BwtBatch* bt, FirstSort* fs)
{
    // private, padded copy of the text (emit may overwrite the user's buffer when dL aliases dT)
    HIP_TRY(c, hipMemcpyAsync(c->dT, dT_user, n, hipMemcpyDeviceToDevice, c->stream));
    HIP_TRY(c, hipMemsetAsync(c->dT + n, 0, 32, c->stream));

    // alphabet: byte histogram -> dense order-preserving codes
    HIP_TRY(c, hipMemsetAsync(c->dscal + DS_BYTEHIST, 0, DS_BYTEHIST_LEN * 4, c->stream));
    {
        const Chunking hc = make_chunking(n, 16 * WG * 16);
        prof_begin(c, BSCGPU_K_MISC, n, 0);
        hipLaunchKernelGGL(bwt_bytehist_kernel, dim3(hc.num_chunks), dim3(WG), 0, c->stream, c->dT, n, hc.chunk_tiles * 16u * WG * 16u, c->dscal + DS_BYTEHIST);
        prof_end(c);
    }
    HIP_TRY(c, hipMemcpyAsync(c->hscal + DS_BYTEHIST, c->dscal + DS_BYTEHIST, DS_BYTEHIST_LEN * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, ctx_sync(c));
    u8 codes[256]; u32 K = 0;
    for (int b = 0; b < 256; ++b) { codes[b] = (u8)K; if (c->hscal[DS_BYTEHIST + b]) ++K; }
    // key layout and pass plan (bwt_plan.h); the single-read passes are asked about the fold's pass count, which does not depend on the answer
    const u32 count = bt ? bt->count : 0u;
    const int wmax = bwt_switches().wmax, fold_np = bwt_key_plan(K, n, count, wmax, false).fold_np;
    const BwtKeyPlan& kp = fs->kp = bwt_key_plan(K, n, count, wmax, c->bwt_fold != 0 && radix_onesweep_wanted(c, n, fold_np, true));
    PackParams& pp = fs->pp;
    pp.cb = kp.cb; pp.w = kp.w; pp.tc = kp.tc; pp.low_shift = kp.low_shift; pp.pred_shift = kp.pred_shift;
    u8* dcodes = fs->dcodes = reinterpret_cast<u8*>(c->dscal + DS_CODES);
    u8* ddecode = fs->ddecode = reinterpret_cast<u8*>(c->dscal + DS_DECODE);
    u8 decode[256]; memset(decode, 0, sizeof decode);
    for (int b = 255; b >= 0; --b) if (c->hscal[DS_BYTEHIST + b]) decode[codes[b]] = (u8)b;
    HIP_TRY(c, hipMemcpyAsync(dcodes, codes, 256, hipMemcpyHostToDevice, c->stream));
    if (pp.pred_shift) HIP_TRY(c, hipMemcpyAsync(ddecode, decode, 256, hipMemcpyHostToDevice, c->stream));
    if (kp.fold) {
        const u32 fold_r = kp.fold_r;
        const bool fused = c->bwt_fold == 1;                // packing counts the byte digits too (else rs_hist_all reads the keys for them)
        if (!c->fold_lds_set) {
            HIP_TRY(c, hipFuncSetAttribute((const void*)bwt_pack_fold_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)fold_lds_bytes(FOLD_MAXP)));
            c->fold_lds_set = true;
        }
        u32* totals = nullptr; u32 stride = 0;
        if (fused) RC_TRY(radix_onesweep_prepare(c, n, fold_np, &totals, &stride));     // (the tables are cleared in front of packing)
        const u32 ntiles = (n + FOLD_TILE - 1) / FOLD_TILE;
        u32* fcnt = c->ISA;                                  // [FOLD_NB][ntiles] counts, then as many offsets: ISA is not built before the first seg
        u32* foff = fcnt + (size_t)FOLD_NB * ntiles;
        u32* fseg = foff + (((size_t)FOLD_NB * ntiles + 3) & ~(size_t)3);     // [FOLD_NB][FOLD_SEGS] records of a bucket per scan segment
        const u32 seg_tiles = (ntiles + FOLD_SEGS - 1) / FOLD_SEGS;
        // an odd number of passes ends in the other pair: the records are packed into the pair from which the sort lands in kA / vA,
        // so that SA can alias vA and the text rounds keep kB / vB
        u64* k0 = (fold_np & 1) ? c->kB : c->kA; u64* k1 = (fold_np & 1) ? c->kA : c->kB;
        u32* v0 = (fold_np & 1) ? c->vB : c->vA; u32* v1 = (fold_np & 1) ? c->vA : c->vB;
        const u32 resident = (u32)c->num_cus * (u32)FOLD_WGS_PER_CU;
        const u32 grid = ntiles < resident ? ntiles : resident;
        prof_begin(c, BSCGPU_K_PACK, (u64)n * 14, n);
        hipLaunchKernelGGL(bwt_fold_count_kernel, dim3((ntiles + FOLD_WAVES - 1) / FOLD_WAVES), dim3(WG), 0, c->stream,
                           c->dT, n, pp.w, (1u << fold_r) - 1u, dcodes, ntiles, fcnt);
        hipLaunchKernelGGL(bwt_fold_scan_kernel, dim3(FOLD_SEGS, FOLD_NB), dim3(WG), 0, c->stream, fcnt, ntiles, seg_tiles, foff, fseg);
        if (fused)
            hipLaunchKernelGGL(bwt_pack_fold_kernel<true>, dim3(grid), dim3(WG), fold_lds_bytes((u32)fold_np), c->stream,
                               c->dT, n, pp, fold_r, dcodes, foff, fseg, ntiles, seg_tiles, k0, v0, (u32)fold_np, totals, stride);
        else
            hipLaunchKernelGGL(bwt_pack_fold_kernel<false>, dim3(grid), dim3(WG), 0, c->stream,
                               c->dT, n, pp, fold_r, dcodes, foff, fseg, ntiles, seg_tiles, k0, v0, 0u, (u32*)nullptr, 0u);
        prof_end(c);
        HIP_TRY(c, hipGetLastError());
        RC_TRY(radix_onesweep_sort(c, k0, k1, v0, v1, n, kp.passes, kp.npass, fused));
        ++c->cnt_bwt_folded;
        fs->ks = c->kA; fs->vs = c->vA;
        return BSC_NO_ERROR;
    }
    prof_begin(c, BSCGPU_K_PACK, (u64)n * 13, n);
    if (bt)
        hipLaunchKernelGGL(bwt_batch_pack_kernel, dim3((n + WG - 1) / WG), dim3(WG), 0, c->stream,
                           c->dT, n, bt->off, bt->count, kp.batch_bb, pp.cb, pp.w, dcodes, c->kA, c->vA);
    else
        hipLaunchKernelGGL(bwt_pack_kernel, dim3((n + 4 * WG - 1) / (4 * WG)), dim3(WG), 0, c->stream,
                           c->dT, n, pp, dcodes, c->kA, c->vA);
    prof_end(c);

    int in_alt = 0;
    RC_TRY(radix_sort_passes(c, c->kA, c->kB, c->vA, c->vB, n, kp.passes, kp.npass, &in_alt));
    fs->ks = in_alt ? c->kB : c->kA;
    fs->vs = in_alt ? c->vB : c->vA;
    return BSC_NO_ERROR;
}

// The first sort alone (bscgpu_bwt_first_sort_device): alphabet, packing and the sort as a transform of this block runs them, the sorted
// (key, value) arrays copied out.  Same retry rule as bwt_device.
int bwt_first_sort_device(bscgpu_ctx* c, const u8* dT_user, int64_t n64, u64* keys_out, u32* vals_out)
{
    if (n64 < 0 || n64 > c->max_n || n64 >= 0x7fffffffll) return BSC_BAD_PARAMETER;
    if (n64 == 0) return BSC_NO_ERROR;
    const u32 n = (u32)n64;
    return with_onesweep_retry(c, [&](bool) -> int {
        FirstSort fs;
        RC_TRY(bwt_first_sort(c, dT_user, n, nullptr, &fs));
        HIP_TRY(c, hipMemcpyAsync(keys_out, fs.ks, (size_t)n * 8, hipMemcpyDeviceToDevice, c->stream));
        HIP_TRY(c, hipMemcpyAsync(vals_out, fs.vs, (size_t)n * 4, hipMemcpyDeviceToDevice, c->stream));
        HIP_TRY(c, ctx_sync(c));
        prof_collect(c);
        return radix_onesweep_check(c);
    });
}

// ---------------------------------------------------------------------------------------------
// The refinement rounds.  What they share:
struct BwtRounds {
    // fixed for the transform
    u32 n; PackParams pp; u32 smask, ta; u8* dcodes;
    int lo_bits;                // next-rank field: values 0 .. n
    // moved by the rounds
    int cur;                    // the half of cpos / csa / cgrp that holds the unsorted set
    u32 U;                      // its records
    u64 h;                      // characters the groups are sorted by
    u32* SA;                    // the sort's value array itself when the rounds do not write to it (they put their output into kB / vB), else a copy
    bool isa_valid;             // ISA exists: the rounds double; else they are rounds on text keys
    bool first_flags;           // c->flags still holds the first seg's flags, indexed by SA slot (bit 1: the slot's suffix is unsorted)
    const u64* ks; const u32* vs; int in_alt;       // where the last sort left its records
    int rounds, text_rounds;
    // debug trace only: wall time of a round (every round ends in a sync)
    bool dbg; double t_round;
};

static double bwt_now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
static double bwt_lap(BwtRounds& s) { const double t = bwt_now_ms(), d = t - s.t_round; s.t_round = t; return d; }

// A round's sort gives up when a group does not fit a workgroup: the word is cleared in front of the launches, read behind them
static int bwt_giveup_clear(bscgpu_ctx* c) { HIP_TRY(c, hipMemsetAsync(c->dscal + DS_GIVEUP, 0, 4, c->stream)); return BSC_NO_ERROR; }
static int bwt_giveup_read(bscgpu_ctx* c, bool* sorted)
{
    HIP_TRY(c, hipMemcpyAsync(c->hscal + DS_GIVEUP, c->dscal + DS_GIVEUP, 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, ctx_sync(c));
    prof_collect(c);
    *sorted = c->hscal[DS_GIVEUP] == 0;
    return BSC_NO_ERROR;
}

// The radix engine is about to use vA: SA moves to its own buffer
static int bwt_sa_to_own_buffer(bscgpu_ctx* c, BwtRounds& s)
{
    if (s.SA == c->vA) {
        const u32 n = s.n;
        HIP_TRY(c, hipMemcpyAsync(c->SA, c->vA, (size_t)n * 4, hipMemcpyDeviceToDevice, c->stream));
        s.SA = c->SA;
    }
    return BSC_NO_ERROR;
}

// The sort of a round on text keys and its verdict, output in kB / vB.  csa: the round's suffixes; subhead: extra group boundaries or
// null.  The caller has cleared the give-up word and opened the profile bracket.
static int bwt_textsort(bscgpu_ctx* c, BwtRounds& s, const u32* csa, const u8* subhead, bool* sorted)
{
    hipLaunchKernelGGL(bwt_round_textsort_kernel, dim3((s.U + RS_T - 1) / RS_T), dim3(WG), 0, c->stream,
                       c->dT, s.dcodes, csa, c->cgrp[s.cur], s.U, s.h, s.n, s.smask, s.pp.cb, s.ta, c->kB, c->vB, c->dscal + DS_GIVEUP, subhead);
    prof_end(c);
    return bwt_giveup_read(c, sorted);
}

static int bwt_round_text(bscgpu_ctx* c, BwtRounds& s, bool* sorted)
{
    const u32 U = s.U;
    RC_TRY(bwt_giveup_clear(c));
    prof_begin(c, BSCGPU_K_GATHER, (u64)U * (4 + 4 + 16 + 8 + 4), U);
    return bwt_textsort(c, s, c->csa[s.cur], nullptr, sorted);
}

// The long groups' tables in an allocation of their own, made when a block first needs them — 16.8 MB per context; round 3 carved them
// out of kA on the strength of a comment.  false: not to be had (the round is handed over)
constexpr size_t LT_BYTES = (size_t)(64 + LG_MAX + (size_t)LG_MAX * LG_BUCKETS) * 4;
static bool bwt_long_tables_ensure(bscgpu_ctx* c)
{
    if (!c->long_tables && hipMalloc((void**)&c->long_tables, LT_BYTES) != hipSuccess) { (void)hipGetLastError(); c->long_tables = nullptr; }
    return c->long_tables != nullptr;
}

// ... with the n_long groups too long for one workgroup split by the top bits of the round's key first.  Group ids go to ISA, which
// does not exist yet on this path — isa_valid is false, it is built at the hand-over —, sub-group heads to flags, which only the
// seg kernels behind the round rewrite; the permuted suffixes to csa[cur ^ 1], the half the next seg writes.
static int bwt_round_text_split(bscgpu_ctx* c, BwtRounds& s, u32 n_long, bool* sorted)
{
    const u32 U = s.U, n = s.n, smask = s.smask, ta = s.ta; const u64 h = s.h; const int cur = s.cur; const PackParams& pp = s.pp; u8* const dcodes = s.dcodes;
    LongTables LT;
    LT.nlong = c->long_tables; LT.khead = LT.nlong + 64; LT.cnt = LT.khead + LG_MAX;
    u8* subhead = c->flags;
    s.first_flags = false;
    HIP_TRY(c, hipMemsetAsync(LT.nlong, 0, LT_BYTES, c->stream));
    HIP_TRY(c, hipMemsetAsync(subhead, 0, (size_t)U + 1, c->stream));
    RC_TRY(bwt_giveup_clear(c));
    const u32 blocks = capped_grid(U, 4096);
    prof_begin(c, BSCGPU_K_GATHER, (u64)U * (8 + (8 + 4 + 16 + 4) * 2), U);
    hipLaunchKernelGGL(bwt_long_heads_kernel, dim3(blocks), dim3(WG), 0, c->stream, c->cpos[cur], c->cgrp[cur], U, LT, c->ISA);
    hipLaunchKernelGGL(bwt_long_count_kernel, dim3(blocks), dim3(WG), 0, c->stream, c->dT, dcodes, c->csa[cur], c->cpos[cur], c->cgrp[cur],
                       U, h, n, smask, pp.cb, ta, LT, c->ISA);
    hipLaunchKernelGGL(bwt_long_scan_kernel, dim3(n_long), dim3(WG), 0, c->stream, LT, U, subhead);
    hipLaunchKernelGGL(bwt_long_scatter_kernel, dim3(blocks), dim3(WG), 0, c->stream, c->dT, dcodes, c->csa[cur], c->cpos[cur], c->cgrp[cur],
                       U, h, n, smask, pp.cb, ta, LT, c->ISA, c->csa[cur ^ 1]);
    return bwt_textsort(c, s, c->csa[cur ^ 1], subhead, sorted);
}

// The seg behind a round on text keys that sorted its records.  *more: the next round is one on text keys too
static int bwt_text_advance(bscgpu_ctx* c, BwtRounds& s, bool* more)
{
    const int cur = s.cur;
    u32 U2 = 0;
    s.first_flags = false;
    RC_TRY((run_seg<false, false>(c, c->kB, c->vB, c->cpos[cur], s.U, 0, s.smask, c->cpos[cur ^ 1], c->csa[cur ^ 1], c->cgrp[cur ^ 1], &U2, s.SA, c->cgrp[cur])));
    s.cur ^= 1;
    ++s.text_rounds;
    s.h += s.ta;
    if (s.dbg) fprintf(stderr, "[bwt] text round %d depth %llu U %u -> %u  (%.2f ms)\n", s.rounds, (unsigned long long)s.h, s.U, U2, bwt_lap(s));
    *more = U2 == 0 || bwt_text_round_pays(s.U, U2, s.text_rounds);
    s.U = U2;
    return BSC_NO_ERROR;
}

// hand over to prefix doubling: ISA from the current order
static int bwt_hand_over(bscgpu_ctx* c, BwtRounds& s)
{
    const u32 n = s.n, U = s.U;
    prof_begin(c, BSCGPU_K_SEG, (u64)n * 8, n);
    hipLaunchKernelGGL(bwt_isa_fill_kernel, dim3(capped_grid(n)), dim3(WG), 0, c->stream, s.SA, n, s.smask, c->ISA, s.first_flags ? c->flags : (const u8*)nullptr);
    prof_end(c);
    prof_begin(c, BSCGPU_K_SEG, (u64)U * 12, U);
    hipLaunchKernelGGL(bwt_isa_fix_kernel, dim3(capped_grid(U)), dim3(WG), 0, c->stream, c->csa[s.cur], c->cgrp[s.cur], U, s.smask, c->ISA);
    prof_end(c);
    s.isa_valid = true;
    return BSC_NO_ERROR;
}

// segmented sort of the grouped records (gives up when a group is too long for one workgroup: the radix engine then takes the round)
static int bwt_round_segsort(bscgpu_ctx* c, BwtRounds& s, bool* sorted)
{
    const u32 U = s.U;
    RC_TRY(bwt_giveup_clear(c));
    prof_begin(c, BSCGPU_K_GATHER, (u64)U * (4 + 4 + 4 + 8 + 4), U);
    hipLaunchKernelGGL(bwt_round_segsort_kernel, dim3((U + RS_T - 1) / RS_T), dim3(WG), 0, c->stream,
                       c->csa[s.cur], c->cgrp[s.cur], c->ISA, U, s.h, (u64)s.n, s.lo_bits, s.smask, c->kB, c->vB, c->dscal + DS_GIVEUP);
    prof_end(c);
    s.ks = c->kB; s.vs = c->vB;
    return bwt_giveup_read(c, sorted);
}

// hybrid round: the long groups' records through the radix engine, the rest through the segmented sort (see bwt_longrec_kernel)
static int bwt_round_hybrid(bscgpu_ctx* c, BwtRounds& s, const BwtRoundCounts& g, int* np)
{
    const u32 U = s.U, n = s.n, smask = s.smask; const u64 h = s.h; const int cur = s.cur, lo_bits = s.lo_bits;
    const u32 UL = g.n_mid_rec;                             // every record of a group of > HY_G records (seg_apply counted them)
    RC_TRY(bwt_sa_to_own_buffer(c, s));
    const Chunking lc = make_chunking(U, LR_TILE);
    u32* lidx = c->cpos[cur ^ 1];                          // the half the seg behind this round writes: free until then
    prof_begin(c, BSCGPU_K_GATHER, (u64)U * 16 + (u64)UL * (4 + 4 + 4 + 8 + 4), U);
    hipLaunchKernelGGL(bwt_longrec_kernel<false>, dim3(lc.num_chunks), dim3(WG), 0, c->stream, c->cpos[cur], c->csa[cur], c->cgrp[cur], c->ISA,
                       U, h, (u64)n, lo_bits, smask, lc.chunk_tiles, lc.num_tiles, c->segsum, lidx, c->kA, c->vA);
    hipLaunchKernelGGL(bwt_longrec_scan_kernel, dim3(1), dim3(WG), 0, c->stream, c->segsum, lc.num_chunks, c->segoff, c->dscal + DS_LRTOTAL);
    hipLaunchKernelGGL(bwt_longrec_kernel<true>, dim3(lc.num_chunks), dim3(WG), 0, c->stream, c->cpos[cur], c->csa[cur], c->cgrp[cur], c->ISA,
                       U, h, (u64)n, lo_bits, smask, lc.chunk_tiles, lc.num_tiles, c->segoff, lidx, c->kA, c->vA);
    prof_end(c);
    RadixPass rp[8];
    *np = bwt_cut_passes(rp, 0, lo_bits + bwt_bit_length((u64)(U - 1) >> LR_HEAD_SHIFT));      // 27 + 18 at 64 M unsorted records: 6 passes
    RC_TRY(radix_sort_passes(c, c->kA, c->kB, c->vA, c->vB, UL, rp, *np, &s.in_alt));
    const u64* lks = s.in_alt ? c->kB : c->kA;
    const u32* lvs = s.in_alt ? c->vB : c->vA;
    u64* ko = s.in_alt ? c->kA : c->kB;                     // the pair the sorted long records are NOT in takes the round's output
    u32* vo = s.in_alt ? c->vA : c->vB;
    prof_begin(c, BSCGPU_K_GATHER, (u64)U * (4 + 4 + 4 + 8 + 4) + (u64)UL * (8 + 4 + 4 + 4 + 8 + 4), U);
    hipLaunchKernelGGL(bwt_round_segsort_kernel, dim3((U + RS_T - 1) / RS_T), dim3(WG), 0, c->stream,
                       c->csa[cur], c->cgrp[cur], c->ISA, U, h, (u64)n, lo_bits, smask, ko, vo, c->dscal + DS_GIVEUP, 1u);
    hipLaunchKernelGGL(bwt_longrec_place_kernel, dim3(capped_grid(UL)), dim3(WG), 0, c->stream, lks, lvs, lidx, c->cgrp[cur], UL, lo_bits, ko, vo);
    prof_end(c);
    HIP_TRY(c, hipGetLastError());
    s.ks = ko; s.vs = vo;
    if (s.dbg) fprintf(stderr, "[bwt] round %d: hybrid, %u of %u records in %u group(s) of > 256\n", s.rounds, UL, U, g.n_mid);
    return BSC_NO_ERROR;
}

// the whole round through the radix engine
static int bwt_round_radix(bscgpu_ctx* c, BwtRounds& s, int* np)
{
    const u32 U = s.U, n = s.n;
    RC_TRY(bwt_sa_to_own_buffer(c, s));
    prof_begin(c, BSCGPU_K_GATHER, (u64)U * (4 + 4 + 4 + 8 + 4), U);
    hipLaunchKernelGGL(bwt_gather_kernel, dim3(capped_grid(U)), dim3(WG), 0, c->stream,
                       c->csa[s.cur], c->cgrp[s.cur], c->ISA, U, s.h, (u64)n, s.lo_bits, s.smask, c->kA, c->vA);
    prof_end(c);

    RadixPass rp[8];
    *np = bwt_cut_passes(rp, 0, s.lo_bits + bwt_bit_length(n - 1));     // key = (group rank << lo_bits) | next rank : 53 bits at n = 2^26 -> 7 passes
    RC_TRY(radix_sort_passes(c, c->kA, c->kB, c->vA, c->vB, U, rp, *np, &s.in_alt));
    s.ks = s.in_alt ? c->kB : c->kA;
    s.vs = s.in_alt ? c->vB : c->vA;
    return BSC_NO_ERROR;
}

// Runs the sort of one round.  *sorted: a text round's or a segmented sort's verdict; *np: digit passes of the radix engine
static int bwt_run_round(bscgpu_ctx* c, BwtRounds& s, BwtRound kind, const BwtRoundCounts& g, bool* sorted, int* np)
{
    switch (kind) {
    case BWT_ROUND_TEXT:       return bwt_round_text(c, s, sorted);
    case BWT_ROUND_TEXT_SPLIT: return bwt_round_text_split(c, s, g.n_long, sorted);
    case BWT_ROUND_HAND_OVER:  return BSC_NO_ERROR;                 // (no sort: the caller hands over)
    case BWT_ROUND_HYBRID:     return bwt_round_hybrid(c, s, g, np);
    case BWT_ROUND_RADIX:      return bwt_round_radix(c, s, np);
    case BWT_ROUND_SEGSORT: {
        const int rc = bwt_round_segsort(c, s, sorted);
        return (rc < 0 || *sorted) ? rc : bwt_round_radix(c, s, np);
    }
    }
    return BSC_BAD_PARAMETER;
}

// The seg behind a doubling round: the new unsorted set, ISA of the suffixes it settled
static int bwt_doubling_advance(bscgpu_ctx* c, BwtRounds& s, BwtRound kind, const BwtRoundCounts& g, int np)
{
    const int cur = s.cur;
    u32 U2 = 0;
    // (the keys' group field starts at lo_bits: a new group that begins where an old one did keeps its rank, its ISA stores are skipped)
    RC_TRY((run_seg<false, true>(c, s.ks, s.vs, c->cpos[cur], s.U, 0, s.smask, c->cpos[cur ^ 1], c->csa[cur ^ 1], c->cgrp[cur ^ 1], &U2, s.SA, nullptr,
                                 bwt_switches().isa_skip ? s.lo_bits : 0)));
    if (kind == BWT_ROUND_HYBRID && c->hscal[DS_LRTOTAL] != g.n_mid_rec) return ctx_fail(c, BSC_GPU_ERROR, "hybrid round: extracted records differ from the counted ones", hipSuccess);
    s.cur ^= 1;
    if (s.dbg) fprintf(stderr, "[bwt] round %d h=%llu U %u -> %u (passes %d)  (%.2f ms)\n", s.rounds, (unsigned long long)s.h, s.U, U2, np, bwt_lap(s));
    s.U = U2;
    s.h <<= 1;
    return BSC_NO_ERROR;
}

// The ending of a batched pass: every block's indexes from the final ISA, every block's L in place; one copy of the results, one sync for the pass
static int bwt_emit_batch(bscgpu_ctx* c, const BwtRounds& s, const BwtBatch* bt, u8* dL_user, int64_t* primary_out)
{
    const u32 n = s.n;
    prof_begin(c, BSCGPU_K_EMIT, (u64)n * 10, n);
    HIP_TRY(c, hipMemsetAsync(bt->res, 0, (size_t)bt->count * 16 * 4, c->stream));
    hipLaunchKernelGGL(bwt_batch_find_kernel, dim3((bt->count + WG - 1) / WG), dim3(WG), 0, c->stream, c->ISA, n, bt->off, bt->rate, bt->count, bt->res);
    hipLaunchKernelGGL(bwt_batch_emit_kernel, dim3((n + WG - 1) / WG), dim3(WG), 0, c->stream, c->dT, s.SA, c->ISA, n, bt->off, bt->rate, bt->count, dL_user);
    prof_end(c);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(bt->res_host, bt->res, (size_t)bt->count * 16 * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, ctx_sync(c));
    prof_collect(c);
    *primary_out = 0;
    return BSC_NO_ERROR;
}

// The ending of a single block: primary index and aux indexes from SA, then the last column
static int bwt_emit_single(bscgpu_ctx* c, const BwtRounds& s, const u8* ddecode, u8* dL_user, int64_t n64, int64_t r, u32* I_host, int64_t* primary_out)
{
    const u32 n = s.n;
    u32 cnt = 0, rshift = 0;
    if (I_host != nullptr) {
        if (r <= 0 || (r & (r - 1)) != 0) return BSC_BAD_PARAMETER;
        cnt = (u32)((n64 - 1) / r) + 1;
        if (cnt > 256) return BSC_BAD_PARAMETER;
        while ((1ll << rshift) < r) ++rshift;
    }
    prof_begin(c, BSCGPU_K_EMIT, (u64)n * 4, n);
    hipLaunchKernelGGL(bwt_find_kernel, dim3((n + 4 * WG - 1) / (4 * WG)), dim3(WG), 0, c->stream,
                       s.SA, n, s.smask, cnt ? (u32)(r - 1) : 0u, rshift, cnt, c->dscal);
    prof_end(c);
    prof_begin(c, BSCGPU_K_EMIT, (u64)n * 6, n);
    if (s.pp.pred_shift)
        hipLaunchKernelGGL(bwt_emit_pred_kernel, dim3((n + 4 * WG - 1) / (4 * WG)), dim3(WG), 0, c->stream,
                           c->dT, s.SA, n, s.pp.pred_shift, ddecode, dL_user, c->dscal);
    else
        hipLaunchKernelGGL(bwt_emit_kernel, dim3((n + 4 * WG - 1) / (4 * WG)), dim3(WG), 0, c->stream,
                           c->dT, s.SA, n, dL_user, c->dscal);
    prof_end(c);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(c->hscal, c->dscal, (DS_AUX + DS_AUX_LEN) * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, ctx_sync(c));
    prof_collect(c);
    *primary_out = c->hscal[DS_PRIMARY];
    for (u32 t = 0; t < cnt; ++t) I_host[t] = c->hscal[DS_AUX + t];
    return BSC_NO_ERROR;
}

// One transform: first sort, first seg, and while suffixes are unsorted: decide the round (bwt_plan.h), run it, seg, advance; then emit.
static int bwt_device_once(bscgpu_ctx* c, const u8* dT_user, u8* dL_user, int64_t n64, int64_t r, u32* I_host, int64_t* primary_out,
                           const BwtBatch* bt)
{
    if (n64 < 0 || n64 > c->max_n || n64 >= 0x7fffffffll) return BSC_BAD_PARAMETER;
    if (n64 == 0) { *primary_out = 0; return BSC_NO_ERROR; }
    const u32 n = (u32)n64;
    const BwtSwitches& sw = bwt_switches();

    FirstSort fs;
    RC_TRY(bwt_first_sort(c, dT_user, n, bt, &fs));
    BwtRounds s;
    s.n = n; s.pp = fs.pp; s.smask = fs.kp.smask; s.ta = fs.kp.ta; s.dcodes = fs.dcodes; s.lo_bits = bwt_bit_length(n);
    s.cur = 0; s.U = 0; s.h = fs.pp.w; s.ks = fs.ks; s.vs = fs.vs; s.in_alt = 0; s.rounds = 0; s.text_rounds = 0; s.first_flags = true;
    // text rounds read the text past a suffix: not across block ends; their keys hold 2 .. 15 characters
    s.isa_valid = bt != nullptr || !(sw.text_rounds && s.ta >= 2 && s.ta <= 15);
    s.SA = (s.vs == c->vA) ? c->vA : c->SA;
    if (s.isa_valid) RC_TRY((run_seg<true, true >(c, s.ks, s.vs, nullptr, n, fs.kp.tail_lo, s.smask, c->cpos[0], c->csa[0], c->cgrp[0], &s.U, s.SA)));
    else             RC_TRY((run_seg<true, false>(c, s.ks, s.vs, nullptr, n, fs.kp.tail_lo, s.smask, c->cpos[0], c->csa[0], c->cgrp[0], &s.U, s.SA)));

    s.dbg = getenv("BSCGPU_DEBUG") != nullptr;
    if (s.dbg) fprintf(stderr, "[bwt] n=%u initial unsorted=%u\n", n, s.U);
    s.t_round = s.dbg ? bwt_now_ms() : 0.0;
    while (s.U > 0) {
        if (++s.rounds > 60) return ctx_fail(c, BSC_GPU_ERROR, "prefix doubling did not converge", hipSuccess);
        // what the seg that produced this unsorted set counted (seg_apply): groups of > RS_G records, which no segmented sort of this
        // round can take, and groups of > HY_G records (hybrid rounds), each with their records
        const BwtRoundCounts g = {s.U, c->hscal[DS_NLONG], c->hscal[DS_EXCESS] + c->hscal[DS_NLONG] * (u32)RS_G,
                                  c->hscal[DS_NMID], c->hscal[DS_MIDEXCESS] + c->hscal[DS_NMID] * (u32)HY_G};
        BwtRound kind = bwt_round_kind(s.isa_valid, g, sw, LG_MAX);
        if (kind == BWT_ROUND_TEXT_SPLIT && !bwt_long_tables_ensure(c)) kind = BWT_ROUND_HAND_OVER;
        bool sorted = false;
        int np = 0;
        if (!s.isa_valid) {
            // a round on text keys; it hands over to doubling when a group does not fit a workgroup or the round did not pay
            RC_TRY(bwt_run_round(c, s, kind, g, &sorted, &np));
            if (s.dbg && kind != BWT_ROUND_TEXT)
                fprintf(stderr, "[bwt] text round %d: %u long group(s) with %u of %u records: %s\n", s.rounds, g.n_long, g.n_long_rec, s.U,
                        kind == BWT_ROUND_HAND_OVER ? "not split (too many / too large)" : sorted ? "split by the top key bits -> sorted" : "split, but a bucket is still too long");
            if (sorted) {
                bool more = false;
                RC_TRY(bwt_text_advance(c, s, &more));
                if (more) continue;
            } else if (s.dbg) fprintf(stderr, "[bwt] text round %d: group too long, handing over\n", s.rounds);
            RC_TRY(bwt_hand_over(c, s));
            if (sorted) continue;                    // the round itself was done; the next one doubles
            kind = bwt_round_kind(true, g, sw, LG_MAX);     // this round doubles
        }
        RC_TRY(bwt_run_round(c, s, kind, g, &sorted, &np));
        RC_TRY(bwt_doubling_advance(c, s, kind, g, np));
    }
    c->stage_ms[5] = s.rounds;
    return bt ? bwt_emit_batch(c, s, bt, dL_user, primary_out) : bwt_emit_single(c, s, fs.ddecode, dL_user, n64, r, I_host, primary_out);
}
