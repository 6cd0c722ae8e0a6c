// radix_sort.hip — stable LSD radix sort of (u64 key [, u32 value]) records for gfx950 (MI355X).
//
// This is the engine under both block sorters: the BWT's suffix sort (initial 8-byte-prefix sort and
// every prefix-doubling round) and the Sort Transform.  It replaces the reference's calls into
// cub::DeviceRadixSort / cub::DeviceSegmentedSort (libcubwt.cu:718, :1691, :2136-2163; st.cu:187-193,
// :273-279) with a design written for CDNA4, not a translation of CUB:
//
//  * One digit pass = three launches on one stream: rs_hist (per-chunk digit counts of the pass's
//    input), rs_scan (256 workgroups, one per digit: exclusive scan over chunks), rs_scatter (the
//    graded kernel).  There is NO inter-workgroup communication inside a launch: on MI355X the eight
//    XCD L2s are not coherent and an agent-scope hand-off costs ~1-3 us under streaming load
//    (MI355X_MICROARCH.md, handoff rows; 4.6 us per hop in tools/ubench.hip), while the chip retires a
//    196 KB tile every ~50 ns: with 256 tiles in flight a decoupled look-back ("onesweep") has to sum ~20
//    predecessor rows per tile through L2-bypassing loads; measured under streaming load it adds 0.07-0.09 ms
//    per pass on the tiles' critical path (tools/ubench_lookback.hip) and gives up the chunk-contiguous
//    output segments write combining needs.
//    The price paid instead is one extra streaming read of the keys per pass (8 B/record, rs_hist, at
//    4.5 TB/s); the scatter pass itself moves exactly the algorithmic 2*(8+4) B/record.
//  * <= 1024 chunks for rs_hist (one 256-thread workgroup each, 4 per CU, all resident; block b runs on XCD b % 8 so
//    every XCD streams an equal contiguous share).  rs_scatter: 256 threads x 16 records (4096-record tiles, one chunk
//    per workgroup) for keys-only passes and small inputs.  A workgroup walks its records tile by tile keeping its 256
//    running global bucket offsets in LDS, so the per-chunk offsets table is only 256 x 1024 u32.
//  * rs_scatter_tiled (large (key, value) passes): 1024 threads x 8 records (8192-record tiles: the longer per-digit runs
//    halve the number of partially written lines), the tiles interleaved so that an XCD always works on 32 consecutive
//    tiles: neighbouring runs of a digit are written at the same time by CUs that share an L2, and the offsets are per tile.
//    0.60-0.62 of 8 TB/s on the BWT's keys.  (The same shape with one contiguous tile range per workgroup, plain and with
//    write combining in LDS, reached 0.55 and was removed: NOTES_r01-r04.md §3.1.)
//  * Inside a tile: wave-striped coalesced loads (each wave64 load instruction covers 512 contiguous
//    bytes of keys), 8-bit digit, stable in-wave ranking by wave64 ballot match (rs_match8: 8 ballots -> peer
//    mask, 32 hand-scheduled VALU instructions per record), per-wave 256-bin histograms in LDS, then the tile is locally
//    reordered through LDS (32 / 64 KB staging) so that every bucket leaves as one contiguous run:
//    consecutive lanes store consecutive addresses.  Integer/index work only — no MFMA.
#include "dev_common.h"
#include "radix_dev.h"
#include <cstdio>
#include <cstdlib>
#include <type_traits>

// Streamed-once inputs are read with non-temporal loads in rs_hist and rs_scatter (+10-20 %: they stop evicting the
// partially written output lines from L2); non-temporal *stores* were measured 20-50 % slower and are not used.
#ifndef RS_NT
#define RS_NT 5      // bit2: nt loads in rs_hist (A/B builds)
#endif
#ifndef RS_WG
#define RS_WG 256      // shape for keys-only passes and small inputs (rs_scatter_tiled serves large pair passes)
#endif
// Phase timing (debug builds, -DRS_PHASE_TIMING=1): thread 0 of every workgroup stamps s_memtime at the phase boundaries of
// its first 32 tiles into the context's scratch buffer; radix_sort_passes dumps the last pass to gpurun_out/phase_timing.bin.
#ifndef RS_PHASE_TIMING
#define RS_PHASE_TIMING 0
#endif
#if RS_PHASE_TIMING
#define RS_PH(i) do { if (t == 0 && tile_no < 32u) tdbg[((size_t)blockIdx.x * 32 + tile_no) * 16 + (i)] = __builtin_amdgcn_s_memtime(); } while (0)
#else
#define RS_PH(i) do { } while (0)
#endif
constexpr int RS_WAVES = RS_WG / 64;
#ifndef RS_ITEMS_N
#define RS_ITEMS_N 16
#endif
constexpr int RS_ITEMS = RS_ITEMS_N;
constexpr int RS_TILE  = RS_WG * RS_ITEMS;       // 4096 records per tile
constexpr int RS_LDS   = RS_TILE * 8 + RS_WAVES * 256 * 4 + 3 * 256 * 4 + 16 * 4;   // 40,000 B -> 4 WG (16 waves) / CU
constexpr int RS_MAX_CHUNKS = 256 * (1024 / RS_WG);       // all workgroups resident at once: 4 per CU
// shape of rs_scatter_tiled for large (key, value) passes
#ifndef RS_BIG_PAIRS
#define RS_BIG_PAIRS 1
#endif
#ifndef RSB_ITEMS_N
#define RSB_ITEMS_N 8
#endif
constexpr int RSB_WG = 1024, RSB_ITEMS = RSB_ITEMS_N;

static inline Chunking rs_chunking(u64 n) {
    // measured: 768 / 512 / 256 chunks (fewer open output lines per XCD, but fewer waves) are 1 / 5 / 40 % slower
    constexpr u32 RS_MAX_CHUNKS_RT = RS_MAX_CHUNKS;
    Chunking c;
    c.num_tiles   = (u32)((n + RS_TILE - 1) / RS_TILE);
    if (c.num_tiles == 0) c.num_tiles = 1;
    c.chunk_tiles = (c.num_tiles + RS_MAX_CHUNKS_RT - 1) / RS_MAX_CHUNKS_RT;
    c.num_chunks  = (c.num_tiles + c.chunk_tiles - 1) / c.chunk_tiles;
    return c;
}

// ---------------------------------------------------------------------------------------------
// rs_hist: per-chunk digit histogram.  counts layout [digit][chunk].
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(RS_WG) void rs_hist_kernel(const u64* __restrict__ keys, u32 n, int shift, u32 mask,
                                                        u32 chunk_tiles, u32 num_chunks, u32* __restrict__ counts)
{
    // BWT keys are text: a handful of digit values dominate, so a single 256-bin histogram per wave serialises its
    // LDS atomics (measured 2.4 TB/s with every lane on one bin).  Each wave keeps HREP replicas selected by the
    // low lane bits, which cuts the worst case from 64-way to 8-way conflicts; replicas are summed at the end.
    constexpr int WG = RS_WG, WAVES = RS_WAVES, HREP = 32 / RS_WAVES;
    __shared__ u32 h[WAVES * HREP * 256];
    const u32 t = threadIdx.x, w = t >> 6;
    for (u32 i = t; i < WAVES * HREP * 256; i += WG) h[i] = 0;
    __syncthreads();

    const u64 start = (u64)blockIdx.x * chunk_tiles * RS_TILE;
    u64 end = start + (u64)chunk_tiles * RS_TILE;
    if (end > n) end = n;
    u32* hw = h + (w * HREP + (t & (HREP - 1))) * 256;

    // 16-byte loads (2 keys per lane), 4 in flight per lane.
    u64 i = start + 2 * t;
    for (; i + 3 * 2 * WG + 1 < end; i += 4 * 2 * WG) {
        ulonglong2 a, b, c, d;
        if (RS_NT & 4) {
            a.x = __builtin_nontemporal_load(keys + i);          a.y = __builtin_nontemporal_load(keys + i + 1);
            b.x = __builtin_nontemporal_load(keys + i + 2 * WG); b.y = __builtin_nontemporal_load(keys + i + 2 * WG + 1);
            c.x = __builtin_nontemporal_load(keys + i + 4 * WG); c.y = __builtin_nontemporal_load(keys + i + 4 * WG + 1);
            d.x = __builtin_nontemporal_load(keys + i + 6 * WG); d.y = __builtin_nontemporal_load(keys + i + 6 * WG + 1);
        } else {
            a = *reinterpret_cast<const ulonglong2*>(keys + i);
            b = *reinterpret_cast<const ulonglong2*>(keys + i + 2 * WG);
            c = *reinterpret_cast<const ulonglong2*>(keys + i + 4 * WG);
            d = *reinterpret_cast<const ulonglong2*>(keys + i + 6 * WG);
        }
        atomicAdd(&hw[(u32)(a.x >> shift) & mask], 1u); atomicAdd(&hw[(u32)(a.y >> shift) & mask], 1u);
        atomicAdd(&hw[(u32)(b.x >> shift) & mask], 1u); atomicAdd(&hw[(u32)(b.y >> shift) & mask], 1u);
        atomicAdd(&hw[(u32)(c.x >> shift) & mask], 1u); atomicAdd(&hw[(u32)(c.y >> shift) & mask], 1u);
        atomicAdd(&hw[(u32)(d.x >> shift) & mask], 1u); atomicAdd(&hw[(u32)(d.y >> shift) & mask], 1u);
    }
    for (; i < end; i += 2 * WG) {
        atomicAdd(&hw[(u32)(keys[i] >> shift) & mask], 1u);
        if (i + 1 < end) atomicAdd(&hw[(u32)(keys[i + 1] >> shift) & mask], 1u);
    }
    __syncthreads();
    if (t < 256) {
        u32 sum = 0;
#pragma unroll 8
        for (int r = 0; r < WAVES * HREP; ++r) sum += h[r * 256 + t];
        counts[(size_t)t * num_chunks + blockIdx.x] = sum;
    }
}

// ---------------------------------------------------------------------------------------------
// rs_scan: workgroup d turns row d of counts into exclusive per-chunk offsets and its row total.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(WG) void rs_scan_kernel(u32* __restrict__ counts, u32 num_chunks, u32* __restrict__ rowtot)
{
    __shared__ u32 scr[8];
    u32* row = counts + (size_t)blockIdx.x * num_chunks;
    u32 carry = 0;
    for (u32 base = 0; base < num_chunks; base += WG) {
        const u32 i = base + threadIdx.x;
        const u32 v = (i < num_chunks) ? row[i] : 0u;
        u32 tot;
        const u32 ex = block_excl_sum(v, scr, &tot);
        if (i < num_chunks) row[i] = carry + ex;
        carry += tot;
    }
    if (threadIdx.x == 0) rowtot[blockIdx.x] = carry;
}

// ---------------------------------------------------------------------------------------------
// rs_scatter: the digit pass.  Reads each record once, writes it once.
// ---------------------------------------------------------------------------------------------
// 256 x 16 (4096-record tiles, 4 workgroups per CU, one rs_hist chunk each): keys-only passes, small inputs, and every pass of
// the three-kernel path that rs_scatter_tiled does not take.
// EMIT_POS: also write, for every input record (in input order, coalesced), the index it lands on — the inverse of the
// pass's permutation, which the device coder needs to find a run inside its sorted copies (devcoder.hip).
template <bool HAS_VAL, bool EMIT_POS = false>
__global__ __launch_bounds__(RS_WG, 4) void rs_scatter_kernel(const u64* __restrict__ kin, u64* __restrict__ kout,
                                                        const u32* __restrict__ vin, u32* __restrict__ vout,
                                                        u32 n, int shift, u32 mask,
                                                        u32 chunk_tiles, u32 num_chunks, u32 num_tiles,
                                                        const u32* __restrict__ offsets,
                                                        const u32* __restrict__ rowtot, u64* __restrict__ sink,
                                                        u32* __restrict__ dstpos = nullptr)
{
    constexpr int WG = RS_WG, WAVES = RS_WAVES, ITEMS = RS_ITEMS, TILE = RS_TILE;
    u64* const tdbg = sink; (void)tdbg;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    u64* skeys  = reinterpret_cast<u64*>(smem);                       // [TILE] staging (reused as u32 for values)
    u32* whist  = reinterpret_cast<u32*>(smem + TILE * 8);            // [WAVES][256] per-wave digit counts / prefixes
    u32* goff   = whist + WAVES * 256;                                // [256] running global bucket offsets
    u32* adj    = goff + 256;                                         // [256] goff - tile-local bucket start
    u32* dstart = adj + 256;                                          // [256] (scratch)
    u32* scr    = dstart + 256;                                       // [8]
    lds_vu32* vwh = (lds_vu32*)whist;

    const u32 t = threadIdx.x, w = t >> 6, lane = t & 63;

    {   // global offset of this chunk's first record of digit t
        u32 tot;
        const u32 base = rs_digit_excl_sum<WAVES>(t < 256 ? rowtot[t] : 0u, scr, &tot);
        if (t < 256) goff[t] = base + offsets[(size_t)t * num_chunks + blockIdx.x];
    }
    // every wave owns (and re-zeroes, see below) its 256 counters
#pragma unroll
    for (int i = 0; i < 4; ++i) whist[w * 256 + i * 64 + lane] = 0;
    __syncthreads();

    // this workgroup's records: its rs_hist chunk (chunk_tiles tiles of RS_TILE records); n < 2^32 - 2^20
    const u32 rec0 = (u32)((u64)blockIdx.x * chunk_tiles * RS_TILE);
    u32 rec1;
    { const u64 e = (u64)rec0 + (u64)chunk_tiles * RS_TILE; rec1 = e > n ? n : (u32)e; }

    // wave-striped ownership: wave w holds records [w*64*ITEMS, (w+1)*64*ITEMS) of the tile, item i = 64 consecutive records
    const u32 wbase = w * (64 * ITEMS) + lane;
    u64 k[ITEMS];
    u32 v[ITEMS];

    // Full tiles run without any branch around a global load or store, so the compiler can wait with exact vmcnt values
    // (a guarded memory instruction makes the number of outstanding operations unknown and later waits conservative);
    // the one partial tile of the whole input is handled by a second, guarded instantiation after the loop.
    // Barriers per tile: after ranking, inside and after the digit scan, after the staging writes, and two around the value
    // staging.  None at the end of a tile: what the next tile writes first (its own wave's counters, then — behind its first
    // barrier — adj / goff) is not read by anyone still in this tile's write-out.
    auto do_tile = [&](const u32 tbase, const u32 nvalid, auto full_tag) __attribute__((always_inline)) {
        constexpr bool FULL = decltype(full_tag)::value;
        const u32 tile_no = (tbase - rec0) / TILE; (void)tile_no;
        RS_PH(0);

#pragma unroll
        for (int i = 0; i < ITEMS; ++i) {
            const u32 idx = wbase + i * 64;
            if (FULL) k[i] = __builtin_nontemporal_load(&kin[(u64)tbase + idx]);
            else k[i] = (idx < nvalid) ? __builtin_nontemporal_load(&kin[(u64)tbase + idx]) : ~0ull;
        }
        RS_PH(1);

        // ---- stable in-wave ranking by ballot match (rs_rank_wave) --------------------------------
        u32 rk[ITEMS];
        rs_rank_wave<ITEMS>(k, shift, mask, vwh + w * 256, rk);
        RS_PH(2);
        // values are fetched only now (they are not needed for ranking): keeps the ranking loop's
        // register footprint at 4 waves/SIMD, and the loads fly under the bucket scan + key reorder.
        if (HAS_VAL) {
#pragma unroll
            for (int i = 0; i < ITEMS; ++i) {
                const u32 idx = wbase + i * 64;
                if (FULL) v[i] = __builtin_nontemporal_load(&vin[(u64)tbase + idx]);
                else v[i] = (idx < nvalid) ? __builtin_nontemporal_load(&vin[(u64)tbase + idx]) : 0u;
            }
        }
        __syncthreads();
        RS_PH(3);

        // ---- per digit: wave prefixes, tile-local bucket start, global adjust -------------------
        {
            u32 c[WAVES];
            u32 tot = 0;
            if (t < 256) {
#pragma unroll
                for (int i = 0; i < WAVES; ++i) { c[i] = whist[i * 256 + t]; tot += c[i]; }
            }
            u32 all;
            const u32 ds = rs_digit_excl_sum<WAVES, false>(tot, scr, &all);
            if (t < 256) {
                u32 run = ds;
#pragma unroll
                for (int i = 0; i < WAVES; ++i) { whist[i * 256 + t] = run; run += c[i]; }
                const u32 g = goff[t];
                adj[t]  = g - ds;
                goff[t] = g + tot;
            }
        }
        __syncthreads();
        RS_PH(4);

        // ---- local reorder through LDS --------------------------------------------------------
#pragma unroll
        for (int i = 0; i < ITEMS; ++i) {
            const u32 d = (u32)(k[i] >> shift) & mask;
            const u32 pos = whist[w * 256 + d] + rk[i];
            rk[i] = pos;
            skeys[pos] = k[i];
            if (EMIT_POS) { const u32 idx = wbase + i * 64; if (FULL || idx < nvalid) dstpos[(u64)tbase + idx] = adj[d] + pos; }
        }
        RS_PH(5);
        __syncthreads();
        RS_PH(6);
#pragma unroll
        for (int i = 0; i < 4; ++i) whist[w * 256 + i * 64 + lane] = 0;       // for the next tile's ranking (own wave's counters only)

        u32 dd[ITEMS / 4];
#pragma unroll
        for (int j = 0; j < ITEMS; ++j) {
            const u32 q = j * WG + t;
            const u64 key = skeys[q];
            const u32 d = (u32)(key >> shift) & mask;
            if ((j & 3) == 0) dd[j >> 2] = d; else dd[j >> 2] |= d << (8 * (j & 3));
            if (FULL || q < nvalid) kout[adj[d] + q] = key;
        }
        RS_PH(7);

        if (HAS_VAL) {
            __syncthreads();
            u32* svals = reinterpret_cast<u32*>(skeys);
#pragma unroll
            for (int i = 0; i < ITEMS; ++i) svals[rk[i]] = v[i];
            __syncthreads();
            RS_PH(8);
#pragma unroll
            for (int j = 0; j < ITEMS; ++j) {
                const u32 q = j * WG + t;
                const u32 d = (dd[j >> 2] >> (8 * (j & 3))) & 0xffu;
                if (FULL || q < nvalid) vout[adj[d] + q] = svals[q];
            }
        }
        RS_PH(9);
        RS_PH(10);
        };
    u32 tbase = rec0;
    for (; tbase + TILE <= rec1; tbase += TILE) do_tile(tbase, (u32)TILE, std::true_type());
    if (tbase < rec1) do_tile(tbase, rec1 - tbase, std::false_type());
}

// ---------------------------------------------------------------------------------------------
// rs_scatter_tiled (large (key, value) passes): the 1024 x 8 digit pass with the tiles INTERLEAVED over the workgroups instead
// of one contiguous range per workgroup: in round it workgroup b takes tile it * 256 + (b % 8) * 32 + b / 8, so an XCD
// (workgroups b % 8) always works on 32 consecutive tiles.  Neighbouring runs of a digit are then written at about the same
// time by CUs that share an L2, which can merge their partial lines, and the reads of a round cover one contiguous 50 MB
// stretch (tools/ubench_wc.hip: misaligned runs 0.541 -> 0.445 ms; tools/ubench_lookback.hip: tile copy 6.05 against 5.33 TB/s).
// The price: offsets per TILE instead of per chunk (counts table [256][tiles], rs_hist launched with one tile per workgroup),
// fetched per tile (one round ahead), and no state carried from tile to tile (no write combining).
// ---------------------------------------------------------------------------------------------
constexpr int RST_LDS = RSB_WG * RSB_ITEMS * 8 + (RSB_WG / 64) * 256 * 4 + 3 * 256 * 4 + 16 * 4;

template <bool HAS_VAL>
__global__ __launch_bounds__(RSB_WG) void rs_scatter_tiled_kernel(const u64* __restrict__ kin, u64* __restrict__ kout,
                                                                  const u32* __restrict__ vin, u32* __restrict__ vout,
                                                                  u32 n, int shift, u32 mask, u32 num_tiles,
                                                                  const u32* __restrict__ offsets /*[256][num_tiles]*/,
                                                                  const u32* __restrict__ rowtot)
{
    constexpr int WG = RSB_WG, WAVES = RSB_WG / 64, ITEMS = RSB_ITEMS, TILE = RSB_WG * RSB_ITEMS;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    u64* skeys  = reinterpret_cast<u64*>(smem);
    u32* whist  = reinterpret_cast<u32*>(smem + TILE * 8);
    u32* adj    = whist + WAVES * 256;
    u32* scr    = adj + 3 * 256;
    lds_vu32* vwh = (lds_vu32*)whist;
    const u32 t = threadIdx.x, w = t >> 6, lane = t & 63;

    u32 dbase;                                            // first output position of digit t & 255
    {
        u32 tot;
        dbase = rs_digit_excl_sum<WAVES>(t < 256 ? rowtot[t] : 0u, scr, &tot);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) whist[w * 256 + i * 64 + lane] = 0;
    __syncthreads();

    const u32 wbase = w * (64 * ITEMS) + lane;
    u64 k[ITEMS];
    u32 v[ITEMS];
    auto prefetch_keys = [&](const u32 tile) __attribute__((always_inline)) {
        const u32 tb = tile * (u32)TILE;
#pragma unroll
        for (int i = 0; i < ITEMS; ++i) { u32 e = tb + wbase + i * 64; e = (tile < num_tiles && e < n) ? e : 0u; k[i] = __builtin_nontemporal_load(&kin[e]); }
    };
    auto prefetch_vals = [&](const u32 tile) __attribute__((always_inline)) {
        const u32 tb = tile * (u32)TILE;
#pragma unroll
        for (int i = 0; i < ITEMS; ++i) { u32 e = tb + wbase + i * 64; e = (tile < num_tiles && e < n) ? e : 0u; v[i] = __builtin_nontemporal_load(&vin[e]); }
    };
    auto fetch_offset = [&](const u32 tile) __attribute__((always_inline)) -> u32 {          // every thread loads (no branch around a load)
        return offsets[(size_t)(t & 255u) * num_tiles + (tile < num_tiles ? tile : num_tiles - 1)];
    };
#ifndef RST_XCD_RUN
#define RST_XCD_RUN 32          // consecutive tiles an XCD works on at a time (A/B builds: 8, 1 = plain round robin)
#endif
    const u32 first = ((blockIdx.x >> 3) / (u32)RST_XCD_RUN) * (8u * (u32)RST_XCD_RUN) + (blockIdx.x & 7u) * (u32)RST_XCD_RUN + ((blockIdx.x >> 3) % (u32)RST_XCD_RUN);
    u32 off_next = fetch_offset(first);
    prefetch_keys(first);
    if (HAS_VAL) prefetch_vals(first);

    auto do_tile = [&](const u32 tile, const u32 nvalid, auto full_tag) __attribute__((always_inline)) {
        constexpr bool FULL = decltype(full_tag)::value;
        const u32 tbase = tile * (u32)TILE;
        const u32 off_cur = off_next;
        off_next = fetch_offset(tile + 256);
        if (!FULL) {
#pragma unroll
            for (int i = 0; i < ITEMS; ++i) if (wbase + i * 64 >= nvalid) k[i] = ~0ull;
        }
        u32 rk[ITEMS];
        rs_rank_wave<ITEMS>(k, shift, mask, vwh + w * 256, rk);
        __syncthreads();
        {
            u32 c[WAVES];
            u32 tot = 0;
            if (t < 256) {
#pragma unroll
                for (int i = 0; i < WAVES; ++i) { c[i] = whist[i * 256 + t]; tot += c[i]; }
            }
            u32 all;
            const u32 ds = rs_digit_excl_sum<WAVES, false>(tot, scr, &all);
            if (t < 256) {
                u32 run = ds;
#pragma unroll
                for (int i = 0; i < WAVES; ++i) { whist[i * 256 + t] = run; run += c[i]; }
                adj[t] = dbase + off_cur - ds;
            }
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < ITEMS; ++i) {
            const u32 d = (u32)(k[i] >> shift) & mask;
            const u32 pos = whist[w * 256 + d] + rk[i];
            rk[i] = pos;
            skeys[pos] = k[i];
        }
        prefetch_keys(tile + 256);
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 4; ++i) whist[w * 256 + i * 64 + lane] = 0;
        u32 dd[ITEMS / 4];
#pragma unroll
        for (int j = 0; j < ITEMS; ++j) {
            const u32 q = j * WG + t;
            const u64 key = skeys[q];
            const u32 d = (u32)(key >> shift) & mask;
            if ((j & 3) == 0) dd[j >> 2] = d; else dd[j >> 2] |= d << (8 * (j & 3));
            if (FULL || q < nvalid) kout[adj[d] + q] = key;
        }
        if (HAS_VAL) {
            __syncthreads();
            u32* svals = reinterpret_cast<u32*>(skeys);
#pragma unroll
            for (int i = 0; i < ITEMS; ++i) svals[rk[i]] = v[i];
            prefetch_vals(tile + 256);
            __syncthreads();
#pragma unroll
            for (int j = 0; j < ITEMS; ++j) {
                const u32 q = j * WG + t;
                const u32 d = (dd[j >> 2] >> (8 * (j & 3))) & 0xffu;
                if (FULL || q < nvalid) vout[adj[d] + q] = svals[q];
            }
        }
        (void)tbase;
    };
    for (u32 tile = first; tile < num_tiles; tile += 256) {
        const u32 left = n - tile * (u32)TILE;
        if (left >= (u32)TILE) do_tile(tile, (u32)TILE, std::true_type());
        else do_tile(tile, left, std::false_type());
    }
}

// ---------------------------------------------------------------------------------------------
// host launcher
// ---------------------------------------------------------------------------------------------
// Per-context (= per-device) setup, called from bscgpu_create with the context's device current: the dynamic-LDS limits
// of the large-tile kernels are a per-device attribute of the function, so every device that gets a context must be told
// (a process-wide `static` here would configure only the first device and race between threads).  rs_scatter_tiled's are set
// where its count table is first allocated (radix_sort_passes).
int radix_engine_setup(bscgpu_ctx* c)
{
    return radix_onesweep_setup(c);
}

int radix_sort_passes(bscgpu_ctx* c, u64* keys, u64* keys_alt, u32* vals, u32* vals_alt, u64 n,
                      const RadixPass* passes, int npasses, int* in_alt, u32* emit_pos, bool aux)
{
    if (emit_pos != nullptr && (npasses != 1 || vals != nullptr)) return BSC_BAD_PARAMETER;     // inverse of ONE keys-only pass
    *in_alt = 0;
    if (n == 0 || npasses == 0) return BSC_NO_ERROR;
    if (n >= 0xfff00000ull) return BSC_BAD_PARAMETER;          // record indexes are u32, with headroom for a tile past the end
    if ((((uintptr_t)keys) | ((uintptr_t)keys_alt)) & 15) return ctx_fail(c, BSC_BAD_PARAMETER, "radix keys not 16B aligned", hipSuccess);

    const Chunking ch = rs_chunking(n);
    const bool has_val = (vals != nullptr);
    // large (key, value) sorts: one histogram read per sort + single-read digit passes (radix_onesweep.hip; BSC_RS_ONESWEEP)
    if (emit_pos == nullptr && !aux && radix_onesweep_wanted(c, n, npasses, has_val)) {
        const int rc = radix_onesweep_sort(c, keys, keys_alt, vals, vals_alt, n, passes, npasses);
        if (rc == BSC_NO_ERROR) *in_alt = (npasses & 1);
        return rc;
    }
    u64 *ksrc = keys, *kdst = keys_alt;
    u32 *vsrc = vals, *vdst = vals_alt;
    const u64 rec_bytes = 8 + (has_val ? 4 : 0);
    // large (key, value) passes: XCD-interleaved 8192-record tiles (rs_scatter_tiled_kernel), enough of them for every CU; everything
    // else (keys-only passes, small inputs, emit_pos) the 256 x 16 rs_scatter_kernel
    const bool tiled = RS_BIG_PAIRS && has_val && ch.num_chunks >= 512 && ch.chunk_tiles >= 2;
    const u32 num_tiles8k = (u32)((n + 8191) / 8192);
    if (tiled && c->tile_counts_cap < (size_t)256 * num_tiles8k) {
        if (c->tile_counts) (void)hipFree(c->tile_counts);
        c->tile_counts = nullptr; c->tile_counts_cap = 0;
        const size_t want = (size_t)256 * ((size_t)(c->max_n > (int64_t)n ? c->max_n : (int64_t)n) / 8192 + 2);
        if (hipMalloc((void**)&c->tile_counts, want * 4) != hipSuccess) return ctx_fail(c, BSC_GPU_NOT_ENOUGH_MEMORY, "tile count table", hipSuccess);
        c->tile_counts_cap = want;
        HIP_TRY(c, hipFuncSetAttribute((const void*)rs_scatter_tiled_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, RST_LDS));
    }

    // passes that also emit the permutation serve the device coder / the inverse BWT: booked apart from the graded digit passes
    // (aux: keys-only passes of the device coder that carry their permutation in the key's low bits)
    const bool book_aux = emit_pos != nullptr || aux;
    const int kind_hist = book_aux ? BSCGPU_K_RADIX_AUX : BSCGPU_K_RADIX_HIST, kind_scan = book_aux ? BSCGPU_K_RADIX_AUX : BSCGPU_K_RADIX_SCAN,
              kind_scatter = book_aux ? BSCGPU_K_RADIX_AUX : BSCGPU_K_RADIX_SCATTER;
    for (int p = 0; p < npasses; ++p) {
        const int shift = passes[p].shift;
        const u32 mask  = (passes[p].bits >= 8) ? 0xffu : ((1u << passes[p].bits) - 1u);

        if (tiled) {
            prof_begin(c, BSCGPU_K_RADIX_HIST, n * 8, n);
            hipLaunchKernelGGL(rs_hist_kernel, dim3(num_tiles8k), dim3(RS_WG), 0, c->stream,
                               ksrc, (u32)n, shift, mask, 2u, num_tiles8k, c->tile_counts);
            prof_end(c);
            prof_begin(c, BSCGPU_K_RADIX_SCAN, (u64)256 * num_tiles8k * 8, 0);
            hipLaunchKernelGGL(rs_scan_kernel, dim3(256), dim3(WG), 0, c->stream, c->tile_counts, num_tiles8k, c->rowtot);
            prof_end(c);
            prof_begin(c, BSCGPU_K_RADIX_SCATTER, 2 * n * rec_bytes, n);
            hipLaunchKernelGGL(rs_scatter_tiled_kernel<true>, dim3(256), dim3(RSB_WG), RST_LDS, c->stream,
                               ksrc, kdst, vsrc, vdst, (u32)n, shift, mask, num_tiles8k, c->tile_counts, c->rowtot);
            prof_end(c);
            HIP_TRY(c, hipGetLastError());
            u64* tk = ksrc; ksrc = kdst; kdst = tk;
            u32* tv = vsrc; vsrc = vdst; vdst = tv;
            continue;
        }
        prof_begin(c, kind_hist, n * 8, n);
        hipLaunchKernelGGL(rs_hist_kernel, dim3(ch.num_chunks), dim3(RS_WG), 0, c->stream,
                           ksrc, (u32)n, shift, mask, ch.chunk_tiles, ch.num_chunks, c->counts);
        prof_end(c);

        prof_begin(c, kind_scan, (u64)256 * ch.num_chunks * 8, 0);
        hipLaunchKernelGGL(rs_scan_kernel, dim3(256), dim3(WG), 0, c->stream, c->counts, ch.num_chunks, c->rowtot);
        prof_end(c);

        prof_begin(c, kind_scatter, 2 * n * rec_bytes + (emit_pos ? 4 * n : 0), n);
        if (has_val)
            hipLaunchKernelGGL((rs_scatter_kernel<true>), dim3(ch.num_chunks), dim3(RS_WG), RS_LDS, c->stream,
                               ksrc, kdst, vsrc, vdst, (u32)n, shift, mask, ch.chunk_tiles, ch.num_chunks,
                               ch.num_tiles, c->counts, c->rowtot, c->wc_sink);
        else if (emit_pos != nullptr)
            hipLaunchKernelGGL((rs_scatter_kernel<false, true>), dim3(ch.num_chunks), dim3(RS_WG), RS_LDS, c->stream,
                               ksrc, kdst, (const u32*)nullptr, (u32*)nullptr, (u32)n, shift, mask,
                               ch.chunk_tiles, ch.num_chunks, ch.num_tiles, c->counts, c->rowtot, c->wc_sink, emit_pos);
        else
            hipLaunchKernelGGL((rs_scatter_kernel<false>), dim3(ch.num_chunks), dim3(RS_WG), RS_LDS, c->stream,
                               ksrc, kdst, (const u32*)nullptr, (u32*)nullptr, (u32)n, shift, mask,
                               ch.chunk_tiles, ch.num_chunks, ch.num_tiles, c->counts, c->rowtot, c->wc_sink, (u32*)nullptr);
        prof_end(c);
        HIP_TRY(c, hipGetLastError());

        u64* tk = ksrc; ksrc = kdst; kdst = tk;
        u32* tv = vsrc; vsrc = vdst; vdst = tv;
    }
#if RS_PHASE_TIMING
    if (n >= (1u << 24)) {      // debug builds: phase stamps of the last pass
        static std::vector<u64> host(256 * 32 * 16);
        if (hipStreamSynchronize(c->stream) == hipSuccess && hipMemcpy(host.data(), c->wc_sink, host.size() * 8, hipMemcpyDeviceToHost) == hipSuccess) {
            if (FILE* f = fopen("gpurun_out/phase_timing.bin", "wb")) { fwrite(host.data(), 8, host.size(), f); fclose(f); }
        }
    }
#endif
    *in_alt = (npasses & 1);
    return BSC_NO_ERROR;
}
