// rangecoder.hip — the range coder of the static / fast coders on the GPU: many probability streams in one launch
// (include/bscgpu.h: bscgpu_rc_encode*).
//
// A range coder cannot be bracketed or composed: a stream is one serial chain.  So one LANE codes one stream, and the
// launch is as wide as there are streams: 8 for the sub-blocks of a single block, thousands for the sub-block streams of a pass.
// The arithmetic is the host's (csrc/host/qlfc.cpp RangeEncoder = rangecoder.h:38-271): 64-bit low with the carry in bit 32, 32-bit
// range, the cached unit and the count of pending 0xffff units, 16-bit little-endian output.
//
// Shape of a workgroup = one wavefront (64 threads), SPW = 64, 8 or 1 streams per wavefront; all three run rc_step below.
//   input    every stream's next RC_REFILL decisions (prefix entries: RC_REFILL / 2) are staged in LDS by the WHOLE wavefront with aligned
//            16-byte loads (consecutive lanes take consecutive pieces of one stream), whatever the alignment of the stream's first
//            entry; a lane then reads its own row, one entry ahead of the step that uses it (the LDS latency is off the chain)
//   output   16-bit units go to a 64-byte LDS ring per lane that mirrors the low address bits of the output; each completed, aligned
//            32-byte half leaves as two 16-byte vector stores.  Only a stream's first and last piece (region starts are merely even)
//            leave as 16-bit stores.
//   bounds   a renormalisation that could carry a stream past out_size + 64 bytes ends the stream (LIBBSC_NOT_COMPRESSIBLE): nothing is
//            ever stored outside out[out_off, out_off + out_size + 64).  The loops are bounded by the streams' counts.
// Plain C++: no inline assembly, no atomics, every store a vector store.
#include "dev_common.h"

namespace {

constexpr int RC_R        = BSCGPU_RC_REFILL;       // body decisions per refill
constexpr int RC_RP       = RC_R / 2;               // prefix entries (u32) per refill: the same bytes
constexpr int RC_PIECES   = RC_R * 2 / 16 + 1;      // aligned 16-byte pieces that cover 2 RC_R bytes at any alignment
constexpr int RC_IN_ROW   = RC_PIECES * 4 + 1;      // dwords per row: odd, so the lanes' rows start on different banks
constexpr int RC_OUT_ROW  = 17;                     // dwords: the 64-byte ring + 1, for the same reason
static_assert(RC_R % 8 == 0 && RC_R * 13 / 8 + 15 + 8 <= RC_PIECES * 16, "a packed refill fits the row, with the two-dword read of its last field");

typedef u32 u32x4 __attribute__((ext_vector_type(4)));

struct RcLane {
    u64 low; u32 range, cache, held;
    u32 written;        // bytes put out so far (into the ring or beyond)
    u32 flushed;        // ... of which have left the ring
    u32 fail;
};

// what a lane needs to store: its region in global memory, its ring in LDS, and the ring position of the region's first byte
struct RcOut { u8* g; u8* ring; u32 a0; bool store; };

__device__ __forceinline__ void rc_flush(RcLane& s, const RcOut& o, u32 upto)
{
    // bytes [s.flushed, upto) of the stream leave the ring.  A whole half of the ring is 32 bytes at a 32-byte-aligned address.
    const u32 lo = s.flushed;
    if (o.store) {
        if (upto - lo == 32u && ((o.a0 + lo) & 31u) == 0u) {
            const u32* r = reinterpret_cast<const u32*>(o.ring + ((o.a0 + lo) & 32u));
            uint4 v0 = make_uint4(r[0], r[1], r[2], r[3]), v1 = make_uint4(r[4], r[5], r[6], r[7]);
            uint4* g = reinterpret_cast<uint4*>(o.g + lo);
            g[0] = v0; g[1] = v1;
        } else {
            for (u32 k = lo; k < upto; k += 2) *reinterpret_cast<u16*>(o.g + k) = *reinterpret_cast<const u16*>(o.ring + ((o.a0 + k) & 63u));
        }
    }
    s.flushed = upto;
}

__device__ __forceinline__ void rc_put16(RcLane& s, const RcOut& o, u32 v)
{
    const u32 pos = o.a0 + s.written;
    *reinterpret_cast<u16*>(o.ring + (pos & 63u)) = (u16)v;
    s.written += 2;
    if (((pos + 2u) & 31u) == 0u) rc_flush(s, o, s.written);
}

// rangecoder.h ShiftLow: release the cached unit (and the pending ones behind it) unless the new unit is 0xffff without a carry
__device__ __forceinline__ void rc_shift(RcLane& s, const RcOut& o)
{
    const u32 low32 = (u32)s.low, carry = (u32)(s.low >> 32);
    if (low32 < 0xffff0000u || carry) {
        u32 v = s.cache + carry;
        for (u32 k = s.held + 1u; k; --k) { rc_put16(s, o, v); v = carry - 1u; }      // 0xffff without a carry, 0x0000 after one
        s.held = 0;
        s.cache = low32 >> 16;
    } else {
        ++s.held;
    }
    s.low = (u64)(u32)(low32 << 16);
}

// bytes the state will put out once its cached unit and its pending units are released
__device__ __forceinline__ u32 rc_committed(const RcLane& s) { return s.written + 2u * s.held + 2u; }

// one decision: the step function of every launch shape
__device__ __forceinline__ void rc_step(RcLane& s, const RcOut& o, u32 region, u32 bit, u32 p, u32 prec)
{
    if (s.range < 0x10000u) {
        if (rc_committed(s) + 8u > region) { s.fail = 1; return; }
        rc_shift(s, o);
        s.range <<= 16;
    }
    const u32 r = (s.range >> prec) * p;
    s.low  += bit ? (u64)r : 0ull;
    s.range = bit ? s.range - r : r;
}

enum : u32 { KIND_NONE = 0, KIND_PREFIX = 1, KIND_BODY = 2 };

// entry i of the lane's staged row, raw: a prefix entry, a 16-bit entry or a 13-bit field
template <int FORM>
__device__ __forceinline__ u32 rc_fetch(const u8* row, u32 off, u32 kind, u32 i)
{
    if (kind == KIND_PREFIX) return *reinterpret_cast<const u32*>(row + off + 4u * min(i, (u32)RC_RP));      // (a wavefront's step count follows its body lanes)
    if (FORM == BSCGPU_RC_STATIC13) {
        const u32 bit = 13u * i, at = off + (bit >> 3);
        const u32* w = reinterpret_cast<const u32*>(row) + (at >> 2);
        const u64 two = ((u64)w[1] << 32) | w[0];
        return (u32)(two >> (((at & 3u) << 3) + (bit & 7u))) & 0x1fffu;
    }
    return *reinterpret_cast<const u16*>(row + off + 2u * i);
}

template <int SPW, int FORM>
__global__ void __launch_bounds__(64)
rc_encode_kernel(const u8* __restrict__ body, const u32* __restrict__ prefix, const bscgpu_rc_stream* __restrict__ streams, int count,
                 u8* __restrict__ out, int* __restrict__ res)
{
    // one array: rows of staged input, output rings, and the byte range every stream wants staged next
    __shared__ __attribute__((aligned(16))) u32 lds[SPW * (RC_IN_ROW + RC_OUT_ROW) + 4 * SPW];
    u32* in_rows = lds;
    u32* rings   = lds + SPW * RC_IN_ROW;
    u64* want    = reinterpret_cast<u64*>(lds + SPW * (RC_IN_ROW + RC_OUT_ROW));      // [SPW][2]: first and one-past-last byte address

    const u32 lane = threadIdx.x;
    const u32 slot = SPW == 1 ? 0u : lane;                                         // at SPW 1 every lane follows the one stream: the chain is wave-uniform
    const int sidx = (int)blockIdx.x * SPW + (int)slot;
    const bool mine = (SPW == 1 || lane < (u32)SPW) && sidx < count;

    bscgpu_rc_stream S;
    S.body = 0; S.count = 0; S.prefix = 0; S.nprefix = 0; S.out_off = 0; S.out_size = 0;
    if (mine) S = streams[sidx];
    const u32 npc = (S.nprefix + RC_RP - 1) / RC_RP, nbc = (S.count + RC_R - 1) / RC_R;
    const u32 nch = mine ? npc + nbc : 0u;
    const u32 maxch = __builtin_amdgcn_readlane(wave_incl_max(nch), 63);

    RcLane s;
    s.low = 0; s.range = 0xffffffffu; s.cache = 0; s.held = 0; s.written = 0; s.flushed = 0; s.fail = 0;
    RcOut o;
    o.g = out + S.out_off;
    o.ring = reinterpret_cast<u8*>(rings + slot * RC_OUT_ROW);
    o.a0 = (u32)(reinterpret_cast<uintptr_t>(o.g) & 63u);
    o.store = mine && (SPW != 1 || lane == 0);
    const u32 region = (u32)S.out_size + 64u;
    const int budget = S.out_size - 16;                                            // rangecoder.h:127
    const u8* row = reinterpret_cast<const u8*>(in_rows + slot * RC_IN_ROW);
    const u64 pbase = reinterpret_cast<u64>(prefix), bbase = reinterpret_cast<u64>(body);

    for (u32 c = 0; c < maxch; ++c) {
        // ---- what this lane's stream wants staged: chunk c of prefix-then-body
        u32 kind = KIND_NONE, n = 0;
        u64 lo = 0, hi = 0;
        if (c < nch && !s.fail) {
            if (c < npc) {
                kind = KIND_PREFIX;
                n = min((u32)RC_RP, S.nprefix - c * RC_RP);
                lo = pbase + 4ull * ((u64)S.prefix + (u64)c * RC_RP);
                hi = lo + 4ull * n;
            } else {
                const u32 k = c - npc;
                kind = KIND_BODY;
                n = min((u32)RC_R, S.count - k * RC_R);
                if (FORM == BSCGPU_RC_STATIC13) { lo = bbase + ((u64)S.body + (u64)k * RC_R) / 8u * 13u; hi = lo + (13ull * n + 7u) / 8u; }
                else                            { lo = bbase + 2ull * ((u64)S.body + (u64)k * RC_R);     hi = lo + 2ull * n; }
            }
        }
        if (lane < (u32)SPW) { want[2 * lane] = lo; want[2 * lane + 1] = hi; }
        __syncthreads();
        // ---- the wavefront stages all rows: piece q of stream t is the aligned 16 bytes at (lo_t & ~15) + 16 q, loaded only while it
        //      holds a byte of [lo_t, hi_t)
        for (u32 item = lane; item < (u32)(SPW * RC_PIECES); item += 64u) {
            const u32 t = item / RC_PIECES, q = item - t * RC_PIECES;
            const u64 tlo = want[2 * t], thi = want[2 * t + 1];
            const u64 a = (tlo & ~15ull) + 16ull * q;
            if (a < thi) {
                const u32x4 v = *reinterpret_cast<const __attribute__((address_space(1))) u32x4*>(a);
                u32* d = in_rows + t * RC_IN_ROW + 4u * q;
                d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
            }
        }
        __syncthreads();
        // ---- every lane codes its staged entries; lanes with fewer (or none) idle
        const u32 off = (u32)(lo & 15ull);
        const u32 nmax = __builtin_amdgcn_readlane(wave_incl_max(n), 63);
        u32 x = rc_fetch<FORM>(row, off, kind, 0);
        for (u32 i = 0; i < nmax; ++i) {
            const u32 xn = rc_fetch<FORM>(row, off, kind, i + 1);                  // (one past the last entry stays inside the row)
            if (i < n && !s.fail) {
                u32 e = x;
                if (SPW == 1) e = __builtin_amdgcn_readfirstlane(e);
                u32 bit, p, prec, stop = 0;
                const u32 full = (int)s.written >= budget ? 1u : 0u;
                if (kind == KIND_PREFIX)               { p = e & 0xffffu; prec = (e >> 16) & 31u; bit = (e >> 24) & 1u; }
                else if (FORM == BSCGPU_RC_STATIC16)   { p = e & 0xfffu;  prec = 12u; bit = (e >> 12) & 1u; stop = (e >> 13) & full; }
                else if (FORM == BSCGPU_RC_STATIC13)   { p = e & 0xfffu;  prec = 12u; bit = e >> 12; stop = full; }
                else                                   { p = e & 0x1fffu; prec = 13u - ((e >> 15) << 1); bit = (e >> 13) & 1u; stop = (e >> 14) & full; }
                if (stop & 1u) s.fail = 1;
                else rc_step(s, o, region, bit, p, prec);
            }
            x = xn;
        }
    }

    // ---- finish: one conditional and three unconditional shifts, then what is left in the ring
    if (mine) {
        if (!s.fail && rc_committed(s) + 8u > region) s.fail = 1;
        if (!s.fail) {
            const u32 shifts = s.range < 0x10000u ? 4u : 3u;
            for (u32 k = 0; k < shifts; ++k) rc_shift(s, o);
            if (s.flushed < s.written) rc_flush(s, o, s.written);
        }
        if (o.store) res[sidx] = s.fail ? BSC_NOT_COMPRESSIBLE : (int)s.written;
    }
}

template <int SPW>
void rc_launch(int form, int blocks, hipStream_t st, const u8* body, const u32* prefix, const bscgpu_rc_stream* streams, int count, u8* out, int* res)
{
    if (form == BSCGPU_RC_STATIC16)      hipLaunchKernelGGL((rc_encode_kernel<SPW, BSCGPU_RC_STATIC16>), dim3(blocks), dim3(64), 0, st, body, prefix, streams, count, out, res);
    else if (form == BSCGPU_RC_STATIC13) hipLaunchKernelGGL((rc_encode_kernel<SPW, BSCGPU_RC_STATIC13>), dim3(blocks), dim3(64), 0, st, body, prefix, streams, count, out, res);
    else                                 hipLaunchKernelGGL((rc_encode_kernel<SPW, BSCGPU_RC_FAST16>),   dim3(blocks), dim3(64), 0, st, body, prefix, streams, count, out, res);
}

size_t rc_align(size_t x) { return (x + 255) & ~(size_t)255; }

}  // namespace

int rc_encode_device(bscgpu_ctx* c, int form, const void* dBody, const u32* prefix, int nprefix_total, const bscgpu_rc_stream* streams,
                     int count, void* dOut, int* res, int spw)
{
    if (count == 0) return BSC_NO_ERROR;
    // stream table, prefix entries, results: one device buffer that grows on demand
    const size_t o_streams = 0, o_prefix = rc_align((size_t)count * sizeof(bscgpu_rc_stream));
    const size_t o_res = o_prefix + rc_align((size_t)nprefix_total * 4 + 16), need = o_res + rc_align((size_t)count * 4);
    if (c->rc_tab_bytes < need) {
        HIP_TRY(c, ctx_sync(c));
        if (c->rc_tab) { (void)hipFree(c->rc_tab); c->rc_tab = nullptr; c->rc_tab_bytes = 0; }
        const size_t cap = need + need / 2;
        if (hipMalloc((void**)&c->rc_tab, cap) != hipSuccess) { (void)hipGetLastError(); return ctx_fail(c, BSC_GPU_NOT_ENOUGH_MEMORY, "range coder: stream table", hipSuccess); }
        c->rc_tab_bytes = cap;
    }
    HIP_TRY(c, hipMemcpyAsync(c->rc_tab + o_streams, streams, (size_t)count * sizeof(bscgpu_rc_stream), hipMemcpyHostToDevice, c->stream));
    if (nprefix_total > 0) HIP_TRY(c, hipMemcpyAsync(c->rc_tab + o_prefix, prefix, (size_t)nprefix_total * 4, hipMemcpyHostToDevice, c->stream));
    const int blocks = (count + spw - 1) / spw;
    u64 decisions = 0;
    for (int i = 0; i < count; ++i) decisions += (u64)streams[i].count + streams[i].nprefix;
    const bscgpu_rc_stream* dS = reinterpret_cast<const bscgpu_rc_stream*>(c->rc_tab + o_streams);
    const u32* dP = reinterpret_cast<const u32*>(c->rc_tab + o_prefix);
    int* dR = reinterpret_cast<int*>(c->rc_tab + o_res);
    prof_begin(c, BSCGPU_K_RC, decisions * (form == BSCGPU_RC_STATIC13 ? 13 : 16) / 8, decisions);
    if (spw == 64)     rc_launch<64>(form, blocks, c->stream, (const u8*)dBody, dP, dS, count, (u8*)dOut, dR);
    else if (spw == 8) rc_launch<8>(form, blocks, c->stream, (const u8*)dBody, dP, dS, count, (u8*)dOut, dR);
    else               rc_launch<1>(form, blocks, c->stream, (const u8*)dBody, dP, dS, count, (u8*)dOut, dR);
    prof_end(c);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(res, dR, (size_t)count * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, ctx_sync(c));
    prof_collect(c);
    return BSC_NO_ERROR;
}

static int rc_args_ok(bscgpu_ctx* c, const void* body, const u32* prefix, int nprefix_total, const bscgpu_rc_stream* streams, int count,
                      const void* out, const int* res, int spw)
{
    if (!c || (spw != 64 && spw != 8 && spw != 1)) return 0;
    if (count > 0 && (!out || !res || (nprefix_total > 0 && !prefix) || (reinterpret_cast<uintptr_t>(out) & 1u))) return 0;
    for (int i = 0; i < count; ++i) if (streams[i].count > 0 && (!body || (reinterpret_cast<uintptr_t>(body) & 1u))) return 0;
    return 1;
}

extern "C" int bscgpu_rc_encode_device(bscgpu_ctx* c, int form, const void* dBody, const uint32_t* prefix, int nprefix_total,
                                       const bscgpu_rc_stream* streams, int count, void* dOut, int* res, int spw)
{
    if (bscgpu_rc_check(form, nprefix_total, streams, count, -1, -1) != BSC_NO_ERROR) return BSC_BAD_PARAMETER;
    if (!rc_args_ok(c, dBody, prefix, nprefix_total, streams, count, dOut, res, spw)) return BSC_BAD_PARAMETER;
    if (hipSetDevice(c->device) != hipSuccess) return BSC_GPU_ERROR;
    return rc_encode_device(c, form, dBody, prefix, nprefix_total, streams, count, dOut, res, spw);
}

extern "C" int bscgpu_rc_encode(bscgpu_ctx* c, int form, const void* body, int64_t body_bytes, const uint32_t* prefix, int nprefix_total,
                                const bscgpu_rc_stream* streams, int count, void* out, int64_t out_bytes, int* res, int spw)
{
    if (body_bytes < 0 || out_bytes < 0 || bscgpu_rc_check(form, nprefix_total, streams, count, body_bytes, out_bytes) != BSC_NO_ERROR) return BSC_BAD_PARAMETER;
    if (!rc_args_ok(c, body, prefix, nprefix_total, streams, count, out, res, spw)) return BSC_BAD_PARAMETER;
    if (count == 0) return BSC_NO_ERROR;
    if (hipSetDevice(c->device) != hipSuccess) return BSC_GPU_ERROR;
    u8* d = nullptr;
    const size_t ob = rc_align((size_t)body_bytes + 16);
    if (hipMalloc((void**)&d, ob + (size_t)out_bytes + 16) != hipSuccess) { (void)hipGetLastError(); return ctx_fail(c, BSC_GPU_NOT_ENOUGH_MEMORY, "range coder: staging", hipSuccess); }
    int rc = BSC_NO_ERROR;
    // (the caller's out bytes go up first: what no stream writes comes back unchanged)
    if ((body_bytes > 0 && hipMemcpyAsync(d, body, (size_t)body_bytes, hipMemcpyHostToDevice, c->stream) != hipSuccess) ||
        (out_bytes > 0 && hipMemcpyAsync(d + ob, out, (size_t)out_bytes, hipMemcpyHostToDevice, c->stream) != hipSuccess)) rc = BSC_GPU_ERROR;
    if (rc == BSC_NO_ERROR) rc = rc_encode_device(c, form, d, prefix, nprefix_total, streams, count, d + ob, res, spw);
    if (rc == BSC_NO_ERROR && out_bytes > 0 && hipMemcpy(out, d + ob, (size_t)out_bytes, hipMemcpyDeviceToHost) != hipSuccess) rc = BSC_GPU_ERROR;
    (void)hipFree(d);
    return rc;
}
