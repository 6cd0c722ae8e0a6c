// batch_decode.cpp — batched decompression (bscgpu_decompress_batch*, bscgpu_unbwt_batch_plan; include/bscgpu.h).
//
// BWT blocks that fit the context go through PASSES: their QLFC payloads are decoded on the host threads into one pinned staging
// buffer per pass, and the pass's inverse BWT is ONE GPU pass (unbwt.hip: unbwt_batch_pass) whose segmented Adler-32 checks every
// block without LZP.  The QLFC decoding of pass k + 1 overlaps the GPU work of pass k.  Every other block, and every block that is
// not clean (a checksum, a decoder or the GPU chain check says so), is decoded by bsc_decompress itself: results[b] is then its
// own return value by construction.
#include <cstring>
#include <memory>
#include <system_error>
#include <thread>
#include <vector>
#include <hip/hip_runtime.h>

#include "../../../include/libbsc.h"
#include "../../../include/bscgpu.h"
#include "../device/dev_common.h"
#include "qlfc.h"
#include "lzp.h"
#include "container.h"
#include "par.h"

using namespace bschost;

extern "C" BSCGPU_API int bscgpu_unbwt_batch_plan(const int* sizes, int count, int64_t cap, int* pass_of)
{
    if (count < 0 || cap < 0 || (count > 0 && (!sizes || !pass_of))) return LIBBSC_BAD_PARAMETER;
    for (int b = 0; b < count; ++b) if (sizes[b] < -1) return LIBBSC_BAD_PARAMETER;
    const int lim = unbwt_batch_max_blocks(cap);
    int passes = 0, members = 0;
    int64_t bytes = 0;
    for (int b = 0; b < count; ++b) {
        const int n = sizes[b];
        if (n < 2 || n > cap) { pass_of[b] = -1; continue; }      // (another route's block does not end a pass: the staging layout is the pass's own)
        if (passes == 0 || bytes + n > cap || members + 1 > lim) { ++passes; bytes = 0; members = 0; }
        pass_of[b] = passes - 1; bytes += n; ++members;
    }
    return passes;
}

// data_sizes[b] from the headers (0 where bsc_block_info refuses one); in_sizes already checked
static int64_t data_sizes_of(const unsigned char* input, const int* in_sizes, int count, int* data_sizes)
{
    int64_t total = 0, o = 0;
    for (int b = 0; b < count; ++b) {
        int bs = 0, ds = 0;
        data_sizes[b] = (in_sizes[b] > 0 && bsc_block_info(input + o, in_sizes[b], &bs, &ds, 0) == LIBBSC_NO_ERROR) ? ds : 0;
        total += data_sizes[b]; o += in_sizes[b];
    }
    return total;
}

static int input_args(const unsigned char* input, const int* in_sizes, int count)
{
    if (count < 0 || (count > 0 && !in_sizes)) return LIBBSC_BAD_PARAMETER;
    int64_t total = 0;
    for (int b = 0; b < count; ++b) { if (in_sizes[b] < 0) return LIBBSC_BAD_PARAMETER; total += in_sizes[b]; }
    if (total > 0 && !input) return LIBBSC_BAD_PARAMETER;
    return LIBBSC_NO_ERROR;
}

extern "C" BSCGPU_API int64_t bscgpu_decompress_batch_sizes(const unsigned char* input, const int* in_sizes, int count, int* data_sizes)
{
    const int rc = input_args(input, in_sizes, count);
    if (rc < 0) return rc;
    if (count > 0 && !data_sizes) return LIBBSC_BAD_PARAMETER;
    return data_sizes_of(input, in_sizes, count, data_sizes);
}

namespace {
struct Pass {
    std::vector<int> m;                  // its blocks, in input order
    std::vector<int64_t> at;             // where block m[i]'s QLFC output starts in the staging buffer (bound layout, then compacted)
    std::vector<int> lz, idx;            // its BWT length and primary index; idx 0: not clean, left to bsc_decompress
};
}

// One implementation for both entry points: output in host memory (`output`) or in HBM (`dOut`).
static int decompress_batch_impl(bscgpu_ctx* c, const unsigned char* input, const int* in_sizes, int count, unsigned char* output,
                                 unsigned char* dOut, int* results, int features, const std::vector<int>& ds)
{
    const bool dev = dOut != nullptr;
    std::vector<int64_t> in_off((size_t)count + 1, 0), out_off((size_t)count + 1, 0);
    std::vector<int> bound((size_t)count, -1), pass_of((size_t)count);
    std::vector<BlockFields> hdr((size_t)count);                    // of the blocks with a bound
    for (int b = 0; b < count; ++b) {
        in_off[b + 1] = in_off[b] + in_sizes[b];
        out_off[b + 1] = out_off[b] + ds[b];
        const unsigned char* in = input + in_off[b];
        int bs = 0, d = 0;
        if (in_sizes[b] >= LIBBSC_HEADER_SIZE && bsc_block_info(in, in_sizes[b], &bs, &d, features) == LIBBSC_NO_ERROR
            && in_sizes[b] >= bs && block_header_read(in, &hdr[b]) && block_holds_payload(hdr[b]) && block_mode_unpack(hdr[b].mode).sorter == LIBBSC_BLOCKSORTER_BWT)
            bound[b] = d;                                        // the QLFC decoders write at most dataSize bytes (bsc_decompress's bound)
    }
    const int npass = bscgpu_unbwt_batch_plan(bound.data(), count, c->max_n, pass_of.data());
    if (npass < 0) return npass;
    std::vector<char> own((size_t)count, 0);
    for (int b = 0; b < count; ++b) own[b] = pass_of[b] < 0;
    if (npass > 0) {
        if (hipSetDevice(c->device) != hipSuccess) return LIBBSC_GPU_ERROR;
        for (int k = 0; k < 2; ++k)
            if (!c->batch_host[k] && hipHostMalloc((void**)&c->batch_host[k], (size_t)c->max_n + 64, hipHostMallocDefault) != hipSuccess) {
                c->batch_host[k] = nullptr;
                return ctx_fail(c, LIBBSC_GPU_NOT_ENOUGH_MEMORY, "batched decompression: pinned pass buffers", hipSuccess);
            }
    }
    const int threads = coder_threads();
    std::vector<std::vector<int>> members((size_t)npass);
    for (int b = 0; b < count; ++b) if (pass_of[b] >= 0) members[pass_of[b]].push_back(b);
    Pass ps[2];

    // host: the checks bsc_decompress makes before the inverse transform, and the QLFC decoders, into the staging buffer
    auto decode = [&](int p) {
        Pass& P = ps[p & 1];
        u8* hb = c->batch_host[p & 1];
        P.m = members[p];
        const int k = (int)P.m.size();
        P.at.assign((size_t)k, 0); P.lz.assign((size_t)k, 0); P.idx.assign((size_t)k, 0);
        for (int i = 1; i < k; ++i) P.at[i] = P.at[i - 1] + bound[P.m[i - 1]];
        // many blocks: they are the parallelism; a few large ones: their sub-blocks are (same bytes either way)
        const int qf = k < threads ? features : features & ~LIBBSC_FEATURE_MULTITHREADING;
        run_bounded(k, threads, [&](int i) {
            const int b = P.m[i];
            CodedPayload pay;
            if (block_coded_payload(input + in_off[b], hdr[b], &pay) != LIBBSC_NO_ERROR) return;
            const int lz = coder_decompress_bounded(pay.data, pay.size, hb + P.at[i], block_mode_unpack(hdr[b].mode).coder, qf, bound[b]);
            const int index = hdr[b].index;
            if (lz < 2 || index <= 0 || index > lz) return;
            P.lz[i] = lz; P.idx[i] = index;
        });
        int64_t q = 0;                                              // compact: the pass's L back to back
        for (int i = 0; i < k; ++i) {
            if (!P.idx[i]) { own[P.m[i]] = 1; continue; }
            if (q != P.at[i]) memmove(hb + q, hb + P.at[i], (size_t)P.lz[i]);
            P.at[i] = q; q += P.lz[i];
        }
    };

    // GPU: one inverse-BWT pass; host: LZP, size and checksum of every block
    std::vector<int> sz, idx, res;
    std::vector<u32> dst, adl;
    auto finish = [&](int p) -> int {
        Pass& P = ps[p & 1];
        u8* hb = c->batch_host[p & 1];
        std::vector<int> g;                                         // the clean blocks of the pass
        for (int i = 0; i < (int)P.m.size(); ++i) if (P.idx[i]) g.push_back(i);
        if (g.empty()) return LIBBSC_NO_ERROR;
        const int k = (int)g.size();
        sz.resize(k); idx.resize(k); res.resize(k); dst.resize(k); adl.resize(k);
        const int64_t base = out_off[P.m[g[0]]], last = P.m[g[k - 1]];
        const bool direct = dev && out_off[last] + P.lz[g[k - 1]] - base < 0xffffffffll;   // the walk writes into the caller's HBM
        int64_t total = 0;
        for (int j = 0; j < k; ++j) {
            const int i = g[j];
            sz[j] = P.lz[i]; idx[j] = P.idx[i];
            dst[j] = direct ? (u32)(out_off[P.m[i]] - base) : (u32)P.at[i];
            total += P.lz[i];
        }
        if (hipMemcpyAsync(c->dT, hb, (size_t)total, hipMemcpyHostToDevice, c->stream) != hipSuccess) return LIBBSC_GPU_ERROR;
        u8* out = direct ? dOut + base : c->dL;
        const int rc = unbwt_batch_pass(c, c->dT, out, sz.data(), idx.data(), k, dst.data(), res.data(), adl.data(), dev ? nullptr : hb);
        if (rc < 0) return rc;
        bool sync = false;
        for (int j = 0; j < k; ++j) {
            const int i = g[j], b = P.m[i];
            if (res[j] != LIBBSC_NO_ERROR) continue;
            const bool lzp = block_mode_has_lzp(hdr[b].mode);
            hipError_t e = hipSuccess;
            if (dev && lzp) e = hipMemcpyAsync(hb + P.at[i], out + dst[j], (size_t)P.lz[i], hipMemcpyDeviceToHost, c->stream);
            else if (dev && !direct) e = hipMemcpyAsync(dOut + out_off[b], out + dst[j], (size_t)P.lz[i], hipMemcpyDeviceToDevice, c->stream);
            if (e != hipSuccess) return LIBBSC_GPU_ERROR;
            sync = sync || dev;
        }
        if (sync && ctx_sync(c) != hipSuccess) return LIBBSC_GPU_ERROR;
        std::vector<unsigned char*> up((size_t)k, nullptr);           // device output: LZP blocks decoded on the host, going up
        run_bounded(k, threads, [&](int j) {
            const int i = g[j], b = P.m[i];
            if (res[j] != LIBBSC_NO_ERROR) { own[b] = 1; return; }   // DATA_CORRUPT / NOT_SUPPORTED: bsc_decompress decides
            const BlockMode m = block_mode_unpack(hdr[b].mode);
            const int lzpHashSize = m.lzp_hash, lzpMinLen = m.lzp_min, n = ds[b];
            const unsigned adler_data = hdr[b].adler_data;
            if (lzpHashSize == 0 && lzpMinLen == 0) {
                if (P.lz[i] != n) { results[b] = LIBBSC_DATA_CORRUPT; return; }
                if (!dev) memcpy(output + out_off[b], hb + P.at[i], (size_t)n);
                results[b] = adl[j] == adler_data ? LIBBSC_NO_ERROR : LIBBSC_DATA_CORRUPT;
                return;
            }
            unsigned char* to = dev ? (unsigned char*)bigbuf_get((size_t)n + 1) : output + out_off[b];
            if (!to) { results[b] = LIBBSC_NOT_ENOUGH_MEMORY; return; }
            int r = lzp_decompress(hb + P.at[i], to, P.lz[i], n, lzpHashSize, lzpMinLen);
            if (r >= LIBBSC_NO_ERROR) r = (r != n || adler_data != adler32(to, (size_t)n)) ? LIBBSC_DATA_CORRUPT : LIBBSC_NO_ERROR;
            results[b] = r;
            if (dev) { if (r == LIBBSC_NO_ERROR) up[j] = to; else bigbuf_put(to); }
        });
        int urc = LIBBSC_NO_ERROR;
        for (int j = 0; j < k; ++j) {
            if (!up[j]) continue;
            const int b = P.m[g[j]];
            if (urc == LIBBSC_NO_ERROR && hipMemcpyAsync(dOut + out_off[b], up[j], (size_t)ds[b], hipMemcpyHostToDevice, c->stream) != hipSuccess) urc = LIBBSC_GPU_ERROR;
        }
        if (urc == LIBBSC_NO_ERROR && ctx_sync(c) != hipSuccess) urc = LIBBSC_GPU_ERROR;
        for (auto* q : up) bigbuf_put(q);
        return urc;
    };

    int rc = LIBBSC_NO_ERROR;
    if (npass > 0) decode(0);
    for (int p = 0; p < npass && rc >= 0; ++p) {
        std::thread next;                                           // decodes pass p + 1 while pass p is on the GPU
        if (p + 1 < npass) {
            try { next = std::thread(decode, p + 1); }
            catch (const std::system_error&) {}                     // no thread to be had: decoded after this pass, here
        }
        rc = finish(p);
        if (next.joinable()) next.join();
        else if (p + 1 < npass) decode(p + 1);
    }
    if (rc < 0) return rc;

    // blocks of their own (stored, ST3..ST8, larger than the context, not clean): bsc_decompress as it is
    std::vector<int> rest;
    for (int b = 0; b < count; ++b) if (own[b]) rest.push_back(b);
    run_bounded((int)rest.size(), threads, [&](int j) {
        const int b = rest[j];
        const unsigned char* in = input + in_off[b];
        if (!dev) { results[b] = bsc_decompress(in, in_sizes[b], output + out_off[b], ds[b], features); return; }
        unsigned char* tmp = (unsigned char*)bigbuf_get((size_t)ds[b] + 1);
        if (!tmp) { results[b] = LIBBSC_NOT_ENOUGH_MEMORY; return; }
        int r = bsc_decompress(in, in_sizes[b], tmp, ds[b], features);
        if (r == LIBBSC_NO_ERROR && ds[b] > 0 && (hipSetDevice(c->device) != hipSuccess || hipMemcpy(dOut + out_off[b], tmp, (size_t)ds[b], hipMemcpyHostToDevice) != hipSuccess))
            r = LIBBSC_GPU_ERROR;
        results[b] = r;
        bigbuf_put(tmp);
    });
    return LIBBSC_NO_ERROR;
}

// refused calls write nothing: every argument is checked, the headers read, before the first byte goes out
static int decompress_batch_entry(bscgpu_ctx* c, const unsigned char* input, const int* in_sizes, int count, unsigned char* out, bool dev,
                                  int64_t out_cap, int* results, int features)
{
    if (!c || input_args(input, in_sizes, count) < 0 || (count > 0 && !results)) return LIBBSC_BAD_PARAMETER;
    std::vector<int> ds((size_t)count);
    const int64_t total = data_sizes_of(input, in_sizes, count, ds.data());
    if (out_cap < total || (total > 0 && !out)) return LIBBSC_BAD_PARAMETER;
    if (count == 0) return LIBBSC_NO_ERROR;
    static unsigned char empty = 0;              // (a batch that decodes to nothing may come with no buffer at all)
    if (!out) out = &empty;
    return decompress_batch_impl(c, input, in_sizes, count, dev ? nullptr : out, dev ? out : nullptr, results, features, ds);
}

extern "C" BSCGPU_API int bscgpu_decompress_batch(bscgpu_ctx* c, const unsigned char* input, const int* in_sizes, int count,
                                                  unsigned char* output, int64_t out_cap, int* results, int features)
{
    return decompress_batch_entry(c, input, in_sizes, count, output, false, out_cap, results, features);
}

extern "C" BSCGPU_API int bscgpu_decompress_batch_device(bscgpu_ctx* c, const unsigned char* input, const int* in_sizes, int count,
                                                         void* dOutput, int64_t out_cap, int* results, int features)
{
    return decompress_batch_entry(c, input, in_sizes, count, (unsigned char*)dOutput, true, out_cap, results, features);
}
