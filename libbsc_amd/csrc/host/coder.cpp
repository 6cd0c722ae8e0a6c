// coder.cpp — block-level coder: split a sorted block into 1/2/4/8 sub-blocks at run boundaries, code each
// independently (one host thread per sub-block), frame them.  Wire format and split rule are the
// reference's (coder.cpp:52-59 counts, :70-109 split, :111-155 serial framing, :159-240 parallel framing).
#include "qlfc.h"
#include "container.h"

#include <cstring>
#include <immintrin.h>
#include <cstdio>
#include <cstdlib>
#include <chrono>
#include <memory>
#include <thread>
#include "par.h"
#include <vector>

namespace bschost {

enum { FEATURE_MULTITHREADING = 2 };

// Sub-block boundaries: sample every 32nd position (1, 33, 65, ...), count the sampled positions that
// start a run, cut whenever the running count reaches total / nblocks, at that sampled position.
void coder_split_blocks(const uint8_t* in, int n, int nblocks, int* start, int* size)
{
    int changes = 0;
    for (int i = 1; i < n; i += 32) changes += (in[i] != in[i - 1]);

    if (changes > nblocks) {
        const int per_block = changes / nblocks;
        int id = 0, seen = 0;
        start[0] = 0;
        for (int i = 1; i < n && id < nblocks - 1; i += 32) {
            if (in[i] != in[i - 1] && ++seen == per_block) {
                seen = 0;
                size[id] = i - start[id];
                start[++id] = i;
            }
        }
        size[nblocks - 1] = n - start[nblocks - 1];
    } else {
        const int each = n / nblocks;
        for (int p = 0; p < nblocks; ++p) {
            start[p] = each * p;
            size[p]  = (p != nblocks - 1) ? each : n - each * (nblocks - 1);
        }
    }
}

static int compress_serial(const uint8_t* in, uint8_t* out, int n, int coder)
{
    const int nblocks = coder_num_blocks(n);
    if (nblocks == 1) {
        const int r = qlfc_encode_block(in, out + 1, n, n - 1, coder);
        if (r < 0) return r;
        out[0] = 1;
        return r + 1;
    }
    int start[8], size[8];
    coder_split_blocks(in, n, nblocks, start, size);
    return frame_serial(out, n, nblocks, size,
        [&](int b, uint8_t* dst, int room) { return qlfc_encode_block(in + start[b], dst, size[b], room, coder); },
        [&](int b, uint8_t* dst) { memcpy(dst, in + start[b], (size_t)size[b]); return 0; });       // stored raw (coder.cpp:136-140)
}

static int compress_parallel(const uint8_t* in, uint8_t* out, int n, int coder)
{
    const int nblocks = coder_num_blocks(n);
    int start[8], size[8], res[8];
    coder_split_blocks(in, n, nblocks, start, size);
    std::unique_ptr<uint8_t, void (*)(void*)> scratch_buf((uint8_t*)bigbuf_get((size_t)n + 64), bigbuf_put);      // (not zeroed, not a fresh mapping per call)
    if (!scratch_buf) return NOT_ENOUGH_MEMORY;
    uint8_t* const scratch = scratch_buf.get();
    run_tasks(nblocks, [&](int b) {
        int r = qlfc_encode_block(in + start[b], scratch + start[b], size[b], size[b], coder);
        res[b] = (r < 0) ? size[b] : r;                     // failed sub-block is stored raw (coder.cpp:194)
    });
    return frame_parallel(out, n, nblocks, size, res,
        [&](int b, uint8_t* dst) { memcpy(dst, (res[b] != size[b] ? scratch : in) + start[b], (size_t)res[b]); return 0; });
}

int coder_compress_views(const RunView* views, int nblocks, const int* start, const int* size, int n,
                         uint8_t* out, int coder, int features, RawFetch& fetch_raw, SubEncode* encode_sub)
{
    if (coder != CODER_STATIC && coder != CODER_ADAPTIVE && coder != CODER_FAST) return BAD_PARAMETER;
    auto encode = [&](int b, int in_size, uint8_t* dst, int room) {
        return encode_sub ? (*encode_sub)(b, dst, room) : qlfc_encode_runs(views[b], in_size, dst, room, coder);
    };
    if (nblocks == 1) {
        const int r = encode(0, n, out + 1, n - 1);
        if (r < 0) return r;
        out[0] = 1;
        return r + 1;
    }
    auto raw = [&](int b, uint8_t* dst) { return fetch_raw(start[b], size[b], dst); };
    if (features & FEATURE_MULTITHREADING) {               // coder.cpp:159-240
        std::vector<std::unique_ptr<uint8_t[]>> scratch((size_t)nblocks);
        int res[8];
        double tms[8];
        run_tasks(nblocks, [&](int b) {
            const auto t0 = std::chrono::steady_clock::now();
            scratch[(size_t)b].reset(new uint8_t[(size_t)size[b] + 64]);        // uninitialised on purpose
            int r = encode(b, size[b], scratch[(size_t)b].get(), size[b]);
            res[b] = (r < 0) ? size[b] : r;
            tms[b] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        });
        if (getenv("BSCGPU_DEBUG")) { fprintf(stderr, "[coder] sub-block ms:"); for (int b = 0; b < nblocks; ++b) fprintf(stderr, " %.1f", tms[b]); fprintf(stderr, "\n"); }
        return frame_parallel(out, n, nblocks, size, res, [&](int b, uint8_t* dst) {
            if (res[b] == size[b]) return raw(b, dst);
            memcpy(dst, scratch[(size_t)b].get(), (size_t)res[b]);
            return 0;
        });
    }
    return frame_serial(out, n, nblocks, size,             // coder.cpp:111-155
        [&](int b, uint8_t* dst, int room) { return encode(b, size[b], dst, room); }, raw);
}

int coder_compress(const uint8_t* in, uint8_t* out, int n, int coder, int features)
{
    if (coder != CODER_STATIC && coder != CODER_ADAPTIVE && coder != CODER_FAST) return BAD_PARAMETER;
    if (coder_num_blocks(n) != 1 && (features & FEATURE_MULTITHREADING)) return compress_parallel(in, out, n, coder);
    return compress_serial(in, out, n, coder);
}

int coder_decompress_bounded(const uint8_t* in, long long in_size, uint8_t* out, int coder, int features, int max_out)
{
    if (coder != CODER_STATIC && coder != CODER_ADAPTIVE && coder != CODER_FAST) return BAD_PARAMETER;
    SubTableReader table;
    const int nblocks = subtable_open(&table, in, in_size, max_out);
    if (nblocks < 0) return nblocks;
    if (nblocks == 1) return qlfc_decode_block_bounded(in + 1, in_size - 1, out, coder, max_out);

    int res[8], isz[8], osz[8];
    long long iptr[8], optr[8];
    for (int b = 0; b < nblocks; ++b) {
        SubBlock s;
        if (subtable_next(&table, &s) < 0) return DATA_CORRUPT;
        isz[b] = s.isz; osz[b] = s.osz; iptr[b] = s.iptr; optr[b] = s.optr;
    }
    auto one = [&](int b) {
        if (isz[b] != osz[b]) { res[b] = qlfc_decode_block_bounded(in + iptr[b], isz[b], out + optr[b], coder, osz[b]); if (res[b] >= 0 && res[b] != osz[b]) res[b] = DATA_CORRUPT; }
        else { res[b] = isz[b]; memcpy(out + optr[b], in + iptr[b], (size_t)isz[b]); }
    };
    if (features & FEATURE_MULTITHREADING) {
        run_tasks(nblocks, one);
    } else {
        for (int b = 0; b < nblocks; ++b) one(b);
    }
    int total = 0, err = OK;
    for (int b = 0; b < nblocks; ++b) { if (res[b] < 0) err = res[b]; total += res[b]; }
    return err == OK ? total : err;
}
int coder_decompress(const uint8_t* in, uint8_t* out, int coder, int features) { return coder_decompress_bounded(in, UNBOUNDED_INPUT, out, coder, features, 0x7fffffff); }

// Adler-32 (adler32.cpp:82-204): s1 = 1 + sum, s2 = sum of s1, mod 65521; deferred modulo every 5552 bytes.
// 32 bytes per step with AVX2: s2 += 32 * s1 + sum (32 - i) * d[i]  (pmaddubsw against the weights 32..1), s1 += sum d[i].
uint32_t adler32(const uint8_t* p, size_t n)
{
    uint32_t s1 = 1, s2 = 0;
    const __m256i weights = _mm256_setr_epi8(32, 31, 30, 29, 28, 27, 26, 25, 24, 23, 22, 21, 20, 19, 18, 17,
                                             16, 15, 14, 13, 12, 11, 10, 9, 8, 7, 6, 5, 4, 3, 2, 1);
    const __m256i ones16 = _mm256_set1_epi16(1);
    while (n > 0) {
        size_t k = n < 5536 ? n : 5536;                       // multiple of 32 below the 5552 overflow bound
        n -= k;
        if (k >= 32) {
            __m256i vs1 = _mm256_setzero_si256(), vs2 = _mm256_setzero_si256(), vacc = _mm256_setzero_si256();   // vacc: sum of s1 before each step
            const size_t steps = k / 32;
            for (size_t i = 0; i < steps; ++i, p += 32) {
                const __m256i d = _mm256_loadu_si256(reinterpret_cast<const __m256i*>(p));
                vacc = _mm256_add_epi32(vacc, vs1);
                vs1 = _mm256_add_epi32(vs1, _mm256_sad_epu8(d, _mm256_setzero_si256()));            // 4 partial byte sums (u64 lanes, low 32 bits used)
                vs2 = _mm256_add_epi32(vs2, _mm256_madd_epi16(_mm256_maddubs_epi16(d, weights), ones16));
            }
            k -= steps * 32;
            auto hsum = [](__m256i v) { __m128i x = _mm_add_epi32(_mm256_castsi256_si128(v), _mm256_extracti128_si256(v, 1));
                                        x = _mm_add_epi32(x, _mm_shuffle_epi32(x, 0x4e)); x = _mm_add_epi32(x, _mm_shuffle_epi32(x, 0xb1)); return (uint32_t)_mm_cvtsi128_si32(x); };
            const uint32_t sum_d = hsum(vs1), sum_w = hsum(vs2), sum_prev = hsum(vacc);
            s2 += (uint32_t)(steps * 32) * s1 + 32u * sum_prev + sum_w;      // every step adds 32 * (s1 before it) + its weighted bytes
            s1 += sum_d;
        }
        while (k--) { s1 += *p++; s2 += s1; }
        s1 %= 65521u; s2 %= 65521u;
    }
    return s1 | (s2 << 16);
}

}  // namespace bschost
