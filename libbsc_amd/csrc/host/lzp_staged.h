// lzp_staged.h — what the host encoder (lzp.cpp), its staged stand-in (lzp_staged.cpp) and the device stage (device/lzp.hip) share:
// the context hash, the variant table, the chunk cut, the flag bits of stage B, the sweep's window size, the result record of a
// chunk and the framing of a block from its chunks' results.  Plain arithmetic, no HIP; the hash helpers also compile for the device.
#pragma once
#include <cstdint>
#include <cstring>
#include "container.h"

#ifdef __HIPCC__
#define LZP_HD __host__ __device__ inline
#else
#define LZP_HD inline
#endif

namespace bschost {
namespace lzp {

constexpr uint8_t FLAG = 0xF2;

LZP_HD uint32_t slot_of(uint32_t c, uint32_t mask) { return ((c >> 15) ^ c ^ (c >> 3)) & mask; }     // lzp.cpp:69
// previous four bytes of position q, newest lowest
LZP_HD uint32_t ctx_of(const uint8_t* T, uint32_t q)
{
    return ((uint32_t)T[q - 4] << 24) | ((uint32_t)T[q - 3] << 16) | ((uint32_t)T[q - 2] << 8) | (uint32_t)T[q - 1];
}

// Where the main phase of the narrow scanner stops, in bytes before the end of the chunk (lzp.cpp:56, :166, :276, :330).
LZP_HD int narrow_guard(int minLen)
{
    if (minLen == 4) return 4 + 32;
    if (minLen <= 8) return 8 + 32;
    if (minLen <= 16) return 16 + 32;
    return minLen + 32;
}
// The narrow variants (lzp.cpp:537-557): probe word W and whether the two words have to be verified
LZP_HD int  narrow_word(int minLen)   { return minLen >= 8 ? 8 : 4; }
LZP_HD bool narrow_verify(int minLen) { return minLen > 16; }

LZP_HD int num_chunks(int n)                                  // lzp.cpp:44-51
{
    if (n < 256 * 1024) return 1;
    if (n < 4 * 1024 * 1024) return 2;
    if (n < 16 * 1024 * 1024) return 4;
    return 8;
}
LZP_HD int chunk_start(int n, int nc, int b) { return b * (n / nc); }
LZP_HD int chunk_size(int n, int nc, int b)  { return b != nc - 1 ? n / nc : n - b * (n / nc); }

// ---- the staged form ----------------------------------------------------------------------------------------------------
// Stage B's byte per position
constexpr uint8_t F_OCC = 1, F_CAND = 2, F_FLAG = 4;
// Stage C: positions of a window, and the stretch in front of `limit` that runs group by group
constexpr int SWEEP_WINDOW = 1024, SWEEP_SERIAL_TAIL = 64;
// hashSize the staged form takes: the table of a chunk has to fit the LDS of one workgroup (2^15 words = 128 KiB of 160)
constexpr int STAGED_MAX_HASH = 15;

// What a chunk's sweep leaves: its size under a budget of its own size (or NOT_COMPRESSIBLE) and the paths it took
enum { CR_RES = 0, CR_MATCHES, CR_DIRTY, CR_ZONES, CR_ESCAPES, CR_WORDS = 8 };
// counters[] of bscgpu_lzp_staged_host / bscgpu_lzp_counters
enum { CNT_MATCHES = 0, CNT_DIRTY, CNT_ZONES, CNT_ESCAPES, CNT_RAW_CHUNKS, CNT_WORDS };
// a chunk's record added to the counters (raw chunks are the frame's to count)
template <class Word>
inline void count_chunk(int64_t* counters, const Word* rec)
{
    counters[CNT_MATCHES] += rec[CR_MATCHES]; counters[CNT_DIRTY] += rec[CR_DIRTY];
    counters[CNT_ZONES] += rec[CR_ZONES]; counters[CNT_ESCAPES] += rec[CR_ESCAPES];
}

// A block's frame from its chunks' own results.  own[b]: chunk b coded with a budget of size[b] bytes (n - 2 for a single chunk) -> its
// size or a negative code.  The scanner's decisions do not depend on its budget; the budget only ends it, with NOT_COMPRESSIBLE, once
// the output reaches budget - 8.  So what the serial rule's smaller budget min(size[b], n - bytes so far) would have given is known
// from own[b]: the same bytes if own[b] < budget - 8, NOT_COMPRESSIBLE otherwise — which frame_serial turns into a raw chunk.
// -> the payload's size (res[b] = bytes chunk b takes, size[b]: raw) or NOT_COMPRESSIBLE; raw_chunks counts the raw ones either way.
struct Frame { int nc, start[8], size[8], res[8], off[8], total, raw_chunks; };
static inline int frame_from_own(int n, int features, const int* own, Frame* F)
{
    const int nc = F->nc = num_chunks(n);
    F->raw_chunks = 0;
    for (int b = 0; b < nc; ++b) { F->start[b] = chunk_start(n, nc, b); F->size[b] = chunk_size(n, nc, b); }
    if (nc == 1) {
        if (own[0] < 0) return F->total = own[0];
        F->res[0] = own[0]; F->off[0] = 1;
        return F->total = own[0] + 1;
    }
    int optr = subtable_bytes(nc);
    if (features & 2 /* LIBBSC_FEATURE_MULTITHREADING */) {
        long long total = optr;
        for (int b = 0; b < nc; ++b) { F->res[b] = own[b] < 0 ? F->size[b] : own[b]; F->raw_chunks += own[b] < 0; total += F->res[b]; }
        if (total >= n) return F->total = LIBBSC_NOT_COMPRESSIBLE;
        for (int b = 0; b < nc; ++b) { F->off[b] = optr; optr += F->res[b]; }
        return F->total = optr;
    }
    for (int b = 0; b < nc; ++b) {
        const int room = F->size[b] < n - optr ? F->size[b] : n - optr;
        int r = (own[b] >= 0 && room >= 16 && own[b] < room - 8) ? own[b] : LIBBSC_NOT_COMPRESSIBLE;
        if (r < 0) {
            ++F->raw_chunks;
            if (optr + F->size[b] >= n) return F->total = LIBBSC_NOT_COMPRESSIBLE;
            r = F->size[b];
        }
        F->res[b] = r; F->off[b] = optr; optr += r;
    }
    return F->total = optr;
}
// the table in front of the payloads: 1 byte for a single chunk, subtable_bytes(nc) otherwise -> its length
static inline int frame_table(const Frame& F, unsigned char* out)
{
    out[0] = (unsigned char)F.nc;
    if (F.nc == 1) return 1;
    for (int b = 0; b < F.nc; ++b) subtable_entry(out, b, F.size[b], F.res[b]);
    return subtable_bytes(F.nc);
}

}  // namespace lzp

// The staged encoder on the host (lzp_staged.cpp): stages A, B and C of DESIGN §3.9 as the device runs them.  hashSize <= STAGED_MAX_HASH.
// -> what lzp_compress returns, the same bytes in out (n bytes); counters[lzp::CNT_WORDS] (or null): the paths taken, summed over chunks.
int lzp_compress_staged(const uint8_t* in, uint8_t* out, int n, int hashSize, int minLen, int features, int64_t* counters);

}  // namespace bschost
