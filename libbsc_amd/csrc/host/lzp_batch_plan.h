// lzp_batch_plan.h — what drives the LZP stage (device/lzp.hip, and its CPU stand-in lzp_staged.cpp): the chunk table of
// a pass of blocks and the piece list that frames them, as pure functions of the sizes and of the chunks' results.  A single block of
// any size is a pass of one block (plan_block, batch_frame with count 1); batch_plan adds the limits of the public batch call.
// Plain arithmetic, no HIP; the CPU tests pin both (bscgpu_lzp_batch_plan, bscgpu_lzp_batch_frame, bscgpu_lzp_staged_host).
#pragma once
#include <cstdint>
#include "lzp_staged.h"

namespace bschost {
namespace lzp {

constexpr int BATCH_LZP_MAX_BLOCKS = 4096;                      // = BSCGPU_ST_BATCH_MAX_BLOCKS
constexpr int BATCH_LZP_MAX_N = 1 << 20;                        // = BSCGPU_BATCH_MAX_N: a block of a pass is one chunk or two
constexpr int BATCH_LZP_MAX_CHUNKS = 2 * BATCH_LZP_MAX_BLOCKS;  // 8192 entries
constexpr int BATCH_LZP_MAX_PIECES = 3 * BATCH_LZP_MAX_BLOCKS;  // a block: its table bytes and at most two payloads
constexpr int BATCH_LZP_TABLE_BYTES = 1 + 8 * 2;                // subtable_bytes(2): the longest table of a block of a pass

// One chunk of the pass: its block, its first byte in the pass, its length and the bytes its sweep may write (lzp.cpp: n - 2 for a
// block that is one chunk, the chunk's size otherwise).  16 bytes: the kernels read it as it stands.
struct BatchChunk { uint32_t block, start, size, cap; };

// lzp.cpp:531: the encoder refuses the block by its size, before it looks at a byte (an empty block included)
inline bool batch_refused_by_size(int n, int minLen) { return (int64_t)n - minLen < 32 || n - 2 < 16; }

// The chunks of block `block`, n bytes (any n up to 2^31 - 1) from `off` of the pass: lzp_staged.h's cut.  -> how many were written
// (1, 2, 4 or 8), 0: the encoder refuses the block by size and it owns no chunk.
inline int plan_block(int n, int minLen, uint32_t block, uint32_t off, BatchChunk* out)
{
    const int nc = num_chunks(n);
    if (nc == 1 && batch_refused_by_size(n, minLen)) return 0;
    for (int i = 0; i < nc; ++i) {
        out[i].block = block; out[i].start = off + (uint32_t)chunk_start(n, nc, i);
        out[i].size = (uint32_t)chunk_size(n, nc, i); out[i].cap = (uint32_t)(nc == 1 ? n - 2 : chunk_size(n, nc, i));
    }
    return nc;
}

// The chunk table of a pass of `count` blocks back to back, in pass order: plan_block per block.
// -> the number of chunks (<= BATCH_LZP_MAX_CHUNKS), or LIBBSC_BAD_PARAMETER with nothing written: count
// outside 0..BATCH_LZP_MAX_BLOCKS, a size negative or not below BATCH_LZP_MAX_N, a pass of 2^31 bytes or more, minLen outside 4..255.
inline int batch_plan(const int* sizes, int count, int minLen, BatchChunk* out)
{
    if (count < 0 || count > BATCH_LZP_MAX_BLOCKS || minLen < 4 || minLen > 255) return LIBBSC_BAD_PARAMETER;
    int64_t total = 0;
    for (int b = 0; b < count; ++b) {
        if (sizes[b] < 0 || sizes[b] >= BATCH_LZP_MAX_N) return LIBBSC_BAD_PARAMETER;
        total += sizes[b];
    }
    if (total >= 0x7fffffffll) return LIBBSC_BAD_PARAMETER;
    int k = 0;
    uint32_t off = 0;
    for (int b = 0; b < count; off += (uint32_t)sizes[b], ++b) k += plan_block(sizes[b], minLen, (uint32_t)b, off, out + k);
    return k;
}

// One piece of the frame: len bytes from src_off of its source to dst_off of the pass's output (the block's offset plus the place
// inside its stream).  Offsets of the staging area and of the raw input are positions in the pass; a table's are into the table bytes.
enum { PIECE_STAGING = 0, PIECE_RAW = 1, PIECE_TABLE = 2 };
struct BatchPiece { uint32_t src, src_off, dst_off, len; };

// The frames of a pass from its chunks' own results (own[k] of chunk k of batch_plan's table: the sweep's size or a negative code):
// frame_from_own per block, both framings.  results[b] = what lzp_compress returns for block b; where that is a size, the block's
// pieces are appended to `pieces` and its table to `table`, in block order: a pass planned by batch_plan has at most
// BATCH_LZP_MAX_PIECES pieces and count * BATCH_LZP_TABLE_BYTES table bytes, a single block of eight chunks 9 and 65.
// *raw_chunks (or null): chunks kept raw, whether their block came out or not.  -> the number of pieces.
// dst (or null: every block at its own offset of the pass): where block b's stream starts in the output, BATCH_NOWHERE: it gets no
// piece; as_it_is (or null): blocks whose sizes[b] raw bytes go to dst[b] in one piece instead — the caller's choice for a block
// without a stream.  Both are made from the results (batch_results) by a caller that packs the pass (block.cpp: a batched pass).
constexpr uint32_t BATCH_NOWHERE = 0xffffffffu;
inline int batch_frame(const int* sizes, int count, int minLen, int features, const int* own, int* results, BatchPiece* pieces,
                       unsigned char* table, int64_t* raw_chunks, const uint32_t* dst = nullptr, const unsigned char* as_it_is = nullptr)
{
    int np = 0, k = 0, tab = 0;
    uint32_t off = 0;
    if (raw_chunks) *raw_chunks = 0;
    for (int b = 0; b < count; off += (uint32_t)sizes[b], ++b) {
        const int n = sizes[b], nc = num_chunks(n);
        const uint32_t to = dst ? dst[b] : off;
        const bool refused = nc == 1 && batch_refused_by_size(n, minLen);
        Frame F;
        const int total = results[b] = refused ? LIBBSC_NOT_COMPRESSIBLE : frame_from_own(n, features, own + k, &F);
        if (!refused) { k += nc; if (raw_chunks) *raw_chunks += F.raw_chunks; }
        if (to == BATCH_NOWHERE) continue;
        if (as_it_is && as_it_is[b]) { if (n > 0) pieces[np++] = {PIECE_RAW, off, to, (uint32_t)n}; continue; }
        if (total < 0) continue;
        const int tab_bytes = frame_table(F, table + tab);
        pieces[np++] = {PIECE_TABLE, (uint32_t)tab, to, (uint32_t)tab_bytes};
        tab += tab_bytes;
        for (int i = 0; i < nc; ++i) {
            if (F.res[i] <= 0) continue;
            const uint32_t kind = nc > 1 && F.res[i] == F.size[i] ? PIECE_RAW : PIECE_STAGING;
            pieces[np++] = {kind, off + (uint32_t)F.start[i], to + (uint32_t)F.off[i], (uint32_t)F.res[i]};
        }
    }
    return np;
}
// ... the results alone
inline void batch_results(const int* sizes, int count, int minLen, int features, const int* own, int* results)
{
    for (int b = 0, k = 0; b < count; ++b) {
        const int nc = num_chunks(sizes[b]);
        if (nc == 1 && batch_refused_by_size(sizes[b], minLen)) { results[b] = LIBBSC_NOT_COMPRESSIBLE; continue; }
        Frame F;
        results[b] = frame_from_own(sizes[b], features, own + k, &F);
        k += nc;
    }
}

}  // namespace lzp
}  // namespace bschost
