// container.h — the block format, and the only place that knows an offset of it (libbsc.cpp:68-81, :213-338, :340-418, :522-617 the
// block; coder.cpp:111-240, lzp.cpp:687-885 the sub-block table), as plain host code without any HIP in it:
//
//   block   = header (LIBBSC_HEADER_SIZE bytes) ++ body
//   header  = le32 blockSize, dataSize, mode, index, adler(data), adler(body), adler(header[0 .. 24))
//   body    = the data itself (mode 0: a stored block), or  payload ++ le32 indexes[num] ++ u8 num  (a coded block)
//   payload = u8 1 ++ one coded sub-block, or  u8 nb ++ nb x {le32 raw size, le32 coded size} ++ the sub-blocks back to back, where
//             coded size == raw size says "kept raw"; the QLFC coder's payload and the LZP stage's output have this same shape
//
// block.cpp, coder.cpp, lzp.cpp, decode.cpp and batch_decode.cpp write and read the format through these functions alone;
// tools/container_probe.cpp holds them to the restatement in tests/pipeline_model.py (tests/test_container_host.py).
#pragma once
#include <stdint.h>
#include <string.h>

#include "../../../include/libbsc.h"

// ---- 1. fields ----------------------------------------------------------------------------------------------------------------------------
// (little-endian hosts only, like the rest of the library: the 32-bit fields are the machine's own)
static inline void le32_store(unsigned char* p, int v) { memcpy(p, &v, 4); }
static inline int  le32_load(const unsigned char* p) { int v; memcpy(&v, p, 4); return v; }

// the mode word: sorter in bits 0-4, coder in 5-7, LZP min length in 8-15, LZP hash size in 16-23; 0 is a stored block
struct BlockMode { int sorter, coder, lzp_hash, lzp_min; };
static inline int block_mode_pack(const BlockMode& m) { return m.sorter + (m.coder << 5) + (m.lzp_min << 8) + (m.lzp_hash << 16); }
static inline BlockMode block_mode_unpack(int mode)
{
    const BlockMode m = { mode & 0x1f, (mode >> 5) & 0x7, (mode >> 16) & 0xff, (mode >> 8) & 0xff };
    return m;
}
static inline bool block_mode_has_lzp(int mode) { return mode != (mode & 0xff); }
static inline int  block_mode_without_lzp(int mode) { return mode & 0xff; }
static inline int  block_mode_with_sorter(int mode, int sorter) { return (mode & ~0x1f) | sorter; }

// ---- 2. block header and trailer ----------------------------------------------------------------------------------------------------------
struct BlockFields { int block_size, data_size, mode, index; unsigned adler_data, adler_body; };

static inline void block_header_write(unsigned char* out, const BlockFields& h)
{
    le32_store(out + 0, h.block_size);
    le32_store(out + 4, h.data_size);
    le32_store(out + 8, h.mode);
    le32_store(out + 12, h.index);
    le32_store(out + 16, (int)h.adler_data);
    le32_store(out + 20, (int)h.adler_body);
    le32_store(out + 24, (int)bsc_adler32(out, 24, 0));
}
// the LIBBSC_HEADER_SIZE bytes at in -> false: the header's own checksum does not hold (h is filled in either way)
static inline bool block_header_read(const unsigned char* in, BlockFields* h)
{
    h->block_size = le32_load(in + 0); h->data_size = le32_load(in + 4); h->mode = le32_load(in + 8); h->index = le32_load(in + 12);
    h->adler_data = (unsigned)le32_load(in + 16); h->adler_body = (unsigned)le32_load(in + 20);
    return (unsigned)le32_load(in + 24) == bsc_adler32(in, 24, 0);
}
static inline unsigned char* block_body(unsigned char* block) { return block + LIBBSC_HEADER_SIZE; }
static inline const unsigned char* block_body(const unsigned char* block) { return block + LIBBSC_HEADER_SIZE; }
static inline bool block_body_ok(const unsigned char* block, const BlockFields& h)
{
    return h.adler_body == bsc_adler32(block_body(block), h.block_size - LIBBSC_HEADER_SIZE, 0);
}

// a stored block around the n bytes that already lie at block_body(out); adler: their Adler-32 -> the block's size
static inline int block_finish_stored(unsigned char* out, int n, unsigned adler)
{
    const BlockFields h = { n + LIBBSC_HEADER_SIZE, n, 0, 0, adler, adler };
    block_header_write(out, h);
    return h.block_size;
}

// a coded block around the `coded` payload bytes (or the coder's negative code) at block_body(out): the trailer behind them, then the
// header.  n_orig: the size of the block's data, adler_data: its Adler-32.  -> the block's size, or LIBBSC_NOT_COMPRESSIBLE: the block
// does not pay (libbsc.cpp:315-318) and the caller stores it, from wherever its data lies
static inline int block_finish_coded(unsigned char* out, int n_orig, int coded, int mode, int index, const int* indexes, int num_indexes,
                                     unsigned adler_data)
{
    if (coded < LIBBSC_NO_ERROR || coded + 1 + 4 * num_indexes >= n_orig) return LIBBSC_NOT_COMPRESSIBLE;
    unsigned char* trailer = block_body(out) + coded;
    if (num_indexes > 0) memcpy(trailer, indexes, (size_t)4 * num_indexes);
    trailer[4 * num_indexes] = (unsigned char)num_indexes;
    const int body = coded + 1 + 4 * num_indexes;
    const BlockFields h = { body + LIBBSC_HEADER_SIZE, n_orig, mode, index, adler_data, bsc_adler32(block_body(out), body, 0) };
    block_header_write(out, h);
    return h.block_size;
}

// a coded block holds at least one payload byte and the index count
static inline bool block_holds_payload(const BlockFields& h) { return h.block_size >= LIBBSC_HEADER_SIZE + 2; }
// for decoders: the payload of the coded block whose header is h (block_size bytes at block, bsc_block_info has passed it): the bytes
// the coder may read and the aux indexes behind them.  -> LIBBSC_NO_ERROR, or LIBBSC_DATA_CORRUPT: the body's checksum does not hold,
// or the block has no room for one payload byte and the index count
struct CodedPayload { const unsigned char* data; long long size; const unsigned char* indexes; int num_indexes; };
static inline int block_coded_payload(const unsigned char* block, const BlockFields& h, CodedPayload* p)
{
    if (!block_holds_payload(h) || !block_body_ok(block, h)) return LIBBSC_DATA_CORRUPT;
    p->num_indexes = block[h.block_size - 1];
    p->size = (long long)h.block_size - LIBBSC_HEADER_SIZE - 1 - 4LL * p->num_indexes;
    if (p->size < 1) return LIBBSC_DATA_CORRUPT;
    p->data = block_body(block);
    p->indexes = p->data + p->size;
    return LIBBSC_NO_ERROR;
}

// the BWT's aux indexes: one every aux_rate(n) positions, the largest power of two <= n / 8 (>= 1), bwt.cpp:192-197
static inline int aux_rate(int n)
{
    int mod = n / 8;
    mod |= mod >> 1; mod |= mod >> 2; mod |= mod >> 4; mod |= mod >> 8; mod |= mod >> 16; mod >>= 1;
    return mod + 1;
}

// ---- 3. sub-block table, writing ----------------------------------------------------------------------------------------------------------
// nb (2 .. 8) sub-blocks of size[b] bytes make a payload of at most n bytes; res[b] is what sub-block b takes in it, size[b] where it is
// kept raw.  The single-sub-block form (out[0] = 1, no table) stays with the callers: their budgets differ.
constexpr int SUBTABLE_MAX = 8;
static inline int subtable_bytes(int nb) { return 1 + 8 * nb; }
static inline void subtable_entry(unsigned char* out, int b, int raw, int coded)
{
    le32_store(out + 1 + 8 * b, raw);
    le32_store(out + 1 + 8 * b + 4, coded);
}

// table and sub-blocks; put(b, dst) puts sub-block b's res[b] bytes, coded or raw, at dst -> 0, or a negative code, which ends it.
// -> the payload's size
template <class Put>
static inline int subtable_write(unsigned char* out, int nb, const int* size, const int* res, Put put)
{
    out[0] = (unsigned char)nb;
    int optr = subtable_bytes(nb);
    for (int b = 0; b < nb; ++b) {
        subtable_entry(out, b, size[b], res[b]);
        const int rc = put(b, out + optr);
        if (rc < 0) return rc;
        optr += res[b];
    }
    return optr;
}

// the parallel rule (coder.cpp:159-240, lzp.cpp:736-790): every sub-block was coded on its own with a budget of its own size; a payload
// that does not come out below n is LIBBSC_NOT_COMPRESSIBLE
template <class Put>
static inline int frame_parallel(unsigned char* out, int n, int nb, const int* size, const int* res, Put put)
{
    long long total = subtable_bytes(nb);
    for (int b = 0; b < nb; ++b) total += res[b];
    if (total >= n) return LIBBSC_NOT_COMPRESSIBLE;
    return subtable_write(out, nb, size, res, put);
}

// the serial rule (coder.cpp:111-155, lzp.cpp:697-731): one sub-block after the other, straight into the payload.  encode(b, dst, room)
// codes sub-block b into at most room bytes -> its size or a negative code: then it is kept raw, raw(b, dst) puts its size[b] bytes
// (-> 0 or a negative code, which ends it) — unless they would reach the n-th byte: LIBBSC_NOT_COMPRESSIBLE.  -> the payload's size
template <class Encode, class Raw>
static inline int frame_serial(unsigned char* out, int n, int nb, const int* size, Encode encode, Raw raw)
{
    out[0] = (unsigned char)nb;
    int optr = subtable_bytes(nb);
    for (int b = 0; b < nb; ++b) {
        const int room = size[b] < n - optr ? size[b] : n - optr;
        int r = encode(b, out + optr, room);
        if (r < 0) {
            if (optr + size[b] >= n) return LIBBSC_NOT_COMPRESSIBLE;
            r = size[b];
            const int rc = raw(b, out + optr);
            if (rc < 0) return rc;
        }
        subtable_entry(out, b, size[b], r);
        optr += r;
    }
    return optr;
}

// Sub-blocks coded on their own (res[] as for the parallel rule) under the serial rule: the serial coder gives sub-block b the budget
// min(size[b], n - bytes so far).  Where that is size[b] for every b its payload is exactly subtable_write's (SERIAL_EXACT), unless a
// raw sub-block reaches the n-th byte (SERIAL_INCOMPRESSIBLE: its answer is LIBBSC_NOT_COMPRESSIBLE); where a budget is smaller, what
// it would have produced is not known (SERIAL_NOT_EXACT) and the block has to be coded serially.
enum SerialVerdict { SERIAL_EXACT, SERIAL_NOT_EXACT, SERIAL_INCOMPRESSIBLE };
static inline SerialVerdict serial_verdict(int n, int nb, const int* size, const int* res)
{
    int optr = subtable_bytes(nb);
    for (int b = 0; b < nb; ++b) {
        if (n - optr < size[b]) return SERIAL_NOT_EXACT;
        if (res[b] == size[b] && optr + size[b] >= n) return SERIAL_INCOMPRESSIBLE;        // coder.cpp:131-134
        optr += res[b];
    }
    return SERIAL_EXACT;
}

// ---- 4. sub-block table, reading ----------------------------------------------------------------------------------------------------------
// A payload of in_size bytes that may decode to at most max_out bytes.  subtable_open -> the number of sub-blocks: 1 is the single form
// (the coded sub-block is in + 1, the caller's decoder bounds it), 2 .. 8 have a table, which lies inside the payload; or
// LIBBSC_DATA_CORRUPT.  subtable_next, once per sub-block in order -> LIBBSC_NO_ERROR and where it lies: isz bytes at in + iptr decode
// to osz bytes at optr (isz == osz: kept raw); or LIBBSC_DATA_CORRUPT: a negative size, a sub-block that leaves the payload (tables
// whose checksum holds can say so), an output past max_out.
struct SubBlock { int isz, osz; long long iptr, optr; };
struct SubTableReader { const unsigned char* in; long long in_size, max_out, ip, op; int b; };
static inline int subtable_open(SubTableReader* t, const unsigned char* in, long long in_size, long long max_out)
{
    if (in_size < 1) return LIBBSC_DATA_CORRUPT;
    const int nb = in[0];
    if (nb == 1) return 1;
    if (nb < 1 || nb > SUBTABLE_MAX || in_size < subtable_bytes(nb)) return LIBBSC_DATA_CORRUPT;
    t->in = in; t->in_size = in_size; t->max_out = max_out; t->ip = subtable_bytes(nb); t->op = 0; t->b = 0;
    return nb;
}
static inline int subtable_next(SubTableReader* t, SubBlock* s)
{
    s->osz = le32_load(t->in + 1 + 8 * t->b);
    s->isz = le32_load(t->in + 1 + 8 * t->b + 4);
    if (s->osz < 0 || s->isz < 0 || t->ip + s->isz > t->in_size || t->op + s->osz > t->max_out) return LIBBSC_DATA_CORRUPT;
    s->iptr = t->ip; s->optr = t->op;
    t->ip += s->isz; t->op += s->osz; ++t->b;
    return LIBBSC_NO_ERROR;
}
