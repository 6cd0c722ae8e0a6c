// lzp_staged.cpp — the LZP encoder in the staged form of DESIGN §3.9, on the host: the CPU stand-in of device/lzp.hip.  It computes what
// lzp_compress computes, by the device's route: (A) every position's predecessor and successor in its hash slot as if every position
// were visited, (B) a byte of flags per position from those links, (C) a sweep over windows of SWEEP_WINDOW positions that takes its
// decisions from the flags, keeps the real table only for the positions whose predecessor a match skipped ("dirty"), and falls back to
// the scanner's group-by-group loop where the group phase matters.  Needs no GPU; the tests hold it to lzp_compress byte for byte and
// the device stage to it counter for counter.
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../../include/bscgpu.h"
#include "lzp.h"
#include "lzp_staged.h"
#include "lzp_batch_plan.h"

namespace bschost {

namespace {

using namespace lzp;

inline uint32_t ld32(const uint8_t* p) { uint32_t v; memcpy(&v, p, 4); return v; }
inline uint64_t ld64(const uint8_t* p) { uint64_t v; memcpy(&v, p, 8); return v; }

struct Chunk {
    const uint8_t* T; int n; uint8_t* out; int cap;
    int hashSize, minLen, W; bool verify;
    uint32_t mask; int limit, eob;
    std::vector<uint32_t> prev0, next0, table;
    std::vector<uint8_t> flags, dirty;
    // the sweep's state
    int p, o, retry_after;
    int64_t cnt[CR_WORDS];

    bool same(int q, int ref) const
    {
        const int far = minLen - W;
        if (W == 4) return ld32(T + q + far) == ld32(T + ref + far) && ld32(T + q) == ld32(T + ref);
        return ld64(T + q + far) == ld64(T + ref + far) && ld64(T + q) == ld64(T + ref);
    }

    // ---- A: links ------------------------------------------------------------------------------------------------------------------
    void links()
    {
        prev0.assign((size_t)n, 0); next0.assign((size_t)n, 0);
        std::vector<uint32_t> last((size_t)mask + 1, 0);             // (the device sorts (slot, position) and links neighbours)
        for (int q = 4; q < n; ++q) {
            const uint32_t s = slot_of(ctx_of(T, (uint32_t)q), mask);
            prev0[(size_t)q] = last[s];
            if (last[s]) next0[last[s]] = (uint32_t)q;
            last[s] = (uint32_t)q;
        }
    }
    // ---- B: flags ------------------------------------------------------------------------------------------------------------------
    void candidates()
    {
        flags.assign((size_t)n, 0); dirty.assign((size_t)n, 0);
        for (int q = 4; q < n; ++q) {
            const uint32_t pv = prev0[(size_t)q];
            uint8_t f = (pv > 0 ? F_OCC : 0) | (T[q] == FLAG ? F_FLAG : 0);
            if (pv > 0 && q < limit + 3 && same(q, (int)pv)) f |= F_CAND;
            flags[(size_t)q] = f;
        }
    }

    // ---- C: the sweep ----------------------------------------------------------------------------------------------------------------
    // What the scanner would find at q: the slot's content (0: empty) and whether it is a candidate.  Before the table is written for q.
    struct Look { uint32_t seen; bool cand, flag; };
    std::vector<Look> win;                                       // a window's look-ups (kept between windows)
    Look look(int q, bool probe)
    {
        const uint8_t f = flags[(size_t)q];
        Look L;
        L.flag = (f & F_FLAG) != 0;
        if (dirty[(size_t)q]) {
            L.seen = table[slot_of(ctx_of(T, (uint32_t)q), mask)];
            L.cand = probe && L.seen > 0 && same(q, (int)L.seen);
        } else {
            L.seen = (f & F_OCC) ? prev0[(size_t)q] : 0;
            L.cand = probe && (f & F_CAND) != 0;
        }
        return L;
    }
    void visit(int q) { uint32_t& t = table[slot_of(ctx_of(T, (uint32_t)q), mask)]; if ((uint32_t)q > t) t = (uint32_t)q; }

    // a candidate at m whose slot held `seen`: measured, then taken or (VERIFY) turned into a literal.  false: the budget is spent
    bool candidate(int m, uint32_t seen)
    {
        int len = verify ? 8 : minLen;
        while (m + len < limit) {
            const uint64_t x = ld64(T + m + len) ^ ld64(T + seen + len);
            if (x) { len += __builtin_ctzll(x) >> 3; break; }
            len += 8;
        }
        if (verify && len < minLen) {
            ++cnt[CR_ZONES];
            retry_after = m + len;
            const uint8_t b = T[m];
            out[o++] = b;
            if (b == FLAG) { out[o++] = 255; ++cnt[CR_ESCAPES]; }
            p = m + 1;
            return true;
        }
        const int excess = len - minLen, k = excess / 254;
        out[o++] = FLAG;
        if (k >= 1 && o + k >= eob) return false;
        memset(out + o, 254, (size_t)k); o += k;
        out[o++] = (uint8_t)(excess - 254 * k);
        ++cnt[CR_MATCHES];
        for (int x = m + 1; x < m + len; ++x) if (next0[(size_t)x]) dirty[next0[(size_t)x]] = 1;
        p = m + len;
        return true;
    }

    // one group of the scanner's main loop at p (lzp.cpp:63), with the staged look-ups.  false: the budget is spent
    bool group()
    {
        const bool probing = !verify || p > retry_after;
        int j = 0, kind = 0; uint32_t seen = 0;
        for (; j < 4; ++j) {
            const Look L = look(p + j, probing);
            cnt[CR_DIRTY] += dirty[(size_t)(p + j)];
            visit(p + j);
            seen = L.seen;
            if (L.seen > 0) {
                if (L.cand) { kind = 1; break; }
                if (L.flag) { kind = 2; break; }
            }
        }
        const int lit = kind == 0 ? 4 : j;
        memcpy(out + o, T + p, (size_t)lit); o += lit; p += lit;
        if (kind == 2) { out[o++] = FLAG; out[o++] = 255; ++p; ++cnt[CR_ESCAPES]; }
        if (kind == 1) return candidate(p, seen);
        return true;
    }

    // a window of nw positions at p, all of them in front of `limit` (main) or all of them behind the main phase (tail: no probing).
    // false: the budget is spent
    bool window(int nw, bool tail)
    {
        std::vector<Look>& L = win;
        L.resize((size_t)nw);
        for (int i = 0; i < nw; ++i) L[(size_t)i] = look(p + i, !tail);      // (dirty positions read the table as the window found it)
        int m = nw, last_esc = -1;
        for (int i = 0; i < nw; ++i) if (L[(size_t)i].seen > 0 && L[(size_t)i].cand) { m = i; break; }
        for (int i = 0; i < m; ++i) if (L[(size_t)i].seen > 0 && L[(size_t)i].flag) last_esc = i;
        // without a match the window ends where a group starts: groups restart behind an escaped literal
        int end = m;
        if (m == nw && !tail) end = last_esc + 1 + ((nw - (last_esc + 1)) & ~3);
        int nesc = 0;
        for (int i = 0; i < end; ++i) nesc += (L[(size_t)i].seen > 0 && L[(size_t)i].flag);
        if (o + end + nesc >= eob) return false;
        // (look-ups behind `end`, or behind the match, were not the scanner's: those positions come again, or never)
        for (int i = 0; i < end + (m < nw ? 1 : 0); ++i) cnt[CR_DIRTY] += dirty[(size_t)(p + i)];
        for (int i = 0; i < end; ++i) {
            out[o++] = T[p + i];
            if (L[(size_t)i].seen > 0 && L[(size_t)i].flag) { out[o++] = 255; ++cnt[CR_ESCAPES]; }
            visit(p + i);
        }
        p += end;
        if (m < nw) { visit(p); return candidate(p, L[(size_t)m].seen); }
        return true;
    }

    int run()
    {
        memset(cnt, 0, sizeof cnt);
        if ((int64_t)n - minLen < 32 || cap < 16) return LIBBSC_NOT_COMPRESSIBLE;
        mask = ((uint32_t)1 << hashSize) - 1;
        W = narrow_word(minLen); verify = narrow_verify(minLen);
        limit = n - narrow_guard(minLen); eob = cap - 8;
        links();
        candidates();
        table.assign((size_t)mask + 1, 0);
        memcpy(out, T, 4);
        p = 4; o = 4; retry_after = 0;
        while (p < limit) {
            if (o >= eob) return LIBBSC_NOT_COMPRESSIBLE;
            const bool serial = (verify && p <= retry_after) || limit - p < SWEEP_SERIAL_TAIL;
            const int nw = limit - p < SWEEP_WINDOW ? limit - p : SWEEP_WINDOW;
            if (!(serial ? group() : window(nw, false))) return LIBBSC_NOT_COMPRESSIBLE;
        }
        while (p < n) {
            if (o >= eob) return LIBBSC_NOT_COMPRESSIBLE;
            if (!window(n - p < SWEEP_WINDOW ? n - p : SWEEP_WINDOW, true)) return LIBBSC_NOT_COMPRESSIBLE;
        }
        return o >= eob ? LIBBSC_NOT_COMPRESSIBLE : o;
    }
};

}  // namespace

int lzp_compress_staged(const uint8_t* in, uint8_t* out, int n, int hashSize, int minLen, int features, int64_t* counters)
{
    if (hashSize > STAGED_MAX_HASH) return LIBBSC_NOT_SUPPORTED;
    // the device's route (lzp.hip: lzp_stage) for a pass of this one block: chunk table, a sweep per entry, piece list, the pieces moved
    int64_t cnt[CNT_WORDS] = {0, 0, 0, 0, 0};
    BatchChunk chunks[8];
    const int nc = plan_block(n, minLen, 0, 0, chunks);
    std::vector<uint8_t> staging((size_t)n + 16);
    int own[8];
    for (int k = 0; k < nc; ++k) {
        Chunk C;
        C.T = in + chunks[k].start; C.n = (int)chunks[k].size;
        C.out = staging.data() + chunks[k].start; C.cap = (int)chunks[k].cap;
        C.hashSize = hashSize; C.minLen = minLen;
        own[k] = C.run();
        count_chunk(cnt, C.cnt);
    }
    int result = 0;
    BatchPiece pieces[1 + 8];
    unsigned char table[1 + 8 * 8];
    const int np = batch_frame(&n, 1, minLen, features, own, &result, pieces, table, &cnt[CNT_RAW_CHUNKS]);
    const uint8_t* const from[3] = {staging.data(), in, table};            // PIECE_STAGING, PIECE_RAW, PIECE_TABLE
    for (int p = 0; p < np; ++p) memcpy(out + pieces[p].dst_off, from[pieces[p].src] + pieces[p].src_off, pieces[p].len);
    if (counters) memcpy(counters, cnt, sizeof cnt);
    return result;
}

}  // namespace bschost

extern "C" int bscgpu_lzp_staged_host(const uint8_t* in, uint8_t* out, int n, int hashSize, int minLen, int features, int64_t* counters)
{
    if (!in || !out || n < 0 || minLen < 4 || minLen > 255 || hashSize < 10 || hashSize > 28) return LIBBSC_BAD_PARAMETER;
    return bschost::lzp_compress_staged(in, out, n, hashSize, minLen, features, counters);
}

// ---- a pass of small blocks (lzp_batch_plan.h) -------------------------------------------------------------------------------------------
extern "C" int bscgpu_lzp_batch_plan(const int* sizes, int count, int minLen, int* chunk_block, int* chunk_start, int* chunk_size, int* chunk_cap)
{
    using namespace bschost::lzp;
    if ((count > 0 && !sizes) || !chunk_block || !chunk_start || !chunk_size || !chunk_cap) return LIBBSC_BAD_PARAMETER;
    std::vector<BatchChunk> t((size_t)BATCH_LZP_MAX_CHUNKS);
    const int k = batch_plan(sizes, count, minLen, t.data());
    for (int i = 0; i < k; ++i) {
        chunk_block[i] = (int)t[(size_t)i].block; chunk_start[i] = (int)t[(size_t)i].start;
        chunk_size[i] = (int)t[(size_t)i].size; chunk_cap[i] = (int)t[(size_t)i].cap;
    }
    return k;
}

extern "C" int bscgpu_lzp_batch_frame(const int* sizes, int count, int minLen, int features, const int* own, int* results, int* piece_src,
                                      int* piece_src_off, int* piece_dst_off, int* piece_len, unsigned char* table, int64_t* raw_chunks)
{
    using namespace bschost::lzp;
    if ((count > 0 && (!sizes || !results)) || !piece_src || !piece_src_off || !piece_dst_off || !piece_len || !table) return LIBBSC_BAD_PARAMETER;
    std::vector<BatchChunk> t((size_t)BATCH_LZP_MAX_CHUNKS);
    const int k = batch_plan(sizes, count, minLen, t.data());
    if (k < 0 || (k > 0 && !own)) return LIBBSC_BAD_PARAMETER;
    std::vector<BatchPiece> p((size_t)BATCH_LZP_MAX_PIECES);
    const int np = batch_frame(sizes, count, minLen, features, own, results, p.data(), table, raw_chunks);
    for (int i = 0; i < np; ++i) {
        piece_src[i] = (int)p[(size_t)i].src; piece_src_off[i] = (int)p[(size_t)i].src_off;
        piece_dst_off[i] = (int)p[(size_t)i].dst_off; piece_len[i] = (int)p[(size_t)i].len;
    }
    return np;
}

extern "C" int bscgpu_lzp_chunk_staged_host(const uint8_t* in, uint8_t* out, int n, int cap, int hashSize, int minLen, int64_t* counters)
{
    using namespace bschost::lzp;
    if (!in || !out || n < 0 || cap < 0 || cap > n || minLen < 4 || minLen > 255 || hashSize < 10 || hashSize > STAGED_MAX_HASH) return LIBBSC_BAD_PARAMETER;
    std::vector<uint8_t> staging((size_t)n + 16);                // (as lzp_compress_staged's: the sweep's own slack)
    bschost::Chunk C;
    C.T = in; C.n = n; C.out = staging.data(); C.cap = cap; C.hashSize = hashSize; C.minLen = minLen;
    const int r = C.run();
    if (counters) { memset(counters, 0, sizeof(int64_t) * CNT_WORDS); count_chunk(counters, C.cnt); }
    if (r > 0) memcpy(out, staging.data(), (size_t)r);
    return r;
}
