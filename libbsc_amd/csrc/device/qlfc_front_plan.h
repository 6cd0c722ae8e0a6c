// qlfc_front_plan.h — the arithmetic of the QLFC front end (qlfc_front.hip) as plain host code without any HIP in it: the sub-block cuts
// from the sampled flag words, a sub-block's alphabet and run range from its first-run row, which rank kernel a set of rows takes, the
// plan of a pass from its block sizes — which blocks are sampled and, once their cuts are known, the sub-block table the kernels read —
// and the word layout of that table in HBM.  Both forms of the front end (one block, a pass) are driven by it.
// tools/front_plan_probe.cpp reads the same from stdin, for tests/test_front_plan_host.py.
#pragma once
#include <stdint.h>
#include <stddef.h>
#include <vector>
#include "../host/qlfc.h"                                               // bschost::coder_num_blocks: sub-blocks of a block of n bytes

typedef unsigned long long qf_word;                                     // a split-flag word (dev_common.h: u64)

constexpr int      FRONT_MAX_BLOCKS = 4096;                             // blocks of a pass (dev_common.h: = BATCH_MAX_BLOCKS)
constexpr int      FRONT_MAX_SUB = 2 * FRONT_MAX_BLOCKS;                // a block of a pass lies below 1 MiB: at most two sub-blocks
constexpr uint32_t FRONT_NO_RUN = 0xffffffffu;                          // first-run entry of a symbol the sub-block does not hold

// ---- cuts ----------------------------------------------------------------------------------------------------------------------------
// The split samples positions 1, 33, 65, .. of a block (coder.cpp:70-109): flag bit q = (L[1 + 32 q] != L[32 q]), 64 to a word.
static inline uint32_t qlfc_split_samples(uint32_t n) { return n >= 2 ? (n - 1 + 31) / 32 : 0; }
static inline uint32_t qlfc_split_words(uint32_t n) { return (qlfc_split_samples(n) + 63) / 64; }

// coder.cpp:70-109 from the flag words: more sampled changes than sub-blocks — a cut wherever changes / nblocks of them have gone by, at
// that sampled position; else nblocks equal parts.  start / size: nblocks entries.
static inline void qlfc_pick_cuts(const qf_word* w, uint32_t nwords, uint32_t n, int nblocks, int* start, int* size)
{
    uint64_t changes = 0;
    for (uint32_t k = 0; k < nwords; ++k) changes += (uint64_t)__builtin_popcountll(w[k]);
    if (changes > (uint64_t)nblocks) {
        const uint64_t per = changes / (uint64_t)nblocks;
        int id = 0; uint64_t seen = 0;
        start[0] = 0;
        for (uint32_t k = 0; k < nwords && id < nblocks - 1; ++k) {
            qf_word bits = w[k];
            const uint64_t pc = (uint64_t)__builtin_popcountll(bits);
            if (seen + pc < per) { seen += pc; continue; }
            while (bits && id < nblocks - 1) {
                const int b = __builtin_ctzll(bits); bits &= bits - 1;
                if (++seen == per) {
                    seen = 0;
                    const int i = 1 + 32 * (int)(k * 64 + (uint32_t)b);
                    size[id] = i - start[id];
                    start[++id] = i;
                }
            }
        }
        size[nblocks - 1] = (int)n - start[nblocks - 1];
    } else {
        const int each = (int)n / nblocks;
        for (int p = 0; p < nblocks; ++p) { start[p] = each * p; size[p] = (p != nblocks - 1) ? each : (int)n - each * (nblocks - 1); }
    }
}

// ---- first-run rows ------------------------------------------------------------------------------------------------------------------
// A row: first_run[c] = index of the first run of symbol c in one sub-block, FRONT_NO_RUN: none.
// alphabet in order of first appearance = symbols sorted by the index of their first run (as block.cpp: host_prepare)
static inline void qlfc_front_first_seen(const uint32_t* first_run /*[256]*/, uint8_t* first_seen /*[256]*/, int* nsym)
{
    uint64_t order[256]; int k = 0;
    for (uint32_t s = 0; s < 256; ++s) if (first_run[s] != FRONT_NO_RUN) order[k++] = ((uint64_t)first_run[s] << 8) | s;
    for (int i = 1; i < k; ++i) { const uint64_t v = order[i]; int j = i; while (j > 0 && order[j - 1] > v) { order[j] = order[j - 1]; --j; } order[j] = v; }
    for (int i = 0; i < k; ++i) first_seen[i] = (uint8_t)(order[i] & 0xffu);
    *nsym = k;
}
// the first run of the sub-block itself = the smallest first run of its symbols (FRONT_NO_RUN: an empty row)
static inline uint32_t qlfc_front_row_first(const uint32_t* first_run /*[256]*/)
{
    uint32_t lo = FRONT_NO_RUN;
    for (int s = 0; s < 256; ++s) if (first_run[s] < lo) lo = first_run[s];
    return lo;
}
// The union alphabet of `rows` rows — the symbols that start a run anywhere in the block or pass — renumbered 0 .. K - 1 in byte order:
// lut[c] = the number of symbol c (0 for one that is absent; 255 at most, which only a wide alphabet reaches).  -> K
static inline uint32_t qlfc_front_alphabet(const uint32_t* first_run, size_t rows, uint8_t* lut /*[256]*/)
{
    bool present[256] = {};
    for (size_t i = 0; i < rows * 256; ++i) if (first_run[i] != FRONT_NO_RUN) present[i & 255u] = true;
    uint32_t K = 0;
    for (int s = 0; s < 256; ++s) { lut[s] = (uint8_t)(present[s] ? (K < 255 ? K : 255) : 0); K += present[s]; }
    return K;
}
// How the rank step holds a set of symbols: renumbered by lut in one 32-bit word, in one 64-bit word, or four words indexed by the byte
enum QfRankPath { QF_RANK_NARROW = 0, QF_RANK_DENSE = 1, QF_RANK_WIDE = 2 };
static inline QfRankPath qlfc_front_rank_path(uint32_t K) { return K <= 32 ? QF_RANK_NARROW : K <= 64 ? QF_RANK_DENSE : QF_RANK_WIDE; }

// ---- the plan of a pass --------------------------------------------------------------------------------------------------------------
// `count` blocks of sizes[b] bytes back to back.  -> their sum, or -1: count outside 0 .. FRONT_MAX_BLOCKS, a size outside
// [0, block_limit), a sum above cap.
static inline int64_t qlfc_pass_total(const int* sizes, int count, int block_limit, int64_t cap)
{
    if (count < 0 || count > FRONT_MAX_BLOCKS) return -1;
    int64_t total = 0;
    for (int b = 0; b < count; ++b) {
        if (sizes[b] < 0 || sizes[b] >= block_limit) return -1;
        total += sizes[b];
    }
    return total > cap ? -1 : total;
}
// sub-blocks of a block of a pass: an empty block has none
static inline int qlfc_pass_num_sub(int n) { return n == 0 ? 0 : bschost::coder_num_blocks(n); }

// Which blocks are sampled (those of more than one sub-block), in block order: table entry k = {first byte of the block in the pass,
// its length, its first flag word}, as qfb_split_flags_kernel reads it; nwords flag words in all, maxq samples in the longest.
struct QfPassFlags {
    std::vector<uint32_t> tab;
    uint32_t nwords = 0, maxq = 0;
    int sampled() const { return (int)(tab.size() / 3); }
};
static inline QfPassFlags qlfc_pass_flags(const int* sizes, int count)
{
    QfPassFlags F;
    uint64_t at = 0;
    for (int b = 0; b < count; ++b) {
        if (qlfc_pass_num_sub(sizes[b]) > 1) {
            const uint32_t nq = qlfc_split_samples((uint32_t)sizes[b]);
            F.tab.push_back((uint32_t)at); F.tab.push_back((uint32_t)sizes[b]); F.tab.push_back(F.nwords);
            F.nwords += qlfc_split_words((uint32_t)sizes[b]); if (nq > F.maxq) F.maxq = nq;
        }
        at += (uint64_t)sizes[b];
    }
    return F;
}
// After the cuts (words: the flag words of all sampled blocks, as F lays them out): blk_sub[0 .. count] = first sub-block of each block,
// sub_start / sub_size per sub-block relative to its block, and the table the kernels read in one piece —
//   sub_off[s]   first byte of sub-block s in the pass (strictly increasing: empty blocks have no sub-block), sub_off[nsub] = the total
//   sub_base[s]  first byte of the BLOCK that holds sub-block s (run starts are relative to it, as RunView expects), right behind sub_off
// -> nsub, or -1: more than FRONT_MAX_SUB sub-blocks (blocks below 1 MiB: cannot happen).
struct QfPassTable {
    std::vector<uint32_t> words;                                        // sub_off [nsub + 1], sub_base [nsub]
    int nsub = 0;
    const uint32_t* sub_off() const { return words.data(); }
    const uint32_t* sub_base() const { return words.data() + nsub + 1; }
};
static inline int qlfc_pass_table(const int* sizes, int count, const QfPassFlags& F, const qf_word* words, int* blk_sub, int* sub_start,
                                  int* sub_size, QfPassTable* T)
{
    std::vector<uint32_t> base;
    T->words.clear(); T->words.reserve((size_t)4 * count + 2);
    int nsub = 0, k = 0;
    uint64_t at = 0;
    for (int b = 0; b < count; ++b) {
        blk_sub[b] = nsub;
        const int nb = qlfc_pass_num_sub(sizes[b]);
        if (nsub + nb > FRONT_MAX_SUB) return -1;
        if (nb == 1) { sub_start[nsub] = 0; sub_size[nsub] = sizes[b]; }
        if (nb > 1) {
            qlfc_pick_cuts(words + F.tab[3 * (size_t)k + 2], qlfc_split_words((uint32_t)sizes[b]), (uint32_t)sizes[b], nb, sub_start + nsub, sub_size + nsub);
            ++k;
        }
        for (int q = 0; q < nb; ++q) { T->words.push_back((uint32_t)at + (uint32_t)sub_start[nsub + q]); base.push_back((uint32_t)at); }
        nsub += nb;
        at += (uint64_t)sizes[b];
    }
    blk_sub[count] = nsub;
    T->words.push_back((uint32_t)at);
    T->words.insert(T->words.end(), base.begin(), base.end());
    T->nsub = nsub;
    return nsub;
}

// ---- the table in HBM (bscgpu_ctx::front_tab), in u32 words --------------------------------------------------------------------------
// sub_off [nsub + 1] with sub_base [nsub] right behind it (one copy up); sub_run [nsub + 1], the first run of every sub-block; the flag
// table; first_run [nsub][256]
constexpr size_t FT_OFF = 0, FT_RUN = FT_OFF + 2 * (size_t)FRONT_MAX_SUB + 1, FT_FLAG = FT_RUN + FRONT_MAX_SUB + 1,
                 FT_FIRST = (FT_FLAG + 3 * (size_t)FRONT_MAX_BLOCKS + 63) / 64 * 64, FT_WORDS = FT_FIRST + (size_t)FRONT_MAX_SUB * 256;
static_assert(FT_RUN - FT_OFF >= 2 * (size_t)FRONT_MAX_SUB + 1 && FT_FLAG - FT_RUN >= (size_t)FRONT_MAX_SUB + 1, "the offsets and first runs of FRONT_MAX_SUB sub-blocks fit");
static_assert(FT_FIRST - FT_FLAG >= 3 * (size_t)FRONT_MAX_BLOCKS && FT_FIRST % 64 == 0, "the flag table of FRONT_MAX_BLOCKS sampled blocks fits; the rows start on a 256-byte line");

// Pinned bytes a pass's caller lends the driver: the larger of the flag words of every block (n_b / 256 + 8 bytes each) and the
// first-run table with sub_run; the flag words land there first, the table after the cuts have been read.
static inline size_t front_scratch_bytes(int64_t max_n)
{
    const size_t flags = (size_t)max_n / 256 + 8 * (size_t)FRONT_MAX_BLOCKS + 64, table = (size_t)FRONT_MAX_SUB * 1024 + 4 * (size_t)(FRONT_MAX_SUB + 1);
    return (flags > table ? flags : table) + 4096;
}
