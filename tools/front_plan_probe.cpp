// front_plan_probe.cpp — drives the arithmetic of the QLFC front end (libbsc_amd/csrc/device/qlfc_front_plan.h) from stdin;
// tests/test_front_plan_host.py compares what it prints with the compiled reference's split, a few lines of Python, the layout
// bscgpu_front_batch_host builds and the values the table layout has always had.  No GPU, no HIP:
//   g++ -std=c++17 -I libbsc_amd/csrc/device tools/front_plan_probe.cpp -o front_plan_probe
// (the test also builds it with -fsanitize=address,undefined and runs that program on the same input).
// One question per line on stdin, a word and numbers separated by blanks (flag words in hex); one JSON object per line on stdout:
//   cuts n nblocks nwords w[nwords]            qlfc_split_samples / _words of n, and qlfc_pick_cuts of the words
//   rows nrows  { k  sym first  x k } x nrows  per row: qlfc_front_first_seen and qlfc_front_row_first; of all rows: qlfc_front_alphabet
//                                              (K, lut) and qlfc_front_rank_path
//   pass count limit cap sizes[count] nwords w[nwords]
//                                              qlfc_pass_total; qlfc_pass_flags (table, nwords, maxq); with as many flag words as
//                                              that asks for, qlfc_pass_table: nsub, blk_sub, sub_start, sub_size, sub_off, sub_base
//   layout max_n                               the FT_* words, the limits and front_scratch_bytes
#include "qlfc_front_plan.h"
#include <cstdio>
#include <cstring>
#include <vector>

template <class T> static void print_list(const char* name, const T* v, size_t n, bool first = false)
{
    printf("%s\"%s\":[", first ? "" : ",", name);
    for (size_t i = 0; i < n; ++i) printf("%s%lld", i ? "," : "", (long long)v[i]);
    printf("]");
}

static bool read_words(std::vector<qf_word>& w)
{
    long long count;
    if (scanf("%lld", &count) != 1 || count < 0 || count > (1 << 22)) return false;
    w.assign((size_t)count + 1, 0);                                     // (+ 1: data() of an empty list must still be a pointer)
    for (long long i = 0; i < count; ++i) if (scanf("%llx", &w[(size_t)i]) != 1) return false;
    w.pop_back();
    return true;
}

static bool asked(const char* word)
{
    if (!strcmp(word, "cuts")) {
        long long n; int nblocks;
        std::vector<qf_word> w;
        if (scanf("%lld %d", &n, &nblocks) != 2 || n < 0 || nblocks < 1 || nblocks > 8 || !read_words(w)) return false;
        int start[8], size[8];
        qlfc_pick_cuts(w.data(), (uint32_t)w.size(), (uint32_t)n, nblocks, start, size);
        printf("{\"samples\":%u,\"words\":%u", qlfc_split_samples((uint32_t)n), qlfc_split_words((uint32_t)n));
        print_list("start", start, (size_t)nblocks); print_list("size", size, (size_t)nblocks);
        printf("}\n");
        return true;
    }
    if (!strcmp(word, "rows")) {
        int nrows;
        if (scanf("%d", &nrows) != 1 || nrows < 0 || nrows > FRONT_MAX_SUB) return false;
        std::vector<uint32_t> first_run((size_t)nrows * 256 + 1, FRONT_NO_RUN);
        for (int r = 0; r < nrows; ++r) {
            int k;
            if (scanf("%d", &k) != 1 || k < 0 || k > 256) return false;
            for (int i = 0; i < k; ++i) {
                int sym; long long first;
                if (scanf("%d %lld", &sym, &first) != 2 || sym < 0 || sym > 255) return false;
                first_run[(size_t)r * 256 + (size_t)sym] = (uint32_t)first;
            }
        }
        printf("{\"rows\":[");
        for (int r = 0; r < nrows; ++r) {
            uint8_t seen[256]; int nsym = -1;
            qlfc_front_first_seen(first_run.data() + (size_t)r * 256, seen, &nsym);
            printf("%s{\"first\":%lld", r ? "," : "", (long long)qlfc_front_row_first(first_run.data() + (size_t)r * 256));
            print_list("first_seen", seen, (size_t)nsym);
            printf("}");
        }
        uint8_t lut[256];
        memset(lut, 0xa5, sizeof lut);
        const uint32_t K = qlfc_front_alphabet(first_run.data(), (size_t)nrows, lut);
        printf("],\"K\":%u,\"path\":%d", K, (int)qlfc_front_rank_path(K));
        print_list("lut", lut, 256);
        printf("}\n");
        return true;
    }
    if (!strcmp(word, "pass")) {
        int count, limit; long long cap;
        if (scanf("%d %d %lld", &count, &limit, &cap) != 3 || count < -1 || count > 2 * FRONT_MAX_BLOCKS) return false;
        std::vector<int> sizes((size_t)(count > 0 ? count : 0) + 1, 0);
        for (int b = 0; b < count; ++b) if (scanf("%d", &sizes[(size_t)b]) != 1) return false;
        std::vector<qf_word> w;
        if (!read_words(w)) return false;
        const int64_t total = qlfc_pass_total(sizes.data(), count, limit, cap);
        printf("{\"total\":%lld", (long long)total);
        if (total >= 0) {
            const QfPassFlags F = qlfc_pass_flags(sizes.data(), count);
            printf(",\"sampled\":%d,\"nwords\":%u,\"maxq\":%u", F.sampled(), F.nwords, F.maxq);
            print_list("flag_tab", F.tab.data(), F.tab.size());
            if (w.size() == F.nwords) {
                std::vector<int> blk_sub((size_t)count + 1, -7), sub_start((size_t)8 * count + 1, -7), sub_size((size_t)8 * count + 1, -7);   // (a block has at most eight)
                QfPassTable T;
                const int nsub = qlfc_pass_table(sizes.data(), count, F, w.data(), blk_sub.data(), sub_start.data(), sub_size.data(), &T);
                printf(",\"nsub\":%d", nsub);
                if (nsub >= 0) {
                    print_list("blk_sub", blk_sub.data(), (size_t)count + 1);
                    print_list("sub_start", sub_start.data(), (size_t)nsub); print_list("sub_size", sub_size.data(), (size_t)nsub);
                    print_list("sub_off", T.sub_off(), (size_t)nsub + 1); print_list("sub_base", T.sub_base(), (size_t)nsub);
                    printf(",\"table_words\":%zu", T.words.size());
                }
            }
        }
        printf("}\n");
        return true;
    }
    if (!strcmp(word, "layout")) {
        long long max_n;
        if (scanf("%lld", &max_n) != 1 || max_n < 0) return false;
        printf("{\"FT_OFF\":%zu,\"FT_RUN\":%zu,\"FT_FLAG\":%zu,\"FT_FIRST\":%zu,\"FT_WORDS\":%zu,\"max_blocks\":%d,\"max_sub\":%d,\"scratch\":%zu}\n",
               FT_OFF, FT_RUN, FT_FLAG, FT_FIRST, FT_WORDS, FRONT_MAX_BLOCKS, FRONT_MAX_SUB, front_scratch_bytes(max_n));
        return true;
    }
    return false;
}

int main()
{
    char word[24];
    while (scanf("%23s", word) == 1) if (!asked(word)) return 1;
    return 0;
}
