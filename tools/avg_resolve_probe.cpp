// avg_resolve_probe.cpp — the exact resolve of open avg_rank flags (devcoder.hip 1a', BSCGPU_OPT_DC_AVG_EXACT) judged on the CPU: the
// host restatement of its kernels (devcoder_model.h: avg_resolve_host) against the plain serial walk of avg_rank_next, and the bound
// the resolve rests on.  The tests use it (tests/test_avg_resolve_host.py, tests/test_gpu_avg_resolve.py).  Not part of the product.
//   g++ -O2 -std=c++17 -march=x86-64-v3 -I libbsc_amd/csrc/host -I libbsc_amd/csrc/device -I include tools/avg_resolve_probe.cpp \
//       libbsc_amd/csrc/host/coder.cpp -o probe -lpthread
//   probe bound                     the width recursion d' = floor(124 d / 128) + 1 from 255 over DC_AVG_WARM steps, and the widest
//                                   bracket [0, 255] leaves behind DC_AVG_WARM runs of one constant rank, over all 256 ranks
//   probe ranks R.bin F.txt         R.bin: one rank byte per run; F.txt: nsub, then first_run[0 .. nsub] and top[0 .. nsub)
//   probe block L.bin               a sorted block: sub-block split and run / rank front end as the stage function has them, top 255
// ranks / block -> one JSON object: und / resolved / left as avg_resolve_host counts them, flags_equal (every ge32 flag equals the
// serial walk's), domain_ok (every chunk's exact start equals the serial walk's value there and lies in its [lo0, hi0]), max_width,
// chain_steps, launched (block: some sub-block has more than 32 symbols; else the device does not run the kernels at all).
#include "../libbsc_amd/csrc/host/qlfc.cpp"
#include "../libbsc_amd/csrc/device/devcoder_model.h"
#include <cstdio>
#include <string>
#include <vector>

using namespace bschost;
namespace bschost { void* bigbuf_get(size_t bytes) { return malloc(bytes); } void bigbuf_put(void* p) { free(p); } }

static int report(const std::vector<uint8_t>& rank, const std::vector<uint32_t>& first, const std::vector<uint32_t>& top, bool launched)
{
    const uint32_t m = (uint32_t)rank.size(), nsub = (uint32_t)top.size();
    std::vector<uint8_t> ge32(m), serial(m);
    std::vector<uint32_t> at(m);                                       // avg_rank in front of every run
    for (uint32_t s = 0; s < nsub; ++s) {
        uint32_t avg = 0;
        for (uint32_t j = first[s]; j < first[s + 1]; ++j) { at[j] = avg; serial[j] = (uint8_t)(avg >= 32u); avg = dcm::avg_rank_next(avg, rank[j]); }
    }
    dcm::AvgResolve R;
    dcm::avg_resolve_host(rank.data(), m, first.data(), nsub, top.data(), ge32.data(), R);
    uint64_t diff = 0; int64_t first_diff = -1;
    for (uint32_t j = 0; j < m; ++j) if (ge32[j] != serial[j]) { if (!diff) first_diff = j; ++diff; }
    bool domain_ok = true;
    for (size_t c = 0; c < R.exact.size(); ++c) {
        const uint32_t x = at[c * dcm::DC_AVG_CH];
        if (R.exact[c] != x || x < R.lo0[c] || x > R.hi0[c]) domain_ok = false;
    }
    uint64_t sub_left = 0; for (uint32_t v : R.sub_left) sub_left += v;
    printf("{\"runs\": %u, \"nsub\": %u, \"chunks\": %zu, \"launched\": %s, \"und\": %llu, \"resolved\": %llu, \"left\": %llu, \"sub_left\": %llu,\n"
           " \"flags_equal\": %s, \"flags_differ\": %llu, \"first_differ\": %lld, \"domain_ok\": %s, \"max_width\": %u, \"chain_steps\": %u}\n",
           m, nsub, R.exact.size(), launched ? "true" : "false", (unsigned long long)R.und, (unsigned long long)R.resolved, (unsigned long long)R.left,
           (unsigned long long)sub_left, diff ? "false" : "true", (unsigned long long)diff, (long long)first_diff, domain_ok ? "true" : "false", R.max_width, R.chain_steps);
    return 0;
}

static bool read_file(const char* path, std::vector<uint8_t>& out)
{
    FILE* f = fopen(path, "rb");
    if (!f) { perror(path); return false; }
    fseek(f, 0, SEEK_END); const long n = ftell(f); fseek(f, 0, SEEK_SET);
    out.resize(n > 0 ? (size_t)n : 0);
    const bool ok = n > 0 && fread(out.data(), 1, (size_t)n, f) == (size_t)n;
    fclose(f);
    return ok;
}

int main(int argc, char** argv)
{
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "bound") {
        uint32_t d = 255;
        for (int t = 0; t < dcm::DC_AVG_WARM; ++t) d = 124u * d / 128u + 1u;
        uint32_t d128 = 255;
        for (int t = 0; t < 128; ++t) d128 = 124u * d128 / 128u + 1u;
        uint32_t widest = 0;
        for (uint32_t r = 0; r < 256; ++r) {
            uint32_t lo = 0, hi = 255;
            for (int t = 0; t < dcm::DC_AVG_WARM; ++t) { lo = dcm::avg_rank_next(lo, r); hi = dcm::avg_rank_next(hi, r); }
            if (hi - lo > widest) widest = hi - lo;
        }
        printf("{\"DC_AVG_CH\": %d, \"DC_AVG_WARM\": %d, \"DC_AVG_CAND\": %d, \"DC_AVG_GROUP\": %d, \"recursion_width\": %u, \"recursion_width_128\": %u, \"constant_rank_width\": %u}\n",
               dcm::DC_AVG_CH, dcm::DC_AVG_WARM, dcm::DC_AVG_CAND, dcm::DC_AVG_GROUP, d, d128, widest);
        return 0;
    }
    if (mode == "ranks" && argc == 4) {
        std::vector<uint8_t> rank;
        if (!read_file(argv[2], rank)) return 2;
        FILE* f = fopen(argv[3], "r");
        if (!f) { perror(argv[3]); return 2; }
        unsigned nsub = 0;
        if (fscanf(f, "%u", &nsub) != 1 || nsub < 1) return 2;
        std::vector<uint32_t> first(nsub + 1), top(nsub);
        for (auto& v : first) if (fscanf(f, "%u", &v) != 1) return 2;
        for (auto& v : top) if (fscanf(f, "%u", &v) != 1) return 2;
        fclose(f);
        if (first[0] != 0 || first[nsub] != rank.size()) return 2;
        for (unsigned s = 0; s < nsub; ++s) if (first[s] >= first[s + 1]) return 2;
        return report(rank, first, top, true);
    }
    if (mode == "block" && argc == 3) {
        std::vector<uint8_t> L;
        if (!read_file(argv[2], L)) return 2;
        const int nb = coder_num_blocks((int)L.size());
        int start[8], size[8];
        coder_split_blocks(L.data(), (int)L.size(), nb, start, size);
        std::vector<uint8_t> rank;
        std::vector<uint32_t> first(1, 0), top;
        bool launched = false;
        for (int sb = 0; sb < nb; ++sb) {
            QlfcRuns R;
            qlfc_runs(L.data() + start[sb], size[sb], R);
            launched |= encode_alphabet(R.view, [](unsigned) {}) > 4;
            rank.insert(rank.end(), R.view.rank, R.view.rank + R.view.count);
            first.push_back((uint32_t)rank.size()); top.push_back(255u);
        }
        return report(rank, first, top, launched);
    }
    fprintf(stderr, "usage: %s bound | ranks R.bin F.txt | block L.bin\n", argv[0]);
    return 2;
}
