// hist_resolve_probe.cpp — the exact resolve of open run_hist brackets (devcoder.hip 1c', BSCGPU_OPT_DC_HIST_EXACT) judged on the CPU:
// the host restatement of its kernels (devcoder_model.h: hist_resolve_host) against the plain serial walk of run_hist_next, and the
// bounds the resolve rests on.  The tests use it (tests/test_hist_resolve_host.py, tests/test_gpu_hist_resolve.py).  Not part of the
// product.
//   g++ -O2 -std=c++17 -march=x86-64-v3 -I libbsc_amd/csrc/host -I libbsc_amd/csrc/device -I include tools/hist_resolve_probe.cpp \
//       libbsc_amd/csrc/host/coder.cpp -o probe -lpthread
//   probe bound          exhaustively, over every pair a <= b of [0, 63] and every increment a run of up to 2^31 - 1 bytes can give (2 for
//                        a run of one byte, 3 b + 3 for b = bsr(run) = 1 .. 30): the update is monotone, the width behind one step is at
//                        most floor((b - a + 3) / 4), [0, 63] is invariant; the fixed points of every class
//   probe runs R.bin     R.bin: pairs of uint32 (chain, run length), the runs in symbol-major order as the device has them
//   probe block L.bin    a sorted block: sub-block split and run front end as the stage function has them, laid out symbol-major
// runs / block -> one JSON object: ext / resolved / chunks / groups / chain_steps as hist_resolve_host counts them, values_equal (every
// run's min(run_hist, 7) equals the serial walk's: the run_hist update of walk_model1, from 0 at the first run of a symbol in a sub-block).
#include "../libbsc_amd/csrc/host/qlfc.cpp"
#include "../libbsc_amd/csrc/device/devcoder_model.h"
#include <cstdio>
#include <string>
#include <vector>

using namespace bschost;
namespace bschost { void* bigbuf_get(size_t bytes) { return malloc(bytes); } void bigbuf_put(void* p) { free(p); } }

// serial[q]: min(run_hist, 7) in front of element q by the plain walk
static int report(const std::vector<uint64_t>& chain, const std::vector<uint32_t>& run, const std::vector<uint8_t>& serial, int nb)
{
    const uint32_t m = (uint32_t)run.size();
    dcm::HistResolve R;
    dcm::hist_resolve_host(chain.data(), run.data(), m, R);
    uint64_t diff = 0; int64_t first_diff = -1;
    for (uint32_t q = 0; q < m; ++q) if (R.hist[q] != serial[q]) { if (!diff) first_diff = q; ++diff; }
    printf("{\"runs\": %u, \"nb\": %d, \"ext\": %llu, \"resolved\": %llu, \"chunks\": %u, \"groups\": %u, \"chain_steps\": %u,\n"
           " \"values_equal\": %s, \"values_differ\": %llu, \"first_differ\": %lld}\n",
           m, nb, (unsigned long long)R.ext, (unsigned long long)R.resolved, R.chunks, R.groups, R.chain_steps,
           diff ? "false" : "true", (unsigned long long)diff, (long long)first_diff);
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
        bool monotone = true, contracts = true, invariant = true, inc_is_next = true;
        uint32_t max_inc = 0, max_image = 0;
        std::vector<uint32_t> incs(1, dcm::run_hist_inc(1u));
        for (uint32_t b = 1; b <= 30; ++b) {
            incs.push_back(dcm::run_hist_inc(1u << b));
            if (dcm::run_hist_inc((2u << b) - 1u) != incs.back()) inc_is_next = false;      // (the class is all the increment sees)
        }
        for (uint32_t r : {1u, 2u, 3u, 4u, 127u, 128u, 1u << 30, 0x7fffffffu})
            for (uint32_t h = 0; h < 64; ++h) if (dcm::run_hist_next(h, r) != (h + dcm::run_hist_inc(r)) >> 2) inc_is_next = false;
        for (uint32_t inc : incs) {
            if (inc > max_inc) max_inc = inc;
            for (uint32_t a = 0; a < 64; ++a)
                for (uint32_t b = a; b < 64; ++b) {
                    const uint32_t na = (a + inc) >> 2, nb = (b + inc) >> 2;
                    if (nb < na) monotone = false;
                    else if (nb - na > (b - a + 3u) / 4u) contracts = false;
                    if (nb > 63u) invariant = false;
                    if (nb > max_image) max_image = nb;
                }
        }
        uint32_t w[4] = {63, 0, 0, 0};
        for (int t = 1; t < 4; ++t) w[t] = (w[t - 1] + 3u) / 4u;
        // fixed points of every class (class 0: a run of one byte)
        bool two_fixed = true, others_closed = true;
        printf("{\"DC_HIST_NP\": %d, \"DC_HIST_CH\": %d, \"DC_HIST_CAND\": %d, \"DC_HIST_GROUP\": %d, \"fixed_points\": [", dcm::DC_HIST_NP, dcm::DC_HIST_CH, dcm::DC_HIST_CAND, dcm::DC_HIST_GROUP);
        for (uint32_t b = 0; b <= 30; ++b) {
            const uint32_t inc = incs[b];
            std::vector<uint32_t> fp;
            for (uint32_t h = 0; h < 64; ++h) if (((h + inc) >> 2) == h) fp.push_back(h);
            if (b >= 1 && b <= 6) { if (fp.size() != 2 || fp[0] != b || fp[1] != b + 1) two_fixed = false; }
            else for (uint32_t h : fp) for (uint32_t g : fp) if ((h < 7u ? h : 7u) != (g < 7u ? g : 7u)) others_closed = false;      // one clamped value
            printf("%s[", b ? ", " : "");
            for (size_t i = 0; i < fp.size(); ++i) printf("%s%u", i ? ", " : "", fp[i]);
            printf("]");
        }
        printf("],\n \"monotone\": %s, \"contracts_by_four\": %s, \"invariant_0_63\": %s, \"inc_is_next\": %s, \"max_inc\": %u, \"max_image\": %u,\n"
               " \"widths\": [%u, %u, %u, %u], \"two_fixed_points_classes_1_to_6\": %s, \"other_classes_one_clamped_value\": %s}\n",
               monotone ? "true" : "false", contracts ? "true" : "false", invariant ? "true" : "false", inc_is_next ? "true" : "false", max_inc, max_image,
               w[0], w[1], w[2], w[3], two_fixed ? "true" : "false", others_closed ? "true" : "false");
        return 0;
    }
    if (mode == "runs" && argc == 3) {
        std::vector<uint8_t> raw;
        if (!read_file(argv[2], raw) || raw.size() % 8) return 2;
        const uint32_t m = (uint32_t)(raw.size() / 8);
        const uint32_t* p = reinterpret_cast<const uint32_t*>(raw.data());
        std::vector<uint64_t> chain(m); std::vector<uint32_t> run(m); std::vector<uint8_t> serial(m);
        uint32_t h = 0;
        for (uint32_t q = 0; q < m; ++q) {
            chain[q] = p[2 * q]; run[q] = p[2 * q + 1];
            if (run[q] < 1u || run[q] > 0x7fffffffu) return 2;
            if (q == 0 || chain[q] != chain[q - 1]) h = 0;
            serial[q] = (uint8_t)(h < 7u ? h : 7u);
            h = dcm::run_hist_next(h, run[q]);
        }
        return report(chain, run, serial, 1);
    }
    if (mode == "block" && argc == 3) {
        std::vector<uint8_t> L;
        if (!read_file(argv[2], L)) return 2;
        const int nb = coder_num_blocks((int)L.size());
        int start[8], size[8];
        coder_split_blocks(L.data(), (int)L.size(), nb, start, size);
        // stream order: symbol, sub-block, length and the serial walk's value of every run
        std::vector<uint8_t> sym, sbs, hs;
        std::vector<uint32_t> len;
        for (int sb = 0; sb < nb; ++sb) {
            QlfcRuns R;
            qlfc_runs(L.data() + start[sb], size[sb], R);
            uint32_t h[256] = {0};
            for (uint32_t j = 0; j < R.view.count; ++j) {
                const uint32_t s = R.view.sym[j], l = R.view.len(j);
                sym.push_back((uint8_t)s); sbs.push_back((uint8_t)sb); len.push_back(l);
                hs.push_back((uint8_t)(h[s] < 7u ? h[s] : 7u));
                h[s] = dcm::run_hist_next(h[s], l);
            }
        }
        // symbol-major, stable: the device's 8-bit radix pass by symbol
        const uint32_t m = (uint32_t)sym.size();
        uint32_t at[257] = {0};
        for (uint32_t j = 0; j < m; ++j) ++at[sym[j] + 1u];
        for (int s = 0; s < 256; ++s) at[s + 1] += at[s];
        std::vector<uint64_t> chain(m); std::vector<uint32_t> run(m); std::vector<uint8_t> serial(m);
        for (uint32_t j = 0; j < m; ++j) {
            const uint32_t q = at[sym[j]]++;
            chain[q] = (uint64_t)sym[j] << 8 | sbs[j]; run[q] = len[j]; serial[q] = hs[j];
        }
        return report(chain, run, serial, nb);
    }
    fprintf(stderr, "usage: %s bound | runs R.bin | block L.bin\n", argv[0]);
    return 2;
}
