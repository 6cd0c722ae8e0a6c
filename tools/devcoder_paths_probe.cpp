// devcoder_paths_probe.cpp — which exits of the device coder (devcoder.hip) a sorted block MUST take, judged on the CPU from the run
// sequence alone.  The tests use it so that a GPU test of a rare path cannot pass on an input that quietly missed the path
// (tests/test_devcoder_paths.py, tests/test_gpu_devcoder_paths.py).  Not part of the product.
//   g++ -O2 -std=c++17 -march=x86-64-v3 -I libbsc_amd/csrc/host -I libbsc_amd/csrc/device -I include tools/devcoder_paths_probe.cpp \
//       libbsc_amd/csrc/host/coder.cpp -o probe -lpthread
//   probe L.bin      -> one JSON object on stdout
//   probe L.bin replay_exact   the same with BSCGPU_OPT_DC_REPLAY_EXACT on: open chunk starts are resolved exactly whatever the length of
//                    the stretch (no bracket exceeds the resolve's cap: tools/replay_resolve_probe.cpp bound), so no chunk is replayed and
//                    FAIL_REPLAY is not among the exits; the object gains "replay_exact": true.  How many chunks the resolve settles
//                    depends on the chain-major layout: replay_resolve_probe block L.bin.
//   probe L.bin [avg_exact] [hist_exact] [replay_exact]   any of the three option words, in any order: the mask the stage must return
//                    under that option set.  With R the block's reasons among AVG and HIST and O the options that are on: if R \ O is
//                    not empty the mask is exactly R \ O (both exits are judged at the first sync, the evaluation never runs: REPLAY is
//                    never beside them); else 16 if a stretch exceeds fail_min and replay_exact is off; else 0.  The counts (avg_und,
//                    hist_ext, hist_fail, the stretches) do not depend on the options; every option word that is on is echoed as true.
//   probe L.bin option_sets [...]   also "fail_mask_by_option_set": the masks of all eight option sets from the one walk, indexed by
//                    avg_exact + 2 hist_exact + 4 replay_exact.
//
// What is computed, per block (sub-block split and run / rank front end as the stage function has them):
//   avg_und      runs whose avg_rank >= 32 flag stays undecided under dc_avg_kernel's rule: chunks of DC_AVG_CH runs of the block's run
//                array, a [0, 255] bracket started DC_AVG_WARM runs early (exact where that reaches the sub-block's first run), reset at
//                sub-block starts.  0 when no sub-block has more than 32 symbols (the kernel is not launched).  Any -> FAIL_AVG.
//   hist_ext     runs whose run_hist bracket over the DC_HIST_NP nearest earlier runs of their symbol stays open (clamped ends differ);
//                hist_closed[k] how many of them close at the k-th widening of the look-back (4 NP, 16 NP, ...), hist_fail how many
//                are still open at the last one (the first K >= DC_HIST_KMAX) with the chain's start out of reach.  Any -> FAIL_HIST.
//   families     for the state, char and static counter families: over all chains (a chain = one counter slot of the reference model:
//                the three slots of every decision come from the host walker itself) the largest event count, the longest STRETCH (and
//                the longest per decision class) —
//                events over which the bracket [vmin, vmax] of the chain's class, restarted wherever it last met, has not met — and
//                RISK, the longest run of consecutive stretches i with len(i) + len(i + 1) > EV.
//
// What follows from the stretches whatever the chain-major layout puts where (EV = events per evaluation chunk of this block; the maps
// are monotone, so a bracket started later encloses one started earlier: the end e(p) of a bracket started at p never decreases with p):
//   stretch >= 3 EV                  some chunk boundary p lies in (a, a + EV]; the chunk at p is inside the chain, has not met by p + EV
//                                    <= b, and the chunk behind it continues the chain: at least one replay.
//   stretch > (DC_REPLAY_MAX + 2) EV DC_REPLAY_MAX + 1 such chunks in a row, and one more behind them: FAIL_REPLAY.
//   risk == 0                        every bracket started anywhere meets within EV events: no replay.
//   risk <= DC_REPLAY_MAX EV         DC_REPLAY_MAX + 1 chunks in a row that do not meet would span more than that: no FAIL_REPLAY.
#include "../libbsc_amd/csrc/host/qlfc.cpp"
#include "../libbsc_amd/csrc/device/devcoder_model.h"
#include <cstdio>
#include <memory>
#include <vector>

using namespace bschost;
// (coder.cpp's only needs beyond qlfc.cpp: the big-buffer pool of the block driver, which nothing here reaches)
namespace bschost { void* bigbuf_get(size_t bytes) { return malloc(bytes); } void bigbuf_put(void* p) { free(p); } }

struct Chain { short lo, hi; uint8_t live; uint32_t events, len, prev; uint64_t run; };
struct FamStat { uint32_t max_events = 0, stretch = 0, by_class[dcm::NUM_CLS] = {0}; uint64_t risk = 0; };      // (classes as the host walker numbers them: NM2 is NM)

struct ProbePolicy {
    Counters1* base; const dcm::ModelParams* M; uint32_t EV;
    std::vector<Chain>* chains;            // [3]: per family, indexed by the slot's offset in Counters1
    FamStat* fam;                          // [3]
    uint64_t decisions = 0;
    struct Live {}; inline Live enter() { return Live(); } inline void leave(const Live&) {}
    inline bool begin_run() { return true; }
    // stretch i + 1 (length next; 0 at the chain's end) is known: settle stretch i = c.prev
    static inline void settle(Chain& c, uint32_t next, uint32_t EV, FamStat& F)
    {
        if ((uint64_t)c.prev + next > EV) { c.run += c.prev; if (c.run > F.risk) F.risk = c.run; } else c.run = 0;
        c.prev = next;
    }
    inline void one(int f, int cls, size_t slot, unsigned bit)
    {
        Chain& c = chains[f][slot];
        const dcm::Rates& R = M->rates[cls][f];
        if (!c.live) { c.live = 1; c.lo = M->vmin[cls][f]; c.hi = M->vmax[cls][f]; c.events = c.len = c.prev = 0; c.run = 0; }
        c.lo = (short)dcm::step(c.lo, bit, R); c.hi = (short)dcm::step(c.hi, bit, R);
        ++c.events; ++c.len;
        FamStat& F = fam[f];
        if (c.events > F.max_events) F.max_events = c.events;
        if (c.len > F.by_class[cls]) { F.by_class[cls] = c.len; if (c.len > F.stretch) F.stretch = c.len; }
        if (c.lo == c.hi) { settle(c, c.len, EV, F); c.len = 0; c.lo = M->vmin[cls][f]; c.hi = M->vmax[cls][f]; }
    }
    template <int CLS> inline void decide(Live&, unsigned bit, short& st, short& ch, short& sp, Mixer*)
    {
        const short* b = reinterpret_cast<const short*>(base);
        one(dcm::FAM_STATE, CLS, (size_t)(&st - b), bit); one(dcm::FAM_CHAR, CLS, (size_t)(&ch - b), bit); one(dcm::FAM_STATIC, CLS, (size_t)(&sp - b), bit);
        ++decisions;
    }
    void finish()
    {
        for (int f = 0; f < 3; ++f) for (Chain& c : chains[f]) if (c.live) { settle(c, c.len, EV, fam[f]); settle(c, 0, EV, fam[f]); c.live = 0; }
    }
};

struct CountPolicy {                       // decisions of a sub-block (the chunk size depends on the block's total)
    uint64_t decisions = 0;
    struct Live {}; inline Live enter() { return Live(); } inline void leave(const Live&) {}
    inline bool begin_run() { return true; }
    template <int CLS> inline void decide(Live&, unsigned, short&, short&, short&, Mixer*) { ++decisions; }
};

int main(int argc, char** argv)
{
    if (argc < 2) { fprintf(stderr, "usage: %s L.bin [avg_exact] [hist_exact] [replay_exact]\n", argv[0]); return 2; }
    bool avg_exact = false, hist_exact = false, replay_exact = false, option_sets = false;
    for (int a = 2; a < argc; ++a) {
        if (!strcmp(argv[a], "avg_exact")) avg_exact = true;
        else if (!strcmp(argv[a], "hist_exact")) hist_exact = true;
        else if (!strcmp(argv[a], "replay_exact")) replay_exact = true;
        else if (!strcmp(argv[a], "option_sets")) option_sets = true;
        else { fprintf(stderr, "%s: unknown option word %s\n", argv[0], argv[a]); return 2; }
    }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    fseek(f, 0, SEEK_END); const long n = ftell(f); fseek(f, 0, SEEK_SET);
    std::vector<uint8_t> L((size_t)n);
    if (n <= 0 || fread(L.data(), 1, (size_t)n, f) != (size_t)n) return 2;
    fclose(f);
    const int nb = coder_num_blocks((int)n);
    int start[8], size[8];
    coder_split_blocks(L.data(), (int)n, nb, start, size);
    const QlfcTables& T = qlfc_tables();
    dcm::ModelParams M; dcm::model_params_from_table(kStaticParams, M);

    std::vector<QlfcRuns> R((size_t)nb);
    int max_rank[8]; uint32_t first[9]; first[0] = 0;
    std::unique_ptr<Counters1> K(new_counters());
    uint64_t D = 0, sub_dec[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    bool may_escape = false;
    for (int sb = 0; sb < nb; ++sb) {
        qlfc_runs(L.data() + start[sb], size[sb], R[sb]);
        max_rank[sb] = encode_alphabet(R[sb].view, [](unsigned) {});
        may_escape |= max_rank[sb] > 4;
        first[sb + 1] = first[sb] + R[sb].view.count;
        CountPolicy cp; walk_model1<false>(R[sb].view, T, max_rank[sb], *K, nullptr, cp);
        D += cp.decisions; sub_dec[sb] = cp.decisions;
    }
    const uint32_t m = first[nb];
    const uint32_t EV = dcm::eval_chunk_events(3 * D);           // jobs: static + char + (state: rank side + run side)

    // ---- avg_rank: dc_avg_kernel's rule over the block's run array
    std::vector<uint8_t> rank(m);
    for (int sb = 0; sb < nb; ++sb) memcpy(rank.data() + first[sb], R[sb].view.rank, R[sb].view.count);
    uint64_t avg_und = 0, avg_und_sb[8] = {0};
    if (may_escape) {
        for (uint64_t j0 = 0; j0 < m; j0 += dcm::DC_AVG_CH) {
            const uint32_t j1 = (uint32_t)(j0 + dcm::DC_AVG_CH < m ? j0 + dcm::DC_AVG_CH : m);
            int sb = 0;
            for (int b = 1; b < nb; ++b) if (j0 >= first[b]) sb = b;
            const uint32_t sbf = first[sb];
            const uint32_t w0 = (uint32_t)j0 > sbf + dcm::DC_AVG_WARM ? (uint32_t)j0 - dcm::DC_AVG_WARM : sbf;
            uint32_t lo = 0, hi = w0 == sbf ? 0u : 255u;
            for (uint32_t j = w0; j < (uint32_t)j0; ++j) { lo = dcm::avg_rank_next(lo, rank[j]); hi = dcm::avg_rank_next(hi, rank[j]); }
            for (uint32_t j = (uint32_t)j0; j < j1; ++j) {
                if (sb + 1 < nb && j == first[sb + 1]) { lo = hi = 0; ++sb; }
                if ((lo >= 32u) != (hi >= 32u)) { ++avg_und; ++avg_und_sb[sb]; }
                lo = dcm::avg_rank_next(lo, rank[j]); hi = dcm::avg_rank_next(hi, rank[j]);
            }
        }
    }

    // ---- run_hist: dc_ctx_kernel's brackets over the earlier runs of the run's symbol in its sub-block
    uint64_t hist_ext = 0, hist_fail = 0, hist_closed[16] = {0};
    int hist_steps = 0;
    for (uint32_t K2 = 4 * dcm::DC_HIST_NP;; K2 *= 4) { ++hist_steps; if (K2 >= (uint32_t)dcm::DC_HIST_KMAX) break; }
    for (int sb = 0; sb < nb; ++sb) {
        const RunView& V = R[sb].view;
        std::vector<std::vector<uint32_t>> prev(256);
        auto clamp7 = [](uint32_t h) { return h < 7u ? h : 7u; };
        for (uint32_t j = 0; j < V.count; ++j) {
            std::vector<uint32_t>& P = prev[V.sym[j]];
            const size_t np = P.size();
            auto walk = [&](size_t cnt, bool exact, uint32_t& cl, uint32_t& ch) {
                uint32_t lo = 0, hi = exact ? 0u : 63u;
                for (size_t t = np - cnt; t < np; ++t) { lo = dcm::run_hist_next(lo, P[t]); hi = dcm::run_hist_next(hi, P[t]); }
                cl = clamp7(lo); ch = clamp7(hi);
            };
            uint32_t cl, ch;
            walk(np < (size_t)dcm::DC_HIST_NP ? np : (size_t)dcm::DC_HIST_NP, np < (size_t)dcm::DC_HIST_NP, cl, ch);
            if (cl != ch) {
                ++hist_ext;
                int stepno = 0;
                for (uint32_t K2 = 4 * dcm::DC_HIST_NP;; K2 *= 4, ++stepno) {
                    walk(np < K2 ? np : K2, np < K2, cl, ch);
                    if (cl == ch) { ++hist_closed[stepno]; break; }
                    if (K2 >= (uint32_t)dcm::DC_HIST_KMAX) { ++hist_fail; break; }
                }
            }
            P.push_back(V.len(j));
        }
    }

    // ---- counter chains
    std::vector<Chain> chains[3];
    for (int fam = 0; fam < 3; ++fam) chains[fam].assign(sizeof(Counters1) / sizeof(short), Chain{0, 0, 0, 0, 0, 0, 0});
    FamStat F[3];
    for (int sb = 0; sb < nb; ++sb) {
        ProbePolicy pol{K.get(), &M, EV, chains, F};
        walk_model1<false>(R[sb].view, T, max_rank[sb], *K, nullptr, pol);
        pol.finish();
    }

    const uint64_t replay_min = 3ull * EV, fail_min = (uint64_t)(dcm::DC_REPLAY_MAX + 2) * EV, keep_max = (uint64_t)dcm::DC_REPLAY_MAX * EV;
    uint32_t stretch = 0; uint64_t risk = 0;
    for (int fam = 0; fam < 3; ++fam) { if (F[fam].stretch > stretch) stretch = F[fam].stretch; if (F[fam].risk > risk) risk = F[fam].risk; }
    // include/bscgpu.h: BSCGPU_DC_FAIL_*.  (With an option on every open flag is resolved: avg_resolve_probe; every open bracket:
    // hist_resolve_probe.  An earlier exit stops the evaluation: a block declined for its contexts is never replayed)
    auto mask_under = [&](bool avg_on, bool hist_on, bool replay_on) {
        const int first_sync = (avg_und && !avg_on ? 2 : 0) | (hist_fail && !hist_on ? 4 : 0);
        return first_sync ? first_sync : stretch > fail_min && !replay_on ? 16 : 0;
    };
    int mask = mask_under(avg_exact, hist_exact, true);
    const bool fail_replay = mask == 0 && stretch > fail_min && !replay_exact;
    const bool no_fail_replay = mask != 0 || risk <= keep_max || replay_exact;
    if (fail_replay) mask |= 16;

    printf("{\"n\": %ld, \"nb\": %d, \"runs\": %u, \"decisions\": %llu, \"ev\": %u,\n", n, nb, m, (unsigned long long)D, EV);
    printf(" \"constants\": {\"DC_EV\": %d, \"DC_REPLAY_MAX\": %d, \"DC_AVG_CH\": %d, \"DC_AVG_WARM\": %d, \"DC_HIST_NP\": %d, \"DC_HIST_KMAX\": %d},\n",
           dcm::DC_EV, dcm::DC_REPLAY_MAX, dcm::DC_AVG_CH, dcm::DC_AVG_WARM, dcm::DC_HIST_NP, dcm::DC_HIST_KMAX);
    printf(" \"sub_runs\": ["); for (int sb = 0; sb < nb; ++sb) printf("%s%u", sb ? ", " : "", first[sb + 1] - first[sb]); printf("],\n");
    printf(" \"sub_decisions\": ["); for (int sb = 0; sb < nb; ++sb) printf("%s%llu", sb ? ", " : "", (unsigned long long)sub_dec[sb]); printf("],\n");
    printf(" \"max_rank\": ["); for (int sb = 0; sb < nb; ++sb) printf("%s%d", sb ? ", " : "", max_rank[sb]); printf("],\n");
    printf(" \"avg_launched\": %s, \"avg_und\": %llu, \"avg_und_sb\": [", may_escape ? "true" : "false", (unsigned long long)avg_und);
    for (int sb = 0; sb < nb; ++sb) printf("%s%llu", sb ? ", " : "", (unsigned long long)avg_und_sb[sb]); printf("],\n");
    printf(" \"hist_ext\": %llu, \"hist_fail\": %llu, \"hist_closed\": [", (unsigned long long)hist_ext, (unsigned long long)hist_fail);
    for (int s = 0; s < hist_steps; ++s) printf("%s%llu", s ? ", " : "", (unsigned long long)hist_closed[s]); printf("],\n");
    static const char* names[3] = {"state", "char", "static"};
    printf(" \"families\": {");
    for (int fam = 0; fam < 3; ++fam) {
        printf("%s\"%s\": {\"max_events\": %u, \"stretch\": %u, \"risk\": %llu, \"stretch_by_class\": [", fam ? ", " : "", names[fam], F[fam].max_events,
               F[fam].stretch, (unsigned long long)F[fam].risk);
        for (int c = 0; c < dcm::NUM_CLS - 1; ++c) printf("%s%u", c ? ", " : "", F[fam].by_class[c]);
        printf("]}");
    }
    printf("},\n");
    printf(" \"replay_min\": %llu, \"fail_min\": %llu, \"keep_max\": %llu,\n", (unsigned long long)replay_min, (unsigned long long)fail_min, (unsigned long long)keep_max);
    // fail_mask: the reason mask the stage must return (0: none of the exits judged here is certain); the three booleans say what is CERTAIN
    if (option_sets) {
        printf(" \"fail_mask_by_option_set\": [");
        for (int o = 0; o < 8; ++o) printf("%s%d", o ? ", " : "", mask_under(o & 1, o & 2, o & 4));
        printf("],\n");
    }
    if (avg_exact) printf(" \"avg_exact\": true,\n");
    if (hist_exact) printf(" \"hist_exact\": true,\n");
    if (replay_exact) printf(" \"replay_exact\": true,\n");
    printf(" \"fail_mask\": %d, \"replay_certain\": %s, \"no_replay_certain\": %s, \"no_fail_replay_certain\": %s}\n", mask,
           (mask == 0 || fail_replay) && stretch >= replay_min && !replay_exact ? "true" : "false", (mask & ~16) != 0 || risk == 0 || replay_exact ? "true" : "false",
           no_fail_replay ? "true" : "false");
    return 0;
}
