// replay_resolve_probe.cpp — the exact resolve of open chunk starts (devcoder.hip 3', BSCGPU_OPT_DC_REPLAY_EXACT) judged on the CPU: the
// bound its candidate cap rests on, and the host restatement of its kernels (devcoder_model.h: replay_resolve_host) against the plain
// serial walk of every chain.  The tests use it (tests/test_replay_resolve_host.py, tests/test_gpu_replay_resolve.py).  Not part of the
// product.
//   g++ -O2 -std=c++17 -march=x86-64-v3 -I libbsc_amd/csrc/host -I libbsc_amd/csrc/device -I include tools/replay_resolve_probe.cpp \
//       libbsc_amd/csrc/host/coder.cpp -o probe -lpthread
//   probe bound                 for both coders, every class and family: (a) exhaustively over all value pairs v < u of the attainable range
//                               and both bits, u' - v' <= d - floor(d a / 4096) with d = u - v and a the bit's rate; (b) from that, the
//                               widest bracket (values) DC_EV steps can leave of the whole range: the recursion's fixed point; (c) the
//                               widest bracket any periodic bit pattern of period <= 8 really leaves.  cap = (b) rounded up to wavefronts.
//   probe block L.bin [cand]    a sorted block: the static coder's four evaluation jobs laid out chain-major as the device has them (row =
//                               decision type, inside a row X-major, inside that stream order), then the evaluation with and without
//                               the resolve: which exit the block must take either way and how many chunks the resolve settles
//   probe events E.bin F.txt    a synthetic evaluation.  F.txt: coder (0 static, 1 fast), EV, cand, jobs; per job: family, events, rows,
//                               then `row count` per non-empty row.  E.bin: the jobs' 16-bit events back to back (X | sub-block << 8 |
//                               bit << 11; bit 12 set where a chain starts that the signature does not show).  Row starts are marked here.
// block / events -> one JSON object: `off` and `on` (resolve) each with open / resolved / replays / fail_replay / starts_equal (every
// start value dc_eval_b_kernel's restatement hands out equals the serial walk's), and stretches / longest / max_width / wide.
#include "../libbsc_amd/csrc/host/qlfc.cpp"
#include "../libbsc_amd/csrc/device/devcoder_model.h"
#include <algorithm>
#include <cstdio>
#include <numeric>
#include <string>
#include <vector>

using namespace bschost;
namespace bschost { void* bigbuf_get(size_t bytes) { return malloc(bytes); } void bigbuf_put(void* p) { free(p); } }

struct Job { std::vector<uint16_t> events; std::vector<uint32_t> rowstart; int fam; };

static void mark_rows(Job& J)
{
    for (int r = 0; r < dcm::DC_ROWS; ++r) if (J.rowstart[r + 1] > J.rowstart[r]) J.events[J.rowstart[r]] |= (uint16_t)dcm::DC_ROWMARK;
}

// the value in front of every chunk's first event by the plain serial walk: one pass over the job, a chain starts at a marked event or
// where the signature changes
static void serial_starts(const Job& J, uint32_t EV, const dcm::ModelParams& M, std::vector<uint16_t>& out)
{
    const uint32_t E = (uint32_t)J.events.size();
    out.assign((E + EV - 1) / EV, 0);
    uint32_t row = 0, prev = 0xffffu;
    int v = 0;
    for (uint32_t k = 0; k < E; ++k) {
        while (J.rowstart[row + 1] <= k) ++row;
        const int cls = dcm::tau_class((int)row);
        const uint32_t e = J.events[k];
        if ((e & (dcm::DC_SIGMASK | dcm::DC_ROWMARK)) != prev) v = M.init[cls];
        prev = e & dcm::DC_SIGMASK;
        if (k % EV == 0) out[k / EV] = (uint16_t)v;
        v = dcm::step(v, (e >> 11) & 1u, M.rates[cls][J.fam]);
    }
}

static void print_side(const char* name, const dcm::ReplayResolve& R, bool equal)
{
    printf(" \"%s\": {\"open\": %u, \"resolved\": %u, \"replays\": %u, \"fail_replay\": %s, \"wide\": %u, \"starts_equal\": %s}", name, R.open, R.resolved, R.replays,
           R.fail_replay ? "true" : "false", R.wide, equal ? "true" : "false");
}

static int report(std::vector<Job>& jobs, uint32_t EV, const dcm::ModelParams& M, uint32_t cand, const char* extra)
{
    jobs.resize(4);
    for (Job& J : jobs) { if (J.rowstart.empty()) J.rowstart.assign(dcm::DC_ROWS + 1, 0); mark_rows(J); }
    dcm::ReplayJob rj[4];
    for (int q = 0; q < 4; ++q) rj[q] = dcm::ReplayJob{jobs[q].events.data(), (uint32_t)jobs[q].events.size(), jobs[q].rowstart.data(), jobs[q].fam};
    dcm::ReplayResolve off, on;
    dcm::replay_resolve_host(rj, EV, M, cand, false, off);
    dcm::replay_resolve_host(rj, EV, M, cand, true, on);
    bool eq_off = true, eq_on = true;
    uint32_t chunks = 0;
    for (int q = 0; q < 4; ++q) {
        std::vector<uint16_t> truth;
        serial_starts(jobs[q], EV, M, truth);
        chunks += (uint32_t)truth.size();
        for (size_t c = 0; c < truth.size(); ++c) {
            const size_t s = off.cstart[q] + c;
            if (off.known[s] ? off.start[s] != truth[c] : !off.fail_replay) eq_off = false;
            if (on.known[s] ? on.start[s] != truth[c] : !on.fail_replay) eq_on = false;
        }
    }
    printf("{\"ev\": %u, \"chunks\": %u, \"cand\": %u, \"DC_RP_CAND\": %d, \"DC_REPLAY_MAX\": %d,%s\n \"stretches\": %u, \"longest\": %u, \"max_width\": %u,\n", EV, chunks,
           cand, dcm::DC_RP_CAND, dcm::DC_REPLAY_MAX, extra, on.stretches, on.longest, on.max_width);
    print_side("off", off, eq_off); printf(",\n"); print_side("on", on, eq_on); printf("}\n");
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

// ---- bound ------------------------------------------------------------------------------------------------------------------------
struct Bound { bool ok = true; int slowest = 4096; uint32_t width = 0, periodic = 0; uint32_t w_cf[dcm::NUM_CLS][3], p_cf[dcm::NUM_CLS][3]; };
static Bound bound_of(const dcm::ModelParams& M, bool one_family)
{
    Bound B;
    for (int c = 0; c < dcm::NUM_CLS; ++c) for (int f = 0; f < 3; ++f) {
        B.w_cf[c][f] = B.p_cf[c][f] = 0;
        if (one_family && f != dcm::FAM_CHAR) continue;
        const dcm::Rates& R = M.rates[c][f];
        const int lo = M.vmin[c][f], hi = M.vmax[c][f];
        // (a) the contraction, every pair and both bits
        for (uint32_t bit = 0; bit < 2; ++bit) {
            const int a = bit ? R.a1 : R.a0;
            std::vector<int> img((size_t)(hi - lo + 1));
            for (int v = lo; v <= hi; ++v) img[(size_t)(v - lo)] = dcm::step(v, bit, R);
            for (int v = lo; v <= hi; ++v) for (int u = v + 1; u <= hi; ++u) {
                const int d = u - v, d2 = img[(size_t)(u - lo)] - img[(size_t)(v - lo)];
                if (d2 < 0 || d2 > d - (d * a) / 4096) B.ok = false;
            }
        }
        // (b) the recursion with the slower of the two rates
        const int a = R.a0 < R.a1 ? R.a0 : R.a1;
        if (hi > lo && a < B.slowest) B.slowest = a;                      // (a counter that never moves — rate 0, one attainable value — has no bracket)
        int d = hi - lo;
        for (int t = 0; t < dcm::DC_EV; ++t) d -= (d * a) / 4096;
        B.w_cf[c][f] = (uint32_t)d + 1u;
        if (B.w_cf[c][f] > B.width) B.width = B.w_cf[c][f];
        // (c) periodic patterns
        for (int period = 1; period <= 8; ++period) for (uint32_t pat = 0; pat < (1u << period); ++pat) {
            int x = lo, y = hi;
            for (int t = 0; t < dcm::DC_EV && x != y; ++t) { const uint32_t b = (pat >> (t % period)) & 1u; x = dcm::step(x, b, R); y = dcm::step(y, b, R); }
            if ((uint32_t)(y - x) + 1u > B.p_cf[c][f]) B.p_cf[c][f] = (uint32_t)(y - x) + 1u;
        }
        if (B.p_cf[c][f] > B.periodic) B.periodic = B.p_cf[c][f];
    }
    return B;
}
static void print_bound(const char* name, const Bound& B)
{
    printf(" \"%s\": {\"contraction_holds\": %s, \"slowest_rate\": %d, \"bound_width\": %u, \"periodic_width\": %u, \"periodic_by_class\": [", name, B.ok ? "true" : "false",
           B.slowest, B.width, B.periodic);
    for (int c = 0; c < dcm::NUM_CLS; ++c) printf("%s[%u, %u, %u]", c ? ", " : "", B.p_cf[c][0], B.p_cf[c][1], B.p_cf[c][2]);
    printf("], \"bound_by_class\": [");
    for (int c = 0; c < dcm::NUM_CLS; ++c) printf("%s[%u, %u, %u]", c ? ", " : "", B.w_cf[c][0], B.w_cf[c][1], B.w_cf[c][2]);
    printf("]}");
}

int main(int argc, char** argv)
{
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "bound") {
        dcm::ModelParams Ms, Mf;
        dcm::model_params_from_table(kStaticParams, Ms); dcm::model_params_fast(Mf);
        const Bound S = bound_of(Ms, false), F = bound_of(Mf, true);
        const uint32_t widest = S.width > F.width ? S.width : F.width;
        printf("{\"DC_EV\": %d, \"DC_RP_CAND\": %d, \"cap\": %u,\n", dcm::DC_EV, dcm::DC_RP_CAND, (widest + 63u) / 64u * 64u);
        print_bound("static", S); printf(",\n"); print_bound("fast", F); printf("}\n");
        return 0;
    }
    if (mode == "events" && argc == 4) {
        std::vector<uint8_t> raw;
        if (!read_file(argv[2], raw)) return 2;
        FILE* f = fopen(argv[3], "r");
        if (!f) { perror(argv[3]); return 2; }
        unsigned coder = 0, EV = 0, cand = 0, njobs = 0;
        if (fscanf(f, "%u %u %u %u", &coder, &EV, &cand, &njobs) != 4 || njobs < 1 || njobs > 4 || EV == 0 || EV % dcm::DC_EB) return 2;
        std::vector<Job> jobs(njobs);
        size_t at = 0;
        for (Job& J : jobs) {
            unsigned E = 0, rows = 0;
            if (fscanf(f, "%d %u %u", &J.fam, &E, &rows) != 3 || J.fam < 0 || J.fam > 2 || at + 2 * (size_t)E > raw.size()) return 2;
            J.events.resize(E);
            memcpy(J.events.data(), raw.data() + at, 2 * (size_t)E); at += 2 * (size_t)E;
            std::vector<uint32_t> cnt(dcm::DC_ROWS, 0);
            for (unsigned r = 0; r < rows; ++r) { unsigned row = 0, n = 0; if (fscanf(f, "%u %u", &row, &n) != 2 || row >= (unsigned)dcm::NUM_TAU) return 2; cnt[row] += n; }
            J.rowstart.assign(dcm::DC_ROWS + 1, 0);
            for (int r = 0; r < dcm::DC_ROWS; ++r) J.rowstart[r + 1] = J.rowstart[r] + cnt[r];
            if (J.rowstart[dcm::DC_ROWS] != E) return 2;
        }
        fclose(f);
        dcm::ModelParams M;
        if (coder) dcm::model_params_fast(M); else dcm::model_params_from_table(kStaticParams, M);
        return report(jobs, EV, M, cand, "");
    }
    if (mode == "block" && (argc == 3 || argc == 4)) {
        std::vector<uint8_t> L;
        if (!read_file(argv[2], L)) return 2;
        const uint32_t cand = argc == 4 ? (uint32_t)atoi(argv[3]) : (uint32_t)dcm::DC_RP_CAND;
        const int nb = coder_num_blocks((int)L.size());
        int start[8], size[8];
        coder_split_blocks(L.data(), (int)L.size(), nb, start, size);
        const QlfcTables& T = qlfc_tables();
        dcm::ModelParams M; dcm::model_params_from_table(kStaticParams, M);
        // the runs of the block in stream order with their contexts (as tools/devcoder_sim.cpp has them)
        struct Run { dcm::Item it; int maxr; uint8_t X[4]; };               // X per job: nothing, symbol, rank state, run state
        std::vector<Run> runs;
        for (int sb = 0; sb < nb; ++sb) {
            QlfcRuns Q; qlfc_runs(L.data() + start[sb], size[sb], Q);
            const int max_rank = encode_alphabet(Q.view, [](unsigned) {});
            uint32_t ctx_rank0 = 0, ctx_rank4 = 0, ctx_run = 0, avg = 0;
            uint8_t rank_hist[256] = {0}, run_hist[256] = {0};
            for (uint32_t j = 0; j < Q.view.count; ++j) {
                const uint32_t c = Q.view.sym[j], rank = Q.view.rank[j], run = Q.view.len(j);
                Run r; r.it = dcm::Item{rank, run, (uint32_t)sb, avg >= 32 ? 1u : 0u}; r.maxr = max_rank;
                r.X[0] = 0; r.X[1] = (uint8_t)c;
                r.X[2] = T.rank_state[dcm::rank_state_index(ctx_run, ctx_rank4, rank_hist[c])];
                r.X[3] = T.run_state[dcm::run_state_index(ctx_rank0, ctx_run, rank, run_hist[c])];
                runs.push_back(r);
                rank_hist[c] = (uint8_t)dcm::bsr(rank);
                avg = dcm::avg_rank_next(avg, rank);
                run_hist[c] = (uint8_t)dcm::run_hist_next(run_hist[c], run);
                ctx_rank0 = ((ctx_rank0 << 1) | (rank == 1 ? 1u : 0u)) & 7u;
                ctx_rank4 = ((ctx_rank4 << 2) | (rank - 1 < 3 ? rank - 1 : 3u)) & 0xffu;
                ctx_run = ((ctx_run << 1) | (run < 3 ? 1u : 0u)) & 0xfu;
            }
        }
        // the four jobs: static (stream order, X ignored, both sides), char (symbol-major, both sides), state (rank side by rank
        // state, run side by run state); a stable sort by X, as the one radix pass over the top byte of the items
        static const int fam_of[4] = {dcm::FAM_STATIC, dcm::FAM_CHAR, dcm::FAM_STATE, dcm::FAM_STATE};
        static const int sides_of[4] = {3, 3, 1, 2};
        std::vector<Job> jobs(4);
        uint64_t Etot = 0;
        for (int q = 0; q < 4; ++q) {
            std::vector<uint32_t> order(runs.size());
            std::iota(order.begin(), order.end(), 0u);
            if (q) std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return runs[a].X[q] < runs[b].X[q]; });
            std::vector<std::vector<uint16_t>> row((size_t)dcm::DC_ROWS);
            for (uint32_t i : order) {
                const Run& r = runs[i];
                const uint32_t sig = (uint32_t)r.X[q] | (r.it.sb << 8);
                dcm::enumerate(r.it, r.maxr, [&](int tau, uint32_t bit, bool run_side) {
                    if (sides_of[q] & (run_side ? 2 : 1)) row[(size_t)tau].push_back((uint16_t)(sig | (bit << 11)));
                });
            }
            Job& J = jobs[q];
            J.fam = fam_of[q];
            J.rowstart.assign(dcm::DC_ROWS + 1, 0);
            for (int r = 0; r < dcm::DC_ROWS; ++r) { J.rowstart[r + 1] = J.rowstart[r] + (uint32_t)row[(size_t)r].size(); J.events.insert(J.events.end(), row[(size_t)r].begin(), row[(size_t)r].end()); }
            Etot += J.events.size();
        }
        char extra[128];
        snprintf(extra, sizeof extra, " \"n\": %zu, \"nb\": %d, \"runs\": %zu, \"decisions\": %zu,", L.size(), nb, runs.size(), jobs[0].events.size());
        return report(jobs, dcm::eval_chunk_events(Etot), M, cand, extra);
    }
    fprintf(stderr, "usage: %s bound | block L.bin [cand] | events E.bin F.txt\n", argv[0]);
    return 2;
}
