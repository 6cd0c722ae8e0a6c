// batch_pass_probe.cpp — walks a batched-compress call through the rules of libbsc_amd/csrc/host/batch_pass_plan.h the way
// compress_batch_impl (block.cpp) does, with the device's answers read from its input; tests/test_batch_pass_plan_host.py compares what
// it prints with pipeline_model.batch_call and with a hand-written table of the edges.  No GPU, no HIP:
//   g++ -std=c++17 -I libbsc_amd/csrc/host tools/batch_pass_probe.cpp -o batch_pass_probe
// One call per line on stdin, numbers separated by blanks:
//   count sorter coder cap dev  front model fast segments packed device_rc (the option values)
//   min_pass_static min_pass_fast target front_host model_host entries  sizes[count]  lz[count]
//   nfacts (pass nsub mrc D pk pbytes nstate blk_state[nstate])*  [adaptive_segments [model_adaptive]]
// A pass without facts has nsub = 0; a pass whose facts have no blk_state has all zeros.  The optional trailing fields are the values of
// BSCGPU_OPT_BATCH_ADAPTIVE_SEGMENTS and BSCGPU_OPT_BATCH_MODEL_ADAPTIVE; a line without them means 0, and only a line with them
// gets the adaptive route's keys ("adaptive_model" of the call, "adaptive": [passes, declined] of a pass) in its answer.
// One JSON object per line on stdout.
#include "batch_pass_plan.h"
#include <cstdio>
#include <cstdlib>
#include <map>
#include <string>
#include <vector>

struct Facts { int nsub = 0, mrc = 0; long long D = 0; int pk = 0; long long pbytes = 0; std::vector<int> state; };

// the numbers of the current line, taken in order
static std::vector<long long> line;
static size_t line_at;
static bool next_line()
{
    std::string text;
    int ch;
    while ((ch = getchar()) != EOF && ch != '\n') text.push_back((char)ch);
    if (ch == EOF && text.empty()) return false;
    line.clear(); line_at = 0;
    const char* p = text.c_str();
    for (char* end; ; p = end) { const long long v = strtoll(p, &end, 10); if (end == p) break; line.push_back(v); }
    return true;
}
static bool read_ints(std::vector<long long>& v, long long n)
{
    if (n < 0 || line_at + (size_t)n > line.size()) return false;
    v.assign(line.begin() + (long)line_at, line.begin() + (long)(line_at + (size_t)n));
    line_at += (size_t)n;
    return true;
}

template <class T> static void print_list(const char* name, const std::vector<T>& v)
{
    printf("\"%s\":[", name);
    for (size_t i = 0; i < v.size(); ++i) printf("%s%lld", i ? "," : "", (long long)v[i]);
    printf("]");
}
static void print_names(const char* name, const std::vector<const char*>& v)
{
    printf("\"%s\":[", name);
    for (size_t i = 0; i < v.size(); ++i) printf("%s\"%s\"", i ? "," : "", v[i]);
    printf("]");
}

int main()
{
    static const char* const CLASS[] = {"empty", "stored", "rides", "single", "sorted"};
    static const char* const STEP[] = {"none", "whole", "segments"};
    static const char* const SOURCE[] = {"l", "runs", "ps16", "ps13", "fast", "device_rc"};
    static const char* const LEFT[] = {"none", "one_by_one", "pipe"};
    while (next_line()) {
        if (line.empty()) continue;
        std::vector<long long> t;
        if (!read_ints(t, 17)) return 1;
        const int count = (int)t[0], sorter = (int)t[1], coder = (int)t[2], dev = (int)t[4], front_host = (int)t[14], model_host = (int)t[15];
        const long long cap = t[3], min_static = t[11], min_fast = t[12], target = t[13], entries = t[16];
        BatchOptions o = {};
        o.front = (int)t[5]; o.model = (int)t[6]; o.model_fast = (int)t[7]; o.segments = (int)t[8]; o.packed = (int)t[9]; o.device_rc = (int)t[10];
        if (!read_ints(t, count)) return 1;
        const std::vector<int> sizes(t.begin(), t.end());
        if (!read_ints(t, count)) return 1;
        const std::vector<int> lz(t.begin(), t.end());
        std::map<int, Facts> facts;
        if (!read_ints(t, 1)) return 1;
        const int nf = (int)t[0];
        for (int k = 0; k < nf; ++k) {
            Facts f;
            if (!read_ints(t, 7)) return 1;
            const int p = (int)t[0], ns = (int)t[6];
            f.nsub = (int)t[1]; f.mrc = (int)t[2]; f.D = t[3]; f.pk = (int)t[4]; f.pbytes = t[5];
            if (!read_ints(t, ns)) return 1;
            f.state.assign(t.begin(), t.end());
            facts[p] = f;
        }
        const bool with_adaptive = line_at < line.size();
        if (with_adaptive) {
            if (!read_ints(t, 1)) return 1;
            o.adaptive_segments = (int)t[0];
            if (line_at < line.size()) { if (!read_ints(t, 1)) return 1; o.model_adaptive = (int)t[0]; }
            if (line_at != line.size()) return 1;
        }

        const bool st = sorter != LIBBSC_BLOCKSORTER_BWT;
        std::vector<int> pass_of((size_t)count);
        const int npass = st ? batch_pass_plan_st(sizes.data(), count, cap, pass_of.data()) : batch_pass_plan_bwt(sizes.data(), count, sorter, cap, pass_of.data());
        const BatchRoute R = batch_route(npass, o, coder, batch_wants_front(npass, o) && front_host != 0, min_static, min_fast, target);
        printf("{\"npass\":%d,", npass);
        print_list("pass_of", pass_of);
        printf(",\"route\":[%d,%d,%d,%d,%d,%d],\"min_pass\":%lld,\"target\":%lld,", R.front, R.model, R.fast_model, R.segments, R.packed, R.device_rc,
               (long long)R.min_pass, (long long)R.segment_target);
        if (with_adaptive) printf("\"adaptive_model\":%d,", R.adaptive_model);
        printf("\"passes\":[");
        std::vector<char> single((size_t)count);
        for (int b = 0; b < count; ++b) single[(size_t)b] = pass_of[(size_t)b] < 0;
        int error = 0;
        for (int b = 0, p = 0; b < count && !error;) {
            if (pass_of[(size_t)b] < 0) { ++b; continue; }
            const int e = batch_pass_end(pass_of.data(), sizes.data(), count, b), cnt = e - b;
            std::vector<BatchClass> cls((size_t)cnt);
            std::vector<const char*> names((size_t)cnt);
            for (int i = 0; i < cnt; ++i) {
                cls[(size_t)i] = batch_block_class(sizes[(size_t)(b + i)], lz[(size_t)(b + i)], st, dev != 0, pass_of[(size_t)(b + i)] >= 0);
                names[(size_t)i] = CLASS[cls[(size_t)i]];
            }
            BatchGeometry G;
            batch_pass_geometry(cls.data(), sizes.data() + b, lz.data() + b, cnt, st, dev != 0, &G);
            Facts f = facts.count(p) ? facts[p] : Facts();
            f.state.resize((size_t)cnt, 0);
            BatchCounters d = {};
            BatchModelStep step = BATCH_MODEL_NONE;
            BatchVerdict v = BATCH_PASS_HOST;
            const bool layout = G.pos > 0 && R.front;
            if (G.pos > 0 && !R.front) ++d.l_passes;
            if (layout) {
                ++d.front_passes;
                step = batch_model_step(R, f.nsub, G.pos, true);
                if (step != BATCH_MODEL_NONE && !model_host) step = batch_model_step(R, f.nsub, G.pos, false);
                std::vector<int> blk_sub((size_t)cnt + 1, 0);          // a sub-block for every entry with bytes in it
                for (int i = 0; i < cnt; ++i) blk_sub[(size_t)i + 1] = blk_sub[(size_t)i] + (G.psz[(size_t)i] > 0);
                const int pk = R.packed ? f.pk : 0;
                if (step == BATCH_MODEL_WHOLE) v = batch_whole_verdict(f.mrc, (uint32_t)f.D, pk, f.pbytes, (size_t)entries);
                if (step == BATCH_MODEL_SEGMENTS) v = batch_segments_verdict(f.mrc, blk_sub.data(), f.state.data(), cnt);
                if (step != BATCH_MODEL_NONE) {
                    const BatchCounters m = batch_model_counters(R, step, v, pk);
                    d.model_passes = m.model_passes; d.model_declined = m.model_declined; d.fast_passes = m.fast_passes; d.fast_declined = m.fast_declined;
                    d.packed_passes = m.packed_passes; d.packed_void = m.packed_void; d.device_rc = m.device_rc;
                    d.adaptive_passes = m.adaptive_passes; d.adaptive_declined = m.adaptive_declined;
                }
                if (v == BATCH_PASS_ERROR) error = f.mrc;
            }
            const bool kept = v == BATCH_PASS_KEPT;
            printf("%s{\"b\":%d,\"e\":%d,", p ? "," : "", b, e);
            print_names("classes", names); printf(",");
            print_list("psz", G.psz); printf(",");
            print_list("prate", G.prate); printf(",");
            print_list("at", G.at);
            printf(",\"pos\":%lld,\"step\":\"%s\",\"kept\":%d,\"counters\":{\"front\":%d,\"l\":%d,\"model\":%d,\"declined\":%d,\"fast\":%d,\"fast_declined\":%d,"
                   "\"packed\":%d,\"void\":%d,\"device_rc\":%d}", (long long)G.pos, G.pos > 0 && !R.front ? "l_down" : STEP[step], kept, d.front_passes, d.l_passes,
                   d.model_passes, d.model_declined, d.fast_passes, d.fast_declined, d.packed_passes, d.packed_void, d.device_rc);
            if (with_adaptive) printf(",\"adaptive\":[%d,%d]", d.adaptive_passes, d.adaptive_declined);
            if (!error) {
                const bool coded = step == BATCH_MODEL_WHOLE && kept && R.device_rc;
                const bool stream = step == BATCH_MODEL_SEGMENTS || (step == BATCH_MODEL_WHOLE && kept && !coded);
                const bool packed = step == BATCH_MODEL_SEGMENTS ? R.packed : kept && R.packed && f.pk;
                for (int i = 0; i < cnt; ++i) {
                    names[(size_t)i] = cls[(size_t)i] != BATCH_SORTED ? "" :
                        SOURCE[batch_block_source(layout, stream, coded, step == BATCH_MODEL_SEGMENTS && f.state[(size_t)i] != 0, R.fast_model, packed)];
                    if (cls[(size_t)i] == BATCH_SINGLE) single[(size_t)(b + i)] = 1;
                }
                printf(","); print_names("sources", names);
            }
            printf("}");
            b = e; ++p;
        }
        std::vector<const char*> left;
        for (int b = 0; b < count && !error; ++b) left.push_back(LEFT[batch_leftover(single[(size_t)b] != 0, pass_of[(size_t)b] >= 0, sizes[(size_t)b], cap, dev != 0)]);
        printf("],\"error\":%d,", error);
        print_names("leftover", left);
        printf("}\n");
    }
    return 0;
}
