// dc_segment_probe.cpp — drives the schedule of a pass in model segments (libbsc_amd/csrc/device/dc_segment_plan.h: DcSegSchedule) the
// way devcoder_pstream_segments does, with a rule in place of the model; tests/test_dc_segment_plan_host.py compares what it prints
// with pipeline_model.segment_schedule and with a hand-written table of the edges.  No GPU, no HIP:
//   g++ -std=c++17 -I libbsc_amd/csrc/device tools/dc_segment_probe.cpp -o dc_segment_probe
// One scenario per line on stdin, numbers separated by blanks:
//   count nsub dcap target cap per_segment_fit packed  blk_sub[count + 1]  dec[nsub]  und[nsub]
//   ndecline (block why)*  nvoid block*  nskew block*  [mix_cap mix[nsub]]
// The optional trailing fields are the adaptive coder's third fact: the longest mixer chain of every sub-block and the step cap; a line
// without them means no such rule.
// The rule: a range declines iff it holds a block of the decline list, with the OR of their reasons (a chain's trouble does not go away
// by adding neighbours); else it is kept with D, pseg and pbseg as dec[] gives them — the 2-byte form after all (void) iff packed and it
// holds a block of the void list, and a packed layout 64 fields longer than the plan's iff it holds one of the skew list.
// One JSON object per line on stdout: the ranges in order with their outcome ("nofit": given up before it ran, "split", "gave_up",
// "kept", "void", "layout": the error that ends the pass), then what the pass left behind.
#include "dc_segment_plan.h"
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

enum { FAIL_AVG = 2, FAIL_CAP = 8, FAIL_MIX = 32 };                   // include/bscgpu.h: BSCGPU_DC_FAIL_*

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
static bool read_ints(std::vector<long long>& v, int n)
{
    if (n < 0 || line_at + (size_t)n > line.size()) return false;
    v.assign(line.begin() + (long)line_at, line.begin() + (long)(line_at + (size_t)n));
    line_at += (size_t)n;
    return true;
}
static bool read_int(int* v) { std::vector<long long> t; if (!read_ints(t, 1)) return false; *v = (int)t[0]; return true; }

template <class T> static void print_list(const char* name, const std::vector<T>& v)
{
    printf(",\"%s\":[", name);
    for (size_t i = 0; i < v.size(); ++i) printf("%s%lld", i ? "," : "", (long long)v[i]);
    printf("]");
}

int main()
{
    while (next_line()) {
        if (line.empty()) continue;
        std::vector<long long> t;
        if (!read_ints(t, 7)) return 1;
        const int count = (int)t[0], nsub = (int)t[1], fit = (int)t[5], packed = (int)t[6];
        const long long dcap = t[2], target = t[3], cap = t[4];
        if (!read_ints(t, count + 1)) return 1;
        const std::vector<int> blk_sub(t.begin(), t.end());
        if (!read_ints(t, nsub)) return 1;
        const std::vector<uint32_t> dec(t.begin(), t.end());
        if (!read_ints(t, nsub)) return 1;
        const std::vector<uint32_t> und(t.begin(), t.end());
        std::vector<int> why_of((size_t)count, 0), is_void((size_t)count, 0), is_skew((size_t)count, 0);
        int k;
        if (!read_int(&k) || !read_ints(t, 2 * k)) return 1;
        for (int i = 0; i < k; ++i) why_of[(size_t)t[2 * i]] = (int)t[2 * i + 1];
        if (!read_int(&k) || !read_ints(t, k)) return 1;
        for (int i = 0; i < k; ++i) is_void[(size_t)t[i]] = 1;
        if (!read_int(&k) || !read_ints(t, k)) return 1;
        for (int i = 0; i < k; ++i) is_skew[(size_t)t[i]] = 1;
        const bool with_mix = line_at < line.size();
        long long mix_cap = 0;
        std::vector<uint32_t> mix;
        if (with_mix) {
            if (!read_ints(t, 1)) return 1;
            mix_cap = t[0];
            if (!read_ints(t, nsub) || line_at != line.size()) return 1;
            mix.assign(t.begin(), t.end());
        }

        std::vector<uint32_t> poff((size_t)nsub + 1, 0xffffffffu), pseg((size_t)nsub + 1), pbseg((size_t)nsub + 1);
        std::vector<int64_t> pbase(packed ? (size_t)nsub + 1 : 0, -1);
        std::vector<int> blk_state((size_t)count, -1);
        DcSegSchedule sch(dec.data(), und.data(), blk_sub.data(), count, nsub, dcap, target, cap, fit != 0, FAIL_AVG, FAIL_CAP, poff.data(),
                          packed ? pbase.data() : nullptr, blk_state.data(), with_mix ? mix.data() : nullptr, mix_cap, FAIL_MIX);
        printf("{\"need\":%lld,\"copy_all\":%s", (long long)sch.planned_need(), sch.copy_all() ? "true" : "false");
        print_list("excluded", blk_state);
        printf(",\"ranges\":[");
        bool error = false;
        DcSegRange g;
        const char* sep = "";
        for (DcSegNext nx; !error && (nx = sch.next(&g)) != DC_SEG_DONE; sep = ",") {
            printf("%s[%d,%d,%d,%d,%lld,%lld,", sep, g.b0, g.b1, g.s0, g.s1, (long long)g.expect, (long long)g.need);
            if (nx == DC_SEG_GIVEN_UP) { printf("\"nofit\",%d]", FAIL_CAP); continue; }
            int why = 0, vd = 0, skew = 0;
            for (int b = g.b0; b < g.b1; ++b) { why |= why_of[(size_t)b]; vd |= is_void[(size_t)b]; skew |= is_skew[(size_t)b]; }
            if (why) { printf("\"%s\",%d]", sch.declined(g, why) ? "gave_up" : "split", why); continue; }
            pseg[0] = pbseg[0] = 0;
            for (int s = g.s0; s < g.s1; ++s) {
                pseg[(size_t)(s - g.s0) + 1] = pseg[(size_t)(s - g.s0)] + dec[(size_t)s];
                pbseg[(size_t)(s - g.s0) + 1] = pbseg[(size_t)(s - g.s0)] + (uint32_t)dc_pack13_fields(dec[(size_t)s]);
            }
            const bool pk = packed && !vd;
            if (pk && skew) pbseg[(size_t)(g.s1 - g.s0)] += 64;
            const int64_t at = sch.kept(g, pseg[(size_t)(g.s1 - g.s0)], pseg.data(), pk ? pbseg.data() : nullptr, pk);
            error = at < 0;
            printf("\"%s\",%lld]", error ? "layout" : packed && !pk ? "void" : "kept", (long long)at);
        }
        printf("],\"error\":%s", error ? "true" : "false");
        if (!error) {
            const DcSegTotals T = sch.finish();
            print_list("blk_state", blk_state);
            print_list("poff", poff);
            if (packed) print_list("pbase", pbase);
            printf(",\"planned\":%d,\"kept\":%d,\"reruns\":%d,\"host_blocks\":%d,\"packed\":%d,\"void\":%d,\"fail\":%d,\"decisions\":%lld", T.planned, T.kept,
                   T.reruns, T.host_blocks, T.kept_packed, T.kept_void, T.fail, (long long)T.decisions);
        }
        printf("}\n");
    }
    return 0;
}
