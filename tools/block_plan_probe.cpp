// block_plan_probe.cpp — drives the plan of a single block in sub-block segments (libbsc_amd/csrc/device/dc_block_plan.h:
// dc_block_segment_plan, DcBlockSchedule) from stdin; tests/test_block_segment_plan_host.py compares what it prints with a Python
// restatement, with brute force over all cut sets and with the packed layout of bscgpu_pstream_pack13_host.  No GPU, no HIP:
//   g++ -std=c++17 -I libbsc_amd/csrc/device tools/block_plan_probe.cpp -o block_plan_probe
// (the test also builds it with -fsanitize=address,undefined and runs that program on the same input).
// One scenario per line on stdin, numbers separated by blanks:
//   nsub count mcap dcap packed nullmask void_seg  runs[count]  dec[count]
// nsub goes to the plan as it is (0 and 9 are the bad-argument cases; count says how many numbers follow); nullmask: bit 0 sub_runs,
// bit 1 sub_dec, bit 2 seg_of is passed as a null pointer; void_seg: the segment whose packed form is taken as void (-1: none).
// One JSON object per line on stdout: rc and seg_of[0..8) as the plan left it (prefilled with -7: nothing is written on an error); for
// rc > 0 the schedule — poff, pbase, the zone's bytes, every segment — and "join": the segments' streams, each laid out on its own the
// way the device lays out a block of those sub-blocks, copied piece by piece (or packed into place: void_seg) into one zone, give the
// whole block's stream where it holds decisions.
// A line that begins with a word asks something else of the header:
//   whole nsub packed dec[nsub]      DcBlockSchedule::whole of the poff these counts sum to: the same keys, one segment
//   maxrank nb nsym[nb]              dc_max_rank of 1..256, and dc_max_rank_table of a first-run table with nsym[b] symbols in sub-block b
//   tries allowed enabled coder_static coder_fast nsub n min_n | dense m n | verdict code sent device_rc zone
//                                    what the driver of one block decides
#include "dc_block_plan.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

template <class T> static void print_list(const char* name, const T* v, int n)
{
    printf(",\"%s\":[", name);
    for (int i = 0; i < n; ++i) printf("%s%lld", i ? "," : "", (long long)v[i]);
    printf("]");
}

// the stream of sub-blocks [s0, s1) as a unit of its own: 16-bit entries, or packed from its own first field
static std::vector<uint8_t> unit_stream(const std::vector<uint16_t>& e, const std::vector<int64_t>& poff, int s0, int s1, bool packed)
{
    const uint16_t* first = e.data() + poff[(size_t)s0];
    const int64_t D = poff[(size_t)s1] - poff[(size_t)s0];
    if (!packed) { std::vector<uint8_t> out((size_t)D * 2); if (D) memcpy(out.data(), first, out.size()); return out; }
    uint32_t rel[DC_BLOCK_MAX_SUB + 1]; int64_t pb[DC_BLOCK_MAX_SUB + 1];
    for (int s = s0; s <= s1; ++s) rel[s - s0] = (uint32_t)(poff[(size_t)s] - poff[(size_t)s0]);
    int64_t fields = 0;
    for (int s = s0; s < s1; ++s) fields += dc_pack13_fields(rel[s - s0 + 1] - rel[s - s0]);
    std::vector<uint8_t> out((size_t)dc_pack13_bytes(fields), 0xa5);
    if (!out.empty() && dc_pack13_host(first, rel, s1 - s0, out.data(), (int64_t)out.size(), pb) != (int64_t)out.size()) out.clear();
    return out;
}

static void print_segment(const DcBlockSeg& g, bool first)
{
    const int ns = g.s1 - g.s0;
    printf("%s{\"s0\":%d,\"s1\":%d,\"r0\":%u,\"r1\":%u,\"expect\":%lld", first ? "" : ",", g.s0, g.s1, g.r0, g.r1, (long long)g.expect);
    print_list("first", g.first, DC_BLOCK_MAX_SUB + 1);
    print_list("src", g.src, ns); print_list("dst", g.dst, ns); print_list("len", g.len, ns);
    printf("}");
}

// a line that began with a word -> false: not understood
static bool asked(const char* word)
{
    if (!strcmp(word, "whole")) {
        int nsub, packed;
        if (scanf("%d %d", &nsub, &packed) != 2 || nsub < 0 || nsub > 64) return false;
        std::vector<uint32_t> poff((size_t)nsub + 1, 0u);
        for (int s = 0; s < nsub; ++s) { long long v; if (scanf("%lld", &v) != 1) return false; poff[(size_t)s + 1] = poff[(size_t)s] + (uint32_t)v; }
        const DcBlockSchedule sch = DcBlockSchedule::whole(poff.data(), nsub, packed != 0);
        printf("{\"segments\":%d", sch.segments());
        if (sch.segments() > 0) {
            std::vector<int64_t> po, pb;
            for (int s = 0; s <= nsub; ++s) { po.push_back(sch.poff_of(s)); pb.push_back(sch.pbase_of(s)); }
            printf(",\"zone\":%lld,\"decisions\":%lld", (long long)sch.zone_bytes(), (long long)sch.decisions());
            print_list("poff", po.data(), nsub + 1);
            print_list("pbase", pb.data(), nsub + 1);
            printf(",\"segs\":[");
            for (int i = 0; i < sch.segments(); ++i) print_segment(sch.segment(i), i == 0);
            printf("]");
        }
        printf("}\n");
        return true;
    }
    if (!strcmp(word, "maxrank")) {
        int nb;
        if (scanf("%d", &nb) != 1 || nb < 0 || nb > DC_BLOCK_MAX_SUB) return false;
        std::vector<uint32_t> first_run((size_t)DC_BLOCK_MAX_SUB * 256, 0xffffffffu);
        for (int b = 0; b < nb; ++b) {
            int nsym;
            if (scanf("%d", &nsym) != 1 || nsym < 0 || nsym > 256) return false;
            for (int k = 0; k < nsym; ++k) first_run[(size_t)b * 256 + (size_t)((k * 7 + b * 31) & 255)] = (uint32_t)k;       // (k -> 7 k + c is a permutation of 0..255)
        }
        int of_count[256], table[DC_BLOCK_MAX_SUB];
        for (int nsym = 1; nsym <= 256; ++nsym) of_count[nsym - 1] = dc_max_rank(nsym);
        for (int& t : table) t = -7;
        dc_max_rank_table(first_run.data(), nb, table);
        printf("{\"rc\":0");
        print_list("max_rank", of_count, 256);
        print_list("table", table, DC_BLOCK_MAX_SUB);
        printf("}\n");
        return true;
    }
    if (!strcmp(word, "tries")) {
        int allowed, enabled, coder_static, coder_fast, nsub; long long n, min_n;
        if (scanf("%d %d %d %d %d %lld %lld", &allowed, &enabled, &coder_static, &coder_fast, &nsub, &n, &min_n) != 7) return false;
        printf("{\"tries\":%d}\n", dc_block_tries_model(allowed != 0, enabled != 0, coder_static != 0, coder_fast != 0, nsub, n, min_n) ? 1 : 0);
        return true;
    }
    if (!strcmp(word, "dense")) {
        long long m, n;
        if (scanf("%lld %lld", &m, &n) != 2) return false;
        printf("{\"dense\":%d}\n", dc_block_runs_too_dense((uint32_t)m, (int)n) ? 1 : 0);
        return true;
    }
    if (!strcmp(word, "verdict")) {
        int code, sent, device_rc, zone;
        if (scanf("%d %d %d %d", &code, &sent, &device_rc, &zone) != 4) return false;
        printf("{\"verdict\":%d}\n", (int)dc_block_verdict(code, sent != 0, device_rc != 0, zone != 0));
        return true;
    }
    return false;
}

int main()
{
    int nsub, count, packed, nullmask, void_seg;
    long long mcap, dcap;
    char word[24];
    while (scanf("%23s", word) == 1) {
        if (word[0] != '-' && (word[0] < '0' || word[0] > '9')) { if (!asked(word)) return 1; continue; }
        nsub = atoi(word);
        if (scanf("%d %lld %lld %d %d %d", &count, &mcap, &dcap, &packed, &nullmask, &void_seg) != 6) return 1;
        if (count < 0 || count > 64) return 1;
        std::vector<uint32_t> runs((size_t)count), dec((size_t)count);
        for (int pass = 0; pass < 2; ++pass)
            for (int i = 0; i < count; ++i) { long long v; if (scanf("%lld", &v) != 1) return 1; (pass ? dec : runs)[(size_t)i] = (uint32_t)v; }
        int seg_of[DC_BLOCK_MAX_SUB];
        for (int& s : seg_of) s = -7;
        const int rc = dc_block_segment_plan(nullmask & 1 ? nullptr : runs.data(), nullmask & 2 ? nullptr : dec.data(), nsub, mcap, dcap, nullmask & 4 ? nullptr : seg_of);
        printf("{\"rc\":%d", rc);
        print_list("seg_of", seg_of, DC_BLOCK_MAX_SUB);
        if (rc > 0 && count >= nsub) {
            uint32_t run_first[DC_BLOCK_MAX_SUB + 1] = {0};
            for (int s = 0; s < nsub; ++s) run_first[s + 1] = run_first[s] + runs[(size_t)s];
            const DcBlockSchedule sch(run_first, dec.data(), nsub, mcap, dcap, packed != 0);
            std::vector<int64_t> poff, pbase;
            for (int s = 0; s <= nsub; ++s) { poff.push_back(sch.poff_of(s)); pbase.push_back(sch.pbase_of(s)); }
            printf(",\"segments\":%d,\"zone\":%lld", sch.segments(), (long long)sch.zone_bytes());
            print_list("poff", poff.data(), nsub + 1);
            print_list("pbase", pbase.data(), nsub + 1);
            // the block's entries: any 16-bit values will do, different at every index
            std::vector<uint16_t> e((size_t)sch.decisions());
            for (size_t i = 0; i < e.size(); ++i) e[i] = (uint16_t)(i * 40503u + 977u);
            std::vector<uint8_t> zone((size_t)sch.zone_bytes() + 1, 0x5a);
            bool join = sch.segments() == rc;
            printf(",\"segs\":[");
            for (int i = 0; i < sch.segments(); ++i) {
                const DcBlockSeg g = sch.segment(i);
                const int ns = g.s1 - g.s0;
                print_segment(g, i == 0);
                uint32_t rel[DC_BLOCK_MAX_SUB + 1];
                for (int s = g.s0; s <= g.s1; ++s) rel[s - g.s0] = (uint32_t)(poff[(size_t)s] - poff[(size_t)g.s0]);
                join = join && sch.agrees(g, rel);
                if (packed && i == void_seg) {
                    join = join && sch.pack_void(g, e.data() + poff[(size_t)g.s0], zone.data());
                    continue;
                }
                const std::vector<uint8_t> unit = unit_stream(e, poff, g.s0, g.s1, packed != 0);
                for (int k = 0; k < ns; ++k) {
                    if (g.src[k] + g.len[k] > (int64_t)unit.size() || g.dst[k] + g.len[k] > sch.zone_bytes()) { join = false; continue; }
                    if (g.len[k]) memcpy(zone.data() + g.dst[k], unit.data() + g.src[k], (size_t)g.len[k]);
                }
            }
            printf("]");
            // against the whole block laid out at once, over the bytes that hold decisions; the byte behind the zone is nobody's
            const std::vector<uint8_t> whole = unit_stream(e, poff, 0, nsub, packed != 0);
            join = join && (int64_t)whole.size() == sch.zone_bytes() && zone.back() == 0x5a;
            for (int s = 0; s < nsub && join; ++s) {
                const int64_t at = packed ? dc_pack13_bytes(pbase[(size_t)s]) : 2 * poff[(size_t)s];
                const int64_t len = packed ? ((int64_t)dec[(size_t)s] + 7) / 8 * 13 : 2 * (int64_t)dec[(size_t)s];
                join = len == 0 || memcmp(zone.data() + at, whole.data() + at, (size_t)len) == 0;
            }
            printf(",\"join\":%s", join ? "true" : "false");
        }
        printf("}\n");
    }
    return 0;
}
