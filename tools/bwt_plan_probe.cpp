// bwt_plan_probe.cpp — prints what the BWT driver's plan (libbsc_amd/csrc/device/bwt_plan.h) decides; tests/test_bwt_plan_host.py
// compares it with pipeline_model.key_geometry and with a hand-written table of round kinds.  No GPU, no HIP:
//   g++ -std=c++17 -I libbsc_amd/csrc/device tools/bwt_plan_probe.cpp -o bwt_plan_probe
// One query per line on stdin, one JSON value per line on stdout:
//   key K n batch_count wmax single_read                                             -> the key plan
//   round isa_valid U n_long n_long_rec n_mid n_mid_rec hybrid hybrid_pct lg_max     -> the round kind
//   pays U U2 text_rounds                                                            -> is the next round one on text keys too
#include "bwt_plan.h"
#include <cstdio>
#include <cstring>

int main()
{
    static const char* const kinds[] = {"text", "text_split", "hand_over", "segsort", "hybrid", "radix"};
    char cmd[16];
    while (scanf("%15s", cmd) == 1) {
        if (!strcmp(cmd, "key")) {
            unsigned K, n, count; int wmax, sr;
            if (scanf("%u %u %u %d %d", &K, &n, &count, &wmax, &sr) != 5) return 1;
            const BwtKeyPlan p = bwt_key_plan(K, n, count, wmax, sr != 0);
            printf("{\"cb\":%u,\"w\":%u,\"tc\":%u,\"low_shift\":%u,\"pred_shift\":%u,\"batch_bb\":%u,\"ta\":%u,\"smask\":%u,\"tail_lo\":%u,"
                   "\"fold_r\":%u,\"fold_np\":%d,\"fold\":%s,\"passes\":[", p.cb, p.w, p.tc, p.low_shift, p.pred_shift, p.batch_bb, p.ta,
                   p.smask, p.tail_lo, p.fold_r, p.fold_np, p.fold ? "true" : "false");
            for (int i = 0; i < p.npass; ++i) printf("%s[%d,%d]", i ? "," : "", p.passes[i].shift, p.passes[i].bits);
            printf("]}\n");
        } else if (!strcmp(cmd, "round")) {
            int isa_valid; BwtRoundCounts g; BwtSwitches sw = {0, 1, 1, 100, 1}; unsigned lg_max;
            if (scanf("%d %u %u %u %u %u %d %d %u", &isa_valid, &g.U, &g.n_long, &g.n_long_rec, &g.n_mid, &g.n_mid_rec, &sw.hybrid,
                      &sw.hybrid_pct, &lg_max) != 9) return 1;
            printf("\"%s\"\n", kinds[bwt_round_kind(isa_valid != 0, g, sw, lg_max)]);
        } else if (!strcmp(cmd, "pays")) {
            unsigned U, U2; int text_rounds;
            if (scanf("%u %u %d", &U, &U2, &text_rounds) != 3) return 1;
            printf("%s\n", bwt_text_round_pays(U, U2, text_rounds) ? "true" : "false");
        } else return 1;
    }
    return 0;
}
