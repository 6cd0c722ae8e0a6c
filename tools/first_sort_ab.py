"""Kernel classes of the 64 MiB BWT's first sort, route by route: python tools/first_sort_ab.py [REPS [LABEL]]
One JSON line per repeat and route (BSCGPU_OPT_BWT_FOLD 0 / 1 / 2, interleaved; a build without the option — BSC_LIB_OVERRIDE — is
measured as it is): event-bracketed ms of packing (on the folded route: count + scan + packing), rs_hist_all, every full-size digit
pass, their sum, and the first seg behind them (seg_reduce reads the sorted arrays next)."""
import json, os, sys
sys.path.insert(0, '.')
import torch
from libbsc_amd import GpuContext, GpuError, api
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 3
label = sys.argv[2] if len(sys.argv) > 2 else "this"
n = 64 << 20
T = api.synth_text_v1(2, n)                      # bench.py's block
ctx = GpuContext(0, max_n=n + 4096)
d = torch.from_numpy(T).cuda(); out = torch.empty_like(d)
try:
    ctx.option_get(20); routes = [0, 1, 2]       # BSCGPU_OPT_BWT_FOLD
except GpuError:
    routes = [None]
ctx.bwt_device(d, out, n, aux_rate=1 << 23)
for rep in range(reps):
    for fold in routes:
        if fold is not None:
            ctx.option_set(20, fold)
        ctx.bwt_device(d, out, n, aux_rate=1 << 23)
        ctx.profile(True); ctx.profile_reset(); ctx.bwt_device(d, out, n, aux_rate=1 << 23)
        k = ctx.profile_get(); sl = ctx.scatter_launches(); ctx.profile(False)
        passes = [round(m, 4) for m, rec in sl if rec == n]
        row = {"build": label, "fold": fold, "rep": rep, "pack": round(k["pack"]["ms"], 4), "radix_hist_all": round(k["radix_hist_all"]["ms"], 4),
               "passes": passes, "seg": round(k["seg"]["ms"], 4), "bwt_kernels": round(sum(v["ms"] for v in k.values()), 4)}
        row["first_sort"] = round(row["pack"] + row["radix_hist_all"] + sum(passes), 4)
        print(json.dumps(row), flush=True)
ctx.close()
