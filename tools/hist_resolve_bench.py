"""hist_resolve_bench.py — what BSCGPU_OPT_DC_HIST_EXACT costs and what it replaces ("Open run_hist brackets, resolved
exactly").  One JSON line per measurement on stdout; legs interleaved (off, on, off, on, ...), the first pair of every leg allocates and
is not reported.  Times of kernel classes are HIP-event times from bscgpu_profile_get: `dc_ctx` = the contexts class, which holds
dc_ctx_kernel with its look-back and, with the option on, the resolve's launches; `model` = every dc_* class and the radix passes of
the model.

  --price    the 64 MiB bench block (synth_text_v1(1)) through compress_device: 0.015 % of its runs are open after nine predecessors,
             so with the option on it pays the map pass and saves their look-backs
  --inputs   hist_q9216 (kept today behind the longest look-back) through the stage function, and the whole block whose BWT declines
             with FAIL_HIST (tests/devcoder_inputs.py: WHOLE_BLOCKS) through compress_device: device model with the option on against
             the host-model fallback of the same block, wall and CPU seconds per block
  --worst    one chain of same-class runs through an 8 MiB block (hist_chain): declined today after every run's look-back, kept with
             the option on.  Under `rocprofv3 --kernel-trace --stats` the same run gives the resolve's launches per kernel.
"""
import argparse
import json
import os
import resource
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

MODEL = ("dc_ctx", "dc_part", "dc_eval", "dc_replay", "dc_pstream", "dc_facts", "radix_scatter", "radix_hist", "radix_scan", "radix_hist_all", "radix_aux")


def cpu_s():
    r = resource.getrusage(resource.RUSAGE_SELF)
    return r.ru_utime + r.ru_stime


def out(**kw):
    print(json.dumps(kw), flush=True)


def classes(st, per=1):
    g = lambda k: st.get(k, dict(ms=0.0))["ms"] / per
    return dict(dc_ctx_ms=round(g("dc_ctx"), 4), model_ms=round(sum(g(k) for k in MODEL), 4))


def counters(c):
    return dict(last_fail=c.option_get(c.CNT_DC_LAST_FAIL), hist_ext=c.option_get(c.CNT_DC_HIST_EXTENDED), resolved=c.option_get(c.CNT_DC_HIST_RESOLVED))


def whole_block(c, T, name, args, leg):
    """T through compress_device, option off / on: wall, CPU and the kernel classes per block"""
    import torch
    d = torch.from_numpy(T).cuda()
    c.profile(True)
    ref = None
    for rep in range(args.reps + 1):
        for opt in (0, 1):
            c.option_set(c.OPT_DC_HIST_EXACT, opt)
            c.profile_reset()
            c0, t0 = cpu_s(), time.perf_counter()
            for _ in range(args.inner):
                got = c.compress_device(d, T.size, 1, 1).tobytes()
            wall, cpu = (time.perf_counter() - t0) / args.inner, (cpu_s() - c0) / args.inner
            ref = ref or got
            assert got == ref
            if rep:
                out(leg=leg, input=name, bytes=int(T.size), option=opt, wall_ms_per_block=round(wall * 1e3, 3), cpu_ms_per_block=round(cpu * 1e3, 3),
                    **classes(c.profile_get(), args.inner), **counters(c))


def stage(c, L, name, args, leg):
    """the sorted block L through the stage function, option off / on (a declined block: the classes up to the exit)"""
    from libbsc_amd.gpu import GpuError
    c.profile(True)
    for rep in range(args.reps + 1):
        for opt in (0, 1):
            c.option_set(c.OPT_DC_HIST_EXACT, opt)
            c.profile_reset()
            kept, D = True, 0
            t0 = time.perf_counter()
            for _ in range(args.inner):
                try:
                    D = int(len(c.qlfc_static_pstream(L)[0]))
                except GpuError:
                    kept = False
            wall = (time.perf_counter() - t0) / args.inner
            if rep:
                out(leg=leg, input=name, bytes=int(L.size), option=opt, kept=kept, decisions=D, stage_wall_ms=round(wall * 1e3, 3), **classes(c.profile_get(), args.inner), **counters(c))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--price", action="store_true")
    ap.add_argument("--inputs", action="store_true")
    ap.add_argument("--worst", action="store_true")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--inner", type=int, default=5, help="blocks per timed loop")
    args = ap.parse_args()
    import devcoder_inputs as di
    from libbsc_amd import GpuContext
    from libbsc_amd.synth import synth_text_v1
    if args.price:
        n = 64 << 20
        c = GpuContext(0, max_n=n + 4096)
        try:
            whole_block(c, synth_text_v1(1, n), "bench block 64 MiB", args, "price")
        finally:
            c.close()
    if args.inputs:
        c = GpuContext(0, max_n=(16 << 20) + 4096)
        try:
            stage(c, di.GENERATORS["hist_q9216"][2](), "hist_q9216", args, "inputs")
            stage(c, di.WHOLE_BLOCKS["fail_hist"][2](), "fail_hist block, the stage", args, "inputs")
            whole_block(c, di.text_with_bwt_like(di.WHOLE_BLOCKS["fail_hist"][2]()), "whole block fail_hist", args, "inputs")
        finally:
            c.close()
    if args.worst:
        c = GpuContext(0, max_n=(16 << 20) + 4096)
        try:
            stage(c, di.hist_chain((8 << 20) // 3), "one chain through 8 MiB", args, "worst")
        finally:
            c.close()


if __name__ == "__main__":
    main()
