"""replay_resolve_bench.py — what BSCGPU_OPT_DC_REPLAY_EXACT costs and what it replaces ("Open chunk starts, resolved
exactly").  One JSON line per measurement on stdout; legs interleaved (off, on, off, on, ...), the first pair of every leg allocates and
is not reported.  Times of kernel classes are HIP-event times from bscgpu_profile_get: `eval` = dc_eval + dc_replay (the evaluation
with the stage in it), `model` = every dc_* class and the radix passes of the model.

  --price    inputs without an open stretch, where the option only adds its two launches: the 64 MiB bench block (synth_text_v1(1))
             through compress_device, and W2's pass (tools/batch_bench.py: 128 x 512 KiB) through compress_batch with
             BSCGPU_OPT_BATCH_MODEL
  --inputs   alt_rf_static_2x61_chunks (kept today behind 3660 serially replayed chunks) through the stage function, and the whole
             block whose BWT declines with FAIL_REPLAY (tests/devcoder_inputs.py: WHOLE_BLOCKS) through compress_device: device
             model with the option on against the host-model fallback of the same block, wall and CPU seconds per block
  --long     one chain open over about 512 and about 1024 chunks per sub-block (32 Mi and 64 Mi single-byte runs, the word of
             alt_rf_static_*): the stage's classes with the option on — how the one-lane chaining scales with the stretch
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

MODEL = ("dc_ctx", "dc_part", "dc_eval", "dc_replay", "dc_pstream", "dc_facts", "radix_scatter", "radix_hist", "radix_scan", "radix_hist_all", "radix_aux")


def cpu_s():
    r = resource.getrusage(resource.RUSAGE_SELF)
    return r.ru_utime + r.ru_stime


def out(**kw):
    print(json.dumps(kw), flush=True)


def classes(st, per=1):
    g = lambda k: st.get(k, dict(ms=0.0))["ms"] / per
    return dict(eval_ms=round(g("dc_eval") + g("dc_replay"), 4), dc_eval_ms=round(g("dc_eval"), 4), dc_replay_ms=round(g("dc_replay"), 4),
                model_ms=round(sum(g(k) for k in MODEL), 4))


def counters(c):
    return dict(last_fail=c.option_get(c.CNT_DC_LAST_FAIL), replays=c.option_get(c.CNT_DC_REPLAYS), resolved=c.option_get(c.CNT_DC_REPLAY_RESOLVED))


def price(args):
    import torch
    import batch_bench as bb
    from libbsc_amd import GpuContext
    from libbsc_amd.synth import synth_text_v1
    n = 64 << 20
    T = synth_text_v1(1, n)
    c = GpuContext(0, max_n=n + 4096)
    try:
        d = torch.from_numpy(T).cuda()
        c.profile(True)
        ref = None
        for rep in range(args.reps + 1):
            for opt in (0, 1):
                c.option_set(c.OPT_DC_REPLAY_EXACT, opt)
                c.profile_reset()
                t0 = time.perf_counter()
                for _ in range(args.inner):
                    got = c.compress_device(d, n, 1, 1).tobytes()
                wall = (time.perf_counter() - t0) / args.inner
                ref = ref or got
                assert got == ref
                if rep:
                    out(leg="price", input="bench block 64 MiB", option=opt, wall_ms_per_block=round(wall * 1e3, 3), **classes(c.profile_get(), args.inner), **counters(c))
        del d
        sizes, blks = bb.workload("W2")
        total = sum(b.size for b in blks)
        c.option_set(c.OPT_BATCH_MODEL, 1)
        ref = None
        for rep in range(args.reps + 1):
            for opt in (0, 1):
                c.option_set(c.OPT_DC_REPLAY_EXACT, opt)
                c.profile_reset()
                p0 = c.option_get(c.CNT_BATCH_MODEL_PASSES)
                t0 = time.perf_counter()
                got = c.compress_batch(blks, 1, 1)
                wall = time.perf_counter() - t0
                ref = ref or got
                assert got == ref
                if rep:
                    out(leg="price", input="W2 pass 128 x 512 KiB", option=opt, bytes=total, wall_ms=round(wall * 1e3, 3), model_passes=c.option_get(c.CNT_BATCH_MODEL_PASSES) - p0,
                        **classes(c.profile_get()), **counters(c))
    finally:
        c.close()


def inputs(args):
    import torch
    import devcoder_inputs as di
    from libbsc_amd import GpuContext
    L = di.GENERATORS["alt_rf_static_2x61_chunks"][2]()
    c = GpuContext(0, max_n=(16 << 20) + 4096)
    try:
        c.profile(True)
        ref = None
        for rep in range(args.reps + 1):
            for opt in (0, 1):
                c.option_set(c.OPT_DC_REPLAY_EXACT, opt)
                c.profile_reset()
                t0 = time.perf_counter()
                for _ in range(args.inner):
                    ps = c.qlfc_static_pstream(L)[0]
                wall = (time.perf_counter() - t0) / args.inner
                ref = ps if ref is None else ref
                assert np.array_equal(ps, ref)
                if rep:
                    out(leg="inputs", input="alt_rf_static_2x61_chunks", option=opt, stage_wall_ms=round(wall * 1e3, 3), **classes(c.profile_get(), args.inner), **counters(c))
    finally:
        c.close()
    T = di.text_with_bwt_like(di.WHOLE_BLOCKS["fail_replay"][2]())
    c = GpuContext(0, max_n=16 << 20)
    try:
        d = torch.from_numpy(T).cuda()
        ref = None
        for rep in range(args.reps + 1):
            for opt in (0, 1):
                c.option_set(c.OPT_DC_REPLAY_EXACT, opt)
                c0, t0 = cpu_s(), time.perf_counter()
                for _ in range(args.inner):
                    got = c.compress_device(d, T.size, 1, 1).tobytes()
                wall, cpu = (time.perf_counter() - t0) / args.inner, (cpu_s() - c0) / args.inner
                ref = ref or got
                assert got == ref
                if rep:
                    out(leg="inputs", input="whole block fail_replay", bytes=int(T.size), option=opt, wall_ms_per_block=round(wall * 1e3, 3), cpu_ms_per_block=round(cpu * 1e3, 3), **counters(c))
    finally:
        c.close()


def long_stretch(args):
    import devcoder_inputs as di
    from libbsc_amd import GpuContext
    c = GpuContext(0, max_n=(64 << 20) + 4096)
    try:
        c.profile(True)
        c.option_set(c.OPT_DC_REPLAY_EXACT, 1)
        for runs in (32 << 20, 64 << 20):
            L = di.periodic(di._W_RF_STATIC, [1], runs)
            for rep in range(args.reps + 1):
                c.profile_reset()
                t0 = time.perf_counter()
                ps = c.qlfc_static_pstream(L)[0]
                wall = time.perf_counter() - t0
                if rep:
                    got = counters(c)
                    out(leg="long", runs=runs, sub_blocks=8, chunks_per_stretch=got["resolved"] // 8, decisions=int(len(ps)), stage_wall_ms=round(wall * 1e3, 3), **classes(c.profile_get()), **got)
            del L, ps
    finally:
        c.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--price", action="store_true")
    ap.add_argument("--inputs", action="store_true")
    ap.add_argument("--long", action="store_true")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--inner", type=int, default=5, help="blocks per timed loop")
    args = ap.parse_args()
    if args.price:
        price(args)
    if args.inputs:
        inputs(args)
    if args.long:
        long_stretch(args)


if __name__ == "__main__":
    main()
