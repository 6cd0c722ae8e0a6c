"""avg_resolve_bench.py — what BSCGPU_OPT_DC_AVG_EXACT costs and what it replaces ("Open avg_rank flags, resolved exactly").
One JSON line per measurement on stdout.

  --worst    an 8 MiB block of constant rank 40 (8 Mi runs, every chunk's start bracket open): the stage with the option off (declined at
             the first sync) and on, the contexts bracket's HIP-event time (`dc_ctx`: flags, items, contexts) either way — the
             difference is the resolve's five launches.  Under `rocprofv3 --kernel-trace --stats` the same run gives them per kernel.
  --blocks   the realistic single-flag block (tests/avg_resolve_inputs.py) and the whole block of constant rank 40
             (tests/devcoder_inputs.py: WHOLE_BLOCKS["fail_avg"]) through compress_device, option off (redone on the host model)
             against on, interleaved: wall and CPU seconds per block
  --batch    a W3-style call (tools/batch_bench.py: 1000 seeded sizes, 1 KiB .. 900 KiB) with two text-then-noise blocks that each leave
             a flag open in front of every 60 MiB of it, BSCGPU_OPT_BATCH_MODEL + _SEGMENTS, option off against on, interleaved: MB/s,
             CPU seconds and BSCGPU_CNT_BATCH_SEG_HOST_BLOCKS
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


def cpu_s():
    r = resource.getrusage(resource.RUSAGE_SELF)
    return r.ru_utime + r.ru_stime


def out(**kw):
    print(json.dumps(kw), flush=True)


def worst(args):
    import devcoder_inputs as di
    from libbsc_amd import GpuContext
    from libbsc_amd.gpu import GpuError
    L = di.const_rank(40, 8 << 20)
    c = GpuContext(0, max_n=(64 << 20) + 4096)
    try:
        c.profile(True)
        for rep in range(args.reps + 1):                               # (the first pair allocates)
            for opt in (0, 1):
                c.option_set(c.OPT_DC_AVG_EXACT, opt)
                c.profile_reset()
                t0 = time.perf_counter()
                try:
                    ps = c.qlfc_static_pstream(L)[0]
                    kept = len(ps)
                except GpuError as e:
                    assert e.code == -4
                    kept = 0
                wall = time.perf_counter() - t0
                if rep:
                    out(leg="worst", option=opt, runs=int(L.size), chunks=(int(L.size) + 1023) // 1024, decisions_kept=kept, stage_wall_ms=round(wall * 1e3, 3),
                        dc_ctx_ms=round(c.profile_get()["dc_ctx"]["ms"], 4), last_fail=c.option_get(c.CNT_DC_LAST_FAIL),
                        undecided=c.option_get(c.CNT_DC_AVG_UNDECIDED), resolved=c.option_get(c.CNT_DC_AVG_RESOLVED))
    finally:
        c.close()


def blocks(args):
    import torch
    import avg_resolve_inputs as ar
    import devcoder_inputs as di
    from libbsc_amd import GpuContext
    for name, T in (("realistic", ar.realistic_text()), ("whole_fail_avg", di.text_with_bwt_like(di.WHOLE_BLOCKS["fail_avg"][2]()))):
        c = GpuContext(0, max_n=8 << 20)
        try:
            d = torch.from_numpy(T).cuda()
            ref = None
            for rep in range(args.reps + 1):
                for opt in (0, 1):
                    c.option_set(c.OPT_DC_AVG_EXACT, opt)
                    c0, t0 = cpu_s(), time.perf_counter()
                    for _ in range(args.inner):
                        got = c.compress_device(d, T.size, 1, 1).tobytes()
                    wall, cpu = (time.perf_counter() - t0) / args.inner, (cpu_s() - c0) / args.inner
                    ref = ref or got
                    assert got == ref
                    if rep:
                        out(leg="blocks", block=name, bytes=int(T.size), option=opt, wall_ms_per_block=round(wall * 1e3, 3), cpu_ms_per_block=round(cpu * 1e3, 3),
                            last_fail=c.option_get(c.CNT_DC_LAST_FAIL), undecided=c.option_get(c.CNT_DC_AVG_UNDECIDED), resolved=c.option_get(c.CNT_DC_AVG_RESOLVED))
        finally:
            c.close()


def batch(args):
    import batch_bench as bb
    from libbsc_amd import GpuContext
    from libbsc_amd.synth import synth_text_v1
    sizes, blks = bb.workload("W3")
    # (text followed by noise as in tests/model_batch_inputs.py; noise seeds 6 and 22 of 1..29 leave a flag open in the block's own BWT)
    text = synth_text_v1(73, 500 << 10)
    bad = [np.concatenate([text, np.random.default_rng(seed).integers(0, 256, 120 << 10, dtype=np.uint8)]) for seed in (6, 22)]
    cases, acc = [], 60 << 20
    for b in blks:
        if acc >= 60 << 20:
            cases += bad
            acc = sum(x.size for x in bad)
        cases.append(b)
        acc += b.size
    total = sum(x.size for x in cases)
    c = GpuContext(0, max_n=(64 << 20) + 4096)
    try:
        c.option_set(c.OPT_BATCH_MODEL, 1)
        c.option_set(c.OPT_BATCH_MODEL_SEGMENTS, 1)
        ref = None
        for rep in range(args.reps + 1):
            for opt in (0, 1):
                c.option_set(c.OPT_DC_AVG_EXACT, opt)
                h0 = c.option_get(c.CNT_BATCH_SEG_HOST_BLOCKS)
                c0, t0 = cpu_s(), time.perf_counter()
                got = c.compress_batch(cases, 1, 1)
                wall, cpu = time.perf_counter() - t0, cpu_s() - c0
                ref = ref or got
                assert got == ref
                if rep:
                    out(leg="batch", blocks=len(cases), bytes=total, option=opt, mb_per_s=round(total / wall / 1e6, 1), cpu_s=round(cpu, 3),
                        seg_host_blocks=c.option_get(c.CNT_BATCH_SEG_HOST_BLOCKS) - h0, undecided_last_pass=c.option_get(c.CNT_DC_AVG_UNDECIDED),
                        resolved_last_pass=c.option_get(c.CNT_DC_AVG_RESOLVED))
    finally:
        c.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worst", action="store_true")
    ap.add_argument("--blocks", action="store_true")
    ap.add_argument("--batch", action="store_true")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--inner", type=int, default=5, help="--blocks: blocks per timed loop")
    args = ap.parse_args()
    if args.worst:
        worst(args)
    if args.blocks:
        blocks(args)
    if args.batch:
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        batch(args)


if __name__ == "__main__":
    main()
