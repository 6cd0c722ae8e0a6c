"""block_segments_bench.py — what BSCGPU_OPT_DC_ARENA_DIV costs on one block ("A block in sub-block segments").
One JSON line per measurement on stdout.

One text block (synth_text_v1, --mib MiB, --seed) through compress_device on four contexts of max_n = the block, k = 1, 2, 4, 8,
interleaved (k = 1, 2, 4, 8, 1, 2, ... --reps times after a round that allocates): wall and CPU milliseconds of the call, the HIP-event
milliseconds of the dc_* classes and of the facts class, the segments the block ran in, the syncs of its model — one for the facts and
two per segment on a divided arena, two for the whole block on an undivided one (counted from the route, not measured) — and
bscgpu_arena_bytes beside bscgpu_model_arena_bytes (the model's own arena, which the first does not count).  A divisor whose plan has no segment for the block (a sub-block alone above the capacity) shows segments 0 and the
host model's time."""
import argparse
import hashlib
import json
import os
import resource
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DC = ("dc_facts", "dc_ctx", "dc_part", "dc_eval", "dc_replay", "dc_pstream")


def cpu_s():
    r = resource.getrusage(resource.RUSAGE_SELF)
    return r.ru_utime + r.ru_stime


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=64)
    ap.add_argument("--seed", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--coder", type=int, default=1)
    ap.add_argument("--divisors", type=int, nargs="*", default=[1, 2, 4, 8])
    args = ap.parse_args()
    import torch
    from libbsc_amd import GpuContext, api
    n = args.mib << 20
    T = api.synth_text_v1(args.seed, n)
    d = torch.from_numpy(T).cuda()
    ctxs = {}
    for k in args.divisors:
        c = GpuContext(0, max_n=n + 4096)
        c.option_set(c.OPT_DC_ARENA_DIV, k)
        c.profile(True)
        ctxs[k] = c
    try:
        md5 = {}
        for rep in range(args.reps + 1):
            for k, c in ctxs.items():
                c.profile_reset()
                t0, c0 = time.perf_counter(), cpu_s()
                blk = c.compress_device(d, n, 1, args.coder).tobytes()
                wall, cpu = time.perf_counter() - t0, cpu_s() - c0
                md5[k] = hashlib.md5(blk).hexdigest()
                if not rep:
                    continue
                p = c.profile_get()
                seg = c.option_get(c.CNT_DC_BLOCK_SEGMENTS)
                fail = c.option_get(c.CNT_DC_LAST_FAIL)
                syncs = 2 if k == 1 else (1 + 2 * seg if seg else 1)
                print(json.dumps(dict(mib=args.mib, coder=args.coder, k=k, rep=rep, wall_ms=round(wall * 1e3, 2), cpu_ms=round(cpu * 1e3, 2), segments=seg,
                                      last_fail=fail, model_syncs=syncs, arena_bytes=c.arena_bytes, model_arena_bytes=c.model_arena_bytes, dcap=c.option_get(c.CNT_DC_DCAP), md5=md5[k],
                                      **{name + "_ms": round(p[name]["ms"], 3) for name in DC}, **{name + "_launches": p[name]["launches"] for name in DC})),
                      flush=True)
        print(json.dumps(dict(same_bytes=len(set(md5.values())) == 1)), flush=True)
    finally:
        for c in ctxs.values():
            c.close()


if __name__ == "__main__":
    main()
