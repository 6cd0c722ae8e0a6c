"""The LZP stage alone: python tools/lzp_device_bench.py [--mib 64] [--lzp 15,128] [--reps 3] [--batch KIB,KIB,...] [--out FILE]

For the bench text and the two file corpora of bench.py --input: bscgpu_lzp_compress_device on a block in HBM — HIP-event time per kernel
class (lzp: keys, links, flags, sweep; radix_aux: the sort's passes) and the call's wall time — against bsc_lzp_compress of the same block
on the host (wall and CPU time; it runs a chunk per thread, at most eight), the two legs alternating.  Next to the times: the block's
matches, dirty look-ups, failed verifies and escaped literals.  One JSON line per input; the outputs are compared byte for byte.

--batch 64,256,512: the stage over a pass instead (bscgpu_lzp_batch_device) — the same input cut into blocks of that many KiB, one run
of the stage for all of them, against the loop of bsc_lzp_compress over the same blocks on 16 threads; one line per input and size."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=64)
    ap.add_argument("--lzp", default="15,128")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--batch", default=None, help="block sizes in KiB: the stage over a pass of such blocks")
    args = ap.parse_args()
    import torch
    from libbsc_amd import GpuContext, api
    from libbsc_amd.synth import image_corpus
    h, m = (int(x) for x in args.lzp.split(","))
    n = args.mib << 20
    ctx = GpuContext(0, max_n=n + 4096)
    ctx.profile(True)
    lines = []
    for name in ("synth-text-v1", "python-source", "binary"):
        T = api.synth_text_v1(10, n) if name == "synth-text-v1" else image_corpus(name, n)
        if T is None:
            print(f"# no files for {name} in this image", flush=True)
            continue
        d = torch.from_numpy(T).cuda()
        if args.batch:
            for kib in (int(x) for x in args.batch.split(",")):
                line = batch_line(ctx, torch, api, name, T, d, kib << 10, h, m, args.reps)
                print(json.dumps(line), flush=True)
                lines.append(line)
            continue
        want = api.bsc_lzp_compress(T, h, m, features=3)                     # (warm: both legs once)
        got = ctx.lzp_compress(d, h, m, features=3, device=True)
        assert got == want, name
        dev_wall, dev_lzp, dev_sort, host_wall, host_cpu = [], [], [], [], []
        for _ in range(args.reps):
            ctx.profile_reset()
            t0 = time.perf_counter()
            r = ctx.L.bscgpu_lzp_compress_device(ctx.h, d.data_ptr(), ctx_out(ctx, torch, n).data_ptr(), n, h, m, 3)
            dev_wall.append((time.perf_counter() - t0) * 1e3)
            assert r == (want if isinstance(want, int) else len(want))
            st = ctx.profile_get()
            dev_lzp.append(st["lzp"]["ms"]); dev_sort.append(st["radix_aux"]["ms"])
            c0, t0 = time.process_time(), time.perf_counter()
            api.bsc_lzp_compress(T, h, m, features=3)
            host_wall.append((time.perf_counter() - t0) * 1e3); host_cpu.append(time.process_time() - c0)
        med = lambda v: round(float(np.median(v)), 3)
        line = dict(input=name, mib=args.mib, hash=h, minlen=m, result=want if isinstance(want, int) else len(want),
                    device_wall_ms=med(dev_wall), device_lzp_class_ms=med(dev_lzp), device_radix_aux_ms=med(dev_sort),
                    host_wall_ms=med(host_wall), host_cpu_s=med(host_cpu), counters=ctx.lzp_counters(),
                    device_wall_all=[round(x, 2) for x in dev_wall], host_wall_all=[round(x, 2) for x in host_wall])
        print(json.dumps(line), flush=True)
        lines.append(line)
    ctx.close()
    if args.out:
        with open(args.out, "w") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


HOST_THREADS = 16


def batch_line(ctx, torch, api, name, T, d, block, h, m, reps):
    """one pass of T in blocks of `block` bytes: the stage's kernel classes and wall time against the host loop on HOST_THREADS threads"""
    from concurrent.futures import ThreadPoolExecutor
    n = T.size
    sizes = np.array([min(block, n - lo) for lo in range(0, n, block)], np.int32)
    offs = np.concatenate([[0], np.cumsum(sizes)])
    blocks = [T[offs[b]:offs[b + 1]] for b in range(sizes.size)]
    res = np.zeros(sizes.size, np.int32)
    out = ctx_out(ctx, torch, n)
    pool = ThreadPoolExecutor(HOST_THREADS)
    host = lambda: list(pool.map(lambda blk: api.bsc_lzp_compress(blk, h, m, features=3), blocks))
    run = lambda: ctx._check(ctx.L.bscgpu_lzp_batch_device(ctx.h, d.data_ptr(), out.data_ptr(), sizes.ctypes.data, sizes.size, h, m, 3, res.ctypes.data))
    want = host()                                                            # (warm: both legs once, and the outputs compared)
    run()
    oh = out.cpu().numpy()
    for b, w in enumerate(want):
        assert res[b] == (w if isinstance(w, int) else len(w)), (name, block, b)
        assert isinstance(w, int) or oh[offs[b]:offs[b] + len(w)].tobytes() == w, (name, block, b)
    dev_wall, dev_lzp, dev_sort, host_wall, host_cpu = [], [], [], [], []
    for _ in range(reps):
        ctx.profile_reset()
        t0 = time.perf_counter()
        run()
        dev_wall.append((time.perf_counter() - t0) * 1e3)
        st = ctx.profile_get()
        dev_lzp.append(st["lzp"]["ms"]); dev_sort.append(st["radix_aux"]["ms"])
        c0, t0 = time.process_time(), time.perf_counter()
        host()
        host_wall.append((time.perf_counter() - t0) * 1e3); host_cpu.append(time.process_time() - c0)
    pool.shutdown()
    med = lambda v: round(float(np.median(v)), 3)
    kept = [w for w in want if not isinstance(w, int)]
    return dict(input=name, mib=n >> 20, block_kib=block >> 10, blocks=int(sizes.size), hash=h, minlen=m,
                coded_blocks=len(kept), coded_bytes=sum(len(w) for w in kept),
                device_wall_ms=med(dev_wall), device_lzp_class_ms=med(dev_lzp), device_radix_aux_ms=med(dev_sort),
                host_threads=HOST_THREADS, host_wall_ms=med(host_wall), host_cpu_s=med(host_cpu), counters=ctx.lzp_counters(),
                device_wall_all=[round(x, 2) for x in dev_wall], host_wall_all=[round(x, 2) for x in host_wall])


_OUT = {}


def ctx_out(ctx, torch, n):
    if n not in _OUT:
        _OUT[n] = torch.empty(n, dtype=torch.uint8, device="cuda")
    return _OUT[n]


if __name__ == "__main__":
    main()
