"""Batched compression of many small blocks against the per-block paths (include/bscgpu.h: bscgpu_compress_batch).

Workloads (inputs from synth_text_v1 seeds, nothing read from outside the tree):
  W1  1024 x 64 KiB      W2  128 x 512 KiB      W3  1000 seeded sizes from 1 KiB to 900 KiB
Each through
  batch         GpuContext.compress_batch on one context (64 MiB + 4096), host input
  batch_device  GpuContext.compress_batch_device on the same context, the blocks back to back in HBM
  pipe          the existing Pipe: bench.py's shape (5 contexts, depth 2, one submitting thread per pipe), blocks from HBM
  dropin16      16 threads calling this library's drop-in bsc_compress (GPU default contexts: NOT a CPU baseline)
  ref_cpu16     16 threads calling the compiled reference's bsc_compress, one block per thread without its own
                threads (features = fast mode only): the reference's block-parallel CPU mode (needs oracle/_ref)
reporting MB/s, CPU-seconds per MB (this process's user + system time) and whether every output equals the pipe's (the
single-block path).  Also the GPU time of one batched 64 MiB pass of W1 (bscgpu_bwt_batch_device) beside one 64 MiB block's BWT.
One JSON line per measurement on stdout.
    python tools/batch_bench.py [--reps 3] [--workloads W1,W2,W3]

--sorter K (default 1, the BWT: the legs above as they are): the same workloads and legs with the sort transform of order K = 3..8
(bscgpu_st_batch_device's passes inside the batch calls; no ref_cpu16 leg for K = 7, 8, which the reference's CPU build does not
encode), and per workload a transform-only leg, the blocks back to back in HBM: GpuContext's st_batch route (bscgpu_st_batch_device)
against a loop of bscgpu_st_encode_device over the same blocks, repetitions interleaved (batch, loop, batch, loop, ...), every
repetition reported.  --transform-only skips the compression legs.
    python tools/batch_bench.py --sorter 5 [--transform-only] [--reps 5] [--workloads W1,W2]

--decode: the decode side on W1..W3 and W4 = 8 x 64 MiB, blocks compressed with -e1 / -e2, without LZP and with
-H15 -M128 (--configs picks some), MB/s of decoded output for
  batch         GpuContext.decompress_batch (host output)
  batch_device  GpuContext.decompress_batch_device (output in HBM)
  dropin16      16 threads calling this library's drop-in bsc_decompress
  ref_cpu16     16 threads calling the compiled reference's bsc_decompress, one block per thread (features = fast mode only)
every output checked against the original.  --decode --profile-pass: one decompress_batch of W1 only (for rocprofv3).
    python tools/batch_bench.py --decode [--reps 2] [--workloads W1,W2,W3,W4] [--configs e1,e2,e1-lzp,e2-lzp]

--front: the batch legs with BSCGPU_OPT_BATCH_FRONT on and off (the QLFC front end of a pass on the GPU, run arrays down
instead of L), host and HBM input, and the pipe, repetitions interleaved (on, off, on_device, off_device, pipe, on, ...); every
repetition's wall time, the medians, CPU-s per MB of the median repetition's neighbours (the mean), a hash check of every output.
--front-only: per workload the stage alone on one pass's L in HBM — bscgpu_qlfc_front_batch_device, wall and the HIP-event time of
its kernel classes (SEG, MISC, GATHER) — against a loop of the single-block front end over the same blocks (the front end of
bscgpu_qlfc_static_pstream, isolated through the same three classes: the device model behind it books to other classes).
--profile-pass with --front: one compress_batch of the workload with the option on, nothing timed (for rocprofv3).
    python tools/batch_bench.py --front [--front-only] [--reps 3] [--workloads W1,W2,W3]

--model: the batch legs with BSCGPU_OPT_BATCH_MODEL on and off (the static coder's model of a pass on the GPU, the
probability stream down, host threads run the range coder only), host and HBM input, and the pipe, repetitions interleaved (on, off,
on_device, off_device, pipe, on, ...), coder -e1; every repetition's wall time, the medians, CPU-s per MB, how many passes the model
kept and declined, a SHA-256 of every output against the pipe's.  --model-only: per workload the stage alone on one pass's L in HBM —
bscgpu_static_pstream_batch_device, wall and the HIP-event time per kernel class (contexts, sorts, partition, evaluation, p stream;
the front end beside them).  The on legs also run with BSCGPU_OPT_DEVICE_RC = 1 (the pass's streams coded by one launch of the
device's range coder).  --model-sweep: on against off on passes of 64 KiB .. 16 MiB cut from the workload's text — the smallest pass
the model route wins on (run it with BSC_BATCH_MODEL_MIN_PASS=0 in the environment).  Raw output belongs under profiles/batch_model/.
With --coder 2 --model and --model-only drive the adaptive coder's route (BSCGPU_OPT_BATCH_MODEL_ADAPTIVE, -e2,
bscgpu_adaptive_pstream_batch_device; no device range coder or packed form there; --segments drives its own segments option, below);
--model-only then also prints the pass's
mixer chains, the longest chain, the walk's wall time and ns per dependent step, the host coder's wall time for the same pass on 16
threads, and the chain cap those two give (the steps the walk does in the host's time, rounded down to a power of two).
With --coder 3 all three drive the fast coder's route instead (BSCGPU_OPT_BATCH_MODEL_FAST, -e0, bscgpu_fast_pstream_batch_device; the
stage-alone leg adds the pass's decisions per byte from the CPU stand-in); raw output under profiles/batch_fast/.
    python tools/batch_bench.py --model [--model-only | --model-sweep] [--reps 3] [--workloads W1,W2,W3]

--segments (with --model, either coder): the whole-call legs become model off / model on / model + BSCGPU_OPT_BATCH_MODEL_SEGMENTS,
host and HBM input, interleaved, with the segment counters of every leg; --model-only runs the segmented stage
(bscgpu_pstream_batch_segments_device) instead of the whole-pass stage, the facts kernels as a class of their own (dc_facts) and the
copy-out included in the wall time.  --packed (with --model, -e1): the whole-call legs become model off / model on / model on +
BSCGPU_OPT_BATCH_MODEL_PACKED for either input kind (with --segments: both model legs segmented), with the packed counters and the
assertion that W1's segmented pass leaves no block to the host for landing space; with --model-only the stage in the packed form beside
the 16-bit one, with the assertion bytes = pbase[nsub] / 8 * 13.  Raw output belongs under profiles/batch_packed/.  --segment-sweep: model + segments on W1 and W2, host input, with BSC_BATCH_MODEL_SEGMENT set to
the capacity / 8, / 4, / 2 and the capacity, interleaved with model on and off.  Raw output belongs under profiles/batch_segments/.
With --coder 2 the segments are the adaptive coder's (BSCGPU_OPT_BATCH_ADAPTIVE_SEGMENTS, bscgpu_adaptive_pstream_batch_segments_device):
the same legs and the same sweep; --model-only adds the third fact's kernel on a line of its own (the -e2 facts stage less the -e1
facts stage), the longest chain the facts report, and the chains, longest chain and walk time summed over the pass's segments.  Raw
output belongs under profiles/batch_adaptive_segments/.
    python tools/batch_bench.py --model --segments [--model-only | --segment-sweep] [--coder 3 | --coder 2] [--reps 3] [--workloads W1,W2,W3]

--lzp H,M: the batch calls with LZP ("A pass of small blocks"), three legs interleaved (host_lzp, option_on, hbm, host_lzp,
...): compress_batch with lzp_compress per block on the host (today's route), the same call with BSCGPU_OPT_BATCH_DEVICE_LZP on (the
raw pass goes up, one run of the stage per pass), and compress_batch_device with the LZP parameters (input in HBM).  Every repetition's
wall time, the medians as MB/s, CPU-s per MB, the passes that took the stage, a SHA-256 of every output against the first leg's.  Raw
output belongs under profiles/batch_lzp/.
    python tools/batch_bench.py --lzp 15,128 [--reps 3] [--workloads W1,W2,W3] [--coder 1]
"""
import argparse
import ctypes as C
import json
import os
import resource
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def cpu_s():
    r = resource.getrusage(resource.RUSAGE_SELF)
    return r.ru_utime + r.ru_stime


def workload(name):
    from libbsc_amd.synth import synth_text_v1
    rng = np.random.default_rng({"W1": 1, "W2": 2, "W3": 3, "W4": 4}[name])
    if name == "W1":
        sizes = [64 << 10] * 1024
    elif name == "W2":
        sizes = [512 << 10] * 128
    elif name == "W4":
        sizes = [64 << 20] * 8
    else:
        sizes = [int(x) for x in rng.integers(1 << 10, 900 << 10, 1000)]
    blocks = [synth_text_v1(1000 + i, n) for i, n in enumerate(sizes)]
    return sizes, blocks


def timed(fn):
    c0, t0 = cpu_s(), time.perf_counter()
    out = fn()
    return out, time.perf_counter() - t0, cpu_s() - c0


def run_batch(ctx, blocks, sorter, coder):
    return ctx.compress_batch(blocks, sorter, coder)


def run_pipe(pipes, dblocks, sizes, sorter, coder, depth):
    out = [None] * len(sizes)

    def worker(k):
        p, tickets = pipes[k], []
        for i in range(k, len(sizes), len(pipes)):
            tickets.append((i, p.submit(dblocks[i], sizes[i], sorter, coder, 3)))
            if len(tickets) >= depth:
                j, t = tickets.pop(0)
                out[j] = bytes(p.wait(t))
        for j, t in tickets:
            out[j] = bytes(p.wait(t))

    th = [threading.Thread(target=worker, args=(k,)) for k in range(len(pipes))]
    for t in th:
        t.start()
    for t in th:
        t.join()
    return out


def run_16(blocks, one):
    out = [None] * len(blocks)
    nxt = [0]
    lock = threading.Lock()

    def worker():
        while True:
            with lock:
                i = nxt[0]
                nxt[0] += 1
            if i >= len(blocks):
                return
            out[i] = one(blocks[i])

    th = [threading.Thread(target=worker) for _ in range(16)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    return out


CONFIGS = {"e1": (1, 0, 0), "e2": (2, 0, 0), "e1-lzp": (1, 15, 128), "e2-lzp": (2, 15, 128)}


def decode_main(args):
    from libbsc_amd import GpuContext
    from libbsc_amd import api
    from oracle.refbind import Ref, REF_SO
    refc = Ref() if os.path.exists(REF_SO) else None
    ctx = GpuContext(0, max_n=(64 << 20) + 4096)
    try:
        for name in args.workloads.split(","):
            sizes, datas = workload(name)
            want = [d.tobytes() for d in datas]
            mb = sum(sizes) / 1e6
            for cfg in args.configs.split(","):
                coder, lzp_hash, lzp_min = CONFIGS[cfg]
                blocks = ctx.compress_batch(datas, 1, coder, lzp_hash, lzp_min)
                assert all(isinstance(b, bytes) for b in blocks)
                if args.profile_pass:
                    got = ctx.decompress_batch(blocks)
                    print(json.dumps({"workload": name, "config": cfg, "leg": "profile_pass", "ok": got == want}), flush=True)
                    continue
                ctx.decompress_batch(blocks[:8])                   # warm-up: pinned buffers, batch table
                legs = ["batch", "batch_device", "dropin16"] + (["ref_cpu16"] if refc else [])
                for leg in legs:
                    best, ok = None, True
                    for _ in range(args.reps):
                        if leg == "batch":
                            out, wall, cpu = timed(lambda: ctx.decompress_batch(blocks))
                        elif leg == "batch_device":
                            def dev():
                                T, offs, res = ctx.decompress_batch_device(blocks)
                                import torch
                                torch.cuda.synchronize()
                                return T, offs, res
                            (T, offs, res), wall, cpu = timed(dev)
                            Th = T.cpu().numpy()
                            out = [Th[offs[b]:offs[b + 1]].tobytes() if res[b] == 0 else res[b] for b in range(len(blocks))]
                            del T
                        elif leg == "dropin16":
                            out, wall, cpu = timed(lambda: run_16(blocks, lambda b: api.bsc_decompress(b)))
                        else:
                            out, wall, cpu = timed(lambda: run_16(blocks, lambda b: refc.decompress(b, features=1)))
                        ok = ok and out == want
                        if best is None or wall < best[0]:
                            best = (wall, cpu)
                    print(json.dumps({"workload": name, "config": cfg, "leg": leg, "blocks": len(sizes), "MB": round(mb, 2),
                                      "MB_s": round(mb / best[0], 1), "ms": round(best[0] * 1e3, 1),
                                      "cpu_s_per_MB": round(best[1] / mb, 4), "identical_to_input": bool(ok)}), flush=True)
            del datas, want
    finally:
        ctx.close()


def st_transform_leg(ctx, name, sizes, blocks, k, reps):
    """the sort transform alone, input and output in HBM: one bscgpu_st_batch_device call against one bscgpu_st_encode_device call per block"""
    import torch
    from libbsc_amd import _native as N
    from libbsc_amd.gpu import st_batch_plan
    flat = torch.from_numpy(np.concatenate(blocks)).cuda()
    out_a, out_b = torch.empty_like(flat), torch.empty_like(flat)
    sz = np.array(sizes, np.int32)
    offs = np.concatenate([[0], np.cumsum(sz, dtype=np.int64)])
    idx_a, idx_b = np.zeros(len(sizes), np.int32), np.zeros(len(sizes), np.int32)
    torch.cuda.synchronize()

    def batch():
        rc = ctx.L.bscgpu_st_batch_device(ctx.h, flat.data_ptr(), out_a.data_ptr(), N.np_ptr(sz), len(sizes), k, N.np_ptr(idx_a))
        assert rc == 0, rc

    def loop():
        src, dst = flat.data_ptr(), out_b.data_ptr()
        for b, n in enumerate(sizes):
            idx_b[b] = ctx.L.bscgpu_st_encode_device(ctx.h, src + int(offs[b]), dst + int(offs[b]), n, k)

    batch(), loop()                                         # warm-up: the batch table, both routes' first launches
    tb, tl = [], []
    for _ in range(reps):
        for fn, ts in ((batch, tb), (loop, tl)):
            t0 = time.perf_counter()
            fn()                                            # (both routes are synchronous on return)
            ts.append(round((time.perf_counter() - t0) * 1e3, 2))
    same = bool(torch.equal(out_a, out_b)) and bool((idx_a == idx_b).all())
    print(json.dumps({"workload": name, "sorter": k, "leg": "st_transform_only", "blocks": len(sizes), "MB": round(sum(sizes) / 1e6, 2),
                      "passes": st_batch_plan(sizes, k, ctx.max_n)[0], "st_batch_ms": tb, "st_encode_device_loop_ms": tl,
                      "speedup_of_medians": round(float(np.median(tl) / np.median(tb)), 2), "identical": same}), flush=True)


def front_main(args):
    """BSCGPU_OPT_BATCH_FRONT on against off inside one process, interleaved"""
    import hashlib
    import torch
    from libbsc_amd import GpuContext
    from libbsc_amd import _native as N
    coder = args.coder
    ctx = GpuContext(0, max_n=(64 << 20) + 4096)
    OPT = ctx.OPT_BATCH_FRONT
    FRONT_CLASSES = ("seg", "misc", "gather")
    pctx = [GpuContext(0, max_n=(1 << 20) + 4096) for _ in range(0 if (args.front_only or args.profile_pass) else args.contexts)]
    pipes = [c.pipe(args.depth) for c in pctx]

    def digest(out):
        h = hashlib.sha256()
        for b in out:
            h.update(b if isinstance(b, bytes) else str(b).encode())
        return h.hexdigest()

    def front_ms(c):
        st = c.profile_get()
        return sum(v["ms"] for k, v in st.items() if k in FRONT_CLASSES)

    try:
        for name in args.workloads.split(","):
            sizes, blocks = workload(name)
            mb = sum(sizes) / 1e6
            flat = torch.from_numpy(np.concatenate(blocks)).cuda()
            torch.cuda.synchronize()
            if args.profile_pass:
                ctx.option_set(OPT, 1)
                ctx.compress_batch(blocks[:8], 1, coder)
                out = ctx.compress_batch(blocks, 1, coder)
                print(json.dumps({"workload": name, "leg": "profile_pass", "blocks": len(out)}), flush=True)
                continue
            if args.front_only:
                # one pass's worth of L (the first blocks that fit a pass), from the batched BWT
                from libbsc_amd.gpu import batch_plan
                _, pass_of = batch_plan(sizes, 1, ctx.max_n)
                cnt = sum(1 for x in pass_of if x == 0)
                psz = sizes[:cnt]
                total = sum(psz)
                dL = torch.empty(total, dtype=torch.uint8, device="cuda")
                ctx.bwt_batch(flat[:total], psz, aux=False, dL=dL)
                Lh = dL.cpu().numpy()
                offs = np.concatenate([[0], np.cumsum(psz)])
                ctx.qlfc_front_batch(dL, psz)                              # warm-up: tables, first launches
                ctx.profile(True)
                tw, tk, tl = [], [], []
                st, sz, nb, poff = (C.c_int * 8)(), (C.c_int * 8)(), C.c_int(0), (C.c_int64 * 9)()
                dummy = np.empty(16, np.uint16)
                f = ctx.L.bscgpu_qlfc_static_pstream
                f.restype = C.c_int64
                f.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.POINTER(C.c_int), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
                d16 = torch.zeros(16, dtype=torch.uint8, device="cuda")
                declined, other_ms = 0, 0.0
                for _ in range(args.reps):
                    ctx.profile_reset()
                    t0 = time.perf_counter()
                    fb = ctx.qlfc_front_batch(dL, psz)
                    tw.append(round((time.perf_counter() - t0) * 1e3, 2))
                    tk.append(round(front_ms(ctx), 3))
                    # the flush: a 16-byte Adler-32 syncs the stream and folds every pending event into the classes (a block the device
                    # model declines returns before its own fold); its own kernel time is measured and taken off
                    ctx.profile_reset()
                    ctx.adler32_device(d16, 16)
                    flush = front_ms(ctx)
                    ctx.profile_reset()
                    for b in range(cnt):                                   # (cap 0: the stream itself is not copied out)
                        rc = f(ctx.h, Lh[offs[b]:].ctypes.data, psz[b], dummy.ctypes.data, 0, C.byref(nb), st, sz, poff, None)
                        assert rc >= 0 or rc == -4, f"block {b}: bscgpu_qlfc_static_pstream returned {rc}"      # -4: the model declined, AFTER the front end ran
                        declined += rc == -4
                    ctx.adler32_device(d16, 16)
                    st_all = ctx.profile_get()
                    assert st_all["seg"]["launches"] >= 2 * cnt, "every block's front end must have been timed"
                    tl.append(round(front_ms(ctx) - flush, 3))
                    other_ms = sum(v["ms"] for k, v in st_all.items() if k not in FRONT_CLASSES)
                ctx.profile(False)
                print(json.dumps({"workload": name, "leg": "front_only", "blocks": cnt, "MB": round(total / 1e6, 2), "runs": fb.m, "sub_blocks": fb.nsub,
                                  "front_batch_wall_ms": tw, "front_batch_kernel_ms": tk, "single_block_loop_kernel_ms": tl,
                                  "loop_blocks_declined_by_device_model": declined // max(args.reps, 1), "loop_ms_in_other_classes_last_rep": round(other_ms, 2),
                                  "kernel_speedup_of_medians": round(float(np.median(tl) / np.median(tk)), 2)}), flush=True)
                continue
            dblocks = [torch.from_numpy(b).cuda() for b in blocks]
            torch.cuda.synchronize()
            want = digest(run_pipe(pipes, dblocks, sizes, 1, coder, args.depth))        # warm-up + the single-block outputs
            for v in (1, 0):
                ctx.option_set(OPT, v)
                ctx.compress_batch(blocks[:8], 1, coder)
            legs = {"batch_on": (1, False), "batch_off": (0, False), "batch_device_on": (1, True), "batch_device_off": (0, True), "pipe": None}
            walls = {k: [] for k in legs}
            cpus = {k: [] for k in legs}
            same = {k: True for k in legs}
            for _ in range(args.reps):
                for leg, how in legs.items():
                    if how is None:
                        out, wall, cpu = timed(lambda: run_pipe(pipes, dblocks, sizes, 1, coder, args.depth))
                    else:
                        ctx.option_set(OPT, how[0])
                        out, wall, cpu = timed((lambda: ctx.compress_batch_device(flat, sizes, 1, coder)) if how[1] else (lambda: ctx.compress_batch(blocks, 1, coder)))
                    walls[leg].append(wall); cpus[leg].append(cpu)
                    same[leg] = same[leg] and digest(out) == want
            for leg in legs:
                w = np.array(walls[leg])
                print(json.dumps({"workload": name, "leg": leg, "blocks": len(sizes), "MB": round(mb, 2), "coder": coder,
                                  "ms": [round(x * 1e3, 1) for x in w], "median_MB_s": round(mb / float(np.median(w)), 1),
                                  "MB_s_min_max": [round(mb / float(w.max()), 1), round(mb / float(w.min()), 1)],
                                  "cpu_s_per_MB": round(float(np.mean(cpus[leg])) / mb, 4), "sha256_equals_pipe": bool(same[leg])}), flush=True)
            del dblocks
    finally:
        for p in pipes:
            p.close()
        for c in pctx:
            c.close()
        ctx.close()


def model_main(args):
    """BSCGPU_OPT_BATCH_MODEL on against off inside one process, interleaved; or the stage alone"""
    import hashlib
    import torch
    from libbsc_amd import GpuContext
    from libbsc_amd.gpu import GpuError, batch_plan
    # --coder 3: the fast coder's route (BSCGPU_OPT_BATCH_MODEL_FAST and its own counters); anything else: the static coder's
    fast = args.coder == 3
    adaptive = args.coder == 2                                    # the adaptive coder's route: whole passes of 16-bit entries, host-coded
    coder = 3 if fast else 2 if adaptive else 1
    ctx = GpuContext(0, max_n=(64 << 20) + 4096)
    OPT = ctx.OPT_BATCH_MODEL_FAST if fast else ctx.OPT_BATCH_MODEL_ADAPTIVE if adaptive else ctx.OPT_BATCH_MODEL
    CNT_PASSES = ctx.CNT_BATCH_FAST_PASSES if fast else ctx.CNT_BATCH_ADAPTIVE_PASSES if adaptive else ctx.CNT_BATCH_MODEL_PASSES
    CNT_DECLINED = ctx.CNT_BATCH_FAST_DECLINED if fast else ctx.CNT_BATCH_ADAPTIVE_DECLINED if adaptive else ctx.CNT_BATCH_MODEL_DECLINED
    stage = ctx.fast_pstream_batch if fast else ctx.adaptive_pstream_batch if adaptive else ctx.static_pstream_batch
    if adaptive and args.packed:
        raise SystemExit("--packed is not the adaptive coder's (-e2): its passes and segments are 16-bit entries")
    # the option that puts a model pass into segments: the adaptive coder has one of its own
    SEG_OPT = ctx.OPT_BATCH_ADAPTIVE_SEGMENTS if adaptive else ctx.OPT_BATCH_MODEL_SEGMENTS
    if args.segments:                                             # the segmented stage: (layout, entries, poff) as the whole-pass stage returns them
        stage = (lambda dL, psz: ctx.adaptive_pstream_batch_segments(dL, psz, 0)[:3]) if adaptive else (lambda dL, psz: ctx.pstream_batch_segments(dL, psz, coder, 0)[:3])
    if args.packed and fast:
        raise SystemExit("--packed is the static coder's (-e1): the fast coder's entries use all 16 bits")
    # --packed --model-only: the stage in the packed 13-bit form beside the 16-bit one, same session, interleaved
    stage13 = (lambda dL, psz: ctx.pstream_batch_segments_packed(dL, psz, coder, 0)[:4]) if args.segments else ctx.static_pstream_batch_packed
    PACKED_KEYS = (ctx.CNT_BATCH_PACKED_PASSES, ctx.CNT_BATCH_PACKED_VOID)
    SEG_KEYS = (ctx.CNT_BATCH_SEGMENTS, ctx.CNT_BATCH_SEG_RERUNS, ctx.CNT_BATCH_SEG_HOST_BLOCKS)
    pctx = [GpuContext(0, max_n=(1 << 20) + 4096) for _ in range(0 if (args.model_only or args.model_sweep or args.segment_sweep) else args.contexts)]
    pipes = [c.pipe(args.depth) for c in pctx]
    CLASSES = {"facts": ("dc_facts",), "contexts": ("dc_ctx",), "sorts": ("radix_scatter", "radix_hist", "radix_scan", "radix_hist_all", "radix_aux"),
               "partition": ("dc_part",), "evaluation": ("dc_eval",), "p_stream": ("dc_pstream",), "front_end": ("seg", "misc", "gather")}

    def digest(out):
        h = hashlib.sha256()
        for b in out:
            h.update(b if isinstance(b, bytes) else str(b).encode())
        return h.hexdigest()

    try:
        for name in args.workloads.split(","):
            sizes, blocks = workload(name)
            mb = sum(sizes) / 1e6
            flat = torch.from_numpy(np.concatenate(blocks)).cuda()
            torch.cuda.synchronize()
            if args.model_sweep:
                # the smallest pass the model route wins on: passes of 2^k bytes cut from the workload's text, on / off interleaved
                # (run with BSC_BATCH_MODEL_MIN_PASS=0 in the environment, so that every pass size is given to the model)
                text = np.concatenate(blocks)
                for total in [1 << k for k in range(16, 25)]:
                    bs = min(total, 128 << 10)
                    part = [text[o:o + bs] for o in range(0, total, bs)]
                    for v in (1, 0):
                        ctx.option_set(OPT, v)
                        ctx.compress_batch(part, 1, coder)
                    t = {1: [], 0: []}
                    kept_n = 0
                    for _ in range(max(args.reps, 5)):
                        for v in (1, 0):
                            ctx.option_set(OPT, v)
                            p0 = ctx.option_get(CNT_PASSES)
                            _, wall, _ = timed(lambda: ctx.compress_batch(part, 1, coder))
                            t[v].append(round(wall * 1e3, 3))
                            if v:
                                kept_n = ctx.option_get(CNT_PASSES) - p0
                    print(json.dumps({"workload": name, "leg": "model_sweep", "coder": coder, "pass_bytes": total, "blocks": len(part), "model_passes_per_call": kept_n,
                                      "on_ms": t[1], "off_ms": t[0], "on_median_ms": float(np.median(t[1])), "off_median_ms": float(np.median(t[0]))}), flush=True)
                continue
            if args.segment_sweep:
                # decisions per segment: the capacity / 8, / 4, / 2 and the capacity, beside model on (whole passes) and off
                dcap = ctx.option_get(ctx.CNT_DC_DCAP)
                legs = {"off": (0, 0, None), "on": (1, 0, None)}
                legs.update({f"segments_{dcap // k}": (1, 1, dcap // k) for k in (8, 4, 2, 1)})
                for how in legs.values():                          # warm-up: arenas, pinned buffers
                    ctx.option_set(OPT, how[0]); ctx.option_set(SEG_OPT, how[1])
                    ctx.compress_batch(blocks[:40], 1, coder)
                t = {k: [] for k in legs}
                cnt = {k: None for k in legs}
                ref = None
                for _ in range(args.reps):
                    for leg, how in legs.items():
                        ctx.option_set(OPT, how[0]); ctx.option_set(SEG_OPT, how[1])
                        if how[2] is None:
                            os.environ.pop("BSC_BATCH_MODEL_SEGMENT", None)
                        else:
                            os.environ["BSC_BATCH_MODEL_SEGMENT"] = str(how[2])
                        c0 = [ctx.option_get(k) for k in SEG_KEYS + (CNT_PASSES, CNT_DECLINED)]
                        out, wall, _ = timed(lambda: ctx.compress_batch(blocks, 1, coder))
                        cnt[leg] = [ctx.option_get(k) - a for k, a in zip(SEG_KEYS + (CNT_PASSES, CNT_DECLINED), c0)]
                        t[leg].append(round(wall * 1e3, 1))
                        ref = ref or digest(out)
                        assert digest(out) == ref, leg
                os.environ.pop("BSC_BATCH_MODEL_SEGMENT", None)
                ctx.option_set(SEG_OPT, 0)
                for leg in legs:
                    w = np.array(t[leg])
                    print(json.dumps({"workload": name, "leg": "segment_sweep_" + leg, "coder": coder, "MB": round(mb, 2), "ms": t[leg],
                                      "median_MB_s": round(mb / float(np.median(w)) * 1e3, 1), "MB_s_min_max": [round(mb / float(w.max()) * 1e3, 1), round(mb / float(w.min()) * 1e3, 1)],
                                      "segments_reruns_host_blocks_passes_declined": cnt[leg], "same_output_in_every_leg": True}), flush=True)
                continue
            if args.model_only:
                _, pass_of = batch_plan(sizes, 1, ctx.max_n)
                cnt = sum(1 for x in pass_of if x == 0)
                psz = sizes[:cnt]
                total = sum(psz)
                dL = torch.empty(total, dtype=torch.uint8, device="cuda")
                ctx.bwt_batch(flat[:total], psz, aux=False, dL=dL)
                rec = {"workload": name, "leg": "model_only", "coder": coder, "blocks": cnt, "MB": round(total / 1e6, 2)}
                if fast:                                                          # decisions per byte from the CPU stand-in: does the pass fit 4 per byte?
                    from libbsc_amd import _native as N
                    from libbsc_amd.gpu import front_batch_host
                    import ctypes as C
                    hfb = front_batch_host(dL.cpu().numpy(), psz)
                    dec = sum(int(N.lib().bscgpu_fast_pstream_host(C.byref(hfb.lay), s, None, 0)) for s in range(hfb.nsub))
                    rec["decisions_per_byte_stand_in"] = round(dec / total, 3)
                try:
                    fb, ps, _ = stage(dL, psz)                                    # warm-up: arenas, tables, first launches
                except GpuError as e:
                    print(json.dumps({**rec, "declined": e.code, "last_fail": ctx.option_get(ctx.CNT_DC_LAST_FAIL)}), flush=True)
                    continue
                if args.packed:                                                   # the layout's deterministic check, and the warm-up of the packed launches
                    try:
                        _, pk, poff13, pbase13 = stage13(dL, psz)
                    except GpuError as e:
                        print(json.dumps({**rec, "packed_declined_or_void": e.code, "last_fail": ctx.option_get(ctx.CNT_DC_LAST_FAIL)}), flush=True)
                        continue
                    assert int(pk.size) == int(pbase13[-1]) // 8 * 13, "bytes copied per pass = pbase[nsub] / 8 * 13"
                    rec.update({"packed_bytes": int(pk.size), "bytes_16_bit": 2 * int(ps.size), "pbase_end": int(pbase13[-1])})
                ctx.profile(True)
                tw, per = [], {k: [] for k in CLASSES}
                tw13, per13 = [], {k: [] for k in CLASSES}
                for _ in range(args.reps):
                    for run, walls, classes in ((stage, tw, per),) + (((stage13, tw13, per13),) if args.packed else ()):
                        ctx.profile_reset()
                        t0 = time.perf_counter()
                        run(dL, psz)
                        walls.append(round((time.perf_counter() - t0) * 1e3, 2))
                        st = ctx.profile_get()
                        for k, names in CLASSES.items():
                            classes[k].append(round(sum(st[n]["ms"] for n in names), 3))
                ctx.profile(False)
                g0 = [ctx.option_get(k) for k in SEG_KEYS]
                stage(dL, psz)
                seg_moved = [ctx.option_get(k) - a for k, a in zip(SEG_KEYS, g0)]
                if args.packed:
                    rec.update({"packed_wall_ms_with_front_end_and_copy_out": tw13, "packed_kernel_ms": per13,
                                "p_stream_ms_median_16_bit_vs_packed": [float(np.median(per["p_stream"])), float(np.median(per13["p_stream"]))],
                                "p_stream_ms_min_max_16_bit": [min(per["p_stream"]), max(per["p_stream"])],
                                "p_stream_ms_min_max_packed": [min(per13["p_stream"]), max(per13["p_stream"])]})
                if adaptive and args.segments:
                    # the third fact's kernel on its own line: the facts stage of -e2 (dc_avg, dc_sub_dec, dc_mix_facts) less the facts
                    # stage of -e1 (the first two), HIP-event time of the dc_facts class, interleaved
                    ctx.profile(True)
                    f2, f1 = [], []
                    for _ in range(args.reps):
                        for run, acc in ((lambda: ctx.adaptive_segment_facts(dL, psz), f2), (lambda: ctx.model_segment_facts(dL, psz, 1), f1)):
                            ctx.profile_reset()
                            run()
                            acc.append(round(ctx.profile_get()["dc_facts"]["ms"], 3))
                    ctx.profile(False)
                    sub_mix = ctx.adaptive_segment_facts(dL, psz)[3]
                    rec.update({"facts_stage_ms_e2": f2, "facts_stage_ms_e1": f1, "mix_facts_kernel_ms_median": round(float(np.median(f2) - np.median(f1)), 3),
                                "longest_chain_by_the_facts": int(sub_mix.max()), "segments_reruns_host_blocks_of_a_run": seg_moved})
                if adaptive:
                    # what the chain cap's default is derived from: the walk's time per dependent step (its wall time over the longest
                    # chain) against the host coder's wall time for the same pass, every block from its runs on 16 threads
                    chains, longest = ctx.option_get(ctx.CNT_DC_MIX_CHAINS), ctx.option_get(ctx.CNT_DC_MIX_LONGEST)
                    walk_us = []
                    for _ in range(args.reps):
                        stage(dL, psz)
                        walk_us.append(ctx.option_get(ctx.CNT_DC_MIX_WALK_US))
                    host_ms = []
                    for _ in range(args.reps):
                        t0 = time.perf_counter()
                        run_16(list(range(cnt)), lambda b: fb.code(b, 2, 1))
                        host_ms.append(round((time.perf_counter() - t0) * 1e3, 1))
                    ns_step = float(np.median(walk_us)) * 1e3 / max(longest, 1)
                    steps = float(np.median(host_ms)) * 1e6 / ns_step
                    rec.update({"mixer_chains": chains, "longest_chain": longest, "walk_us": walk_us, "walk_ns_per_step_of_the_longest_chain": round(ns_step, 1),
                                "host_coder_ms_16_threads": host_ms, "steps_the_walk_does_in_the_host_time": int(steps),
                                "chain_cap_power_of_two": 1 << (int(steps).bit_length() - 1)})
                print(json.dumps({**rec, "runs": fb.m, "sub_blocks": fb.nsub, "decisions": int(ps.size), "replays": ctx.option_get(ctx.CNT_DC_REPLAYS),
                                  "wall_ms_with_front_end_and_copy_out": tw, "kernel_ms": per,
                                  "model_kernel_ms_median": round(float(sum(np.median(v) for k, v in per.items() if k != "front_end")), 3)}), flush=True)
                continue
            dblocks = [torch.from_numpy(b).cuda() for b in blocks]
            torch.cuda.synchronize()
            want = digest(run_pipe(pipes, dblocks, sizes, 1, coder, args.depth))        # warm-up + the single-block outputs
            for v in (1, 0):
                ctx.option_set(OPT, v)
                ctx.compress_batch(blocks[:40], 1, coder)
            legs = {"batch_on": (1, False, 0), "batch_off": (0, False, 0), "batch_on_device_rc": (1, False, 1),
                    "batch_device_on": (1, True, 0), "batch_device_off": (0, True, 0), "batch_device_on_device_rc": (1, True, 1), "pipe": None}
            if adaptive:                                           # (the device's range coder does not take this coder's passes)
                legs = {k: v for k, v in legs.items() if not k.endswith("device_rc")}
            if args.segments:                                      # (option, HBM input, device RC, segments)
                legs = {"batch_off": (0, False, 0, 0), "batch_on": (1, False, 0, 0), "batch_segments": (1, False, 0, 1),
                        "batch_device_off": (0, True, 0, 0), "batch_device_on": (1, True, 0, 0), "batch_device_segments": (1, True, 0, 1), "pipe": None}
            if args.packed:                                        # (..., packed): packed on / packed off / model off, interleaved, either input kind
                sg = 1 if args.segments else 0
                legs = {"batch_off": (0, False, 0, 0, 0), "batch_on": (1, False, 0, sg, 0), "batch_on_packed": (1, False, 0, sg, 1),
                        "batch_device_off": (0, True, 0, 0, 0), "batch_device_on": (1, True, 0, sg, 0), "batch_device_on_packed": (1, True, 0, sg, 1), "pipe": None}
            packed_cnt = {k: None for k in legs}
            segs = {k: None for k in legs}
            walls = {k: [] for k in legs}
            cpus = {k: [] for k in legs}
            same = {k: True for k in legs}
            kept = {k: 0 for k in legs}
            declined = {k: 0 for k in legs}
            for _ in range(args.reps):
                for leg, how in legs.items():
                    if how is None:
                        out, wall, cpu = timed(lambda: run_pipe(pipes, dblocks, sizes, 1, coder, args.depth))
                    else:
                        ctx.option_set(OPT, how[0])
                        ctx.option_set(ctx.OPT_DEVICE_RC, how[2])
                        ctx.option_set(SEG_OPT, how[3] if len(how) > 3 else 0)
                        ctx.option_set(ctx.OPT_BATCH_MODEL_PACKED, how[4] if len(how) > 4 else 0)
                        p0, d0 = ctx.option_get(CNT_PASSES), ctx.option_get(CNT_DECLINED)
                        g0 = [ctx.option_get(k) for k in SEG_KEYS]
                        k0 = [ctx.option_get(k) for k in PACKED_KEYS]
                        out, wall, cpu = timed((lambda: ctx.compress_batch_device(flat, sizes, 1, coder)) if how[1] else (lambda: ctx.compress_batch(blocks, 1, coder)))
                        segs[leg] = [ctx.option_get(k) - a for k, a in zip(SEG_KEYS, g0)]
                        packed_cnt[leg] = [ctx.option_get(k) - a for k, a in zip(PACKED_KEYS, k0)]
                        if leg == "batch_on_packed":
                            packed_fail = ctx.option_get(ctx.CNT_DC_LAST_FAIL)
                        kept[leg] = ctx.option_get(CNT_PASSES) - p0
                        declined[leg] = ctx.option_get(CNT_DECLINED) - d0
                    walls[leg].append(wall); cpus[leg].append(cpu)
                    same[leg] = same[leg] and digest(out) == want
            for leg in legs:
                w = np.array(walls[leg])
                print(json.dumps({"workload": name, "leg": leg, "blocks": len(sizes), "MB": round(mb, 2), "coder": coder,
                                  "ms": [round(x * 1e3, 1) for x in w], "median_MB_s": round(mb / float(np.median(w)), 1),
                                  "MB_s_min_max": [round(mb / float(w.max()), 1), round(mb / float(w.min()), 1)],
                                  "cpu_s_per_MB": round(float(np.mean(cpus[leg])) / mb, 4), "model_passes": kept[leg], "model_declined": declined[leg],
                                  **({"segments_reruns_host_blocks": segs[leg]} if args.segments or args.packed else {}),
                                  **({"packed_passes_void": packed_cnt[leg]} if args.packed else {}),
                                  "sha256_equals_pipe": bool(same[leg])}), flush=True)
            if args.packed and args.segments and name == "W1":
                # derived, not measured: W1's -e1 pass exceeds the pinned landing buffer as 16-bit entries and fits it packed.  What the
                # packed leg still leaves to the host was excluded for another reason (an undecided avg_rank flag, a rare exit), which its
                # reason mask names; BSCGPU_DC_FAIL_CAP (8) may not be among them
                h16, h13 = segs["batch_on"][2], segs["batch_on_packed"][2]
                print(json.dumps({"workload": name, "check": "segment host blocks through landing space", "16_bit": h16, "packed": h13,
                                  "reason_mask_of_the_packed_leg": packed_fail}), flush=True)
                assert h13 <= h16 and (h13 == 0 or (packed_fail & ctx.DC_FAIL_CAP) == 0), "a block of W1 left out for landing space in the packed leg"
            del dblocks
    finally:
        for p in pipes:
            p.close()
        for c in pctx:
            c.close()
        ctx.close()


def lzp_main(args):
    import hashlib
    import torch
    from libbsc_amd import GpuContext
    h, m = (int(x) for x in args.lzp.split(","))
    sorter, coder = args.sorter, args.coder
    ctx = GpuContext(0, max_n=(64 << 20) + 4096)

    def digest(out):
        d = hashlib.sha256()
        for o in out:
            d.update(o if isinstance(o, bytes) else str(o).encode())
        return d.hexdigest()

    try:
        for name in args.workloads.split(","):
            sizes, blocks = workload(name)
            mb = sum(sizes) / 1e6
            flat = torch.from_numpy(np.concatenate(blocks)).cuda()
            torch.cuda.synchronize()

            def leg(which):
                ctx.option_set(ctx.OPT_BATCH_DEVICE_LZP, 1 if which == "option_on" else 0)
                if which == "hbm":
                    return ctx.compress_batch_device(flat, sizes, sorter, coder, lzp_hash=h, lzp_min=m)
                return ctx.compress_batch(blocks, sorter, coder, lzp_hash=h, lzp_min=m)

            legs = ("host_lzp", "option_on", "hbm")
            want = digest(leg("host_lzp"))                                       # warm-up, and the outputs to compare with
            for which in legs[1:]:
                leg(which)
            walls, cpus, ok, passes = {k: [] for k in legs}, {k: [] for k in legs}, {k: True for k in legs}, {k: 0 for k in legs}
            for _ in range(args.reps):
                for which in legs:
                    p0 = ctx.option_get(ctx.CNT_BATCH_LZP_PASSES)
                    out, wall, cpu = timed(lambda: leg(which))
                    walls[which].append(wall); cpus[which].append(cpu)
                    passes[which] = ctx.option_get(ctx.CNT_BATCH_LZP_PASSES) - p0
                    ok[which] = ok[which] and digest(out) == want
            for which in legs:
                med = float(np.median(walls[which]))
                print(json.dumps({"workload": name, "lzp": [h, m], "coder": coder, **({"sorter": sorter} if sorter != 1 else {}), "leg": which,
                                  "blocks": len(sizes), "MB": round(mb, 2), "MB_s": round(mb / med, 1), "ms": round(med * 1e3, 1),
                                  "ms_all": [round(w * 1e3, 1) for w in walls[which]],
                                  "cpu_s_per_MB": round(float(np.median(cpus[which])) / mb, 4), "stage_passes": passes[which],
                                  "identical_to_host_lzp": bool(ok[which])}), flush=True)
            del flat
    finally:
        ctx.option_set(ctx.OPT_BATCH_DEVICE_LZP, 0)
        ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--workloads", default=None)
    ap.add_argument("--coder", type=int, default=1)
    ap.add_argument("--contexts", type=int, default=5)
    ap.add_argument("--depth", type=int, default=2)
    ap.add_argument("--sorter", type=int, default=1, help="1 = BWT (default), 3..8 = the sort transform of that order")
    ap.add_argument("--transform-only", action="store_true", help="with --sorter 3..8: only the st_batch against st_encode_device leg")
    ap.add_argument("--decode", action="store_true", help="the decode side: decompress_batch against the per-block paths")
    ap.add_argument("--configs", default="e1,e2,e1-lzp,e2-lzp")
    ap.add_argument("--profile-pass", action="store_true", help="with --decode: one decompress_batch per workload and config, nothing timed")
    ap.add_argument("--front", action="store_true", help="BSCGPU_OPT_BATCH_FRONT on against off, interleaved (BWT, --coder)")
    ap.add_argument("--front-only", action="store_true", help="with --front: the front-end stage alone against a loop of the single-block front end")
    ap.add_argument("--model", action="store_true", help="BSCGPU_OPT_BATCH_MODEL on against off, interleaved (BWT, -e1); with --coder 3: BSCGPU_OPT_BATCH_MODEL_FAST (-e0); with --coder 2: BSCGPU_OPT_BATCH_MODEL_ADAPTIVE (-e2)")
    ap.add_argument("--model-only", action="store_true", help="with --model: the model stage alone on one pass, per kernel class")
    ap.add_argument("--model-sweep", action="store_true", help="with --model: on against off on passes of 64 KiB .. 16 MiB (set BSC_BATCH_MODEL_MIN_PASS=0)")
    ap.add_argument("--segments", action="store_true", help="implies --model: legs model off / on / on + BSCGPU_OPT_BATCH_MODEL_SEGMENTS; with --model-only: the segmented stage")
    ap.add_argument("--packed", action="store_true", help="with --model (and --segments, --model-only): BSCGPU_OPT_BATCH_MODEL_PACKED on / off / model off, interleaved (-e1)")
    ap.add_argument("--segment-sweep", action="store_true", help="with --model: BSC_BATCH_MODEL_SEGMENT over the capacity / 8 .. the capacity, host input (set BSC_BATCH_MODEL_MIN_PASS=0 for one-pass workloads of the fast coder)")
    ap.add_argument("--lzp", default=None, help="H,M: the batch calls with LZP — host LZP, BSCGPU_OPT_BATCH_DEVICE_LZP on, input in HBM — interleaved")
    args = ap.parse_args()
    if args.lzp:
        args.workloads = args.workloads or "W1,W2,W3"
        return lzp_main(args)
    if args.segment_sweep:
        args.workloads = args.workloads or "W1,W2"
        args.segments = True
        return model_main(args)
    if args.model or args.model_only or args.model_sweep or args.segments:        # (--segments is a form of --model)
        args.workloads = args.workloads or "W1,W2,W3"
        return model_main(args)
    if args.front or args.front_only:
        args.workloads = args.workloads or "W1,W2,W3"
        return front_main(args)
    if args.decode:
        args.workloads = args.workloads or "W1,W2,W3,W4"
        return decode_main(args)
    args.workloads = args.workloads or "W1,W2,W3"
    import torch
    from libbsc_amd import GpuContext
    from libbsc_amd import _native as N
    from libbsc_amd import api
    from oracle.refbind import Ref, REF_SO
    refc = Ref() if os.path.exists(REF_SO) else None
    sorter, coder = args.sorter, args.coder
    ctx = GpuContext(0, max_n=(64 << 20) + 4096)
    pctx = [GpuContext(0, max_n=(1 << 20) + 4096) for _ in range(0 if args.transform_only else args.contexts)]
    pipes = [c.pipe(args.depth) for c in pctx]
    try:
        for name in args.workloads.split(","):
            sizes, blocks = workload(name)
            mb = sum(sizes) / 1e6
            if sorter != 1:
                st_transform_leg(ctx, name, sizes, blocks, sorter, max(args.reps, 5))
                if args.transform_only:
                    continue
            dblocks = [torch.from_numpy(b).cuda() for b in blocks]
            torch.cuda.synchronize()
            ref = run_pipe(pipes, dblocks, sizes, sorter, coder, args.depth)         # warm-up + the single-block outputs
            run_batch(ctx, blocks[:8], sorter, coder)
            flat = torch.from_numpy(np.concatenate(blocks)).cuda()
            legs = ["batch", "batch_device", "pipe", "dropin16"] + (["ref_cpu16"] if refc and sorter <= 6 else [])
            for leg in legs:
                best = None
                ok = True
                for _ in range(args.reps):
                    if leg == "batch":
                        out, wall, cpu = timed(lambda: run_batch(ctx, blocks, sorter, coder))
                    elif leg == "pipe":
                        out, wall, cpu = timed(lambda: run_pipe(pipes, dblocks, sizes, sorter, coder, args.depth))
                    elif leg == "batch_device":
                        out, wall, cpu = timed(lambda: ctx.compress_batch_device(flat, sizes, sorter, coder))
                    elif leg == "dropin16":
                        out, wall, cpu = timed(lambda: run_16(blocks, lambda b: bytes(api.bsc_compress(b, sorter, coder))))
                    else:
                        out, wall, cpu = timed(lambda: run_16(blocks, lambda b: refc.compress(b, sorter, coder, features=1)))
                    ok = ok and all(a == b for a, b in zip(out, ref))
                    if best is None or wall < best[0]:
                        best = (wall, cpu)
                print(json.dumps({"workload": name, **({"sorter": sorter} if sorter != 1 else {}),
                                  "leg": leg, "blocks": len(sizes), "MB": round(mb, 2), "MB_s": round(mb / best[0], 1),
                                  "ms": round(best[0] * 1e3, 1), "cpu_s_per_MB": round(best[1] / mb, 4),
                                  "identical_to_single_block_path": bool(ok)}), flush=True)
            if name == "W1" and sorter == 1:
                # one 64 MiB batched pass of W1's blocks: GPU time of the sort alone
                flat = torch.from_numpy(np.concatenate(blocks)).cuda()
                dL = torch.empty_like(flat)
                sz = np.array(sizes, np.int32)
                prim = np.zeros(len(sizes), np.int32)
                num = np.zeros(len(sizes), np.uint8)
                idx = np.zeros(16 * len(sizes), np.int32)
                torch.cuda.synchronize()
                ts = []
                for _ in range(max(args.reps, 3)):
                    t0 = time.perf_counter()
                    rc = ctx.L.bscgpu_bwt_batch_device(ctx.h, flat.data_ptr(), dL.data_ptr(), N.np_ptr(sz), len(sizes), N.np_ptr(prim),
                                                       N.np_ptr(num), N.np_ptr(idx))
                    ts.append(time.perf_counter() - t0)
                    assert rc == 0, rc
                one = torch.from_numpy(np.concatenate(blocks)).cuda()
                t1 = []
                for _ in range(max(args.reps, 3)):
                    t0 = time.perf_counter()
                    ctx.bwt_device(one, dL, one.numel(), None)
                    t1.append(time.perf_counter() - t0)
                print(json.dumps({"workload": "W1", "leg": "bwt_batch_device_64MiB_pass", "ms": round(min(ts) * 1e3, 2),
                                  "single_64MiB_block_bwt_ms": round(min(t1) * 1e3, 2)}), flush=True)
            del dblocks
    finally:
        for p in pipes:
            p.close()
        for c in pctx:
            c.close()
        ctx.close()


if __name__ == "__main__":
    main()
