"""What a decision costs the range coder on the GPU (csrc/device/rangecoder.hip): python tools/rc_device_bench.py [--mib 64] [--out FILE]

Input: the bench block's real probability streams (synth-text v1, seed 2, 64 MiB -> BWT on the GPU -> the device model's 16-bit
entries of its 8 sub-blocks, about 183 M decisions).  Legs: the 8 streams as they are (with their header and alphabet entries), then
the block cut into 64, 512 and 4096 pieces of equal length, each coded as a stream of its own, each at 64, 8 and 1 streams per
wavefront.  The kernel runs alone on the device; times are the HIP-event times around the kernel launch (the context's profiling
brackets, class "rc": the table upload before and the result copy behind it are outside); legs are interleaved, three repetitions
each, the median is reported.  In the same process bscgpu_rc_encode_host codes the same streams on one thread.  Every output of every
leg is compared with the host twin's.

One JSON line per (pieces, streams per wavefront) and one per host leg go to --out (default profiles/device_rc/rc_device_bench.jsonl);
a table goes to stdout: ns per decision per stream (kernel time / decisions of the longest stream: the serial chain's step), aggregate
decisions per second, wavefronts launched and how many of them the device holds at once."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from libbsc_amd import GpuContext, api, gpu

# wavefronts per CU the kernel's resources admit (23 040 B of LDS per wavefront at 64 streams; 8 per SIMD otherwise)
WAVES_PER_CU = {64: 7, 8: 32, 1: 32}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=64)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--pieces", default="8,64,512,4096")
    ap.add_argument("--out", default=os.path.join("profiles", "device_rc", "rc_device_bench.jsonl"))
    a = ap.parse_args()
    import torch
    n = a.mib << 20
    T = api.synth_text_v1(2, n)
    ctx = GpuContext(0, max_n=n + 4096)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    L, _, _ = ctx.bwt(T)
    ps, st, sz, poff, _ = ctx.qlfc_static_pstream(L)
    nb = len(st)
    prefixes = [gpu.rc_prefix(_first_seen(L[st[b]:st[b] + sz[b]]), sz[b], 1) for b in range(nb)]
    print(f"# synth-text v1 seed 2, {a.mib} MiB: {nb} sub-blocks, {ps.size} decisions, {cus} CUs", flush=True)
    d_body = torch.from_numpy(ps.view(np.int16)).cuda()
    legs = {}
    for pieces in [int(x) for x in a.pieces.split(",")]:
        streams, prefix = _cut(pieces, nb, poff, sz, prefixes)
        nout = max(s[4] + s[5] + 64 for s in streams)
        t0 = time.perf_counter()
        want_res, want = gpu.rc_encode_host(gpu.RC_STATIC16, ps, prefix, streams, out=np.zeros(nout, np.uint8))
        host_s = time.perf_counter() - t0
        assert min(want_res) > 0, "a stream of the bench block does not fit its region"
        legs[pieces] = dict(streams=streams, prefix=prefix, want_res=want_res, want=want, nout=nout, host_s=host_s,
                            dec=sum(s[1] + s[3] for s in streams), longest=max(s[1] + s[3] for s in streams), ms={64: [], 8: [], 1: []})
    d_out = torch.zeros(max(v["nout"] for v in legs.values()), dtype=torch.uint8, device="cuda")
    ctx.profile(True)
    for rep in range(a.reps + 1):                               # repetition 0 warms up (and is the one whose bytes are compared)
        for pieces, v in legs.items():
            for spw in (64, 8, 1):
                if rep == 0:
                    d_out.zero_()
                ctx.profile_reset()
                res = ctx.rc_encode_device(gpu.RC_STATIC16, d_body, v["prefix"], v["streams"], d_out, streams_per_wave=spw)
                k = ctx.profile_get()["rc"]
                assert k["launches"] == 1
                if rep == 0:
                    assert res == v["want_res"], (pieces, spw, "res differs from the host twin's")
                    got = d_out[:v["nout"]].cpu().numpy()
                    for s, r in zip(v["streams"], res):
                        assert np.array_equal(got[s[4]:s[4] + r], v["want"][s[4]:s[4] + r]), (pieces, spw, s)
                else:
                    v["ms"][spw].append(k["ms"])
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as fh:
        print(f"{'streams':>8} {'per wave':>8} {'kernel ms':>10} {'ns/decision/stream':>19} {'Mdecisions/s':>13} {'wavefronts':>10} {'resident':>9}")
        for pieces, v in legs.items():
            row = dict(leg="host", streams=pieces, decisions=v["dec"], seconds=v["host_s"], ns_per_decision=1e9 * v["host_s"] / v["dec"], threads=1)
            fh.write(json.dumps(row) + "\n")
            print(f"{pieces:>8} {'host':>8} {1e3 * v['host_s']:>10.1f} {row['ns_per_decision']:>19.2f} {v['dec'] / v['host_s'] / 1e6:>13.1f}")
            for spw in (64, 8, 1):
                ms = sorted(v["ms"][spw])
                med = ms[len(ms) // 2]
                waves = (pieces + spw - 1) // spw
                resident = min(waves, cus * WAVES_PER_CU[spw])
                row = dict(leg="device", streams=pieces, streams_per_wave=spw, decisions=v["dec"], longest_stream=v["longest"], ms=v["ms"][spw],
                           ms_median=med, ns_per_decision_per_stream=1e6 * med / v["longest"], decisions_per_s=v["dec"] / (1e-3 * med),
                           wavefronts=waves, wavefronts_resident=resident, outputs_equal_host=True)
                fh.write(json.dumps(row) + "\n")
                print(f"{pieces:>8} {spw:>8} {med:>10.2f} {row['ns_per_decision_per_stream']:>19.2f} {row['decisions_per_s'] / 1e6:>13.1f} {waves:>10} {resident:>9}", flush=True)
    ctx.close()


def _first_seen(sub):
    _, idx = np.unique(sub, return_index=True)
    return sub[np.sort(idx)]


def _cut(pieces, nb, poff, sz, prefixes):
    """`pieces` streams: the sub-block streams as they are (pieces == nb, with their prefixes), else every sub-block's stream cut into
    pieces / nb runs of equal length -> (stream tuples, prefix array)"""
    streams, off = [], 0
    if pieces == nb:
        prefix, at = np.concatenate(prefixes), 0
        for b in range(nb):
            streams.append((poff[b], poff[b + 1] - poff[b], at, prefixes[b].size, off, sz[b]))
            at += prefixes[b].size
            off += (sz[b] + 64 + 63) // 64 * 64
        return streams, prefix
    per = pieces // nb
    for b in range(nb):
        cnt = poff[b + 1] - poff[b]
        step = (cnt + per - 1) // per
        for k in range(per):
            lo = min(cnt, k * step)
            c = min(cnt, lo + step) - lo
            osz = c // 2 + 1024                                 # text: well under two bits per decision
            streams.append((poff[b] + lo, c, 0, 0, off, osz))
            off += (osz + 64 + 63) // 64 * 64
    return streams, np.zeros(0, np.uint32)


if __name__ == "__main__":
    main()
