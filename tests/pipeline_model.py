"""Numpy model of the device pipeline in libbsc_amd/csrc/device/bwt.hip and st.hip.

Each function mirrors ONE kernel (same inputs, same outputs, same index arithmetic) with vectorised
numpy, so the algorithm (tail-suffix ordering, head/rank semantics, doubling keys, emit indexing,
aux indexes, ST key layout) can be checked against the reference on a machine without a GPU.
It is test infrastructure; nothing in the product imports it.
"""
import numpy as np


def bwt_pack(T, n):
    tc = min(n, 7)
    Tp = np.concatenate([T, np.zeros(16, np.uint8)]).astype(np.uint64)
    i = np.arange(n, dtype=np.int64)
    key = np.zeros(n, np.uint64)
    for b in range(8):
        key |= Tp[i + b] << np.uint64(8 * (7 - b))
    tail = i + 8 > n
    slot = np.where(tail, n - 1 - i, i + tc)
    keys = np.empty(n, np.uint64); vals = np.empty(n, np.uint32)
    keys[slot] = key; vals[slot] = i
    return keys, vals


def radix_sort(keys, vals, passes):
    """stable LSD passes [(shift, bits)]"""
    for shift, bits in passes:
        d = (keys >> np.uint64(shift)) & np.uint64((1 << bits) - 1)
        o = np.argsort(d, kind="stable")
        keys = keys[o]
        if vals is not None:
            vals = vals[o]
    return keys, vals


def seg(keys, sa, cpos_in, m, n, initial):
    """returns flags-derived (rank per element, unsorted mask)"""
    head = np.ones(m + 1, bool)
    if m > 1:
        head[1:m] = keys[1:] != keys[:-1]
        if initial:
            tail_lo = n - 7 if n >= 8 else 0
            t = sa >= tail_lo
            head[1:m] |= t[1:] | t[:-1]
    uns = ~(head[:m] & head[1:m + 1])
    pos = np.arange(m, dtype=np.int64) if initial else cpos_in.astype(np.int64)
    hp = np.where(head[:m], pos + 1, 0)
    rank = np.maximum.accumulate(hp) - 1
    return pos, rank.astype(np.uint32), uns


def seg_long_counts(pos, rank, uns, limit=1024):
    """What seg_apply counts for free (bwt.hip, DS_NLONG / DS_EXCESS): an unsorted record knows its SA slot (pos) and the slot of its
    group's head (rank), and members of a group are contiguous in SA — the record `limit` places behind its head proves a group of more
    than `limit` records (one such record per long group), every record at or beyond that distance counts as excess."""
    d = pos[uns].astype(np.int64) - rank[uns].astype(np.int64)
    return int(np.count_nonzero(d == limit)), int(np.count_nonzero(d >= limit))


def bit_length(x):
    return int(x).bit_length()


def key_geometry(K, n, batch_count=0):
    """The first sort's key layout as bwt_key_plan (libbsc_amd/csrc/device/bwt_plan.h; test_bwt_plan_host.py holds the two together) derives it from the alphabet size K of the text (of the whole pass for a batch), the
    length n and the number of blocks of a batched pass (0: a single block):
      cb          bits per character: the smallest with 2^cb >= K, at least 4; a batch codes 1..K (0 = past the block's end): K + 1
      w           characters per key: 64 / cb; a batch keeps batch_bb bits for the block field on top, at most 16 characters
      low_shift   lowest key bit in use; passes: the (shift, bits) digit passes, 8 bits each, the topmost with what is left
      ta          characters per round on text keys (they need 4 bits beside the characters): w, or w - 1 where w cb + 4 > 64
      pred_shift  where the value carries the code of the character in front of the suffix: idx_bits while idx_bits + cb <= 32 on a single
                  block, else 0 (L is then gathered from the text)
      batch_bb    bits of the block field"""
    bt = batch_count > 0
    batch_bb = bit_length(batch_count - 1) if bt else 0
    kk = K + (1 if bt else 0)
    cb = max(4, bit_length(kk - 1), 1)
    w = min(16, (64 - batch_bb) // cb) if bt else 64 // cb
    low_shift = 64 - cb * w - batch_bb
    passes = [(s, min(8, 64 - s)) for s in range(low_shift, 64, 8)]
    ta = w if cb * w + 4 <= 64 else w - 1
    idx_bits = bit_length(n - 1)
    pred_shift = idx_bits if (not bt and idx_bits >= 1 and idx_bits + cb <= 32) else 0
    return dict(cb=cb, w=w, low_shift=low_shift, passes=passes, ta=ta, pred_shift=pred_shift, batch_bb=batch_bb)


def bwt_model(T, r=None):
    """-> (L, primary (1-based), I array like libsais_bwt_aux), rounds"""
    T = np.asarray(T, np.uint8)
    n = T.size
    keys, vals = bwt_pack(T, n)
    keys, vals = radix_sort(keys, vals, [(8 * p, 8) for p in range(8)])
    SA = np.zeros(n, np.uint32); ISA = np.zeros(n, np.uint32)
    pos, rank, uns = seg(keys, vals, None, n, n, True)
    SA[pos] = vals; ISA[vals] = rank
    cpos, csa, cgrp = pos[uns].astype(np.uint32), vals[uns], rank[uns]
    h = 8; rounds = 0
    lo_bits, hi_bits = bit_length(n), bit_length(n - 1)
    while cpos.size:
        rounds += 1
        assert rounds <= 40
        p = csa.astype(np.int64) + h
        nxt = np.where(p < n, ISA[np.minimum(p, n - 1)].astype(np.uint64) + 1, 0).astype(np.uint64)
        k = (cgrp.astype(np.uint64) << np.uint64(32)) | nxt
        passes = [(s, min(8, lo_bits - s)) for s in range(0, lo_bits, 8)] + [(32 + s, min(8, hi_bits - s)) for s in range(0, hi_bits, 8)]
        ks, vs = radix_sort(k, csa, passes)
        pos, rank, uns = seg(ks, vs, cpos, cpos.size, n, False)
        SA[pos] = vs; ISA[vs] = rank
        cpos, csa, cgrp = pos[uns].astype(np.uint32), vs[uns], rank[uns]
        h *= 2
    # emit
    pidx = int(ISA[0])
    L = np.empty(n, np.uint8)
    o = np.arange(n, dtype=np.int64)
    j = np.where(o <= pidx, o - 1, o)
    j[0] = 0
    src = SA[j].astype(np.int64) - 1
    L[:] = T[np.maximum(src, 0)]
    L[0] = T[n - 1]
    I = None
    if r:
        cnt = (n - 1) // r + 1
        I = ISA[np.arange(cnt, dtype=np.int64) * r].astype(np.int64) + 1
    return L, pidx + 1, I, rounds, SA


def st_model(T, k):
    T = np.asarray(T, np.uint8)
    n = T.size
    i = np.arange(n, dtype=np.int64)
    Tc = T.astype(np.uint64)
    if k < 8:
        key = Tc[(i - 1) % n] << np.uint64(56)
        for b in range(7):
            key |= Tc[(i + b) % n] << np.uint64(8 * (6 - b))
        ks, _ = radix_sort(key, None, [((7 - k) * 8 + 8 * p, 8) for p in range(k)])
        out = (ks >> np.uint64(56)).astype(np.uint8)
        index = int(np.flatnonzero(ks == key[0])[0])
    else:
        key = np.zeros(n, np.uint64)
        for b in range(8):
            key |= Tc[(i + b) % n] << np.uint64(8 * (7 - b))
        val = T[(i - 1) % n].astype(np.uint32) | np.where(i == 0, 0x100, 0).astype(np.uint32)
        ks, vs = radix_sort(key, val, [(8 * p, 8) for p in range(8)])
        out = (vs & 0xff).astype(np.uint8)
        index = int(np.flatnonzero(vs & 0x100)[0])
    return out, index


# ---- a pass in model segments (devcoder.hip: devcoder_pstream_segments) --------------------------------------------------------------
FAIL_AVG, FAIL_CAP = 2, 8                                       # include/bscgpu.h: BSCGPU_DC_FAIL_*


def segment_plan(dec, und, blk_sub, dcap, target):
    """bscgpu_model_segment_plan -> (segments, the segment of every block or -1)"""
    limit = target if 0 < target < dcap else dcap
    nseg, is_open, filled, seg_of = 0, False, 0, []
    for b in range(len(blk_sub) - 1):
        s0, s1 = blk_sub[b], blk_sub[b + 1]
        if s0 == s1:
            seg_of.append(-1)
            continue
        d = sum(dec[s0:s1])
        if any(und[s0:s1]) or d > dcap:
            seg_of.append(-1)
            is_open = False
            continue
        if not is_open or filled + d > limit:
            nseg, is_open, filled = nseg + 1, True, 0
        filled += d
        seg_of.append(nseg - 1)
    return nseg, seg_of


def segment_schedule(dec, und, blk_sub, dcap, target, cap, per_segment_fit, packed, model=lambda b0, b1: (0, False, False)):
    """What the host side of a pass in model segments does, written down from the driver as it stood when the whole of it was one
    function (the work stack, the room rule, the cut, the re-run budget, poff / pbase) — the reference tools/dc_segment_probe.cpp's
    output is held against.  dec / und: decisions and undecided flags per sub-block; model(b0, b1) stands for the device:
    -> (reason mask the range declines with or 0, its packed form is void, its packed layout is 64 fields longer than the plan's).
    -> dict with the probe's keys."""
    count, nsub = len(blk_sub) - 1, len(dec)
    member = lambda b: blk_sub[b + 1] > blk_sub[b]
    blk_dec = lambda b: sum(dec[blk_sub[b]:blk_sub[b + 1]])
    span_need = lambda s0, s1: sum((d + 63) // 64 * 104 if packed else d for d in dec[s0:s1])
    nseg, seg_of = segment_plan(dec, und, blk_sub, dcap, target)
    state, todo, planned = [0] * count, [], 0
    for b in range(count - 1, -1, -1):
        if not member(b):
            continue
        if seg_of[b] < 0:
            state[b] = FAIL_AVG if any(und[blk_sub[b]:blk_sub[b + 1]]) else FAIL_CAP
            continue
        planned += span_need(blk_sub[b], blk_sub[b + 1])
        if todo and seg_of[todo[-1][0]] == seg_of[b]:
            todo[-1][0] = b
        else:
            todo.append([b, b + 1])
    copy_all = per_segment_fit or planned <= cap
    nblk = sum(member(b) for b in range(count))
    lg = 0
    while (1 << lg) < nblk:
        lg += 1
    rerun_max = 2 * lg + 2
    out = dict(need=planned, copy_all=copy_all, excluded=list(state), ranges=[], error=False)
    reruns = kept = kept_packed = kept_void = base = base_dec = filled = 0
    poff, pbase = [0] * (nsub + 1), [0] * (nsub + 1)

    def fill_to(s):
        nonlocal filled
        while filled < s:
            poff[filled + 1], pbase[filled + 1] = poff[filled], pbase[filled]
            filled += 1

    def give_up(b0, b1, why):
        for b in range(b0, b1):
            if member(b):
                state[b] = why

    while todo:
        b0, b1 = todo.pop()
        s0, s1 = blk_sub[b0], blk_sub[b1]
        expect, need = sum(dec[s0:s1]), span_need(s0, s1)
        row = [b0, b1, s0, s1, expect, need]
        if per_segment_fit and base + need > cap:
            give_up(b0, b1, FAIL_CAP)
            out["ranges"].append(row + ["nofit", FAIL_CAP])
            continue
        why, void, skew = model(b0, b1)
        if why:
            members = sum(member(b) for b in range(b0, b1))
            if members < 2 or reruns + 2 > rerun_max:
                give_up(b0, b1, why)
                out["ranges"].append(row + ["gave_up", why])
                continue
            cut, acc, best, seen = -1, 0, 0, 0
            for b in range(b0, b1):
                if not member(b):
                    continue
                acc += blk_dec(b)
                seen += 1
                if seen == members:
                    break
                dist = abs(acc * 2 - expect)
                if cut < 0 or dist < best:
                    cut, best = b + 1, dist
            todo.append([cut, b1])
            todo.append([b0, cut])
            reruns += 2
            out["ranges"].append(row + ["split", why])
            continue
        D = expect
        fill_to(s0)
        for s in range(s0, s1):
            poff[s + 1] = poff[s] + dec[s]
        filled = s1
        is_packed = packed and not void
        if packed:
            for s in range(s0, s1):
                pbase[s + 1] = pbase[s] + (dec[s] + 63) // 64 * 64
            if is_packed and skew:
                pbase[s1] += 64
            if (pbase[s1] - pbase[s0]) // 8 * 13 != need:
                out["ranges"].append(row + ["layout", -1])
                out["error"] = True
                return out
            kept_packed, kept_void = kept_packed + is_packed, kept_void + (not is_packed)
        out["ranges"].append(row + ["void" if packed and not is_packed else "kept", base])
        base += need if packed else D
        base_dec += D
        kept += 1
    fill_to(nsub)
    out.update(blk_state=state, poff=poff, planned=nseg, kept=kept, reruns=reruns, host_blocks=sum(x != 0 for x in state), packed=kept_packed,
               void=kept_void, fail=int(np.bitwise_or.reduce(np.array(state + [0]))), decisions=base_dec)
    if packed:
        out["pbase"] = pbase
    return out


def segment_counters(dec, blk_sub, dcap, target=0, decline=(), why=4, und=None):
    """(segments kept, re-runs, blocks left to the host) of a 16-bit pass whose landing buffer holds everything, when exactly the ranges
    that hold a block of `decline` decline (reason mask `why`)"""
    dec, blk_sub = [int(x) for x in dec], [int(x) for x in blk_sub]
    r = segment_schedule(dec, [0] * len(dec) if und is None else [int(x) for x in und], blk_sub, dcap, target, sum(dec), False, False,
                         lambda b0, b1: (why if any(b0 <= b < b1 for b in decline) else 0, False, False))
    return r["kept"], r["reruns"], r["host_blocks"]


# ---- the batched-compress driver (block.cpp: compress_batch_impl) ---------------------------------------------------------------------
BATCH_MAX_N, BATCH_MAX_BLOCKS, HEADER_SIZE, NOT_SUPPORTED = 1 << 20, 4096, 28, -4      # include/bscgpu.h, include/libbsc.h
BATCH_MIN_PASS, BATCH_FAST_MIN_PASS = 16 << 20, 32 << 20                               # block.cpp: BATCH_MODEL_*MIN_PASS_DEFAULT
CODER_STATIC, CODER_FAST = 1, 3


def aux_rate(n):
    """the largest power of two <= n / 8, at least 1 (block.cpp: aux_rate)"""
    m = n // 8
    return 1 << (m.bit_length() - 1) if m > 0 else 1


def batch_plan(sizes, sorter, cap):
    """bscgpu_batch_plan / bscgpu_st_batch_plan (sorter 1: BWT, 3..8: ST) -> (passes, pass_of)"""
    passes, cur, span, filled, pass_of = 0, -1, 0, 0, []
    for n in sizes:
        if not (sorter in (1, 3, 4, 5, 6, 7, 8) and 0 < n < BATCH_MAX_N and n <= cap):
            pass_of.append(-1)
            if n > 0:
                cur = -1
            elif cur >= 0:
                span += 1
            continue
        if cur < 0 or filled + n > cap or span + 1 > BATCH_MAX_BLOCKS:
            cur, filled, span = passes, 0, 0
            passes += 1
        pass_of.append(cur)
        filled += n
        span += 1
    return passes, pass_of


def batch_call(sizes, sorter, coder, cap, dev, lz, opts, facts, entries, min_pass=None, target=0, front_host=True, model_host=True):
    """What compress_batch_impl decides for one call, written down from the function as it stood when all of it was one body — the
    reference tools/batch_pass_probe.cpp's output is held against.
      sizes, sorter, coder, cap (the context's max_n), dev (input in HBM); lz[b]: what LZP left of block b (its size where LZP is off
      or gave up); opts: the context's option values front, model, fast, segments, packed, device_rc; min_pass: the environment's
      override of the smallest modelled pass or None; target: the segment target; front_host / model_host: the pinned buffers are to
      be had; entries: 16-bit entries a pinned stream buffer holds
      facts[p]: what the device says of pass p (a pass that never asks takes defaults): nsub, mrc, D, pk, pbytes, blk_state
    -> dict with the probe's keys."""
    st = sorter != 1
    npass, pass_of = batch_plan(sizes, sorter, cap)
    front = npass > 0 and opts["front"] != 0 and front_host
    fast_model = front and opts["fast"] != 0 and coder == CODER_FAST
    model = fast_model or (front and opts["model"] != 0 and coder == CODER_STATIC)
    model_min_pass = min_pass if min_pass is not None else BATCH_FAST_MIN_PASS if fast_model else BATCH_MIN_PASS
    segments = model and opts["segments"] != 0 and opts["device_rc"] == 0
    segment_target = target if segments else 0
    packed_route = model and not fast_model and opts["packed"] != 0
    out = dict(npass=npass, pass_of=pass_of, route=[int(front), int(model), int(fast_model), int(segments), int(packed_route),
                                                     int(model and opts["device_rc"] != 0)],
               min_pass=model_min_pass, target=segment_target, passes=[], error=0)
    single = [int(p < 0) for p in pass_of]
    count, b, p = len(sizes), 0, 0
    while b < count:
        if pass_of[b] < 0:
            b += 1
            continue
        e = b
        for q in range(b, count):
            if not (pass_of[q] == pass_of[b] or (pass_of[q] < 0 and sizes[q] == 0)):
                break
            if pass_of[q] == pass_of[b]:
                e = q + 1
        cls = []
        for q in range(b, e):
            n = sizes[q]
            if pass_of[q] < 0:
                cls.append("empty")
            elif n <= HEADER_SIZE:
                cls.append("rides" if dev else "stored")
            elif not st and aux_rate(lz[q]) < 2:
                cls.append("single")
            else:
                cls.append("sorted")
        psz, prate, at, pos = [], [], [], 0
        for i, q in enumerate(range(b, e)):
            srt = cls[i] == "sorted"
            at.append(pos)
            prate.append((0 if st else aux_rate(lz[q])) if srt else -1)
            if dev:
                psz.append(sizes[q])
                pos += sizes[q]
            else:
                psz.append(lz[q] if srt else 0)
                pos += lz[q] if srt else 0
        cnt = dict(front=0, l=0, model=0, declined=0, fast=0, fast_declined=0, packed=0, void=0, device_rc=0)
        row = dict(b=b, e=e, classes=cls, psz=psz, prate=prate, at=at, pos=pos, step="none", kept=0, counters=cnt)
        out["passes"].append(row)
        f = facts.get(p, {})
        nsub, mrc = f.get("nsub", 0), f.get("mrc", 0)
        ok, no = ("fast", "fast_declined") if fast_model else ("model", "declined")
        error = 0
        if pos > 0 and not front:
            row["step"] = "l_down"
            cnt["l"] += 1
        elif pos > 0:
            cnt["front"] += 1
            if segments and nsub > 0 and pos >= model_min_pass and model_host:
                row["step"] = "segments"
                if mrc < 0 and mrc != NOT_SUPPORTED:
                    error = mrc
                else:
                    state = f.get("blk_state", [0] * (e - b))
                    kept = mrc >= 0 and any(psz[i] > 0 and state[i] == 0 for i in range(e - b))
                    row["kept"] = int(kept)
                    cnt[ok if kept else no] += 1
            elif model and nsub > 0 and pos >= model_min_pass and model_host:
                row["step"] = "whole"
                pk = f.get("pk", 0) if packed_route else 0
                if mrc == NOT_SUPPORTED:
                    cnt[no] += 1
                elif mrc < 0:
                    error = mrc
                elif (f.get("pbytes", 0) + 8 <= entries * 2) if pk else (f.get("D", 0) <= entries):
                    row["kept"] = 1
                    if packed_route:
                        cnt["packed" if pk else "void"] += 1
                    if opts["device_rc"] != 0:
                        cnt["device_rc"] += 1
                    cnt[ok] += 1
        if error:
            out["error"] = error
            break
        # what every sorted block is coded from (code_sorted_block's arguments as code_block chose them)
        state = f.get("blk_state", [0] * (e - b)) if row["step"] == "segments" else [0] * (e - b)
        pk = f.get("pk", 0) if packed_route else 0
        coded = row["step"] == "whole" and row["kept"] and opts["device_rc"] != 0
        stream = row["step"] == "segments" or (row["step"] == "whole" and row["kept"] and not coded)
        is_packed = packed_route if row["step"] == "segments" else bool(row["kept"] and pk)
        row["sources"] = ["" if cls[i] != "sorted" else "l" if not front else "device_rc" if coded else "runs" if not stream or state[i]
                          else "fast" if coder == CODER_FAST else "ps13" if is_packed else "ps16" for i in range(e - b)]
        for i, q in enumerate(range(b, e)):
            if cls[i] == "single":
                single[q] = 1
        b, p = e, p + 1
    piped = lambda q: pass_of[q] < 0 and sizes[q] <= cap and (dev or sizes[q] > HEADER_SIZE)
    out["leftover"] = [] if out["error"] else ["none" if not single[q] else "pipe" if piped(q) else "one_by_one" for q in range(count)]
    return out


# ---- the block format (libbsc_amd/csrc/host/container.h), restated from the reference's layout --------------------------------------
# A block is a 28-byte header (seven little-endian words, the last the Adler-32 of the six before it) and a body: the data itself
# (mode 0), or the coder's payload, the aux indexes and their count byte.  A payload of more than one sub-block is a count byte, a
# table of {raw size, coded size} and the sub-blocks back to back (coded size == raw size: kept raw).
NOT_COMPRESSIBLE, DATA_CORRUPT = -3, -6


def _adler(b):
    import zlib
    return zlib.adler32(bytes(b)) & 0xffffffff


def _words(*v):
    import struct
    return b"".join(struct.pack("<I", x & 0xffffffff) for x in v)


def mode_pack(sorter, coder, lzp_hash, lzp_min):
    return sorter | coder << 5 | lzp_min << 8 | lzp_hash << 16


def mode_unpack(mode):
    """-> [sorter, coder, lzp_hash, lzp_min]"""
    return [mode & 31, mode >> 5 & 7, mode >> 16 & 255, mode >> 8 & 255]


def block_header(block_size, data_size, mode, index, adler_data, adler_body):
    six = _words(block_size, data_size, mode, index, adler_data, adler_body)
    return six + _words(_adler(six))


def stored_block(data):
    return block_header(len(data) + HEADER_SIZE, len(data), 0, 0, _adler(data), _adler(data)) + bytes(data)


def coded_block(n_orig, payload, mode, index, indexes, adler_data, coded=None):
    """coded: what the coder returned where that is not len(payload) (a negative code) -> the block, or NOT_COMPRESSIBLE: store it"""
    coded = len(payload) if coded is None else coded
    if coded < 0 or coded + 1 + 4 * len(indexes) >= n_orig:
        return NOT_COMPRESSIBLE
    body = bytes(payload[:coded]) + _words(*indexes) + bytes([len(indexes)])
    return block_header(len(body) + HEADER_SIZE, n_orig, mode, index, adler_data, _adler(body)) + body


def coded_payload(block):
    """the decoders' view of a coded block whose header has passed -> dict(num, size, data, indexes: offsets) or DATA_CORRUPT"""
    import struct
    bs, adler_body = struct.unpack_from("<i", block, 0)[0], struct.unpack_from("<I", block, 20)[0]
    if bs < HEADER_SIZE + 2 or _adler(block[HEADER_SIZE:bs]) != adler_body:
        return DATA_CORRUPT
    num = block[bs - 1]
    size = bs - HEADER_SIZE - 1 - 4 * num
    return DATA_CORRUPT if size < 1 else dict(num=num, size=size, data=HEADER_SIZE, indexes=HEADER_SIZE + size)


def _sub_bytes(b, raw, k):
    return bytes([(0xA0 if raw else 0xC0) + b]) * k        # what tools/container_probe.cpp's stand-in coder writes


def frame_parallel(n, size, res):
    """every sub-block coded on its own with a budget of its own size (res[b] == size[b]: kept raw) -> the payload or NOT_COMPRESSIBLE"""
    if 1 + 8 * len(size) + sum(res) >= n:
        return NOT_COMPRESSIBLE
    table = b"".join(_words(s, r) for s, r in zip(size, res))
    return bytes([len(size)]) + table + b"".join(_sub_bytes(b, r == s, r) for b, (s, r) in enumerate(zip(size, res)))


def frame_serial(n, size, c):
    """one sub-block after the other with the budget min(size[b], n - bytes so far); the stand-in coder needs c[b] bytes and gives up
    without room for them or where c[b] >= size[b] -> (the payload or NOT_COMPRESSIBLE, the budgets handed out)"""
    optr, table, subs, rooms = 1 + 8 * len(size), b"", b"", []
    for b, (s, k) in enumerate(zip(size, c)):
        room = min(s, n - optr)
        rooms.append(room)
        raw = k >= s or k > room
        if raw:
            if optr + s >= n:
                return NOT_COMPRESSIBLE, rooms
            k = s
        table += _words(s, k)
        subs += _sub_bytes(b, raw, k)
        optr += k
    return bytes([len(size)]) + table + subs, rooms


def serial_verdict(n, size, res):
    """sub-blocks coded on their own, under the serial rule: 'exact' (the serial coder's payload is frame_parallel's table and
    sub-blocks, whatever their total), 'incompressible' (its answer is NOT_COMPRESSIBLE), 'not_exact' (a budget was smaller: unknown)"""
    optr = 1 + 8 * len(size)
    for s, r in zip(size, res):
        if n - optr < s:
            return "not_exact"
        if r == s and optr + s >= n:
            return "incompressible"
        optr += r
    return "exact"


def subtable_parse(data, in_size, max_out):
    """-> (nb or DATA_CORRUPT, [[isz, osz, iptr, optr] of the sub-blocks up to the first bad one], 0 or DATA_CORRUPT); nb == 1 has no table"""
    import struct
    if in_size < 1:
        return DATA_CORRUPT, [], DATA_CORRUPT
    nb = data[0]
    if nb == 1:
        return 1, [], 0
    if nb < 1 or nb > 8 or in_size < 1 + 8 * nb:
        return DATA_CORRUPT, [], DATA_CORRUPT
    ip, op, subs = 1 + 8 * nb, 0, []
    for b in range(nb):
        osz, isz = struct.unpack_from("<ii", data, 1 + 8 * b)
        if osz < 0 or isz < 0 or ip + isz > in_size or op + osz > max_out:
            return nb, subs, DATA_CORRUPT
        subs.append([isz, osz, ip, op])
        ip, op = ip + isz, op + osz
    return nb, subs, 0
