"""Per-GPU context: thin object wrapper over the bscgpu_* C ABI (include/bscgpu.h)."""
import ctypes as C

import numpy as np

from . import _native as N


class GpuError(RuntimeError):
    def __init__(self, code, msg=""):
        super().__init__(f"bscgpu error {code}: {msg}")
        self.code = code


def _dptr(t):
    """device pointer of a torch CUDA tensor (or a raw int).  The context runs on its own non-blocking HIP stream,
    so pending torch work that produces the tensor (an async clone / copy on torch's stream) must have finished:
    synchronise torch's current stream before handing the pointer over."""
    if isinstance(t, int):
        return C.c_void_p(t)
    import torch
    torch.cuda.current_stream(t.device).synchronize()
    return C.c_void_p(t.data_ptr())


class GpuContext:
    """One context per GPU (mirrors libcubwt's device storage handle, libcubwt.cuh:60-71)."""

    def __init__(self, device=0, max_n=64 << 20):
        self.L = N.lib()
        h = C.c_void_p()
        rc = self.L.bscgpu_create(C.byref(h), int(device), int(max_n))
        if rc != 0:
            raise GpuError(rc, "bscgpu_create failed (no GPU / out of memory?)")
        self.h = h
        self.device = device
        self.max_n = max_n

    def close(self):
        if getattr(self, "h", None):
            self.L.bscgpu_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc < 0:
            raise GpuError(rc, (self.L.bscgpu_last_error(self.h) or b"").decode())
        return rc

    @property
    def arena_bytes(self):
        return int(self.L.bscgpu_arena_bytes(self.h))

    @property
    def model_arena_bytes(self):
        """bscgpu_model_arena_bytes: the device model's own arena (0 before the first block or pass that takes the device model)"""
        f = self.L.bscgpu_model_arena_bytes
        f.restype = C.c_int64
        f.argtypes = [C.c_void_p]
        return int(f(self.h))

    # ---- host-pointer entry points (shape of the reference hooks) -----------------------------
    def bwt(self, data, aux_rate=None):
        """-> (L np.uint8[n], primary index, I list or None).  libcubwt_bwt / libcubwt_bwt_aux."""
        T = np.ascontiguousarray(np.frombuffer(bytes(data), np.uint8) if not isinstance(data, np.ndarray) else data)
        n = T.size
        Lout = np.empty(max(n, 1), np.uint8)
        if aux_rate:
            cnt = (n - 1) // aux_rate + 1 if n > 0 else 0
            I = (C.c_uint32 * max(cnt, 1))()
            rc = self.L.bscgpu_bwt_aux(self.h, N.np_ptr(T), N.np_ptr(Lout), n, aux_rate, I)
            self._check(rc)
            return Lout[:n], int(I[0]) if cnt else 0, [int(I[t]) for t in range(cnt)]
        rc = self._check(self.L.bscgpu_bwt(self.h, N.np_ptr(T), N.np_ptr(Lout), n))
        return Lout[:n], int(rc), None

    def unbwt(self, L, index, out=None):
        """bscgpu_unbwt: inverse BWT of L (np.uint8) with the 1-based primary index -> (text np.uint8, rc); out: the caller's
        buffer (contiguous uint8, at least len(L) bytes), left as it is where rc is not 0"""
        a = np.ascontiguousarray(L, dtype=np.uint8)
        if out is None:
            out = np.empty(max(a.size, 1), np.uint8)
        assert out.dtype == np.uint8 and out.flags.c_contiguous and out.size >= a.size
        f = self.L.bscgpu_unbwt
        f.restype = C.c_int
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64]
        rc = f(self.h, N.np_ptr(a), N.np_ptr(out), a.size, int(index))
        return out[:a.size], int(rc)

    def st_encode(self, data, k):
        T = np.array(np.frombuffer(bytes(data), np.uint8) if not isinstance(data, np.ndarray) else data, copy=True)
        rc = self._check(self.L.bscgpu_st_encode(self.h, N.np_ptr(T), T.size, k))
        return T, int(rc)

    # ---- device-pointer entry points -------------------------------------------------------
    def bwt_device(self, dT, dL, n, aux_rate=None):
        if aux_rate:
            cnt = (n - 1) // aux_rate + 1
            I = (C.c_uint32 * cnt)()
            rc = self._check(self.L.bscgpu_bwt_device(self.h, _dptr(dT), _dptr(dL), n, aux_rate, I))
            return int(rc), [int(I[t]) for t in range(cnt)]
        rc = self._check(self.L.bscgpu_bwt_device(self.h, _dptr(dT), _dptr(dL), n, 0, None))
        return int(rc), None

    def bwt_first_sort_device(self, dT, n):
        """bscgpu_bwt_first_sort_device: the first sort of bwt_device's transform of this block alone -> (keys u64[n], vals u32[n])"""
        import torch
        keys = torch.empty(n, dtype=torch.int64, device=dT.device)
        vals = torch.empty(n, dtype=torch.int32, device=dT.device)
        self._check(self.L.bscgpu_bwt_first_sort_device(self.h, _dptr(dT), n, _dptr(keys), _dptr(vals)))
        return keys.cpu().numpy().view(np.uint64), vals.cpu().numpy().view(np.uint32)

    def st_encode_device(self, dT, dOut, n, k):
        return int(self._check(self.L.bscgpu_st_encode_device(self.h, _dptr(dT), _dptr(dOut), n, k)))

    def adler32_device(self, dT, n):
        out = C.c_uint32(0)
        self._check(self.L.bscgpu_adler32_device(self.h, _dptr(dT), n, C.byref(out)))
        return int(out.value)

    def radix_sort(self, keys, keys_alt, vals, vals_alt, n, begin_bit=0, end_bit=64):
        """torch int64 / int32 CUDA tensors (bit patterns are treated as unsigned). Returns (keys, vals) tensors
        that hold the result."""
        alt = C.c_int(0)
        self._check(self.L.bscgpu_radix_sort_u64(self.h, _dptr(keys), _dptr(keys_alt),
                                                 _dptr(vals) if vals is not None else None,
                                                 _dptr(vals_alt) if vals_alt is not None else None,
                                                 n, begin_bit, end_bit, C.byref(alt)))
        return (keys_alt, vals_alt) if alt.value else (keys, vals)

    def qlfc_static_pstream(self, L, debug=False):
        """bscgpu_qlfc_static_pstream: (entries u16[D], sub_start, sub_size, poff[nb+1], dbg [3,D] or None); raises GpuError
        with code -4 when the block has to take the host model."""
        a = np.ascontiguousarray(L, dtype=np.uint8)
        cap = 16 * a.size + 65536               # decisions: ~3 per byte on text, ~9 on random bytes
        out = np.empty(cap, np.uint16)
        dbg = np.empty((3, cap), np.uint16) if debug else None
        nb = C.c_int(0); st = (C.c_int * 8)(); sz = (C.c_int * 8)(); poff = (C.c_int64 * 9)()
        f = self.L.bscgpu_qlfc_static_pstream
        f.restype = C.c_int64
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.POINTER(C.c_int), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        D = f(self.h, N.np_ptr(a), a.size, out.ctypes.data, cap, C.byref(nb), st, sz, poff, dbg.ctypes.data if debug else None)
        self._check(D)
        if D > cap:
            raise GpuError(-2, f"{D} decisions exceed the buffer of {cap}")
        k = nb.value
        return out[:D], list(st[:k]), list(sz[:k]), list(poff[:k + 1]), (dbg[:, :D] if debug else None)

    def qlfc_static_pstream_packed(self, L):
        """bscgpu_qlfc_static_pstream_packed: (fields u16[D] unpacked from the 13-bit stream, sub_start, sub_size, poff, pbase, packed bytes);
        raises GpuError -4 when the block takes the host model or the packed form was not produced."""
        a = np.ascontiguousarray(L, dtype=np.uint8)
        cap = 26 * a.size + 65536 + 8 * 104
        out = np.zeros(cap + 8, np.uint8)
        nb = C.c_int(0); st = (C.c_int * 8)(); sz = (C.c_int * 8)(); poff = (C.c_int64 * 9)(); pbase = (C.c_int64 * 9)()
        f = self.L.bscgpu_qlfc_static_pstream_packed
        f.restype = C.c_int64
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.POINTER(C.c_int), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        D = f(self.h, N.np_ptr(a), a.size, out.ctypes.data, cap, C.byref(nb), st, sz, poff, pbase)
        self._check(D)
        k = nb.value
        po, pb = list(poff[:k + 1]), list(pbase[:k + 1])
        nbytes = pb[k] // 8 * 13
        if nbytes > cap:
            raise GpuError(-2, f"{nbytes} bytes exceed the buffer of {cap}")
        fields = np.empty(D, np.uint16)
        for b in range(k):                                         # field i of sub-block b: bits [13 i, 13 i + 13) from byte pbase[b] / 8 * 13 on
            cnt = po[b + 1] - po[b]
            base = pb[b] // 8 * 13
            bit = np.arange(cnt, dtype=np.int64) * 13
            byte = base + (bit >> 3)
            w = out[byte].astype(np.uint32) | (out[byte + 1].astype(np.uint32) << 8) | (out[byte + 2].astype(np.uint32) << 16)
            fields[po[b]:po[b + 1]] = ((w >> (bit & 7).astype(np.uint32)) & 0x1fff).astype(np.uint16)
        return fields, list(st[:k]), list(sz[:k]), po, pb, out[:nbytes]

    def qlfc_pstream_facts(self, L, coder=1):
        """bscgpu_qlfc_pstream_facts: what the plan of a block in sub-block segments is made of -> (sub_start, sub_size, sub_runs,
        sub_dec: decisions of every sub-block for `coder` (1: -e1, 3: -e0), sub_und: its avg_rank flags left open), lists of nb"""
        a = np.ascontiguousarray(L, dtype=np.uint8)
        nb = C.c_int(0); st = (C.c_int * 8)(); sz = (C.c_int * 8)()
        runs, dec, und = (C.c_uint32 * 8)(), (C.c_uint32 * 8)(), (C.c_uint32 * 8)()
        f = self.L.bscgpu_qlfc_pstream_facts
        f.restype = C.c_int
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_int), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        self._check(f(self.h, N.np_ptr(a), a.size, int(coder), C.byref(nb), st, sz, runs, dec, und))
        k = nb.value
        return list(st[:k]), list(sz[:k]), list(runs[:k]), list(dec[:k]), list(und[:k])

    # ---- the range coder as a stage: many probability streams in one launch (include/bscgpu.h) ----
    def rc_encode(self, form, body, prefix, streams, streams_per_wave=64, out=None):
        """bscgpu_rc_encode: code `streams` (tuples body, count, prefix, nprefix, out_off, out_size) of the host arrays body (uint16
        entries, or the packed bytes for RC_STATIC13) and prefix (uint32 entries of rc_prefix) on the GPU -> (res list, out np.uint8).
        out: the bytes the regions are laid into (a copy is used; default zeros up to the last region's end); res[i] = bytes of
        stream i at out[out_off:], or LIBBSC_NOT_COMPRESSIBLE.  The bytes are rc_encode_host's."""
        b, p, st, o, res = _rc_args(form, body, prefix, streams, out)
        self._check(self.L.bscgpu_rc_encode(self.h, int(form), N.np_ptr(b), b.nbytes, N.np_ptr(p), p.size, st, len(st), N.np_ptr(o), o.size,
                                            N.np_ptr(res), int(streams_per_wave)))
        return [int(x) for x in res[:len(st)]], o

    def rc_encode_device(self, form, dBody, prefix, streams, dOut, streams_per_wave=64):
        """bscgpu_rc_encode_device: the same with the body and the output regions in device tensors (or raw device pointers) -> res list"""
        p = np.ascontiguousarray(prefix, dtype=np.uint32)
        st = rc_streams(streams)
        res = np.zeros(max(len(st), 1), np.int32)
        self._check(self.L.bscgpu_rc_encode_device(self.h, int(form), _dptr(dBody), N.np_ptr(p) if p.size else None, p.size, st, len(st),
                                                   _dptr(dOut), N.np_ptr(res), int(streams_per_wave)))
        return [int(x) for x in res[:len(st)]]

    def compress_device(self, dInput, n, sorter=1, coder=1, features=3, lzp_hash=0, lzp_min=0):
        """bsc_compress of n bytes in HBM -> the block (np.uint8).  lzp_hash / lzp_min: with the LZP stage in front
        (bscgpu_compress_device_lzp; lzp_hash 10..15, else the stage declines: GpuError LIBBSC_NOT_SUPPORTED)"""
        out = np.empty(n + 28, np.uint8)
        if lzp_hash or lzp_min:
            rc = self._check(self.L.bscgpu_compress_device_lzp(self.h, _dptr(dInput), N.np_ptr(out), n, lzp_hash, lzp_min, sorter, coder, features))
        else:
            rc = self._check(self.L.bscgpu_compress_device(self.h, _dptr(dInput), N.np_ptr(out), n, sorter, coder, features))
        return out[:rc]

    # ---- the LZP encoder stage (include/bscgpu.h) --------------------------------
    def lzp_compress(self, data, hash_size, min_len, features=3, device=False):
        """bscgpu_lzp_compress: bsc_lzp_compress on the GPU -> bytes, or the negative libbsc code (LIBBSC_NOT_COMPRESSIBLE,
        LIBBSC_NOT_SUPPORTED for hash_size >= 16).  device=True: `data` is a uint8 device tensor and the stage runs from HBM to HBM
        (bscgpu_lzp_compress_device).  lzp_counters() says which paths the block took."""
        if device:
            import torch
            n = int(data.numel())
            dout = torch.empty(max(n, 1), dtype=torch.uint8, device=data.device)
            r = self.L.bscgpu_lzp_compress_device(self.h, _dptr(data), _dptr(dout), n, hash_size, min_len, features)
            return dout[:r].cpu().numpy().tobytes() if r >= 0 else r
        a = np.ascontiguousarray(np.frombuffer(bytes(data), np.uint8) if not isinstance(data, np.ndarray) else data, dtype=np.uint8)
        inp = a if a.size else np.zeros(1, np.uint8)
        out = np.empty(a.size + 64, np.uint8)
        r = self.L.bscgpu_lzp_compress(self.h, N.np_ptr(inp), N.np_ptr(out), a.size, hash_size, min_len, features)
        return out[:r].tobytes() if r >= 0 else r

    def lzp_compress_batch(self, blocks, sizes=None, hash_size=15, min_len=128, features=3, device=False, dOut=None):
        """bscgpu_lzp_batch_device: bsc_lzp_compress of every block of a pass in one run of the stage -> list of bytes, or the negative
        libbsc code of a block (LIBBSC_NOT_COMPRESSIBLE).  device=True: `blocks` is a uint8 device tensor that holds the blocks back to
        back and `sizes` their lengths; else `blocks` is a list of bytes / uint8 arrays, which go up first.  dOut: a uint8 device tensor
        of the pass's size that takes the output (in the input's layout).  Raises GpuError for a batch-level error
        (LIBBSC_BAD_PARAMETER, LIBBSC_NOT_SUPPORTED for hash_size >= 16).  lzp_counters() gives the sums over the pass."""
        import torch
        if device:
            dT = blocks
            sz = np.ascontiguousarray(np.asarray(sizes, dtype=np.int32))
        else:
            arrs = [np.frombuffer(bytes(b), np.uint8) if not isinstance(b, np.ndarray) else np.asarray(b, np.uint8).ravel() for b in blocks]
            sz = np.array([a.size for a in arrs], np.int32)
            host = np.concatenate(arrs) if arrs and int(sz.sum()) else np.zeros(1, np.uint8)
            dT = torch.from_numpy(np.ascontiguousarray(host)).cuda(self.device)
        total = int(sz.astype(np.int64).sum())
        out = dOut if dOut is not None else torch.empty(max(min(total, int(dT.numel())), 1), dtype=torch.uint8, device=dT.device)
        results = np.zeros(max(sz.size, 1), np.int32)
        self._check(self.L.bscgpu_lzp_batch_device(self.h, _dptr(dT), _dptr(out), N.np_ptr(sz), sz.size, hash_size, min_len, features,
                                                   N.np_ptr(results)))
        Oh = out[:total].cpu().numpy()
        res, o = [], 0
        for b in range(sz.size):
            r = int(results[b])
            res.append(Oh[o:o + r].tobytes() if r >= 0 else r)
            o += int(sz[b])
        return res

    def lzp_counters(self):
        """the last block (or pass) given to the LZP stage: dict(matches, dirty, serial_zones, escapes, raw_chunks)"""
        return {k: self.option_get(self.CNT_LZP_MATCHES + i) for i, k in enumerate(LZP_COUNTERS)}

    # ---- batches of small blocks (one suffix sort per pass, include/bscgpu.h) ----------------
    def bwt_batch(self, dT, sizes, aux=True, dL=None):
        """BWT of every block of a batch laid out back to back in the uint8 device tensor dT -> [(L np.uint8, primary, indexes)];
        primary / indexes as bsc_bwt_encode of the block alone (primary < 0: its error code; indexes None without aux)."""
        import torch
        sz = np.ascontiguousarray(np.asarray(sizes, dtype=np.int32))
        cnt = sz.size
        out = dT if dL is None else dL
        prim = np.zeros(max(cnt, 1), np.int32)
        num = np.zeros(max(cnt, 1), np.uint8)
        idx = np.zeros(16 * max(cnt, 1), np.int32)
        self._check(self.L.bscgpu_bwt_batch_device(self.h, _dptr(dT), _dptr(out), N.np_ptr(sz), cnt, N.np_ptr(prim),
                                                   N.np_ptr(num) if aux else None, N.np_ptr(idx) if aux else None))
        torch.cuda.synchronize(out.device)
        Lh = out[:int(sz.sum())].cpu().numpy() if cnt else np.zeros(0, np.uint8)
        res, o = [], 0
        for b in range(cnt):
            n = int(sz[b])
            res.append((Lh[o:o + n].copy(), int(prim[b]), [int(x) for x in idx[16 * b:16 * b + int(num[b])]] if aux else None))
            o += n
        return res

    def st_batch(self, dT, sizes, k, dOut=None):
        """sort transform of order k of every block of a batch laid out back to back in the uint8 device tensor dT ->
        [(bytes np.uint8, index)] as bsc_st_encode of the block alone (index < 0: its error code); in place unless dOut is given"""
        import torch
        sz = np.ascontiguousarray(np.asarray(sizes, dtype=np.int32))
        cnt = sz.size
        out = dT if dOut is None else dOut
        idx = np.zeros(max(cnt, 1), np.int32)
        self._check(self.L.bscgpu_st_batch_device(self.h, _dptr(dT), _dptr(out), N.np_ptr(sz), cnt, int(k), N.np_ptr(idx)))
        torch.cuda.synchronize(out.device)
        Oh = out[:int(sz.sum())].cpu().numpy() if cnt else np.zeros(0, np.uint8)
        res, o = [], 0
        for b in range(cnt):
            n = int(sz[b])
            res.append((Oh[o:o + n].copy(), int(idx[b])))
            o += n
        return res

    def _batch_results(self, out, sz, results):
        blocks, o = [], 0
        for b in range(sz.size):
            r = int(results[b])
            blocks.append(out[o:o + r].tobytes() if r >= 0 else r)
            o += int(sz[b]) + 28
        return blocks

    def compress_batch(self, blocks, sorter=1, coder=1, lzp_hash=0, lzp_min=0, features=3):
        """bsc_compress of every block (bytes / uint8 arrays) in one batched call -> list of compressed blocks (bytes), or the
        libbsc error code of a block where bsc_compress would return one."""
        arrs = [np.frombuffer(bytes(b), np.uint8) if not isinstance(b, np.ndarray) else np.asarray(b, np.uint8).ravel() for b in blocks]
        sz = np.array([a.size for a in arrs], np.int32)
        inp = np.concatenate(arrs) if arrs else np.zeros(0, np.uint8)
        inp = np.ascontiguousarray(inp) if inp.size else np.zeros(1, np.uint8)
        out = np.empty(int(sz.sum()) + 28 * sz.size + 1, np.uint8)
        results = np.zeros(max(sz.size, 1), np.int32)
        self._check(self.L.bscgpu_compress_batch(self.h, N.np_ptr(inp), N.np_ptr(sz), sz.size, N.np_ptr(out), N.np_ptr(results),
                                                 lzp_hash, lzp_min, sorter, coder, features))
        return self._batch_results(out, sz, results)

    def compress_batch_device(self, dT, sizes, sorter=1, coder=1, features=3, lzp_hash=0, lzp_min=0):
        """compress_batch for blocks laid out back to back in a uint8 device tensor.  lzp_hash / lzp_min: with the LZP stage over every
        pass in front (bscgpu_compress_batch_device_lzp; lzp_hash 10..15, else GpuError LIBBSC_NOT_SUPPORTED)"""
        sz = np.ascontiguousarray(np.asarray(sizes, dtype=np.int32))
        out = np.empty(int(sz.sum()) + 28 * sz.size + 1, np.uint8)
        results = np.zeros(max(sz.size, 1), np.int32)
        if lzp_hash or lzp_min:
            self._check(self.L.bscgpu_compress_batch_device_lzp(self.h, _dptr(dT), N.np_ptr(sz), sz.size, N.np_ptr(out), N.np_ptr(results),
                                                                lzp_hash, lzp_min, sorter, coder, features))
        else:
            self._check(self.L.bscgpu_compress_batch_device(self.h, _dptr(dT), N.np_ptr(sz), sz.size, N.np_ptr(out), N.np_ptr(results),
                                                            sorter, coder, features))
        return self._batch_results(out, sz, results)

    def qlfc_front_batch(self, dL, sizes):
        """bscgpu_qlfc_front_batch_device: the QLFC front end of a pass whose sorted blocks lie back to back in the uint8 device tensor
        dL -> FrontBatch (the layout of include/bscgpu.h)"""
        fb = FrontBatch(sizes)
        self._check(self.L.bscgpu_qlfc_front_batch_device(self.h, _dptr(dL), N.np_ptr(fb.sizes), fb.count, C.byref(fb.lay)))
        return fb

    def static_pstream_batch(self, dL, sizes):
        """bscgpu_static_pstream_batch_device: front end and static-coder model (-e1) of a pass whose sorted blocks lie back to back in
        the uint8 device tensor dL -> (FrontBatch, entries np.uint16[D], poff np.uint32[nsub + 1]); raises GpuError -4 when the device
        declines the pass (option_get(CNT_DC_LAST_FAIL) says why)."""
        fb = FrontBatch(sizes)
        cap = 4 * int(self.max_n) + 65536                       # the device model's own capacity in decisions
        out = np.empty(cap, np.uint16)
        poff = np.zeros(2 * fb.count + 2, np.uint32)
        D = int(self.L.bscgpu_static_pstream_batch_device(self.h, _dptr(dL), N.np_ptr(fb.sizes), fb.count, C.byref(fb.lay), N.np_ptr(out), cap,
                                                          N.np_ptr(poff)))
        self._check(D)
        if D > cap:
            raise GpuError(-2, f"{D} decisions exceed the buffer of {cap}")
        return fb, out[:D], poff[:fb.nsub + 1]

    def fast_pstream_batch(self, dL, sizes):
        """bscgpu_fast_pstream_batch_device: static_pstream_batch for the fast coder (-e0) -> (FrontBatch, entries np.uint16[D] in the
        RC_FAST16 form, poff np.uint32[nsub + 1]); raises GpuError -4 when the device declines the pass"""
        fb = FrontBatch(sizes)
        cap = 4 * int(self.max_n) + 65536                       # the device model's own capacity in decisions
        out = np.empty(cap, np.uint16)
        poff = np.zeros(2 * fb.count + 2, np.uint32)
        D = int(self.L.bscgpu_fast_pstream_batch_device(self.h, _dptr(dL), N.np_ptr(fb.sizes), fb.count, C.byref(fb.lay), N.np_ptr(out), cap,
                                                        N.np_ptr(poff)))
        self._check(D)
        if D > cap:
            raise GpuError(-2, f"{D} decisions exceed the buffer of {cap}")
        return fb, out[:D], poff[:fb.nsub + 1]

    def adaptive_pstream_batch(self, dL, sizes, dbg=False):
        """bscgpu_adaptive_pstream_batch_device: static_pstream_batch for the adaptive coder (-e2) -> (FrontBatch, entries np.uint16[D]
        in the static coder's form, poff np.uint32[nsub + 1]); dbg=True: a fourth item, planes np.uint16[4][D] (state / char / static
        counter values and the mixer id per decision); raises GpuError -4 when the device declines the pass"""
        fb = FrontBatch(sizes)
        cap = 4 * int(self.max_n) + 65536                       # the device model's own capacity in decisions
        out = np.empty(cap, np.uint16)
        planes = np.zeros((4, cap), np.uint16) if dbg else None
        poff = np.zeros(2 * fb.count + 2, np.uint32)
        D = int(self.L.bscgpu_adaptive_pstream_batch_device(self.h, _dptr(dL), N.np_ptr(fb.sizes), fb.count, C.byref(fb.lay), N.np_ptr(out), cap,
                                                            N.np_ptr(poff), N.np_ptr(planes) if dbg else None))
        self._check(D)
        if D > cap:
            raise GpuError(-2, f"{D} decisions exceed the buffer of {cap}")
        return (fb, out[:D], poff[:fb.nsub + 1]) + ((planes[:, :D],) if dbg else ())

    def model_segment_facts(self, dL, sizes, coder=1):
        """bscgpu_model_segment_facts_device: front end of a pass and what the segment plan is made of -> (FrontBatch, sub_dec
        np.uint32[nsub]: decisions of every sub-block for `coder`, sub_und np.uint32[nsub]: its undecided avg_rank flags)"""
        fb = FrontBatch(sizes)
        dec, und = np.zeros(2 * fb.count + 2, np.uint32), np.zeros(2 * fb.count + 2, np.uint32)
        self._check(self.L.bscgpu_model_segment_facts_device(self.h, _dptr(dL), N.np_ptr(fb.sizes), fb.count, C.byref(fb.lay), int(coder),
                                                             N.np_ptr(dec), N.np_ptr(und)))
        return fb, dec[:fb.nsub], und[:fb.nsub]

    def pstream_batch_segments(self, dL, sizes, coder=1, target=0, cap=None):
        """bscgpu_pstream_batch_segments_device: front end and the model of `coder` (1: -e1, 3: -e0) of a pass in model segments of at
        most `target` decisions (0: the arena's capacity) -> (FrontBatch, entries np.uint16[D] of the kept sub-blocks back to back,
        poff np.uint32[nsub + 1], blk_state np.int32[count]: 0 or the DC_FAIL_* mask that leaves the block to the host model)"""
        fb = FrontBatch(sizes)
        if cap is None:
            cap = 16 * int(fb.sizes.sum()) + 4096                  # (a pass may hold more decisions than one segment's capacity)
        out = np.empty(max(cap, 1), np.uint16)
        poff = np.zeros(2 * fb.count + 2, np.uint32)
        state = np.zeros(max(fb.count, 1), np.int32)
        D = int(self.L.bscgpu_pstream_batch_segments_device(self.h, _dptr(dL), N.np_ptr(fb.sizes), fb.count, C.byref(fb.lay), int(coder), int(target),
                                                            N.np_ptr(out), cap, N.np_ptr(poff), N.np_ptr(state)))
        self._check(D)
        if D > cap:
            raise GpuError(-2, f"{D} decisions exceed the buffer of {cap}")
        return fb, out[:D], poff[:fb.nsub + 1], state[:fb.count]

    def adaptive_segment_facts(self, dL, sizes):
        """bscgpu_adaptive_segment_facts_device: model_segment_facts for the adaptive coder (-e2) -> (FrontBatch, sub_dec, sub_und,
        sub_mix np.uint32[nsub]: the longest mixer chain of every sub-block, meaningful where sub_und is 0)"""
        fb = FrontBatch(sizes)
        dec, und, mix = (np.zeros(2 * fb.count + 2, np.uint32) for _ in range(3))
        self._check(self.L.bscgpu_adaptive_segment_facts_device(self.h, _dptr(dL), N.np_ptr(fb.sizes), fb.count, C.byref(fb.lay),
                                                                N.np_ptr(dec), N.np_ptr(und), N.np_ptr(mix)))
        return fb, dec[:fb.nsub], und[:fb.nsub], mix[:fb.nsub]

    def adaptive_pstream_batch_segments(self, dL, sizes, target=0, cap=None):
        """bscgpu_adaptive_pstream_batch_segments_device: pstream_batch_segments for the adaptive coder (-e2): entries in the static
        coder's 16-bit form; blk_state may hold DC_FAIL_MIX (a block with a mixer chain above the step cap)"""
        fb = FrontBatch(sizes)
        if cap is None:
            cap = 16 * int(fb.sizes.sum()) + 4096
        out = np.empty(max(cap, 1), np.uint16)
        poff = np.zeros(2 * fb.count + 2, np.uint32)
        state = np.zeros(max(fb.count, 1), np.int32)
        D = int(self.L.bscgpu_adaptive_pstream_batch_segments_device(self.h, _dptr(dL), N.np_ptr(fb.sizes), fb.count, C.byref(fb.lay), int(target),
                                                                     N.np_ptr(out), cap, N.np_ptr(poff), N.np_ptr(state)))
        self._check(D)
        if D > cap:
            raise GpuError(-2, f"{D} decisions exceed the buffer of {cap}")
        return fb, out[:D], poff[:fb.nsub + 1], state[:fb.count]

    # ---- batched decompression (one inverse-BWT pass for many blocks, include/bscgpu.h) -------
    def unbwt_batch(self, dL, sizes, primary, dT=None):
        """inverse BWT of every block of a batch laid out back to back in the uint8 device tensor dL (primary: 1-based indexes) ->
        (T tensor in the same layout, results list as bscgpu_unbwt returns them per block); in place unless dT is given"""
        sz = np.ascontiguousarray(np.asarray(sizes, dtype=np.int32))
        prim = np.ascontiguousarray(np.asarray(primary, dtype=np.int32))
        assert prim.size == sz.size
        out = dL if dT is None else dT
        results = np.zeros(max(sz.size, 1), np.int32)
        self._check(self.L.bscgpu_unbwt_batch_device(self.h, _dptr(dL), _dptr(out), N.np_ptr(sz), sz.size, N.np_ptr(prim), N.np_ptr(results)))
        return out, [int(x) for x in results[:sz.size]]

    @staticmethod
    def _pack(blocks):
        arrs = [np.frombuffer(bytes(b), np.uint8) if not isinstance(b, np.ndarray) else np.asarray(b, np.uint8).ravel() for b in blocks]
        isz = np.array([a.size for a in arrs], np.int32)
        inp = np.concatenate(arrs) if arrs else np.zeros(0, np.uint8)
        return (np.ascontiguousarray(inp) if inp.size else np.zeros(1, np.uint8)), isz

    def decompress_batch(self, blocks, features=3):
        """bsc_decompress of every compressed block (bytes / uint8 arrays) in one batched call -> list of the decoded blocks (bytes),
        or the libbsc error code of a block where bsc_decompress would return one"""
        inp, isz = self._pack(blocks)
        ds = np.zeros(max(isz.size, 1), np.int32)
        total = self._check(int(self.L.bscgpu_decompress_batch_sizes(N.np_ptr(inp), N.np_ptr(isz), isz.size, N.np_ptr(ds))))
        out = np.empty(max(total, 1), np.uint8)
        results = np.zeros(max(isz.size, 1), np.int32)
        self._check(self.L.bscgpu_decompress_batch(self.h, N.np_ptr(inp), N.np_ptr(isz), isz.size, N.np_ptr(out), total,
                                                   N.np_ptr(results), features))
        res, o = [], 0
        for b in range(isz.size):
            n = int(ds[b])
            res.append(out[o:o + n].tobytes() if results[b] == 0 else int(results[b]))
            o += n
        return res

    def decompress_batch_device(self, blocks, features=3):
        """decompress_batch with the output in HBM -> (uint8 device tensor, offsets[count + 1], results list): block b's bytes are
        out[offsets[b]:offsets[b + 1]] where results[b] == 0"""
        import torch
        inp, isz = self._pack(blocks)
        ds = np.zeros(max(isz.size, 1), np.int32)
        total = self._check(int(self.L.bscgpu_decompress_batch_sizes(N.np_ptr(inp), N.np_ptr(isz), isz.size, N.np_ptr(ds))))
        out = torch.empty(max(total, 1), dtype=torch.uint8, device=f"cuda:{self.device}")
        results = np.zeros(max(isz.size, 1), np.int32)
        self._check(self.L.bscgpu_decompress_batch_device(self.h, N.np_ptr(inp), N.np_ptr(isz), isz.size, _dptr(out), total,
                                                          N.np_ptr(results), features))
        offs = [0]
        for b in range(isz.size):
            offs.append(offs[-1] + int(ds[b]))
        return out[:total], offs, [int(x) for x in results[:isz.size]]

    def pipe(self, depth=2, reuse_outputs=False):
        return Pipe(self, depth, reuse_outputs)

    # ---- measurement / test knobs (include/bscgpu.h: BSCGPU_OPT_*, BSCGPU_CNT_*) ---------------------------------
    OPT_RS_ONESWEEP, CNT_OS_RETRIES, OPT_DC_PACKED_STREAM = 1, 2, 4
    OPT_BATCH_FRONT, CNT_BATCH_FRONT_PASSES, CNT_BATCH_L_PASSES = 9, 10, 11     # the compress-batch passes' route and how many took each
    OPT_DEVICE_RC, CNT_DEVICE_RC_BLOCKS = 12, 13       # a device-model block's streams are range-coded on the GPU (default 0) and how many were
    OPT_BATCH_MODEL, CNT_BATCH_MODEL_PASSES, CNT_BATCH_MODEL_DECLINED = 14, 15, 16    # the static coder's model of a compress-batch pass on the GPU
    OPT_BATCH_MODEL_FAST, CNT_BATCH_FAST_PASSES, CNT_BATCH_FAST_DECLINED = 17, 18, 19    # ... the fast coder's (-e0), an option of its own
    OPT_BATCH_MODEL_ADAPTIVE, CNT_BATCH_ADAPTIVE_PASSES, CNT_BATCH_ADAPTIVE_DECLINED = 38, 39, 40    # ... the adaptive coder's (-e2), an option of its own
    OPT_BATCH_ADAPTIVE_SEGMENTS = 44                 # ... in model segments (default 0; with OPT_BATCH_MODEL_ADAPTIVE and -e2 only)
    CNT_DC_MIX_CHAINS, CNT_DC_MIX_LONGEST, CNT_DC_MIX_WALK_US = 41, 42, 43     # mixer chains of the last -e2 pass on the device model, the steps of the longest, its walk's wall time (get only)
    OPT_BWT_FOLD, CNT_BWT_FOLDED = 20, 21            # key packing sorts the first-sort key's leftover low bits (default 1) and how many sorts took that route
    # a model pass in segments (default 0), segments kept, halves run again, blocks that ended on the host model; the model's capacity in decisions
    OPT_BATCH_MODEL_SEGMENTS, CNT_BATCH_SEGMENTS, CNT_BATCH_SEG_RERUNS, CNT_BATCH_SEG_HOST_BLOCKS, CNT_DC_DCAP = 22, 23, 24, 25, 26
    CNT_DC_REPLAYS, CNT_DC_LAST_FAIL, CNT_DC_AVG_UNDECIDED, CNT_DC_HIST_EXTENDED = 5, 6, 7, 8      # the last device-model block (get only)
    OPT_DC_REPLAY_EXACT, CNT_DC_REPLAY_RESOLVED = 32, 33    # open chunk starts of the evaluation resolved exactly; chunks that settled (get only)
    OPT_DC_AVG_EXACT, CNT_DC_AVG_RESOLVED = 30, 31      # open avg_rank flags resolved exactly on the device; what that settled (get only)
    OPT_DC_HIST_EXACT, CNT_DC_HIST_RESOLVED = 34, 35    # open run_hist brackets resolved exactly on the device; runs that settled (get only)
    # the device model's arena carved for max_n / k (1, 2, 4, 8; a block above it runs in sub-block segments); segments of the last block (get only)
    OPT_DC_ARENA_DIV, CNT_DC_BLOCK_SEGMENTS = 36, 37
    # host blocks with LZP are preprocessed on the device (default 0); blocks that took that route / that the stage declined; the paths of
    # the last block given to the stage (get only): matches, dirty look-ups, failed verifies, escaped literals, chunks kept raw
    OPT_DEVICE_LZP, CNT_LZP_BLOCKS, CNT_LZP_DECLINED = 45, 46, 47
    CNT_LZP_MATCHES, CNT_LZP_DIRTY, CNT_LZP_SERIAL_ZONES, CNT_LZP_ESCAPES, CNT_LZP_RAW_CHUNKS = 48, 49, 50, 51, 52
    # the members of a host-input pass with LZP go up raw and one run of the stage per pass preprocesses them (default 0); passes of either
    # batch call that took the stage, and their sorted blocks
    OPT_BATCH_DEVICE_LZP, CNT_BATCH_LZP_PASSES, CNT_BATCH_LZP_BLOCKS = 53, 54, 55
    DC_FAIL_AVG, DC_FAIL_HIST, DC_FAIL_CAP, DC_FAIL_REPLAY, DC_FAIL_MIX = 2, 4, 8, 16, 32          # BSCGPU_DC_FAIL_*

    def option_set(self, key, value):
        return self._check(self.L.bscgpu_option_set(self.h, key, value))

    def option_get(self, key):
        return self._check(self.L.bscgpu_option_get(self.h, key))

    # ---- profiling ---------------------------------------------------------------------------
    def profile(self, on=True):
        self.L.bscgpu_profile_enable(self.h, 1 if on else 0)

    def profile_reset(self):
        self.L.bscgpu_profile_reset(self.h)

    def profile_get(self):
        arr = (N.KStat * len(N.K_NAMES))()
        self.L.bscgpu_profile_get(self.h, arr)
        return {N.K_NAMES[i]: dict(ms=arr[i].ms, launches=int(arr[i].launches), bytes=int(arr[i].bytes),
                                   records=int(arr[i].records)) for i in range(len(N.K_NAMES))}

    def scatter_launches(self, max_n=4096):
        ms = (C.c_double * max_n)()
        rec = (C.c_uint64 * max_n)()
        cnt = self.L.bscgpu_profile_scatter_launches(self.h, ms, rec, max_n)
        return [(ms[i], int(rec[i])) for i in range(cnt)]

    def last_stage_ms(self):
        out = (C.c_double * 6)()
        self.L.bscgpu_last_stage_ms(self.h, out)
        return list(out)


RC_STATIC16, RC_STATIC13, RC_FAST16 = 0, 1, 2      # BSCGPU_RC_*: the form of a stream's body
RC_REFILL = 128                                    # BSCGPU_RC_REFILL: decisions a wavefront stages per stream and refill
RC_PREFIX_MAX = 32 + 256 * 8                       # BSCGPU_RC_PREFIX_MAX
NOT_COMPRESSIBLE = -3                              # LIBBSC_NOT_COMPRESSIBLE
NOT_SUPPORTED = -4                                 # LIBBSC_NOT_SUPPORTED
LZP_COUNTERS = ("matches", "dirty", "serial_zones", "escapes", "raw_chunks")     # BSCGPU_CNT_LZP_MATCHES .. _RAW_CHUNKS


def lzp_staged_host(data, hash_size, min_len, features=3):
    """bscgpu_lzp_staged_host: the LZP stage's algorithm on the CPU (no GPU, no context) -> (bytes or the negative libbsc code,
    dict of the path counters in the order of LZP_COUNTERS)"""
    a = np.ascontiguousarray(np.frombuffer(bytes(data), np.uint8) if not isinstance(data, np.ndarray) else data, dtype=np.uint8)
    inp = a if a.size else np.zeros(1, np.uint8)
    out = np.empty(a.size + 64, np.uint8)
    cnt = np.zeros(len(LZP_COUNTERS), np.int64)
    r = N.lib().bscgpu_lzp_staged_host(N.np_ptr(inp), N.np_ptr(out), a.size, hash_size, min_len, features, N.np_ptr(cnt))
    return (out[:r].tobytes() if r >= 0 else r), dict(zip(LZP_COUNTERS, (int(x) for x in cnt)))


LZP_BATCH_MAX_CHUNKS, LZP_BATCH_MAX_PIECES, LZP_BATCH_TABLE_BYTES = 8192, 3 * 4096, 17     # csrc/host/lzp_batch_plan.h
PIECE_STAGING, PIECE_RAW, PIECE_TABLE = 0, 1, 2


def lzp_batch_plan(sizes, min_len):
    """bscgpu_lzp_batch_plan: the chunk table of the LZP stage over a pass of blocks back to back (no GPU, no context) -> list of
    (block, start in the pass, size, cap) per chunk in pass order, or the negative libbsc code (LIBBSC_BAD_PARAMETER)"""
    sz = np.ascontiguousarray(np.asarray(sizes, dtype=np.int32))
    t = np.zeros((4, LZP_BATCH_MAX_CHUNKS), np.int32)
    k = N.lib().bscgpu_lzp_batch_plan(N.np_ptr(sz) if sz.size else None, sz.size, min_len, N.np_ptr(t[0]), N.np_ptr(t[1]), N.np_ptr(t[2]), N.np_ptr(t[3]))
    return k if k < 0 else [tuple(int(x) for x in t[:, i]) for i in range(k)]


def lzp_batch_frame(sizes, min_len, features, own):
    """bscgpu_lzp_batch_frame: the frames of a pass from its chunks' own results (own[k] for chunk k of lzp_batch_plan) -> (results per
    block, list of pieces (source, source offset, offset in the output, length), the table bytes, raw chunks)"""
    sz = np.ascontiguousarray(np.asarray(sizes, dtype=np.int32))
    ow = np.ascontiguousarray(np.asarray(own, dtype=np.int32))
    results = np.zeros(max(sz.size, 1), np.int32)
    p = np.zeros((4, LZP_BATCH_MAX_PIECES), np.int32)
    table = np.zeros(max(sz.size, 1) * LZP_BATCH_TABLE_BYTES, np.uint8)
    raw = np.zeros(1, np.int64)
    k = N.lib().bscgpu_lzp_batch_frame(N.np_ptr(sz) if sz.size else None, sz.size, min_len, features, N.np_ptr(ow) if ow.size else None,
                                       N.np_ptr(results), N.np_ptr(p[0]), N.np_ptr(p[1]), N.np_ptr(p[2]), N.np_ptr(p[3]), N.np_ptr(table), N.np_ptr(raw))
    if k < 0:
        return k
    return [int(x) for x in results[:sz.size]], [tuple(int(x) for x in p[:, i]) for i in range(k)], table, int(raw[0])


def lzp_chunk_staged_host(data, cap, hash_size, min_len):
    """bscgpu_lzp_chunk_staged_host: the CPU stand-in's sweep of one chunk under a budget of cap bytes -> (bytes or the negative libbsc
    code, dict of the path counters)"""
    a = np.ascontiguousarray(data, dtype=np.uint8)
    out = np.empty(a.size + 64, np.uint8)
    cnt = np.zeros(len(LZP_COUNTERS), np.int64)
    r = N.lib().bscgpu_lzp_chunk_staged_host(N.np_ptr(a), N.np_ptr(out), a.size, cap, hash_size, min_len, N.np_ptr(cnt))
    return (out[:r].tobytes() if r >= 0 else r), dict(zip(LZP_COUNTERS, (int(x) for x in cnt)))


def rc_streams(streams):
    """a list of (body, count, prefix, nprefix, out_off, out_size) tuples (or an RcStream array) -> ctypes array of bscgpu_rc_stream"""
    if isinstance(streams, C.Array):
        return streams
    arr = (N.RcStream * len(streams))()
    for i, t in enumerate(streams):
        arr[i] = N.RcStream(*[int(x) for x in t])
    return arr


def _rc_args(form, body, prefix, streams, out):
    b = np.ascontiguousarray(body, dtype=np.uint8 if form == RC_STATIC13 else np.uint16)
    p = np.ascontiguousarray(prefix, dtype=np.uint32)
    st = rc_streams(streams)
    end = max([int(s.out_off) + int(s.out_size) + 64 for s in st], default=0)
    o = np.zeros(end, np.uint8) if out is None else np.array(out, dtype=np.uint8, copy=True)
    if int(N.lib().bscgpu_rc_check(int(form), p.size, st, len(st), b.nbytes, o.size)) < 0:
        raise GpuError(-1, "range coder streams: bad form, shape, or a stream outside body / prefix / out")
    return b, p, st, o, np.zeros(max(len(st), 1), np.int32)


def rc_prefix(first_seen, in_size, coder=1):
    """bscgpu_rc_prefix: the decisions the p-stream coders issue before the body (header word, alphabet) as uint32 entries
    {[15:0] p, [20:16] precision, [24] bit}; coder 1 (static) or 3 (fast)"""
    fs = np.ascontiguousarray(first_seen, dtype=np.uint8)
    out = np.zeros(RC_PREFIX_MAX, np.uint32)
    n = int(N.lib().bscgpu_rc_prefix(N.np_ptr(fs), fs.size, int(in_size), int(coder), N.np_ptr(out), out.size))
    if n < 0:
        raise GpuError(n, "bscgpu_rc_prefix")
    return out[:n].copy()


def rc_encode_host(form, body, prefix, streams, out=None):
    """bscgpu_rc_encode_host: GpuContext.rc_encode's CPU stand-in (no GPU): the same streams through the host's scalar range encoder"""
    b, p, st, o, res = _rc_args(form, body, prefix, streams, out)
    rc = int(N.lib().bscgpu_rc_encode_host(int(form), N.np_ptr(b), N.np_ptr(p), p.size, st, len(st), N.np_ptr(o), N.np_ptr(res)))
    if rc < 0:
        raise GpuError(rc, "bscgpu_rc_encode_host")
    return [int(x) for x in res[:len(st)]], o


class _FrontLayout(C.Structure):
    """bscgpu_front_layout (include/bscgpu.h)"""
    _fields_ = [("count", C.c_int), ("nsub", C.c_int), ("m", C.c_int64), ("sizes", C.c_void_p), ("blk_sub", C.c_void_p),
                ("sub_start", C.c_void_p), ("sub_size", C.c_void_p), ("sub_run", C.c_void_p), ("nsym", C.c_void_p),
                ("first_seen", C.c_void_p), ("sym", C.c_void_p), ("rank", C.c_void_p), ("start", C.c_void_p)]


class FrontBatch:
    """The front end's layout of a pass (bscgpu_front_layout): owns the arrays, exposes them trimmed once a call has filled them.
    blk_sub[count + 1]; per sub-block sub_start / sub_size / nsym / first_seen[., 256] and sub_run[nsub + 1]; per run sym / rank / start."""

    def __init__(self, sizes):
        self.sizes = np.ascontiguousarray(np.asarray(sizes, dtype=np.int32))
        cnt = self.count = int(self.sizes.size)
        total = int(self.sizes.sum()) if cnt else 0
        self._a = dict(blk_sub=np.zeros(cnt + 1, np.int32), sub_start=np.zeros(2 * cnt + 1, np.int32), sub_size=np.zeros(2 * cnt + 1, np.int32),
                       sub_run=np.zeros(2 * cnt + 1, np.uint32), nsym=np.zeros(2 * cnt + 1, np.int32),
                       first_seen=np.zeros((2 * cnt + 1, 256), np.uint8), sym=np.zeros(total + 1, np.uint8),
                       rank=np.zeros(total + 1, np.uint8), start=np.zeros(total + 1, np.uint32))
        self.lay = _FrontLayout()
        self.lay.sizes = self.sizes.ctypes.data
        for k, v in self._a.items():
            setattr(self.lay, k, v.ctypes.data)

    nsub = property(lambda self: int(self.lay.nsub))
    m = property(lambda self: int(self.lay.m))
    blk_sub = property(lambda self: self._a["blk_sub"])
    sub_start = property(lambda self: self._a["sub_start"][:self.nsub])
    sub_size = property(lambda self: self._a["sub_size"][:self.nsub])
    sub_run = property(lambda self: self._a["sub_run"][:self.nsub + 1])
    nsym = property(lambda self: self._a["nsym"][:self.nsub])
    sym = property(lambda self: self._a["sym"][:self.m])
    rank = property(lambda self: self._a["rank"][:self.m])
    start = property(lambda self: self._a["start"][:self.m])

    def first_seen(self, s):
        return self._a["first_seen"][s, :int(self._a["nsym"][s])]

    def code(self, block, coder=1, features=3):
        """bscgpu_front_batch_code: what bsc_coder_compress gives for this block's L -> bytes, or its negative code"""
        out = np.empty(int(self.sizes[block]) + 4096, np.uint8)
        r = int(N.lib().bscgpu_front_batch_code(C.byref(self.lay), int(block), N.np_ptr(out), int(coder), int(features)))
        return out[:r].tobytes() if r >= 0 else r


def front_batch_host(L, sizes):
    """bscgpu_front_batch_host: the layout of a pass built on the CPU from L (uint8, the blocks back to back) -> FrontBatch"""
    a = np.ascontiguousarray(L, dtype=np.uint8)
    fb = FrontBatch(sizes)
    assert a.size >= int(fb.sizes.sum())
    rc = int(N.lib().bscgpu_front_batch_host(N.np_ptr(a) if a.size else None, N.np_ptr(fb.sizes), fb.count, C.byref(fb.lay)))
    if rc < 0:
        raise GpuError(rc, "bscgpu_front_batch_host")
    return fb


def static_pstream_host(fb, s):
    """bscgpu_static_pstream_host: GpuContext.static_pstream_batch's CPU stand-in for sub-block s of a FrontBatch (no GPU): the host
    model's own walk, recording {[11:0] p, [12] bit, [13] run start} instead of coding -> np.uint16 entries"""
    cap = 16 * int(fb.sub_size[s]) + 64
    out = np.empty(cap, np.uint16)
    n = int(N.lib().bscgpu_static_pstream_host(C.byref(fb.lay), int(s), N.np_ptr(out), cap))
    if n < 0:
        raise GpuError(n, "bscgpu_static_pstream_host")
    if n > cap:
        out = np.empty(n, np.uint16)
        n = int(N.lib().bscgpu_static_pstream_host(C.byref(fb.lay), int(s), N.np_ptr(out), n))
    return out[:n]


def front_batch_code_ps(fb, block, ps, poff, features=3):
    """bscgpu_front_batch_code_ps: FrontBatch.code for the static coder from the sub-blocks' probability streams (ps uint16 entries,
    sub-block s at poff[s]) -> bytes, or its negative code"""
    p = np.ascontiguousarray(ps, dtype=np.uint16)
    o = np.ascontiguousarray(poff, dtype=np.uint32)
    assert o.size == fb.nsub + 1 and (p.size >= int(o[-1]))
    if p.size == 0:
        p = np.zeros(1, np.uint16)
    out = np.empty(int(fb.sizes[block]) + 4096, np.uint8)
    r = int(N.lib().bscgpu_front_batch_code_ps(C.byref(fb.lay), int(block), N.np_ptr(p), N.np_ptr(o), N.np_ptr(out), int(features)))
    return out[:r].tobytes() if r >= 0 else r


def fast_pstream_host(fb, s):
    """bscgpu_fast_pstream_host: GpuContext.fast_pstream_batch's CPU stand-in for sub-block s of a FrontBatch (no GPU): the host fast
    coder's own walk, recording {[12:0] counter value, [13] bit, [14] run start, [15] run side} instead of coding -> np.uint16 entries"""
    cap = 16 * int(fb.sub_size[s]) + 64
    out = np.empty(cap, np.uint16)
    n = int(N.lib().bscgpu_fast_pstream_host(C.byref(fb.lay), int(s), N.np_ptr(out), cap))
    if n < 0:
        raise GpuError(n, "bscgpu_fast_pstream_host")
    if n > cap:
        out = np.empty(n, np.uint16)
        n = int(N.lib().bscgpu_fast_pstream_host(C.byref(fb.lay), int(s), N.np_ptr(out), n))
    return out[:n]


def adaptive_pstream_host(fb, s, dbg=False):
    """bscgpu_adaptive_pstream_host: GpuContext.adaptive_pstream_batch's CPU stand-in for sub-block s of a FrontBatch (no GPU): the host
    model's walk with the adaptive counters and the mixer step the device uses, recording {[11:0] p, [12] bit, [13] run start} ->
    np.uint16 entries; dbg=True: (entries, planes np.uint16[4][n]: state / char / static counter values and the mixer id per decision)"""
    f = N.lib().bscgpu_adaptive_pstream_host
    n = int(f(C.byref(fb.lay), int(s), None, 0, None))
    if n < 0:
        raise GpuError(n, "bscgpu_adaptive_pstream_host")
    out = np.empty(max(n, 1), np.uint16)
    planes = np.zeros((4, max(n, 1)), np.uint16) if dbg else None
    n2 = int(f(C.byref(fb.lay), int(s), N.np_ptr(out), max(n, 1), N.np_ptr(planes) if dbg else None))
    assert n2 == n
    return (out[:n], planes[:, :n]) if dbg else out[:n]


def adaptive_longest_chain_host(fb, s, per_mixer=False):
    """bscgpu_adaptive_longest_chain_host: the longest mixer chain of sub-block s of a FrontBatch, the host walker's own count (no GPU)
    -> int; per_mixer=True: (int, np.uint32[1896] decisions of every mixer)"""
    cnt = np.zeros(1896, np.uint32) if per_mixer else None
    n = int(N.lib().bscgpu_adaptive_longest_chain_host(C.byref(fb.lay), int(s), N.np_ptr(cnt) if per_mixer else None))
    if n < 0:
        raise GpuError(n, "bscgpu_adaptive_longest_chain_host")
    return (n, cnt) if per_mixer else n


def front_batch_code_psf(fb, block, ps, poff, features=3):
    """bscgpu_front_batch_code_psf: FrontBatch.code for the fast coder from the sub-blocks' streams (ps uint16 entries in the RC_FAST16
    form, sub-block s at poff[s]) -> bytes, or its negative code"""
    p = np.ascontiguousarray(ps, dtype=np.uint16)
    o = np.ascontiguousarray(poff, dtype=np.uint32)
    assert o.size == fb.nsub + 1 and (p.size >= int(o[-1]))
    if p.size == 0:
        p = np.zeros(1, np.uint16)
    out = np.empty(int(fb.sizes[block]) + 4096, np.uint8)
    r = int(N.lib().bscgpu_front_batch_code_psf(C.byref(fb.lay), int(block), N.np_ptr(p), N.np_ptr(o), N.np_ptr(out), int(features)))
    return out[:r].tobytes() if r >= 0 else r


def batch_plan(sizes, sorter=1, cap=64 << 20):
    """bscgpu_batch_plan: the pass of every block of a batch, -1 for the single-block path -> (passes, list)"""
    sz = np.ascontiguousarray(np.asarray(sizes, dtype=np.int32))
    pass_of = np.zeros(max(sz.size, 1), np.int32)
    n = N.lib().bscgpu_batch_plan(N.np_ptr(sz), sz.size, sorter, int(cap), N.np_ptr(pass_of))
    return int(n), [int(x) for x in pass_of[:sz.size]]


ST_BATCH_MAX_N, ST_BATCH_MAX_BLOCKS = 1 << 20, 4096      # BSCGPU_ST_BATCH_MAX_N, BSCGPU_ST_BATCH_MAX_BLOCKS (include/bscgpu.h)


def st_batch_plan(sizes, k, cap=64 << 20):
    """bscgpu_st_batch_plan: the pass of every block of an ST batch of order k, -1 for the single-block path -> (passes, list)"""
    sz = np.ascontiguousarray(np.asarray(sizes, dtype=np.int32))
    pass_of = np.full(max(sz.size, 1), -2, np.int32)
    n = N.lib().bscgpu_st_batch_plan(N.np_ptr(sz), sz.size, int(k), int(cap), N.np_ptr(pass_of))
    return int(n), [int(x) for x in pass_of[:sz.size]]


def model_segment_plan(sub_dec, sub_und, blk_sub, dcap, target=0):
    """bscgpu_model_segment_plan: the model segment of every block of a pass, -1 for a block left out -> (segments, list)"""
    dec = np.ascontiguousarray(np.asarray(sub_dec, dtype=np.uint32))
    und = np.ascontiguousarray(np.asarray(sub_und, dtype=np.uint32))
    bs = np.ascontiguousarray(np.asarray(blk_sub, dtype=np.int32))
    count = bs.size - 1
    assert count >= 0 and dec.size == und.size and (count == 0 or dec.size >= int(bs[-1]))
    seg_of = np.full(max(count, 1), -2, np.int32)
    if dec.size == 0:                                           # (blocks without a sub-block: the arrays are never read)
        dec = und = np.zeros(1, np.uint32)
    n = int(N.lib().bscgpu_model_segment_plan(N.np_ptr(dec), N.np_ptr(und), N.np_ptr(bs), count,
                                              int(dcap), int(target), N.np_ptr(seg_of)))
    if n < 0:
        raise GpuError(n, "bscgpu_model_segment_plan")
    return n, [int(x) for x in seg_of[:count]]


def block_segment_plan(sub_runs, sub_dec, mcap, dcap):
    """bscgpu_block_segment_plan: where a single block is cut for an arena of mcap runs and dcap decisions -> (segments, segment of
    every sub-block); raises GpuError -4 when a sub-block alone exceeds a capacity, -1 for bad arguments"""
    runs = np.ascontiguousarray(np.asarray(sub_runs, dtype=np.uint32))
    dec = np.ascontiguousarray(np.asarray(sub_dec, dtype=np.uint32))
    assert runs.size == dec.size
    seg_of = np.full(8, -2, np.int32)
    f = N.lib().bscgpu_block_segment_plan
    f.restype = C.c_int
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_int64, C.c_void_p]
    n = int(f(N.np_ptr(runs) if runs.size else None, N.np_ptr(dec) if dec.size else None, runs.size, int(mcap), int(dcap), N.np_ptr(seg_of)))
    if n < 0:
        raise GpuError(n, "bscgpu_block_segment_plan")
    return n, [int(x) for x in seg_of[:runs.size]]


def unbwt_batch_plan(sizes, cap=64 << 20):
    """bscgpu_unbwt_batch_plan: sizes[b] = a BWT block's length, -1 for a block of another route -> (passes, pass of every block)"""
    sz = np.ascontiguousarray(np.asarray(sizes, dtype=np.int32))
    pass_of = np.zeros(max(sz.size, 1), np.int32)
    n = N.lib().bscgpu_unbwt_batch_plan(N.np_ptr(sz), sz.size, int(cap), N.np_ptr(pass_of))
    return int(n), [int(x) for x in pass_of[:sz.size]]


def coder_pool_stats(reset=False):
    """how the process's coder pool has coded the pipes' blocks: {scalar x8 tasks, pairs x4 tasks, eight_lanes x1 task, host_model}"""
    out = (C.c_uint64 * 4)()
    N.lib().bscgpu_coder_pool_stats(out, 1 if reset else 0)
    return {"scalar_tasks": int(out[0]), "pair_tasks": int(out[1]), "eight_lane_task": int(out[2]), "host_model": int(out[3])}


class Pipe:
    """Several blocks in flight on one GPU (bscgpu_pipe_*): submit() runs the GPU stage, the host coder of that
    block runs on worker threads while the next block is sorted."""

    def __init__(self, ctx, depth=2, reuse_outputs=False):
        # reuse_outputs: wait() returns a view into one of `depth` recycled output buffers, valid until `depth` further
        # submits (no 64 MiB allocation and no page faults per block); default: a fresh array per block
        self.reuse = reuse_outputs
        self._pool = {}
        self._seq = 0
        self.ctx = ctx
        self.L = ctx.L
        h = C.c_void_p()
        ctx._check(self.L.bscgpu_pipe_create(ctx.h, depth, C.byref(h)))
        self.h = h
        self.depth = depth
        self._out = {}

    def _new_out(self, n):
        if not self.reuse:
            return np.empty(n + 28, np.uint8)
        k = self._seq % self.depth
        self._seq += 1
        buf = self._pool.get(k)
        if buf is None or buf.size < n + 28:
            buf = self._pool[k] = np.empty(n + 28, np.uint8)
        return buf[:n + 28]

    def submit(self, dInput, n, sorter=1, coder=1, features=3):
        out = self._new_out(n)
        t = self.ctx._check(self.L.bscgpu_pipe_submit(self.h, _dptr(dInput), N.np_ptr(out), n, sorter, coder, features))
        self._out[t] = (out, dInput)          # keep both alive until wait()
        return t

    def submit_host(self, data, sorter=1, coder=1, lzp_hash=0, lzp_min=0, features=3):
        """Host-resident block (np.uint8) with bsc_compress's full parameter list, LZP included."""
        a = np.ascontiguousarray(data, dtype=np.uint8)
        out = self._new_out(a.size)
        t = self.ctx._check(self.L.bscgpu_pipe_submit_host(self.h, N.np_ptr(a), N.np_ptr(out), a.size, lzp_hash, lzp_min,
                                                            sorter, coder, features))
        self._out[t] = (out, a)
        return t

    def wait(self, ticket):
        rc = self.ctx._check(self.L.bscgpu_pipe_wait(self.h, ticket))
        out, _ = self._out.pop(ticket)
        return out[:rc]

    def close(self):
        if getattr(self, "h", None):
            self.L.bscgpu_pipe_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---- the packed 13-bit stream of a pass (include/bscgpu.h, "the packed 13-bit stream of a pass") -----------------------------------
P13_SLACK = 8                                       # bytes behind a packed stream that a coder's 4-byte entry read may touch


def pstream_pack13_host(ps, poff):
    """bscgpu_pstream_pack13_host: the CPU stand-in for the packed layout of a pass: 16-bit static entries (sub-block s at
    [poff[s], poff[s + 1])) -> (bytes np.uint8[pbase[nsub] / 8 * 13], pbase np.int64[nsub + 1])"""
    p = np.ascontiguousarray(ps, dtype=np.uint16)
    o = np.ascontiguousarray(poff, dtype=np.uint32)
    nsub = int(o.size) - 1
    assert nsub >= 0 and p.size >= int(o[-1])
    if p.size == 0:
        p = np.zeros(1, np.uint16)
    pbase = np.zeros(nsub + 1, np.int64)
    n = int(N.lib().bscgpu_pstream_pack13_host(N.np_ptr(p), N.np_ptr(o), nsub, None, 0, N.np_ptr(pbase)))
    if n < 0:
        raise GpuError(n, "bscgpu_pstream_pack13_host")
    out = np.full(n + P13_SLACK, 0xa5, np.uint8)     # (not zero: the call has to write every byte of the layout itself)
    n2 = int(N.lib().bscgpu_pstream_pack13_host(N.np_ptr(p), N.np_ptr(o), nsub, N.np_ptr(out), n, N.np_ptr(pbase)))
    if n2 != n:
        raise GpuError(n2, "bscgpu_pstream_pack13_host")
    return out[:n], pbase


def front_batch_code_ps13(fb, block, packed, poff, pbase, features=3):
    """bscgpu_front_batch_code_ps13: FrontBatch.code for the static coder from the pass's packed stream (sub-block s's RC_STATIC13
    body at decision pbase[s]) -> bytes, or its negative code"""
    o = np.ascontiguousarray(poff, dtype=np.uint32)
    pb = np.ascontiguousarray(pbase, dtype=np.int64)
    assert o.size == fb.nsub + 1 and pb.size == fb.nsub + 1
    b = np.zeros(int(pb[-1]) // 8 * 13 + P13_SLACK, np.uint8)
    src = np.ascontiguousarray(packed, dtype=np.uint8)
    assert src.size >= b.size - P13_SLACK
    b[:b.size - P13_SLACK] = src[:b.size - P13_SLACK]
    out = np.empty(int(fb.sizes[block]) + 4096, np.uint8)
    r = int(N.lib().bscgpu_front_batch_code_ps13(C.byref(fb.lay), int(block), N.np_ptr(b), N.np_ptr(o), N.np_ptr(pb), N.np_ptr(out), int(features)))
    return out[:r].tobytes() if r >= 0 else r


def _static_pstream_batch_packed(self, dL, sizes, cap_bytes=None):
    """bscgpu_static_pstream_batch_packed_device: static_pstream_batch with the stream in the packed 13-bit form -> (FrontBatch, bytes
    np.uint8[pbase[nsub] / 8 * 13], poff np.uint32[nsub + 1], pbase np.int64[nsub + 1]); raises GpuError -4 when the device declines
    the pass or (option_get(CNT_DC_LAST_FAIL) == 0) the packed form was void"""
    fb = FrontBatch(sizes)
    if cap_bytes is None:
        cap_bytes = 2 * (4 * int(self.max_n) + 65536)           # the device's stream buffer
    out = np.full(cap_bytes + P13_SLACK, 0xa5, np.uint8)
    poff = np.zeros(2 * fb.count + 2, np.uint32)
    pbase = np.zeros(2 * fb.count + 2, np.int64)
    D = int(self.L.bscgpu_static_pstream_batch_packed_device(self.h, _dptr(dL), N.np_ptr(fb.sizes), fb.count, C.byref(fb.lay), N.np_ptr(out),
                                                             cap_bytes, N.np_ptr(poff), N.np_ptr(pbase)))
    self._check(D)
    n = int(pbase[fb.nsub]) // 8 * 13
    if n > cap_bytes:
        raise GpuError(-2, f"{n} bytes exceed the buffer of {cap_bytes}")
    return fb, out[:n], poff[:fb.nsub + 1], pbase[:fb.nsub + 1]


def _pstream_batch_segments_packed(self, dL, sizes, coder=1, target=0, cap_bytes=None):
    """bscgpu_pstream_batch_segments_packed_device: pstream_batch_segments for -e1 with the kept segments' streams in the packed 13-bit
    form -> (FrontBatch, bytes np.uint8[pbase[nsub] / 8 * 13], poff np.uint32[nsub + 1], pbase np.int64[nsub + 1], blk_state
    np.int32[count]); above cap_bytes the bytes are counted, not copied (the returned array is then empty)"""
    fb = FrontBatch(sizes)
    if cap_bytes is None:
        cap_bytes = 26 * int(fb.sizes.sum()) + 104 * 2 * fb.count + 4096
    out = np.full(max(cap_bytes, 0) + P13_SLACK, 0xa5, np.uint8)
    poff = np.zeros(2 * fb.count + 2, np.uint32)
    pbase = np.zeros(2 * fb.count + 2, np.int64)
    state = np.zeros(max(fb.count, 1), np.int32)
    D = int(self.L.bscgpu_pstream_batch_segments_packed_device(self.h, _dptr(dL), N.np_ptr(fb.sizes), fb.count, C.byref(fb.lay), int(coder), int(target),
                                                               N.np_ptr(out), int(cap_bytes), N.np_ptr(poff), N.np_ptr(pbase), N.np_ptr(state)))
    self._check(D)
    n = int(pbase[fb.nsub]) // 8 * 13
    return fb, (out[:n] if n <= cap_bytes else out[:0]), poff[:fb.nsub + 1], pbase[:fb.nsub + 1], state[:fb.count]


GpuContext.static_pstream_batch_packed = _static_pstream_batch_packed
GpuContext.pstream_batch_segments_packed = _pstream_batch_segments_packed
# the packed 13-bit stream for the static coder's batch model (default 0); passes / segments that went down packed, and as 16-bit entries after all
GpuContext.OPT_BATCH_MODEL_PACKED, GpuContext.CNT_BATCH_PACKED_PASSES, GpuContext.CNT_BATCH_PACKED_VOID = 27, 28, 29
