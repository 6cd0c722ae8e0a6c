"""Inputs and a Python twin for the range coder stage (bscgpu_rc_encode*, include/bscgpu.h), shared by test_rc_streams_host.py (CPU)
and test_gpu_rc_device.py.

The twin is a few lines of range coder written from the format (32-bit range, 64-bit low with the carry in bit 32, a cached 16-bit
unit and a count of pending 0xffff units, 16-bit little-endian output; finish = one conditional and three unconditional shifts).  It
exists to DRIVE one generator: steered() looks at the twin's state before every decision and picks the entry that pushes low against
2^32, so that units pend, and then the entry that overflows, so that a carry runs into two or more pending units.  Uniform random entries
practically never do that (one pending unit and no carry into it in 400 000 decisions), so random data does not test the carry path."""
import numpy as np

STATIC16, STATIC13, FAST16 = 0, 1, 2
NOT_COMPRESSIBLE = -3
M32 = 0xffffffff


class Twin:
    """one stream of the range coder, in Python"""

    def __init__(self):
        self.low, self.range, self.cache, self.held = 0, M32, 0, 0
        self.out = bytearray()
        self.carries = self.carries2 = self.longest = 0      # carries into pending units, into >= 2 of them, longest pending stretch

    def _put(self, v):
        self.out += bytes((v & 0xff, (v >> 8) & 0xff))

    def shift(self):
        low32, carry = self.low & M32, self.low >> 32
        if low32 < 0xffff0000 or carry:
            self._put(self.cache + carry)
            if carry and self.held:
                self.carries += 1
                self.carries2 += self.held >= 2
            for _ in range(self.held):
                self._put(carry - 1)                          # 0xffff without a carry, 0x0000 after one
            self.held = 0
            self.cache = low32 >> 16
        else:
            self.held += 1
            self.longest = max(self.longest, self.held)
        self.low = (low32 << 16) & M32

    def renorm(self):
        if self.range < 0x10000:
            self.shift()
            self.range = (self.range << 16) & M32

    def apply(self, bit, p, prec):
        r = (self.range >> prec) * p
        if bit:
            self.low += r
            self.range -= r
        else:
            self.range = r

    def encode(self, bit, p, prec=12):
        self.renorm()
        self.apply(bit, p, prec)

    def finish(self):
        if self.range < 0x10000:
            self.shift()
        for _ in range(3):
            self.shift()
        return bytes(self.out)


def twin_bytes(prefix, body, form=STATIC16):
    """prefix entries (uint32) then 16-bit body entries through the twin -> bytes (no budget: for streams with room)"""
    t = Twin()
    for e in np.asarray(prefix).tolist():
        t.encode((e >> 24) & 1, e & 0xffff, (e >> 16) & 31)
    for x in np.asarray(body).tolist():
        if form == FAST16:
            t.encode((x >> 13) & 1, x & 0x1fff, 13 - ((x >> 15) << 1))
        else:
            t.encode((x >> 12) & 1, x & 0xfff, 12)
    return t.finish()


def steered(seed, steps):
    """-> (uint16 STATIC16 entries, the twin that coded them).  The coder's interval is [low, low + range).  Units pend while it lies
    across a multiple of 2^32 (nobody knows yet whether a carry will come), so the generator waits, on seeded random entries, until a
    renormalisation leaves the interval across 2^32, and then keeps it there: the 1-bit with the largest p that keeps low below 2^32
    (or, when even p = 1 carries, the 0-bit with p = 1, which keeps the top above), each of which shrinks the range by about 2^12, so the
    next units pend.  Once k units pend (k = 2 .. 6, seeded) it picks the 1-bit with the smallest p that carries."""
    rng = np.random.default_rng(seed)
    rnd_p = rng.integers(1, 4096, steps).tolist()
    rnd_b = rng.integers(0, 2, steps).tolist()
    rnd_k = rng.integers(0, 64, steps).tolist()
    t = Twin()
    out = np.empty(steps, np.uint16)
    target = 2
    for i in range(steps):
        t.renorm()
        q = t.range >> 12
        room = M32 - t.low                                     # largest r that does not carry
        bit, p = rnd_b[i], rnd_p[i]
        if t.held == 0:
            target = 2 + rnd_k[i] % 5
        if 0 <= room < t.range - 1 and rnd_k[i] != 63:         # across 2^32, and not yet carried
            if t.held >= target:
                bit, p = 1, min(4095, room // q + 1)           # smallest p with low + q p >= 2^32 (4095: not yet, stays across)
            elif room >= q:
                bit, p = 1, min(4095, room // q)
            else:
                bit, p = 0, 1
        t.apply(bit, p, 12)
        out[i] = p | (bit << 12) | ((i % 5 == 0) << 13)
    return out, t


def pack_p13(entries):
    """16-bit static entries -> the packed form: 13 bits per decision {[11:0] p, [12] bit}, eight in 13 bytes, the last group zero-padded"""
    e = (np.asarray(entries, dtype=np.uint16) & 0x1fff).astype("<u2")
    pad = (-e.size) % 8
    e = np.concatenate([e, np.zeros(pad, "<u2")])
    bits = np.unpackbits(e.view(np.uint8).reshape(-1, 2), axis=1, bitorder="little")[:, :13]
    return np.packbits(bits.reshape(-1), bitorder="little")


def first_seen(L):
    """distinct symbols of a sub-block in order of first appearance"""
    a = np.asarray(L, dtype=np.uint8)
    _, idx = np.unique(a, return_index=True)
    return a[np.sort(idx)]


def random_static(rng, n, run_every=4):
    """n STATIC16 entries: p in 1..4095, a random bit, a run-start mark on every run_every-th"""
    e = rng.integers(1, 4096, n).astype(np.uint16) | (rng.integers(0, 2, n).astype(np.uint16) << 12)
    e[::run_every] |= 1 << 13
    return e


def skewed_static(rng, n, run_every=4):
    """n STATIC16 entries that compress: the coded bit is the likely one nine times in ten"""
    p = rng.integers(1, 400, n).astype(np.uint16)
    bit = (rng.integers(0, 10, n) != 0).astype(np.uint16)      # bit 1 takes range - r: likely when p is small
    e = p | (bit << 12)
    e[::run_every] |= 1 << 13
    return e


def random_fast(rng, n, run_every=4):
    """n FAST16 entries: both precisions mixed — 13 bits on the rank side, 11 on the run side (bit 15), p inside the precision"""
    side = rng.integers(0, 2, n).astype(np.uint16)
    p = np.where(side == 1, rng.integers(1, 1 << 11, n), rng.integers(1, 1 << 13, n)).astype(np.uint16)
    e = p | (rng.integers(0, 2, n).astype(np.uint16) << 13) | (side << 15)
    e[::run_every] |= 1 << 14
    return e


def coin_flips(n, form=STATIC16):
    """n decisions at probability one half with alternating bits: one output bit each, whatever the coder does"""
    bit = (np.arange(n) & 1).astype(np.uint16)
    if form == FAST16:
        return (np.uint16(1 << 12) | (bit << 13) | np.uint16(1 << 14)).astype(np.uint16)      # rank side: 4096 / 8192, every entry a run start
    return (np.uint16(2048) | (bit << 12) | np.uint16(1 << 13)).astype(np.uint16)


def lay_out(counts, out_sizes, nprefix=None, body_gap=0, body_first=0, canary=0, form=STATIC16):
    """streams back to back -> (list of stream tuples, body entries needed, out bytes needed).  body_first: index of the first stream's
    first entry; body_gap: entries left between two streams (packed: both in decisions, kept multiples of 8); canary: bytes left free
    behind every region.  Prefix ranges are consecutive (nprefix[i] entries each)."""
    st, b, o, pf = [], body_first, 0, 0
    for i, (c, osz) in enumerate(zip(counts, out_sizes)):
        npf = 0 if nprefix is None else nprefix[i]
        st.append((b, c, pf, npf, o, osz))
        pf += npf
        b += c + body_gap
        if form == STATIC13:
            b = (b + 7) // 8 * 8
        o += osz + 64 + canary
        o += o & 1
    return st, b, o


def plain_prefix(rng, n):
    """n prefix entries of the static kind (precision 12, p 2048) with seeded bits"""
    return (np.uint32(2048) | (np.uint32(12) << 16) | (rng.integers(0, 2, n).astype(np.uint32) << 24)).astype(np.uint32)
