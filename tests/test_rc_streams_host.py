"""The range coder stage on the CPU (no GPU): bscgpu_rc_prefix and bscgpu_rc_encode_host (include/bscgpu.h), the stand-in the device
kernel is compared against in test_gpu_rc_device.py.

A stream = the prefix entries of rc_prefix (header word + alphabet) + a body of probability entries.  With the static model's trace
(Oracle.static_pstream) as the body the bytes must be the reference's bsc_qlfc_static_encode_block; with the fast coder's trace
(tools/devcoder_fast_sim.cpp --trace: the chains the device model runs, walked on the CPU) those of its fast coder."""
import os
import subprocess

import numpy as np
import pytest

import rc_inputs as ri
from libbsc_amd import api, gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def orc():
    from oracle.refbind import Oracle
    return Oracle()


def _sorted_blocks(ref):
    bwt = lambda T: np.ascontiguousarray(ref.bwt_encode(T)[0])
    rng = np.random.default_rng(40)
    return [("text300k", bwt(api.synth_text_v1(3, 300_000))),
            ("ab", (np.arange(600_000) % 2).astype(np.uint8)),
            ("tiny", np.array([1, 1, 2, 2, 2, 1, 3], np.uint8)),
            ("40 symbols", bwt(rng.integers(100, 140, 120_000, dtype=np.uint8) // np.uint8(1)))]


def _sub_blocks(L):
    """the sub-blocks bsc_coder_compress cuts the sorted block into (coder.cpp:70-109), through the library's own split"""
    fb = gpu.front_batch_host(L, [L.size])
    return [L[int(s):int(s) + int(z)] for s, z in zip(fb.sub_start, fb.sub_size)]


def _one(form, body, prefix, count, out_size, body_first=0):
    res, out = gpu.rc_encode_host(form, body, prefix, [(body_first, count, 0, len(prefix), 0, out_size)])
    return res[0] if res[0] < 0 else out[:res[0]].tobytes()


def test_static_streams_equal_the_reference(ref, orc):
    """rc_prefix + Oracle.static_pstream through rc_encode_host = bsc_qlfc_static_encode_block, for every sub-block; the packed form
    gives the same bytes (none of these streams is near its budget)"""
    seen = 0
    for name, L in _sorted_blocks(ref):
        subs = _sub_blocks(L)
        assert len(subs) == api_num_blocks(L.size), name
        for sub in subs:
            want = ref.qlfc_encode_block(sub, 1)
            tr, _ = orc.static_pstream(sub)
            pre = gpu.rc_prefix(ri.first_seen(sub), sub.size, 1)
            got = _one(ri.STATIC16, tr, pre, tr.size, sub.size)
            assert got == want, (name, sub.size)
            if isinstance(want, bytes):
                assert len(want) < sub.size - 64, name                     # with room: the packed form's budget test cannot differ
                assert _one(ri.STATIC13, ri.pack_p13(tr), pre, tr.size, sub.size) == want, (name, sub.size, "packed")
                seen += 1
    assert seen >= 5


def api_num_blocks(n):
    return 1 if n < 256 * 1024 else 2 if n < 1 << 20 else 4 if n < 4 << 20 else 8      # coder.cpp:59-68 (bsc_coder_num_blocks)


def test_packed_body_at_any_group_offset():
    """a packed body starts at any multiple of 8 decisions of the packed space; same bytes as the 16-bit form"""
    rng = np.random.default_rng(1)
    e = ri.skewed_static(rng, 1000)
    pre = ri.plain_prefix(rng, 40)
    want = _one(ri.STATIC16, e, pre, e.size, 4096)
    assert want == ri.twin_bytes(pre, e)
    for first in (8, 24, 64, 1000 // 8 * 8):
        packed = np.concatenate([rng.integers(0, 256, first // 8 * 13, dtype=np.uint8), ri.pack_p13(e)])
        assert _one(ri.STATIC13, packed, pre, e.size, 4096, body_first=first) == want, first


def test_fast_stream_equals_the_fast_coder(ref, tmp_path):
    """The fast form.  A fast trace IS available on the CPU: tools/devcoder_fast_sim.cpp --trace writes the entry stream of the chains
    the device model runs.  rc_prefix(coder 3) + that trace through rc_encode_host must be api.bsc_qlfc_encode_block(..., coder=3),
    which is also the reference's."""
    exe = str(tmp_path / "fast_sim")
    subprocess.run(["g++", "-O0", "-std=c++17", "-march=x86-64-v3", "-I", os.path.join(ROOT, "libbsc_amd/csrc/host"), "-I", os.path.join(ROOT, "libbsc_amd/csrc/device"),
                    "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tools/devcoder_fast_sim.cpp"), "-o", exe], check=True)
    rng = np.random.default_rng(2)
    L = np.ascontiguousarray(ref.bwt_encode(api.synth_text_v1(3, 300_000))[0])
    cases = _sub_blocks(L) + [np.array([1, 1, 2, 2, 2, 1, 3], np.uint8), np.repeat(rng.integers(0, 5, 3000).astype(np.uint8), rng.integers(1, 60, 3000))]
    for k, sub in enumerate(cases):
        src, dst = tmp_path / f"in{k}.bin", tmp_path / f"tr{k}.bin"
        sub.tofile(src)
        subprocess.run([exe, "--trace", str(src), str(dst)], check=True)
        tr = np.fromfile(dst, np.uint16)
        assert tr.size > 0 and (tr >> 15).any() and not (tr >> 15).all()          # both precisions occur
        want = api.bsc_qlfc_encode_block(sub, coder=3)
        assert want == ref.qlfc_encode_block(sub, 3)
        pre = gpu.rc_prefix(ri.first_seen(sub), sub.size, 3)
        assert _one(ri.FAST16, tr, pre, tr.size, sub.size) == want, (k, sub.size)


def _alphabet_bits(fs):
    """the alphabet header restated from the decoder's side: per slot the next new symbol, bit by bit from the top, a bit being coded
    only where both values are still possible among the symbols not used yet (or the previous one, which ends the list)"""
    used, prev, bits = set(), -1, []
    for slot in range(256):
        cur = int(fs[slot]) if slot < len(fs) else int(fs[-1])
        for b in range(7, -1, -1):
            cand = [c for c in range(256) if (c == prev or c not in used) and (c >> (b + 1)) == (cur >> (b + 1))]
            if any(c >> b & 1 for c in cand) and any(not (c >> b & 1) for c in cand):
                bits.append(cur >> b & 1)
        if cur == prev:
            break
        prev = cur
        used.add(cur)
    return bits


@pytest.mark.parametrize("nsym", [1, 2, 17, 256])
def test_rc_prefix(nsym, ref, orc):
    rng = np.random.default_rng(nsym)
    fs = rng.permutation(256)[:nsym].astype(np.uint8)
    in_size = 123_456 + nsym
    bits = [in_size >> b & 1 for b in range(31, -1, -1)] + _alphabet_bits(fs)
    st, fa = gpu.rc_prefix(fs, in_size, 1), gpu.rc_prefix(fs, in_size, 3)
    assert st.size == fa.size == len(bits) <= gpu.RC_PREFIX_MAX
    assert ((st >> 24) & 1).tolist() == bits and ((fa >> 24) & 1).tolist() == bits
    assert (st & 0xffffff == (12 << 16 | 2048)).all() and not (st >> 25).any()          # encode_half
    assert (fa[:32] == st[:32]).all() and (fa[32:] & 0xffffff == (1 << 16 | 1)).all()   # the fast coder's alphabet: precision 1, p 1
    # and inside a real stream: a sub-block with exactly these symbols, in this order of first appearance
    sub = np.concatenate([fs, fs[rng.integers(0, nsym, 3000)]])
    tr, _ = orc.static_pstream(sub)
    pre = gpu.rc_prefix(ri.first_seen(sub), sub.size, 1)
    want = ref.qlfc_encode_block(sub, 1, out_size=2 * sub.size)
    assert isinstance(want, bytes) and _one(ri.STATIC16, tr, pre, tr.size, 2 * sub.size) == want
    # bad arguments
    L = gpu.N.lib()
    buf = np.zeros(8, np.uint32)
    assert L.bscgpu_rc_prefix(gpu.N.np_ptr(fs), nsym, in_size, 2, gpu.N.np_ptr(buf), 8) == -1        # the adaptive coder has no p stream
    assert L.bscgpu_rc_prefix(gpu.N.np_ptr(fs), nsym, 0, 1, gpu.N.np_ptr(buf), 8) == -1
    assert L.bscgpu_rc_prefix(gpu.N.np_ptr(fs), nsym, in_size, 1, gpu.N.np_ptr(buf), 8) == -1        # cap too small
    assert L.bscgpu_rc_prefix(gpu.N.np_ptr(fs), nsym, in_size, 1, None, 0) == len(bits)              # asking for the count


def test_steered_stream_carries_into_pending_units():
    e, t = ri.steered(5, 20_000)
    assert t.carries2 >= 100 and t.longest >= 4, (t.carries, t.carries2, t.longest)
    want = t.finish()
    got = _one(ri.STATIC16, e, np.zeros(0, np.uint32), e.size, len(want) + 4096)
    assert got == want
    assert _one(ri.STATIC13, ri.pack_p13(e), np.zeros(0, np.uint32), e.size, len(want) + 4096) == want


def test_coin_flips_do_not_fit():
    n = 64_000
    for form in (ri.STATIC16, ri.STATIC13, ri.FAST16):
        e = ri.coin_flips(n, ri.FAST16 if form == ri.FAST16 else ri.STATIC16)
        body = ri.pack_p13(e) if form == ri.STATIC13 else e
        assert _one(form, body, np.zeros(0, np.uint32), n, n // 16) == ri.NOT_COMPRESSIBLE, form
        r = _one(form, body, np.zeros(0, np.uint32), n, n)                   # one bit per decision: n / 8 bytes and the coder's slack
        assert isinstance(r, bytes) and n // 8 <= len(r) <= n // 8 + 8, form


def test_a_stream_never_leaves_its_region():
    """no run-start mark anywhere: the 16-bit forms' own budget test never fires, the stage's bound does — and nothing is written behind
    out_size + 64 bytes; streams laid out back to back, a canary behind each"""
    rng = np.random.default_rng(3)
    e = ri.random_static(rng, 20_000) & np.uint16(0x1fff)
    st, nbody, nout = ri.lay_out([5000, 5000, 5000], [100, 3000, 0], canary=32)
    canary = np.full(nout, 0xa5, np.uint8)
    res, out = gpu.rc_encode_host(ri.STATIC16, e, np.zeros(0, np.uint32), st, out=canary)
    assert res[0] == ri.NOT_COMPRESSIBLE and res[2] == ri.NOT_COMPRESSIBLE and res[1] > 500
    assert out[st[1][4]:st[1][4] + res[1]].tobytes() == ri.twin_bytes([], e[5000:10000])
    for s in st:
        assert (out[s[4] + s[5] + 64:s[4] + s[5] + 64 + 32] == 0xa5).all()


def test_stream_shapes_are_checked():
    e = np.zeros(100, np.uint16)
    bad = [[(0, 10, 0, 0, 1, 100)],            # odd out_off
           [(0, 10, 0, 1, 0, 100)],            # prefix range outside the prefix array
           [(95, 10, 0, 0, 0, 100)],           # body outside the array
           [(0, 10, 0, 0, 0, -1)]]             # negative out_size
    for st in bad:
        with pytest.raises(gpu.GpuError):
            gpu.rc_encode_host(ri.STATIC16, e, np.zeros(0, np.uint32), st, out=np.zeros(400, np.uint8))
    with pytest.raises(gpu.GpuError):
        gpu.rc_encode_host(ri.STATIC13, np.zeros(100, np.uint8), np.zeros(0, np.uint32), [(4, 8, 0, 0, 0, 100)])      # not a multiple of 8
    with pytest.raises(gpu.GpuError):
        gpu.rc_encode_host(3, e, np.zeros(0, np.uint32), [(0, 10, 0, 0, 0, 100)])
    res, out = gpu.rc_encode_host(ri.STATIC16, e, np.zeros(0, np.uint32), [])
    assert res == [] and out.size == 0
    res, out = gpu.rc_encode_host(ri.STATIC16, e, np.zeros(0, np.uint32), [(0, 0, 0, 0, 0, 100)])             # an empty stream: finish alone
    assert out[:res[0]].tobytes() == ri.Twin().finish()
