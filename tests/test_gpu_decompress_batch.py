"""Batched decompression (bscgpu_unbwt_batch_device / bscgpu_decompress_batch*): every block must decode exactly as it does alone —
the inverse BWT against the texts the reference's forward BWT came from, whole blocks against bsc_decompress and the originals."""
import numpy as np
import pytest

from test_gpu_device import _corpus
from test_gpu_batch import _hazards

pytestmark = pytest.mark.gpu

MIB = 1 << 20


@pytest.fixture(scope="module")
def dctx():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from libbsc_amd import GpuContext
    c = GpuContext(0, max_n=(16 << 20) + 4096)
    yield c
    c.close()


def _flat(arrs):
    return np.concatenate(arrs) if sum(a.size for a in arrs) else np.zeros(1, np.uint8)


def test_unbwt_batch_matches_reference(dctx, ref):
    import torch
    rng = np.random.default_rng(4)
    cases = [c[1] for c in _corpus(rng) if c[1].size < 4 * MIB] + [c[1] for c in _hazards(rng)]
    enc = [ref.bwt_encode(T, aux=False) for T in cases]
    order = rng.permutation(len(cases))
    for k in range(3):                       # several batches: the same block beside different neighbours
        part = [int(i) for i in order[k::3]]
        Ls = [np.asarray(enc[i][0][:cases[i].size], np.uint8) for i in part]
        prim = [enc[i][1] for i in part]
        dL = torch.from_numpy(_flat(Ls)).cuda()
        T, res = dctx.unbwt_batch(dL, [cases[i].size for i in part], prim)
        Th = T.cpu().numpy()
        o = 0
        for j, i in enumerate(part):
            n = cases[i].size
            if prim[j] <= 0 or prim[j] > n:
                assert res[j] == -1, (n, prim[j], res[j])
            else:
                assert res[j] == 0, (n, res[j])
                assert np.array_equal(Th[o:o + n], cases[i]), f"n={n}: text differs"
            o += n


def test_unbwt_batch_isolates_bad_blocks(dctx, ref):
    import torch
    from libbsc_amd.synth import synth_text_v1
    from unbwt_inputs import lf_verdict
    texts = [synth_text_v1(50 + i, n) for i, n in enumerate([3000, 70000, 400000, 65536, 129, 250000, 17])]
    enc = [ref.bwt_encode(T, aux=False) for T in texts]
    Ls = [np.asarray(e[0][:t.size], np.uint8).copy() for e, t in zip(enc, texts)]
    prim = [e[1] for e in enc]
    bad_prim, bad_col = 2, 5
    prim[bad_prim] = prim[bad_prim] + 1 if prim[bad_prim] < texts[bad_prim].size else prim[bad_prim] - 1
    Ls[bad_col][1000:1100] = Ls[bad_col][5000:5100]
    sizes = [t.size for t in texts]
    offs = np.concatenate([[0], np.cumsum(sizes)])
    dL = torch.from_numpy(_flat(Ls)).cuda()
    dT = torch.full((int(offs[-1]),), 0xAB, dtype=torch.uint8, device=dL.device)
    _, res = dctx.unbwt_batch(dL, sizes, prim, dT=dT)
    Th = dT.cpu().numpy()
    for b, T in enumerate(texts):
        got = Th[offs[b]:offs[b + 1]]
        if b in (bad_prim, bad_col):
            want_rc, want = lf_verdict(Ls[b], prim[b])             # the plain LF walk's verdict (tests/unbwt_inputs.py)
            assert res[b] == want_rc and (res[b] != 0 or np.array_equal(got, want)), (b, res[b])
            if res[b] == -6:
                assert (got == 0xAB).all(), f"block {b} failed but wrote its range"
        else:
            assert res[b] == 0 and np.array_equal(got, T), f"block {b} beside the bad ones"


def _blocks(ref, coder, lzp):
    """the reference's blocks (BWT, ST3..ST6, stored, tiny, empty) and ours for ST7 / ST8 -> (originals, blocks)"""
    from libbsc_amd import api
    from libbsc_amd.synth import synth_text_v1
    rng = np.random.default_rng(coder * 13 + lzp[0])
    datas, blocks = [], []
    for i, n in enumerate(rng.integers(2000, 150000, 8)):
        d = synth_text_v1(60 + i, int(n))
        datas.append(d); blocks.append(ref.compress(d, 1, coder, lzp[0], lzp[1]))
    for k in (3, 4, 5, 6):
        d = synth_text_v1(70 + k, 40000 + 1000 * k)
        datas.append(d); blocks.append(ref.compress(d, k, coder, lzp[0], lzp[1]))
    for k in (7, 8):
        d = synth_text_v1(80 + k, 30000)
        datas.append(d); blocks.append(api.bsc_compress(d, k, coder, lzp[0], lzp[1]))
    for d in (rng.integers(0, 256, 20000, dtype=np.uint8), synth_text_v1(90, 28), synth_text_v1(91, 5), np.zeros(0, np.uint8),
              synth_text_v1(92, 65536), synth_text_v1(93, 65535)):
        datas.append(d); blocks.append(ref.compress(d, 1, coder, lzp[0], lzp[1]))
    for b in blocks:
        assert isinstance(b, bytes), b
    return datas, blocks


@pytest.mark.parametrize("coder", [1, 2, 3])
@pytest.mark.parametrize("lzp", [(0, 0), (15, 128)])
def test_decompress_batch_matches_reference_blocks(dctx, ref, coder, lzp):
    from libbsc_amd import api
    datas, blocks = _blocks(ref, coder, lzp)
    got = dctx.decompress_batch(blocks)
    for d, blk, g in zip(datas, blocks, got):
        assert g == d.tobytes(), f"n={d.size} coder={coder} lzp={lzp}: {g if isinstance(g, int) else 'bytes differ'}"
        assert g == api.bsc_decompress(blk)
    T, offs, res = dctx.decompress_batch_device(blocks)
    assert res == [0] * len(blocks)
    Th = T.cpu().numpy()
    for b, d in enumerate(datas):
        assert Th[offs[b]:offs[b + 1]].tobytes() == d.tobytes(), f"device output, block {b}"


def test_round_trip_of_compress_batch(dctx):
    from libbsc_amd.synth import synth_text_v1
    rng = np.random.default_rng(8)
    datas = [synth_text_v1(100 + i, int(n)) for i, n in enumerate(rng.integers(1, 300000, 40))]
    for lzp in ((0, 0), (15, 128)):
        blocks = dctx.compress_batch(datas, 1, 2, lzp[0], lzp[1])
        assert dctx.decompress_batch(blocks) == [d.tobytes() for d in datas]


def test_damaged_blocks_get_their_own_error(dctx, ref):
    from libbsc_amd import api
    from libbsc_amd.synth import synth_text_v1
    datas = [synth_text_v1(200 + i, 50000 + 7000 * i) for i in range(6)]
    blocks = [ref.compress(d, 1, 1) for d in datas]
    broken = bytearray(blocks[1]); broken[100] ^= 0x55            # payload checksum no longer matches
    blocks[1] = bytes(broken)
    blocks[3] = blocks[3][:-5]                                     # a truncated in_sizes[b]
    blocks[4] = blocks[4][:20]                                     # shorter than a header
    got = dctx.decompress_batch(blocks)
    for b, (d, blk) in enumerate(zip(datas, blocks)):
        want = api.bsc_decompress(blk)
        if b in (1, 3, 4):
            assert isinstance(want, int) and got[b] == want, (b, got[b] if isinstance(got[b], int) else "bytes", want)
        else:
            assert got[b] == d.tobytes(), b
    _, _, res = dctx.decompress_batch_device(blocks)
    assert [r for b, r in enumerate(res) if b in (1, 3, 4)] == [api.bsc_decompress(blocks[b]) for b in (1, 3, 4)]
    assert [r for b, r in enumerate(res) if b not in (1, 3, 4)] == [0, 0, 0]


def _seal(b, size=True):
    import struct
    from libbsc_amd import api
    if size:
        b[0:4] = struct.pack("<i", len(b))
    b[20:24] = struct.pack("<I", api.bsc_adler32(np.frombuffer(bytes(b[28:]), np.uint8)))
    b[24:28] = struct.pack("<I", api.bsc_adler32(np.frombuffer(bytes(b[:24]), np.uint8)))
    return bytes(b)


def test_sealed_damage_reaches_the_batched_route(dctx, ref):
    """Damaged blocks whose checksums were repaired (the recipe of test_decompress_survives_corrupt_streams, plus directed edits of the
    primary index and the aux-index count) pass every check in front of the GPU pass: garbage reaches the QLFC decoders and the
    batched inverse BWT.  Interleaved with clean blocks in one call, every block must come back exactly as bsc_decompress returns it
    alone — the error code or the bytes.  (The reference's decoder is not asked: it has no chain check.)  Random edits start at
    offset 8: blockSize is rewritten anyway, and dataSize only decides how much the caller allocates."""
    import struct
    from libbsc_amd import api
    from libbsc_amd.synth import synth_text_v1
    rng = np.random.default_rng(78)
    src = []
    for i, (coder, lzp, n) in enumerate([(1, (0, 0), 2000), (2, (0, 0), 70_000), (3, (0, 0), 9001), (1, (15, 128), 40_000),
                                         (2, (15, 128), 5000), (3, (15, 128), 23_456)]):
        T = synth_text_v1(400 + i, n)
        if lzp[0]:
            T = np.concatenate([T, T[:n // 2], T[n // 3:]])[:70_000]       # something for LZP to find
        src.append((T, ref.compress(T, 1, coder, lzp[0], lzp[1])))
        assert isinstance(src[-1][1], bytes) and api.bsc_decompress(src[-1][1]) == T.tobytes()
    damaged = []
    for it in range(114):
        b = bytearray(src[it % len(src)][1])
        for _ in range(int(rng.integers(1, 4))):
            mode = int(rng.integers(0, 4)); pos = int(rng.integers(8, len(b)))
            if mode == 0: b[pos] ^= 1 << int(rng.integers(0, 8))
            elif mode == 1: b[pos] = int(rng.integers(0, 256))
            elif mode == 2 and len(b) > 40: del b[pos]
            else: b.insert(pos, int(rng.integers(0, 256)))
        damaged.append(_seal(b, size=bool(rng.integers(0, 4))))
    for T, blk in src:                                                    # directed header edits
        index = struct.unpack("<i", blk[12:16])[0]
        for value in (0, T.size + 1, -1, index - 1, index + 1):
            b = bytearray(blk)
            b[12:16] = struct.pack("<i", value)
            damaged.append(_seal(b))
        b = bytearray(blk)
        b[-1] = min(b[-1] + 1 + int(rng.integers(0, 4)), 255)             # more aux indexes than the block has
        damaged.append(_seal(b))
        if blk[-1] > 0:                                                   # (blocks from 64 KiB on carry aux indexes)
            b = bytearray(blk)                                            # an aux index moved: a shortcut, not data — the block still decodes
            b[-5:-1] = struct.pack("<i", struct.unpack("<i", blk[-5:-1])[0] ^ 1)
            damaged.append(_seal(b))
            assert api.bsc_decompress(damaged[-1]) == T.tobytes()
    assert len(damaged) == 152
    blocks, clean_of = [], {}
    for i, d in enumerate(damaged):                                       # damaged and clean blocks alternate
        blocks.append(d)
        clean_of[len(blocks)] = src[i % len(src)][0]
        blocks.append(src[i % len(src)][1])
    want = [api.bsc_decompress(blk) for blk in blocks]
    codes = sorted({w for w in want if isinstance(w, int)})
    decoded = sum(1 for b, w in enumerate(want) if b not in clean_of and not isinstance(w, int))
    print("error codes met:", codes, "damaged blocks that decode:", decoded)
    assert any(isinstance(w, int) for w in want)
    got = dctx.decompress_batch(blocks)
    for b, (g, w) in enumerate(zip(got, want)):
        assert g == w, (b, g if isinstance(g, int) else "bytes", w if isinstance(w, int) else "bytes")
        if b in clean_of:
            assert g == clean_of[b].tobytes(), b
    T, offs, res = dctx.decompress_batch_device(blocks)
    assert res == [w if isinstance(w, int) else 0 for w in want]
    Th = T.cpu().numpy()
    for b, w in enumerate(want):
        if not isinstance(w, int):
            assert Th[offs[b]:offs[b + 1]].tobytes() == w, f"device output, block {b}"


def test_many_passes_and_the_single_block_path(ref):
    """max_n = 4 MiB: 2500 blocks take many passes, a 3 MiB block fills a pass of its own, a 6 MiB block takes bsc_decompress"""
    from libbsc_amd import GpuContext, api
    from libbsc_amd.synth import synth_text_v1
    rng = np.random.default_rng(12)
    sizes = [int(x) for x in rng.integers(1, 24000, 2500)]
    text = synth_text_v1(300, sum(sizes))
    offs = np.concatenate([[0], np.cumsum(sizes)])
    datas = [text[offs[b]:offs[b + 1]].copy() for b in range(len(sizes))]
    c = GpuContext(0, max_n=4 << 20)
    try:
        blocks = c.compress_batch(datas, 1, 1)
        big3, big6 = synth_text_v1(301, 3 * MIB), synth_text_v1(302, 6 * MIB)
        datas[1200:1200] = [big3]; blocks[1200:1200] = [api.bsc_compress(big3, 1, 1)]
        datas[1800:1800] = [big6]; blocks[1800:1800] = [api.bsc_compress(big6, 1, 1)]
        got = c.decompress_batch(blocks)
        assert got == [d.tobytes() for d in datas]
        T, o, res = c.decompress_batch_device(blocks)
        assert res == [0] * len(blocks)
        assert T.cpu().numpy().tobytes() == b"".join(d.tobytes() for d in datas)
    finally:
        c.close()


def test_bad_arguments(dctx):
    from libbsc_amd import _native as N
    L = N.lib()
    d = np.frombuffer(dctx.compress_batch([np.arange(100, dtype=np.uint8)])[0], np.uint8).copy()
    isz = np.array([d.size], np.int32)
    out = np.full(200, 0xAB, np.uint8)
    res = np.full(1, 12345, np.int32)
    neg = np.array([-3], np.int32)
    assert L.bscgpu_decompress_batch(dctx.h, N.np_ptr(d), N.np_ptr(isz), -1, N.np_ptr(out), 200, N.np_ptr(res), 3) == -1
    assert L.bscgpu_decompress_batch(dctx.h, None, N.np_ptr(isz), 1, N.np_ptr(out), 200, N.np_ptr(res), 3) == -1
    assert L.bscgpu_decompress_batch(dctx.h, N.np_ptr(d), None, 1, N.np_ptr(out), 200, N.np_ptr(res), 3) == -1
    assert L.bscgpu_decompress_batch(dctx.h, N.np_ptr(d), N.np_ptr(isz), 1, None, 200, N.np_ptr(res), 3) == -1
    assert L.bscgpu_decompress_batch(dctx.h, N.np_ptr(d), N.np_ptr(isz), 1, N.np_ptr(out), 200, None, 3) == -1
    assert L.bscgpu_decompress_batch(None, N.np_ptr(d), N.np_ptr(isz), 1, N.np_ptr(out), 200, N.np_ptr(res), 3) == -1
    assert L.bscgpu_decompress_batch(dctx.h, N.np_ptr(d), N.np_ptr(neg), 1, N.np_ptr(out), 200, N.np_ptr(res), 3) == -1
    assert L.bscgpu_decompress_batch(dctx.h, N.np_ptr(d), N.np_ptr(isz), 1, N.np_ptr(out), 99, N.np_ptr(res), 3) == -1
    assert L.bscgpu_decompress_batch_device(dctx.h, N.np_ptr(d), N.np_ptr(isz), 1, None, 200, N.np_ptr(res), 3) == -1
    ds = np.full(1, 777, np.int32)
    assert L.bscgpu_decompress_batch_sizes(N.np_ptr(d), N.np_ptr(neg), 1, N.np_ptr(ds)) == -1
    prim = np.array([5], np.int32)
    assert L.bscgpu_unbwt_batch_device(dctx.h, None, None, N.np_ptr(isz), 1, N.np_ptr(prim), N.np_ptr(res)) == -1
    assert (out == 0xAB).all() and (res == 12345).all() and (ds == 777).all(), "a refused call wrote something"
    assert L.bscgpu_decompress_batch_sizes(N.np_ptr(d), N.np_ptr(isz), 1, N.np_ptr(ds)) == 100 and ds[0] == 100
    assert L.bscgpu_decompress_batch(dctx.h, N.np_ptr(d), N.np_ptr(isz), 1, N.np_ptr(out), 100, N.np_ptr(res), 3) == 0
    assert res[0] == 0 and (out[:100] == np.arange(100)).all()
