"""The host arithmetic of the LZP stage over a pass (csrc/host/lzp_batch_plan.h; DESIGN §3.9, "A pass of small blocks"), no GPU: the chunk
table (bscgpu_lzp_batch_plan) against lzp_staged.h's cut rule per block, and the piece list (bscgpu_lzp_batch_frame): every block's
stream rebuilt on the CPU from the pieces, with the staging bytes of the stand-in's sweep per chunk, must be api.bsc_lzp_compress's."""
import numpy as np
import pytest

import lzp_batch_inputs as B
import lzp_device_inputs as I
from libbsc_amd import api, gpu

KIB256, MIB = 256 * 1024, 1 << 20


# ---- the chunk table ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("min_len", [4, 255])
def test_plan_equals_the_cut_rule_per_block(min_len):
    sizes = [0, 1, 28, 29, min_len + 31, min_len + 32, 17, 18, KIB256 - 1, KIB256, KIB256 + 1, 0, MIB - 1, 5000, min_len + 31, 300_000]
    got = gpu.lzp_batch_plan(sizes, min_len)
    assert got == B.plan(sizes, min_len)
    by_block = {}
    for b, start, size, cap in got:
        by_block.setdefault(b, []).append((start, size, cap))
    off = np.concatenate([[0], np.cumsum(sizes)])
    for b, n in enumerate(sizes):
        if n - min_len < 32 or n - 2 < 16:
            assert b not in by_block, (b, n, "a refused size owns no chunk")
            continue
        nc = B.num_chunks(n)
        assert [s for s, _, _ in by_block[b]] == [int(off[b]) + B.chunk_start(n, nc, i) for i in range(nc)]
        assert [s for _, s, _ in by_block[b]] == [B.chunk_size(n, nc, i) for i in range(nc)]
        assert sum(s for _, s, _ in by_block[b]) == n
        assert [c for _, _, c in by_block[b]] == ([n - 2] if nc == 1 else [B.chunk_size(n, nc, i) for i in range(nc)])
    # the boundary of the refusal, and the last chunk one byte longer
    assert (sizes.index(min_len + 31) in by_block, sizes.index(min_len + 32) in by_block) == (False, True)
    assert 6 not in by_block and 7 not in by_block                             # 17: n - 2 < 16; 18: n - minLen < 32 for every minLen
    assert [s for _, s, _ in by_block[sizes.index(KIB256 + 1)]] == [KIB256 // 2, KIB256 // 2 + 1]
    assert len(by_block[sizes.index(KIB256 - 1)]) == 1 and len(by_block[sizes.index(KIB256)]) == 2 and len(by_block[sizes.index(MIB - 1)]) == 2


def test_plan_limits():
    assert gpu.lzp_batch_plan([], 32) == []
    assert gpu.lzp_batch_plan([MIB - 1], 32) == B.plan([MIB - 1], 32)
    assert gpu.lzp_batch_plan([MIB], 32) == api.BAD_PARAMETER, "a block of 1 MiB is no block of a pass"
    assert gpu.lzp_batch_plan([100, -1, 100], 32) == api.BAD_PARAMETER
    got = gpu.lzp_batch_plan([100] * 4096, 32)
    assert len(got) == 4096 and got[-1] == (4095, 409_500, 100, 98)
    assert gpu.lzp_batch_plan([100] * 4097, 32) == api.BAD_PARAMETER
    full = gpu.lzp_batch_plan([KIB256] * 4096, 32)
    assert len(full) == gpu.LZP_BATCH_MAX_CHUNKS == 8192, "the table's last entry"
    assert full[-1] == (4095, 4095 * KIB256 + KIB256 // 2, KIB256 // 2, KIB256 // 2)
    assert gpu.lzp_batch_plan([MIB - 1] * 2047, 32) != api.BAD_PARAMETER
    assert gpu.lzp_batch_plan([MIB - 1] * 2049, 32) == api.BAD_PARAMETER, "positions of a pass are below 2^31 - 1"
    for m in (3, 256):
        assert gpu.lzp_batch_plan([1000], m) == api.BAD_PARAMETER


# ---- the piece list -------------------------------------------------------------------------------------------------------------------------
def _rebuild(blocks, h, m, f):
    """plan -> the stand-in's sweep per chunk -> frame -> every block's stream from the pieces; -> (streams, results, raw chunks)"""
    sizes = B.sizes_of(blocks)
    T = B.joined(blocks)
    table = gpu.lzp_batch_plan(sizes, m)
    staging = np.zeros(T.size + 16, np.uint8)
    own = []
    for _, start, size, cap in table:
        got, _ = gpu.lzp_chunk_staged_host(T[start:start + size], cap, h, m)
        own.append(got if isinstance(got, int) else len(got))
        if not isinstance(got, int):
            staging[start:start + len(got)] = np.frombuffer(got, np.uint8)
    results, pieces, tab, raw = gpu.lzp_batch_frame(sizes, m, f, own)
    out = np.full(T.size, 0xA5, np.uint8)
    written = np.zeros(T.size, np.int32)
    sources = {gpu.PIECE_STAGING: staging, gpu.PIECE_RAW: T, gpu.PIECE_TABLE: tab}
    for src, so, do, ln in pieces:
        assert ln > 0 and so + ln <= sources[src].size and do + ln <= T.size, "a piece stays inside its source and the output"
        out[do:do + ln] = sources[src][so:so + ln]
        written[do:do + ln] += 1
    off = np.concatenate([[0], np.cumsum(sizes)])
    streams = []
    for b, r in enumerate(results):
        lo = int(off[b])
        if r >= 0:
            assert (written[lo:lo + r] == 1).all() and not written[lo + r:int(off[b + 1])].any(), (b, "the pieces tile the block's stream")
            streams.append(out[lo:lo + r].tobytes())
        else:
            assert not written[lo:int(off[b + 1])].any(), (b, "a block without a stream gets no piece")
            streams.append(r)
    assert len(pieces) <= 3 * len(sizes)
    return streams, results, raw


@pytest.mark.parametrize("features", I.FEATURES)
def test_pieces_rebuild_the_host_encoders_streams(features):
    """a raw first chunk, a raw second chunk, a block that is not compressible, single chunks, refused and empty blocks"""
    blocks = (B.raw_pass() + [("empty", np.zeros(0, np.uint8)), ("text", I.corpora()["text"]), ("short", I.corpora()["text"][:40])]
              + B.neighbours_pass()[2:] + [("f2_runs", I.corpora()["f2_runs"])])
    for h, m in ((15, 32), (10, 8), (15, 128)):
        streams, results, raw = _rebuild(blocks, h, m, features)
        assert streams == B.wants(blocks, h, m, features), (h, m)
        assert raw == B.staged_counters(blocks, h, m, features)["raw_chunks"]
        if (h, m) == (15, 32):
            assert results[2] == api.NOT_COMPRESSIBLE and results[3] == api.NOT_COMPRESSIBLE and results[5] == api.NOT_COMPRESSIBLE
            assert raw >= 2, "both raw chunks are there"


@pytest.mark.parametrize("features", I.FEATURES)
def test_pieces_of_random_results(features):
    """random own[] for random sizes: what every block gets is frame_from_own's answer for it alone, its pieces tile exactly its stream
    and read only the chunk they belong to"""
    rng = np.random.default_rng(31 + features)
    for it in range(40):
        sizes = [int(rng.choice([0, 20, 40, 5000, KIB256 - 1, KIB256, 300_001, MIB - 1])) for _ in range(int(rng.integers(1, 12)))]
        m = int(rng.choice([4, 32, 255]))
        table = gpu.lzp_batch_plan(sizes, m)
        own = [api.NOT_COMPRESSIBLE if rng.random() < 0.35 else int(rng.integers(4, max(5, cap - 8))) for _, _, _, cap in table]
        results, pieces, tab, raw = gpu.lzp_batch_frame(sizes, m, features, own)
        off = np.concatenate([[0], np.cumsum(sizes)])
        chunks_of = {}
        for k, (b, start, size, cap) in enumerate(table):
            chunks_of.setdefault(b, []).append((start, size, own[k]))
        covered = np.zeros(int(off[-1]) + 1, np.int32)
        tab_at, raw_alone = 0, 0
        for b, n in enumerate(sizes):
            mine = [p for p in pieces if off[b] <= p[2] < off[b + 1]]
            ch = chunks_of.get(b, [])
            alone = gpu.lzp_batch_frame([n], m, features, [o for _, _, o in ch])
            assert results[b] == alone[0][0], (it, b)
            raw_alone += alone[3]
            if results[b] < 0:
                assert not mine
                continue
            assert mine[0][0] == gpu.PIECE_TABLE and mine[0][1] == tab_at and mine[0][2] == off[b] and mine[0][3] == (1 if len(ch) == 1 else 17)
            assert tab[tab_at] == len(ch)
            tab_at += mine[0][3]
            at = int(off[b]) + mine[0][3]
            payload = mine[1:]
            assert len(payload) == len(ch)
            for (src, so, do, ln), (start, size, o) in zip(payload, ch):
                assert do == at and so == start, (it, b)
                kept_raw = src == gpu.PIECE_RAW
                assert ln == (size if kept_raw else o) and (len(ch) > 1 or not kept_raw)
                if len(ch) > 1:
                    i = ch.index((start, size, o))
                    assert int.from_bytes(bytes(tab[tab_at - 17 + 1 + 8 * i:tab_at - 17 + 9 + 8 * i]), "little") == size + (ln << 32)
                at += ln
            assert at == off[b] + results[b]
            covered[int(off[b]):at] += 1
        assert covered.max(initial=0) <= 1
        assert raw == raw_alone, it
