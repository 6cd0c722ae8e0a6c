"""The block format in one header (libbsc_amd/csrc/host/container.h: fields, block header and trailer, the sub-block table written under
the parallel and the serial rule and read back) judged on the CPU through tools/container_probe.cpp: against the restatement in
pipeline_model (written from the reference's layout, not from the header), against bsc_block_info / bsc_decompress of the built
library, over a fixed-seed sweep and a hand-written table of the edges; the probe once more under AddressSanitizer + UBSan."""
import json
import os
import random
import struct
import subprocess

import numpy as np
import pytest

import pipeline_model as M
from libbsc_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = lambda nb: 1 + 8 * nb


def build_probe(exe, extra=()):
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", *extra, "-I", os.path.join(ROOT, "libbsc_amd", "csrc", "host"),
                    os.path.join(ROOT, "tools", "container_probe.cpp"), "-o", exe], check=True)


def asker(exe):
    def ask(lines):
        r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        out = [json.loads(l) for l in r.stdout.splitlines()]
        assert len(out) == len(lines)
        return out
    return ask


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("container_probe") / "container_probe")
    build_probe(exe)
    return asker(exe)


hx = lambda b: bytes(b).hex() or "-"
ints = lambda *v: " ".join(str(int(x)) for x in v)
frame = lambda cmd, n, size, res: f"{cmd} {n} {len(size)} {ints(*size)} {ints(*res)}"
payload_of = lambda g: g["result"] if g["result"] < 0 else bytes.fromhex(g["bytes"])


# ---- fields, header, stored and coded blocks ------------------------------------------------------------------------------------------
def test_header_and_mode_word_round_trip(probe):
    rng = random.Random(20261020)
    rows = [(28, 0, 0, 0, 1, 1), (0x7fffffff, 0x7fffffff, M.mode_pack(8, 3, 28, 255), 0x7fffffff, 0xffffffff, 0xfffffffe)]
    rows += [(rng.randrange(1 << 31), rng.randrange(1 << 31), M.mode_pack(rng.choice([0, 1, 3, 8]), rng.randrange(4), *rng.choice([(0, 0), (10, 4), (16, 128), (28, 255)])),
              rng.randrange(1 << 31), rng.randrange(1 << 32), rng.randrange(1 << 32)) for _ in range(50)]
    for row, g in zip(rows, probe(["H " + ints(*row) for row in rows])):
        assert bytes.fromhex(g["bytes"]) == M.block_header(*row), row
        assert (g["ok"], g["fields"], g["mode"], g["repacked"]) == (1, list(row), M.mode_unpack(row[2]), row[2]), row
        assert g["lzp"] == (M.mode_unpack(row[2])[2:] != [0, 0])
    # one bit of every byte of a header: its checksum says so, and so does bsc_block_info
    good = M.block_header(1000 + 28, 1000, M.mode_pack(1, 1, 0, 0), 17, 5, 6)
    bad = [good[:i] + bytes([good[i] ^ 0x10]) + good[i + 1:] for i in range(28)]
    for b, g in zip(bad, probe(["R " + hx(b) for b in bad])):
        assert g["ok"] == 0 and api.bsc_block_info(b)[0] == api.DATA_CORRUPT
    assert api.bsc_block_info(good) == (0, 1028, 1000)
    assert [g["rate"] for g in probe([f"A {n}" for n in (0, 1, 15, 16, 17, 31, 32, 65535, 65536, (1 << 30) + 5)])] == \
           [M.aux_rate(n) for n in (0, 1, 15, 16, 17, 31, 32, 65535, 65536, (1 << 30) + 5)] == [1, 1, 1, 2, 2, 2, 4, 4096, 8192, 1 << 27]


def test_stored_blocks_equal_bsc_store_and_decode(probe):
    rng = np.random.default_rng(2)
    datas = [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in (0, 1, 28, 29, 1000)]
    for d, g in zip(datas, probe(["S " + hx(d) for d in datas])):
        blk = bytes.fromhex(g["bytes"])
        assert g["result"] == len(d) + 28 and blk == M.stored_block(d) == api.bsc_store(d)
        assert api.bsc_block_info(blk) == (0, len(d) + 28, len(d))
        assert api.bsc_decompress(blk) == d


def test_coded_blocks_decode_and_the_store_rule_at_its_boundary(probe):
    """A coded block put together by the header — payload from the library's coder, BWT from the model — is what bsc_block_info and
    bsc_decompress of the library accept, with and without aux indexes; the reader gives the decoders' view of it.  The rule
    "coded + 1 + 4 * num >= n: store it" on both sides of its boundary, and a coder's negative code."""
    from libbsc_amd.synth import synth_text_v1
    T = synth_text_v1(11, 3000)
    r = M.aux_rate(T.size)
    L, primary, I, _, _ = M.bwt_model(T, r)
    payload = api.bsc_coder_compress(L, 1, features=1)
    assert isinstance(payload, bytes) and payload[0] == 1
    mode, adler = M.mode_pack(1, 1, 0, 0), api.bsc_adler32(T)
    for idx in ([], [int(x) - 1 for x in I[1:]]):
        line = f"C {T.size} {mode} {primary} {adler} {len(payload)} {len(idx)} {ints(*idx)} {hx(payload)}"
        g = probe([line])[0]
        blk = bytes.fromhex(g["bytes"])
        assert g["result"] == len(blk) == 28 + len(payload) + 4 * len(idx) + 1
        assert blk == M.coded_block(T.size, payload, mode, primary, idx, adler)
        assert api.bsc_block_info(blk) == (0, len(blk), T.size)
        assert api.bsc_decompress(blk) == T.tobytes()
        d = probe(["D " + hx(blk)])[0]
        want = M.coded_payload(blk)
        assert (d["ok"], d["result"], d["body_ok"]) == (1, 0, 1) and {k: d[k] for k in want} == want and d["num"] == len(idx)
        assert blk[d["indexes"]:d["indexes"] + 4 * len(idx)] == b"".join(struct.pack("<i", x) for x in idx)
        # a damaged body: the checksum's verdict, as bsc_decompress gives it
        hurt = blk[:40] + bytes([blk[40] ^ 1]) + blk[41:]
        d = probe(["D " + hx(hurt)])[0]
        assert (d["ok"], d["result"], d["body_ok"]) == (1, M.DATA_CORRUPT, 0) and M.coded_payload(hurt) == M.DATA_CORRUPT
        assert api.bsc_decompress(hurt) == api.DATA_CORRUPT
    # blocks the decoders refuse before any payload byte: no room for a payload byte and the count; more indexes than the body holds
    for body in (b"", b"\x00", b"\x01\x01", b"\x07" * 9 + b"\x03"):
        blk = M.block_header(28 + len(body), 100, mode, 1, 0, M._adler(body)) + body
        d = probe(["D " + hx(blk)])[0]
        assert (d["ok"], d["result"]) == (1, M.DATA_CORRUPT) and M.coded_payload(blk) == M.DATA_CORRUPT, body
        assert api.bsc_decompress(blk) == api.DATA_CORRUPT, body
    # the store rule: n_orig one above, at and one below coded + 1 + 4 * num; a negative code from the coder
    pay = bytes(range(50))
    rows = [(n, num, coded) for num in (0, 3) for n in (50 + 1 + 4 * num + 1, 50 + 1 + 4 * num, 50 + 4 * num) for coded in (50,)] + [(1000, 2, -3), (1000, 0, -2)]
    got = probe([f"C {n} {mode} 5 77 {coded} {num} {ints(*range(num))} {hx(pay)}" for n, num, coded in rows])
    for (n, num, coded), g in zip(rows, got):
        want = M.coded_block(n, pay, mode, 5, list(range(num)), 77, coded)
        assert payload_of(g) == want, (n, num, coded)
        assert (want == M.NOT_COMPRESSIBLE) == (coded < 0 or n <= 50 + 1 + 4 * num)


# ---- the sub-block table, writing ------------------------------------------------------------------------------------------------------
def framing_edges():
    """(n, size[], res-or-c[]): for the parallel framer and the verdict the third is res[] (res == size: raw), for the serial framer what
    the stand-in coder needs."""
    t2, t3 = TABLE(2), TABLE(3)
    rows = []
    for d in (-1, 0, 1):                                       # total exactly n - 1, n, n + 1
        rows.append((t2 + 300 + d, [400, 500], [100, 200]))
        rows.append((t3 + 600 + d, [400, 200, 300], [100, 200, 300]))          # ... with raw sub-blocks in it
    rows += [(5000, [400, 500, 600], [400, 100, 100]), (5000, [400, 500, 600], [100, 500, 100]), (5000, [400, 500, 600], [100, 100, 600])]   # raw first, middle, last
    for d in (-1, 0, 1):                                       # a raw last sub-block with optr + size exactly n - 1, n (and n + 1)
        rows.append((t2 + 100 + 500 - d, [400, 500], [100, 500]))
        rows.append((t3 + 400 + 50 + 300 - d, [400, 200, 300], [400, 50, 300]))
    for d in (0, 1, 2):                                        # room exactly size_b, size_b - 1 (and - 2) for the last and for a middle sub-block
        rows.append((t2 + 100 + 500 - d, [400, 500], [100, 499]))
        rows.append((t2 + 100 + 500 - d, [400, 500], [100, 498]))
        rows.append((t3 + 400 + 200 - d, [400, 200, 300], [400, 150, 10]))
        rows.append((t3 + 100 + 200 - d, [400, 200, 300], [100, 199, 10]))
    rows += [(10, [400, 500], [100, 200]), (t2, [400, 500], [0, 0]), (t2 + 1, [400, 500], [0, 0]), (100000, [1] * 8, [1] * 8), (100000, [3] * 8, [2] * 8)]
    return rows


def framing_sweep():
    rng = random.Random(20261020)
    rows = []
    for i in range(3000):
        nb = rng.randint(2, 8)
        size = [rng.randint(1, 400) for _ in range(nb)]
        c = [s if rng.random() < 0.25 else rng.randint(0, s + 1) if rng.random() < 0.2 else rng.randint(max(0, s - 3), s) if rng.random() < 0.2 else rng.randint(0, s // 2)
             for s in size]
        total = TABLE(nb) + sum(min(x, s) for x, s in zip(c, size))
        n = total + rng.choice([-1, 0, 1]) if rng.random() < 0.3 else sum(size) + rng.randint(-60, 90) if rng.random() < 0.6 else rng.randint(total - 300, total + 300)
        rows.append((max(n, 0), size, c))
    return rows


def held_to_the_restatement(probe, rows):
    seen = dict(par_ok=0, par_nc=0, ser_ok=0, ser_nc=0, ser_raw=0, ser_small_room=0, ser_room_cut_then_coded=0, exact=0, not_exact=0, incompressible=0)
    par = probe([frame("P", n, size, [min(x, s) for x, s in zip(c, size)]) for n, size, c in rows])
    ser = probe([frame("Q", n, size, c) for n, size, c in rows])
    ver = probe([frame("V", n, size, [min(x, s) for x, s in zip(c, size)]) for n, size, c in rows])
    for (n, size, c), p, q, v in zip(rows, par, ser, ver):
        res = [min(x, s) for x, s in zip(c, size)]
        want_p, (want_q, want_rooms), want_v = M.frame_parallel(n, size, res), M.frame_serial(n, size, c), M.serial_verdict(n, size, res)
        assert payload_of(p) == want_p, (n, size, res)
        assert payload_of(q) == want_q and q["rooms"] == want_rooms, (n, size, c)
        assert v["verdict"] == want_v, (n, size, res)
        # what the verdict claims, held to the serial framer itself
        if want_v == "exact":
            assert want_rooms == size and want_q == want_p != M.NOT_COMPRESSIBLE, (n, size, c)      # (every step of an exact walk ends below n)
        if want_v == "incompressible":
            assert want_q == M.NOT_COMPRESSIBLE, (n, size, c)
        seen["par_ok" if want_p != M.NOT_COMPRESSIBLE else "par_nc"] += 1
        seen["ser_ok" if want_q != M.NOT_COMPRESSIBLE else "ser_nc"] += 1
        seen[want_v] += 1
        if want_q != M.NOT_COMPRESSIBLE:
            coded = [struct.unpack_from("<i", want_q, 1 + 8 * b + 4)[0] for b in range(len(size))]
            seen["ser_raw"] += any(r == s for r, s in zip(coded, size))
            seen["ser_small_room"] += want_rooms != size
            seen["ser_room_cut_then_coded"] += any(r < s and k < s for r, s, k in zip(want_rooms, size, coded))
    return seen


def test_framers_and_verdict_equal_the_restatement_over_a_sweep(probe):
    seen = held_to_the_restatement(probe, framing_sweep())
    assert all(seen.values()), f"the sweep never reached: {[k for k, v in seen.items() if not v]}"


def test_framers_and_verdict_at_their_edges(probe):
    rows = framing_edges()
    held_to_the_restatement(probe, rows)
    t2 = TABLE(2)
    par = lambda n, size, res: payload_of(probe([frame("P", n, size, res)])[0])
    ser = lambda n, size, c: probe([frame("Q", n, size, c)])[0]
    ver = lambda n, size, res: probe([frame("V", n, size, res)])[0]["verdict"]
    # the parallel rule: a total of n - 1 is a payload, n and n + 1 are not
    assert [par(t2 + 300 + d, [400, 500], [100, 200]) == M.NOT_COMPRESSIBLE for d in (1, 0, -1)] == [False, True, True]
    assert len(par(t2 + 301, [400, 500], [100, 200])) == t2 + 300
    # the serial rule: a raw last sub-block that ends at n - 1 is kept, one that reaches n is not
    assert [ser(t2 + 600 + d, [400, 500], [100, 500])["result"] for d in (1, 0)] == [t2 + 600, M.NOT_COMPRESSIBLE]
    assert [ver(t2 + 600 + d, [400, 500], [100, 500]) for d in (1, 0, -1)] == ["exact", "incompressible", "not_exact"]
    # room exactly size_b: the sub-block is coded as on its own; size_b - 1: coded where it fits, else raw — which then reaches n
    g = ser(t2 + 600, [400, 500], [100, 499])
    assert (g["rooms"], g["result"], ver(t2 + 600, [400, 500], [100, 499])) == ([400, 500], t2 + 599, "exact")
    g = ser(t2 + 599, [400, 500], [100, 499])
    assert (g["rooms"], g["result"], ver(t2 + 599, [400, 500], [100, 499])) == ([400, 499], t2 + 599, "not_exact")
    g = ser(t2 + 598, [400, 500], [100, 499])
    assert (g["rooms"], g["result"], ver(t2 + 598, [400, 500], [100, 499])) == ([400, 498], M.NOT_COMPRESSIBLE, "not_exact")
    # a raw first sub-block makes the second's budget smaller than its size wherever n < table + both sizes
    assert ser(t2 + 800, [400, 500], [400, 100])["rooms"] == [400, 400] and ver(t2 + 800, [400, 500], [400, 100]) == "not_exact"


@pytest.mark.parametrize("coder", [1, 3])
def test_verdict_holds_against_the_reference_coder(probe, ref, coder):
    """serial_verdict over what the reference itself produced: its parallel frame (features 3) gives size[] and the res[] of sub-blocks
    coded on their own; where the verdict is 'exact' its serial frame (features 1) is byte for byte the parallel one, where it is
    'incompressible' its serial answer is LIBBSC_NOT_COMPRESSIBLE ('not_exact' claims nothing).  A raw last sub-block leaves every
    budget whole (exact); a raw first one leaves the second less than its size (not exact)."""
    from test_host_coder import _raw_sub_block_cases
    verdicts = {}
    for name, L in _raw_sub_block_cases():
        if name not in ("text+noise", "noise+text", "lowent600k"):
            continue
        par, ser = ref.coder_compress(L, coder, features=3), ref.coder_compress(L, coder, features=1)
        nb, subs, rc = M.subtable_parse(par, len(par), L.size)
        assert nb == 2 and rc == 0
        v = probe([frame("V", L.size, [s[1] for s in subs], [s[0] for s in subs])])[0]["verdict"]
        if v == "exact":
            assert ser == par, name
        if v == "incompressible":
            assert ser == api.NOT_COMPRESSIBLE, name
        verdicts[name] = v
    assert (verdicts["text+noise"], verdicts["noise+text"]) == ("exact", "not_exact"), verdicts


# ---- the sub-block table, reading -------------------------------------------------------------------------------------------------------
def table_cases():
    """(payload, in_size, max_out): a good two-sub-block payload and what can be wrong with one"""
    size, res = [300_000, 300_000], [100, 120]
    good = M.frame_parallel(1 << 20, size, res)
    n = len(good)

    def patched(field, value, data=good):
        b = bytearray(data)
        b[field:field + 4] = struct.pack("<i", value)
        return bytes(b)
    rows = [(good, n, 600_000), (good, n, 599_999), (good, n - 1, 600_000), (good, n + 0, 1 << 40)]
    # the cases of test_decompress_rejects_frame_tables_that_leave_the_payload: a coded size far past the payload, INT_MAX, the second
    # sub-block as long as the block, the first as long as the payload; a short payload announcing 16 MB; a table cut short
    rows += [(patched(1 + 4, 16187462), n, 600_000), (patched(1 + 4, 0x7fffffff), n, 600_000), (patched(1 + 8 + 4, n + 29), n, 600_000),
             (patched(1 + 4, n), n, 600_000), (patched(1 + 4, 16187462)[:184], 184, 600_000), (bytes([8]) + good[1:6], 6, 600_000)]
    rows += [(bytes([0]) + good[1:], n, 600_000), (bytes([9]) + good[1:] + bytes(100), n + 100, 600_000), (b"", 0, 10), (b"\x01", 1, 0), (b"\x01abc", 4, 10)]
    rows += [(patched(1, -1), n, 600_000), (patched(1 + 4, -1), n, 600_000), (patched(1 + 8, -5), n, 600_000), (patched(1 + 8 + 4, -(1 << 31)), n, 600_000)]
    rows += [(good, TABLE(2) - 1, 600_000), (good, TABLE(2), 600_000), (good, TABLE(2) + 100, 600_000), (good, TABLE(2) + 219, 600_000)]   # the table cut one byte short; sub-blocks cut
    eight = M.frame_parallel(1 << 20, [1000] * 8, [10 * b + 1 for b in range(7)] + [1000])
    rows += [(eight, len(eight), 8000), (eight, len(eight), 7999), (eight, len(eight) - 1, 8000), (eight, TABLE(8) - 1, 8000)]
    return rows


def test_table_parser_gives_the_decoders_bounds_and_codes(probe):
    rows = table_cases()
    got = probe([f"T {in_size} {max_out} {hx(data)}" for data, in_size, max_out in rows])
    verdicts = []
    for (data, in_size, max_out), g in zip(rows, got):
        nb, subs, rc = M.subtable_parse(data, in_size, max_out)
        assert (g["nb"], g["subs"], g["result"]) == (nb, subs, rc), (data[:20], in_size, max_out)
        verdicts.append(rc)
    assert verdicts[:4] == [0, M.DATA_CORRUPT, M.DATA_CORRUPT, 0] and set(verdicts[4:10]) == {M.DATA_CORRUPT}
    assert got[0]["subs"] == [[100, 300_000, 17, 0], [120, 300_000, 117, 300_000]]
    assert [g["nb"] for g in got[10:15]] == [M.DATA_CORRUPT, M.DATA_CORRUPT, M.DATA_CORRUPT, 1, 1]
    assert verdicts[15:19] == [M.DATA_CORRUPT] * 4 and verdicts[19:23] == [M.DATA_CORRUPT, M.DATA_CORRUPT, M.DATA_CORRUPT, M.DATA_CORRUPT]
    assert verdicts[23:] == [0, M.DATA_CORRUPT, M.DATA_CORRUPT, M.DATA_CORRUPT] and len(got[23]["subs"]) == 8
    # the library's decoder behind a sealed block says the same to every table the parser refuses (the sub-blocks here are no coder's
    # output: a table that passes ends in the sub-block decoders, which is not this test's subject)
    mode = M.mode_pack(1, 1, 0, 0)
    for (data, in_size, max_out), rc in zip(rows, verdicts):
        if rc == M.DATA_CORRUPT and in_size >= 1 and max_out <= 600_000:
            body = data[:in_size] + b"\x00"                                              # no aux indexes
            blk = M.block_header(28 + len(body), max_out, mode, 1, 0, M._adler(body)) + body
            assert api.bsc_block_info(blk)[0] == 0 and api.bsc_decompress(blk) == api.DATA_CORRUPT, (data[:20], in_size, max_out)


# ---- the same under AddressSanitizer + UBSan ----------------------------------------------------------------------------------------------
def test_probe_is_clean_under_sanitizers_on_the_edge_tables(tmp_path):
    """a stand-alone program: nothing is preloaded and nothing is loaded into Python"""
    exe = str(tmp_path / "container_probe_san")
    build_probe(exe, ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    ask = asker(exe)
    rows = framing_edges()
    lines = [frame(cmd, n, size, c if cmd == "Q" else [min(x, s) for x, s in zip(c, size)]) for n, size, c in rows for cmd in "PQV"]
    lines += [f"T {in_size} {max_out} {hx(data)}" for data, in_size, max_out in table_cases()]
    lines += ["S -", "S " + hx(b"abc"), "H 28 0 0 0 1 1", f"C 100 33 5 77 50 3 1 2 3 {hx(bytes(50))}", f"C 54 33 5 77 50 0 {hx(bytes(50))}", "C 1000 33 5 77 -3 0 -",
              "D " + hx(M.block_header(28, 100, 33, 1, 0, 1)), "D " + hx(M.coded_block(1000, bytes(50), 33, 5, [1, 2, 3], 77)), "A 0", "A 2147483647"]
    ask(lines)
