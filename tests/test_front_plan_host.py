"""The arithmetic of the QLFC front end (libbsc_amd/csrc/device/qlfc_front_plan.h — what both forms of qlfc_front.hip are driven by)
judged on the CPU through tools/front_plan_probe.cpp: the cuts from flag words against the reference's split, first-seen order, alphabet
and rank path against a few lines of Python, the plan of a pass against the layout bscgpu_front_batch_host builds, and the table layout
against the values it has always had.  The probe is also built with AddressSanitizer and UBSan and run, as that program, on the same
lines."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

from front_inputs import KI, mixed_batch, runs_block

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NO_RUN = 0xFFFFFFFF
MAX_N = 1 << 20                                                 # BSCGPU_BATCH_MAX_N: a block of a pass lies below it


def _build(tmp_path_factory, name, extra):
    exe = str(tmp_path_factory.mktemp(name) / name)
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", *extra, "-I", os.path.join(ROOT, "libbsc_amd", "csrc", "device"),
                    os.path.join(ROOT, "tools", "front_plan_probe.cpp"), "-o", exe], check=True)
    return exe


def _ask(exe, lines):
    r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    out = [json.loads(l) for l in r.stdout.splitlines()]
    assert len(out) == len(lines)
    return out, r.stderr


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    exe = _build(tmp_path_factory, "front_plan_probe", [])
    return lambda lines: _ask(exe, lines)[0]


# ---- inputs and the lines they become ----------------------------------------------------------------------------------------------
def _flag_words(a):
    """bit q = (a[1 + 32 q] != a[32 q]), 64 to a word: what qf_split_flags_kernel writes -> list of ints"""
    f = a[1::32] != a[0:a.size - 1:32][:a[1::32].size]
    pad = np.zeros((-f.size) % 64, bool)
    bits = np.concatenate([f, pad]).reshape(-1, 64)
    return [int(x) for x in (bits.astype(np.uint64) << np.arange(64, dtype=np.uint64)).sum(axis=1, dtype=np.uint64)]


def _hex(words):
    return " ".join([str(len(words))] + ["%x" % w for w in words])


def _cut_inputs():
    """(name, bytes): every n with a random 2-symbol text, with the noisy stretch and with few sampled changes"""
    rng = np.random.default_rng(20261021)
    out = []
    for n in (2, 33, 4097, 262144, 262145, 1048575):
        out.append((f"random2 n={n}", rng.integers(0, 2, n, dtype=np.uint8)))
        a = np.full(n, 7, np.uint8)                             # constant but for one 300-byte noisy stretch: cuts 32 bytes apart
        at = min(n // 3, max(n - 300, 0))
        a[at:at + 300] = rng.integers(0, 256, a[at:at + 300].size, dtype=np.uint8)
        out.append((f"noisy n={n}", a))
        b = np.full(n, 1, np.uint8)                             # two sampled changes (positions 33 and 97): at most nblocks for every nblocks
        b[33:] = 2
        b[97:] = 3
        out.append((f"few n={n}", b))
    return out


def _orc_split(a, nb):
    from oracle.refbind import Oracle
    L = Oracle().L
    st, sz = (C.c_int * 8)(), (C.c_int * 8)()
    L.orc_split_blocks.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    L.orc_split_blocks.restype = None
    L.orc_split_blocks(a.ctypes.data, a.size, nb, st, sz)
    return list(st[:nb]), list(sz[:nb])


def _cut_lines():
    return [(name, a, nb, f"cuts {a.size} {nb} {_hex(_flag_words(a))}") for name, a in _cut_inputs() for nb in (2, 4, 8)]


K_CASES = (1, 2, 32, 33, 64, 65, 256)


def _row_cases():
    """per K: rows (dicts symbol -> first run) of a block of three sub-blocks whose union alphabet has K symbols"""
    rng = np.random.default_rng(5)
    cases = []
    for K in K_CASES:
        alpha = [int(x) for x in rng.permutation(256)[:K]]
        rows = []
        for r in range(3):
            syms = alpha if r == 0 else [s for s in alpha if rng.random() < 0.5]
            firsts = rng.permutation(100000)[:len(syms)] + 100000 * r
            rows.append({s: int(f) for s, f in zip(syms, firsts)})
        rows.append({})                                         # an empty row changes nothing
        cases.append((K, rows))
    return cases


def _row_line(rows):
    parts = ["rows", str(len(rows))]
    for row in rows:
        parts.append(str(len(row)))
        for s, f in row.items():
            parts += [str(s), str(f)]
    return " ".join(parts)


def _pass_cases():
    rng = np.random.default_rng(77)
    edge = [0, 0, 5000, 0, 0, 300 * KI, 0, 70, 0, 0]            # empty blocks first, last and adjacent
    return [("mixed_batch", mixed_batch(0)),
            ("4096 one-byte blocks", [np.full(1, b & 255, np.uint8) for b in range(4096)]),
            ("empty blocks", [runs_block(rng, n, 9) for n in edge]),
            ("one block of 1 MiB - 1", [runs_block(rng, MAX_N - 1, 33)])]


def _pass_line(blocks, limit=MAX_N, cap=1 << 40):
    words = []
    for a in blocks:
        if a.size >= 256 * KI:                                  # two sub-blocks: the block is sampled, its words follow the ones before
            words += _flag_words(a)
    return f"pass {len(blocks)} {limit} {cap} {' '.join(str(a.size) for a in blocks)} {_hex(words)}"


LAYOUT_MAX_N = (1, 1 << 20, 64 << 20, 1 << 30)
# what the parent's qlfc_front.hip computed (FT_* in u32 words; front_scratch_bytes is the first-run table's 8 MiB up to max_n = 2 GiB)
LAYOUT_WANT = dict(FT_OFF=0, FT_RUN=16385, FT_FLAG=24578, FT_FIRST=36928, FT_WORDS=2134080, max_blocks=4096, max_sub=8192)
SCRATCH_WANT = {1: 8425476, 1 << 20: 8425476, 64 << 20: 8425476, 1 << 30: 8425476}


def _all_lines():
    return ([l for _, _, _, l in _cut_lines()] + [_row_line(rows) for _, rows in _row_cases()] + [_pass_line(b) for _, b in _pass_cases()]
            + [f"layout {n}" for n in LAYOUT_MAX_N])


# ---- cuts --------------------------------------------------------------------------------------------------------------------------
def test_cuts_match_reference_split(probe):
    cases = _cut_lines()
    got = probe([l for _, _, _, l in cases])
    adaptive = equal = close = 0
    for (name, a, nb, _), g in zip(cases, got):
        n = a.size
        assert g["samples"] == (0 if n < 2 else (n - 1 + 31) // 32) and g["words"] == (g["samples"] + 63) // 64, name
        st, sz = _orc_split(a, nb)
        assert (g["start"], g["size"]) == (st, sz), f"{name} nblocks={nb}"
        sampled = int(np.count_nonzero(a[1::32] != a[0:n - 1:32][:a[1::32].size]))
        adaptive += sampled > nb
        equal += sampled <= nb
        close += sampled > nb and min(sz[:-1]) == 32
    assert adaptive and equal and close, "both branches of the split, and cuts 32 bytes apart, must occur"


# ---- first seen, alphabet, rank path -----------------------------------------------------------------------------------------------
def test_rows_alphabet_and_rank_path(probe):
    cases = _row_cases()
    got = probe([_row_line(rows) for _, rows in cases])
    for (K, rows), g in zip(cases, got):
        for row, gr in zip(rows, g["rows"]):
            assert gr["first_seen"] == sorted(row, key=row.get), f"K={K}"
            assert gr["first"] == (min(row.values()) if row else NO_RUN), f"K={K}"
        present = sorted(set().union(*rows))
        assert g["K"] == K == len(present)
        assert g["lut"] == [min(present.index(c), 255) if c in present else 0 for c in range(256)], f"K={K}"
        assert g["path"] == (0 if K <= 32 else 1 if K <= 64 else 2), f"K={K}"


# ---- the plan of a pass ------------------------------------------------------------------------------------------------------------
def test_pass_plan_matches_host_layout(probe):
    from libbsc_amd.gpu import front_batch_host
    cases = _pass_cases()
    got = probe([_pass_line(b) for _, b in cases])
    for (name, blocks), g in zip(cases, got):
        sizes = [b.size for b in blocks]
        want = front_batch_host(np.concatenate(blocks), sizes)
        big = [b for b in blocks if b.size >= 256 * KI]
        assert g["total"] == sum(sizes) and g["sampled"] == len(big), name
        assert g["nwords"] == sum(((b.size - 1 + 31) // 32 + 63) // 64 for b in big), name
        assert g["maxq"] == max([(b.size - 1 + 31) // 32 for b in big], default=0), name
        offs = np.concatenate([[0], np.cumsum(sizes)])
        tab, w0 = [], 0
        for i, b in enumerate(blocks):
            if b.size >= 256 * KI:
                tab += [int(offs[i]), b.size, w0]
                w0 += ((b.size - 1 + 31) // 32 + 63) // 64
        assert g["flag_tab"] == tab, name
        nsub = g["nsub"]
        assert nsub == want.nsub and g["table_words"] == 2 * nsub + 1, name
        assert g["blk_sub"] == list(want.blk_sub) and g["sub_start"] == list(want.sub_start) and g["sub_size"] == list(want.sub_size), name
        sub_off = g["sub_off"]
        assert all(x < y for x, y in zip(sub_off, sub_off[1:])) and sub_off[nsub] == sum(sizes), name
        blk_of = np.searchsorted(np.asarray(want.blk_sub), np.arange(nsub), side="right") - 1
        assert g["sub_base"] == [int(offs[b]) for b in blk_of], name
        assert sub_off[:nsub] == [base + st for base, st in zip(g["sub_base"], g["sub_start"])], name


def test_pass_arguments(probe):
    got = probe(["pass -1 1048576 100 0", "pass 4097 1048576 100000 " + "1 " * 4097 + "0", "pass 2 1048576 100 50 1048576 0",
                 "pass 2 1048576 100 60 -1 0", "pass 2 1048576 100 60 41 0", "pass 2 1048576 100 60 40 0", "pass 0 1048576 100 0"])
    assert [g["total"] for g in got] == [-1, -1, -1, -1, -1, 100, 0]
    assert got[5]["nsub"] == 2 and got[6]["nsub"] == 0 and got[6]["sub_off"] == [0]


# ---- the table layout --------------------------------------------------------------------------------------------------------------
def test_layout_is_the_parents(probe):
    got = probe([f"layout {n}" for n in LAYOUT_MAX_N])
    for n, g in zip(LAYOUT_MAX_N, got):
        scratch = g.pop("scratch")
        assert g == LAYOUT_WANT and scratch == SCRATCH_WANT[n], f"max_n={n}"
        # both tenants fit: the flag words of a pass (n_b / 256 bytes rounded up to a word per block) and the first-run rows with sub_run
        assert scratch >= n // 256 + 8 * g["max_blocks"] and scratch >= g["max_sub"] * 1024 + 4 * (g["max_sub"] + 1)


# ---- sanitizers --------------------------------------------------------------------------------------------------------------------
def test_probe_under_sanitizers(tmp_path_factory, probe):
    """the same lines through the probe built with AddressSanitizer and UBSan, as a stand-alone program: same answers, no report"""
    exe = _build(tmp_path_factory, "front_plan_probe_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    lines = _all_lines()
    got, err = _ask(exe, lines)
    assert "runtime error" not in err and "AddressSanitizer" not in err, err[-2000:]
    assert got == probe(lines)
