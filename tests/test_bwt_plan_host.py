"""The BWT driver's plan (libbsc_amd/csrc/device/bwt_plan.h — what bwt.hip launches by) judged on the CPU through
tools/bwt_plan_probe.cpp: the key plan against pipeline_model.key_geometry over every alphabet size, lengths on both sides of every
rule's edge and every width of a batch's block field; the round decision and the "pays" rule against a hand-written table of their
edges."""
import json
import os
import subprocess

import pytest

from pipeline_model import key_geometry

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NS = [1, 2, 15, 16, 17, 1000, 1 << 24, (1 << 24) + 1, 1 << 26, 1 << 28, (1 << 28) + 1, (1 << 31) - 2]
COUNTS = [0, 1, 2, 5, 100, 4096]
LG_MAX = 4096


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("bwt_plan_probe") / "bwt_plan_probe")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "libbsc_amd", "csrc", "device"),
                    os.path.join(ROOT, "tools", "bwt_plan_probe.cpp"), "-o", exe], check=True)

    def ask(lines):
        r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True)
        out = [json.loads(l) for l in r.stdout.splitlines()]
        assert len(out) == len(lines)
        return out
    return ask


def test_key_plan_equals_the_model(probe):
    cases = [(K, n, cnt, sr) for K in range(1, 257) for n in NS for cnt in COUNTS for sr in (0, 1)]
    got = probe([f"key {K} {n} {cnt} 0 {sr}" for K, n, cnt, sr in cases])
    folds = 0
    for (K, n, cnt, sr), p in zip(cases, got):
        g = key_geometry(K, n, cnt)
        for f in ("cb", "w", "low_shift", "ta", "pred_shift", "batch_bb"):
            assert p[f] == g[f], (K, n, cnt, sr, f, p, g)
        cb, w = g["cb"], g["w"]
        r = (cb * w) & 7
        npf = (cb * w - r) // 8
        fold = bool(sr) and cnt == 0 and 1 <= r <= 4 and r <= cb and n >= w        # the condition bwt_first_sort folds under
        assert (p["fold_r"], p["fold_np"], p["fold"]) == (r, npf, fold), (K, n, cnt, sr, p)
        want = [(g["low_shift"] + r + 8 * q, 8) for q in range(npf)] if fold else g["passes"]
        assert [tuple(x) for x in p["passes"]] == want, (K, n, cnt, sr, p, g)
        folds += fold
    assert folds > 0 and any(p["pred_shift"] for p in got) and any(p["ta"] != p["w"] for p in got)


def test_key_cap(probe):
    """BSC_BWT_W: at most that many characters per key of a single block, from 2 up; a batch keeps its own"""
    w = [p["w"] for p in probe([f"key 28 1000 0 {m} 0" for m in (0, 1, 2, 11, 12, 13)] + ["key 28 1000 3 5 0"])]
    assert w == [12, 12, 2, 11, 12, 12, key_geometry(28, 1000, 3)["w"]]


def _round(isa_valid, U, n_long, n_long_rec, n_mid=0, n_mid_rec=0, hybrid=1, pct=100):
    return f"round {int(isa_valid)} {U} {n_long} {n_long_rec} {n_mid} {n_mid_rec} {hybrid} {pct} {LG_MAX}"


ROUND_TABLE = [
    # rounds on text keys (no ISA yet): a long group or none
    (_round(False, 50_000, 0, 0), "text"),
    (_round(False, 50_000, 1, 1025), "text_split"),
    # ... the long groups hold an eighth of the records, or one more
    (_round(False, 80_000, 2, 10_000), "text_split"),
    (_round(False, 80_000, 2, 10_001), "hand_over"),
    (_round(False, 80_007, 2, 10_000), "text_split"),
    (_round(False, 80_007, 2, 10_001), "hand_over"),
    # ... as many long groups as the tables hold, or one more
    (_round(False, 8 * 4097 * 1025, LG_MAX, LG_MAX * 1025), "text_split"),
    (_round(False, 8 * 4097 * 1025, LG_MAX + 1, (LG_MAX + 1) * 1025), "hand_over"),
    # doubling rounds: the same counts with ISA built
    (_round(True, 50_000, 0, 0), "segsort"),
    (_round(True, 50_000, 0, 0, 3, 900), "segsort"),
    (_round(True, 50_000, 1, 1025, 1, 1025), "hybrid"),
    (_round(True, 50_000, 1, 1025, 0, 0), "radix"),
    # ... n_mid_rec * 100 against U * pct, at equality and one above
    (_round(True, 5_000, 1, 5_000, 1, 5_000), "hybrid"),
    (_round(True, 5_000, 1, 5_000, 1, 5_001), "radix"),
    (_round(True, 10_000, 1, 2_000, 2, 3_000, pct=30), "hybrid"),
    (_round(True, 10_000, 1, 2_000, 2, 3_001, pct=30), "radix"),
    (_round(True, 10_001, 1, 2_000, 2, 3_000, pct=30), "hybrid"),             # 300 000 <= 300 030
    (_round(True, 3_000_000_000, 1, 2_000, 2, 3_000_000_000), "hybrid"),      # (64-bit products)
    # ... hybrid rounds off
    (_round(True, 50_000, 1, 1025, 1, 1025, hybrid=0), "radix"),
    (_round(True, 50_000, 0, 0, 1, 300, hybrid=0), "segsort"),
]

PAYS_TABLE = [
    # U2 < 65536 pays whatever U was; else U2 <= U / 4; never an eighth text round's successor
    ("pays 200000 65535 7", True), ("pays 200000 65536 7", False), ("pays 200000 65535 8", False),
    ("pays 1000000 250000 7", True), ("pays 1000000 250001 7", False), ("pays 1000000 250000 8", False),
    ("pays 1000003 250000 7", True), ("pays 1000003 250001 7", False),
    ("pays 1000000 65535 1", True), ("pays 262144 65536 1", True), ("pays 262143 65536 1", False),
]


def test_round_decision_at_its_edges(probe):
    got = probe([q for q, _ in ROUND_TABLE] + [q for q, _ in PAYS_TABLE])
    for (q, want), g in zip(ROUND_TABLE + PAYS_TABLE, got):
        assert g == want, (q, g, want)
