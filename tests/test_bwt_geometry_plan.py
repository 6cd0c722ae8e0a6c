"""What the BWT key-geometry sweep covers (no GPU): pipeline_model.key_geometry restates how bwt_key_plan (libbsc_amd/csrc/device/bwt_plan.h;
test_bwt_plan_host.py compares the two field by field) lays out the first sort's keys from the alphabet size, the block length and the block count of a batched pass; the case list of bwt_geometry_cases.py must reach every
layout the rules can produce — character widths, key lengths, digit passes, the text rounds' key lengths, values with and without the
predecessor's code, every width of the block field — with the alphabet each case is meant to have."""
import numpy as np

import bwt_geometry_cases as gc
from pipeline_model import key_geometry


def test_key_geometry_follows_the_rules():
    g = key_geometry(28, 64 << 20)                       # the bench text: 28 symbols
    assert (g["cb"], g["w"], g["low_shift"], g["ta"], g["pred_shift"], g["batch_bb"]) == (5, 12, 4, 12, 26, 0)
    assert g["passes"] == [(4, 8), (12, 8), (20, 8), (28, 8), (36, 8), (44, 8), (52, 8), (60, 4)]
    # cb = max(4, ceil(log2 K)), w = 64 / cb, ta in {15, 12, 10, 8, 7}
    assert [key_geometry(K, 1000)["cb"] for K in (1, 2, 16, 17, 32, 33, 64, 65, 128, 129, 256)] == [4, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8]
    assert [(key_geometry(K, 1000)["w"], key_geometry(K, 1000)["ta"]) for K in (16, 32, 64, 128, 256)] == [(16, 15), (12, 12), (10, 10), (9, 8), (8, 7)]
    # a batch codes K + 1 values and keeps the block field on top
    assert [key_geometry(K, 1000, 100)["cb"] for K in (15, 16, 31, 32, 63, 64, 127, 128, 255, 256)] == [4, 5, 5, 6, 6, 7, 7, 8, 8, 9]
    g = key_geometry(256, 1000, 4096)
    assert (g["cb"], g["batch_bb"], g["w"], g["low_shift"], g["pred_shift"]) == (9, 12, 5, 7, 0)
    assert key_geometry(15, 1000, 1)["w"] == 16 and key_geometry(15, 1000, 2)["w"] == 15
    # the values carry the predecessor's code while idx_bits + cb <= 32
    assert key_geometry(256, 1 << 24)["pred_shift"] == 24 and key_geometry(256, (1 << 24) + 1)["pred_shift"] == 0
    assert key_geometry(16, 1 << 28)["pred_shift"] == 28 and key_geometry(16, (1 << 28) + 1)["pred_shift"] == 0
    for K in range(1, 257):
        for cnt in (0, 1, 2, 5, 100, 4096):
            g = key_geometry(K, 5000, cnt)
            assert g["low_shift"] >= 0 and g["cb"] * g["w"] + g["batch_bb"] + g["low_shift"] == 64 and 2 <= g["ta"] <= 16
            assert sum(b for _, b in g["passes"]) == 64 - g["low_shift"] and all(1 <= b <= 8 for _, b in g["passes"])


def _single_geo():
    return [(K, n, key_geometry(K, n)) for K, n in gc.SINGLE_CASES]


def _batch_geo():
    return [(K, sizes, key_geometry(K, sum(sizes), len(sizes))) for K, sizes in gc.BATCH_CASES]


def test_every_character_width_single_and_batched():
    assert {g["cb"] for _, _, g in _single_geo()} == {4, 5, 6, 7, 8}
    assert {g["cb"] for _, _, g in _batch_geo()} == {4, 5, 6, 7, 8, 9}
    assert {g["ta"] for _, _, g in _single_geo()} == {15, 12, 10, 8, 7}            # bwt_text_window loads its fifth word only for a > 12
    assert {len(g["passes"]) for _, _, g in _single_geo()} == {8}
    assert len({(g["low_shift"], tuple(g["passes"])) for _, _, g in _batch_geo()}) >= 8


def test_both_sides_of_every_power_of_two():
    ks = {K for K, _ in gc.SINGLE_CASES}
    for p in (16, 32, 64, 128):
        assert {p, p + 1} <= ks and key_geometry(p, 3001)["cb"] + 1 == key_geometry(p + 1, 3001)["cb"]
    assert 256 in ks
    kb = {K for K, _ in gc.BATCH_CASES}
    for p in (16, 32, 64, 128, 256):                     # the batch's K + 1 rule: the width changes between K = p - 1 and p
        assert {p - 1, p} <= kb and key_geometry(p - 1, 3001, 100)["cb"] + 1 == key_geometry(p, 3001, 100)["cb"]


def test_block_field_widths():
    assert {0, 1, 2, 6, 7, 12} <= {g["batch_bb"] for _, _, g in _batch_geo()}


def test_block_lengths_around_the_key_length():
    # single blocks: n can only come down to w where the alphabet fits into w characters, i.e. cb = 4
    n4 = {n for K, n, g in _single_geo() if g["cb"] == 4}
    assert {15, 16, 17} <= n4
    for cb in (4, 5, 6, 7, 8):
        ns = sorted(n for K, n, g in _single_geo() if g["cb"] == cb)
        assert any(2000 <= n <= 9000 for n in ns) and any(90_000 <= n <= 110_000 for n in ns), cb
    # batches: blocks of w - 1, w, w + 1 characters beside larger ones at every width
    for cb in (4, 5, 6, 7, 8, 9):
        ok = False
        for K, sizes, g in _batch_geo():
            if g["cb"] == cb and {g["w"] - 1, g["w"], g["w"] + 1} <= set(sizes) and any(2000 <= n <= 9000 for n in sizes) and any(90_000 <= n <= 110_000 for n in sizes):
                ok = True
        assert ok, cb


def test_single_read_passes_and_the_predecessor_boundary():
    for cb in (4, 5, 6, 7, 8):
        assert any(g["cb"] == cb and n > gc.OS_MIN_RECORDS for K, n, g in _single_geo()), cb
    for cb in (4, 5, 6, 7, 8, 9):
        assert any(g["cb"] == cb and sum(sizes) > gc.OS_MIN_RECORDS for K, sizes, g in _batch_geo()), cb
    p = {n: g["pred_shift"] for K, n, g in _single_geo() if g["cb"] == 8}
    assert p[1 << 24] == 24 and p[(1 << 24) + 1] == 0
    assert all(g["pred_shift"] == 0 for _, _, g in _batch_geo())


def test_batches_are_one_pass_of_small_blocks():
    from libbsc_amd.gpu import batch_plan
    for K, sizes in gc.BATCH_CASES:
        assert max(sizes) < gc.BATCH_MAX_N and len(sizes) <= 4096
        npass, plan = batch_plan(sizes, 1, (16 << 20) + 4096)
        assert npass == 1 and plan == [0] * len(sizes), (K, len(sizes))


def test_texts_have_the_alphabet_of_their_case():
    """the geometry is derived from the text's own byte histogram: a case only covers its layout if every symbol occurs"""
    for K, n in gc.SINGLE_CASES:
        if n > 200_000:
            continue                                     # (the large ones are checked where they run: test_gpu_bwt_geometry.py)
        T = gc.single_text(K, n)
        a = np.unique(T)
        assert T.size == n and a.size == K and (K < 2 or (a[0] == 0 and a[-1] == 255)), (K, n)
    for K, sizes in gc.BATCH_CASES:
        if sum(sizes) > 1_500_000:
            continue
        Ts = gc.batch_texts(K, sizes)
        assert [t.size for t in Ts] == sizes
        assert np.unique(np.concatenate(Ts)).size == K, (K, len(sizes))
    T = gc.single_text(16, 100_003)
    assert np.array_equal(T, gc.single_text(16, 100_003))
    # not noise: the first sort leaves work for the rounds (many suffixes share their first w characters)
    g = key_geometry(16, T.size)
    lut = np.zeros(256, np.uint64); lut[gc.alphabet(16)] = np.arange(16, dtype=np.uint64)
    c = np.concatenate([lut[T], np.zeros(g["w"], np.uint64)])
    key = np.zeros(T.size, np.uint64)
    for b in range(g["w"]):
        key = (key << np.uint64(g["cb"])) | c[b:b + T.size]
    _, cnt = np.unique(key, return_counts=True)
    assert cnt[cnt > 1].sum() > T.size // 20


def test_log_texts_leave_long_groups_for_the_first_round():
    """the debug-log check's inputs, by the first sort's own arithmetic: the `split` text leaves exactly one group of more than 1024 records
    holding at most an eighth of the unsorted suffixes (the split is taken), the `doubling` text dozens (handed over)"""
    for cb, K in gc.LOG_CASES.items():
        g = key_geometry(K, gc.LOG_N)
        assert g["cb"] == cb
        lut = np.zeros(256, np.uint64); lut[gc.alphabet(K)] = np.arange(K, dtype=np.uint64)
        for kind, T in zip(("split", "doubling"), gc.log_texts(K)):
            assert np.unique(T).size == K
            c = np.concatenate([lut[T], np.zeros(g["w"], np.uint64)])
            key = np.zeros(T.size, np.uint64)
            for b in range(g["w"]):
                key = (key << np.uint64(cb)) | c[b:b + T.size]
            _, cnt = np.unique(key, return_counts=True)
            U, n_long, n_long_rec = int(cnt[cnt > 1].sum()), int((cnt > 1024).sum()), int(cnt[cnt > 1024].sum())
            if kind == "split":
                assert n_long == 1 and n_long_rec <= U // 8, (cb, U, n_long, n_long_rec)
            else:
                assert n_long >= 4 * g["w"], (cb, n_long)
