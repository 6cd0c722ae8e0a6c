"""The pass plan of the BWT's first sort with the leftover digit folded into key packing (bwt.hip: bwt_first_sort) — a Python twin of
the plan, checked for what it covers, where it applies, and that it sorts as the plan it replaces."""
import numpy as np
import pytest

from pipeline_model import key_geometry


def fold_plan(K, n=1 << 20, batch_count=0):
    """-> (fold, passes): fold = (shift, bits) of the digit key packing sorts on, or None; passes = the (shift, bits) digit passes of the
    sort behind it.  r = (cb w) mod 8 bits are folded when the block is single, 1 <= r <= 4 and r <= cb (the digit then lies inside the
    key's last character); the passes are then whole bytes from low_shift + r.  Otherwise the plan key_geometry describes."""
    g = key_geometry(K, n, batch_count)
    bits = g["cb"] * g["w"]
    r = bits % 8
    if batch_count == 0 and 1 <= r <= 4 and r <= g["cb"]:
        return (g["low_shift"], r), [(g["low_shift"] + r + 8 * p, 8) for p in range((bits - r) // 8)]
    return None, list(g["passes"])


def lsd_sort(keys, digits):
    """stable LSD sort of the keys' indexes over the (shift, bits) digits, lowest first"""
    order = np.arange(keys.size)
    for shift, bits in digits:
        d = (keys[order] >> np.uint64(shift)) & np.uint64((1 << bits) - 1)
        order = order[np.argsort(d, kind="stable")]
    return order


@pytest.mark.parametrize("batch_count", [0, 1, 100])
def test_every_key_bit_is_sorted_on_exactly_once(batch_count):
    for K in range(2, 257):
        g = key_geometry(K, 1 << 20, batch_count)
        fold, passes = fold_plan(K, 1 << 20, batch_count)
        digits = ([fold] if fold else []) + passes
        covered = [b for s, w in digits for b in range(s, s + w)]
        assert covered == list(range(g["low_shift"], 64)), (K, batch_count, digits)       # in order, no bit twice, none left out
        assert all(1 <= w <= 8 for _, w in digits) and len(passes) <= 8
        if fold:
            assert all(w == 8 and s % 8 == 0 for s, w in passes), (K, passes)           # what is left is byte aligned
            assert len(passes) == len(g["passes"]) - 1                                  # one pass fewer than the plan it replaces
            assert fold[0] + fold[1] <= g["low_shift"] + g["cb"]                        # the folded digit lies inside the last character


def test_the_route_applies_exactly_at_five_and_six_bit_characters():
    for K in range(2, 257):
        cb = key_geometry(K, 1 << 20)["cb"]
        fold, passes = fold_plan(K)
        assert (fold is not None) == (cb in (5, 6)), (K, cb)
        if fold:
            assert fold == (4, 4) and passes == [(8 * p, 8) for p in range(1, 8)], (K, fold, passes)
        assert fold_plan(K, 1 << 20, batch_count=3)[0] is None                           # never a batched pass


@pytest.mark.parametrize("K", [17, 32, 33, 64])
def test_the_folded_plan_sorts_as_the_plan_it_replaces(K):
    g = key_geometry(K, 1 << 20)
    rng = np.random.default_rng(K)
    n = 20_000
    # keys as packing forms them: w characters of cb bits, the bits below low_shift zero; few distinct values per digit so that ties —
    # where stability decides — are everywhere
    keys = np.zeros(n, np.uint64)
    for t in range(g["w"]):
        keys |= rng.integers(0, min(K, 3 + t), n).astype(np.uint64) << np.uint64(64 - g["cb"] * (t + 1))
    fold, passes = fold_plan(K)
    assert fold is not None
    got = lsd_sort(keys, [fold] + passes)
    want = lsd_sort(keys, g["passes"])
    assert np.array_equal(got, want)
    assert np.array_equal(got, np.argsort(keys, kind="stable"))
