"""bsc_bwt_decode's host walk against the plain LF oracle (tests/unbwt_inputs.py): on every (L, primary index) pair of the list the
return code AND the text are the oracle's.  A pair is valid iff the rows 0..n form one cycle through the sentinel row; a walk that
meets the sentinel row early must not restart at row 0 and come out "closed" by luck."""
import numpy as np
import pytest

import unbwt_inputs as U
from libbsc_amd import api


def test_oracle_on_known_pairs():
    ab = np.frombuffer(b"abb", np.uint8)
    assert U.lf_verdict(ab, 1) == (-6, None)                          # the smallest pair the old host rule accepted ...
    rc, text = U.parent_host_rule(ab, 1)
    assert rc == 0 and text.tobytes() == b"a\0a"                      # ... as this
    for T in (b"banana", b"abracadabra", b"aaaa", b"ab", b"mississippi"):
        t = np.frombuffer(T, np.uint8)
        L, idx = U.bwt(t)
        rc, text = U.lf_verdict(L, idx)
        assert rc == 0 and text.tobytes() == T
    L, idx = U.bwt(np.frombuffer(b"banana", np.uint8))
    assert (L.tobytes(), idx) == (b"annbaa", 4)                       # rows: "", a, ana, anana, [banana], na, nana
    rng = np.random.default_rng(1)
    T = rng.integers(0, 3, 3000, dtype=np.uint8)                      # prefix doubling against the naive sort
    b = T.tobytes()
    assert np.array_equal(U.suffix_array(T), np.array(sorted(range(T.size), key=lambda i: b[i:])))


def test_the_list_holds_every_class():
    """conditions on the list, by the oracle alone: without them a test over the list could pass on one class only"""
    count, accepted = U.census(U.index_pairs() + U.column_pairs())
    print("index + column pairs:", count, "broken pairs the parent's host rule accepts:", accepted)
    assert count["valid-other"] >= 50
    assert count["broken"] >= 2000
    assert accepted >= 50
    sizes = {p.L.size for p in U.index_pairs()}
    assert sizes == set(U.SIZES)
    assert len(U.column_pairs()) == 300 and all(8 <= p.L.size <= 400 for p in U.column_pairs())
    assert {p.cls for p in U.large_pairs()} >= {"valid", "broken"}


def _check(p, features, aux=()):
    back, rc = api.bsc_bwt_decode(p.L, p.idx, aux, features=features)
    assert rc == p.rc, (p, features, len(aux), rc)
    if rc == 0:
        assert np.array_equal(back, p.text), (p, features, "the text is not the oracle's")
    else:
        assert np.array_equal(back, p.L), (p, features, "a refused block was written")


@pytest.mark.parametrize("features", [1, 3])
def test_host_walk_gives_the_oracles_verdict(features):
    for p in U.small_pairs():
        _check(p, features)


@pytest.mark.parametrize("features", [1, 3])
def test_host_walk_gives_the_oracles_verdict_on_large_blocks(features):
    for p in U.large_pairs():
        _check(p, features)


@pytest.mark.parametrize("features", [1, 3])
def test_chains_from_aux_indexes_follow_the_same_rule(features):
    """the right aux indexes of an undamaged block give the text; a damaged L with its original aux indexes gives -6 or the oracle's
    text (the chains' end rows are checked, so a consistent set of chains IS the single walk), never anything else"""
    for n in (16, 17, 100, 383, 1000):
        T = (np.random.default_rng(n).integers(0, 4, n) + 97).astype(np.uint8)
        L, idx, aux = U.bwt(T, aux=True)
        assert len(aux) == (n - 1) // U.aux_rate(n) >= 1
        back, rc = api.bsc_bwt_decode(L, idx, aux, features=features)
        assert rc == 0 and np.array_equal(back, T), n
    damaged = 0
    for p in U.column_pairs() + U.large_pairs():
        if p.aux is None or not p.aux:
            continue
        back, rc = api.bsc_bwt_decode(p.L, p.idx, p.aux, features=features)
        if p.cls == "valid":
            assert rc == 0 and np.array_equal(back, p.T), p
            continue
        damaged += 1
        assert rc == -6 or (rc == 0 and p.rc == 0 and np.array_equal(back, p.text)), (p, rc)
        if rc == -6:
            assert np.array_equal(back, p.L), (p, "a refused block was written")
    assert damaged >= 250
