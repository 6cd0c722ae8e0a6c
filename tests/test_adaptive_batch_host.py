"""The adaptive coder's model (-e2) of a pass on the CPU (no GPU): the stand-in bscgpu_adaptive_pstream_host — the host model's walk with
the mixer step that the device shares (devcoder_model.h) — against the host coder and the compiled reference: every block of every
pass coded from the stand-in's streams (bscgpu_front_batch_code_ps: an -e2 stream is a static-form body) equals bscgpu_front_batch_code
with coder 2 and the reference's bsc_coder_compress byte for byte; a sub-block's stream through the range coder stage behind coder 1's
prefix equals its coded bytes; the mixer ids equal a numpy restatement of the instance table; and the decisions are the static coder's.

The mixer's arithmetic wraps on some inputs (the reference's int overflow); host and device share one unsigned text of it, and no
small input is known to reach the wrap: nothing here claims to."""
import ctypes as C

import numpy as np
import pytest

import adaptive_batch_inputs as ab
import model_batch_inputs as mb
import rc_inputs as ri
from libbsc_amd import gpu

NAMES = list(ab.PASSES)


@pytest.mark.parametrize("name", NAMES)
def test_blocks_code_from_the_stand_ins_streams(name, ref):
    blocks, fb, ps, poff, _ = ab.reference(name)
    assert ps.size == int(poff[-1])
    coded = 0
    for b, a in enumerate(blocks):
        got = gpu.front_batch_code_ps(fb, b, ps, poff, 3)
        if a.size == 0:
            assert got == -1
            continue
        assert got == fb.code(b, 2, 3), f"{name}: block {b} (n={a.size}) differs from front_batch_code with coder 2"
        assert got == ref.coder_compress(a, 2, 3), f"{name}: block {b} (n={a.size}) differs from the reference"
        coded += 1
    assert coded == sum(1 for a in blocks if a.size), "no block is left out"


def test_serial_framing_too(ref):
    blocks, fb, ps, poff, _ = ab.reference("mixed")
    for b, a in enumerate(blocks):
        if a.size:
            got = gpu.front_batch_code_ps(fb, b, ps, poff, 1)
            assert got == fb.code(b, 2, 1) and got == ref.coder_compress(a, 2, 1), f"block {b} (n={a.size})"


@pytest.mark.parametrize("name", NAMES)
def test_a_sub_block_stream_is_a_static_body_behind_coder_1s_prefix(name, ref):
    """header word, alphabet and stop rule are the static coder's: rc_prefix(..., 1), which keeps refusing coder 2"""
    blocks, fb, ps, poff, _ = ab.reference(name)
    s = max(range(fb.nsub), key=lambda q: int(poff[q + 1]) - int(poff[q]))          # the sub-block with the most decisions
    sub = mb.sub_bytes(fb, blocks, s)
    want = ref.qlfc_encode_block(sub, 2)
    pre = gpu.rc_prefix(fb.first_seen(s), sub.size, 1)
    cnt = int(poff[s + 1]) - int(poff[s])
    res, out = gpu.rc_encode_host(ri.STATIC16, ps, pre, [(int(poff[s]), cnt, 0, len(pre), 0, sub.size)])
    got = res[0] if res[0] < 0 else out[:res[0]].tobytes()
    assert got == want, f"{name}: sub-block {s} (n={sub.size})"


@pytest.mark.parametrize("name", ["hist_above_clamp", "escape", "tiny_alphabets"])
def test_mixer_ids_equal_the_table(name):
    _, fb, _, poff, dbg = ab.reference(name)
    for s in range(fb.nsub):
        want = ab.mixer_ids(fb, s)
        got = dbg[3, int(poff[s]):int(poff[s + 1])]
        assert got.size == want.size, f"{name}: sub-block {s}: {got.size} decisions, the table's walk {want.size}"
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, f"{name}: sub-block {s}: {bad.size} mixer ids differ, first at {int(bad[0])}: {int(got[bad[0]])} != {int(want[bad[0]])}"
    assert int(dbg[3].max()) < ab.NUM_MIX


def test_the_inputs_reach_what_they_are_built_for():
    _, fb, _, poff, dbg = ab.reference("hist_above_clamp")
    rows = ab.run_exp_rows(dbg[3])
    assert rows.max() > 7, f"run_exp rows {rows.tolist()}: run_hist must settle above the static model's clamp"
    s0 = int(fb.blk_sub[1])                                                           # the twin with runs of 2^7 bytes stays at the clamp
    assert ab.run_exp_rows(dbg[3, int(poff[s0]):]).max() <= 7
    _, fb, _, poff, dbg = ab.reference("escape")
    ids = dbg[3]
    esc = (ids >= ab.MIX_RP) & (ids < ab.MIX_NF)
    assert esc[:int(poff[int(fb.blk_sub[1])])].mean() > 0.3, "the noise block codes its ranks through rank_esc"
    second = esc[int(poff[int(fb.blk_sub[1])]):]
    flips = np.count_nonzero(np.diff(second.astype(np.int8)) != 0)
    assert second.any() and not second.all() and flips >= 2, "text - noise - text crosses avg_rank 32 both ways"
    _, fb, _, _, dbg = ab.reference("tiny_alphabets")
    assert sorted(set(int(n) for n in fb.nsym)) == [1, 2, 3, 5]


@pytest.mark.parametrize("name", NAMES)
def test_decisions_are_the_static_coders(name):
    """same decisions, different probabilities: per sub-block the coded bits and the run-start marks of the static stand-in"""
    _, fb, ps, poff, _ = ab.reference(name)
    sps, spoff = mb.host_streams(fb)
    assert np.array_equal(poff, spoff)
    assert np.array_equal(ps & (ab.PS_BIT | ab.PS_RUN), sps & (ab.PS_BIT | ab.PS_RUN))
    if ps.size > 10000:
        assert (ps != sps).mean() > 0.5, "the probabilities are the mixer's, not the static blend"
    assert not (ps & 0xc000).any() and (ps & 0xfff).min() >= 1


def test_bad_arguments_and_counting():
    from libbsc_amd import _native as N
    _, fb, ps, poff, dbg = ab.reference("tiny_alphabets")
    L = N.lib()
    e = np.zeros(16, np.uint16)
    assert L.bscgpu_adaptive_pstream_host(None, 0, N.np_ptr(e), 16, None) == -1
    assert L.bscgpu_adaptive_pstream_host(C.byref(fb.lay), fb.nsub, N.np_ptr(e), 16, None) == -1
    assert L.bscgpu_adaptive_pstream_host(C.byref(fb.lay), -1, N.np_ptr(e), 16, None) == -1
    assert L.bscgpu_adaptive_pstream_host(C.byref(fb.lay), 0, None, 4, None) == -1
    s = fb.nsub - 1
    n = int(L.bscgpu_adaptive_pstream_host(C.byref(fb.lay), s, None, 0, None))       # counting only
    assert n == int(poff[s + 1]) - int(poff[s]) and n > 16
    e[:] = 0xffff
    planes = np.full((4, 8), 0xffff, np.uint16)
    assert int(L.bscgpu_adaptive_pstream_host(C.byref(fb.lay), s, N.np_ptr(e), 8, N.np_ptr(planes))) == n      # counted, not written, past cap
    assert np.array_equal(e[:8], ps[int(poff[s]):int(poff[s]) + 8]) and (e[8:] == 0xffff).all()
    assert np.array_equal(planes, dbg[:, int(poff[s]):int(poff[s]) + 8])


@pytest.mark.parametrize("name", NAMES)
def test_gpu_inputs_fit_the_device_models_capacity(name):
    """the passes the GPU tests expect the device to keep: within the runs and decisions the context's arena holds, and no chain near
    the step cap's default (1 << 18)"""
    _, fb, _, poff, dbg = ab.reference(name)
    cap = ab.CAPACITY[name]
    assert fb.m <= cap // 4 and int(poff[-1]) <= cap
    sub = np.repeat(np.arange(fb.nsub, dtype=np.int64), np.diff(poff.astype(np.int64)))
    longest = int(np.unique(sub << 11 | dbg[3].astype(np.int64), return_counts=True)[1].max())
    print(f"{name}: {fb.m} runs, {int(poff[-1])} decisions, longest mixer chain {longest}")
    assert 64 < longest < 1 << 18
