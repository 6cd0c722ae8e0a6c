"""The fast coder's model (-e0) of a pass on the CPU (no GPU): the stand-in bscgpu_fast_pstream_host against the chains the device
model runs (tools/devcoder_fast_sim.cpp --trace), its streams through the range coder stage against the reference's coded
sub-blocks, the coding of a block from its sub-blocks' streams (bscgpu_front_batch_code_psf) against bscgpu_front_batch_code and the
compiled reference, and the capacity the GPU tests' passes need."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import fast_batch_inputs as fbi
import model_batch_inputs as mb
import rc_inputs as ri
from libbsc_amd import gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def mixed():
    blocks = mb.mixed_batch(0)
    fb, _ = mb.layout(blocks)
    ps, poff = fbi.host_streams(fb)
    return blocks, fb, ps, poff


@pytest.fixture(scope="module")
def fast_sim(tmp_path_factory):
    """tools/devcoder_fast_sim.cpp, built as tests/test_rc_streams_host.py builds it"""
    exe = str(tmp_path_factory.mktemp("fast_sim") / "fast_sim")
    subprocess.run(["g++", "-O1", "-std=c++17", "-march=x86-64-v3", "-I", os.path.join(ROOT, "libbsc_amd/csrc/host"), "-I", os.path.join(ROOT, "libbsc_amd/csrc/device"),
                    "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tools/devcoder_fast_sim.cpp"), "-o", exe], check=True)
    return exe


def test_stand_in_equals_the_device_chains(mixed, fast_sim, tmp_path):
    blocks, fb, ps, poff = mixed
    assert fb.nsub > len(blocks) - 1
    sides = 0
    for s in range(fb.nsub):
        sub = mb.sub_bytes(fb, blocks, s)
        src, dst = tmp_path / f"in{s}.bin", tmp_path / f"tr{s}.bin"
        sub.tofile(src)
        subprocess.run([fast_sim, "--trace", str(src), str(dst)], check=True)
        want = np.fromfile(dst, np.uint16)
        got = ps[int(poff[s]):int(poff[s + 1])]
        assert got.size == want.size, f"sub-block {s} (n={sub.size}): {got.size} decisions, the chains' walk {want.size}"
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, f"sub-block {s} (n={sub.size}): {bad.size} entries differ, first at {int(bad[0])}: {int(got[bad[0]]):#x} != {int(want[bad[0]]):#x}"
        runs = int(fb.sub_run[s + 1]) - int(fb.sub_run[s])
        assert int(np.count_nonzero(got & fbi.PSF_RUN)) == runs, f"sub-block {s}: one run-start mark per run"
        assert (got & fbi.PSF_SIDE).any() and not (got & fbi.PSF_SIDE).all(), f"sub-block {s}: both precisions occur"
        sides += 1
    assert sides == fb.nsub


def test_stand_in_streams_code_to_the_reference_sub_blocks(mixed, ref):
    blocks, fb, ps, poff = mixed
    coded = 0
    for s in range(fb.nsub):
        sub = mb.sub_bytes(fb, blocks, s)
        want = ref.qlfc_encode_block(sub, 3)
        pre = gpu.rc_prefix(fb.first_seen(s), sub.size, 3)
        cnt = int(poff[s + 1]) - int(poff[s])
        res, out = gpu.rc_encode_host(ri.FAST16, ps, pre, [(int(poff[s]), cnt, 0, len(pre), 0, sub.size)])
        got = res[0] if res[0] < 0 else out[:res[0]].tobytes()
        assert got == want, f"sub-block {s} (n={sub.size})"
        coded += isinstance(want, bytes)
    assert coded >= 20


@pytest.mark.parametrize("features", [1, 3])
def test_code_from_streams_equals_code_from_runs_and_the_reference(mixed, ref, features):
    blocks, fb, ps, poff = mixed
    for b, a in enumerate(blocks):
        if a.size == 0:
            assert gpu.front_batch_code_psf(fb, b, ps, poff, features) == -1
            continue
        got = gpu.front_batch_code_psf(fb, b, ps, poff, features)
        assert got == fb.code(b, 3, features), f"block {b} (n={a.size}) features={features}: differs from front_batch_code"
        assert got == ref.coder_compress(a, 3, features), f"block {b} (n={a.size}) features={features}: differs from the reference"


@pytest.mark.parametrize("features", [1, 3])
def test_code_from_streams_with_a_raw_sub_block(ref, features):
    a = mb.raw_second_sub_block()
    rng = np.random.default_rng(8)
    blocks = [mb.runs_block(rng, 5000, 17), a, rng.integers(0, 256, 5000, dtype=np.uint8)]
    fb, _ = mb.layout(blocks)
    ps, poff = fbi.host_streams(fb)
    for b, x in enumerate(blocks):
        got = gpu.front_batch_code_psf(fb, b, ps, poff, features)
        assert got == fb.code(b, 3, features) and got == ref.coder_compress(x, 3, features), f"block {b}"
    got = gpu.front_batch_code_psf(fb, 1, ps, poff, features)
    size1, res1 = (int(x) for x in np.frombuffer(got[9:17], np.int32))
    assert got[0] == 2 and size1 == res1 and len(got) < a.size, "the second sub-block must be stored raw inside a block that compresses"
    assert gpu.front_batch_code_psf(fb, 2, ps, poff, features) == -3, "the noise block is LIBBSC_NOT_COMPRESSIBLE"


def test_bad_arguments(mixed):
    from libbsc_amd import _native as N
    _, fb, ps, poff = mixed
    L = N.lib()
    out = np.zeros(1 << 21, np.uint8)
    e = np.zeros(16, np.uint16)
    assert L.bscgpu_fast_pstream_host(None, 0, N.np_ptr(e), 16) == -1
    assert L.bscgpu_fast_pstream_host(C.byref(fb.lay), fb.nsub, N.np_ptr(e), 16) == -1
    assert L.bscgpu_fast_pstream_host(C.byref(fb.lay), -1, N.np_ptr(e), 16) == -1
    n = int(L.bscgpu_fast_pstream_host(C.byref(fb.lay), 0, None, 0))               # counting only
    assert n == int(poff[1]) - int(poff[0])
    assert L.bscgpu_front_batch_code_psf(C.byref(fb.lay), fb.count, N.np_ptr(ps), N.np_ptr(poff), N.np_ptr(out), 3) == -1
    assert L.bscgpu_front_batch_code_psf(C.byref(fb.lay), 0, None, N.np_ptr(poff), N.np_ptr(out), 3) == -1
    assert L.bscgpu_front_batch_code_psf(None, 0, N.np_ptr(ps), N.np_ptr(poff), N.np_ptr(out), 3) == -1


@pytest.mark.parametrize("name", ["mixed", "pass_of_4096", "chain_identity", "long_chain", "fill"])
def test_gpu_inputs_fit_the_device_models_capacity(name):
    """the passes the GPU tests expect the device to keep: capacity is the only exit such a pass can take with this coder"""
    blocks = dict(mixed=lambda: mb.mixed_batch(0), pass_of_4096=mb.pass_of_4096, chain_identity=mb.chain_identity_pass,
                  long_chain=mb.long_chain_pass, fill=mb.fill_pass)[name]()
    fb, _ = mb.layout(blocks)
    _, poff = fbi.host_streams(fb)
    cap = fbi.CAPACITY[name]
    print(f"{name}: {fb.m} runs, {int(poff[-1])} decisions, capacity {cap}")
    assert fb.m <= cap // 4, "runs within the context's bytes (FAIL_CAP otherwise)"
    assert int(poff[-1]) <= cap, "decisions within four per byte of the context (FAIL_CAP otherwise)"


def test_decline_input_exceeds_capacity():
    blocks = fbi.noise_pass()
    fb, _ = mb.layout(blocks)
    _, poff = fbi.host_streams(fb)
    n = sum(b.size for b in blocks)
    assert int(poff[-1]) > 10 * n > 4 * 2 * fbi.MIB, f"{int(poff[-1])} decisions for {n} bytes"


def test_long_chain_pass_must_replay():
    """the walk the GPU test's assertion on BSCGPU_CNT_DC_REPLAYS rests on: the pass holds a chain of strictly alternating bits longer
    than three evaluation chunks, and the fast model's bracket never closes under such a chain"""
    fb, _ = mb.layout(mb.long_chain_pass())
    chains = fbi.alternating_rank_first_chains(fb)
    print("alternating chains:", sorted(chains)[-4:])
    assert fbi.bracket_stays_open_under_alternating_bits()
    assert fbi.replay_must_happen(fb)
    # the walk's premise against the coder's own decisions: in the stand-in's stream the first entry of a run is its "rank != 1"
    # decision, and for a symbol of such a chain its coded bit alternates over the symbol's runs
    seen = 0
    for s in range(fb.nsub):
        r0, r1 = int(fb.sub_run[s]), int(fb.sub_run[s + 1])
        sym, rank = fb.sym[r0:r1], fb.rank[r0:r1]
        if r1 - r0 < 3 * fbi.DC_EV:
            continue
        ps = gpu.fast_pstream_host(fb, s)
        first = ps[(ps & fbi.PSF_RUN) != 0]
        assert first.size == r1 - r0 and not (first & fbi.PSF_SIDE).any()
        for c in np.unique(sym):
            bits = ((first[sym == c] & fbi.PSF_BIT) != 0)
            assert np.array_equal(bits, rank[sym == c] != 1)
            if bits.size >= 3 * fbi.DC_EV and (bits[1:] != bits[:-1]).all():
                seen += 1
    assert seen >= 1
    fb, _ = mb.layout(mb.chain_identity_pass())
    assert not fbi.replay_must_happen(fb)
