"""The LZP encoder stage on the GPU (csrc/device/lzp.hip): bscgpu_lzp_compress from host memory and
bscgpu_lzp_compress_device from HBM must give what api.bsc_lzp_compress gives (and the reference, where it was built), with the path
counters of the CPU stand-in; the opt-in route (BSCGPU_OPT_DEVICE_LZP) and bscgpu_compress_device_lzp must give bsc_compress's bytes.
Inputs and the host encoder's answers: tests/lzp_device_inputs.py."""
import ctypes as C
import hashlib
import json
import os

import numpy as np
import pytest

import lzp_device_inputs as I
from libbsc_amd import api, gpu

pytestmark = pytest.mark.gpu

MAX_N = (4 << 20) + 4096


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but torch.cuda.is_available() is False")
    return torch


@pytest.fixture(scope="module")
def ctx(torch_cuda):
    from libbsc_amd import GpuContext
    c = GpuContext(0, max_n=MAX_N)
    yield c
    c.close()


@pytest.fixture(scope="module")
def reference():
    """the compiled reference where it was built (oracle/_ref), else None: the host encoder, which the CPU tests pin to it, stands in"""
    from oracle.refbind import REF_SO, Ref
    return Ref() if os.path.exists(REF_SO) else None


def _check(ctx, torch, key, T, h, m, f, reference=None):
    want = I.want(key, T, h, m, f)
    if reference is not None:
        assert reference.lzp_compress(T, h, m, features=f) == want, (key, h, m, f, "host encoder vs reference")
    _, cnt = gpu.lzp_staged_host(T, h, m, features=f)
    got = ctx.lzp_compress(T, h, m, features=f)
    assert got == want, (key, h, m, f, "host pointers")
    assert ctx.lzp_counters() == cnt, (key, h, m, f, "host pointers")
    d = torch.from_numpy(T).cuda()
    got = ctx.lzp_compress(d, h, m, features=f, device=True)
    assert got == want, (key, h, m, f, "HBM")
    assert ctx.lzp_counters() == cnt, (key, h, m, f, "HBM")
    assert d.cpu().numpy().tobytes() == T.tobytes(), "the input in HBM is the caller's"
    return cnt


@pytest.mark.parametrize("features", I.FEATURES)
@pytest.mark.parametrize("name", list(I.corpora()))
def test_stage_equals_host_encoder(ctx, torch_cuda, reference, name, features):
    T = I.corpora()[name]
    for h in I.HASHES:
        for m in I.MINLENS:
            _check(ctx, torch_cuda, name, T, h, m, features, reference if features == 3 and h == 15 else None)


def test_stage_tiny_sizes(ctx, torch_cuda):
    """the 1500 tiny inputs, both entry points, counters included: refused sizes, chunks that are all last stretch and tail"""
    for it, (T, h, m, f) in enumerate(I.tiny_cases()):
        _check(ctx, torch_cuda, ("tiny", it), T, h, m, f)
    assert ctx.lzp_compress(np.zeros(0, np.uint8), 15, 32) == api.NOT_COMPRESSIBLE


@pytest.mark.parametrize("features", I.FEATURES)
def test_stage_chunk_thresholds(ctx, torch_cuda, reference, features):
    big = I.threshold_block()
    for n in I.THRESHOLD_SIZES + ((4 << 20) + 5,):
        _check(ctx, torch_cuda, ("threshold", n), big[:n], 15, 32, features, reference)


@pytest.mark.parametrize("features", I.FEATURES)
def test_stage_first_chunk_kept_raw(ctx, torch_cuda, reference, features):
    cnt = _check(ctx, torch_cuda, "first_chunk_raw", I.first_chunk_raw(), 15, 32, features, reference)
    assert cnt["raw_chunks"] == 1


@pytest.mark.parametrize("name", list(I.PATHS))
def test_stage_takes_every_path(ctx, torch_cuda, name):
    make, h, m, f, counter = I.PATHS[name]
    cnt = _check(ctx, torch_cuda, ("path", name), make(), h, m, f)
    if counter is None:
        assert I.want(("path", name), make(), h, m, f) == api.NOT_COMPRESSIBLE
    else:
        assert cnt[counter] > 0, (name, cnt)


def test_stage_declines_wide_tables_and_bad_parameters(ctx, torch_cuda):
    T = np.zeros(1000, np.uint8)
    d = torch_cuda.from_numpy(T).cuda()
    for h in (16, 17, 18):
        assert ctx.lzp_compress(T, h, 32) == gpu.NOT_SUPPORTED
        assert ctx.lzp_compress(d, h, 32, device=True) == gpu.NOT_SUPPORTED
    for h, m in ((9, 32), (29, 32), (15, 3), (15, 256)):
        assert ctx.lzp_compress(T, h, m) == api.BAD_PARAMETER
    assert ctx.lzp_compress(np.zeros(40, np.uint8), 15, 32) == api.NOT_COMPRESSIBLE
    st = ctx.profile_get()
    assert "lzp" in st


@pytest.mark.parametrize("minlen", [8, 32, 128])
def test_stage_eight_chunks_golden(torch_cuda, minlen):
    """the committed 17 MiB vectors of the reference (tests/golden/lzp_golden.json): eight chunks, -H15, both framings"""
    from libbsc_amd import GpuContext
    from libbsc_amd.synth import synth_repeat_v1
    gold = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "lzp_golden.json")))
    rows = [e for e in gold["stage"] if e["n"] > (6 << 20) and e["hash"] == 15 and e["minlen"] == minlen]
    assert len(rows) == 2
    T = synth_repeat_v1(rows[0]["seed"], rows[0]["n"], rows[0]["period"])
    c = GpuContext(0, max_n=T.size + 4096)
    try:
        c.profile(True)
        for e in rows:
            got = c.lzp_compress(T, 15, minlen, features=e["features"])
            assert len(got) == e["size"] and hashlib.md5(got).hexdigest() == e["md5"], e
            assert got[0] == 8 and c.lzp_counters()["matches"] > 0
        st = c.profile_get()
        # two calls, four ranges each: key; link + flag; sweep; frame
        assert st["lzp"]["launches"] == 8 and st["lzp"]["ms"] > 0 and st["radix_aux"]["launches"] > 0, "the stage is a class of its own in the profile"
    finally:
        c.close()


@pytest.mark.parametrize("features", I.FEATURES)
@pytest.mark.parametrize("name", ["first_chunk_raw", "two_chunks"])
def test_stage_output_over_input(ctx, torch_cuda, name, features):
    """bscgpu_lzp_compress_device with dOut == dIn: the stage works on its own copy of the block, so a chunk kept raw — read when the
    output is already being written — and the coded chunks come out as with an output of their own"""
    key, T = {"first_chunk_raw": ("first_chunk_raw", I.first_chunk_raw()),
              "two_chunks": (("threshold", 256 * 1024), I.threshold_block()[:256 * 1024])}[name]
    want = I.want(key, T, 15, 32, features)
    assert not isinstance(want, int) and want[0] == 2
    d = torch_cuda.from_numpy(T).cuda()
    r = ctx.L.bscgpu_lzp_compress_device(ctx.h, d.data_ptr(), d.data_ptr(), T.size, 15, 32, features)
    assert r == len(want), (name, features)
    assert d[:r].cpu().numpy().tobytes() == want, (name, features)
    if name == "first_chunk_raw":
        assert ctx.lzp_counters()["raw_chunks"] == 1


def test_stage_tables_are_counted_once(torch_cuda):
    """a single block allocates the stage's tables on first use (test_gpu_lzp_batch.py: test_tables_are_counted's bounds); the next
    block and a pass on the same context find them there"""
    from libbsc_amd import GpuContext
    c = GpuContext(0, max_n=1 << 20)
    try:
        before = c.arena_bytes
        T = I.corpora()["zeros"]
        want = I.want("zeros", T, 15, 32, 3)
        assert c.lzp_compress(T, 15, 32, features=3) == want
        grown = c.arena_bytes - before
        assert 600_000 < grown < 800_000, grown
        assert c.lzp_compress(T, 15, 32, features=3) == want
        assert c.arena_bytes - before == grown
        assert c.lzp_compress_batch([T], None, 15, 32, 3) == [want]
        assert c.arena_bytes - before == grown
    finally:
        c.close()


@pytest.mark.parametrize("h,m", [(15, 8), (10, 40), (15, 128)])
def test_block_and_pass_share_the_kernels(ctx, torch_cuda, h, m):
    """one block of two chunks through lzp_compress and as a pass of one block through lzp_compress_batch: the same bytes, the same
    counters.  The block is the `text` corpus continued to 300 000 bytes (the corpus itself has 150 000, one chunk: the generator
    with the corpus's seed, whose first 150 000 bytes are the corpus)."""
    from libbsc_amd.synth import synth_text_v1
    T = synth_text_v1(3, 300_000)
    assert T[:150_000].tobytes() == I.corpora()["text"].tobytes()
    alone = ctx.lzp_compress(T, h, m, features=3)
    cnt = ctx.lzp_counters()
    assert alone == I.want(("text300k",), T, h, m, 3)
    assert ctx.lzp_compress_batch([T], None, h, m, 3) == [alone]
    assert ctx.lzp_counters() == cnt


# ---- the route -------------------------------------------------------------------------------------------------------------------------
def _pcnt(key):
    L = gpu.N.lib()
    L.bscgpu_process_counter.restype = C.c_longlong
    L.bscgpu_process_counter.argtypes = [C.c_int]
    return L.bscgpu_process_counter(key)


PCNT_REDONE, PCNT_DEVICE_LZP = 2, 4


@pytest.fixture(scope="module")
def route_block():
    from libbsc_amd.synth import synth_repeat_v1
    return synth_repeat_v1(9, (2 << 20) + 77, 40_000, 48)


@pytest.mark.parametrize("sorter", [1, 5])
def test_route_equals_host_route(ctx, torch_cuda, route_block, monkeypatch, sorter):
    """bsc_compress (which takes the route from BSC_DEVICE_LZP as it stands at the call) and Pipe.submit_host, -H15 with -M32 and -M128,
    the three coders: the option changes the route, not a byte"""
    T = route_block
    pipe = ctx.pipe(2)
    try:
        for m in (32, 128):
            for coder in (1, 2, 3):
                monkeypatch.delenv("BSC_DEVICE_LZP", raising=False)
                want = api.bsc_compress(T, sorter, coder, lzp_hash=15, lzp_min=m)
                assert not isinstance(want, int) and (want[9] != 0 or want[10] != 0), "the mode word says LZP stayed on"
                monkeypatch.setenv("BSC_DEVICE_LZP", "1")
                p0 = _pcnt(PCNT_DEVICE_LZP)
                assert api.bsc_compress(T, sorter, coder, lzp_hash=15, lzp_min=m) == want, (sorter, coder, m, "bsc_compress")
                assert _pcnt(PCNT_DEVICE_LZP) > p0, "bsc_compress took the device stage"
                for on in (0, 1):
                    ctx.option_set(ctx.OPT_DEVICE_LZP, on)
                    b0 = ctx.option_get(ctx.CNT_LZP_BLOCKS)
                    got = pipe.wait(pipe.submit_host(T, sorter, coder, 15, m, 3)).tobytes()
                    assert got == want, (sorter, coder, m, on, "pipe")
                    assert ctx.option_get(ctx.CNT_LZP_BLOCKS) - b0 == on
    finally:
        ctx.option_set(ctx.OPT_DEVICE_LZP, 0)
        pipe.close()


def test_route_survives_a_redo(torch_cuda):
    """test_lzp_blocks_take_the_device_model_and_survive_a_redo's second input: LZP removes the copy of the noise, the sorted block's last
    sub-block is stored raw, the device-model block is redone on the host model — which uploads the raw block and runs the stage again"""
    from libbsc_amd import GpuContext
    from libbsc_amd.synth import synth_repeat_v1
    rng = np.random.default_rng(8)
    a = synth_repeat_v1(9, 8 << 20, 40_000, 48)
    lut = np.arange(256, dtype=np.uint8)
    for i, v in enumerate([10, 32] + list(range(97, 123))):
        lut[v] = i
    T = np.concatenate([lut[a], rng.integers(0, 256, 2_000_000, dtype=np.uint8)])
    want = api.bsc_compress(T, 1, 1, lzp_hash=15, lzp_min=32)
    c = GpuContext(0, max_n=T.size + 4096)
    pipe = c.pipe(2)
    try:
        c.option_set(c.OPT_DEVICE_LZP, 1)
        r0, b0 = _pcnt(PCNT_REDONE), c.option_get(c.CNT_LZP_BLOCKS)
        assert pipe.wait(pipe.submit_host(T, 1, 1, 15, 32, 3)).tobytes() == want
        assert _pcnt(PCNT_REDONE) - r0 == 1 and c.option_get(c.CNT_LZP_BLOCKS) - b0 == 2, "redone once: the stage ran twice"
        d = torch_cuda.from_numpy(T).cuda()
        assert c.compress_device(d, T.size, 1, 1, lzp_hash=15, lzp_min=32).tobytes() == want
        assert _pcnt(PCNT_REDONE) - r0 == 2
    finally:
        pipe.close(); c.close()


def test_route_random_block_goes_on_without_lzp(ctx, torch_cuda):
    T = np.random.default_rng(3).integers(0, 256, 1_000_000, dtype=np.uint8)
    want = api.bsc_compress(T, 1, 1, lzp_hash=15, lzp_min=32)
    pipe = ctx.pipe(2)
    try:
        ctx.option_set(ctx.OPT_DEVICE_LZP, 1)
        b0 = ctx.option_get(ctx.CNT_LZP_BLOCKS)
        assert pipe.wait(pipe.submit_host(T, 1, 1, 15, 32, 3)).tobytes() == want
        assert ctx.option_get(ctx.CNT_LZP_BLOCKS) - b0 == 1
        d = torch_cuda.from_numpy(T).cuda()
        assert ctx.compress_device(d, T.size, 1, 1, lzp_hash=15, lzp_min=32).tobytes() == want
    finally:
        ctx.option_set(ctx.OPT_DEVICE_LZP, 0)
        pipe.close()


def test_route_declines_wide_tables(torch_cuda, route_block):
    from libbsc_amd import GpuContext, GpuError
    T = route_block[:1_000_000]
    want = api.bsc_compress(T, 1, 1, lzp_hash=18, lzp_min=32)
    c = GpuContext(0, max_n=T.size + 4096)
    pipe = c.pipe(2)
    try:
        c.option_set(c.OPT_DEVICE_LZP, 1)
        assert pipe.wait(pipe.submit_host(T, 1, 1, 18, 32, 3)).tobytes() == want
        assert c.option_get(c.CNT_LZP_BLOCKS) == 0 and c.option_get(c.CNT_LZP_DECLINED) == 1
        with pytest.raises(GpuError) as e:
            c.compress_device(torch_cuda.from_numpy(T).cuda(), T.size, 1, 1, lzp_hash=18, lzp_min=32)
        assert e.value.code == gpu.NOT_SUPPORTED
    finally:
        pipe.close(); c.close()


@pytest.mark.parametrize("sorter,coder", [(1, 1), (1, 2), (5, 3)])
def test_compress_device_with_lzp(ctx, torch_cuda, route_block, sorter, coder):
    """bsc_compress's full parameter list for input in HBM"""
    T = route_block
    d = torch_cuda.from_numpy(T).cuda()
    for m in (32, 128):
        want = api.bsc_compress(T, sorter, coder, lzp_hash=15, lzp_min=m)
        assert ctx.compress_device(d, T.size, sorter, coder, lzp_hash=15, lzp_min=m).tobytes() == want, (sorter, coder, m)
        assert api.bsc_decompress(want) == T.tobytes()
    assert ctx.compress_device(d, T.size, sorter, coder).tobytes() == api.bsc_compress(T, sorter, coder)
