"""The range coder on the GPU (csrc/device/rangecoder.hip, include/bscgpu.h bscgpu_rc_encode*): many probability streams in one launch,
one lane per stream, and the opt-in route of a device-model block through it (BSCGPU_OPT_DEVICE_RC).

Every stage case is compared with the CPU stand-in rc_encode_host (which test_rc_streams_host.py pins to the reference and to a Python
twin) on res[] and on the bytes, at 64, 8 and 1 streams per wavefront; the output buffer is filled with a pattern first, and every byte
outside the streams' regions must still carry it afterwards.  Everything is bit-exact."""
import ctypes as C

import numpy as np
import pytest

import devcoder_inputs as di
import rc_inputs as ri

pytestmark = pytest.mark.gpu

SPW = [64, 8, 1]
FORMS = [ri.STATIC16, ri.STATIC13, ri.FAST16]
PATTERN = 0xa5


@pytest.fixture(scope="module")
def ctx():
    from libbsc_amd import GpuContext
    c = GpuContext(0, max_n=(16 << 20) + 4096)
    yield c
    c.close()


def _body(form, rng, n, kind="random"):
    """n decisions of body in 16-bit entries of the form's kind (the packed form is made from them per stream: _pack)"""
    if form == ri.FAST16:
        return ri.random_fast(rng, n)
    return ri.skewed_static(rng, n) if kind == "skewed" else ri.random_static(rng, n)


def _place(form, entries16, streams):
    """the body array a launch reads: 16-bit forms take the entries as they are; the packed form gets every stream's entries packed
    at its own start (decision index in the packed space, a multiple of 8), the 16-bit stream positions being the same numbers"""
    if form != ri.STATIC13:
        return entries16
    end = max([s[0] + (s[1] + 7) // 8 * 8 for s in streams], default=0)
    out = np.zeros(end // 8 * 13 + 16, np.uint8)
    for s in streams:
        p = ri.pack_p13(entries16[s[0]:s[0] + s[1]])
        out[s[0] // 8 * 13:s[0] // 8 * 13 + p.size] = p
    return out


def _check(ctx, form, entries16, prefix, streams, spw):
    from libbsc_amd import gpu
    body = _place(form, entries16, streams)
    nout = max(s[4] + s[5] + 64 for s in streams) + 96
    fill = np.full(nout, PATTERN, np.uint8)
    want_res, want = gpu.rc_encode_host(form, body, prefix, streams, out=fill)
    res, out = ctx.rc_encode(form, body, prefix, streams, streams_per_wave=spw, out=fill)
    assert res == want_res, (form, spw, [(i, a, b) for i, (a, b) in enumerate(zip(res, want_res)) if a != b][:5])
    owned = np.zeros(nout, bool)
    for s, r in zip(streams, res):
        owned[s[4]:s[4] + s[5] + 64] = True
        if r >= 0:
            assert r <= s[5] + 64
            assert np.array_equal(out[s[4]:s[4] + r], want[s[4]:s[4] + r]), (form, spw, s)
    assert (out[~owned] == PATTERN).all(), (form, spw, "bytes outside every region were written")
    return res


@pytest.mark.parametrize("spw", SPW)
@pytest.mark.parametrize("form", FORMS)
def test_lengths_around_the_refill(ctx, form, spw):
    """body lengths around the refill size in ONE launch (a wavefront holds unequal lengths, some of them none), prefixes around the
    prefix refill (half as many entries); regions back to back at even, otherwise unaligned offsets with a gap behind each"""
    from libbsc_amd import gpu
    R = gpu.RC_REFILL
    rng = np.random.default_rng(100 + form)
    counts = [0, 1, 7, 8, 9, 63, 64, 65, R - 1, R, R + 1, 2 * R + 3]
    npre = [0, 1, R // 2 - 1, R // 2, R // 2 + 1, R + 2, 0, 33, 2, 64, 5, R // 2]
    st, nbody, _ = ri.lay_out(counts, [101 + 2 * c for c in counts], nprefix=npre, canary=30, form=form)
    res = _check(ctx, form, _body(form, rng, nbody + 8), ri.plain_prefix(rng, sum(npre)), st, spw)
    assert all(r > 0 for r in res)


@pytest.mark.parametrize("spw", SPW)
@pytest.mark.parametrize("count", [1, 8, 63, 64, 65, 200])
def test_stream_counts(ctx, count, spw):
    """the last wavefront need not be full"""
    rng = np.random.default_rng(count)
    for form in FORMS:
        counts = rng.integers(0, 300, count).tolist()
        npre = rng.integers(0, 70, count).tolist()
        st, nbody, _ = ri.lay_out(counts, [600] * count, nprefix=npre, form=form)
        _check(ctx, form, _body(form, rng, nbody + 8), ri.plain_prefix(rng, sum(npre)), st, spw)


@pytest.mark.parametrize("spw", SPW)
def test_body_alignment(ctx, spw):
    """16-bit bodies that start at odd entry indexes (a 2-byte-aligned address, staged by aligned 16-byte loads all the same) and packed
    bodies that start at multiples of 8 decisions which are not multiples of 64 (any byte alignment)"""
    rng = np.random.default_rng(7)
    counts = [301, 77, 1, 515, 129, 255, 65, 9]
    for form in (ri.STATIC16, ri.FAST16):
        st, nbody, _ = ri.lay_out(counts, [400] * len(counts), body_first=1, body_gap=1, form=form)
        assert all(s[0] % 2 == 1 for s in st)
        _check(ctx, form, _body(form, rng, nbody + 8), np.zeros(0, np.uint32), st, spw)
    st, at = [], 8
    for k, c in enumerate(counts):
        at += 8 * (at % 64 == 0)                                   # never on a multiple of 64
        st.append((at, c, 0, 0, 464 * k, 400))
        at = (at + c + 7) // 8 * 8
    nbody = at
    assert all(s[0] % 8 == 0 and s[0] % 64 != 0 for s in st), [s[0] for s in st]
    assert len({s[0] // 8 * 13 % 16 for s in st}) >= 4                                # several byte alignments
    _check(ctx, ri.STATIC13, _body(ri.STATIC13, rng, nbody + 8), np.zeros(0, np.uint32), st, spw)


@pytest.mark.parametrize("spw", SPW)
def test_long_outputs_and_canaries(ctx, spw):
    """streams of a few kilobytes of output (many 32-byte pieces), regions back to back with 32 bytes of pattern behind each: _check
    asserts the pattern is intact"""
    rng = np.random.default_rng(9)
    counts = [5000, 12000, 3, 7000]
    for form in FORMS:
        st, nbody, _ = ri.lay_out(counts, [1201, 3000, 40, 2001], nprefix=[40, 0, 3, 100], canary=32, form=form)
        res = _check(ctx, form, _body(form, rng, nbody + 8), ri.plain_prefix(rng, 143), st, spw)
        assert min(res) > 0 and max(res) > 1500


STEERED, _STEERED_TWIN = ri.steered(5, 20_000)
STEERED_CARRIES2 = _STEERED_TWIN.carries2
STEERED_BYTES = _STEERED_TWIN.finish()


@pytest.mark.parametrize("spw", SPW)
def test_steered_stream_beside_ordinary_ones(ctx, spw):
    """carries into two and more pending units (the twin counted them), in a lane between ordinary streams"""
    assert STEERED_CARRIES2 >= 100
    rng = np.random.default_rng(11)
    a, b = ri.random_static(rng, 904), ri.skewed_static(rng, 4000)
    entries = np.concatenate([a, STEERED, b])
    st, _, _ = ri.lay_out([a.size, STEERED.size, b.size], [400, 9000, 3000], form=ri.STATIC13)
    assert [s[0] for s in st] == [0, 904, 20904]                   # multiples of 8: the same layout serves the packed form
    for form in (ri.STATIC16, ri.STATIC13):
        res = _check(ctx, form, entries, np.zeros(0, np.uint32), st, spw)
        assert res[1] == len(STEERED_BYTES) and res[0] > 0 and res[2] > 0


@pytest.mark.parametrize("spw", SPW)
@pytest.mark.parametrize("form", FORMS)
def test_budget(ctx, form, spw):
    """three streams in one wavefront, the middle one coin flips with a small out_size: NOT_COMPRESSIBLE there, the neighbours right,
    nothing behind any region"""
    rng = np.random.default_rng(13 + form)
    n = 6000
    left, right = _body(form, rng, 704), _body(form, rng, 1300)
    flips = ri.coin_flips(n, ri.FAST16 if form == ri.FAST16 else ri.STATIC16)
    entries = np.concatenate([left, flips, right])
    st = [(0, 700, 0, 0, 0, 500), (704, n, 0, 0, 566, n // 16), (704 + n, 1300, 0, 0, 1008, 1000)]      # 566 + 375 + 64 = 1005
    res = _check(ctx, form, entries, np.zeros(0, np.uint32), st, spw)
    assert res[1] == ri.NOT_COMPRESSIBLE and res[0] > 0 and res[2] > 0


@pytest.mark.parametrize("spw", SPW)
def test_fast_form_mixes_both_precisions(ctx, spw):
    rng = np.random.default_rng(17)
    e = ri.random_fast(rng, 3000)
    assert (e >> 15).any() and not (e >> 15).all()
    pre = np.concatenate([ri.plain_prefix(rng, 32), (np.uint32(1) | (np.uint32(1) << 16) | (rng.integers(0, 2, 50).astype(np.uint32) << 24))])
    st = [(0, 1500, 0, 82, 0, 2000), (1500, 1500, 0, 82, 2064, 2000)]
    res = _check(ctx, ri.FAST16, e, pre.astype(np.uint32), st, spw)
    assert min(res) > 0


def test_bad_arguments_launch_nothing(ctx):
    from libbsc_amd import gpu
    e = np.zeros(64, np.uint16)
    with pytest.raises(gpu.GpuError):
        ctx.rc_encode(ri.STATIC16, e, np.zeros(0, np.uint32), [(0, 10, 0, 0, 0, 100)], streams_per_wave=16)
    with pytest.raises(gpu.GpuError):
        ctx.rc_encode(ri.STATIC16, e, np.zeros(0, np.uint32), [(60, 10, 0, 0, 0, 100)])
    res, out = ctx.rc_encode(ri.STATIC16, e, np.zeros(0, np.uint32), [])
    assert res == []


# ---- the block route -------------------------------------------------------------------------------------------------------------
_REF = {}


def _ref_block(ref, key, T, coder):
    if (key, coder) not in _REF:
        _REF[(key, coder)] = ref.compress(T, 1, coder)
    return _REF[(key, coder)]


def _pcounters():
    from libbsc_amd import _native
    lib = _native.lib()
    lib.bscgpu_process_counter.restype = C.c_longlong
    lib.bscgpu_process_counter.argtypes = [C.c_int]
    return [lib.bscgpu_process_counter(k) for k in (1, 2)]          # device-model blocks, blocks redone on the host model


def _both_routes(ctx, T, coder):
    """compress_device with the option off and on -> (bytes off, bytes on, blocks the device range coder took, process counters' deltas on)"""
    import torch
    d = torch.from_numpy(T).cuda()
    assert ctx.option_get(ctx.OPT_DEVICE_RC) == 0                   # the default
    off = ctx.compress_device(d, T.size, 1, coder).tobytes()
    c0, p0 = ctx.option_get(ctx.CNT_DEVICE_RC_BLOCKS), _pcounters()
    assert ctx.option_set(ctx.OPT_DEVICE_RC, 1) == 0
    try:
        on = ctx.compress_device(d, T.size, 1, coder).tobytes()
    finally:
        ctx.option_set(ctx.OPT_DEVICE_RC, 0)
    p1 = _pcounters()
    return off, on, ctx.option_get(ctx.CNT_DEVICE_RC_BLOCKS) - c0, [b - a for a, b in zip(p0, p1)]


@pytest.mark.parametrize("coder", [1, 3])
@pytest.mark.parametrize("mib", [1, 5])
def test_block_route_is_byte_identical(ctx, ref, mib, coder):
    """1 MiB and 5 MiB text blocks (2 and 4 sub-blocks): the option on = the option off = the compiled reference; one block counted"""
    from libbsc_amd import api
    T = api.synth_text_v1(30 + mib, mib << 20)
    off, on, took, (dm, redo) = _both_routes(ctx, T, coder)
    assert took == 1 and dm == 1 and redo == 0
    assert on == off
    assert on == _ref_block(ref, mib, T, coder)


def test_block_route_with_16_bit_entries(ctx, ref):
    """the static coder's stream as 16-bit entries (OPT_DC_PACKED_STREAM 0): the other body form of the same route"""
    from libbsc_amd import api
    T = api.synth_text_v1(31, 1 << 20)
    assert ctx.option_set(ctx.OPT_DC_PACKED_STREAM, 0) == 1
    try:
        off, on, took, (dm, redo) = _both_routes(ctx, T, 1)
    finally:
        ctx.option_set(ctx.OPT_DC_PACKED_STREAM, 1)
    assert took == 1 and dm == 1 and redo == 0
    assert on == off == _ref_block(ref, 1, T, 1)


def test_incompressible_sub_block_redoes_the_block(ctx, ref, coder=1):
    """2 MiB whose second half is random bytes (the first: one letter): half a run per byte, so the model takes it, and the second
    sub-block of the sorted block is random bytes that do not fit their budget — the stream ends NOT_COMPRESSIBLE on the device as on
    the host, the block is redone on the host model, same bytes both ways"""
    rng = np.random.default_rng(21)
    T = np.concatenate([np.full(1 << 20, 97, np.uint8), rng.integers(0, 256, 1 << 20, dtype=np.uint8)])
    off, on, took, (dm, redo) = _both_routes(ctx, T, coder)
    assert took == 1 and dm == 1 and redo == 1, (took, dm, redo)
    assert on == off == _ref_block(ref, "half random", T, coder)


def test_declined_block_takes_the_host_route(ctx, ref):
    """a block the model declines (undecided avg_rank flags): bytes unchanged, not counted"""
    T = di.text_with_bwt_like(di.WHOLE_BLOCKS["fail_avg"][2]())
    off, on, took, (dm, redo) = _both_routes(ctx, T, 1)
    assert ctx.option_get(ctx.CNT_DC_LAST_FAIL) == di.FAIL_AVG
    assert took == 0 and dm == 0 and redo == 0
    assert on == off == _ref_block(ref, "fail_avg", T, 1)
