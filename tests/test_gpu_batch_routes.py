"""Every route a pass of the compress-batch calls can take, on one fixed batch: each block's bytes against the reference, host input
against input in HBM, and the counters a call moves against pipeline_model.batch_call — the driver's decisions restated — given that
the device kept every stream."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from pipeline_model import BATCH_MAX_N, batch_call

pytestmark = pytest.mark.gpu

MAX_N = 4 << 20
# what a block larger than the context comes to: host input LIBBSC_GPU_NOT_ENOUGH_MEMORY (bsc_compress on the context), input in HBM
# LIBBSC_BAD_PARAMETER (bscgpu_compress_device)
TOO_LARGE = {False: -9, True: -1}
ROUTES = {                                                      # name: (coder, the options that are on)
    "l_down": (1, ()), "front": (1, ("front",)), "model": (1, ("front", "model")), "packed": (1, ("front", "model", "packed")),
    "segments": (1, ("front", "model", "segments")), "segments_packed": (1, ("front", "model", "segments", "packed")),
    "fast": (3, ("front", "fast")), "device_rc": (1, ("front", "model", "device_rc")),
}


@pytest.fixture(autouse=True)
def every_pass_size_goes_to_the_model(monkeypatch):
    monkeypatch.setenv("BSC_BATCH_MODEL_MIN_PASS", "0")


@pytest.fixture(scope="module")
def ctx():
    from libbsc_amd import GpuContext
    c = GpuContext(0, max_n=MAX_N)
    yield c
    c.close()


def _batch():
    """about 60 blocks, 10 MiB of them in three passes: text of 120 .. 200 KB, among it the short, the empty and the stored; then
    one block for the pipe and one that is larger than the context"""
    from libbsc_amd.api import synth_text_v1
    rng = np.random.default_rng(20261020)
    cuts = np.concatenate([[0], np.cumsum(rng.integers(120_000, 200_001, 54))])
    text = synth_text_v1(3000, int(cuts[-1]))
    blocks = [text[cuts[i]:cuts[i + 1]].copy() for i in range(54)]
    small = [synth_text_v1(4000 + n, n) for n in (1, 27, 28, 29, 30)] + [rng.integers(0, 256, 3000, dtype=np.uint8)]
    for k, s in enumerate(small):
        blocks.insert(5 + 9 * k, s)
    empty = np.zeros(0, np.uint8)
    for at in (40, 20, 0):
        blocks.insert(at, empty)
    return blocks + [synth_text_v1(5000, BATCH_MAX_N), np.full(MAX_N + 5000, 97, np.uint8), empty]


@pytest.fixture(scope="module")
def batch(ref):
    blocks = _batch()
    with ThreadPoolExecutor(8) as pool:                          # (the reference once per coder, shared by the routes)
        want = {coder: list(pool.map(lambda b: None if b.size > MAX_N else ref.compress(b, 1, coder), blocks)) for coder in (1, 3)}
    return blocks, want


def _counters(c):
    keys = ("FRONT_PASSES", "L_PASSES", "MODEL_PASSES", "MODEL_DECLINED", "FAST_PASSES", "FAST_DECLINED", "SEGMENTS", "SEG_RERUNS", "SEG_HOST_BLOCKS",
            "PACKED_PASSES", "PACKED_VOID")
    out = {k: c.option_get(getattr(c, "CNT_BATCH_" + k)) for k in keys}
    out["DEVICE_RC_BLOCKS"] = c.option_get(c.CNT_DEVICE_RC_BLOCKS)
    return out


def _call(c, on, fn):
    keys = dict(front=c.OPT_BATCH_FRONT, model=c.OPT_BATCH_MODEL, fast=c.OPT_BATCH_MODEL_FAST, segments=c.OPT_BATCH_MODEL_SEGMENTS,
                packed=c.OPT_BATCH_MODEL_PACKED, device_rc=c.OPT_DEVICE_RC)
    old = {k: c.option_set(key, int(k in on)) for k, key in keys.items()}
    try:
        c0 = _counters(c)
        out = fn()
        return out, {k: v - c0[k] for k, v in _counters(c).items()}
    finally:
        for k, key in keys.items():
            c.option_set(key, old[k])


def _restated(sizes, coder, on, dev, lz=None):
    """the counters the call moves when the device keeps every stream: no pass declines, every stream has landing room and its packed
    form, and a segmented pass is one segment (its decisions are below the arena's 4 per byte of the context)"""
    opts = {k: int(k in on) for k in ("front", "model", "fast", "segments", "packed", "device_rc")}
    kept = {p: dict(nsub=1, mrc=0, D=0, pk=1, pbytes=0) for p in range(len(sizes))}
    r = batch_call(sizes, 1, coder, MAX_N, dev, lz or sizes, opts, kept, 1 << 40, min_pass=0)
    total = lambda k: sum(p["counters"][k] for p in r["passes"])
    segs = sum(p["step"] == "segments" for p in r["passes"])
    want = dict(FRONT_PASSES=total("front"), L_PASSES=total("l"), MODEL_PASSES=total("model"), MODEL_DECLINED=total("declined"), FAST_PASSES=total("fast"),
                FAST_DECLINED=total("fast_declined"), SEGMENTS=segs, SEG_RERUNS=0, SEG_HOST_BLOCKS=0,
                PACKED_PASSES=total("packed") + (segs if r["route"][4] else 0), PACKED_VOID=total("void"), DEVICE_RC_BLOCKS=total("device_rc"))
    return r, want


@pytest.mark.parametrize("route", sorted(ROUTES))
def test_route(ctx, batch, route):
    import torch
    blocks, want = batch
    coder, on = ROUTES[route]
    sizes = [int(b.size) for b in blocks]
    got, moved = _call(ctx, on, lambda: ctx.compress_batch(blocks, 1, coder))
    flat = torch.from_numpy(np.concatenate(blocks)).cuda()
    got_d, moved_d = _call(ctx, on, lambda: ctx.compress_batch_device(flat, sizes, 1, coder))
    for dev, (out, cnt) in enumerate(((got, moved), (got_d, moved_d))):
        r, counters = _restated(sizes, coder, on, bool(dev))
        print(route, "dev" if dev else "host", cnt, flush=True)
        assert r["npass"] == 3 and r["leftover"][-3:-1] == ["pipe", "one_by_one"]
        # (the block that goes through the pipe is of the size the single-block path gives to the device model: with the device's range
        # coder on, that path counts it too)
        counters["DEVICE_RC_BLOCKS"] += sum(k == "pipe" and n >= BATCH_MAX_N for k, n in zip(r["leftover"], sizes)) if "device_rc" in on else 0
        assert cnt == counters, f"{route}, {'HBM' if dev else 'host'} input: counters moved {cnt}, restated {counters}"
        for b, (g, w) in enumerate(zip(out, want[coder])):
            w = TOO_LARGE[bool(dev)] if w is None else w
            assert g == w, f"{route}, {'HBM' if dev else 'host'} input: block {b} ({sizes[b]} bytes) differs from the reference"
    assert [g for g, w in zip(got_d, want[coder]) if w is not None] == [g for g, w in zip(got, want[coder]) if w is not None]
    stored = sizes.index(3000)
    assert len(got[stored]) == 3000 + 28, "the random block is stored"


def test_lzp_call(ctx, ref):
    """A call with LZP (15, 128) that holds 4096 zeros.  The block was meant to reach the class "left to the single path" (a sorter input
    under 16 bytes); the reference's LZP never leaves so little: 177 bytes of these zeros, and at least 40 of any constant block of 29
    bytes .. 64 KiB at any minimum length (smaller ones it refuses), so on real input the class is out of reach and the host probe
    (test_batch_pass_plan_host.py) is what covers it.  Held here: the LZP route's bytes and counters."""
    from libbsc_amd.api import synth_text_v1
    blocks = [synth_text_v1(6000, 50_000), np.zeros(4096, np.uint8), synth_text_v1(6001, 30_000)]
    want = [ref.compress(b, 1, 1, 15, 128) for b in blocks]
    lz = [ref.lzp_compress(b, 15, 128) for b in blocks]
    lz = [b.size if isinstance(z, int) else len(z) for b, z in zip(blocks, lz)]
    assert lz[1] == 177
    got, moved = _call(ctx, ("front", "model"), lambda: ctx.compress_batch(blocks, 1, 1, 15, 128))
    assert got == want
    r, counters = _restated([b.size for b in blocks], 1, ("front", "model"), False, lz=lz)
    assert r["passes"][0]["classes"] == ["sorted"] * 3 and r["passes"][0]["pos"] == sum(lz) and r["leftover"] == ["none"] * 3
    assert moved == counters
