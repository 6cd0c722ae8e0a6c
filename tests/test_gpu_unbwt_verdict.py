"""The GPU inverse BWT (unbwt.hip: bscgpu_unbwt, bscgpu_unbwt_batch_device) against the plain LF oracle of tests/unbwt_inputs.py:
on damaged (L, primary index) pairs the return code and, on 0, the text are fully determined — "-6 or some other text" is not a
verdict.  And the LIBBSC_NOT_SUPPORTED exits of the step cap, reached with BSC_UNBWT_STEP_CAP=64 in child processes."""
import os
import subprocess
import sys

import numpy as np
import pytest

import unbwt_inputs as U

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE = 4096                                  # ub_keys_batch_kernel's tile (UB_TILE)


@pytest.fixture(scope="module")
def vctx():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but torch.cuda.is_available() is False")
    from libbsc_amd import GpuContext
    c = GpuContext(0, max_n=(4 << 20) + 4096)
    yield c
    c.close()


def _sample(rng, pairs, per_class):
    """a seeded sample that holds every class"""
    out = []
    for cls in ("valid", "valid-other", "broken"):
        mine = [p for p in pairs if p.cls == cls]
        out += [mine[i] for i in rng.permutation(len(mine))[:per_class]]
    return out


def _check_single(ctx, p):
    out = np.full(p.L.size, 0xAB, np.uint8)
    back, rc = ctx.unbwt(p.L, p.idx, out=out)
    assert rc == p.rc, (p, rc)
    if rc == 0:
        assert np.array_equal(back, p.text), (p, "the text is not the oracle's")
    else:
        assert (out == 0xAB).all(), (p, "a refused block was written")


def test_single_block_verdict_small(vctx):
    pairs = _sample(np.random.default_rng(31), U.small_pairs(), 100)
    assert len(pairs) >= 230 and {p.cls for p in pairs} == {"valid", "valid-other", "broken"}
    for p in pairs:
        _check_single(vctx, p)


def test_single_block_verdict_large(vctx):
    for p in U.large_pairs():
        _check_single(vctx, p)


def _batch_order(rng):
    """the whole small list in seeded random order, with the 2- and 3-byte blocks as one run in the middle (over a hundred
    blocks inside one or two tiles of the keys kernel)"""
    rest = U.index_pairs() + U.column_pairs()
    rest = [rest[i] for i in rng.permutation(len(rest))]
    tiny = list(U.tiny_pairs()) + [p for p in rest if p.L.size <= 3]
    rest = [p for p in rest if p.L.size > 3]
    tiny = [tiny[i] for i in rng.permutation(len(tiny))]
    cut = len(rest) // 2
    return rest[:cut] + tiny + rest[cut:]


@pytest.mark.parametrize("in_place", [True, False])
def test_batched_verdict(vctx, in_place):
    import torch
    pairs = _batch_order(np.random.default_rng(32))
    sizes = [p.L.size for p in pairs]
    offs = np.concatenate([[0], np.cumsum(sizes)])
    assert len(pairs) > 4096, "more than one pass"
    # what the pass must hold: many tiny blocks inside one tile (counted straight into H), blocks that straddle tile ends, every class
    starts, ends = offs[:-1], offs[1:]
    tiny_in_tile = np.bincount((starts // TILE)[(np.array(sizes) <= 3) & (starts // TILE == (ends - 1) // TILE)])
    assert tiny_in_tile.max() >= 50, tiny_in_tile.max()
    assert int(((starts // TILE) != ((ends - 1) // TILE)).sum()) >= 100
    assert {p.cls for p in pairs} == {"valid", "valid-other", "broken"}
    flat = np.concatenate([p.L for p in pairs])
    dL = torch.from_numpy(flat.copy()).cuda()
    dT = None if in_place else torch.full((flat.size,), 0xAB, dtype=torch.uint8, device=dL.device)
    T, res = vctx.unbwt_batch(dL, sizes, [p.idx for p in pairs], dT=dT)
    Th = T.cpu().numpy()
    if not in_place:
        assert np.array_equal(dL.cpu().numpy(), flat), "the input was written"
    failed = 0
    for b, p in enumerate(pairs):
        got = Th[offs[b]:offs[b + 1]]
        assert res[b] == p.rc, (b, p, res[b])
        if p.rc == 0:
            assert np.array_equal(got, p.text), (b, p, "the text is not the oracle's")
        else:
            failed += 1
            want = p.L if in_place else np.full(p.L.size, 0xAB, np.uint8)
            assert np.array_equal(got, want), (b, p, "a refused block's range was written")
    assert failed >= 2000


def _child(code, **env):
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=dict(os.environ, **env), cwd=ROOT)
    assert r.returncode == 0 and "child ok" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
    return r.stdout


PRELUDE = """
import sys
sys.path.insert(0, 'tests')
import numpy as np
import unbwt_inputs as U
from libbsc_amd import api
"""


def test_stage_api_across_the_threshold():
    """BSC_GPU_UNBWT_MIN_N=2: bsc_bwt_decode sends every block to bscgpu_unbwt — the answer is the one the host walk gives without it"""
    code = PRELUDE + """
rng = np.random.default_rng(33)
pairs = []
for cls in ('valid', 'valid-other', 'broken'):
    mine = [p for p in U.small_pairs() if p.cls == cls]
    pairs += [mine[i] for i in rng.permutation(len(mine))[:100]]
accepted = 0
for p in pairs:
    back, rc = api.bsc_bwt_decode(p.L, p.idx)
    assert rc == p.rc, (p, rc)
    assert np.array_equal(back, p.text if rc == 0 else p.L), p
    accepted += int(p.cls == 'broken' and U.parent_host_rule(p.L, p.idx)[0] == 0)
print('child ok', len(pairs), accepted)
"""
    out = _child(code, BSC_GPU_UNBWT_MIN_N="2")
    assert int(out.split()[-2]) >= 230


# ---- the step cap: LIBBSC_NOT_SUPPORTED (-4) from a walk of more than BSC_UNBWT_STEP_CAP steps between two marked rows -------------------
def _cap_texts():
    from libbsc_amd.synth import synth_text_v1
    return [synth_text_v1(45, 40), synth_text_v1(46, 70_000), synth_text_v1(47, 17), np.zeros(50_000, np.uint8), synth_text_v1(48, 60)]


def test_step_cap_declines_single_blocks():
    code = PRELUDE + """
import torch
from libbsc_amd import GpuContext
from libbsc_amd.synth import synth_text_v1
ctx = GpuContext(0, max_n=(1 << 20) + 4096)
for seed, n, want in ((41, 300_000, -4), (45, 40, 0)):
    T = synth_text_v1(seed, n)
    L, idx = U.bwt(T)
    assert U.lf_verdict(L, idx)[0] == 0
    out = np.full(n, 0xAB, np.uint8)
    back, rc = ctx.unbwt(L, idx, out=out)
    assert rc == want, (n, rc)
    assert np.array_equal(out, T) if want == 0 else (out == 0xAB).all(), n
ctx.close()
print('child ok')
"""
    _child(code, BSC_UNBWT_STEP_CAP="64")


def test_step_cap_leaves_the_stage_api_to_the_host_walk():
    code = PRELUDE + """
from libbsc_amd.synth import synth_text_v1
T = synth_text_v1(41, 300_000)
L, idx = U.bwt(T)
back, rc = api.bsc_bwt_decode(L, idx)
assert rc == 0 and np.array_equal(back, T), rc
small = synth_text_v1(45, 40)
L, idx = U.bwt(small)
back, rc = api.bsc_bwt_decode(L, idx)
assert rc == 0 and np.array_equal(back, small), rc
print('child ok')
"""
    _child(code, BSC_UNBWT_STEP_CAP="64", BSC_GPU_UNBWT_MIN_N="2")


def test_step_cap_declines_blocks_of_a_batch(ref, tmp_path):
    """[40 bytes, 70 000 of text, 17 bytes, 50 000 zeros, 60 bytes] under a cap of 64: the long blocks are declined (-4, their range
    not written), their neighbours decode; whole blocks of the same texts decode through bsc_decompress for the declined ones"""
    texts = _cap_texts()
    files = {}
    for i, T in enumerate(texts):
        files[f"t{i}"] = T
        files[f"e1_{i}"] = np.frombuffer(ref.compress(T, 1, 1), np.uint8)
        files[f"lzp_{i}"] = np.frombuffer(ref.compress(T, 1, 1, 15, 128), np.uint8)
    path = str(tmp_path / "cap.npz")
    np.savez(path, **files)
    code = PRELUDE + f"""
import torch
from libbsc_amd import GpuContext
z = np.load({path!r})
texts = [z[f't{{i}}'] for i in range(5)]
enc = [U.bwt(T) for T in texts]
sizes = [T.size for T in texts]
offs = np.concatenate([[0], np.cumsum(sizes)])
ctx = GpuContext(0, max_n=(1 << 20) + 4096)
dL = torch.from_numpy(np.concatenate([e[0] for e in enc])).cuda()
dT = torch.full((int(offs[-1]),), 0xAB, dtype=torch.uint8, device=dL.device)
_, res = ctx.unbwt_batch(dL, sizes, [e[1] for e in enc], dT=dT)
assert res == [0, -4, 0, -4, 0], res
Th = dT.cpu().numpy()
for b, T in enumerate(texts):
    got = Th[offs[b]:offs[b + 1]]
    assert np.array_equal(got, T) if res[b] == 0 else (got == 0xAB).all(), b
for kind in ('e1', 'lzp'):
    blocks = [z[f'{{kind}}_{{i}}'].tobytes() for i in range(5)]
    assert ctx.decompress_batch(blocks) == [T.tobytes() for T in texts], kind
    out, o, res = ctx.decompress_batch_device(blocks)
    assert res == [0] * 5, (kind, res)
    assert out.cpu().numpy().tobytes() == b''.join(T.tobytes() for T in texts), kind
ctx.close()
print('child ok')
"""
    _child(code, BSC_UNBWT_STEP_CAP="64")


def test_step_cap_values_below_16_are_ignored():
    code = PRELUDE + """
import torch
from libbsc_amd import GpuContext
from libbsc_amd.synth import synth_text_v1
ctx = GpuContext(0, max_n=(1 << 20) + 4096)
T = synth_text_v1(41, 300_000)
L, idx = U.bwt(T)
back, rc = ctx.unbwt(L, idx)
assert rc == 0 and np.array_equal(back, T), rc
ctx.close()
print('child ok')
"""
    _child(code, BSC_UNBWT_STEP_CAP="15")
