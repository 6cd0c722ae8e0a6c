"""The two forms of the QLFC front end (qlfc_front.hip) on the same L: a block with its cuts by value (bscgpu_qlfc_pstream_facts:
qlfc_front_split + qlfc_front_runs) and a pass of that one block with its table in HBM (bscgpu_qlfc_front_batch_device) must give the
same sub-blocks with the same number of runs each, and the pass's layout must be the CPU stand-in's (bscgpu_front_batch_host).  Sizes
around a tile of 4096 bytes, a chunk, the step from one sub-block to two and the largest block of a pass; alphabets on both sides of
the rank kernel's 32- and 64-symbol layouts; the block whose cuts lie 32 bytes apart."""
import numpy as np
import pytest

from front_inputs import layouts_equal, runs_block

pytestmark = pytest.mark.gpu

MIB = 1 << 20
SIZES = (4095, 4096, 4097, 65537, 262143, 262144, 262177, 1048575)
ALPHABETS = (2, 33, 65)


@pytest.fixture(scope="module")
def fctx():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from libbsc_amd import GpuContext
    c = GpuContext(0, max_n=MIB)
    yield c
    c.close()


def _noisy_stretch(n=262144):
    """constant except for one 300-byte noisy stretch: the adaptive split cuts where the sampled run starts are, 32 bytes apart"""
    rng = np.random.default_rng(262144)
    a = np.full(n, 7, np.uint8)
    a[n // 3:n // 3 + 300] = rng.integers(0, 256, 300, dtype=np.uint8)
    return a


def _check_forms(ctx, L):
    import torch
    from libbsc_amd.gpu import front_batch_host
    st, sz, runs, _, _ = ctx.qlfc_pstream_facts(L, 1)
    got = ctx.qlfc_front_batch(torch.from_numpy(L).cuda(), [L.size])
    assert got.nsub == len(st), f"{got.nsub} sub-blocks in the pass form, {len(st)} in the single-block form"
    assert list(got.sub_start) == st and list(got.sub_size) == sz
    assert [int(x) for x in np.diff(got.sub_run.astype(np.int64))] == runs
    bad = layouts_equal(got, front_batch_host(L, [L.size]))
    assert not bad, "; ".join(bad)
    return got


@pytest.mark.parametrize("K", ALPHABETS)
@pytest.mark.parametrize("n", SIZES)
def test_forms_agree(fctx, n, K):
    L = runs_block(np.random.default_rng(1000 * K + n % 997), n, K, mean_run=3.0, skew=0.3)
    got = _check_forms(fctx, L)
    assert got.nsub == (1 if n < 262144 else 2)
    assert int(np.unique(got.sym).size) == K, "the union alphabet must reach the layout the case is named for"


def test_forms_agree_on_noisy_stretch(fctx):
    got = _check_forms(fctx, _noisy_stretch())
    assert got.nsub == 2 and 0 < int(got.sub_size[0]) - 262144 // 3 < 300, "the cut lies inside the noisy stretch"
