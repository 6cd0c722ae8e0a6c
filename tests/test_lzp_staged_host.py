"""CPU tests of the LZP stage's algorithm through its stand-in, bscgpu_lzp_staged_host: links as if every position were
visited, a byte of flags per position, and a sweep over windows that asks a real table only for positions whose predecessor a match
skipped.  It must give what the host encoder gives, byte for byte and code for code, and every path of it is pinned by its counter on a
named input (tests/lzp_device_inputs.py).  The device stage is held to the same answers and the same counters in test_gpu_lzp_device.py."""
import numpy as np
import pytest

import lzp_device_inputs as I
from libbsc_amd import api, gpu


def _same(key, T, h, m, f):
    got, cnt = gpu.lzp_staged_host(T, h, m, features=f)
    assert got == I.want(key, T, h, m, f), (key, h, m, f)
    return got, cnt


@pytest.mark.parametrize("features", I.FEATURES)
@pytest.mark.parametrize("name", list(I.corpora()))
def test_staged_equals_host_encoder(name, features):
    T = I.corpora()[name]
    for h in I.HASHES:
        for m in I.MINLENS:
            got, _ = _same(name, T, h, m, features)
            if not isinstance(got, int):
                assert api.bsc_lzp_decompress(got, T.size, h, m) == T.tobytes(), (name, h, m)


def test_staged_tiny_sizes():
    """n - minLen < 32 is refused; sizes around the main-phase guard, where the whole chunk is the last stretch and the tail"""
    for it, (T, h, m, f) in enumerate(I.tiny_cases()):
        got, _ = gpu.lzp_staged_host(T, h, m, features=f)
        assert got == api.bsc_lzp_compress(T, h, m, features=f), (it, T.size, h, m, f)


@pytest.mark.parametrize("features", I.FEATURES)
def test_staged_chunk_thresholds(features):
    """1 -> 2 -> 4 chunks; under the serial framing the last chunk's budget is what the chunks before it left"""
    big = I.threshold_block()
    for n in I.THRESHOLD_SIZES:
        got, cnt = _same(("threshold", n), big[:n], 15, 32, features)
        assert not isinstance(got, int) and got[0] == (1 if n < 256 * 1024 else 2 if n < (4 << 20) else 4) and cnt["matches"] > 0


@pytest.mark.parametrize("features", I.FEATURES)
def test_staged_first_chunk_kept_raw(features):
    T = I.first_chunk_raw()
    got, cnt = _same("first_chunk_raw", T, 15, 32, features)
    assert got[0] == 2 and got[1:5] == got[5:9] and got[9:13] != got[13:17] and cnt["raw_chunks"] == 1


@pytest.mark.parametrize("name", list(I.PATHS))
def test_every_path_is_taken(name):
    make, h, m, f, counter = I.PATHS[name]
    T = make()
    got, cnt = _same(("path", name), T, h, m, f)
    if counter is None:
        assert got == api.NOT_COMPRESSIBLE
    else:
        assert not isinstance(got, int) and cnt[counter] > 0, (name, cnt)


def test_staged_eight_chunks_golden():
    """a committed 17 MiB vector of the reference (tests/golden/lzp_golden.json): eight chunks, both framings"""
    import hashlib
    import json
    import os
    from libbsc_amd.synth import synth_repeat_v1
    gold = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "lzp_golden.json")))
    rows = [e for e in gold["stage"] if e["n"] > (6 << 20) and e["hash"] == 15 and e["minlen"] == 32]
    assert len(rows) == 2
    T = synth_repeat_v1(rows[0]["seed"], rows[0]["n"], rows[0]["period"])
    for e in rows:
        got, cnt = gpu.lzp_staged_host(T, 15, 32, features=e["features"])
        assert len(got) == e["size"] and hashlib.md5(got).hexdigest() == e["md5"] and got[0] == 8 and cnt["matches"] > 0, e


def test_frame_from_chunks_own_results_equals_the_container_rules(tmp_path):
    """frame_from_own (lzp_staged.h) says what a chunk coded under a budget of its own size would have returned under the serial rule's
    smaller budget.  tools/lzp_frame_probe.cpp draws own[] around every boundary of that rule and holds totals, tables, offsets and raw
    counts to container.h's frame_serial / frame_parallel, a stand-alone program under AddressSanitizer + UBSan (nothing is preloaded);
    the case no corpus reaches — a chunk that was coded and is kept raw because the room left is smaller — must occur."""
    import json
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "lzp_frame_probe")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(root, "libbsc_amd", "csrc", "host"), os.path.join(root, "tools", "lzp_frame_probe.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    j = json.loads(r.stdout.splitlines()[-1])
    assert j["mismatch"] == 0 and j["cases"] > 50_000 and j["coded_chunks_flipped_to_raw"] > 1000 and j["raw_by_own"] > 1000 \
        and j["not_compressible"] > 1000, j


def test_staged_declines_wide_tables_and_bad_parameters():
    T = np.zeros(1000, np.uint8)
    for h in (16, 17, 18):
        assert gpu.lzp_staged_host(T, h, 32)[0] == gpu.NOT_SUPPORTED
    assert gpu.lzp_staged_host(T, 9, 32)[0] == api.BAD_PARAMETER
    assert gpu.lzp_staged_host(T, 29, 32)[0] == api.BAD_PARAMETER
    assert gpu.lzp_staged_host(T, 15, 3)[0] == api.BAD_PARAMETER
    assert gpu.lzp_staged_host(T, 15, 256)[0] == api.BAD_PARAMETER
    assert gpu.lzp_staged_host(np.zeros(40, np.uint8), 15, 32)[0] == api.NOT_COMPRESSIBLE
