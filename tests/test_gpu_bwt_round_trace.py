"""The BWT driver's round trace does not move: which kind of round every unsorted set gets, in which order, with how many records and
digit passes.  The `[bwt]` debug lines of a fixed list of seeded inputs (bwt_inputs.TRACE_RUNS: text, planted phrases, source-like and
object-like blocks, a periodic string, one batched pass, and the source-like block again without hybrid rounds), milliseconds
stripped, against tests/golden/bwt_round_trace.json — recorded by make_bwt_round_trace.py at the parent of the driver's refactor.
Every block must also equal libsais's BWT (the child process asserts it)."""
import json

import pytest

import bwt_inputs as bi
from make_bwt_round_trace import GOLDEN, missing_outcomes

pytestmark = pytest.mark.gpu


def test_round_trace_equals_the_recorded_one(ref):
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but torch.cuda.is_available() is False")
    with open(GOLDEN) as fh:
        want = json.load(fh)
    assert want["sizes"] == bi.TRACE_SIZES, "the trace was recorded over other inputs"
    assert not missing_outcomes(want), missing_outcomes(want)          # the list reaches every kind of round and both endings of a split
    assert list(want["runs"]) == [run for run, _, _ in bi.TRACE_RUNS]
    for run, names, env in bi.TRACE_RUNS:
        got = bi.collect_trace(names, env)                             # (one child per run; it checks every block against libsais)
        for name in names:
            print(f"-- {run} / {name}: {len(got[name])} lines")
            assert got[name] == want["runs"][run][name], (run, name, got[name], want["runs"][run][name])
        assert all(lines and lines[0].startswith("[bwt] n=") for lines in got.values())
