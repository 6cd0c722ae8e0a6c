"""Records tests/golden/bwt_round_trace.json: the BWT driver's `[bwt]` debug lines (without their milliseconds) over the inputs of
bwt_inputs.TRACE_RUNS, every block checked against libsais on the way.

    python tests/make_bwt_round_trace.py            (on the GPU, with the library of the commit the trace is to be taken FROM)

The stored trace is what a change of the driver must leave as it is (test_gpu_bwt_round_trace.py), so it is recorded with the parent of
such a change, never with the changed code.  The list must reach every kind of round: a missing outcome fails the recording."""
import json
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bwt_inputs as bi

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bwt_round_trace.json")


def missing_outcomes(trace):
    lines = [l for run in trace["runs"].values() for ls in run.values() for l in ls]
    return [what for what, pat in bi.TRACE_OUTCOMES.items() if not any(re.search(pat, l) for l in lines)]


if __name__ == "__main__":
    trace = {"sizes": bi.TRACE_SIZES, "runs": bi.collect_all()}
    for run, t in trace["runs"].items():
        for name, lines in t.items():
            print(f"-- {run} / {name}")
            for l in lines:
                print("  ", l)
    miss = missing_outcomes(trace)
    out = sys.argv[1] if len(sys.argv) > 1 else GOLDEN
    with open(out, "w") as fh:
        json.dump(trace, fh, indent=1)
        fh.write("\n")
    print("wrote", out)
    if miss:
        sys.exit("the list does not reach: " + "; ".join(miss))
