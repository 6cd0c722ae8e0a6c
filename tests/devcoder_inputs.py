"""Deterministic sorted blocks (the coder's input L) that drive the device coder's rare exits, shared by the CPU judge
(test_devcoder_paths.py, which asks tools/devcoder_paths_probe.cpp whether an input really takes the path it is tagged with) and the GPU
tests (test_gpu_devcoder_paths.py).  A block is built from its runs: the QLFC rank of a run is the number of distinct symbols between
it and the next run of its symbol, so a cyclic walk over r + 1 symbols has constant rank r, and a periodic word over a few symbols has
a periodic rank sequence.

Tags (what the probe must confirm: check_tag below):
  avg_off        no sub-block has more than 32 symbols: dc_avg_kernel is not launched
  avg_decides    launched, every flag decided, block stays on the device
  fail_avg       undecided avg_rank flags                                    -> declined, BSCGPU_DC_FAIL_AVG
  hist_ext       runs enter the extended run_hist look-back and close at widening step `step`, block stays on the device
  fail_hist      a run_hist bracket open after the last widening             -> declined, BSCGPU_DC_FAIL_HIST
  replay_kept    a chain of family `fam` whose bracket stays open over >= 3 chunks but never over enough for the replay limit:
                 at least one chunk is replayed, block stays on the device
  fail_replay    a chain whose bracket stays open over more than DC_REPLAY_MAX + 2 chunks -> declined, BSCGPU_DC_FAIL_REPLAY
"""
import numpy as np

def _symbols(k):
    """k distinct byte values spread over the byte range, 0 and 255 first (k >= 2)"""
    s = [0, 255] + [int(x) for x in (np.arange(1, 255) * 37) % 254 + 1]
    out = s[:k]
    assert len(set(out)) == k
    return np.array(out, dtype=np.uint8)


def runs_to_block(sym, length):
    return np.repeat(np.asarray(sym, dtype=np.uint8), np.asarray(length, dtype=np.int64))


def const_rank(r, runs=300_000):
    """cyclic walk over r + 1 symbols, every run of length 1 (run_hist contracts under runs of 1): rank r throughout, except the last
    occurrence of every symbol in a sub-block"""
    a = _symbols(r + 1)
    return a[np.arange(runs) % (r + 1)]


def avg_warm_edge(sb0_runs, sb1_runs, r=40):
    """Two sub-blocks of exactly sb0_runs and sb1_runs runs, constant rank r (32..62: a warmed-up bracket never decides).  An avg_rank
    lane starts exact only where its warm-up reaches the sub-block's first run, i.e. at most DC_AVG_WARM runs behind it: with
    sb0_runs = DC_AVG_CH - DC_AVG_WARM = 256 the lane of runs 1024.. is exact and 1792 runs of the second sub-block decide; one run
    less in front, or a few dozen more behind, and they do not.
    Layout: the split samples every 32nd position and halves the sampled run starts.  First sub-block: runs of 1024 bytes (every start
    sampled); second: sb0_runs + 1 groups of 32 bytes whose inner run starts (runs of 2 bytes) fall between the samples."""
    a = _symbols(r + 1)
    groups = sb0_runs + 1
    assert groups <= sb1_runs <= 15 * groups
    per = [sb1_runs // groups + (1 if g < sb1_runs % groups else 0) for g in range(groups)]
    len1 = []
    for k in per:
        len1 += [2] * (k - 1) + [32 - 2 * (k - 1)]
    length = [1025] + [1024] * (sb0_runs - 1) + len1
    sym = np.concatenate([a[np.arange(sb0_runs) % (r + 1)], a[np.arange(sb1_runs) % (r + 1)]])
    if sym[sb0_runs - 1] == sym[sb0_runs]:                      # the two sub-blocks must not merge their border runs
        sym[sb0_runs:] = a[(np.arange(sb1_runs) + 1) % (r + 1)]
    return runs_to_block(sym, length)


def hist_chain(q, sep=1):
    """One symbol with q runs of length 2 (two fixed points of run_hist, 1 and 2: its bracket never closes by itself), separated by runs
    of `sep` bytes of a second symbol (1 or >= 128: those contract): the run with P earlier runs enters the extended look-back for
    P >= 9 and closes only where the look-back reaches the chain's start (P < 36, 144, 576, 2304, 9216)."""
    sym = np.tile(_symbols(2), q)
    length = np.tile(np.array([sep, 2]), q)
    return runs_to_block(sym, length)


def hist_mixed(period, runs=60_000):
    """One symbol with runs of length 2 and, every `period`-th, one of length 20 (another class: both ends of the bracket land on 4),
    separated by single bytes: the look-back closes on the data, at the first widening that reaches back `period` runs."""
    sym = np.tile(_symbols(2), runs)
    la = np.full(runs, 2)
    la[period - 1::period] = 20
    length = np.stack([np.ones(runs, dtype=np.int64), la], axis=1).ravel()
    return runs_to_block(sym, length)


def periodic(word, lengths, runs):
    """runs runs: symbols word[j % len(word)] (indices into the symbol list), run lengths lengths[j % len(lengths)]"""
    a = _symbols(max(word) + 1)
    w = np.asarray(word)
    for i in range(len(w)):
        assert w[i] != w[(i + 1) % len(w)]
    j = np.arange(runs)
    return runs_to_block(a[w[j % len(w)]], np.asarray(lengths)[j % len(lengths)])


def pair_swap(k, runs, extra=0, every=0):
    """Cycles over k symbols (k even) that alternate between the order 0 1 2 3 .. and 1 0 3 2 ..: the ranks alternate k and k - 2.
    With every > 0, `extra` further symbols appear once each every `every` runs (a sub-block then has k + extra symbols, which sets
    how many exponent bits a rank has: max_rank)."""
    assert k % 2 == 0
    a = _symbols(k + extra)
    j = np.arange(runs)
    pos, cyc = j % k, (j // k) & 1
    idx = np.where(cyc == 1, pos ^ 1, pos)
    if every:
        grp = np.arange(k, k + extra)
        rows = idx[:runs // every * every].reshape(-1, every)
        idx = np.concatenate([rows, np.tile(grp, (rows.shape[0], 1))], axis=1).ravel()
    return a[idx]


# name -> (tag, extra, builder).  `extra`: step for hist_ext, fam for replay_kept, sub_runs where the layout is part of the case.
GENERATORS = {}


def _gen(name, tag, builder, **extra):
    assert name not in GENERATORS
    GENERATORS[name] = (tag, extra, builder)


# ---- avg_rank bracket: constant rank on both sides of each boundary
_gen("rank31", "avg_off", lambda: const_rank(31))
_gen("rank32", "fail_avg", lambda: const_rank(32))
_gen("rank62", "fail_avg", lambda: const_rank(62))
_gen("rank63", "avg_decides", lambda: const_rank(63))
_gen("rank40_one_lane", "avg_decides", lambda: const_rank(40, 1024))          # a single lane: exact from the sub-block's first run
_gen("rank40_warm_1792", "avg_decides", lambda: avg_warm_edge(256, 1792), sub_runs=[256, 1792])
_gen("rank40_warm_front_255", "fail_avg", lambda: avg_warm_edge(255, 1793), sub_runs=[255, 1793])
# (seven runs in the third lane: last occurrences, whose small ranks have pulled the upper end below 32 by then — decided after all)
_gen("rank40_warm_1799", "avg_decides", lambda: avg_warm_edge(256, 1799), sub_runs=[256, 1799])
_gen("rank40_warm_1856", "fail_avg", lambda: avg_warm_edge(256, 1856), sub_runs=[256, 1856])

# ---- run_hist bracket: P same-class predecessors on both sides of every widening
for _q, _step in ((9, None), (10, 0), (36, 0), (37, 1), (144, 1), (145, 2), (576, 2), (577, 3), (2304, 3), (2305, 4), (9216, 4)):
    if _step is None:
        _gen(f"hist_q{_q}", "avg_off", lambda q=_q: hist_chain(q))
    else:
        _gen(f"hist_q{_q}", "hist_ext", lambda q=_q: hist_chain(q), step=_step)
_gen("hist_q9217", "fail_hist", lambda: hist_chain(9217))
_gen("hist_q40000", "fail_hist", lambda: hist_chain(40000))
_gen("hist_two_sub_blocks_kept", "hist_ext", lambda: hist_chain(2 * 9216, sep=158), step=4)
_gen("hist_two_sub_blocks_fail", "fail_hist", lambda: hist_chain(2 * 9216 + 8, sep=158))
for _p, _step in ((12, 0), (50, 1), (200, 2), (1000, 3), (5000, 4)):
    _gen(f"hist_mixed_p{_p}", "hist_ext", lambda p=_p: hist_mixed(p), step=_step)

# ---- counter brackets: rank and run-length sequences with a short period.  A chain that sees a periodic bit sequence settles on two
# different orbits from the two ends of its range; the contexts (previous four runs, run_hist) are periodic too, so which families see
# the alternation depends on whether their contexts tell the phases apart.  `fam` / `cls`: where the probe must find a stretch of at
# least three chunks (dcm::CLS_*: 0 RF, 1 RE, 2 RM, 3 RP, 4 NF, 5 NE, 6 NM).
_W_RF_STATIC, _W_RF_STATE, _W_RM_STATIC = [0, 1, 0, 2], [0, 1, 0, 1, 2], [0, 1, 0, 2, 3]
_gen("alt_rf_static_5_chunks", "replay_kept", lambda: periodic(_W_RF_STATIC, [1], 5 * 8192 + 100), fam="static", cls=0)
_gen("alt_rf_static_2x61_chunks", "replay_kept", lambda: periodic(_W_RF_STATIC, [1], 1_000_000), fam="static", cls=0)
_gen("alt_rf_static_2x73_chunks", "fail_replay", lambda: periodic(_W_RF_STATIC, [1], 1_200_000), fam="static", cls=0)
_gen("alt_rf_state_char", "replay_kept", lambda: periodic(_W_RF_STATE, [1], 300_000), fam="state", cls=0)
_gen("alt_rf_state_2x73_chunks", "fail_replay", lambda: periodic(_W_RF_STATE, [1], 1_500_000), fam="state", cls=0)
_gen("alt_rm_static", "replay_kept", lambda: periodic(_W_RM_STATIC, [1], 300_000), fam="static", cls=2)
_gen("alt_nf_char", "replay_kept", lambda: periodic([0, 1, 2], [1, 2], 400_000), fam="char", cls=4)
_gen("alt_nm_static", "replay_kept", lambda: periodic([0, 1], [4, 6, 1, 1], 400_000), fam="static", cls=6)
_gen("alt_rm_state", "replay_kept", lambda: periodic([0, 1, 2, 0, 1, 3], [4, 6, 1, 1], 400_000), fam="state", cls=2)
_gen("alt_ne_state", "replay_kept", lambda: hist_mixed(12, 120_000), fam="state", cls=5)
_gen("alt_char_static_fail", "fail_replay", lambda: periodic(_W_RF_STATIC, [1, 1, 2], 2_200_000), fam="char", cls=4)
_gen("alt_rp_escape", "replay_kept", lambda: pair_swap(66, 400_000), fam="static", cls=3)
# (twelve symbols in every sub-block: the exponent of these ranks is closed by a zero, B < max_rank.  The exponent's own chains — class
# RE — meet within some 40 events under this alternation in all three families; it is the mantissa's that stay open)
_gen("alt_rm_static_max_rank_3", "replay_kept", lambda: pair_swap(4, 400_000, extra=8, every=20_000), fam="static", cls=2)


# ---- whole blocks: texts whose BWT takes the path --------------------------------------------------------------------------
# A sorted block is the BWT of a text only if its LF mapping is ONE cycle.  Swapping two adjacent, different symbols whose positions lie
# on two cycles joins the cycles (the mapping is composed with a transposition), so a few dozen swaps at run borders turn a generated
# block into a real BWT that keeps its run structure almost everywhere; walking the LF mapping backwards then gives the text.  Whether
# the text's BWT still takes the path is for the probe to say (test_devcoder_paths.py, on the reference's bwt_encode of the text).
def _cycle_labels(psi):
    lab = np.arange(psi.size, dtype=np.int64)
    jump = psi.copy()
    k = 1
    while k < psi.size:
        lab = np.minimum(lab, lab[jump])
        jump = jump[jump]
        k *= 2
    return lab


def text_with_bwt_like(L):
    """a text whose BWT is L up to a few swaps of neighbouring symbols"""
    L = np.array(L, dtype=np.uint8)
    psi = np.argsort(L, kind="stable").astype(np.int64)              # row of the sorted column -> position in L
    inv = np.empty_like(psi)
    inv[psi] = np.arange(psi.size)
    cyc = _cycle_labels(psi)[inv]                                    # cycle of every position of L
    parent = {}

    def find(x):
        while parent.get(x, x) != x:
            parent[x] = parent.get(parent[x], parent[x])
            x = parent[x]
        return x
    last = -5
    for i in np.nonzero((L[1:] != L[:-1]) & (cyc[1:] != cyc[:-1]))[0].tolist():
        if i <= last + 1:
            continue
        a, b = find(int(cyc[i])), find(int(cyc[i + 1]))
        if a != b:
            parent[a] = b
            L[i], L[i + 1] = L[i + 1], L[i]
            last = i
    psi = np.argsort(L, kind="stable").astype(np.int64)
    seq = np.zeros(1, dtype=np.int64)
    jump = psi.copy()
    while seq.size < L.size:
        seq = np.concatenate([seq, jump[seq]])
        jump = jump[jump]
    return L[psi][seq[:L.size]]


# name -> (tag, extra, builder of the block the text is made from).  bsc_compress tries the device model only on blocks of >= 1 MiB with
# at least two sub-blocks and at most 0.70 runs per byte, hence the run lengths 1 1 2 4 1 (their period 5 against the words' 4 gives every
# symbol every length: run_hist contracts).
WHOLE_BLOCKS = {
    "replay_kept": ("replay_kept", dict(fam="static", cls=0), lambda: periodic(_W_RF_STATIC, [1, 1, 2, 4, 1], 600_000)),
    "fail_replay": ("fail_replay", dict(fam="static", cls=0), lambda: periodic(_W_RF_STATIC, [1, 1, 2, 4, 1], 1_400_000)),
    "fail_avg": ("fail_avg", {}, lambda: runs_to_block(const_rank(40, 600_000), np.tile([1, 1, 2, 4], 150_000))),
    "fail_hist": ("fail_hist", {}, lambda: hist_chain(400_000)),
}


def build_probe(dirname):
    """compile tools/devcoder_paths_probe.cpp into dirname -> path of the program"""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(str(dirname), "devcoder_paths_probe")
    subprocess.run(["g++", "-O2", "-std=c++17", "-march=x86-64-v3", "-I", os.path.join(root, "libbsc_amd/csrc/host"), "-I", os.path.join(root, "libbsc_amd/csrc/device"),
                    "-I", os.path.join(root, "include"), os.path.join(root, "tools/devcoder_paths_probe.cpp"), os.path.join(root, "libbsc_amd/csrc/host/coder.cpp"),
                    "-o", exe, "-lpthread"], check=True)
    return exe


PROBE_OPTIONS = ("avg_exact", "hist_exact", "replay_exact")       # the probe's option words: BSCGPU_OPT_DC_{AVG,HIST,REPLAY}_EXACT on


def run_probe(exe, L, dirname, options=()):
    """the probe's verdict on the sorted block L (a dict: tools/devcoder_paths_probe.cpp); options: the words of PROBE_OPTIONS that are on"""
    import json
    import os
    import subprocess
    assert all(o in PROBE_OPTIONS for o in options), options
    path = os.path.join(str(dirname), "probe_input.bin")
    np.ascontiguousarray(L, dtype=np.uint8).tofile(path)
    r = subprocess.run([exe, path, *options], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return json.loads(r.stdout)


FAIL_AVG, FAIL_HIST, FAIL_CAP, FAIL_REPLAY = 2, 4, 8, 16           # include/bscgpu.h: BSCGPU_DC_FAIL_*
FAMILIES = ("state", "char", "static")


def check_tag(name, verdict, table=None):
    """assert that the probe's verdict confirms what generator `name` is tagged with"""
    tag, extra, _ = (GENERATORS if table is None else table)[name]
    v = verdict
    if "sub_runs" in extra:
        assert v["sub_runs"] == extra["sub_runs"], (name, v["sub_runs"])
    if tag == "avg_off":
        assert v["fail_mask"] == 0 and not v["avg_launched"], (name, v)
    elif tag == "avg_decides":
        assert v["fail_mask"] == 0 and v["avg_launched"] and v["avg_und"] == 0, (name, v)
    elif tag == "fail_avg":
        assert v["fail_mask"] == FAIL_AVG and v["avg_launched"] and v["avg_und"] > 0, (name, v)
    elif tag == "hist_ext":
        assert v["fail_mask"] == 0 and v["hist_fail"] == 0 and v["hist_ext"] > 0, (name, v)
        step = extra["step"]
        assert v["hist_closed"][step] > 0 and not any(v["hist_closed"][step + 1:]), (name, v)
    elif tag == "fail_hist":
        assert v["fail_mask"] == FAIL_HIST and v["hist_fail"] > 0, (name, v)
    elif tag == "replay_kept":
        assert v["fail_mask"] == 0 and v["replay_certain"] and v["no_fail_replay_certain"], (name, v)
        assert v["families"][extra["fam"]]["stretch_by_class"][extra["cls"]] >= v["replay_min"], (name, v)
    elif tag == "fail_replay":
        assert v["fail_mask"] == FAIL_REPLAY and v["avg_und"] == 0 and v["hist_fail"] == 0, (name, v)
        assert v["families"][extra["fam"]]["stretch_by_class"][extra["cls"]] > v["fail_min"], (name, v)
    else:
        raise AssertionError(f"unknown tag {tag}")
