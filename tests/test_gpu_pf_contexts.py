"""Partition function: one context folds many sequences (ccj_pf_create_cap / ccj_pf_rebind /
ccj_pf_reset, pf_many), with the per-sequence tables built on the GPU from the key tables.

Everything is held against tests/golden/pf_golden.json (the reference's own part_func.cc): a fold
through a reused context must give what a fresh context gives, bit for bit.  The goldens' 64 cases
fall in 6 groups of (parameters, dangles), since a context holds one such pair.
"""
import json
import os
import random
import struct
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(os.path.dirname(__file__), "golden", "pf_golden.json")

with open(GOLD) as _f:
    CASES = json.load(_f)["cases"]
BY_NAME = {c["name"]: c for c in CASES}
GROUPS = sorted({(c["params"], c["dangles"]) for c in CASES})


def _group(g):
    return [c for c in CASES if (c["params"], c["dangles"]) == g]


def _wbits(ws):
    return ["%016x" % struct.unpack("<Q", struct.pack("<d", w))[0] for w in ws]


def _fold_and_check(pf, case):
    """What test_gpu_pf.py::test_pf_matches_reference checks of a fresh context."""
    import ccj_amd
    e = pf.ccj_pf()
    assert repr(e) == repr(float(case["energy"])) or (e != e and case["energy"] == "nan"), case["name"]
    assert _wbits(pf.W()) == case["wbits"], case["name"]
    h = pf.hashes()
    bad = {k: (h[k], v) for k, v in {**case["h2"], **case["h4"]}.items() if h[k] != v}
    assert not bad, (case["name"], bad)
    assert pf.exp_hashes() == case["exp"]
    if "srand" in case:
        pf.srand(case["srand"])
        try:
            got = pf.sample(5)
            assert "sample_exit" not in case
            assert got == case["samples"]
        except ccj_amd.SampleExit as ex:
            assert ex.structures == case["samples"]
            assert ex.stdout == case["sample_exit"]


def _long_short(cases):
    """longest, shortest, 2nd longest, 2nd shortest, ...: every bind changes the length a lot, and
    the cases without levels (n = 1, 2, 3) sit between long ones."""
    s = sorted(cases, key=lambda c: len(c["seq"]))
    out = []
    while s:
        out.append(s.pop())
        if s:
            out.append(s.pop(0))
    return out


# ---- 1. capacity context ------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("g", GROUPS, ids=["%s-d%d" % g for g in GROUPS])
def test_capacity_context_folds_the_group(g):
    import ccj_amd
    order = _long_short(_group(g))
    pf = ccj_amd.W_final_pf(order[0]["seq"], dangle=g[1], params=g[0], capacity=100)
    try:
        assert pf.capacity == 100
        for k, c in enumerate(order):
            if k:
                pf.rebind(c["seq"])
            assert pf.n == len(c["seq"]) == ccj_amd.lib().ccj_pf_n(pf._h)
            _fold_and_check(pf, c)
        assert pf.capacity == 100
    finally:
        pf.close()


# ---- 2. reset at the same length ----------------------------------------------------------------
def _fresh(seq, g):
    import ccj_amd
    pf = ccj_amd.W_final_pf(seq, dangle=g[1], params=g[0])
    try:
        e = pf.ccj_pf()
        return repr(e), _wbits(pf.W()), pf.hashes()
    finally:
        pf.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n", [12, 16, 20, 25, 30, 32])
def test_reset_at_the_same_length(n):
    """Per group, one plain ccj_pf_create context of length n (first bound to a sequence that is
    not a golden: a golden reversed), then every golden case of that length through reset."""
    import ccj_amd
    folded = 0
    for g in GROUPS:
        cs = [c for c in _group(g) if len(c["seq"]) == n]
        if not cs:
            continue
        pf = ccj_amd.W_final_pf(cs[-1]["seq"][::-1], dangle=g[1], params=g[0])
        try:
            assert pf.capacity == n
            pf.ccj_pf()
            for c in cs:
                pf.reset(c["seq"])
                _fold_and_check(pf, c)
                folded += 1
            with pytest.raises(ccj_amd.CCJError):
                pf.reset(cs[0]["seq"] + "A")
        finally:
            pf.close()
    assert folded == sum(1 for c in CASES if len(c["seq"]) == n) >= 6


@pytest.mark.gpu
def test_reset_dense_then_sparse_then_golden():
    """The copies of PL / PR / PM (d_cx, d_pmx) are written only where the pair can pair and read as
    0 elsewhere.  A densely pairing sequence leaves values in them; in poly-A no pair can pair, and
    in the golden after it other pairs can: without zeroing the copies again, the later sequences
    are folded over the earlier one's values.  (With the bundled parameter sets those values meet
    a weight of 0 — see the next test, which is the one that fails without the zeroing.)"""
    import ccj_amd
    g = ("default", 2)
    gold = next(c for c in _group(g) if len(c["seq"]) == 30)
    dense, sparse = "CG" * 15, "A" * 30
    assert sum(1 for i in range(30) for j in range(i + 1, 30) if {dense[i], dense[j]} == {"C", "G"}) > 200
    want_dense, want_sparse = _fresh(dense, g), _fresh(sparse, g)
    assert want_dense[2]["PL"] != want_sparse[2]["PL"]
    pf = ccj_amd.W_final_pf(gold["seq"], dangle=g[1], params=g[0])
    try:
        _fold_and_check(pf, gold)
        for seq, want in ((dense, want_dense), (sparse, want_sparse)):
            pf.reset(seq)
            e = pf.ccj_pf()
            assert (repr(e), _wbits(pf.W())) == want[:2], seq
            h = pf.hashes()
            assert not {k: (h[k], v) for k, v in want[2].items() if h[k] != v}, seq
        pf.reset(gold["seq"])
        _fold_and_check(pf, gold)
    finally:
        pf.close()


@pytest.mark.gpu
def test_reset_zeroes_the_copies_where_the_weights_do_not_mask_them():
    """With the bundled parameter sets a stale value in the copies is harmless: the only unmasked
    reads of a copy (the stack terms of k_pf_iloop) multiply it by get_e_stP of a pair type 0, and
    expstack[0][*] = expstack[*][0] = exp(-INF) = 0 there.  A parameter blob may have finite
    entries in that row and column (here 0, a weight of 1); then the copy itself must be 0 where
    the inner pair cannot pair.  Dense sequence, then a golden sequence on the same context,
    against a fresh context each."""
    import ccj_amd
    blob = bytearray(ccj_amd.load_params("default"))
    stack = list(struct.unpack_from("<64i", blob, 16))  # ccj_energy_params.stack[8][8]
    assert stack[0] == stack[9 * 0 + 3] == stack[8 * 3] == 10000000
    for x in range(8):
        stack[x] = stack[8 * x] = 0
    struct.pack_into("<64i", blob, 16, *stack)
    blob = bytes(blob)
    gold = next(c for c in _group(("default", 2)) if len(c["seq"]) == 30)
    dense = "CG" * 15

    def fresh(seq):
        pf = ccj_amd.W_final_pf(seq, dangle=2, params=blob)
        try:
            return repr(pf.ccj_pf()), _wbits(pf.W()), pf.hashes()
        finally:
            pf.close()

    want = {s: fresh(s) for s in (dense, gold["seq"])}
    pf = ccj_amd.W_final_pf(gold["seq"][::-1], dangle=2, params=blob)
    try:
        for s in (dense, gold["seq"], dense):
            pf.reset(s)
            got = repr(pf.ccj_pf()), _wbits(pf.W()), pf.hashes()
            assert got == want[s], s
    finally:
        pf.close()


# ---- 3. setup tables against the host builder ---------------------------------------------------
def _host_built(seq, g, monkeypatch, **kw):
    import ccj_amd
    monkeypatch.setenv("CCJ_PF_HOST_SETUP", "1")
    try:
        pf = ccj_amd.W_final_pf(seq, dangle=g[1], params=g[0], **kw)
        try:
            return pf.setup_hashes()
        finally:
            pf.close()
    finally:
        monkeypatch.delenv("CCJ_PF_HOST_SETUP")


@pytest.mark.gpu
def test_setup_tables_equal_the_host_builder(monkeypatch):
    """pt, est, hp, the items with their per-level firsts, and the ieO / ieI / mO / mI rows of the
    pairing intervals: a capacity-60 context rebound to a sequence holds what the host builder
    (CCJ_PF_HOST_SETUP=1: one pow per entry) uploads for it."""
    import ccj_amd
    g = ("default", 2)
    by_n = {len(c["seq"]): c for c in _group(g)}
    seqs = [by_n[n]["seq"] for n in (60, 3, 44, 8, 30, 23)]
    seqs.append(by_n[40]["seq"].replace("U", "T"))
    want = [_host_built(s, g, monkeypatch) for s in seqs]
    assert len({w["ieO"] for w in want}) >= 6 and sorted(want[0]) == sorted(ccj_amd.PF_SETUP_TABLES)
    pf = ccj_amd.W_final_pf(by_n[50]["seq"], dangle=g[1], params=g[0], capacity=60)
    try:
        for s, w in zip(seqs, want):
            pf.rebind(s)
            assert pf.setup_hashes() == w, len(s)
    finally:
        pf.close()
    # noGU: other pairs, other items and masks
    s = by_n[60]["seq"]
    w = _host_built(s, g, monkeypatch, noGU=True)
    assert w["items"] != want[0]["items"]
    pf = ccj_amd.W_final_pf(by_n[50]["seq"], dangle=g[1], params=g[0], capacity=60, noGU=True)
    try:
        pf.rebind(s)
        assert pf.setup_hashes() == w
    finally:
        pf.close()


# ---- 4. refusals --------------------------------------------------------------------------------
@pytest.mark.gpu
def test_refusals_leave_the_context_usable(monkeypatch):
    import ccj_amd
    from ccj_amd import CCJ_E_ARG, CCJ_E_STATE, CCJError
    c40, c60, c30 = BY_NAME["big40_default"], BY_NAME["big60_default"], next(
        c for c in _group(("default", 2)) if len(c["seq"]) == 30)
    pf = ccj_amd.W_final_pf(c40["seq"], dangle=2, params="default", capacity=60)
    try:
        for bad in ("A" * 61, c40["seq"][:20] + "X" + c40["seq"][21:], ""):
            with pytest.raises(CCJError) as e:
                pf.rebind(bad)
            assert e.value.code == CCJ_E_ARG
        assert pf.n == 40 and pf.seq == c40["seq"]
        _fold_and_check(pf, c40)      # the previous binding still folds to its golden
        pf.reset(c40["seq"])
        for call in (pf.W, pf.hashes, lambda: pf.sample(1), lambda: pf.get2("V")):
            with pytest.raises(CCJError) as e:
                call()
            assert e.value.code == CCJ_E_STATE
        _fold_and_check(pf, c40)
        # a fold that ends in CCJ_E_PF_RANGE (the bound lowered as in test_pf_range_exit) ...
        pf.rebind(c60["seq"])
        monkeypatch.setenv("CCJ_PF_RANGE_LOG2", "10")
        with pytest.raises(CCJError) as e:
            pf.ccj_pf()
        assert e.value.code == 10
        with pytest.raises(CCJError) as e:
            pf.W()
        assert e.value.code == CCJ_E_STATE
        monkeypatch.delenv("CCJ_PF_RANGE_LOG2")
        # ... leaves the context able to fold the next sequence
        pf.rebind(c30["seq"])
        _fold_and_check(pf, c30)
        pf.rebind(c60["seq"])
        _fold_and_check(pf, c60)
    finally:
        pf.close()
    with pytest.raises(CCJError):
        ccj_amd.W_final_pf("A" * 20, capacity=10)


# ---- 5. pf_many ---------------------------------------------------------------------------------
def _shuffled27():
    cs = _group(("default", 2))
    assert len(cs) == 27
    random.Random(2027).shuffle(cs)
    return cs


@pytest.mark.gpu
def test_pf_many_records_in_input_order():
    import ccj_amd
    cs = _shuffled27()
    recs = ccj_amd.pf_many([c["seq"] for c in cs], 2, "default")
    assert len(recs) == 27
    for c, (seq, e, wn) in zip(cs, recs):
        assert seq == c["seq"]
        assert repr(e) == repr(float(c["energy"])), c["name"]
        assert _wbits([wn])[0] == c["wbits"][-1], c["name"]
    assert ccj_amd.pf_many([]) == []


_CHILD = r"""
import json, struct, sys
sys.path.insert(0, sys.argv[1])
import ccj_amd
recs = ccj_amd.pf_many(json.loads(sys.argv[2]), 2, "default")
out = []
for seq, e, w in recs:
    if e is None:
        out.append([seq, None, w.code])
    else:
        out.append([seq, repr(e), "%016x" % struct.unpack("<Q", struct.pack("<d", w))[0]])
print("RESULT " + json.dumps(out))
"""


@pytest.mark.gpu
def test_pf_many_failing_member_does_not_disturb_the_rest():
    """With the exactness bound lowered to 2^10 (CCJ_PF_RANGE_LOG2, a child process) big60_default
    ends in CCJ_E_PF_RANGE, as in test_pf_range_exit, and the cases without levels (n <= 3: every
    P is 0) cannot.  Every member that folds, before and after a failing one, gives its golden."""
    cs = [c for c in _shuffled27() if c["name"] != "big60_default"]
    tail = [c for c in cs if len(c["seq"]) <= 3]
    cs = [c for c in cs if len(c["seq"]) > 3]
    cs = cs[:5] + [BY_NAME["big60_default"]] + cs[5:] + tail
    env = dict(os.environ, CCJ_PF_RANGE_LOG2="10")
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT, json.dumps([c["seq"] for c in cs])], capture_output=True,
                       text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    got = json.loads(next(ln for ln in r.stdout.splitlines() if ln.startswith("RESULT "))[7:])
    assert [x[0] for x in got] == [c["seq"] for c in cs]
    ok = 0
    for c, (_, e, w) in zip(cs, got):
        if e is None:
            assert w == 10, c["name"]  # CCJ_E_PF_RANGE
            assert len(c["seq"]) > 3
        else:
            assert e == repr(float(c["energy"])) and w == c["wbits"][-1], c["name"]
            ok += 1
    assert got[5][1] is None and ok >= len(tail) == 3
