"""Identical to the reference, or CCJ_E_RANGE, on the GPU (-m gpu).

tests/golden/range_cases.json holds folds whose penalties pen_in / pen_out differ by one unit: under
pen_in no 4-D value lies below -32768 before its store (the fold must succeed and equal the
restatement in all 31 hashes: values sit at -32768 .. -32757, the off-by-one guard), under pen_out one
does (the reference's int16 store wraps, the engine must refuse with RangeError).  The pair goes
through every kind of context; the refusal must not stick to a context; and the sites that raise it
must all be reached by some fold.
"""
import json
import os
import subprocess
import sys
import threading

import pytest

from tests.oracle_lib import ROOT, OracleFold, blob, golden

pytestmark = pytest.mark.gpu

DOC = golden("range_cases.json")
CASES = DOC["cases"]
BY_NAME = {c["name"]: c for c in CASES}
LONG = next(c for c in CASES if len(c["seq"]) > 40)
SHORT = [c for c in CASES if len(c["seq"]) <= 30]
D4_CASE = BY_NAME["n20_T04_d2_bp"]            # the wrapped store is PM (a d4 matrix)
TABCF_CASE = BY_NAME["n24_DP09_d1_appos_bp"]  # the wrapped stores are PR tables and a closed form
# the wrapped store PO(1,23,25,26) lies in a-block 22, which rank (22 // 4) % 2 = 1 of two owns
RANK1_CASE = BY_NAME["n26_DP09_d0_apneg_bp"]

_oracles = {}
_flags = {}  # (case name, split_target) -> range_flags() of its pen_out fold


def _oracle(seq, case, which):
    """One restatement fold per input, shared and never changed: (hashes, W(n), low_stores)."""
    key = (seq, case["name"], which)
    if key not in _oracles:
        o = OracleFold(seq, blob(case["params"]), case["dangles"], 0, threads=0 if len(seq) > 40 else None, pen=case[which])
        _oracles[key] = (o.hashes(), o.W(len(seq)), o.low_stores())
        o.close()
    return _oracles[key]


def _wf(case, which, seq=None, **kw):
    from ccj_amd import W_final
    kw.setdefault("split_target", case["split_target"])
    return W_final(seq or case["seq"], case["dangles"], params=case["params"], pen=case[which], **kw)


def _run(wf):
    """fill + result.  Under such penalties the reference's own backtrack often exits ("This should not
    have happened!"); the engine reproduces that, and it is a result like any other here.  A RangeError
    is not caught."""
    from ccj_amd import BacktrackExit
    try:
        e = wf.ccj()
        return ("ok", wf.structure, e, wf.stdout_msgs)
    except BacktrackExit as ex:
        return ("exit", ex.exit_code, ex.msg, ex.stdout)


def _record(seq, res):
    """fold_many's record of a _run outcome."""
    return (seq, res[1], res[2], res[3], 0, "") if res[0] == "ok" else (seq, None, None, res[3], res[1], res[2])


def _assert_identical(wf, case, which, seq=None):
    """The fold of wf was accepted: all 31 hashes and W(n) are the restatement's, no site flagged."""
    seq = seq or case["seq"]
    want, wn, low = _oracle(seq, case, which)
    assert low == 0
    got = wf.hashes()
    assert len(want) == 31 and got == want, [k for k in want if got[k] != want[k]]
    assert wf.W(len(seq)) == wn
    assert wf.range_flags() == 0


def _assert_refused(wf, fold=None):
    """fold() (default wf.ccj) raises RangeError; nothing is reported; the flags say where."""
    from ccj_amd import CCJ_E_RANGE, RangeError
    with pytest.raises(RangeError) as ei:
        (fold or wf.ccj)()
    e = ei.value
    assert e.code == CCJ_E_RANGE and "-32768" in e.msg
    assert e.flags == wf.range_flags() != 0
    assert wf.structure is None and wf.energy is None
    with pytest.raises(RangeError):  # and stays refused for this fold
        wf.result()
    return e.flags


def _inside_same_length(case):
    """Another sequence of the case's length that stays inside the domain under pen_out: a prefix that
    does (the fixture lists them), behind unpaired A; the restatement confirms it."""
    n, full = len(case["seq"]), case["seq"]
    cands = ["A" * (n - m) + full[:m] for m in case["inside_prefixes"]]
    cands += [full[:m] + "A" * (n - m) for m in range(n - 2, 7, -2)]  # shorter and shorter heads
    for seq in cands:
        if seq != full and _oracle(seq, case, "pen_out")[2] == 0:
            return seq
    # a closed form's restart branch 32767 + cp (l - k) depends on the length alone: under such
    # penalties even a sequence without a single pair is outside, and no reset can lead back inside
    assert _oracle("A" * n, case, "pen_out")[2] > 0, "fixture: no padded prefix stays inside the domain"
    return None


@pytest.mark.parametrize("case", CASES, ids=lambda c: c["name"])
def test_pen_in_folds_bit_identical(case):
    wf = _wf(case, "pen_in")
    try:
        _run(wf)
        _assert_identical(wf, case, "pen_in")
    finally:
        wf.close()


@pytest.mark.parametrize("case", CASES, ids=lambda c: c["name"])
def test_pen_out_is_refused_and_the_flag_does_not_stick(case):
    wf = _wf(case, "pen_out")
    try:
        _flags[(case["name"], case["split_target"])] = _assert_refused(wf)
        assert len(wf.hashes()) == 31  # the clamp-only matrices stay readable
        other = _inside_same_length(case)
        if other is None:  # every sequence of this length is outside: the iff on one without pairs
            wf.reset("A" * len(case["seq"]))
            _assert_refused(wf)
            return
        wf.reset(other)
        _run(wf)
        _assert_identical(wf, case, "pen_out", other)
        wf.reset(case["seq"])  # and refuses again
        _assert_refused(wf)
    finally:
        wf.close()


@pytest.mark.parametrize("case", [D4_CASE, TABCF_CASE], ids=lambda c: c["name"])
def test_pair_through_rebind_at_a_larger_capacity(case):
    n = len(case["seq"])
    prefix = case["seq"][:case["inside_prefixes"][0]]
    inn = _wf(case, "pen_in", capacity=n + 5)
    out = _wf(case, "pen_out", seq=prefix, capacity=n + 5)
    fresh = _wf(case, "pen_out", capacity=n + 5)
    try:
        _run(inn)
        _assert_identical(inn, case, "pen_in")
        _run(out)
        _assert_identical(out, case, "pen_out", prefix)
        out.rebind(case["seq"])
        flags = _assert_refused(out)
        out.rebind(prefix)
        _run(out)
        _assert_identical(out, case, "pen_out", prefix)
        assert _assert_refused(fresh) == flags
    finally:
        for wf in (inn, out, fresh):
            wf.close()


def _fresh(case, seq):
    """The outcome (_run) of seq under pen_out in a context of its own."""
    wf = _wf(case, "pen_out", seq=seq)
    try:
        return _run(wf)
    finally:
        wf.close()


@pytest.mark.parametrize("case", [D4_CASE, TABCF_CASE], ids=lambda c: c["name"])
def test_lockstep_member_outside_the_domain_leaves_its_neighbours_alone(case):
    from ccj_amd import LockstepBatch, RangeError
    n = len(case["seq"])
    a, b = case["seq"][:case["inside_prefixes"][0]], case["seq"][:case["inside_prefixes"][2]]
    batch = LockstepBatch(n, 3, case["dangles"], params=case["params"], pen=case["pen_out"])
    try:
        batch.bind([a, case["seq"], b])
        batch.fold()  # the batch itself is fine
        ma, mid, mb = batch.members
        assert isinstance(mid.refused, RangeError) and mid.refused.flags == mid.range_flags() != 0
        assert mid.structure is None and mid.energy is None and mid.exit is None
        for m, s in ((ma, a), (mb, b)):
            assert m.refused is None
            _assert_identical(m, case, "pen_out", s)
            got = ("ok", m.structure, m.energy, m.stdout_msgs) if m.exit is None else \
                ("exit", m.exit.exit_code, m.exit.msg, m.exit.stdout)
            assert got == _fresh(case, s)
        batch.bind([b, a])  # the refusal does not stick to the member
        batch.fold()
        assert [m.refused for m in batch.members] == [None, None]
        _assert_identical(batch.members[1], case, "pen_out", a)
    finally:
        batch.close()


@pytest.mark.parametrize("lockstep", [0, 3], ids=["contexts", "lockstep"])
def test_fold_many_records_a_refused_fold(lockstep):
    from ccj_amd import RANGE_EXIT_CODE, fold_many
    case = D4_CASE
    a, b = case["seq"][:case["inside_prefixes"][0]], case["seq"][:case["inside_prefixes"][1]]
    seqs = [a, case["seq"], b, case["seq"]]
    recs = fold_many(seqs, case["dangles"], params=case["params"], pen=case["pen_out"], contexts=2, lockstep=lockstep)
    assert [r[0] for r in recs] == seqs
    for r in (recs[1], recs[3]):
        assert r[1:4] == (None, None, "") and r[4] == RANGE_EXIT_CODE and "-32768" in r[5]
        assert RANGE_EXIT_CODE not in (0, 1, 134)  # the reference's own exit codes
    assert recs[0] == _record(a, _fresh(case, a)) and recs[2] == _record(b, _fresh(case, b))


def test_fold_cli_reports_the_refusal():
    from ccj_amd import RANGE_EXIT_CODE
    from ccj_amd.cli import fold_cli
    case = TABCF_CASE
    code, out, err = fold_cli(case["seq"], case["params"], case["dangles"], False, pen=case["pen_out"])
    assert code == RANGE_EXIT_CODE and out == "" and "-32768" in err
    code, out, err = fold_cli(case["seq"], case["params"], case["dangles"], False, pen=case["pen_in"])
    assert code != RANGE_EXIT_CODE and "-32768" not in err  # the reference's own outcome, result or exit


@pytest.mark.parametrize("kind", ["host_traceback", "d4_full", "shard_simulate2", "overlap_d2h"])
@pytest.mark.parametrize("case", [D4_CASE, TABCF_CASE], ids=lambda c: c["name"])
def test_pair_in_every_kind_of_context(case, kind, monkeypatch):
    if kind == "d4_full":
        monkeypatch.setenv("CCJ_D4_FULL", "1")  # read when the context is created
    kw = {"host_traceback": {"host_traceback": True}, "d4_full": {}, "overlap_d2h": {"overlap_d2h": True, "host_traceback": True},
          "shard_simulate2": {"shard_world": 2, "shard_simulate": True}}[kind]
    inn, out = _wf(case, "pen_in", **kw), _wf(case, "pen_out", **kw)
    try:
        _run(inn)
        _assert_identical(inn, case, "pen_in")
        assert _assert_refused(out) == _flags.get((case["name"], case["split_target"]), out.range_flags())
    finally:
        inn.close()
        out.close()


def _fold_pair(case, which):
    """Two ranks as their own contexts and threads over an in-process group; each rank's outcome."""
    from ccj_amd import BacktrackExit, LocalGroup, RangeError
    g = LocalGroup(2)
    ranks = [_wf(case, which, shard_world=2, shard_rank=r, local_group=g) for r in range(2)]
    res = [None, None]

    def run(r):
        try:
            ranks[r].fill()
            try:
                ranks[r].result()
            except BacktrackExit:
                pass
            res[r] = ("ok", ranks[r].range_flags())
        except RangeError as e:
            res[r] = ("range", e.flags, ranks[r].range_flags())
        except Exception as e:  # noqa: BLE001
            res[r] = ("error", repr(e))

    th = [threading.Thread(target=run, args=(r,), daemon=True) for r in range(2)]
    for x in th:
        x.start()
    for x in th:
        x.join(timeout=120)
    assert not [r for r, x in enumerate(th) if x.is_alive()], "a rank did not finish within 120 s (contexts left open)"
    return g, ranks, res


def test_both_ranks_of_an_in_process_group_refuse():
    """The wrapped store of this case belongs to rank 1 (a-block 22): rank 0 sees no site of its own and
    must still return the same code and flags."""
    case = RANK1_CASE
    (cell,) = [v[1] for v in case["wrapped"].values()]
    assert ((cell[1] - cell[0]) // 4) % 2 == 1
    g, ranks, res = _fold_pair(case, "pen_out")
    try:
        assert res[0][0] == res[1][0] == "range", res
        assert res[0] == res[1] and res[0][1] == res[0][2] != 0
    finally:
        for wf in ranks:
            wf.close()
        g.close()
    g, ranks, res = _fold_pair(case, "pen_in")
    try:
        assert res == [("ok", 0), ("ok", 0)], res
        for wf in ranks:
            _assert_identical(wf, case, "pen_in")
    finally:
        for wf in ranks:
            wf.close()
        g.close()


@pytest.mark.parametrize("target", ["all_regime", "default"])
def test_long_case_same_verdict_under_both_targets(target):
    tg = LONG["split_target"] if target == "all_regime" else 0
    inn, out = _wf(LONG, "pen_in", split_target=tg), _wf(LONG, "pen_out", split_target=tg)
    try:
        if tg:
            s = out.level_schedule(0)
            assert 0 < s.g_lo < s.g_hi  # leaders and ring partials are on the path
        _run(inn)
        _assert_identical(inn, LONG, "pen_in")
        _flags[(LONG["name"], tg)] = _assert_refused(out)
    finally:
        inn.close()
        out.close()


_CHILD = r"""
import ctypes, json, sys
sys.path.insert(0, sys.argv[1])
from ccj_amd import MAT4, BacktrackExit, W_final, lib
from tests.mloop2d_cases import valid_cells
from tests.oracle_lib import golden
SIX = ("PMmloop00", "PMmloop01", "PMmloop10", "POmloop00", "POmloop01", "POmloop10")
out = {}
for c in golden("range_cases.json")["cases"]:
    if c["name"] not in sys.argv[2:]:
        continue
    n = len(c["seq"])
    wf = W_final(c["seq"], c["dangles"], params=c["params"], pen=c["pen_out"], split_target=c["split_target"])
    try:
        outcome = ["ok", wf.ccj()]
    except BacktrackExit as ex:  # the reference's own exit: the fold was accepted
        outcome = ["exit", ex.exit_code]
    wbp = (ctypes.c_int * ((n + 1) * (n + 1)))()
    for i in range(1, n + 1):
        for j in range(i, n + 1):
            wbp[i * (n + 1) + j] = wf.get2("WBP", i, j)
    cells = list(valid_cells(n))
    L = lib()
    L.ccj_pmpo2d_closed.restype = ctypes.c_longlong
    L.ccj_pmpo2d_closed.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_int), ctypes.c_int, ctypes.c_int,
                                    ctypes.POINTER(ctypes.c_int16), ctypes.c_longlong]
    host = (ctypes.c_int16 * (6 * len(cells)))()
    assert L.ccj_pmpo2d_closed(n, wbp, c["pen_out"][10], c["pen_out"][11], host, len(cells)) == len(cells)
    diffs = sum(wf.get4(MAT4.index(nm), *cell) != host[m * len(cells) + k]
                for m, nm in enumerate(SIX) for k, cell in enumerate(cells))
    out[c["name"]] = {"flags": wf.range_flags(), "outcome": outcome, "cf_diffs": diffs,
                      "cf_cells": 6 * len(cells), "hashes": len(wf.hashes())}
    wf.close()
print("RESULT " + json.dumps(out))
"""


def test_allow_out_of_range_keeps_the_clamp_only_fold():
    """CCJ_ALLOW_OUT_OF_RANGE=1 (a child process): the pen_out fold completes as it did before the
    check existed, the flags still report, and the six closed-form matrices equal the clamp-only host
    code (ccj_pmpo2d_closed over the fold's own WBP), not the restatement, which wraps."""
    names = [D4_CASE["name"], TABCF_CASE["name"]]
    env = dict(os.environ, CCJ_ALLOW_OUT_OF_RANGE="1")
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT] + names, capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    got = json.loads(next(ln for ln in r.stdout.splitlines() if ln.startswith("RESULT "))[7:])
    for nm in names:
        case, g = BY_NAME[nm], got[nm]
        assert g["outcome"][0] in ("ok", "exit") and g["hashes"] == 31
        assert g["cf_diffs"] == 0 and g["cf_cells"] > 0
        wf = _wf(case, "pen_out")
        try:
            assert g["flags"] == _assert_refused(wf) != 0  # the same flags with and without the switch
        finally:
            wf.close()


def test_every_site_is_reached():
    """Over all pen_out folds of this file: LEVEL, TAB and CF occur, and PARTIAL on a fold that shares
    split points (run alone, the folds are made here).  ILOOP is not asserted: no fixture case reaches it.
    Under the reference's e_intP = 0.74 the interior-loop energies of these parameter sets are positive,
    so an interior-loop minimum lies above the stored inner value it was formed from; with e_intP = -0.74
    (n29_T04_d0_eintneg_bp) the first wrap is in PO, which has no interior-loop minimum.  On every
    pen_in fold the site stays silent (values down to -32768), which is the half a false alarm would break."""
    from ccj_amd import RANGE_CF, RANGE_LEVEL, RANGE_PARTIAL, RANGE_TAB
    for case in CASES:
        if (case["name"], case["split_target"]) not in _flags:
            wf = _wf(case, "pen_out")
            try:
                _flags[(case["name"], case["split_target"])] = _assert_refused(wf)
            finally:
                wf.close()
    print({k: v for k, v in _flags.items()})
    seen = 0
    for v in _flags.values():
        seen |= v
    for bit, nm in ((RANGE_LEVEL, "LEVEL"), (RANGE_TAB, "TAB"), (RANGE_CF, "CF")):
        assert seen & bit, (nm, _flags)
    shared = [v for (nm, tg), v in _flags.items() if tg > 0]
    assert any(v & RANGE_PARTIAL for v in shared), _flags
    # a fold whose wrapped stores are all closed-form ones raises CF alone
    for nm in DOC["closed_form_first_search"]["found"]:
        assert _flags[(nm, BY_NAME[nm]["split_target"])] == RANGE_CF, (nm, _flags)
