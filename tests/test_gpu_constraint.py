"""Constrained folding on the GPU (-m gpu): forbidden pairs and unpaired positions
(include/ccj.h ccj_constraint).

The fixtures (tests/golden/constraint_cases.json) carry the 31 hashes and W(n) of the masked
restatement (tests/masked_oracle.py; held against the reference on the CPU by
tests/test_constraint_oracle.py).  Every kind of context must reproduce them, the traceback must
respect the constraint on both executors, and no context may carry a constraint past its binding.
"""
import ctypes
import json
import os
import subprocess
import sys

import pytest

import ccj_amd
from ccj_amd import Constraint, LockstepBatch, W_final, fold_many
from tests.constraint_cases import case_id, cases, constraint_of, gu_pairs, pairs_of, pseudoknotted_e2e
from tests.oracle_lib import ROOT, OracleFold, blob, golden

pytestmark = pytest.mark.gpu

CASES = cases()
_plain = {}


def _wf(c, constrained=True, **kw):
    return W_final(c["seq"], c["dangles"], params=c["params"], noGU=bool(c["noGU"]),
                   constraint=constraint_of(c) if constrained else None, **kw)


def _outcome(wf):
    """("ok", structure, energy) or ("exit", code, stderr) of a filled context."""
    try:
        e = wf.result()
        return ("ok", wf.structure, e)
    except ccj_amd.BacktrackExit as ex:
        return ("exit", ex.exit_code, ex.msg)


def _check(wf, c, what=""):
    """The filled context against the fixture: hashes, W(n), energy, and the constraint in the structure."""
    n = len(c["seq"])
    out = _outcome(wf)
    got = wf.hashes()
    bad = [k for k in c["hashes"] if got[k] != c["hashes"][k]]
    assert not bad, (what, case_id(c), bad)
    assert wf.W(n) == c["Wn"], (what, case_id(c))
    # every fixture has a finite W(n) and no fixture's traceback ends in a reference exit
    assert out[0] == "ok", (what, case_id(c), out)
    assert out[2] == c["Wn"] / 100.0
    F = constraint_of(c).forbidden(n)
    prs = pairs_of(out[1])
    assert not prs & F, (what, case_id(c), out[1], sorted(prs & F))
    if c["unpaired"]:
        assert all(out[1][p] == "." for p, ch in enumerate(c["unpaired"]) if ch == "x"), (out[1], c["unpaired"])
    return out


def _plain_hashes(c):
    """The unconstrained fold's hashes (the restatement; equal to the reference's, tests/test_oracle.py)."""
    key = (c["seq"], c["params"], c["dangles"], c["noGU"])
    if key not in _plain:
        o = OracleFold(c["seq"], blob(c["params"]), c["dangles"], c["noGU"])
        _plain[key] = o.hashes()
        o.close()
    return _plain[key]


@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_fixture_on_both_traceback_executors(c):
    wf = _wf(c)
    hw = _wf(c, host_traceback=True)
    try:
        wf.fill()
        dev = _check(wf, c, "device traceback")
        F = constraint_of(c).forbidden(len(c["seq"]))
        assert 0 < wf.constraint_count() <= len(F)  # every fixture forbids pairs of an MFE structure
        hw.fill()
        host = _check(hw, c, "host traceback")
        assert dev == host
        if c["kind"] == "x_everywhere":
            assert dev == ("ok", "." * len(c["seq"]), 0.0)
    finally:
        wf.close()
        hw.close()


_CHILD = """
import json, sys
sys.path.insert(0, %r)
from ccj_amd import W_final
from tests.constraint_cases import cases, constraint_of
out = []
for c in cases():
    wf = W_final(c["seq"], c["dangles"], params=c["params"], noGU=bool(c["noGU"]), constraint=constraint_of(c))
    wf.fill()
    wf.result()
    counts = wf.il_counts()
    out.append(dict(hashes=wf.hashes(), Wn=wf.W(len(c["seq"])), structure=wf.structure, counts=counts))
    wf.close()
print(json.dumps(out))
"""


def test_fixtures_with_the_full_candidate_lists():
    """CCJ_IL_PRUNE=0 (read when a fill is enqueued): every fixture in one child process that keeps the
    full interior-loop lists gives the same matrices, and the default run did drop entries."""
    env = dict(os.environ, CCJ_IL_PRUNE="0")
    r = subprocess.run([sys.executable, "-c", _CHILD % ROOT], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    full = json.loads(r.stdout.splitlines()[-1])
    assert len(full) == len(CASES)
    dropped = 0
    for c, f in zip(CASES, full):
        assert f["hashes"] == c["hashes"] and f["Wn"] == c["Wn"], case_id(c)
        assert f["counts"][0] == f["counts"][1] and f["counts"][2] == f["counts"][3]
        wf = _wf(c)
        try:
            wf.fill()
            _check(wf, c)
            assert wf.structure == f["structure"]
            k = wf.il_counts()
            assert (k[1], k[3]) == (f["counts"][1], f["counts"][3])
            dropped += k[1] - k[0] + k[3] - k[2]
        finally:
            wf.close()
    assert dropped > 0


NOGU_E2E = [c for c in golden("e2e.json") if c["noGU"] and len(c["seq"]) <= 48]


def test_gu_constraint_is_the_reference_noGU_run():
    """F = every G-U position pair with noGU off: the last stdout line of the reference's --noGU run
    (or its exit), on every noGU fold of e2e.json with n <= 48."""
    assert len(NOGU_E2E) >= 9
    for c in NOGU_E2E:
        cons = Constraint(forbid=gu_pairs(c["seq"].replace("T", "U")))
        wf = W_final(c["seq"], c["dangles"], params=c["params"], noGU=False, constraint=cons)
        try:
            wf.fill()
            out = _outcome(wf)
            if c["rc"] == 0:
                assert out[0] == "ok" and f"{out[1]} ({out[2]:g})" == c["stdout"].splitlines()[-1], (c["seq"], c["params"])
            else:
                assert out[0] == "exit" and (out[1], out[2]) == (c["rc"], c["stderr"])
        finally:
            wf.close()


def test_allow_only_the_golden_structure():
    """Allowing only the pairs of the reference's MFE structure gives the same energy, and a structure
    whose pairs are a subset of it (on the pseudoknotted e2e folds with n <= 36)."""
    todo = pseudoknotted_e2e(36)
    assert len(todo) >= 20
    for c, st, en in todo:
        gold = pairs_of(st)
        wf = W_final(c["seq"], c["dangles"], params=c["params"], noGU=bool(c["noGU"]),
                     constraint=Constraint(allow_only=sorted(gold)))
        try:
            e = wf.ccj()
            assert "(%g)" % e == en, (c["seq"], c["params"], e, en)
            assert pairs_of(wf.structure) <= gold, (c["seq"], wf.structure, st)
        finally:
            wf.close()


# ---- every kind of context equals a fresh constrained context ------------------------------------

OTHER = "GGGAAACCCUUUGGGAAACCCAUAUGCGCAUAUGCGC"  # an unconstrained fold of another sequence first


def test_reset_constrained_after_an_unconstrained_fold():
    for c in CASES[:6]:
        n = len(c["seq"])
        wf = W_final(OTHER[:n], c["dangles"], params=c["params"], noGU=bool(c["noGU"]))
        try:
            wf.ccj()
            assert wf.constraint_count() == 0
            wf.reset(c["seq"], constraint_of(c))
            wf.fill()
            _check(wf, c, "reset")
        finally:
            wf.close()


def test_rebind_at_a_larger_capacity():
    for c in CASES[6:]:
        n = len(c["seq"])
        wf = W_final(OTHER[:n - 3], c["dangles"], params=c["params"], noGU=bool(c["noGU"]), capacity=n + 5)
        try:
            wf.ccj()
            wf.rebind(c["seq"], constraint_of(c))
            assert wf.n == n and wf.capacity == n + 5
            wf.fill()
            _check(wf, c, "rebind")
        finally:
            wf.close()


def _same_problem(params, dangles, noGU):
    return [c for c in CASES if (c["params"], c["dangles"], c["noGU"]) == (params, dangles, noGU)]


def test_lockstep_members_with_different_constraints():
    """Turner04 d2: two fixtures with their constraints, one of them a second time without one."""
    a, b = [c for c in _same_problem("Turner04", 2, 0) if len(c["seq"]) == 30]
    batch = LockstepBatch(36, 3, 2, params="Turner04")
    try:
        batch.bind([a["seq"], b["seq"], a["seq"]], [constraint_of(a), constraint_of(b), None])
        batch.fold()
        m = batch.members
        _check(m[0], a, "member 0")
        _check(m[1], b, "member 1")
        assert m[2].hashes() == _plain_hashes(a) and m[2].constraint_count() == 0
        # the stale-mask test of a batch: the same members, bound plainly
        batch.bind([b["seq"], a["seq"]])
        batch.fold()
        assert batch.members[0].hashes() == _plain_hashes(b)
        assert batch.members[1].hashes() == _plain_hashes(a)
    finally:
        batch.close()


@pytest.mark.parametrize("lockstep", [0, 2], ids=["contexts", "lockstep"])
def test_fold_many_with_constraints(lockstep):
    cs = _same_problem("Turner04", 2, 0)
    assert len(cs) == 3
    seqs = [c["seq"] for c in cs] + [cs[0]["seq"]]
    cons = [constraint_of(c) for c in cs] + [None]
    recs = fold_many(seqs, 2, params="Turner04", contexts=2, lockstep=lockstep, constraints=cons)
    for c, rec in zip(cs, recs):
        wf = _wf(c)
        try:
            wf.fill()
            out = _check(wf, c)
        finally:
            wf.close()
        assert out[0] == "ok" and rec[1:3] == (out[1], out[2]) and rec[4] == 0
    plain = W_final(seqs[3], 2, params="Turner04")
    try:
        e = plain.ccj()
        assert recs[3][1:3] == (plain.structure, e)
        assert plain.structure != recs[0][1]  # the constraint of the same sequence changed its fold
    finally:
        plain.close()


def test_band_sharded_simulation():
    for c in (CASES[0], CASES[9]):
        wf = _wf(c, shard_world=2, shard_simulate=True)
        try:
            wf.fill()
            _check(wf, c, "shard_simulate world 2")
        finally:
            wf.close()


def test_leader_launch_at_n30():
    """Split target 8 at n = 30: levels share and the leader launch runs (ccj_level_schedule)."""
    c = next(c for c in CASES if len(c["seq"]) == 30 and c["kind"] == "mix")
    wf = _wf(c, split_target=8)
    try:
        sch = [wf.level_schedule(t) for t in range(len(c["seq"]) - 2)]
        assert any(s.sharing and s.lead_split for s in sch)
        wf.fill()
        _check(wf, c, "split target 8")
    finally:
        wf.close()


# ---- no stale constraint, and refusals -------------------------------------------------------------

def test_plain_reset_and_rebind_drop_the_constraint():
    c = CASES[0]
    assert c["hashes"] != _plain_hashes(c)
    wf = _wf(c, capacity=len(c["seq"]) + 2)
    try:
        wf.fill()
        _check(wf, c)
        wf.reset(c["seq"])
        wf.fill()
        _outcome(wf)  # W is computed with the result
        assert wf.hashes() == _plain_hashes(c) and wf.constraint_count() == 0
        wf.rebind(c["seq"], constraint_of(c))
        wf.fill()
        _check(wf, c)
        wf.rebind(c["seq"])
        wf.fill()
        _outcome(wf)
        assert wf.hashes() == _plain_hashes(c) and wf.constraint_count() == 0
    finally:
        wf.close()


def _raw(unpaired=None, forbid=(), allow_only=None):
    """A ccj_constraint that has not passed ccj_amd.Constraint's own checks."""
    fb = (ctypes.c_int * max(1, 2 * len(forbid)))(*[v for p in forbid for v in p])
    ao = None if allow_only is None else (ctypes.c_int * max(1, 2 * len(allow_only)))(*[v for p in allow_only for v in p])
    c = ccj_amd._Constraint(unpaired.encode() if unpaired is not None else None, ctypes.cast(fb, ctypes.POINTER(ctypes.c_int)),
                            len(forbid), ctypes.cast(ao, ctypes.POINTER(ctypes.c_int)) if ao is not None else None,
                            0 if allow_only is None else len(allow_only))
    return c, (fb, ao)


def _bad_constraints(n):
    return [_raw(unpaired="." * (n - 1)), _raw(unpaired="." * (n - 1) + "("), _raw(forbid=[(5, 5)]), _raw(forbid=[(7, 3)]),
            _raw(forbid=[(0, 4)]), _raw(forbid=[(2, n + 1)]), _raw(allow_only=[(1, n + 1)]), _raw(unpaired="." * n, forbid=[(3, 2)])]


def test_a_refused_constraint_leaves_the_binding():
    c = CASES[1]
    n = len(c["seq"])
    L = ccj_amd.lib()
    wf = _wf(c)
    try:
        for bad, _keep in _bad_constraints(n):
            for fn in (L.ccj_reset_constrained, L.ccj_rebind_constrained):
                assert fn(wf._h, OTHER[:n].encode(), ctypes.byref(bad)) == ccj_amd.CCJ_E_ARG
                assert b"constraint" in L.ccj_last_error(wf._h)
        with pytest.raises(ccj_amd.CCJError):
            wf.reset(OTHER[:n], Constraint(forbid=[(2, n + 1)]))
        assert wf.constraint_count() > 0
        wf.fill()
        _check(wf, c, "after refusals")
    finally:
        wf.close()


def test_a_refused_member_list_leaves_the_batch():
    a, b = [c for c in _same_problem("Turner04", 2, 0) if len(c["seq"]) == 30]
    L = ccj_amd.lib()
    batch = LockstepBatch(36, 2, 2, params="Turner04")
    try:
        batch.bind([a["seq"], b["seq"]], [constraint_of(a), None])
        good, _k1 = _raw(forbid=[(1, 9)])
        bad, _k2 = _raw(forbid=[(4, 31)])
        seqs = (ctypes.c_char_p * 2)(OTHER[:30].encode(), OTHER[:30].encode())
        cons = (ctypes.POINTER(ccj_amd._Constraint) * 2)(ctypes.pointer(good), ctypes.pointer(bad))
        assert L.ccj_batch_bind_constrained(batch._h, seqs, cons, 2) == ccj_amd.CCJ_E_ARG
        with pytest.raises(ccj_amd.CCJError):
            batch.bind([OTHER[:30], OTHER[:30]], [None, Constraint(forbid=[(4, 31)])])
        batch.fold()
        _check(batch.members[0], a, "member 0 after a refused bind")
        assert batch.members[1].hashes() == _plain_hashes(b)
    finally:
        batch.close()
