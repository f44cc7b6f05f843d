"""The constraint reaches every reader of the pair table (-m gpu).

tests/golden/constraint_site_cases.json holds, for every reader of the pair table in the fill that a
constraint can decide (the sites of tests/masked_oracle.py), small constrained folds whose matrices
change when that one reader ignores the constraint (tests/test_constraint_sites.py holds the fixtures
to that on the CPU).  An engine that reads the 8x8 table where it should read the binding's relation
fails them here.  Every case goes through each kind of context: fresh on both traceback executors,
reset, rebind at a larger capacity, a lockstep batch next to its own unconstrained twin, the full
candidate lists, and the band-sharded simulation.
"""
import json
import os
import subprocess
import sys

import pytest

import ccj_amd
from ccj_amd import Constraint, LockstepBatch, W_final
from tests.constraint_cases import pairs_of
from tests.constraint_site_cases import case_id, cases, one_case_per_site
from tests.oracle_lib import ROOT, OracleFold, blob

pytestmark = pytest.mark.gpu

CASES = cases()
OTHER = "GGGAAACCCUUUGGGAAACCCAUAUGCGCAUAUGCGC"  # an unconstrained fold of another sequence first
_plain = {}


def _constraint(c):
    return Constraint(c["unpaired"], [tuple(p) for p in c["forbid"]],
                      None if c["allow_only"] is None else [tuple(p) for p in c["allow_only"]])


def _wf(c, **kw):
    return W_final(c["seq"], c["dangles"], params=c["params"], noGU=bool(c["noGU"]), constraint=_constraint(c), **kw)


def _outcome(wf):
    """("ok", structure, energy) or ("exit", code, stderr) of a filled context."""
    try:
        e = wf.result()
        return ("ok", wf.structure, e)
    except ccj_amd.BacktrackExit as ex:
        return ("exit", ex.exit_code, ex.msg)


def _check(wf, c, what, out=None):
    """The filled context against the fixture: the 31 hashes, W(n), and the constraint in the structure."""
    n = len(c["seq"])
    out = _outcome(wf) if out is None else out
    got = wf.hashes()
    bad = [k for k in c["hashes"] if got[k] != c["hashes"][k]]
    assert not bad, (what, case_id(c), bad, sorted(c["pins"]))
    assert wf.W(n) == c["Wn"], (what, case_id(c))
    if out[0] == "ok":
        assert out[2] == c["Wn"] / 100.0, (what, case_id(c), out)
        F = _constraint(c).forbidden(n)
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
def test_fresh_context_on_both_traceback_executors(c):
    wf = _wf(c)
    hw = _wf(c, host_traceback=True)
    try:
        wf.fill()
        dev = _check(wf, c, "device traceback")
        assert wf.constraint_count() > 0
        hw.fill()
        host = _check(hw, c, "host traceback")
        assert dev == host  # the structure, or the same reference exit
    finally:
        wf.close()
        hw.close()


@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_reset_after_an_unconstrained_fold(c):
    n = len(c["seq"])
    seq0 = OTHER[:n].replace("U", "T") if c["params"].startswith("DNA") else OTHER[:n]
    wf = W_final(seq0, c["dangles"], params=c["params"], noGU=bool(c["noGU"]))
    try:
        wf.ccj()
        assert wf.constraint_count() == 0
        wf.reset(c["seq"], _constraint(c))
        wf.fill()
        _check(wf, c, "reset")
    finally:
        wf.close()


@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_rebind_at_capacity_n_plus_5(c):
    n = len(c["seq"])
    wf = W_final(OTHER[:n - 3], c["dangles"], params=c["params"], noGU=bool(c["noGU"]), capacity=n + 5)
    try:
        wf.ccj()
        wf.rebind(c["seq"], _constraint(c))
        assert wf.n == n and wf.capacity == n + 5
        wf.fill()
        _check(wf, c, "rebind")
    finally:
        wf.close()


@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_lockstep_beside_its_unconstrained_twin(c):
    n = len(c["seq"])
    batch = LockstepBatch(n + 2, 2, c["dangles"], params=c["params"], noGU=bool(c["noGU"]))
    try:
        batch.bind([c["seq"], c["seq"]], [_constraint(c), None])
        batch.fold()
        m = batch.members
        out = ("exit", m[0].exit.exit_code, m[0].exit.msg) if m[0].exit is not None else ("ok", m[0].structure, m[0].energy)
        _check(m[0], c, "lockstep member", out)
        assert m[1].hashes() == _plain_hashes(c) and m[1].constraint_count() == 0
        assert c["hashes"] != _plain_hashes(c)  # the constraint decides something in every case
    finally:
        batch.close()


_CHILD = """
import json, sys
sys.path.insert(0, %r)
import ccj_amd
from ccj_amd import Constraint, W_final
from tests.constraint_site_cases import cases
out = []
for c in cases():
    cons = Constraint(c["unpaired"], [tuple(p) for p in c["forbid"]])
    wf = W_final(c["seq"], c["dangles"], params=c["params"], noGU=bool(c["noGU"]), constraint=cons)
    wf.fill()
    try:
        wf.result()
    except ccj_amd.BacktrackExit:
        pass
    out.append(dict(hashes=wf.hashes(), Wn=wf.W(len(c["seq"])), structure=wf.structure, counts=wf.il_counts()))
    wf.close()
print(json.dumps(out))
"""


def test_with_the_full_candidate_lists():
    """CCJ_IL_PRUNE=0 (read when a fill is enqueued): every case in one child process that keeps the
    full interior-loop lists gives the fixture's matrices."""
    assert all(c["allow_only"] is None for c in CASES)
    env = dict(os.environ, CCJ_IL_PRUNE="0")
    r = subprocess.run([sys.executable, "-c", _CHILD % ROOT], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    full = json.loads(r.stdout.splitlines()[-1])
    assert len(full) == len(CASES)
    for c, f in zip(CASES, full):
        bad = [k for k in c["hashes"] if f["hashes"][k] != c["hashes"][k]]
        assert not bad and f["Wn"] == c["Wn"], (case_id(c), bad)
        assert f["counts"][0] == f["counts"][1] and f["counts"][2] == f["counts"][3]  # nothing was dropped


@pytest.mark.parametrize("c", one_case_per_site(), ids=case_id)
def test_band_sharded_simulation(c):
    wf = _wf(c, shard_world=2, shard_simulate=True)
    try:
        wf.fill()
        _check(wf, c, "shard_simulate world 2")
    finally:
        wf.close()
