"""Every launch regime of the level chain at small n (-m gpu), on real reference hashes.

k_level4d runs with split 1, 2, 4 or 8; on the sharing levels [g_lo, g_hi) k_level4d_lead runs
its scans over 2, 4 or 8 waves; with g_lo > 0 the followers of levels g_lo .. g_lo+2 whose leader
would lie below g_lo scan their full range.  Which of these a level gets is decided by n and the
split target, and under the default target nothing below n = 159 shares at all.
The split_target option reproduces every regime at n = 52 .. 64: tests/schedule_rows.py lists the
rows, tests/test_schedule.py pins on the CPU what they reach, and every test here first reads the
context's own schedule getter (W_final.level_schedule) and asserts the regimes it is about to
run, so a tuning change cannot silently empty a test.

References: the reference's own fill (tests/golden/hashes.json, the six cases with n >= 51, and
tests/golden/e2e.json for the traceback) and the C restatement (OracleFold) for fresh inputs.
On a hash mismatch the report names the first differing cell in level order and the regime of
its level (tests/oracle_lib.py explain_mismatch).
"""
import json
import os
import random
import subprocess
import sys
import threading

import pytest

from tests.oracle_lib import ROOT, OracleFold, blob, explain_mismatch, golden
from tests.schedule_rows import (ALL_REGIMES, ALL_REGIME_TARGET, BOUNDARY_TARGET, SHARDED, flips, nlev, schedule,
                                 signature)

pytestmark = pytest.mark.gpu

FIX = [c for c in golden("hashes.json") if len(c["seq"]) >= 51]
E2E = {(c["seq"], c["params"], c["dangles"], c["noGU"]): c for c in golden("e2e.json")}


def _id(c):
    return f"n{len(c['seq'])}-{c['params']}-d{c['dangles']}-g{c['noGU']}"


def _wf(case, target, **kw):
    from ccj_amd import W_final
    return W_final(case["seq"], case["dangles"], params=case["params"], noGU=bool(case["noGU"]), split_target=target, **kw)


def _ran(wf, n, target, world=1, ranks=None):
    """The schedule the context itself reports, per rank: it resolved the target we passed, and it
    equals the context-free helper level by level.  Returns the union of its regimes."""
    assert wf.schedule_options() == (target, True)
    got = set()
    for r in (range(world) if ranks is None else ranks):
        sch = [wf.level_schedule(t, r) for t in range(nlev(n))]
        assert sch == schedule(n, target, world, r)
        got |= {s.regime for s in sch}
    return got


def _result(wf):
    from ccj_amd import BacktrackExit
    try:
        e = wf.result()
        return ("ok", e, wf.structure, wf.stdout_msgs)
    except BacktrackExit as ex:
        return ("exit", ex.exit_code, ex.msg, ex.stdout)


def _check_reference(wf, case, world=1, simulate=True):
    """All 31 hashes and W(n) against the reference's fill; the traceback against its CLI run."""
    n = len(case["seq"])
    res = _result(wf)  # W is computed here, before any backtrack exit of the reference's
    got = wf.hashes()
    assert len(case["hashes"]) == 31
    bad = [k for k in case["hashes"] if got[k] != case["hashes"][k]]
    assert not bad, explain_mismatch(wf, case["seq"], case["params"], case["dangles"], case["noGU"], bad, world, simulate)
    assert wf.W(n) == case["mfe"]
    e2e = E2E.get((case["seq"], case["params"], case["dangles"], case["noGU"]))
    if e2e is not None:
        if res[0] == "ok":
            assert e2e["rc"] == 0 and f"{res[2]} ({res[1]:g})" == e2e["stdout"].splitlines()[-1]
        else:
            assert res[1] == e2e["rc"] and res[2] == e2e["stderr"]


def test_fixtures_are_the_reference_runs_the_rows_were_made_for():
    assert sorted((len(c["seq"]), c["params"], c["dangles"]) for c in FIX) == [
        (52, "Turner04", 0), (52, "Turner04", 1), (54, "DirksPierce09", 2), (54, "Turner04", 2),
        (55, "DirksPierce03", 1), (55, "Turner04", 1)]
    assert all(k in E2E for k in [(c["seq"], c["params"], c["dangles"], c["noGU"]) for c in FIX])


@pytest.mark.parametrize("case", FIX, ids=_id)
def test_reference_fixture_in_every_regime(case):
    """Plain split 1, 2, 4, 8 and lead split 2, 4, 8 in one unsharded fold with g_lo > 0."""
    n = len(case["seq"])
    target = ALL_REGIME_TARGET[n]
    wf = _wf(case, target)
    try:
        assert _ran(wf, n, target) == ALL_REGIMES
        s = wf.level_schedule(0)
        assert 0 < s.g_lo < s.g_hi == nlev(n)
        wf.fill()
        _check_reference(wf, case)
    finally:
        wf.close()


@pytest.mark.parametrize("cls", [0, 1, 2, 3])
@pytest.mark.parametrize("case", FIX, ids=_id)
def test_leaderless_boundary_classes(case, cls):
    """g_lo mod 4 = cls: which followers of levels g_lo .. g_lo+2 find no leader below g_lo."""
    n = len(case["seq"])
    target = BOUNDARY_TARGET[n][cls]
    wf = _wf(case, target)
    try:
        got = _ran(wf, n, target)
        s = wf.level_schedule(0)
        assert 0 < s.g_lo < s.g_hi == nlev(n) and s.g_lo % 4 == cls
        assert {(1, 2), (1, 4)} <= got
        wf.fill()
        _check_reference(wf, case)
    finally:
        wf.close()


N55 = next(c for c in FIX if len(c["seq"]) == 55 and c["params"] == "Turner04")
# every target in [352, 400] at which g_lo or a level's lead split changes, and the target below it
# (400: the first target at which n = 55 does not share any more)
THRESHOLDS = sorted({t - d for t in flips(55, ALL_REGIME_TARGET[55] - 1, 400) for d in (0, 1)})


@pytest.mark.parametrize("target", THRESHOLDS)
def test_targets_on_either_side_of_each_threshold(target):
    n = 55
    wf = _wf(N55, target)
    try:
        _ran(wf, n, target)
        sig = (wf.level_schedule(0).g_lo, tuple(wf.level_schedule(t).lead_split for t in range(nlev(n))))
        assert sig == signature(n, target)
        wf.fill()
        _check_reference(wf, N55)
    finally:
        wf.close()


def test_mismatch_report_names_cell_level_and_regime():
    """The failure report itself, run where it has something to say: a correct Turner04 fold held
    against the oracle's DirksPierce09 fold of the same sequence."""
    n, target = 55, ALL_REGIME_TARGET[55]
    wf = _wf(N55, target)
    try:
        wf.fill()
        _result(wf)
        text = explain_mismatch(wf, N55["seq"], "DirksPierce09", N55["dangles"], N55["noGU"], ["PK", "PL", "V", "WM"])
        assert "first differing 4-D cell: P" in text and "level t=" in text and " a=" in text
        assert "level regime: sharing=" in text and "plain split" in text and "lead split" in text
        assert f"g_lo={wf.level_schedule(0).g_lo} " in text
        assert "first differing V(i, j) by span: (" in text
    finally:
        wf.close()


def _rseq(seed, n, alphabet):
    r = random.Random(seed)
    return "".join(r.choice(alphabet) for _ in range(n))


# n, alphabet, parameter set, dangles, noGU (n <= 64: the sequential oracle takes about 2 s there and
# about 5 s at n = 72)
FRESH = [(57, "ACGU", "Turner04", 2, 0), (58, "GGCCAU", "DirksPierce09", 1, 0), (59, "GCAU", "DirksPierce03", 0, 1),
         (60, "AU", "CaoChen09", 2, 0), (61, "ACGU", "Matthews04", 1, 1), (62, "GGCCAU", "Turner04", 0, 0),
         (63, "GCAU", "CaoChen09", 2, 1), (64, "ACGU", "DirksPierce09", 2, 0)]


@pytest.mark.parametrize("n,alphabet,params,d,g", FRESH, ids=lambda v: str(v))
def test_fresh_inputs_in_every_regime_match_oracle(n, alphabet, params, d, g):
    """Seeded inputs under the all-regime target of their n: every matrix against the C restatement,
    and the device traceback against the host executor on the same schedule."""
    seq = _rseq(6200 + n, n, alphabet)
    case = {"seq": seq, "params": params, "dangles": d, "noGU": g}
    target = ALL_REGIME_TARGET[n]
    o = OracleFold(seq, blob(params), d, g)
    dev = _wf(case, target)
    host = _wf(case, target, host_traceback=True)
    try:
        assert _ran(dev, n, target) == ALL_REGIMES and _ran(host, n, target) == ALL_REGIMES
        assert dev.level_schedule(0).g_lo > 0
        dev.fill()
        host.fill()
        rd, rh = _result(dev), _result(host)
        want = o.hashes()
        for wf in (dev, host):
            got = wf.hashes()
            bad = [k for k in want if got[k] != want[k]]
            assert not bad, explain_mismatch(wf, seq, params, d, g, bad)
        assert rd == rh
        assert [dev.W(j) for j in range(n + 1)] == [host.W(j) for j in range(n + 1)] == [o.W(j) for j in range(n + 1)]
    finally:
        dev.close()
        host.close()
        o.close()


@pytest.mark.parametrize("world", [2, 3, 4])
@pytest.mark.parametrize("case", FIX, ids=_id)
def test_sharded_simulation_in_every_regime(case, world):
    """Every rank's launches in one context: a rank's own block count moves its plain and lead
    splits again (the union per row is pinned in tests/test_schedule.py)."""
    n = len(case["seq"])
    target = ALL_REGIME_TARGET[n]
    wf = _wf(case, target, shard_world=world, shard_simulate=True)
    try:
        got = _ran(wf, n, target, world)
        assert got == SHARDED[(n, target, world)] and (1, 8) in got
        assert wf.level_schedule(0).g_lo > 0
        wf.fill()
        _check_reference(wf, case, world)
    finally:
        wf.close()


def _fold_group(case, world, target):
    """Every rank as its own context and thread, exchanging through an in-process group (the real
    sharded path: own blocks only, edge and bulk all-gathers), as tests/test_gpu_shard.py does."""
    from ccj_amd import LocalGroup
    g = LocalGroup(world)
    ranks = [_wf(case, target, shard_world=world, shard_rank=r, local_group=g) for r in range(world)]
    errs = []

    def run(wf):
        try:
            wf.fill()
        except Exception as e:  # noqa: BLE001
            errs.append(repr(e))

    th = [threading.Thread(target=run, args=(wf,), daemon=True) for wf in ranks]
    for x in th:
        x.start()
    for x in th:
        x.join(timeout=120)
    # a rank still inside ccj_fill owns its context: fail without closing anything it may touch
    alive = [r for r, x in enumerate(th) if x.is_alive()]
    assert not alive, f"ranks {alive} did not finish their fill within 120 s (contexts left open)"
    assert not errs, errs
    return g, ranks


@pytest.mark.parametrize("world", [2, 4])
def test_exchange_group_with_sharing_on_a_late_range(world):
    """The edge / bulk exchange with sharing active and g_lo > 0 (the ring partials of the leaders
    stay on their rank; the cells they complete travel): every rank holds the reference's fold."""
    case = next(c for c in FIX if len(c["seq"]) == 55 and c["params"] == "DirksPierce03")
    n, target = 55, ALL_REGIME_TARGET[55]
    g, ranks = _fold_group(case, world, target)
    try:
        got = set()
        for r, wf in enumerate(ranks):
            got |= _ran(wf, n, target, world, ranks=[r])
            s = wf.level_schedule(0)
            assert 0 < s.g_lo < s.g_hi == nlev(n)
            assert any(wf.level_schedule(t).lead_split >= 2 for t in range(nlev(n)))
        assert got == SHARDED[(n, target, world)]
        for wf in ranks:
            _check_reference(wf, case, world, simulate=False)
    finally:
        for wf in ranks:
            wf.close()
        g.close()


def test_reset_across_regimes_matches_oracle():
    """One context under an all-regime target, rebound to an AU-poor, a GC-rich and a mixed sequence:
    the schedule stays, the work lists change, every fold equals the oracle."""
    n, params = 55, "Turner04"
    target = ALL_REGIME_TARGET[n]
    seqs = [_rseq(31, n, "AAAAUC"), _rseq(32, n, "GGCCAU"), _rseq(33, n, "ACGU")]
    case = {"seq": _rseq(30, n, "ACGU"), "params": params, "dangles": 2, "noGU": 0}
    wf = _wf(case, target)
    try:
        for s in seqs:
            wf.reset(s)
            assert _ran(wf, n, target) == ALL_REGIMES and wf.level_schedule(0).g_lo > 0
            wf.fill()
            _result(wf)
            o = OracleFold(s, blob(params), 2, 0, threads=0)
            try:
                got, want = wf.hashes(), o.hashes()
                bad = [k for k in want if got[k] != want[k]]
                assert not bad, explain_mismatch(wf, s, params, 2, 0, bad)
                assert wf.W(n) == o.W(n)
            finally:
                o.close()
    finally:
        wf.close()


@pytest.mark.parametrize("mode", [{"CCJ_CHECK_ITEMS": "1"}, {"CCJ_HOST_COUNT": "1", "CCJ_CHECK_ITEMS": "1"}],
                         ids=["items-gpu-count-checked", "items-host-count"])
def test_item_modes_under_an_all_regime_target(mode):
    """tests/test_gpu_items.py's two child modes once more, with CCJ_SPLIT_TARGET in the child's
    environment, on the two n = 55 reference fixtures (unsharded and 4 shards in one context)."""
    from tests.test_gpu_items import CHILD
    n, target = 55, ALL_REGIME_TARGET[55]
    picked = [c for c in FIX if len(c["seq"]) == n]
    assert len(picked) == 2
    cases = [dict({k: c[k] for k in ("seq", "dangles", "params", "noGU")}, tag=_id(c)) for c in picked]
    env = dict(os.environ, CCJ_SPLIT_TARGET=str(target), **mode)
    env.pop("CCJ_SHARE_SPLITS", None)
    p = subprocess.run([sys.executable, "-c", CHILD, ROOT, json.dumps(cases)], env=env, capture_output=True, text=True,
                       timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    got = json.loads(p.stdout.strip().splitlines()[-1])
    assert len(got) == 2 * len(picked)
    by_tag = {_id(c): c for c in picked}
    for r in got:
        case, world = by_tag[r["tag"]], r["world"]
        assert r["target"] == target and r["g_lo"] > 0
        want = ALL_REGIMES if world == 1 else SHARDED[(n, target, world)]
        assert {tuple(x) for x in r["regimes"]} == want
        bad = [k for k in case["hashes"] if r["hashes"][k] != case["hashes"][k]]
        assert not bad, f"{r['tag']} world {world}: matrices differ from the reference: {bad}"
        e2e = E2E[(case["seq"], case["params"], case["dangles"], case["noGU"])]
        assert r["line"] == e2e["stdout"].splitlines()[-1]
