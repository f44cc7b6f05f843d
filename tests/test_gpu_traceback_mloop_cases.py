"""GPU tests (-m gpu) over tests/golden/traceback_mloop_cases.json: folds with a strongly negative bp,
inside the int16 domain (tests/test_traceback_mloop_cases.py), under which the reference's own
traceback enters the multiloop-family nodes: the 16 P_P{L,R,M,O}mloop / ...00 / ...01 / ...10 cases
of ccj_traceback.h, P_WB, P_WBP and the multiloop sub-case of P_PL / P_PR / P_PM / P_PO.  The engine
serves these twelve matrices from 2-D tables (tab_get) and closed forms (cf_get); here, against what
the reference itself printed:

  * the device fill's 31 matrix hashes and W(n), per case;
  * the device traceback and the host executor (host_traceback=True): stdout, stderr and exit code;
  * the two smallest cases in a lean, a full-d4 (CCJ_D4_FULL=1), an overlap_d2h and a two-rank context:
    all 22 matrices cell by cell against the C restatement, then the traceback in that context;
  * the n = 57 .. 64 cases under every launch regime of the level chain (ALL_REGIME_TARGET);
  * the largest case band-sharded over an in-process world of 2.
"""
import threading

import pytest

from tests.mloop2d_cases import valid_cells
from tests.oracle_lib import HASH_NAMES, OracleFold, blob, first_difference, golden
from tests.schedule_rows import ALL_REGIME_TARGET, ALL_REGIMES, nlev, schedule
from tests.test_traceback_mloop_cases import case_id

pytestmark = pytest.mark.gpu

CASES = golden("traceback_mloop_cases.json")["cases"]
BY_SIZE = sorted(CASES, key=lambda c: len(c["seq"]))  # stable: ties keep the fixture's order
SMALLEST = BY_SIZE[:2]
LARGEST = BY_SIZE[-1]
REGIME_CASES = [c for c in CASES if len(c["seq"]) in ALL_REGIME_TARGET]

_columns = {}


def _wf(case, **kw):
    from ccj_amd import W_final
    return W_final(case["seq"], case["dangles"], params=case["params"], noGU=bool(case["noGU"]), pen=tuple(case["pen"]), **kw)


def _want(case):
    return case["rc"], case["stdout"], case["stderr"]


def _output(wf, case):
    """(rc, stdout, stderr) of this context's traceback, put together as ccj_amd.cli.fold_cli prints it."""
    from ccj_amd import BacktrackExit
    from ccj_amd.cli import fmt_energy
    try:
        e = wf.result()
        return 0, wf.stdout_msgs + case["seq"] + "\n" + f"{wf.structure} ({fmt_energy(e)})\n", ""
    except BacktrackExit as ex:
        return ex.exit_code, ex.stdout, ex.msg


def _check_hashes(wf, case):
    """All 31 hashes and W(n) against the reference's (call after _output: W is computed there)."""
    got = wf.hashes()
    assert len(case["hashes"]) == 31
    bad = [k for k in case["hashes"] if got[k] != case["hashes"][k]]
    if bad:
        o = OracleFold(case["seq"], blob(case["params"]), case["dangles"], case["noGU"], pen=case["pen"])
        try:
            where = first_difference(wf.get4, o.get4, o.n, bad)
        finally:
            o.close()
        assert not bad, f"matrices differ from the reference: {bad}; first 4-D difference: {where}"
    assert wf.W(len(case["seq"])) == case["mfe"]


def _fold_pair(case, **kw):
    """Two ranks as their own contexts and threads over an in-process group."""
    from ccj_amd import LocalGroup
    g = LocalGroup(2)
    ranks = [_wf(case, shard_world=2, shard_rank=r, local_group=g, **kw) for r in range(2)]
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
    # a rank still inside its fill owns its context: fail without closing anything it may touch
    alive = [r for r, x in enumerate(th) if x.is_alive()]
    assert not alive, f"ranks {alive} did not finish their fill within 120 s (contexts left open)"
    assert not errs, errs
    return g, ranks


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_device_fill_matches_reference(case):
    wf = _wf(case)
    try:
        wf.fill()
        _output(wf, case)
        _check_hashes(wf, case)
    finally:
        wf.close()


@pytest.mark.parametrize("host", [False, True], ids=["device", "host"])
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_traceback_matches_reference(case, host):
    from ccj_amd.cli import fold_cli
    rc, out, err = fold_cli(case["seq"], case["params"], case["dangles"], bool(case["noGU"]), pen=tuple(case["pen"]),
                            host_traceback=host)
    assert out == case["stdout"]
    assert err == case["stderr"]
    assert rc == case["rc"]


# ---- the two smallest cases: all 22 matrices cell by cell, then the traceback, per kind of context
def _oracle_columns(case):
    """The restatement's 22 matrices over every valid cell of the case, read once and never changed."""
    key = case_id(case)
    if key not in _columns:
        o = OracleFold(case["seq"], blob(case["params"]), case["dangles"], case["noGU"], pen=case["pen"])
        try:
            assert o.low_stores() == 0
            assert o.hashes() == case["hashes"]  # the restatement is the reference's, cell by cell
            cells = list(valid_cells(o.n))
            _columns[key] = (cells, [[o.get4(x, *c) for c in cells] for x in range(22)])
        finally:
            o.close()
    return _columns[key]


def _check_all22_cells(wf, case):
    cells, cols = _oracle_columns(case)
    for x in range(22):
        diff = [(c, wf.get4(x, *c), v) for c, v in zip(cells, cols[x]) if wf.get4(x, *c) != v]
        assert not diff, f"{HASH_NAMES[x]}: {len(diff)} cells differ, first (cell, got, oracle) = {diff[0]}"


@pytest.mark.parametrize("host", [False, True], ids=["device", "host"])
@pytest.mark.parametrize("kind", ["lean", "d4_full", "overlap_d2h", "sharded2"])
@pytest.mark.parametrize("case", SMALLEST, ids=case_id)
def test_all_22_matrices_then_traceback_in_every_kind_of_context(case, kind, host, monkeypatch):
    """A lean context's traceback reads the twelve matrices through DevStore from the tables and closed
    forms; a full one (the switch, a mirror streamed during the fill, each rank of a pair) reads d4."""
    if kind == "sharded2":
        g, ranks = _fold_pair(case, host_traceback=host)
        try:
            for wf in ranks:
                _check_all22_cells(wf, case)
                assert _output(wf, case) == _want(case)
                _check_hashes(wf, case)
        finally:
            for wf in ranks:
                wf.close()
            g.close()
        return
    if kind == "d4_full":
        monkeypatch.setenv("CCJ_D4_FULL", "1")  # read when the context is created: d4 keeps 22 slots
    wf = _wf(case, host_traceback=host, overlap_d2h=(kind == "overlap_d2h"))
    try:
        wf.fill()
        _check_all22_cells(wf, case)
        assert _output(wf, case) == _want(case)
        _check_hashes(wf, case)
    finally:
        wf.close()


# ---- n = 57 .. 64: every launch regime of the level chain
def test_regime_cases_exist():
    assert len(REGIME_CASES) >= 2


@pytest.mark.parametrize("case", REGIME_CASES, ids=case_id)
def test_every_regime_matches_reference(case):
    """Plain split 1, 2, 4, 8 and lead split 2, 4, 8 in one fold with g_lo > 0 (the context's own
    schedule getter says so): hashes, W(n) and both executors' output equal the reference's."""
    n = len(case["seq"])
    target = ALL_REGIME_TARGET[n]
    dev = _wf(case, split_target=target)
    host = _wf(case, split_target=target, host_traceback=True)
    try:
        for wf in (dev, host):
            assert wf.schedule_options() == (target, True)
            sch = [wf.level_schedule(t) for t in range(nlev(n))]
            assert sch == schedule(n, target)
            assert {s.regime for s in sch} == ALL_REGIMES
            s = wf.level_schedule(0)
            assert 0 < s.g_lo < s.g_hi == nlev(n)
        dev.fill()
        host.fill()
        for wf in (dev, host):
            assert _output(wf, case) == _want(case)
            _check_hashes(wf, case)
    finally:
        dev.close()
        host.close()


# ---- the largest case, band-sharded
def test_sharded_world2_matches_reference():
    """Both ranks of a band-sharded fold end with the reference's matrices and print its output."""
    case = LARGEST
    g, ranks = _fold_pair(case)
    try:
        for wf in ranks:
            assert _output(wf, case) == _want(case)
            _check_hashes(wf, case)
    finally:
        for wf in ranks:
            wf.close()
        g.close()
