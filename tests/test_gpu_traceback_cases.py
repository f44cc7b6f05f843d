"""GPU tests (-m gpu) over tests/golden/traceback_cases.json: folds that drive the reference's own
traceback through every case and sub-branch a search could reach (oracle/gen_traceback_cases.py),
several with non-default pseudoknot penalties (ccj_problem.pen).  Per case, against what the
reference itself printed:

  * the device fill's 31 matrix hashes and W(n): pins the tables the engine builds from `pen`
    (the int16-saturated stack terms, the interior-loop precompute, the packed iloop entries);
  * the device traceback (k_backtrack): structure, energy, side messages, or the exit's stderr and
    code;
  * the same node logic (ccj_traceback.h) through the host executor (host_traceback=True);
  * the three largest cases band-sharded over an in-process world of 2.
"""
import threading

import pytest

from tests.oracle_lib import golden
from tests.test_traceback_cases import case_id

pytestmark = pytest.mark.gpu

CASES = golden("traceback_cases.json")["cases"]
LARGEST = sorted(CASES, key=lambda c: -len(c["seq"]))[:3]


def _pen(case):
    return tuple(case["pen"]) if case["pen"] is not None else None


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_device_fill_matches_reference(case):
    from ccj_amd import W_final
    wf = W_final(case["seq"], case["dangles"], params=case["params"], noGU=bool(case["noGU"]), pen=_pen(case))
    try:
        wf.fill()
        try:
            wf.result()
        except Exception:
            pass  # the reference exits in some backtracks; W is computed before it
        got = wf.hashes()
        bad = [k for k in case["hashes"] if got[k] != case["hashes"][k]]
        assert not bad, f"matrices differ from the reference: {bad}"
        assert wf.W(len(case["seq"])) == case["mfe"]
    finally:
        wf.close()


@pytest.mark.parametrize("host", [False, True], ids=["device", "host"])
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_traceback_matches_reference(case, host):
    from ccj_amd.cli import fold_cli
    rc, out, err = fold_cli(case["seq"], case["params"], case["dangles"], bool(case["noGU"]), pen=_pen(case),
                            host_traceback=host)
    assert out == case["stdout"]
    assert err == case["stderr"]
    assert rc == case["rc"]


@pytest.mark.parametrize("case", LARGEST, ids=case_id)
def test_sharded_world2_matches_reference(case):
    """Both ranks of a band-sharded fold (own contexts, in-process exchange group) end with the
    reference's matrices and print the reference's output."""
    from ccj_amd import BacktrackExit, LocalGroup, W_final
    from ccj_amd.cli import fmt_energy
    g = LocalGroup(2)
    ranks = [W_final(case["seq"], case["dangles"], params=case["params"], noGU=bool(case["noGU"]), pen=_pen(case),
                     shard_world=2, shard_rank=r, local_group=g) for r in range(2)]
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
    try:
        assert not errs, errs
        for wf in ranks:
            try:
                e = wf.result()
                got = (0, wf.stdout_msgs + case["seq"] + "\n" + f"{wf.structure} ({fmt_energy(e)})\n", "")
            except BacktrackExit as ex:
                got = (ex.exit_code, ex.stdout, ex.msg)
            assert got == (case["rc"], case["stdout"], case["stderr"])
            h = wf.hashes()
            bad = [k for k in case["hashes"] if h[k] != case["hashes"][k]]
            assert not bad, bad
            assert wf.W(len(case["seq"])) == case["mfe"]
    finally:
        for wf in ranks:
            wf.close()
        g.close()
