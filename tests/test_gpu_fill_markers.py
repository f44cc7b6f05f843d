"""Timing mode 2 (a marker pair around every kernel family launch of the fill) on each kind of fill (-m gpu).

The markers are recorded by the code that launches the kernels, and ccj_fill_device reads every pair
back, so a pair that was not recorded fails the fill.  The n = 52 reference fixture at split target
328 reaches all six launch regimes (tests/schedule_rows.py), the leader launch included.  It is folded
as an unsharded context, as a shard_simulate context of world 3 and as an in-process group of world 2,
each with set_timing(1) and set_timing(2): the markers must not change a result, and mode 2 must
leave a time for every level.
"""
import ctypes
import math
import threading

import pytest

from tests.oracle_lib import golden
from tests.schedule_rows import ALL_REGIME_TARGET, nlev

pytestmark = pytest.mark.gpu

CASE = next(c for c in golden("hashes.json") if len(c["seq"]) == 52)
N = len(CASE["seq"])
TARGET = ALL_REGIME_TARGET[N]
KINDS = {"unsharded": {}, "simulate3": {"shard_world": 3, "shard_simulate": True}, "group2": {"shard_world": 2}}
_DP = ctypes.POINTER(ctypes.c_double)


def _wf(**kw):
    from ccj_amd import W_final
    return W_final(CASE["seq"], CASE["dangles"], params=CASE["params"], noGU=bool(CASE["noGU"]), split_target=TARGET, **kw)


def _result(wf):
    from ccj_amd import BacktrackExit
    try:
        return ("ok", wf.result(), wf.structure, wf.stdout_msgs)
    except BacktrackExit as ex:
        return ("exit", ex.exit_code, ex.msg, ex.stdout)


def _times(wf, group):
    """name -> the per-level array of a mode-2 fill (level and iloop: the levels; diag2d: every span)."""
    from ccj_amd import lib
    L = lib()
    L.ccj_level_times.argtypes = [ctypes.c_void_p, _DP, _DP, ctypes.c_int]
    L.ccj_iloop_times.argtypes = [ctypes.c_void_p, _DP, ctypes.c_int]
    L.ccj_ppush_times.argtypes = [ctypes.c_void_p, _DP, ctypes.c_int]
    L.ccj_exchange_times.argtypes = [ctypes.c_void_p, _DP, _DP, ctypes.c_int]
    lv, dg, il, pp, xe, xb = [(ctypes.c_double * N)(*([math.nan] * N)) for _ in range(6)]
    assert L.ccj_level_times(wf._h, lv, dg, N) == 0
    assert L.ccj_iloop_times(wf._h, il, N) == 0
    assert L.ccj_ppush_times(wf._h, pp, N) == 0
    out = {"level": list(lv)[:nlev(N)], "diag2d": list(dg), "iloop": list(il)[:nlev(N)], "ppush": list(pp)[:nlev(N)]}
    if group:
        assert L.ccj_exchange_times(wf._h, xe, xb, N) == 0
        out.update(edge=list(xe)[:nlev(N)], bulk=list(xb)[:nlev(N)])
    return out


def _fold(kind, mode):
    """[(hashes, result, times or None) of every context of the fold]: one, or the group's ranks."""
    from ccj_amd import LocalGroup
    group = kind == "group2"
    g = LocalGroup(2) if group else None
    ranks = [_wf(shard_rank=r, local_group=g, **KINDS[kind]) for r in range(2)] if group else [_wf(**KINDS[kind])]
    errs = []

    def run(wf):
        try:
            wf.set_timing(mode)
            wf.fill()
        except Exception as e:  # noqa: BLE001
            errs.append(repr(e))

    try:
        th = [threading.Thread(target=run, args=(wf,), daemon=True) for wf in ranks]
        for x in th:
            x.start()
        for x in th:
            x.join(timeout=120)
        alive = [r for r, x in enumerate(th) if x.is_alive()]
        assert not alive, f"ranks {alive} did not finish their fill within 120 s (contexts left open)"
        assert not errs, errs  # mode 2: every marker pair fill_finish reads was recorded
        out = []
        for wf in ranks:
            res = _result(wf)  # W is computed here, so before the hashes
            out.append((wf.hashes(), res, _times(wf, group) if mode == 2 else None))
        return out
    finally:
        if not any(x.is_alive() for x in th):
            for wf in ranks:
                wf.close()
            if g is not None:
                g.close()


@pytest.fixture(scope="module")
def plain():
    """The unsharded mode-1 fold every other fold is held against."""
    (hashes, res, _), = _fold("unsharded", 1)
    return hashes, res


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("kind", list(KINDS))
def test_markers_leave_results_alone_and_time_every_level(plain, kind, mode):
    assert len(CASE["hashes"]) == 31
    for rank, (hashes, res, times) in enumerate(_fold(kind, mode)):
        bad = [k for k in CASE["hashes"] if hashes[k] != CASE["hashes"][k]]
        assert not bad, f"{kind} mode {mode} rank {rank}: matrices differ from the reference: {bad}"
        assert res == plain[1], f"{kind} mode {mode} rank {rank}"
        if mode == 2:
            assert set(times) == {"level", "diag2d", "iloop", "ppush"} | ({"edge", "bulk"} if kind == "group2" else set())
            for name, v in times.items():
                print(f"{kind} rank {rank} {name}: sum {sum(v):.4f} ms min {min(v):.5f} max {max(v):.5f}")
                assert all(math.isfinite(x) and x >= 0 for x in v), (kind, rank, name, v)
                assert sum(v) > 0, (kind, rank, name)
