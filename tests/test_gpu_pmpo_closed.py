"""The PM / PO multiloop families in closed form (ccj_amd/csrc/ccj_pmpo2d.h), on the GPU (-m gpu).

The level kernels no longer compute PMmloop00/01/10 and POmloop00/01/10: k_diag2d fills nine 2-D
tables, get_PMmloop / get_POmloop evaluate the 10 / 01 values from them, the loop records and the
leader partials shrink to the PfromX / PK fields, and every reader of the six matrices (get4, the
hashes, the host mirror, both traceback executors) is served by the evaluators.  Everything here is
held against the C restatement (OracleFold) with the same sequence and penalties: the defaults, the
all-negative set of tests/mloop2d_cases.py and a set with bp < 0 < cp.
"""
import threading

import pytest

from tests.mloop2d_cases import NEG_PEN, rseq, valid_cells
from tests.oracle_lib import HASH_NAMES, OracleFold, blob, first_difference
from tests.schedule_rows import ALL_REGIME_TARGET, ALL_REGIMES, nlev, schedule, share_range

pytestmark = pytest.mark.gpu

MIX_PEN = tuple(NEG_PEN[:10]) + (-40, 12) + tuple(NEG_PEN[12:])  # bp < 0 < cp
PENS = {"def": None, "neg": NEG_PEN, "mix": MIX_PEN}
SIX = ("PMmloop00", "PMmloop01", "PMmloop10", "POmloop00", "POmloop01", "POmloop10")

_oracles = {}
_columns = {}


def _oracle(seq, params, dangles, pen_id):
    """One restatement fold per input, shared by the tests that need it and never changed."""
    key = (seq, params, dangles, pen_id)
    if key not in _oracles:
        o = OracleFold(seq, blob(params), dangles, 0, threads=0, pen=PENS[pen_id])
        _oracles[key] = (o, o.hashes())
    return _oracles[key]


def _wf(seq, params, dangles, pen_id, **kw):
    from ccj_amd import W_final
    return W_final(seq, dangles, params=params, pen=PENS[pen_id], **kw)


def _result(wf):
    from ccj_amd import BacktrackExit
    try:
        e = wf.result()
        return ("ok", e, wf.structure, wf.stdout_msgs)
    except BacktrackExit as ex:
        return ("exit", ex.exit_code, ex.msg, ex.stdout)


def _check_hashes(wf, o, want):
    """All 31 hashes (call after _result: W is computed there)."""
    got = wf.hashes()
    assert len(want) == 31
    bad = [k for k in want if got[k] != want[k]]
    assert not bad, (bad, first_difference(wf.get4, o.get4, o.n, bad))


# ---- n = 32: all 22 matrices cell by cell and the 31 hashes, per kind of context and penalty set
SMALL = (rseq(5401, 32, "GCGCAU"), "Turner04", 2)


def _oracle_columns(pen_id):
    """The restatement's 22 matrices over every valid cell of SMALL, read once per penalty set."""
    if pen_id not in _columns:
        seq, params, d = SMALL
        o, _ = _oracle(seq, params, d, pen_id)
        cells = list(valid_cells(o.n))
        _columns[pen_id] = (cells, [[o.get4(x, *c) for c in cells] for x in range(22)])
    return _columns[pen_id]


def _check_all22_cells(wf, pen_id):
    cells, cols = _oracle_columns(pen_id)
    for x in range(22):
        diff = [(c, wf.get4(x, *c), v) for c, v in zip(cells, cols[x]) if wf.get4(x, *c) != v]
        assert not diff, f"{HASH_NAMES[x]}: {len(diff)} cells differ, first (cell, got, oracle) = {diff[0]}"


def _fold_pair(seq, params, dangles, pen_id, **kw):
    """Two ranks as their own contexts and threads over an in-process group (own blocks only, edge
    and bulk all-gathers), as tests/test_gpu_shard.py folds them."""
    from ccj_amd import LocalGroup
    g = LocalGroup(2)
    ranks = [_wf(seq, params, dangles, pen_id, shard_world=2, shard_rank=r, local_group=g, **kw) for r in range(2)]
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
    alive = [r for r, x in enumerate(th) if x.is_alive()]
    assert not alive, f"ranks {alive} did not finish their fill within 120 s (contexts left open)"
    assert not errs, errs
    return g, ranks


def test_changed_penalty_sets_make_the_six_finite_at_n32():
    """What the n = 32 checks under the negative and mixed sets are worth: each of the six matrices
    holds many values below 32767, and no two of the 22 are equal cell for cell (a slot swap shows)."""
    for pen_id in ("neg", "mix"):
        cells, cols = _oracle_columns(pen_id)
        for nm in SIX:
            assert sum(v < 32767 for v in cols[HASH_NAMES.index(nm)]) > 1000, (pen_id, nm)
        same = [(HASH_NAMES[x], HASH_NAMES[y]) for x in range(22) for y in range(x + 1, 22) if cols[x] == cols[y]]
        assert not same, (pen_id, same)


@pytest.mark.parametrize("pen_id", ["def", "neg", "mix"])
@pytest.mark.parametrize("kind", ["lean", "d4_full", "overlap_d2h", "host_traceback", "sharded2"])
def test_all_22_matrices_and_hashes_in_every_kind_of_context(kind, pen_id, monkeypatch):
    seq, params, d = SMALL
    o, want = _oracle(seq, params, d, pen_id)
    if kind == "sharded2":
        g, ranks = _fold_pair(seq, params, d, pen_id)
        try:
            res = []
            for wf in ranks:
                res.append(_result(wf))
                _check_hashes(wf, o, want)
                _check_all22_cells(wf, pen_id)
            assert res[0] == res[1]
        finally:
            for wf in ranks:
                wf.close()
            g.close()
        return
    if kind == "d4_full":
        monkeypatch.setenv("CCJ_D4_FULL", "1")  # read when the context is created: d4 keeps 22 slots
    host = kind == "host_traceback"
    wf = _wf(seq, params, d, pen_id, host_traceback=host, overlap_d2h=(kind == "overlap_d2h"))
    ref = _wf(seq, params, d, pen_id, host_traceback=not host)  # the other traceback executor
    try:
        wf.fill()
        ref.fill()
        r1, r2 = _result(wf), _result(ref)
        _check_hashes(wf, o, want)
        _check_all22_cells(wf, pen_id)
        assert r1 == r2  # structure, energy and messages: device traceback == host executor
        assert [wf.W(j) for j in range(o.n + 1)] == [o.W(j) for j in range(o.n + 1)]
    finally:
        wf.close()
        ref.close()


# ---- n = 57 .. 64: every launch regime of the level chain, and the four leaderless-boundary classes
REGIME_INPUTS = {57: (rseq(5457, 57, "ACGU"), "Turner04", 2), 64: (rseq(5464, 64, "GGCCAU"), "DirksPierce09", 1)}
BOUNDARY_N = 60
BOUNDARY_INPUT = (rseq(5460, BOUNDARY_N, "GCAU"), "Turner04", 0)


def _boundary_targets(n):
    """g_lo mod 4 -> the first split target (a multiple of 8) whose schedule shares with that class of
    g_lo > 0, from the schedule helper (the sweep tests/schedule_rows.py describes)."""
    out = {}
    for tg in range(200, 520, 8):
        g_lo, g_hi = share_range(n, tg)
        if 0 < g_lo < g_hi:
            out.setdefault(g_lo % 4, tg)
    return out


BOUNDARY = _boundary_targets(BOUNDARY_N)


def _ran(wf, n, target):
    """The context's own schedule getter: the target we passed, level by level equal to the helper."""
    assert wf.schedule_options() == (target, True)
    sch = [wf.level_schedule(t) for t in range(nlev(n))]
    assert sch == schedule(n, target)
    return {s.regime for s in sch}


def _fold_both_and_check(inp, pen_id, target, want_regimes=None, cls=None):
    seq, params, d = inp
    n = len(seq)
    o, want = _oracle(seq, params, d, pen_id)
    dev = _wf(seq, params, d, pen_id, split_target=target)
    host = _wf(seq, params, d, pen_id, split_target=target, host_traceback=True)
    try:
        for wf in (dev, host):
            got = _ran(wf, n, target)
            s = wf.level_schedule(0)
            assert 0 < s.g_lo < s.g_hi == nlev(n)
            if want_regimes is not None:
                assert got == want_regimes
            if cls is not None:
                assert s.g_lo % 4 == cls and {(1, 2), (1, 4)} <= got
        dev.fill()
        host.fill()
        rd, rh = _result(dev), _result(host)
        for wf in (dev, host):
            _check_hashes(wf, o, want)
        assert rd == rh
        assert [dev.W(j) for j in range(n + 1)] == [host.W(j) for j in range(n + 1)] == [o.W(j) for j in range(n + 1)]
    finally:
        dev.close()
        host.close()


@pytest.mark.parametrize("pen_id", ["def", "neg"])
@pytest.mark.parametrize("n", sorted(REGIME_INPUTS))
def test_every_regime_matches_oracle(n, pen_id):
    """Plain split 1, 2, 4, 8 (followers, full scans) and lead split 2, 4, 8 in one fold with g_lo > 0:
    the shrunk records and partials pass through every reduction path."""
    _fold_both_and_check(REGIME_INPUTS[n], pen_id, ALL_REGIME_TARGET[n], want_regimes=ALL_REGIMES)


def test_boundary_sweep_found_all_four_classes():
    assert sorted(BOUNDARY) == [0, 1, 2, 3]


@pytest.mark.parametrize("pen_id", ["def", "neg"])
@pytest.mark.parametrize("cls", [0, 1, 2, 3])
def test_leaderless_boundary_classes_match_oracle(cls, pen_id):
    """g_lo mod 4 = cls: which followers of levels g_lo .. g_lo+2 find no leader and scan in full."""
    _fold_both_and_check(BOUNDARY_INPUT, pen_id, BOUNDARY[cls], cls=cls)


# ---- reset: no stale table entries
def test_reset_leaves_no_stale_table_entries():
    """One context with the negative set (every table entry finite), rebound from a GC-rich sequence
    to an A-rich one (few pairs, other WB / WBP) and on to a mixed one: each fold equals the oracle's."""
    n, params, d = 40, "Turner04", 2
    seqs = [rseq(5501, n, "GCGCAU"), rseq(5502, n, "AAAAAC"), rseq(5503, n, "ACGU")]
    wf = _wf(seqs[0], params, d, "neg")
    try:
        tables = []
        for k, s in enumerate(seqs):
            if k:
                wf.reset(s)
            wf.fill()
            _result(wf)
            o, want = _oracle(s, params, d, "neg")
            _check_hashes(wf, o, want)
            tables.append(tuple(want[nm] for nm in SIX))
        assert len(set(tables)) == len(seqs)  # the folds do differ in the six matrices
    finally:
        wf.close()
