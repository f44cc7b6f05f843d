"""The PL / PR multiloop families as 2-D tables (ccj_amd/csrc/ccj_mloop2d.h), on the GPU (-m gpu).

The level kernels no longer compute PLmloop00/01/10 and PRmloop00/01/10 per cell: k_diag2d fills
six tables, PL / PR read them, and every reader of the six matrices (get4, the hashes, the host
mirror, the device traceback) is served from the tables.  Everything here is held against the C
restatement (OracleFold) with the same sequence and penalties: the default ones and a set with
negative PSM, PPS, ap, bp and cp (tests/mloop2d_cases.py), under which the six families, the PM / PO
families and PL / PR are finite, so the shrunk loop records and leader partials carry real values.

Each of the 22 matrices has one carrier (d4, the loop records, the tables: ccj_engine.h carrier), and
the host mirror get4 reads is put together from all three: one test reads all 22 cell by cell, in
every kind of context.
"""
import threading

import pytest

from tests.mloop2d_cases import FAMILY_L, FAMILY_R, NEG_PEN, rseq, valid_cells
from tests.oracle_lib import HASH_NAMES, OracleFold, blob, first_difference
from tests.schedule_rows import ALL_REGIME_TARGET, ALL_REGIMES, nlev, schedule, share_range

pytestmark = pytest.mark.gpu

PENS = {"def": None, "neg": NEG_PEN}
SIX = FAMILY_L + FAMILY_R

_oracles = {}


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


def _check_six_cells(wf, o):
    n = o.n
    for nm in SIX:
        x = HASH_NAMES.index(nm)
        pairs = ((c, wf.get4(x, *c), o.get4(x, *c)) for c in valid_cells(n))
        diff = [p for p in pairs if p[1] != p[2]]
        assert not diff, f"{nm}: {len(diff)} cells differ, first (cell, got, oracle) = {diff[0]}"


# ---- n = 32: every cell of the six matrices through get4, and the 31 hashes, per kind of context
SMALL = (rseq(5201, 32, "GCGCAU"), "Turner04", 2)


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


@pytest.mark.parametrize("pen_id", ["def", "neg"])
@pytest.mark.parametrize("kind", ["default", "d4_full", "host_traceback", "sharded2"])
def test_six_matrices_and_hashes_in_every_kind_of_context(kind, pen_id, monkeypatch):
    seq, params, d = SMALL
    o, want = _oracle(seq, params, d, pen_id)
    if kind == "sharded2":
        g, ranks = _fold_pair(seq, params, d, pen_id)
        try:
            for wf in ranks:
                _result(wf)
                _check_hashes(wf, o, want)
                _check_six_cells(wf, o)
        finally:
            for wf in ranks:
                wf.close()
            g.close()
        return
    if kind == "d4_full":
        monkeypatch.setenv("CCJ_D4_FULL", "1")  # read when the context is created: d4 keeps 22 slots
    wf = _wf(seq, params, d, pen_id, host_traceback=(kind == "host_traceback"))
    ref = _wf(seq, params, d, pen_id, host_traceback=(kind != "host_traceback"))  # the other executor
    try:
        wf.fill()
        ref.fill()
        r1, r2 = _result(wf), _result(ref)
        _check_hashes(wf, o, want)
        _check_six_cells(wf, o)
        assert r1 == r2  # structure, energy and messages: device traceback == host executor
        assert [wf.W(j) for j in range(o.n + 1)] == [o.W(j) for j in range(o.n + 1)]
    finally:
        wf.close()
        ref.close()


def test_negative_set_makes_the_families_finite_at_n32():
    """What the n = 32 checks under the negative set are worth: each of the six matrices, and PM / PO
    multiloop values the records and partials carry, hold many values below 32767."""
    seq, params, d = SMALL
    o, _ = _oracle(seq, params, d, "neg")
    for nm in SIX + ("PMmloop00", "PMmloop10", "POmloop00", "POmloop10", "PL", "PR"):
        x = HASH_NAMES.index(nm)
        assert sum(o.get4(x, *c) < 32767 for c in valid_cells(o.n)) > 1000, nm


# ---- n = 32: every cell of all 22 matrices through the host mirror, per kind of context
_all22 = {}


def _oracle_all22():
    """The restatement's 22 matrices over every valid cell of SMALL under the negative set, read once.
    The slot order of a level (ccj_engine.h mslot) decides where get4 finds a matrix in the mirror, and
    a swap of two slots can hide only between matrices that are equal cell for cell: so first, on
    the restatement alone, every matrix holds many finite values and no two are equal."""
    if not _all22:
        seq, params, d = SMALL
        o, _ = _oracle(seq, params, d, "neg")
        cells = list(valid_cells(o.n))
        cols = [[o.get4(x, *c) for c in cells] for x in range(22)]
        for x in range(22):
            assert sum(v < 32767 for v in cols[x]) > 1000, HASH_NAMES[x]
        same = [(HASH_NAMES[x], HASH_NAMES[y]) for x in range(22) for y in range(x + 1, 22) if cols[x] == cols[y]]
        assert not same, same
        _all22["cells"], _all22["cols"] = cells, cols
    return _all22["cells"], _all22["cols"]


def _check_all22_cells(wf):
    cells, cols = _oracle_all22()
    for x in range(22):
        diff = [(c, wf.get4(x, *c), v) for c, v in zip(cells, cols[x]) if wf.get4(x, *c) != v]
        assert not diff, f"{HASH_NAMES[x]}: {len(diff)} cells differ, first (cell, got, oracle) = {diff[0]}"


@pytest.mark.parametrize("kind", ["lean", "d4_full", "overlap_d2h", "sharded2"])
def test_all_22_matrices_cell_by_cell_through_the_host_mirror(kind, monkeypatch):
    """get4 reads the host mirror (cell_offset_host).  A lean context copies 8 slots per level from
    d4 and 14 written out from the records and tables; a full one (the switch, a mirror streamed
    during the fill, each rank of a band-sharded pair) copies d4's 22."""
    _oracle_all22()
    seq, params, d = SMALL
    if kind == "sharded2":
        g, ranks = _fold_pair(seq, params, d, "neg")
        try:
            for wf in ranks:
                _check_all22_cells(wf)
        finally:
            for wf in ranks:
                wf.close()
            g.close()
        return
    if kind == "d4_full":
        monkeypatch.setenv("CCJ_D4_FULL", "1")  # read when the context is created
    wf = _wf(seq, params, d, "neg", overlap_d2h=(kind == "overlap_d2h"))
    try:
        wf.fill()
        _check_all22_cells(wf)
    finally:
        wf.close()


# ---- n = 57 .. 64: every launch regime of the level chain, and the four leaderless-boundary classes
REGIME_INPUTS = {57: (rseq(5257, 57, "ACGU"), "Turner04", 2), 64: (rseq(5264, 64, "GGCCAU"), "DirksPierce09", 1)}
BOUNDARY_N = 60
BOUNDARY_INPUT = (rseq(5260, BOUNDARY_N, "GCAU"), "Turner04", 0)


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
    """Plain split 1, 2, 4, 8 (followers, full scans) and lead split 2, 4, 8 in one fold with g_lo > 0."""
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
    to an A-rich one (few pairs, other WB / WBP) and back to a mixed one: each fold equals the oracle's."""
    n, params, d = 40, "Turner04", 2
    seqs = [rseq(5301, n, "GCGCAU"), rseq(5302, n, "AAAAAC"), rseq(5303, n, "ACGU")]
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
