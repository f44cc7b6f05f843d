"""Reset, rebind and lockstep folds under non-default pseudoknot penalties (-m gpu): the folds of
tests/pen_companions.py (strongly negative bp, e_stP / e_intP overrides) through ccj_reset, ccj_rebind at
capacity n and n + 5, LockstepBatch, fold_many on both of its paths, and two penalty sets alive at once.

Under the default penalties the twelve table-carried matrices (PL / PR mloop00/01/10 in the int16 tables,
PM / PO mloop00/01/10 as closed forms of the int32 tables) are almost everywhere 32767 and no traceback
enters a P_P?mloop*, P_WB or P_WBP node, so a stale table entry behind a reset or rebind, a member reading
another member's tables, or a batched k_diag2d launch that loses a member's table workgroups rarely
changes a hash and never a structure.  Here those matrices are dense (tests/test_pen_companions.py), and
every binding is followed by another of the same or a smaller length with other values in them.

One fold is one (case, sequence), checked the same way everywhere (_check_fold):

  * all 31 hashes and W(n): the reference's own for the case's sequence, the C restatement's under the
    case's penalties for a companion; on a mismatch the first differing cell against the restatement;
  * the traceback: for the case's sequence the reference's (rc, stdout, stderr); for a companion the
    outcome of a fresh plain context with host_traceback=True and the same penalties.

For companions the traceback is therefore engine against engine, across two storage paths (the device
executor over DevStore's tables and closed forms in a rebound or batched layout, against the host executor
over the expanded mirror of a fresh one).  What pins the node logic against the reference is the fixture
sequence folded in the same context or batch, before and after its companions.
"""
import random

import pytest

from tests.lockstep_rows import TARGET_SPLITS, option, splits
from tests.mloop2d_cases import valid_cells
from tests.oracle_lib import HASH_NAMES, first_difference, golden
from tests.pen_companions import (CASES, MLOOP_CASES, OWN, PAIR_CASES, SMALLEST, SPLIT_CASE, case_id, expected, oracle,
                                  sequences)
from tests.test_gpu_schedule import _check_reference
from tests.test_gpu_traceback_mloop_cases import _output

pytestmark = pytest.mark.gpu

REBIND_ORDER = (OWN, "head7", "tail2", "mid", OWN, "head3")  # dense first, shorter layouts inside it, back
RESET_ORDER = (OWN, "reverse", "shuffle", OWN)
EXIT_CASE = next(c for c in MLOOP_CASES if c["rc"] == 1 and len(c["seq"]) == 32)
MANY_CASES = [next(c for c in MLOOP_CASES if c["rc"] == rc and len(c["seq"]) >= 30) for rc in (0, 1)]

_fresh_outputs = {}
_columns = {}


def _kw(case):
    return dict(params=case["params"], noGU=bool(case["noGU"]), pen=tuple(case["pen"]))


def _ctx(case, seq, **kw):
    from ccj_amd import W_final
    return W_final(seq, case["dangles"], **_kw(case), **kw)


def _batch(case, capacity, members, **kw):
    from ccj_amd import LockstepBatch
    return LockstepBatch(capacity, members, case["dangles"], **_kw(case), **kw)


def _fresh_output(case, name):
    """(rc, stdout, stderr) of a fresh plain context's host traceback of the companion; once per process."""
    key = (case_id(case), name)
    if key not in _fresh_outputs:
        from ccj_amd.cli import fold_cli
        _fresh_outputs[key] = fold_cli(sequences(case)[name], case["params"], case["dangles"], bool(case["noGU"]),
                                       pen=tuple(case["pen"]), host_traceback=True)
    return _fresh_outputs[key]


def _check_cells(wf, case, name):
    """All 22 matrices of the folded context cell by cell against the restatement (the two smallest
    cases: n <= 18)."""
    key = (case_id(case), name)
    if key not in _columns:
        o = oracle(case, sequences(case)[name])
        try:
            cells = list(valid_cells(o.n))
            _columns[key] = (cells, [[o.get4(x, *c) for c in cells] for x in range(22)])
        finally:
            o.close()
    cells, cols = _columns[key]
    for x in range(22):
        diff = [(c, wf.get4(x, *c), v) for c, v in zip(cells, cols[x]) if wf.get4(x, *c) != v]
        assert not diff, f"{HASH_NAMES[x]} of {name}: {len(diff)} cells differ, first (cell, got, oracle) = {diff[0]}"


def _check_fold(wf, case, name, cells=False):
    want = expected(case, name)
    seq = want["seq"]
    assert (wf.n, wf.seq) == (len(seq), seq)
    out = _output(wf, want)  # W is computed here, before any backtrack exit of the reference's
    got = wf.hashes()
    bad = [k for k in want["hashes"] if got[k] != want["hashes"][k]]
    if bad:
        o = oracle(case, seq)
        try:
            where = first_difference(wf.get4, o.get4, o.n, bad)
        finally:
            o.close()
        assert not bad, f"{name}: matrices differ: {bad}; first 4-D difference against the restatement: {where}"
    assert len(want["hashes"]) == 31 and wf.W(len(seq)) == want["mfe"], name
    if cells:
        _check_cells(wf, case, name)
    assert out == (want["output"] if name == OWN else _fresh_output(case, name)), name
    return out


# ---- reset: other values in the same dense tables
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_reset_to_sequences_of_the_same_length(case):
    seqs = sequences(case)
    order = [k for k in RESET_ORDER if k in seqs]
    wf = _ctx(case, seqs[OWN])
    try:
        for k, name in enumerate(order):
            if k:
                wf.reset(seqs[name])
            wf.fill()
            _check_fold(wf, case, name)
    finally:
        wf.close()


# ---- rebind: capacity n and n + 5
def _rebind_sequence(case, extra, cells=False, **mode):
    seqs = sequences(case)
    order = [k for k in REBIND_ORDER if k in seqs]
    n = len(seqs[OWN])
    wf = _ctx(case, seqs[OWN], capacity=n + extra, **mode)
    try:
        assert wf.capacity == n + extra
        for k, name in enumerate(order):
            if k:
                wf.rebind(seqs[name])
            wf.fill()
            _check_fold(wf, case, name, cells)
            assert wf.capacity == n + extra
    finally:
        wf.close()


@pytest.mark.parametrize("extra", [0, 5], ids=["cap-n", "cap-n+5"])
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_rebind_to_shorter_layouts_and_back(case, extra):
    _rebind_sequence(case, extra)


@pytest.mark.parametrize("mode", [dict(), dict(host_traceback=True), dict(overlap_d2h=True)],
                         ids=["device", "host-traceback", "overlap-d2h"])
@pytest.mark.parametrize("extra", [0, 5], ids=["cap-n", "cap-n+5"])
@pytest.mark.parametrize("case", SMALLEST, ids=case_id)
def test_rebind_mirror_follows_the_binding_cell_by_cell(case, extra, mode):
    """After every binding all 22 matrices through get4: the mirror behind k_expand (which writes the
    twelve table-carried slots out), whose level offsets follow the bound n."""
    _rebind_sequence(case, extra, cells=True, **mode)


# ---- lockstep
def _fold_members(batch, folds, cells=()):
    """Bind the batch to folds = [(case, name)], fold, check every member; cells: member indices that
    also get the cell-by-cell check.  Returns each member's (rc, stdout, stderr)."""
    batch.bind([sequences(c)[name] for c, name in folds])
    assert batch.count == len(folds) == len(batch.members)
    batch.fold()
    outs = []
    for k, (wf, (case, name)) in enumerate(zip(batch.members, folds)):
        outs.append(_check_fold(wf, case, name, cells=k in cells))
        assert (wf.exit is not None) == (wf.structure is None) == (outs[-1][0] != 0)
    print("members (sequence, exit code):", [(name, o[0]) for (_, name), o in zip(folds, outs)])
    return outs


def _three_rounds(batch, folds, cells=()):
    """All members; then the three shortest alone (the others idle); then all in reverse order."""
    first = _fold_members(batch, folds, cells)
    short = sorted(folds, key=lambda f: len(sequences(f[0])[f[1]]))[:3]
    _fold_members(batch, short, [k for k in cells if k < 3])
    assert batch.count == 3 < batch.size
    back = _fold_members(batch, folds[::-1], cells)
    assert back == first[::-1]
    return first


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_lockstep_batch_of_a_case_and_its_companions(case):
    folds = [(case, name) for name in sequences(case)]
    batch = _batch(case, len(case["seq"]), 7)
    try:
        _three_rounds(batch, folds, cells=(0, len(folds) - 1) if case in SMALLEST else ())
    finally:
        batch.close()


def test_lockstep_batch_of_two_reference_pinned_sequences():
    """The two CaoChen06 d1 cases share one penalty set: both fixtures and their companions in one batch."""
    a, b = PAIR_CASES
    assert a["pen"] == b["pen"] and (a["params"], a["dangles"], a["noGU"]) == (b["params"], b["dangles"], b["noGU"])
    folds = [f for pair in zip([(a, k) for k in sequences(a)], [(b, k) for k in sequences(b)]) for f in pair]
    assert len(folds) == len(sequences(a)) + len(sequences(b)) >= 12
    batch = _batch(a, 49, len(folds))
    try:
        _three_rounds(batch, folds)
    finally:
        batch.close()


def test_lockstep_reference_exit_beside_members_that_end_normally():
    case = EXIT_CASE
    assert case["rc"] == 1 and "P_PM" in case["stderr"]
    folds = [(case, name) for name in sequences(case)]
    batch = _batch(case, len(case["seq"]), 7)
    try:
        outs = _fold_members(batch, folds)
        assert outs[0] == (1, case["stdout"], case["stderr"])
        assert batch.members[0].exit is not None and "P_PM" in batch.members[0].exit.msg
        ended = [rc for rc, _, _ in outs]
        assert 1 in ended and 0 in ended, ended
    finally:
        batch.close()


def _split_lengths():
    return [len(s) for s in sequences(SPLIT_CASE).values()]


def test_split_case_reaches_every_split():
    lengths = _split_lengths()
    assert 57 <= max(lengths) <= 59
    assert set().union(*(splits(lengths, target) for target in TARGET_SPLITS)) == {1, 2, 4, 8}


@pytest.mark.parametrize("target", sorted(TARGET_SPLITS))
def test_lockstep_under_every_split_target(target):
    case = SPLIT_CASE
    folds = [(case, name) for name in sequences(case)]
    batch = _batch(case, len(case["seq"]), 7, split_target=option(target))
    try:
        assert batch._all[0].schedule_options() == (target, False)
        _fold_members(batch, folds)
    finally:
        batch.close()


# ---- fold_many, both paths
@pytest.mark.parametrize("case", MANY_CASES, ids=case_id)
def test_fold_many_passes_the_penalties_on_both_paths(case):
    from ccj_amd import fold_many
    from ccj_amd.batch import record_stdout
    names = list(sequences(case))
    random.Random(7).shuffle(names)
    seqs = [sequences(case)[k] for k in names]
    plain = fold_many(seqs, case["dangles"], contexts=2, **_kw(case))
    lock = fold_many(seqs, case["dangles"], lockstep=4, **_kw(case))
    assert [r[0] for r in plain] == seqs
    assert lock == plain
    for rec, name in zip(plain, names):
        got = (rec[4], record_stdout(rec), rec[5])
        assert got == (expected(case, name)["output"] if name == OWN else _fresh_output(case, name)), name
        assert (rec[1] is None) == (rec[4] != 0)


# ---- two penalty sets alive at once
def test_two_penalty_sets_alive_at_once():
    """A default-penalty capacity context and a bp < 0 batch, folded alternately and bound again: each
    keeps its own penalty tables (est, ie and the list energies are rebuilt per binding and per member)."""
    case = MANY_CASES[0]
    assert case["params"] == "Turner04" and case["pen"][10] < 0
    by_n = {len(c["seq"]): c for c in golden("hashes.json")
            if (c["params"], c["dangles"], c["noGU"]) == ("Turner04", 2, 0)}
    d33, d20 = by_n[33], by_n[20]
    folds = [(case, name) for name in sequences(case)]
    from ccj_amd import W_final
    wf = W_final(d33["seq"], 2, params="Turner04", capacity=40)
    batch = _batch(case, len(case["seq"]), 7)
    try:
        wf.fill()
        _check_reference(wf, d33)
        _fold_members(batch, folds)
        wf.rebind(d20["seq"])
        wf.fill()
        _check_reference(wf, d20)
        _fold_members(batch, folds[::-1][:4])
        wf.rebind(d33["seq"])
        wf.fill()
        _check_reference(wf, d33)
        _fold_members(batch, folds)
    finally:
        batch.close()
        wf.close()
