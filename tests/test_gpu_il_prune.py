"""The pruned interior-loop candidate lists change nothing the fill produces (-m gpu).

k_build_il drops the candidates that are dominated through a stacked pair (DESIGN.md §3,
ccj_amd/csrc/ccj_ilprune.h); CCJ_IL_PRUNE=0, read when a fill is enqueued, keeps the full lists.  Every
fold here runs both ways in the same kind of context and must give the same hashes of all 22 matrices
(and the 2-D ones and W), the same energy and structure or the same refusal, and the same range flags;
the device lists' kept and full counts must be those of the host form of the rule.  Sequences of
n = 40 .. 64 have u1, u2 >= 1 windows in all three roles (PL, PR, PM).
"""
import pytest

from tests.il_prune_cases import PEN_OTHER, lists, range_case, rseq

pytestmark = pytest.mark.gpu

LONG = range_case("n58_T04_d2_bp")
# name -> (sequence, parameter set, dangles, noGU, penalties, split_target)
FOLDS = {
    "T04_d2": (rseq(31, 48), "Turner04", 2, False, None, 0),
    "DP09_d0": (rseq(32, 44, "GGGCCCAU"), "DirksPierce09", 0, False, None, 0),
    "T04_d0_noGU": (rseq(33, 52), "Turner04", 0, True, None, 0),
    "DP09_d2_noGU": (rseq(34, 40, "GGCCAUU"), "DirksPierce09", 2, True, None, 0),
    "T04_d2_pen": (rseq(35, 46), "Turner04", 2, False, PEN_OTHER, 0),
    "range_pen_in": (LONG["seq"], LONG["params"], LONG["dangles"], False, tuple(LONG["pen_in"]), LONG["split_target"]),
    "range_pen_out": (LONG["seq"], LONG["params"], LONG["dangles"], False, tuple(LONG["pen_out"]), LONG["split_target"]),
}
# every fold in a plain context; one default fold, the penalty set and the range pair in the other kinds
IN_EVERY_KIND = ("T04_d2", "T04_d2_pen", "range_pen_in", "range_pen_out")
CASES = [(f, "plain") for f in FOLDS] + [(f, k) for k in ("rebind", "shard_simulate") for f in IN_EVERY_KIND]


def _kw(fold):
    _, params, _, noGU, pen, target = FOLDS[fold]
    return dict(params=params, noGU=noGU, pen=pen, split_target=target)


def _record(wf, fill=True):
    """What a fold produced: the outcome (energy and structure, the reference's exit, or the refusal),
    the range flags, the hashes, and the lists' counts."""
    from ccj_amd import BacktrackExit, RangeError
    try:
        if fill:
            wf.fill()
        outcome = ("ok", wf.result(), wf.structure)
    except BacktrackExit as ex:
        outcome = ("exit", ex.exit_code, ex.msg)
    except RangeError as ex:
        outcome = ("range", ex.flags)
    return {"outcome": outcome, "flags": wf.range_flags(), "hashes": wf.hashes(), "counts": wf.il_counts()}


def _fold(fold, kind):
    from ccj_amd import W_final
    seq, _, dangles = FOLDS[fold][:3]
    if kind == "rebind":  # a longer sequence first, in a context of capacity n + 5
        wf = W_final(seq[5:] + seq[:10], dangles, capacity=len(seq) + 5, **_kw(fold))
    elif kind == "shard_simulate":
        wf = W_final(seq, dangles, shard_world=2, shard_simulate=True, **_kw(fold))
    else:
        wf = W_final(seq, dangles, **_kw(fold))
    try:
        if kind == "rebind":
            assert wf.n == len(seq) + 5 == wf.capacity
            _record(wf)
            wf.rebind(seq)
        return _record(wf)
    finally:
        wf.close()


def _host_counts(fold, seq=None):
    s, params, dangles, noGU, pen, _ = FOLDS[fold]
    return lists(seq or s, params, dangles, pen, noGU)["counts"]


def _check_pair(on, off, want):
    """on / off: the records with the pruned and the full lists; want: the host form's counts."""
    assert on["hashes"] == off["hashes"] and len(on["hashes"]) == 31
    assert on["outcome"] == off["outcome"]
    assert on["flags"] == off["flags"]
    assert on["counts"] == want, "the device lists keep what the host form of the rule keeps"
    assert off["counts"] == (want[1], want[1], want[3], want[3]), "CCJ_IL_PRUNE=0 keeps every entry"
    assert want[0] < want[1] and want[2] < want[3], "the fold has dominated candidates in il and in ilm"


@pytest.mark.parametrize("fold,kind", CASES, ids=lambda v: v)
def test_same_fold_with_and_without_pruning(fold, kind, monkeypatch):
    monkeypatch.setenv("CCJ_IL_PRUNE", "0")
    off = _fold(fold, kind)
    monkeypatch.delenv("CCJ_IL_PRUNE")
    on = _fold(fold, kind)
    _check_pair(on, off, _host_counts(fold))
    assert (on["flags"] != 0) == (on["outcome"][0] == "range") == (fold == "range_pen_out")


@pytest.mark.parametrize("fold", IN_EVERY_KIND)
def test_lockstep_batch_of_mixed_lengths(fold, monkeypatch):
    from ccj_amd import LockstepBatch
    seq, _, dangles = FOLDS[fold][:3]
    seqs = [seq, seq[:41], seq[2:], seq[4:47][::-1]]
    assert len({len(s) for s in seqs}) == 4 and min(len(s) for s in seqs) >= 40

    def run():
        batch = LockstepBatch(len(seq), 4, dangles, **_kw(fold))
        try:
            batch.bind(seqs)
            batch.fold()
            out = []
            for wf in batch.members:
                rec = _record(wf, fill=False)
                assert (wf.refused is not None) == (rec["outcome"][0] == "range")
                out.append(rec)
            return out
        finally:
            batch.close()

    monkeypatch.setenv("CCJ_IL_PRUNE", "0")
    off = run()
    monkeypatch.delenv("CCJ_IL_PRUNE")
    on = run()
    for s, a, b in zip(seqs, on, off):
        _check_pair(a, b, _host_counts(fold, s))
    assert (on[0]["outcome"][0] == "range") == (fold == "range_pen_out")
