"""The Python face of constrained folding, without a GPU: ccj_amd.Constraint (parsing and the defects
it refuses, the same ones the ABI refuses with CCJ_E_ARG), the host entry points that take a
ccj_constraint, and the --constraints grammar of python -m ccj_amd.batch."""
import ctypes
import io

import pytest

import ccj_amd
from ccj_amd import CCJ_E_ARG, CCJError, Constraint
from ccj_amd import batch as batch_tool
from tests.oracle_lib import blob


def test_string_form():
    c = Constraint.parse("..x..x\n")
    assert c.unpaired == "..x..x" and c.forbid == () and c.allow_only is None
    assert c.forbidden(6) == {(1, 3), (2, 3), (3, 4), (3, 5), (3, 6), (1, 6), (2, 6), (4, 6), (5, 6)}
    assert Constraint("......").forbidden(6) == set()


def test_lists_and_the_order_of_the_three_parts():
    c = Constraint(unpaired="x....", forbid=[(2, 4)], allow_only=[(1, 5), (2, 4), (2, 5)])
    # allow-only first (the complement), then x and forbid on top
    assert c.forbidden(5) == {(i, j) for i in range(1, 6) for j in range(i + 1, 6)} - {(2, 5)}
    assert Constraint(allow_only=[]).forbidden(3) == {(1, 2), (1, 3), (2, 3)}
    assert Constraint(forbid=[[1, 4]]).forbid == ((1, 4),)
    assert "forbid=[(1, 4)]" in repr(Constraint(forbid=[(1, 4)]))


@pytest.mark.parametrize("kw", [dict(unpaired="..(.."), dict(unpaired="..X.."), dict(unpaired=5), dict(forbid=[(3, 3)]),
                                dict(forbid=[(4, 2)]), dict(forbid=[(0, 2)]), dict(forbid=[(1,)]), dict(forbid=[(1.5, 3)]),
                                dict(allow_only=[(2, 1)]), dict(forbid=["ab"])])
def test_defects_refused_at_construction(kw):
    with pytest.raises(CCJError) as ei:
        Constraint(**kw)
    assert ei.value.code == CCJ_E_ARG


@pytest.mark.parametrize("c", [Constraint("...."), Constraint("......"), Constraint(forbid=[(2, 6)]), Constraint(allow_only=[(1, 9)])])
def test_defects_refused_against_a_length(c):
    with pytest.raises(CCJError) as ei:
        c.check(5)
    assert ei.value.code == CCJ_E_ARG
    with pytest.raises(CCJError):
        ccj_amd.il_prune_host("GGGAC", "Turner04", windows=False, constraint=c)


def test_code_attribute_exists():
    assert CCJError(CCJ_E_ARG, "x").code == CCJ_E_ARG


def _raw(unpaired=None, forbid=(), allow_only=None, n_forbid=None):
    fb = (ctypes.c_int * max(1, 2 * len(forbid)))(*[v for p in forbid for v in p])
    ao = None if allow_only is None else (ctypes.c_int * max(1, 2 * len(allow_only)))(*[v for p in allow_only for v in p])
    c = ccj_amd._Constraint(unpaired.encode() if unpaired is not None else None, ctypes.cast(fb, ctypes.POINTER(ctypes.c_int)),
                            len(forbid) if n_forbid is None else n_forbid,
                            ctypes.cast(ao, ctypes.POINTER(ctypes.c_int)) if ao is not None else None,
                            0 if allow_only is None else len(allow_only))
    return c, (fb, ao)


def test_the_abi_refuses_the_same_defects():
    """ccj_work_model_seq_constrained runs the ABI's own check of a ccj_constraint (no GPU, no context)."""
    L = ccj_amd.lib()
    seq, n = b"GGGAAAUCCC", 10
    out = (ctypes.c_double * 4)()
    plain = (ctypes.c_double * 4)()
    assert L.ccj_work_model_seq_constrained(seq, 0, None, plain) == 0
    ok, _k = _raw(unpaired="." * n)
    assert L.ccj_work_model_seq_constrained(seq, 0, ctypes.byref(ok), out) == 0 and list(out) == list(plain)
    for kw in (dict(unpaired="." * 9), dict(unpaired="." * 11), dict(unpaired="....(....."), dict(forbid=[(4, 4)]),
               dict(forbid=[(6, 2)]), dict(forbid=[(0, 3)]), dict(forbid=[(1, 11)]), dict(allow_only=[(3, 12)]),
               dict(forbid=[(1, 5)], n_forbid=-1)):
        bad, _k = _raw(**kw)
        assert L.ccj_work_model_seq_constrained(seq, 0, ctypes.byref(bad), out) == CCJ_E_ARG, kw
    # a forbidden pair takes its interior-loop candidates out of the model; one that cannot pair changes nothing
    fb, _k = _raw(forbid=[(1, 10), (2, 9), (3, 8)])
    assert L.ccj_work_model_seq_constrained(seq, 0, ctypes.byref(fb), out) == 0 and out[2] < plain[2]
    aa, _k = _raw(forbid=[(4, 6)])
    assert L.ccj_work_model_seq_constrained(seq, 0, ctypes.byref(aa), out) == 0 and list(out) == list(plain)


def test_the_host_rule_under_a_constraint_has_no_list_for_a_forbidden_pair():
    seq = "GGGGAAAACCCCAAAAGGGGAAAACCCC"
    plain = ccj_amd.il_prune_host(seq, blob("Turner04"))
    cons = ccj_amd.il_prune_host(seq, blob("Turner04"), constraint=Constraint(forbid=[(1, 12)]))
    w, p = 11, 1
    assert plain["st_il"][w, p].any() and not cons["st_il"][w, p].any()
    assert cons["ie"][w, p] == 32767 and cons["ie"][w - 2, p + 1] == plain["ie"][w - 2, p + 1] != 32767
    assert cons["counts"][1] < plain["counts"][1]
    # and as a candidate of the pairs around it: (1, 12) sits in no window
    for ww in range(len(seq)):
        for pp in range(1, len(seq) - ww + 1):
            for u1, u2 in zip(*cons["st_ilm"][ww, pp].nonzero()):
                assert (pp - 1 - u1, pp + ww + 1 + u2) != (1, 12)
    empty = ccj_amd.il_prune_host(seq, blob("Turner04"), constraint=Constraint("." * len(seq)))
    assert empty["counts"] == plain["counts"] and (empty["st_il"] == plain["st_il"]).all()


# ---- python -m ccj_amd.batch --constraints ---------------------------------------------------------

def test_grammar_one_sequence_per_line():
    recs = batch_tool.read_records(["acgu\n", "..x.\n", "\n", "GGGT\n", "CCCC\n", "xx..\n"])
    assert recs == [("ACGU", "..x."), ("GGGU", None), ("CCCC", "xx..")]


def test_grammar_fasta():
    recs = batch_tool.read_records([">a\n", "ACG\n", "UUU\n", "x.....\n", ">b\n", "AAA\n", ">c\n", "GG\n", "..\n", "..\n"])
    assert recs == [("ACGUUU", "x....."), ("AAA", None), ("GG", ".."), ("", "..")]


def test_grammar_orphan_lines():
    assert batch_tool.read_records(["..x\n", "ACGU\n"]) == [("", "..x"), ("ACGU", None)]
    assert batch_tool.read_records(["ACGU\n", "....\n", "x...\n"]) == [("ACGU", "...."), ("", "x...")]


def test_without_the_flag_the_grammar_is_unchanged():
    assert batch_tool.read_sequences(["acgu\n", ">x\n", "GG\n", "CC\n"]) == ["ACGU", "GGCC"]
    assert batch_tool.read_sequences(["ACGU\n", "..x.\n"]) == ["ACGU", "..X."]


def test_bad_constraint_lines_are_reported_and_not_folded(tmp_path, monkeypatch):
    seen = {}

    def fake_fold_many(seqs, *a, **kw):
        seen["seqs"], seen["constraints"] = list(seqs), kw.get("constraints")
        return [(s, "." * len(s), 0.0, "", 0, "") for s in seqs]

    monkeypatch.setattr(batch_tool, "fold_many", fake_fold_many)
    f = tmp_path / "in.txt"
    f.write_text("ACGU\n..x.\nGGGG\n...\nCCCC\nAXGU\n")
    out, err = io.StringIO(), io.StringIO()
    code = batch_tool.run(["--constraints", "-P", "Turner04", str(f)], stdout=out, stderr=err)
    assert code == 1
    assert seen["seqs"] == ["ACGU", "CCCC"] and seen["constraints"] == ["..x.", None]
    assert "Constraint line of length 3 for a sequence of length 4." in err.getvalue()
    assert out.getvalue() == "ACGU\n.... (0)\nCCCC\n.... (0)\nSequence contains character X that is not G,C,A,U, or T.\n"
    # no constraint line at all: fold_many gets None, as without the flag
    f.write_text("ACGU\nGGGG\n")
    assert batch_tool.run(["--constraints", "-P", "Turner04", str(f)], stdout=io.StringIO(), stderr=io.StringIO()) == 0
    assert seen["constraints"] is None
