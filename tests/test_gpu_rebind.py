"""One context, any length up to its capacity (-m gpu): ccj_create_cap / ccj_rebind, W_final(capacity=),
W_final.rebind, fold_many and python -m ccj_amd.batch.

A rebind moves every level of every buffer, so each fold after one is held against the reference's
own run of that sequence (tests/golden/hashes.json: all 31 hashes and the MFE; tests/golden/e2e.json:
its last stdout line, or its exit code and stderr), in orders that put the shortest layouts directly
behind the longest (what a stale sentinel or descriptor would break), across sharing ranges that
move with n, with the host mirror in both of its modes, and after every refusal.
"""
import os
import random
import subprocess
import sys

import pytest

from tests.oracle_lib import ROOT, OracleFold, blob, explain_mismatch, golden
from tests.schedule_rows import ALL_REGIMES, ALL_REGIME_TARGET, nlev, schedule
from tests.test_gpu_schedule import _check_reference, _result

pytestmark = pytest.mark.gpu

HASHES = golden("hashes.json")
E2E = golden("e2e.json")


def _group(params, dangles):
    return sorted((c for c in HASHES if (c["params"], c["dangles"], c["noGU"]) == (params, dangles, 0)),
                  key=lambda c: len(c["seq"]))


def _long_short(cases):
    """Longest, shortest, second longest, second shortest, ..."""
    cases, out = list(cases), []
    while cases:
        out.append(cases.pop())
        if cases:
            out.append(cases.pop(0))
    return out


def _ctx(case, capacity, **kw):
    from ccj_amd import W_final
    return W_final(case["seq"], case["dangles"], params=case["params"], noGU=bool(case["noGU"]), capacity=capacity, **kw)


def _bound(wf, case):
    assert (wf.n, wf.seq) == (len(case["seq"]), case["seq"])
    assert wf.structure is None and wf.energy is None and wf.stdout_msgs == ""


A = _group("Turner04", 2)
B = _group("DirksPierce09", 2)


def test_fixture_groups_are_the_ones_the_orders_were_made_for():
    assert [len(c["seq"]) for c in A] == [1, 2, 3, 4, 9, 10, 12, 20, 22, 24, 24, 30, 30, 31, 32, 32, 33, 35, 42, 50, 54]
    assert [len(c["seq"]) for c in B] == [10, 14, 19, 25, 30, 32, 34, 39, 39, 40, 44, 50, 54]
    assert [len(c["seq"]) for c in _long_short(A)][:6] == [54, 1, 50, 2, 42, 3]


@pytest.mark.parametrize("cases", [A, B], ids=["Turner04-d2", "DirksPierce09-d2"])
def test_mixed_lengths_in_one_context(cases):
    """Every fixture of the group through one capacity-54 context, long and short alternating; the
    lengths without any 4-D level (n <= 2) directly behind the longest."""
    order = _long_short(cases)
    # group A is created on its longest sequence (length = capacity), group B on its shortest
    first = order[0] if cases is A else cases[0]
    wf = _ctx(first, 54)
    try:
        assert wf.capacity == 54 and wf.n == len(first["seq"])
        for k, case in enumerate(order):
            if k or case is not first:
                wf.rebind(case["seq"])
            _bound(wf, case)
            assert wf.capacity == 54
            wf.fill()
            _check_reference(wf, case)
    finally:
        wf.close()


def test_sharing_ranges_that_move_with_n():
    """Target 96: the range is empty at n = 17 and 32 and starts at level 6, 6, 3, 2, 2 at n = 37, 38,
    47, 52, 55 (read from the getter, not stated here), so the leader lists, the ring's slot size and
    the leaderless boundary move with every rebind.  n = 32 (one of the two) and n = 47 end in the
    reference's P_PR exit."""
    cases = {len(c["seq"]): [] for c in _group("Turner04", 1)}
    for c in _group("Turner04", 1):
        cases[len(c["seq"])].append(c)
    assert sorted((n, len(v)) for n, v in cases.items()) == [(17, 1), (32, 2), (37, 1), (38, 1), (47, 1), (52, 1), (55, 1)]
    order = [cases[n].pop(0) for n in (55, 17, 47, 32, 52, 37, 38, 32)]
    wf = _ctx(order[0], 55, split_target=96)
    ranges, exits = [], 0
    try:
        for k, case in enumerate(order):
            n = len(case["seq"])
            if k:
                wf.rebind(case["seq"])
            assert wf.schedule_options() == (96, True)
            sch = [wf.level_schedule(t) for t in range(nlev(n))]
            assert sch == schedule(n, 96)
            ranges.append((sch[0].g_lo, sch[0].g_hi))
            wf.fill()
            _check_reference(wf, case)
            exits += _result(wf)[0] == "exit"
    finally:
        wf.close()
    assert (0, 0) in ranges and len(set(ranges)) >= 5, ranges
    assert exits == 2


def test_all_regimes_then_none_then_all():
    target = ALL_REGIME_TARGET[54]
    assert target == 344
    by_n = {len(c["seq"]): c for c in A}
    c54, c20, c50 = by_n[54], by_n[20], by_n[50]
    wf = _ctx(c54, 54, split_target=target)
    got54 = []
    try:
        for k, case in enumerate([c54, c20, c54, c50, c54]):
            n = len(case["seq"])
            if k:
                wf.rebind(case["seq"])
            sch = [wf.level_schedule(t) for t in range(nlev(n))]
            assert sch == schedule(n, target)
            if n == 54:
                assert {s.regime for s in sch} == ALL_REGIMES and 0 < sch[0].g_lo < sch[0].g_hi == nlev(n)
            if n == 20:
                assert (sch[0].g_lo, sch[0].g_hi) == (0, 0) and not any(s.sharing for s in sch)
            wf.fill()
            _check_reference(wf, case)
            if n == 54:
                got54.append((_result(wf), wf.hashes()))
    finally:
        wf.close()
    assert len(got54) == 3 and got54[0] == got54[1] == got54[2]


def _rseq(seed, n, alphabet):
    r = random.Random(seed)
    return "".join(r.choice(alphabet) for _ in range(n))


SEQ62 = {"seq": _rseq(6262, 62, "GGCCAU"), "params": "Turner04", "dangles": 2, "noGU": 0}


@pytest.fixture(scope="module")
def oracle62():
    """The C restatement's fold of the GC-rich n = 62 sequence: its hashes and W(n), computed once."""
    o = OracleFold(SEQ62["seq"], blob("Turner04"), 2, 0)
    try:
        return o.hashes(), o.W(62)
    finally:
        o.close()


@pytest.mark.parametrize("alphabet,n", [("AAAAUC", 45), ("AAAUGC", 41), ("GGCCAU", 27)])
def test_sparse_folds_behind_a_dense_fold_match_oracle(alphabet, n):
    """Sequences in which few pairs can form, bound directly behind the dense n = 62 fold: most of
    their cells stay at the never-set 32767, which a stale finite value met through a null list entry
    or a sentinel pad would undercut.  Against the C restatement."""
    case = dict(SEQ62, seq=_rseq(4100 + n, n, alphabet))
    wf = _ctx(SEQ62, 62)
    o = OracleFold(case["seq"], blob("Turner04"), 2, 0)
    try:
        wf.fill()
        _result(wf)
        wf.rebind(case["seq"])
        wf.fill()
        _result(wf)
        got, want = wf.hashes(), o.hashes()
        bad = [x for x in want if got[x] != want[x]]
        assert not bad, explain_mismatch(wf, case["seq"], "Turner04", 2, 0, bad)
        assert [wf.W(j) for j in range(n + 1)] == [o.W(j) for j in range(n + 1)]
    finally:
        wf.close()
        o.close()


@pytest.mark.parametrize("target", [0, 96], ids=["default-target", "target96"])
def test_no_stale_state_behind_a_dense_fold(target, oracle62):
    """A GC-rich n = 62 fold writes many cells of the interior-loop copies; the n = 33 and n = 12
    layouts then lie inside what it wrote, and the n = 62 layout again over theirs.  Every fold equals
    the reference fixture (n = 33, 12) or the oracle (n = 62), and a fresh context of its length:
    hashes, energy, structure and side messages."""
    by_n = {len(c["seq"]): c for c in A}
    want_h, want_w = oracle62
    wf = _ctx(SEQ62, 62, split_target=target)
    try:
        for k, case in enumerate([SEQ62, by_n[33], by_n[12], SEQ62]):
            n = len(case["seq"])
            if k:
                wf.rebind(case["seq"])
            wf.fill()
            if case is SEQ62:
                res, got = _result(wf), wf.hashes()
                bad = [x for x in want_h if got[x] != want_h[x]]
                assert not bad, explain_mismatch(wf, case["seq"], "Turner04", 2, 0, bad)
                assert wf.W(n) == want_w
            else:
                _check_reference(wf, case)
                res, got = _result(wf), wf.hashes()
            fresh = _ctx(case, None, split_target=target)
            try:
                assert fresh.capacity == n
                fresh.fill()
                assert _result(fresh) == res
                assert fresh.hashes() == got
            finally:
                fresh.close()
    finally:
        wf.close()


@pytest.mark.parametrize("mode", [dict(host_traceback=True), dict(overlap_d2h=True),
                                  dict(host_traceback=True, overlap_d2h=True)],
                         ids=["host-traceback", "overlap-d2h", "host-traceback-overlap-d2h"])
def test_mirror_modes_follow_the_binding(mode):
    """The pinned host mirror is allocated once for the capacity; its level offsets follow the bound n."""
    order = _long_short(A)[:6]
    wf = _ctx(order[0], 54, **mode)
    try:
        for k, case in enumerate(order):
            if k:
                wf.rebind(case["seq"])
            wf.fill()
            _check_reference(wf, case)
    finally:
        wf.close()


def test_refusals_leave_the_binding_usable():
    from ccj_amd import CCJ_E_ARG, CCJ_E_STATE, CCJError, W_final
    by_n = {len(c["seq"]): c for c in A}
    case = by_n[35]
    wf = _ctx(case, 42)

    def still_folds():
        assert (wf.n, wf.seq, wf.capacity) == (35, case["seq"], 42)
        wf.fill()
        _check_reference(wf, case)

    try:
        still_folds()
        with pytest.raises(CCJError) as e:
            wf.rebind(by_n[50]["seq"])  # beyond the capacity
        assert e.value.code == CCJ_E_ARG
        still_folds()
        with pytest.raises(CCJError) as e:
            wf.rebind("ACGUX" * 6)  # a character outside ACGUT
        assert e.value.code == CCJ_E_ARG
        still_folds()
        wf.fill_async()
        with pytest.raises(CCJError) as e:
            wf.rebind(by_n[20]["seq"])  # a fold is in flight
        assert e.value.code == CCJ_E_STATE
        wf.wait()
        still_folds()
        with pytest.raises(CCJError):
            wf.reset(by_n[20]["seq"])  # reset keeps refusing another length
        still_folds()
        wf.rebind(by_n[20]["seq"])  # and the same rebind is fine once nothing is in flight
        wf.fill()
        _check_reference(wf, by_n[20])
    finally:
        wf.close()
    with pytest.raises(CCJError) as e:
        W_final(case["seq"], 2, params="Turner04", capacity=34)  # a sequence longer than the capacity
    assert e.value.code == CCJ_E_ARG
    for simulate in (True, False):
        with pytest.raises(CCJError) as e:
            W_final(case["seq"], 2, params="Turner04", capacity=42, shard_world=2, shard_simulate=simulate)
        assert e.value.code == CCJ_E_ARG
    # a band-sharded context of capacity = length exists as before, and holds its one length
    sh = W_final(case["seq"], 2, params="Turner04", capacity=35, shard_world=2, shard_simulate=True)
    try:
        with pytest.raises(CCJError) as e:
            sh.rebind(by_n[20]["seq"])
        assert e.value.code == CCJ_E_ARG
        sh.fill()
        _check_reference(sh, case, world=2)
    finally:
        sh.close()


T1 = [c for c in E2E if (c["params"], c["dangles"], c["noGU"]) == ("Turner04", 1, 0)]


def _shuffled():
    cases = list(T1)
    random.Random(7).shuffle(cases)
    return cases


def test_e2e_cases_are_the_ten_the_batch_tests_expect():
    assert sorted(len(c["seq"]) for c in T1) == [17, 32, 32, 37, 38, 47, 52, 55, 62, 62]
    assert sorted(c["rc"] for c in T1) == [0] * 8 + [1, 1]


@pytest.mark.parametrize("contexts", [1, 2, 3])
def test_fold_many_matches_the_reference_runs(contexts):
    from ccj_amd import fold_many
    from ccj_amd.batch import record_stdout
    cases = _shuffled()
    recs = fold_many([c["seq"] for c in cases], 1, params="Turner04", contexts=contexts)
    assert len(recs) == len(cases)
    for rec, c in zip(recs, cases):
        assert rec[0] == c["seq"]
        assert (rec[4], record_stdout(rec), rec[5]) == (c["rc"], c["stdout"], c["stderr"])
        assert (rec[1] is None) == (c["rc"] != 0)


def test_batch_module_prints_what_the_command_line_prints(tmp_path):
    cases = _shuffled()
    f = tmp_path / "seqs.txt"
    # one per line, lower case and DNA letters in places: upper-cased, T -> U like the command line
    f.write_text("".join((c["seq"].lower().replace("u", "t") if k % 2 else c["seq"]) + "\n" for k, c in enumerate(cases)))
    p = subprocess.run([sys.executable, "-m", "ccj_amd.batch", "-d", "1", "-P", "Turner04", "--contexts", "2", str(f)],
                       cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=120)
    assert p.stdout == "".join(c["stdout"] for c in cases)
    assert p.stderr == "".join(c["stderr"] for c in cases)
    assert p.returncode == 1
    # the same records as FASTA, sequences wrapped over lines
    g = tmp_path / "seqs.fa"
    g.write_text("".join(f">s{k}\n{c['seq'][:20]}\n{c['seq'][20:]}\n" for k, c in enumerate(cases[:3])))
    from ccj_amd.batch import read_sequences
    with open(g) as fh:
        assert read_sequences(fh) == [c["seq"] for c in cases[:3]]
