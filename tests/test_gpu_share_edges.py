"""Split-point sharing in the gap columns whose other gap is short, on the GPU (-m gpu).

A leader with a short other gap masks follower r on its top r-b (r-a) split points, whose W operand
level t does not have yet, and the follower scans them itself.  A masked point that leaked, a top
point scanned twice or not at all, changes a matrix, so every fold here is held against the
reference's hashes (tests/golden/hashes.json) or the C restatement (OracleFold), with sharing on
every level (split_target=-1: g_lo = 0, every a and b in {0, 1, 2} meets every r) and under the
split targets of tests/schedule_rows.py (g_lo > 0, lead splits 4 and 8: a follower with top points
inside a split leader launch).  CCJ_SHARE_EDGES=0 (read when a context is created) is the rule this
replaced; tests/test_share_edges.py pins the roles themselves on the CPU.
"""
import pytest

from ccj_amd import PEN_DEFAULT, share_roles
from tests.il_prune_cases import rseq
from tests.oracle_lib import OracleFold, blob, golden
from tests.schedule_rows import ALL_REGIME_TARGET, BOUNDARY_TARGET, nlev

pytestmark = pytest.mark.gpu


def _pen(**kw):
    names = ("PS", "PSM", "PSP", "PB", "PUP", "PPS", "a", "b", "c", "ap", "bp", "cp", "e_stP", "e_intP")
    return tuple(kw.get(k, v) for k, v in zip(names, PEN_DEFAULT))


# negative PUP and PPS make the W operands finite and negative; negative bp and cp the short-gap
# cells' own values (the multiloop seeds): a masked split point that leaked then changes a hash
PEN_W = _pen(PUP=-3, PPS=-20)
PEN_BC = _pen(bp=-40, cp=-3)

_oracles = {}


def _oracle(seq, params, dangles, noGU, pen):
    """One restatement fold per input, shared by the tests that need it and never changed."""
    key = (seq, params, dangles, noGU, pen)
    if key not in _oracles:
        o = OracleFold(seq, blob(params), dangles, noGU, threads=0, pen=pen)
        try:
            _oracles[key] = o.hashes()
        finally:
            o.close()
    return _oracles[key]


def _fold(seq, params, dangles=2, noGU=0, pen=None, probe=None, **kw):
    from ccj_amd import W_final
    wf = W_final(seq, dangles, params=params, noGU=bool(noGU), pen=pen, **kw)
    try:
        if probe is not None:
            probe(wf)
        wf.fill()
        try:
            wf.result()
        except Exception:
            pass  # reference backtrack exits; the matrices are complete
        return wf.hashes()
    finally:
        wf.close()


def _shares_everywhere(n):
    def probe(wf):
        sch = [wf.level_schedule(t) for t in range(nlev(n))]
        assert all(s.sharing and s.lead_split == 2 for s in sch) and (sch[0].g_lo, sch[0].g_hi) == (0, nlev(n))
    return probe


GOLDEN = {len(c["seq"]): c for c in golden("hashes.json") if 12 <= len(c["seq"]) <= 40 and not c["noGU"]}
GOLDEN_NOGU = [c for c in golden("hashes.json") if 12 <= len(c["seq"]) <= 40 and c["noGU"]][:2]
EVERYWHERE = [GOLDEN[n] for n in sorted(GOLDEN)] + GOLDEN_NOGU


def test_small_cases_cover_the_short_gaps():
    """n = 12 .. 40 with noGU cases, and in them every cut (r, other gap) on both sides."""
    ns = sorted(len(c["seq"]) for c in EVERYWHERE)
    assert ns[0] == 12 and ns[-1] >= 38 and len(GOLDEN_NOGU) == 2
    for n in (ns[0], ns[-1]):
        cuts = [set(), set()]
        for t in range(nlev(n)):
            for a in range(t + 1):
                x = share_roles(n, t, a, 0)
                for side, (s, oth) in enumerate(((x.a_side, t - a), (x.b_side, a))):
                    if s.role == 2 and s.top:
                        cuts[side].add((s.low, oth, s.top))
        assert cuts[0] == cuts[1] == {(r, o, r - o) for r in (1, 2, 3) for o in range(r)}


@pytest.mark.parametrize("case", EVERYWHERE, ids=lambda c: f"n{len(c['seq'])}-{c['params']}-d{c['dangles']}-g{c['noGU']}")
def test_every_level_shares_matches_reference(case):
    n = len(case["seq"])
    got = _fold(case["seq"], case["params"], case["dangles"], case["noGU"], split_target=-1, probe=_shares_everywhere(n))
    bad = [k for k in case["hashes"] if got[k] != case["hashes"][k]]
    assert not bad, f"matrices differ from the reference: {bad}"


ORACLE_CASES = {
    "ggccau": (rseq(7301, 37, "GGCCAU"), "Turner04", 2, 0, None),
    "ggccau_nogu": (rseq(7302, 29, "GGCCAU"), "DirksPierce09", 1, 1, None),
    "pen_w": (rseq(7303, 36, "GCGCAU"), "Turner04", 2, 0, PEN_W),
    "pen_bc": (rseq(7304, 40, "GCGCAU"), "DirksPierce09", 2, 0, PEN_BC),
    "pen_w_n17": (rseq(7305, 17, "GCGCAU"), "Turner04", 0, 0, PEN_W),
}


@pytest.mark.parametrize("name", sorted(ORACLE_CASES))
def test_every_level_shares_matches_oracle(name):
    seq, params, dangles, noGU, pen = ORACLE_CASES[name]
    want = _oracle(seq, params, dangles, noGU, pen)
    got = _fold(seq, params, dangles, noGU, pen, split_target=-1, probe=_shares_everywhere(len(seq)))
    assert len(want) == 31 and got == want, [k for k in want if got.get(k) != want[k]]


# ---- g_lo > 0, lead splits 4 and 8 (tests/schedule_rows.py): on == off == reference
FIXTURES = {len(c["seq"]): c for c in golden("hashes.json") if len(c["seq"]) in BOUNDARY_TARGET}
ROWS = sorted({(n, tg) for n in FIXTURES for tg in [ALL_REGIME_TARGET[n], *BOUNDARY_TARGET[n].values()]})


def _split_leaders_with_top_points(n, target, wf):
    """(lead split, side) of the leader-launch blocks that hold a follower side with top points"""
    out = set()
    for t in range(nlev(n)):
        ls = wf.level_schedule(t).lead_split
        for a in range(t + 1):
            x = share_roles(n, t, a, target)
            if x.in_lead:
                out |= {(ls, side) for side, s in enumerate((x.a_side, x.b_side)) if s.role == 2 and s.top}
    return out


@pytest.mark.parametrize("n,target", ROWS)
def test_split_leader_launch_on_off_reference(n, target, monkeypatch):
    case = FIXTURES[n]
    seen = {}

    def probe(wf):
        s = wf.level_schedule(0)
        assert 0 < s.g_lo < s.g_hi == nlev(n) and wf.schedule_options()[0] == target
        seen["top"] = _split_leaders_with_top_points(n, target, wf)

    on = _fold(case["seq"], case["params"], case["dangles"], case["noGU"], split_target=target, probe=probe)
    if target == ALL_REGIME_TARGET[n]:
        # a follower with top points, on either side, in a launch split 4 ways and (n = 52 has its
        # 8-way levels too, but no such block on them) 8 ways
        assert {(4, 0), (4, 1)} | ({(8, 0), (8, 1)} if n > 52 else set()) <= seen["top"]
    monkeypatch.setenv("CCJ_SHARE_EDGES", "0")
    off = _fold(case["seq"], case["params"], case["dangles"], case["noGU"], split_target=target)
    assert on == off
    bad = [k for k in case["hashes"] if on[k] != case["hashes"][k]]
    assert not bad, f"matrices differ from the reference: {bad}"


@pytest.mark.parametrize("pen_id", ["pen_w", "pen_bc"])
def test_split_leader_launch_changed_penalties(pen_id, monkeypatch):
    n, pen = 58, {"pen_w": PEN_W, "pen_bc": PEN_BC}[pen_id]
    seq, target = rseq(7310, n, "GCGCAU"), ALL_REGIME_TARGET[n]
    want = _oracle(seq, "Turner04", 2, 0, pen)
    on = _fold(seq, "Turner04", pen=pen, split_target=target)
    monkeypatch.setenv("CCJ_SHARE_EDGES", "0")
    off = _fold(seq, "Turner04", pen=pen, split_target=target)
    assert on == off == want, [k for k in want if on.get(k) != want[k] or off.get(k) != want[k]]


def test_simulated_two_rank_shard(monkeypatch):
    n = 55
    case, target = FIXTURES[n], ALL_REGIME_TARGET[n]
    kw = dict(split_target=target, shard_world=2, shard_simulate=True)
    on = _fold(case["seq"], case["params"], case["dangles"], case["noGU"], **kw)
    bad = [k for k in case["hashes"] if on[k] != case["hashes"][k]]
    assert not bad, f"matrices differ from the reference: {bad}"
    monkeypatch.setenv("CCJ_SHARE_EDGES", "0")
    assert _fold(case["seq"], case["params"], case["dangles"], case["noGU"], **kw) == on
