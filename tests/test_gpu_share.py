"""Split-point sharing (ccj_engine.h) on the GPU (-m gpu).

A leader cell scans its whole split range for itself and the next SHARE_R-1 cells of each of its
gap columns; the followers scan only the split points the leader did not see.  Min is
order-independent, so the fill must stay bit-identical to the reference.  By default (split
target 9216) sharing covers the levels from the first one that runs unsplit to the last, and no
level runs unsplit below n = 159: at smaller n the default schedule shares nothing.
split_target=-1 turns level splitting off so that sharing covers every level (g_lo = 0, lead
split 2), which exercises leaders, followers and the ring at small n; the other regimes (lead
splits 4 and 8, g_lo > 0 and its leaderless followers, the split plain launches below g_lo) are
reached at n = 52 .. 64 by tests/test_gpu_schedule.py, and tests/test_schedule.py pins which n and
targets reach what.
"""
import random

import pytest

from tests.oracle_lib import OracleFold, blob, golden

pytestmark = pytest.mark.gpu


def _rseq(seed, n, alphabet="ACGU"):
    r = random.Random(seed)
    return "".join(r.choice(alphabet) for _ in range(n))


def _hashes(seq, params, d=2, g=0, probe=None, **kw):
    from ccj_amd import W_final
    wf = W_final(seq, d, params=params, noGU=bool(g), **kw)
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


CASES = [c for c in golden("hashes.json") if len(c["seq"]) >= 12][::3]


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"n{len(c['seq'])}-{c['params']}-d{c['dangles']}-g{c['noGU']}")
def test_sharing_on_every_level_matches_reference(case):
    got = _hashes(case["seq"], case["params"], case["dangles"], case["noGU"], split_target=-1)
    bad = [k for k in case["hashes"] if got[k] != case["hashes"][k]]
    assert not bad, f"matrices differ from the reference: {bad}"


@pytest.mark.parametrize("seed", range(6))
def test_sharing_random_inputs_match_oracle(seed):
    r = random.Random(3100 + seed)
    n = r.randint(30, 70)
    seq = _rseq(4100 + seed, n, r.choice(["ACGU", "GGCCAU", "GCAU"]))
    params = r.choice(["Turner04", "DirksPierce09", "DirksPierce03", "CaoChen09"])
    o = OracleFold(seq, blob(params), 2, 0)
    try:
        assert _hashes(seq, params, split_target=-1) == o.hashes()
    finally:
        o.close()


@pytest.mark.parametrize("n,seed", [(90, 1), (140, 2), (168, 3)])
def test_sharing_on_off_identical(n, seed):
    """Default schedule == sharing off == sharing everywhere.  At n = 90 and 140 the default schedule
    shares nothing (it is the share-off schedule: every level splits); n = 168 is a little above the
    smallest n whose default schedule shares (159), with all three lead splits and g_lo > 0; the
    context's schedule getter says which is which."""
    seq = _rseq(seed, n)
    seen = {}

    def probe(key):
        def f(wf):
            seen[key] = [wf.level_schedule(t) for t in range(n - 2)]
        return f

    h_on = _hashes(seq, "Turner04", probe=probe("default"))
    assert _hashes(seq, "Turner04", share_splits=-1, probe=probe("off")) == h_on
    assert _hashes(seq, "Turner04", split_target=-1, probe=probe("everywhere")) == h_on
    assert not any(s.sharing or s.lead_split for s in seen["off"])
    assert all(s.regime == (1, 2) for s in seen["everywhere"])
    if n >= 159:
        g_lo = seen["default"][0].g_lo
        assert 0 < g_lo and seen["default"][0].g_hi == n - 2
        assert {s.lead_split for s in seen["default"][g_lo:]} == {2, 4, 8}
        assert all(s.split > 1 and not s.sharing for s in seen["default"][:g_lo])
    else:
        assert seen["default"] == seen["off"]


def test_sharing_n400_same_result():
    """BASELINE config-5 size (n = 400, past the stock reference's n >= 214 abort): sharing on and
    off give the same MFE, structure and W array (full hashes would copy 47 GB to the host)."""
    from ccj_amd import W_final
    n = 400
    seq = _rseq(6, n)
    out = []
    for kw in ({}, {"share_splits": -1}):
        wf = W_final(seq, 2, params="Turner04", **kw)
        try:
            e = wf.ccj()
            out.append((e, wf.structure, [wf.W(j) for j in range(n + 1)]))
        finally:
            wf.close()
    assert out[0] == out[1]
    assert len(out[0][1]) == n and out[0][0] == out[0][2][n] / 100.0
