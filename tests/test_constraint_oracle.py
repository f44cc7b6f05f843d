"""The CPU oracle of constrained folding (no GPU): the masked restatement (tests/masked_oracle.py) is
the restatement with every position lookup of the pair table routed through a mask of the
constraint's set F (include/ccj.h).  Here it is held against what is known without it:
the reference's hashes under an empty mask, the reference's own --noGU runs under the mask of every
G-U position pair, and the allow-only property on the reference's MFE structures.  Then the committed
fixtures are reproduced, and the candidate-list pruning rule under a constraint
(ccj_il_prune_host_constrained) is held against the masked restatement's matrices.
"""
import os
import sys

import numpy as np
import pytest

import ccj_amd
from tests.constraint_cases import case_id, cases, constraint_of, gu_pairs, pairs_of, pseudoknotted_e2e
from tests.masked_oracle import MaskedFold, mask_of, masked_source
from tests.mloop2d_cases import valid_cells
from tests.oracle_lib import HASH_NAMES, ROOT, OracleFold, blob, golden

INF = 10000000
TURN = 3
NMAX = 36


def _hashes(seq, params, dangles, noGU, **cons):
    m = MaskedFold(seq, blob(params), dangles, noGU, **cons)
    try:
        return m.hashes(), m.W(len(seq)), m.low_stores()
    finally:
        m.close()


def test_the_restatement_has_eleven_position_lookups():
    src = masked_source()  # asserts the count and that none is left
    assert src.count("mpair(o, ") == 11 + 0 and "static inline int mpair(" in src


def test_empty_mask_is_the_reference():
    """All folds of hashes.json with noGU off and n <= 36: the masked restatement with an empty mask
    gives the reference's 31 hashes; on a sample it is also held against OracleFold directly."""
    todo = [c for c in golden("hashes.json") if not c["noGU"] and len(c["seq"]) <= NMAX]
    assert len(todo) >= 50
    for x, c in enumerate(todo):
        h, _, _ = _hashes(c["seq"], c["params"], c["dangles"], 0)
        assert h == c["hashes"], (c["seq"], c["params"], c["dangles"])
        if x % 10 == 0:
            o = OracleFold(c["seq"], blob(c["params"]), c["dangles"], 0)
            assert o.hashes() == h
            o.close()


def test_gu_mask_is_the_reference_noGU_run():
    """F = every G-U position pair with noGU off is the reference's --noGU fold, matrix for matrix."""
    todo = [c for c in golden("hashes.json") if c["noGU"] and len(c["seq"]) <= NMAX]
    assert len(todo) >= 9
    for c in todo:
        seq = c["seq"].replace("T", "U") if c["params"].startswith("DNA") else c["seq"]
        pairs = [(i, j) for i, j in gu_pairs(seq)]
        h, _, _ = _hashes(c["seq"], c["params"], c["dangles"], 0, forbid=pairs)
        assert h == c["hashes"], (c["seq"], c["params"], c["dangles"])


def test_allow_only_the_mfe_structure_keeps_the_energy():
    """On the pseudoknotted e2e folds with n <= 34: allowing only the pairs of the reference's MFE
    structure leaves W(n) unchanged, and forbidding one pair of it never lowers W(n)."""
    todo = pseudoknotted_e2e(34)
    assert len(todo) >= 20
    for c, st, en in todo:
        n = len(c["seq"])
        args = (c["seq"], c["params"], c["dangles"], int(bool(c["noGU"])))
        _, w0, _ = _hashes(*args)
        assert "%g" % (w0 / 100.0) == en.strip("()"), (c["seq"], w0, en)
        prs = sorted(pairs_of(st))
        _, w1, _ = _hashes(*args, allow_only=prs)
        assert w1 == w0, (c["seq"], c["params"], w0, w1)
        _, w2, _ = _hashes(*args, forbid=[prs[len(prs) // 2]])
        assert w2 >= w0, (c["seq"], c["params"], w0, w2)


def test_the_committed_fixtures_are_reproduced():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import gen_constraint_cases
    finally:
        sys.path.pop(0)
    assert gen_constraint_cases.generate() == cases()


def test_fixtures_cover_the_kinds_and_stay_inside_the_domain():
    cs = cases()
    kinds = {c["kind"] for c in cs}
    assert {"x_in_helix", "forbid_mid_pair", "forbid_pk_helix", "allow_only_mfe", "mix", "x_everywhere"} <= kinds
    assert {c["dangles"] for c in cs} == {0, 1, 2}
    assert any(c["params"].startswith("DNA") for c in cs) and any(c["params"] == "Turner04" for c in cs)
    assert any(c["params"].startswith("DirksPierce") for c in cs)
    assert all(20 <= len(c["seq"]) <= 36 for c in cs)
    for c in cs:
        if c["kind"] == "x_everywhere":
            assert c["Wn"] == 0


# ---- the pruning rule under a mask -----------------------------------------------------------------

def _relation(c):
    """can(i, j): pair type > 0 under the binding (the table after noGU, minus F; no distance rule)."""
    seq = c["seq"].replace("T", "U")
    table = {"AU", "UA", "GC", "CG"} | (set() if c["noGU"] else {"GU", "UG"})
    _, F = mask_of(len(seq), c["unpaired"], [tuple(p) for p in c["forbid"]],
                   None if c["allow_only"] is None else [tuple(p) for p in c["allow_only"]])
    return lambda i, j: seq[i - 1] + seq[j - 1] in table and (i, j) not in F


def _matrices(c):
    names = ("PL", "PR", "PM", "PfromL", "PfromR", "PfromM", "PLmloop01", "PLmloop10", "PRmloop01", "PRmloop10",
             "PMmloop01", "PMmloop10")
    n = len(c["seq"])
    m = MaskedFold(c["seq"], blob(c["params"]), c["dangles"], c["noGU"], unpaired=c["unpaired"],
                   forbid=[tuple(p) for p in c["forbid"]],
                   allow_only=None if c["allow_only"] is None else [tuple(p) for p in c["allow_only"]])
    M = {x: np.full((n + 2,) * 4, INF, dtype=np.int64) for x in names}
    for cell in valid_cells(n):
        for x in names:
            M[x][cell] = m.get4(HASH_NAMES.index(x), *cell)
    assert m.low_stores() == 0
    m.close()
    return M


@pytest.mark.parametrize("c", cases(), ids=case_id)
def test_pruned_lists_under_a_mask_restate_the_masked_fill(c):
    """PL, PR and PM of every cell from the kept entries of the constrained lists and the level kernel's
    own terms equal the masked restatement's values (as tests/test_il_prune.py does without a mask); the
    lists hold exactly the candidates whose two pairs can pair under the binding."""
    seq, n = c["seq"], len(c["seq"])
    can = _relation(c)
    L = ccj_amd.il_prune_host(seq, blob(c["params"]), c["dangles"], bool(c["noGU"]), constraint=constraint_of(c))
    M = _matrices(c)
    pen = ccj_amd.PEN_DEFAULT
    ap, bp = pen[9], pen[10]
    est, ie = L["est"].astype(np.int64), L["ie"].astype(np.int64)
    U = ccj_amd.IL_U
    # the lists: own pair and candidate both able to pair under the binding
    for kind, st in ((0, L["st_il"]), (1, L["st_ilm"])):
        for w in range(n):
            for p in range(1, n - w + 1):
                q = p + w
                got = {(int(a), int(b)) for a, b in np.argwhere(st[w, p] != 0)}
                want = set()
                if can(p, q):
                    for u1 in range(U):
                        for u2 in range(U):
                            if kind == 0:
                                d, dp = p + 1 + u1, q - 1 - u2
                                ok = u1 <= min(w, 30) - 2 and u2 <= min(w - u1 - 6, 28) and can(d, dp)
                            else:
                                d, dp = p - 1 - u1, q + 1 + u2
                                ok = d >= 1 and dp <= n and can(d, dp)
                            if ok:
                                want.add((u1, u2))
                assert got == want, (kind, p, q)

    def kept_min(kind, w, p, plane_of):
        st, e = (L["st_ilm"], L["e_ilm"]) if kind else (L["st_il"], L["e_il"])
        best = None
        for u1, u2 in np.argwhere(st[w, p] == 1):
            if u1 == 0 and u2 == 0:
                continue
            v = plane_of(int(u1), int(u2)) + int(e[w, p, u1, u2])
            best = v if best is None else np.minimum(best, v)
        return best

    cells = 0
    for i in range(1, n + 1):
        for j in range(i, n + 1):
            if not can(i, j):
                continue
            w = j - i
            b1 = np.full((n + 2, n + 2), INF, dtype=np.int64)
            if w > TURN + 2:
                pin = M["PL"][i + 1, j - 1]
                b1 = np.minimum(pin + est[w, i], pin + ie[w, i])
                km = kept_min(0, w, i, lambda u1, u2: M["PL"][i + 1 + u1, j - 1 - u2])
                if km is not None:
                    b1 = np.minimum(b1, km)
            b2 = np.minimum(M["PLmloop10"][i + 1, j - 1], M["PLmloop01"][i + 1, j - 1]) + ap + 2 * bp if w >= 2 else INF
            b3 = M["PfromL"][i + 1, j - 1] if w >= TURN + 1 else INF
            got = np.minimum(np.minimum(np.minimum(b1, b2), b3), 32767)
            for kk in range(j + 2, n + 1):
                assert (got[kk, kk:n + 1] == M["PL"][i, j, kk, kk:n + 1]).all(), ("PL", i, j, kk)
                cells += n + 1 - kk
    for k in range(3, n + 1):
        for l in range(k, n + 1):
            if not can(k, l):
                continue
            w = l - k
            b1 = np.full((n + 2, n + 2), INF, dtype=np.int64)
            if w > TURN + 2:
                pin = M["PR"][:, :, k + 1, l - 1]
                b1 = np.minimum(pin + est[w, k], pin + ie[w, k])
                km = kept_min(0, w, k, lambda u1, u2: M["PR"][:, :, k + 1 + u1, l - 1 - u2])
                if km is not None:
                    b1 = np.minimum(b1, km)
            b2 = np.minimum(M["PRmloop10"][:, :, k + 1, l - 1], M["PRmloop01"][:, :, k + 1, l - 1]) + ap + 2 * bp if w >= 2 else INF
            b3 = M["PfromR"][:, :, k + 1, l - 1] if w >= TURN + 1 else INF
            got = np.minimum(np.minimum(np.minimum(b1, b2), b3), 32767)
            for ii in range(1, k - 1):
                assert (got[ii, ii:k - 1] == M["PR"][ii, ii:k - 1, k, l]).all(), ("PR", ii, k, l)
                cells += k - 1 - ii
    ii, ll = np.meshgrid(np.arange(n + 2), np.arange(n + 2), indexing="ij")
    for j in range(1, n + 1):
        for k in range(j + 2, n + 1):
            if not can(j, k):
                continue
            w = k - j
            inner = (ii < j) & (ll > k)
            b1 = np.full((n + 2, n + 2), INF, dtype=np.int64)
            b2 = b3 = INF
            if j >= 2 and k < n and w > TURN:
                pin = M["PM"][:, j - 1, k + 1, :]
                b1 = np.where(inner, pin + est[w + 2, j - 1], INF)
                b1 = np.minimum(b1, np.where((ii < j - 1) & (ll > k + 1), pin + ie[w + 2, j - 1], INF))
                st, e = L["st_ilm"], L["e_ilm"]
                for u1, u2 in np.argwhere(st[w, j] == 1):
                    if u1 == 0 and u2 == 0:
                        continue
                    d, dp = j - 1 - int(u1), k + 1 + int(u2)
                    b1 = np.minimum(b1, np.where((ii < d) & (ll > dp), M["PM"][:, d, dp, :] + int(e[w, j, u1, u2]), INF))
            if j >= 2 and k < n:
                b2 = np.minimum(M["PMmloop10"][:, j - 1, k + 1, :], M["PMmloop01"][:, j - 1, k + 1, :]) + ap + 2 * bp
                b3 = M["PfromM"][:, j - 1, k + 1, :]
            b4 = np.where((ii == j) & (ll == k), 0, INF)
            got = np.minimum(np.minimum(np.minimum(b1, b2), np.minimum(b3, b4)), 32767)
            assert (got[1:j + 1, k:n + 1] == M["PM"][1:j + 1, j, k, k:n + 1]).all(), ("PM", j, k)
            cells += j * (n + 1 - k)
    if c["kind"] != "x_everywhere":
        assert cells > 1000
