"""Interior-loop candidates dominated through a stacked pair, on the CPU (no GPU).

The list builder drops a candidate (d,dp) of pair (p,q) when an intermediate pair stacked on (p,q)
("near") or on (d,dp) ("far") carries the same inner value into the cell at no higher energy
(ccj_amd/csrc/ccj_ilprune.h).  Here the host form of the rule (ccj_il_prune_host) is held against a
brute-force evaluation of the same two witnesses from the windows of the pairs involved, against the
restatement's matrices (no dropped candidate undercuts its witness at any cell that reads it), and
against a fill restated with the kept entries only.
"""
import numpy as np
import pytest

import bench
import ccj_amd
from tests.il_prune_cases import CPU_FOLDS, FAR, NEAR, U, can_pair, entries, lists, window
from tests.mloop2d_cases import valid_cells
from tests.oracle_lib import HASH_NAMES, OracleFold, blob

INF = 10000000  # include/ccj_params.h CCJ_INF: what the restatement's getter returns outside the valid cells
TURN = 3
_mats = {}


def _matrices(name):
    """PL, PR, PM and the matrices their cells read, as dense [i][j][k][l] arrays (INF outside the valid
    cells, like the restatement's getter), once per fold."""
    if name not in _mats:
        seq, params, dangles, pen = CPU_FOLDS[name]
        o = OracleFold(seq, blob(params), dangles, 0, pen=pen)
        n = len(seq)
        names = ("PL", "PR", "PM", "PfromL", "PfromR", "PfromM", "PLmloop01", "PLmloop10", "PRmloop01", "PRmloop10",
                 "PMmloop01", "PMmloop10")
        M = {x: np.full((n + 2,) * 4, INF, dtype=np.int64) for x in names}
        for c in valid_cells(n):
            for x in names:
                M[x][c] = o.get4(HASH_NAMES.index(x), *c)
        M["low_stores"] = o.low_stores()
        o.close()
        _mats[name] = M
    return _mats[name]


def _fold_lists(name):
    seq, params, dangles, pen = CPU_FOLDS[name]
    return seq, lists(seq, params, dangles, pen)


def _stack(L, x, y):
    """The level kernel's (0,0) terms on the pair stacked inside (x,y): min(est, ie)."""
    return min(int(L["est"][y - x, x]), int(L["ie"][y - x, x]))


def _witnesses(L, kind, w, p, u1, u2):
    """[(bit, (x, y), E1, E2)] of the near and far intermediates of a candidate, where they can pair:
    E1 carries (x,y) into the list's own pair, E2 carries the candidate into (x,y).  Every energy is read
    from a window or a plane, none from the rule."""
    q = p + w
    e, st = (L["e_ilm"], L["st_ilm"]) if kind else (L["e_il"], L["st_il"])
    if u1 < 1 or u2 < 1:
        return []
    if kind == 0:
        d, dp = p + 1 + u1, q - 1 - u2
        near, far = (p + 1, q - 1), (d - 1, dp + 1)
        sN, sF = _stack(L, p, q), _stack(L, d - 1, dp + 1)
        nw, npos = w - 2, p + 1  # the near pair's own list holds the candidate at (u1-1, u2-1)
    else:
        d, dp = p - 1 - u1, q + 1 + u2
        near, far = (p - 1, q + 1), (d + 1, dp - 1)
        sN, sF = _stack(L, p - 1, q + 1), _stack(L, d, dp)
        nw, npos = w + 2, p - 1
    one = (u1, u2) == (1, 1)
    out = []
    if st[w, p, 0, 0]:
        if one:
            out.append((NEAR, near, sN, sF))
        else:
            assert st[nw, npos, u1 - 1, u2 - 1], "the candidate is in the near pair's own window"
            out.append((NEAR, near, sN, int(e[nw, npos, u1 - 1, u2 - 1])))
    if st[w, p, u1 - 1, u2 - 1]:
        out.append((FAR, far, sN if one else int(e[w, p, u1 - 1, u2 - 1]), sF))
    return out


@pytest.mark.parametrize("name", ["T04_n34", "DP09_n32_gc"])
def test_host_rule_equals_the_brute_force_witnesses(name):
    seq, L = _fold_lists(name)
    n = len(seq)
    dropped = 0
    for kind in (0, 1):
        st, e = (L["st_ilm"], L["e_ilm"]) if kind else (L["st_il"], L["e_il"])
        for w in range(n):
            for p in range(1, n - w + 1):
                got = {(int(a), int(b)) for a, b in np.argwhere(st[w, p] != 0)}
                want = set(window(seq, kind, p, p + w)) if can_pair(seq, p, p + w) else set()
                assert got == want, f"kept + dropped is the full list of kind {kind} pair {(p, p + w)}"
                for u1, u2 in got:
                    E = int(e[w, p, u1, u2])
                    dom = {bit for bit, _, E1, E2 in _witnesses(L, kind, w, p, u1, u2) if E1 + E2 <= E}
                    bits = int(st[w, p, u1, u2]) >> 1
                    assert (bits != 0) == bool(dom), (kind, w, p, u1, u2)
                    assert bool(bits & FAR) == (FAR in dom)
                    # the near witness costs an E_IntLoop, so the rule skips it where far already drops
                    assert bool(bits & NEAR) == (NEAR in dom and ((u1, u2) == (1, 1) or FAR not in dom))
                    dropped += bits != 0
    c = L["counts"]
    assert c[1] == int((L["st_il"] != 0).sum()) and c[0] == int((L["st_il"] == 1).sum())
    assert c[3] == int((L["st_ilm"] != 0).sum()) and c[2] == int((L["st_ilm"] == 1).sum())
    assert dropped == c[1] - c[0] + c[3] - c[2] > 0


@pytest.mark.parametrize("name", list(CPU_FOLDS))
def test_no_dropped_candidate_undercuts_its_witness(name):
    """At every cell that reads a dropped candidate, the term through each of its witnesses is no higher
    (on the restatement's stored values; inside the domain they are the engine's)."""
    seq, L = _fold_lists(name)
    M = _matrices(name)
    assert M["low_stores"] == 0
    n = len(seq)
    up = np.triu(np.ones((n + 2, n + 2), dtype=bool))  # [a][b] with a <= b
    checks = 0
    for w, p, u1, u2 in entries(L, 0):
        bits = int(L["st_il"][w, p, u1, u2]) >> 1
        if not bits:
            continue
        q, E = p + w, int(L["e_il"][w, p, u1, u2])
        d, dp = p + 1 + u1, q - 1 - u2
        for bit, (x, y), E1, _ in _witnesses(L, 0, w, p, u1, u2):
            if not bits & bit:
                continue
            # PL: closing pair (i,j) = (p,q), every (k,l) behind it
            a, b = M["PL"][x, y, q + 2:n + 1, :n + 1], M["PL"][d, dp, q + 2:n + 1, :n + 1]
            m = up[q + 2:n + 1, :n + 1]
            assert (a[m] + E1 <= b[m] + E).all(), ("PL", name, w, p, u1, u2, bit)
            checks += int(m.sum())
            # PR: closing pair (k,l) = (p,q), every (i,j) in front of it
            if p >= 3:
                a, b = M["PR"][1:p - 1, 1:p - 1, x, y], M["PR"][1:p - 1, 1:p - 1, d, dp]
                m = up[1:p - 1, 1:p - 1]
                assert (a[m] + E1 <= b[m] + E).all(), ("PR", name, w, p, u1, u2, bit)
                checks += int(m.sum())
    for w, p, u1, u2 in entries(L, 1):
        bits = int(L["st_ilm"][w, p, u1, u2]) >> 1
        if not bits or w <= TURN:  # no cell reads the list of a pair (j,k) closer than TURN (get_PMiloop's can_pair)
            continue
        q, E = p + w, int(L["e_ilm"][w, p, u1, u2])
        d, dp = p - 1 - u1, q + 1 + u2
        for bit, (x, y), E1, _ in _witnesses(L, 1, w, p, u1, u2):
            if not bits & bit:
                continue
            # PM: pair (j,k) = (p,q), every cell whose bounds d > i, dp < l admit the candidate
            a, b = M["PM"][1:d, x, y, dp + 1:n + 1], M["PM"][1:d, d, dp, dp + 1:n + 1]
            assert (a + E1 <= b + E).all(), ("PM", name, w, p, u1, u2, bit)
            checks += a.size
    assert checks > 1000


def _kept_min(M, L, kind, w, p, plane_of):
    """min over the kept entries of pair (p, p+w) past (0,0) of energy + partner plane."""
    st, e = (L["st_ilm"], L["e_ilm"]) if kind else (L["st_il"], L["e_il"])
    best = None
    for u1, u2 in np.argwhere(st[w, p] == 1):
        if u1 == 0 and u2 == 0:
            continue
        v = plane_of(int(u1), int(u2)) + int(e[w, p, u1, u2])
        best = v if best is None else np.minimum(best, v)
    return best


@pytest.mark.parametrize("name", ["T04_n34", "DP09_n32_gc"])
def test_pruned_fill_restated_gives_the_stored_values(name):
    """PL, PR and PM of every cell from the kept entries and the level kernel's own terms (the stack,
    the loop without unpaired bases, the multiloop and Pfrom terms) equal the stored values."""
    seq, L = _fold_lists(name)
    M = _matrices(name)
    n = len(seq)
    pen = CPU_FOLDS[name][3] or ccj_amd.PEN_DEFAULT
    ap, bp = pen[9], pen[10]
    est, ie = L["est"].astype(np.int64), L["ie"].astype(np.int64)
    cells = 0
    for i, j, k, l in valid_cells(n):
        if k != j + 2 or l != k:  # once per (i,j): the planes below cover every (k,l)
            continue
        # ---- PL: closing pair (i,j), planes over (k,l)
        if can_pair(seq, i, j):
            w = j - i
            b1 = np.full((n + 2, n + 2), INF, dtype=np.int64)
            if w > TURN + 2:
                pin = M["PL"][i + 1, j - 1]
                b1 = np.minimum(pin + est[w, i], pin + ie[w, i])
                km = _kept_min(M, L, 0, w, i, lambda u1, u2: M["PL"][i + 1 + u1, j - 1 - u2])
                if km is not None:
                    b1 = np.minimum(b1, km)
            b2 = np.minimum(M["PLmloop10"][i + 1, j - 1], M["PLmloop01"][i + 1, j - 1]) + ap + 2 * bp if w >= 2 else INF
            b3 = M["PfromL"][i + 1, j - 1] if w >= TURN + 1 else INF
            got = np.minimum(np.minimum(np.minimum(b1, b2), b3), 32767)
            for kk in range(j + 2, n + 1):
                assert (got[kk, kk:n + 1] == M["PL"][i, j, kk, kk:n + 1]).all(), ("PL", i, j, kk)
                cells += n + 1 - kk
    for i, j, k, l in valid_cells(n):
        if i != 1 or j != 1:  # once per (k,l): planes over (i,j)
            continue
        if can_pair(seq, k, l):
            w = l - k
            b1 = np.full((n + 2, n + 2), INF, dtype=np.int64)
            if w > TURN + 2:
                pin = M["PR"][:, :, k + 1, l - 1]
                b1 = np.minimum(pin + est[w, k], pin + ie[w, k])
                km = _kept_min(M, L, 0, w, k, lambda u1, u2: M["PR"][:, :, k + 1 + u1, l - 1 - u2])
                if km is not None:
                    b1 = np.minimum(b1, km)
            b2 = np.minimum(M["PRmloop10"][:, :, k + 1, l - 1], M["PRmloop01"][:, :, k + 1, l - 1]) + ap + 2 * bp if w >= 2 else INF
            b3 = M["PfromR"][:, :, k + 1, l - 1] if w >= TURN + 1 else INF
            got = np.minimum(np.minimum(np.minimum(b1, b2), b3), 32767)
            for ii in range(1, k - 1):
                assert (got[ii, ii:k - 1] == M["PR"][ii, ii:k - 1, k, l]).all(), ("PR", ii, k, l)
                cells += k - 1 - ii
    # ---- PM: pair (j,k), planes over (i,l); the candidate's bounds d > i, dp < l are per cell
    for j in range(1, n + 1):
        for k in range(j + 2, n + 1):
            if not can_pair(seq, j, k):
                continue
            w = k - j
            ii, ll = np.meshgrid(np.arange(n + 2), np.arange(n + 2), indexing="ij")
            inner = (ii < j) & (ll > k)
            b1 = np.full((n + 2, n + 2), INF, dtype=np.int64)
            b2 = b3 = INF
            if j >= 2 and k < n and w > TURN:  # get_PMiloop: can_pair(j,k) includes the distance rule
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
                b3 = M["PfromM"][:, j - 1, k + 1, :]  # k >= j + TURN - 1 holds in every valid cell
            b4 = np.where((ii == j) & (ll == k), 0, INF)
            got = np.minimum(np.minimum(np.minimum(b1, b2), np.minimum(b3, b4)), 32767)
            assert (got[1:j + 1, k:n + 1] == M["PM"][1:j + 1, j, k, k:n + 1]).all(), ("PM", j, k)
            cells += j * (n + 1 - k)
    assert cells > 10000


def test_the_headline_fold_drops_at_least_half():
    """Guard against silent disabling: 57.4 % by count with the reference's energies."""
    c = ccj_amd.il_prune_host(bench.rseq(5, 200), "Turner04", windows=False)["counts"]
    assert 0 < c[0] + c[2] <= 0.5 * (c[1] + c[3])


def test_a_short_fold_drops_some():
    c = ccj_amd.il_prune_host(bench.rseq(11, 30), "Turner04", windows=False)["counts"]
    assert c[0] < c[1] and c[2] < c[3]
