"""Every reader of the pair table is pinned by leaving it out (no GPU).

A constrained fold is the reference's fold with every position lookup of the pair table masked
(DESIGN.md §1).  tests/masked_oracle.py names those lookups as sites and builds, per site, the
omission variant: that one reader on the bare table, every other masked.  The fixtures of
tests/golden/constraint_site_cases.json (tools/gen_constraint_site_cases.py) are constrained folds
that a site's omission changes, so an engine that forgets the constraint at one reader fails them on
the GPU (tests/test_gpu_constraint_sites.py).  Here the fixtures are held to that claim, the sites
without a fixture to the list that may have none, and the forbidden-pair property (no V left at a
forbidden pair ever reaches W(n)) to a seeded sweep.
"""
import os
import random
import sys

import pytest

from tests.constraint_site_cases import OBSERVED, UNOBSERVED, case_id, cases, site_file
from tests.masked_oracle import (CALLS, LOOKUPS, MAY_BE_UNOBSERVED, SITES, SPLIT, MaskedFold, OmittedFold, StrictFold,
                                 build_variants, fold_case as _fold, masked_source)
from tests.oracle_lib import HASH_NAMES, ROOT, OracleFold, blob


@pytest.fixture(scope="module")
def variants():
    """Each variant the fixtures need, compiled once."""
    build_variants(OBSERVED, strict=True)


def test_the_sites_are_the_eleven_lookups_and_every_call():
    assert len(LOOKUPS) == 11 and len(SITES) == 9 + len(CALLS) == 25 and len(set(SITES)) == 25
    plain = masked_source()
    assert plain.count("mpair(o, ") == 11 and "_raw(o, " not in plain
    for s in SITES + list(SPLIT):
        src = masked_source(omit=s)  # asserts the lookup count, their operands, and that no call is missed
        raw = src.count("ptype_raw(o, ") + src.count("can_pair_raw(o, ")
        if s in CALLS:
            assert src.count("mpair(o, ") == 11 and raw == CALLS[s][4], s
        else:
            assert src.count("mpair(o, ") == 10 and raw == 0, s
    strict = masked_source(strict=True)
    assert strict.count("mpair(o, ") == 11 and strict.count("ccj_mask[") == plain.count("ccj_mask[") + 1


@pytest.mark.parametrize("c", cases(), ids=case_id)
def test_fixture_under_the_full_mask_and_its_omissions(c, variants):
    h, w, low = _fold(MaskedFold, c)
    assert h == c["hashes"] and w == c["Wn"] and low == 0 == c["low_stores"]
    assert _fold(StrictFold, c)[1] == c["strict_Wn"] == c["Wn"]
    assert c["pins"] or c["kind"].startswith("traceback_")  # those pin the traceback's own check, on the GPU
    for site, pin in c["pins"].items():
        ho, wo, _ = _fold(OmittedFold, c, site)
        differs = [k for k in HASH_NAMES if ho[k] != h[k]]
        # a fixture that its site's omission does not change pins nothing
        assert differs and differs == pin["differs"], (site, differs, pin["differs"])
        assert wo == pin["Wn"], (site, wo, pin["Wn"])


def test_every_site_is_pinned_twice_or_listed_as_unobserved():
    f = site_file()
    assert f["sites"] == SITES
    assert set(UNOBSERVED) <= MAY_BE_UNOBSERVED
    assert all(len(why) > 40 for why in UNOBSERVED.values())  # each listing carries its argument
    for s in SITES:
        pinned = [c for c in cases() if s in c["pins"]]
        if s in UNOBSERVED:
            assert not pinned, s
        else:
            assert len(pinned) >= 2, s
            assert len({(c["params"], c["kind"]) for c in pinned}) >= 2, s
    assert all(12 <= len(c["seq"]) <= 30 for c in cases())
    assert sum(c["kind"].startswith("traceback_") for c in cases()) >= 2


def test_the_committed_fixtures_are_reproduced(variants):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import gen_constraint_site_cases
    finally:
        sys.path.pop(0)
    assert gen_constraint_site_cases.generate() == site_file()


SMALL = [("GCGCCGAGCCCC", "Turner04", 1), ("UUGGAGCCUUUCAAGGCGCCU", "Turner04", 2), ("GGCCAGGUACCUGGAUCC", "DirksPierce09", 0)]


def test_empty_mask_every_variant_is_the_plain_restatement():
    build_variants(SITES, strict=True)
    for seq, params, dangles in SMALL:
        o = OracleFold(seq, blob(params), dangles, 0)
        want = o.hashes()
        o.close()
        c = dict(seq=seq, params=params, dangles=dangles, noGU=0, unpaired=None, forbid=[], allow_only=None)
        assert _fold(StrictFold, c)[0] == want
        for s in SITES:
            assert _fold(OmittedFold, c, s)[0] == want, (s, seq)


def _junction(rng):
    """A closing G-C stem around two G-C hairpins, n 18-32: the shape whose fold closes a multiloop
    with V < 0 (two times in three under the two parameter sets below)."""
    comp = {"G": "C", "C": "G"}

    def stem(k):
        a = "".join(rng.choice("GC") for _ in range(k))
        return a, "".join(comp[x] for x in reversed(a))

    def hairpin():
        a, b = stem(rng.randint(3, 4))
        return a + "".join(rng.choice("AAGU") for _ in range(rng.randint(3, 4))) + b

    while True:
        a, b = stem(rng.randint(2, 4))
        seq = a + "A" * rng.randint(0, 1) + hairpin() + "A" * rng.randint(0, 1) + hairpin() + "A" * rng.randint(0, 1) + b
        if 18 <= len(seq) <= 32:
            return seq


SWEEP = 300


def test_no_forbidden_pair_reaches_W():
    """300 seeded folds, n 18-32, each with something to forbid: every multiloop-closed pair with
    V < 0 of the unconstrained fold is forbidden.  Candidates are drawn (G-C junctions, every fifth a
    random sequence) until 300 of them have such a pair; a candidate without one asserts nothing and
    is not counted.  V is not guarded by the pair type, so such a pair keeps a V in the masked fold (a
    multiloop branch with type 0); W(n) must equal that of the strict variant, where no masked pair
    stores a V.  If this ever fails, the masked fold holds a structure with a forbidden pair and the
    definition of DESIGN.md §1 has to change (engine and oracle together)."""
    rng = random.Random(3)
    drawn = swept = kept_a_V = 0
    while swept < SWEEP and drawn < 5 * SWEEP:
        drawn += 1
        seq = _junction(rng) if drawn % 5 else "".join(rng.choice("GGCCAU") for _ in range(rng.randint(18, 32)))
        n = len(seq)
        assert 18 <= n <= 32
        c = dict(seq=seq, dangles=rng.choice([0, 0, 1, 2]), params=rng.choice(["Turner04", "DirksPierce09"]), noGU=0,
                 unpaired=None, forbid=[], allow_only=None)
        m = MaskedFold(seq, blob(c["params"]), c["dangles"], 0)
        closed = [(i, j) for i in range(1, n + 1) for j in range(i + 4, n + 1)
                  if m.get2(4, i, j) == ord("M") and m.get2(3, i, j) < 0]
        m.close()
        if not closed:
            continue
        swept += 1
        c["forbid"] = closed
        m = MaskedFold(seq, blob(c["params"]), c["dangles"], 0, forbid=closed)
        kept_a_V += any(m.get2(4, i, j) != ord("N") for i, j in closed)  # Vtype N: nothing stored
        w = m.W(n)
        m.close()
        assert _fold(StrictFold, c)[1] == w, (c, w)
    print("candidates drawn:", drawn, "folds swept:", swept, "of which a forbidden pair kept a V:", kept_a_V)
    assert swept == SWEEP, (drawn, swept)
    # The innermost forbidden closer encloses stems the mask does not touch, and the multiloop branch
    # of compute_V reads no table row that is INF at pair type 0: it keeps a V in every swept fold, so
    # in every one of them the strict variant differs from the mask in V and still gives the same W(n).
    assert kept_a_V == swept, (swept, kept_a_V)
