"""The masked restatement: the C restatement of the fill (oracle/ccj_oracle.c) with one change,
built at test time — TEST INFRASTRUCTURE ONLY.

A constrained fold (include/ccj.h) is the reference's fold in which every lookup
pair[S[i]][S[j]] at positions (i, j) gives 0 where (i, j) lies in the constraint's set F.  The
restatement consults the pair table at positions in exactly 11 places, each of the form
`o->pair[(o->)S[a]][(o->)S[b]]`.  This module rewrites those 11 lookups to `mpair(o, a, b)` (the
table entry, or 0 where a symmetric (n+1) x (n+1) byte mask is set), compiles the result in a
temporary directory with the flags of oracle/Makefile, and binds it like tests/oracle_lib.py.
A restatement that gains, loses or reshapes a lookup fails the build loudly.

Omission variants (tests/test_constraint_sites.py).  masked_source(omit=SITE) is the
masked restatement with the one reader SITE left on the bare table, every other reader masked: the
fold an engine computes that forgot the constraint at that one reader.  A site is one of the 11
lookups, named by function and operand (SITES); the two lookups inside ptype() and can_pair() are
split into one site per call of those functions, rewritten to an unmasked twin (ptype_raw,
can_pair_raw).  "ptype" and "can_pair" name all the calls of one function at once.
masked_source(strict=True) is the full mask in which compute_V returns, before it stores, at a
masked (i, j): a forbidden pair never holds a V.
"""
import contextlib
import ctypes
import os
import re
import shutil
import subprocess
import tempfile

from tests.oracle_lib import HASH_NAMES, PkPenalties, ROOT

N_LOOKUPS = 11
_LOOKUP = re.compile(r"o->pair\[(?:o->)?S\[([^\[\]]+)\]\]\[(?:o->)?S\[([^\[\]]+)\]\]")
# anything that still indexes the pair table by an encoded base
_LEFT = re.compile(r"pair\[[^\]]*S\[")
_MPAIR = """
/* the constraint's set F, mask[a * (n + 1) + b] (symmetric); NULL: none */
static const unsigned char *ccj_mask;
void ccj_masked_set(const unsigned char *mask) { ccj_mask = mask; }
static inline int mpair(const oracle *o, int a, int b) {
    if (ccj_mask && a >= 1 && b >= 1 && a <= o->n && b <= o->n && ccj_mask[(size_t)a * (size_t)(o->n + 1) + (size_t)b]) return 0;
    return MPAIR_TABLE(o, a, b);
}
"""
_TABLE = "#define MPAIR_TABLE(o, a, b) ((o)->pair[(o)->S[a]][(o)->S[b]])\n"
# the unmasked twins of ptype() and can_pair(), for the one call an omission variant leaves out
_RAW = """static inline int ptype_raw(const oracle *o, int i, int j) { return MPAIR_TABLE(o, i, j); }
static inline int can_pair_raw(const oracle *o, int i, int j) {
    if (j - i <= TURN) return 0;
    return MPAIR_TABLE(o, i, j) > 0;
}
"""
_RAW_ANCHOR = "/* pseudo_loop.cc:822-840 */\n"

# The 11 lookups in the order they stand in ccj_oracle.c: (site name, or the function whose calls
# are the sites; the lookup's operands as the regular expression captures them).
LOOKUPS = [
    ("can_pair", ("i", "j")), ("ptype", ("i", "j")),
    ("E_MLStem.ij", ("i", "j")), ("E_MLStem.i1j", ("i + 1", "j")), ("E_MLStem.ij1", ("i", "j - 1")),
    ("E_MLStem.i1j1", ("i + 1", "j - 1")),
    ("E_MbLoop.ji", ("j", "i")),
    ("E_ext_Stem.ij", ("i", "j")), ("E_ext_Stem.i1j", ("i + 1", "j")), ("E_ext_Stem.ij1", ("i", "j - 1")),
    ("E_ext_Stem.i1j1", ("i + 1", "j - 1")),
]
# One site per call of ptype() / can_pair(): name -> (function, text that holds the call(s), which
# of that text's occurrences in the file, how often the text occurs, calls inside the text).
CALLS = {
    "compute_int.ij_kl": ("ptype", "ptype(o, i, j), o->rtype[ptype(o, k, l)]", 0, 1, 2),
    "compute_V.ij": ("ptype", "int tc = ptype(o, i, j);", 0, 1, 1),
    "compute_V.iloop_kl": ("ptype", "tc, o->rtype[ptype(o, k, l)]", 0, 1, 1),
    "get_PfromMdoubleprime.il": ("ptype", "return ptype(o, i, l) == 0 ? INF : 0;", 0, 1, 1),
    "PL.ij": ("ptype", "if (ptype(o, i, j) > 0) {", 0, 1, 1),
    "PR.kl": ("ptype", "if (ptype(o, k, l) > 0) {", 0, 1, 1),
    "PM.jk": ("ptype", "if (ptype(o, j, k) > 0) {", 0, 1, 1),
    "PO.il": ("ptype", "if (ptype(o, i, l) > 0) {", 0, 1, 1),
    "get_PLiloop.ij": ("can_pair", "if (!can_pair(o, i, j)) return INF;", 0, 1, 1),
    "get_PLiloop.ddp": ("can_pair", "if (!can_pair(o, d, dp)) continue;", 0, 4, 1),
    "get_PRiloop.kl": ("can_pair", "if (!can_pair(o, k, l)) return INF;", 0, 1, 1),
    "get_PRiloop.ddp": ("can_pair", "if (!can_pair(o, d, dp)) continue;", 1, 4, 1),
    "get_PMiloop.jk": ("can_pair", "if (!can_pair(o, j, k)) return INF;", 0, 1, 1),
    "get_PMiloop.ddp": ("can_pair", "if (!can_pair(o, d, dp)) continue;", 2, 4, 1),
    "get_POiloop.il": ("can_pair", "if (!can_pair(o, i, l)) return INF;", 0, 1, 1),
    "get_POiloop.ddp": ("can_pair", "if (!can_pair(o, d, dp)) continue;", 3, 4, 1),
}
SPLIT = ("can_pair", "ptype")
SITES = [nm for nm, _ in LOOKUPS if nm not in SPLIT] + list(CALLS)
# the only sites a fixture file may declare unobserved (none of them has to be)
MAY_BE_UNOBSERVED = {s for s, c in CALLS.items() if c[0] == "can_pair"} | {"get_PfromMdoubleprime.il"} | \
    {nm for nm, _ in LOOKUPS if nm.startswith("E_ext_Stem.")}
_STRICT_ANCHOR = "    int en[3];\n    int tc = ptype(o, i, j);\n"
_STRICT = "    int en[3];\n    if (ccj_mask && ccj_mask[(size_t)i * (size_t)(o->n + 1) + (size_t)j]) return;\n" \
          "    int tc = ptype(o, i, j);\n"

_libs = {}


def _find_nth(src, text, k):
    pos = -1
    for _ in range(k + 1):
        pos = src.index(text, pos + 1)
    return pos


def masked_source(omit=None, strict=False):
    """ccj_oracle.c with its position lookups of the pair table replaced by mpair(); omit: the one
    site (of SITES, or "ptype" / "can_pair") that keeps the bare table; strict: compute_V stores
    nothing at a masked (i, j)."""
    assert omit is None or omit in SITES or omit in SPLIT, f"no such site: {omit}"
    with open(os.path.join(ROOT, "oracle", "ccj_oracle.c")) as f:
        src = f.read()
    seen = []

    def rewrite(m):
        x = len(seen)
        seen.append((m.group(1), m.group(2)))
        if x < N_LOOKUPS and LOOKUPS[x][0] == omit:
            return "MPAIR_TABLE(o, %s, %s)" % (m.group(1), m.group(2))
        return "mpair(o, %s, %s)" % (m.group(1), m.group(2))

    src = _LOOKUP.sub(rewrite, src)
    assert len(seen) == N_LOOKUPS, f"{len(seen)} position lookups of the pair table in ccj_oracle.c, expected {N_LOOKUPS}"
    assert seen == [ops for _, ops in LOOKUPS], f"the lookups changed their order or operands: {seen}"
    left = _LEFT.findall(src)
    assert not left, f"position lookups of the pair table the substitution missed: {left}"
    # every call of ptype() and can_pair() belongs to exactly one site
    for fn in SPLIT:
        calls = len(re.findall(r"\b%s\(o, " % fn, src))
        assert calls == sum(c[4] for c in CALLS.values() if c[0] == fn), f"{calls} calls of {fn}(): a site table entry is missing"
    spans = []
    for nm, (fn, text, which, count, ncalls) in CALLS.items():
        assert src.count(text) == count, f"site {nm}: {text!r} occurs {src.count(text)} times, expected {count}"
        assert text.count(fn + "(o, ") == ncalls
        spans.append((_find_nth(src, text, which), len(text), nm))
    assert len({s[0] for s in spans}) == len(spans), "two sites name the same call"
    if omit in CALLS:
        fn, text = CALLS[omit][:2]
        at = next(s[0] for s in spans if s[2] == omit)
        src = src[:at] + text.replace(fn + "(o, ", fn + "_raw(o, ") + src[at + len(text):]
    assert src.count(_RAW_ANCHOR) == 1, "compute_int's heading moved"
    src = src.replace(_RAW_ANCHOR, _RAW + _RAW_ANCHOR)
    if strict:
        assert src.count(_STRICT_ANCHOR) == 1, "compute_V's first lines moved"
        src = src.replace(_STRICT_ANCHOR, _STRICT)
    marker = "} oracle;\n"
    assert src.count(marker) == 1, "the oracle struct's end moved"
    return src.replace(marker, marker + _TABLE + _MPAIR)


def _flags():
    with open(os.path.join(ROOT, "oracle", "Makefile")) as f:
        mk = f.read()
    m = re.search(r"^ORACLE_CFLAGS\s*:=\s*(.+)$", mk, re.M)
    assert m, "ORACLE_CFLAGS left oracle/Makefile"
    return [x.replace("../include", os.path.join(ROOT, "include")) for x in m.group(1).split()]


def masked_lib(omit=None, strict=False):
    """The masked restatement, or one of its variants, compiled to a path of its own and loaded once."""
    key = (omit, strict)
    if key not in _libs:
        tmp = tempfile.mkdtemp(prefix="ccj_masked_")
        try:
            tag = ("_strict" if strict else "") + ("_" + re.sub(r"\W", "_", omit) if omit else "")
            c = os.path.join(tmp, "ccj_masked%s.c" % tag)
            so = os.path.join(tmp, "libccj_masked%s.so" % tag)
            with open(c, "w") as f:
                f.write(masked_source(omit, strict))
            r = subprocess.run([os.environ.get("CC", "gcc")] + _flags() + ["-shared", "-o", so, c, "-lm"],
                               capture_output=True, text=True)
            assert r.returncode == 0, r.stderr
            L = ctypes.CDLL(so)
        finally:
            shutil.rmtree(tmp, ignore_errors=True)
        L.ccj_masked_set.argtypes = [ctypes.c_char_p]
        L.ccj_oracle_fold_pen.restype = ctypes.c_void_p
        L.ccj_oracle_fold_pen.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_int, ctypes.c_int,
                                          ctypes.POINTER(PkPenalties)]
        L.ccj_oracle_hashes.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64)]
        L.ccj_oracle_free.argtypes = [ctypes.c_void_p]
        L.ccj_oracle_W.argtypes = [ctypes.c_void_p, ctypes.c_int]
        L.ccj_oracle_W.restype = ctypes.c_int
        L.ccj_oracle_get4.argtypes = [ctypes.c_void_p] + [ctypes.c_int] * 5
        L.ccj_oracle_get4.restype = ctypes.c_int
        L.ccj_oracle_get2.argtypes = [ctypes.c_void_p] + [ctypes.c_int] * 3
        L.ccj_oracle_get2.restype = ctypes.c_int
        L.ccj_oracle_low_stores.argtypes = [ctypes.c_void_p]
        L.ccj_oracle_low_stores.restype = ctypes.c_longlong
        _libs[key] = L
    return _libs[key]


def build_variants(sites, strict=False):
    """Compile the omission variants of `sites` (and the strict variant) side by side; each is
    loaded once per process like masked_lib()."""
    from concurrent.futures import ThreadPoolExecutor
    keys = [(s, False) for s in sites] + ([(None, True)] if strict else [])
    with ThreadPoolExecutor(min(8, os.cpu_count() or 1)) as ex:
        list(ex.map(lambda k: masked_lib(*k), [k for k in keys if k not in _libs]))


def mask_of(n, unpaired=None, forbid=(), allow_only=None):
    """The set F of a constraint (include/ccj.h) as the (n+1) x (n+1) byte mask, and as a set of
    pairs (i, j), i < j."""
    F = set()
    if allow_only is not None:
        keep = {(min(i, j), max(i, j)) for i, j in allow_only}
        F = {(i, j) for i in range(1, n + 1) for j in range(i + 1, n + 1)} - keep
    if unpaired:
        assert len(unpaired) == n
        for p, ch in enumerate(unpaired, 1):
            if ch == "x":
                F |= {(min(p, q), max(p, q)) for q in range(1, n + 1) if q != p}
    F |= {(min(i, j), max(i, j)) for i, j in forbid}
    m = bytearray((n + 1) * (n + 1))
    for i, j in F:
        m[i * (n + 1) + j] = m[j * (n + 1) + i] = 1
    return bytes(m), F


@contextlib.contextmanager
def _one_thread(L):
    """The folds here are small (n <= 36): a team of OpenMP threads costs them far more than it
    saves.  One thread for the call, then the setting as it was."""
    if not hasattr(L, "omp_set_num_threads"):
        yield
        return
    before = L.omp_get_max_threads()
    L.omp_set_num_threads(1)
    try:
        yield
    finally:
        L.omp_set_num_threads(before)


class MaskedFold:
    """The masked restatement's sequential fill for one sequence under the constraint's set F."""
    _omit, _strict = None, False

    def __init__(self, seq, blob, dangles=2, noGU=0, unpaired=None, forbid=(), allow_only=None, mask=None):
        L = self._L = masked_lib(self._omit, self._strict)
        self.n = len(seq)
        if mask is None:
            mask, _ = mask_of(self.n, unpaired, forbid, allow_only)
        assert len(mask) == (self.n + 1) ** 2
        self._blob = ctypes.create_string_buffer(blob, len(blob))
        self._mask = ctypes.create_string_buffer(mask, len(mask))
        L.ccj_masked_set(self._mask)
        try:
            with _one_thread(L):
                self.h = L.ccj_oracle_fold_pen(seq.encode(), self._blob, dangles, noGU, None)
        finally:
            L.ccj_masked_set(None)
        if not self.h:
            raise MemoryError("oracle allocation failed")

    def hashes(self):
        out = (ctypes.c_uint64 * 31)()
        with _one_thread(self._L):
            self._L.ccj_oracle_hashes(self.h, out)
        return {HASH_NAMES[i]: "%016x" % out[i] for i in range(31)}

    def get4(self, m, i, j, k, l):
        return self._L.ccj_oracle_get4(self.h, m, i, j, k, l)

    def get2(self, m, i, j):
        return self._L.ccj_oracle_get2(self.h, m, i, j)

    def W(self, j):
        return self._L.ccj_oracle_W(self.h, j)

    def low_stores(self):
        return self._L.ccj_oracle_low_stores(self.h)

    def close(self):
        if self.h:
            self._L.ccj_oracle_free(self.h)
            self.h = None

    def __del__(self):
        self.close()


class OmittedFold(MaskedFold):
    """The fill of the omission variant of one site: OmittedFold(site, seq, blob, ...)."""

    def __init__(self, site, *args, **kw):
        self._omit = site
        super().__init__(*args, **kw)


class StrictFold(MaskedFold):
    """The fill of the strict variant: the full mask, and no V is stored at a masked (i, j)."""
    _strict = True


def cons_of(c):
    """The constraint of a fixture case (tests/golden/constraint*_cases.json) as the keyword arguments of MaskedFold."""
    return dict(unpaired=c["unpaired"], forbid=[tuple(p) for p in c["forbid"]],
                allow_only=None if c["allow_only"] is None else [tuple(p) for p in c["allow_only"]])


def fold_case(cls, c, *site):
    """(hashes, W(n), low stores) of one fold of the fixture case c by MaskedFold, StrictFold or
    OmittedFold (then with its site)."""
    from tests.oracle_lib import blob
    m = cls(*site, c["seq"], blob(c["params"]), c["dangles"], c["noGU"], **cons_of(c))
    try:
        return m.hashes(), m.W(len(c["seq"])), m.low_stores()
    finally:
        m.close()
