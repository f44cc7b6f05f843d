"""The masked restatement: the C restatement of the fill (oracle/ccj_oracle.c) with one change,
built at test time — TEST INFRASTRUCTURE ONLY.

A constrained fold (include/ccj.h) is the reference's fold in which every lookup
pair[S[i]][S[j]] at positions (i, j) gives 0 where (i, j) lies in the constraint's set F.  The
restatement consults the pair table at positions in exactly 11 places, each of the form
`o->pair[(o->)S[a]][(o->)S[b]]`.  This module rewrites those 11 lookups to `mpair(o, a, b)` (the
table entry, or 0 where a symmetric (n+1) x (n+1) byte mask is set), compiles the result in a
temporary directory with the flags of oracle/Makefile, and binds it like tests/oracle_lib.py.
A restatement that gains, loses or reshapes a lookup fails the build loudly.
"""
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

_lib = None


def masked_source():
    """ccj_oracle.c with its position lookups of the pair table replaced by mpair()."""
    with open(os.path.join(ROOT, "oracle", "ccj_oracle.c")) as f:
        src = f.read()
    src, count = _LOOKUP.subn(r"mpair(o, \1, \2)", src)
    assert count == N_LOOKUPS, f"{count} position lookups of the pair table in ccj_oracle.c, expected {N_LOOKUPS}"
    left = _LEFT.findall(src)
    assert not left, f"position lookups of the pair table the substitution missed: {left}"
    marker = "} oracle;\n"
    assert src.count(marker) == 1, "the oracle struct's end moved"
    return src.replace(marker, marker + _TABLE + _MPAIR)


def _flags():
    with open(os.path.join(ROOT, "oracle", "Makefile")) as f:
        mk = f.read()
    m = re.search(r"^ORACLE_CFLAGS\s*:=\s*(.+)$", mk, re.M)
    assert m, "ORACLE_CFLAGS left oracle/Makefile"
    return [x.replace("../include", os.path.join(ROOT, "include")) for x in m.group(1).split()]


def masked_lib():
    global _lib
    if _lib is None:
        tmp = tempfile.mkdtemp(prefix="ccj_masked_")
        try:
            c = os.path.join(tmp, "ccj_masked.c")
            so = os.path.join(tmp, "libccj_masked.so")
            with open(c, "w") as f:
                f.write(masked_source())
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
        _lib = L
    return _lib


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


class MaskedFold:
    """The masked restatement's sequential fill for one sequence under the constraint's set F."""

    def __init__(self, seq, blob, dangles=2, noGU=0, unpaired=None, forbid=(), allow_only=None, mask=None):
        L = masked_lib()
        self.n = len(seq)
        if mask is None:
            mask, _ = mask_of(self.n, unpaired, forbid, allow_only)
        assert len(mask) == (self.n + 1) ** 2
        self._blob = ctypes.create_string_buffer(blob, len(blob))
        self._mask = ctypes.create_string_buffer(mask, len(mask))
        L.ccj_masked_set(self._mask)
        try:
            self.h = L.ccj_oracle_fold_pen(seq.encode(), self._blob, dangles, noGU, None)
        finally:
            L.ccj_masked_set(None)
        if not self.h:
            raise MemoryError("oracle allocation failed")

    def hashes(self):
        out = (ctypes.c_uint64 * 31)()
        masked_lib().ccj_oracle_hashes(self.h, out)
        return {HASH_NAMES[i]: "%016x" % out[i] for i in range(31)}

    def get4(self, m, i, j, k, l):
        return masked_lib().ccj_oracle_get4(self.h, m, i, j, k, l)

    def get2(self, m, i, j):
        return masked_lib().ccj_oracle_get2(self.h, m, i, j)

    def W(self, j):
        return masked_lib().ccj_oracle_W(self.h, j)

    def low_stores(self):
        return masked_lib().ccj_oracle_low_stores(self.h)

    def close(self):
        if self.h:
            masked_lib().ccj_oracle_free(self.h)
            self.h = None

    def __del__(self):
        self.close()
