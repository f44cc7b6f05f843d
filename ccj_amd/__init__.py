"""ccj_amd — MI355X-native CCJ pseudoknot MFE engine (host mirror of the reference API).

The reference exposes CCJ through a C++ class and a free function:

    W_final(std::string seq, int dangle);  double W_final::ccj();  std::string W_final::structure
        (reference src/W_final.hh:18-71, src/W_final.cc:20-105)
    std::string ccj(std::string seq, double &energy, int dangle)       (reference src/CCJ.cc:44-49)

This package mirrors that surface in Python on top of libccj_hip.so (include/ccj.h).  The fill
always runs on the GPU through hand-written HIP kernels; there is no CPU fallback — if the
extension is missing or no GPU is visible the calls raise.
"""
from __future__ import annotations

import ctypes
import os
from typing import Optional

__all__ = [
    "W_final", "ccj", "load_params", "load_par", "ParFileError", "param_path", "CCJError", "BacktrackExit", "lib", "MAT4", "MAT2",
    "num_cells", "comm_unique_id", "shard_blocks", "level_layout", "level_schedule", "LevelSchedule",
    "DEFAULT_SPLIT_TARGET", "LocalGroup", "W_final_pf", "PF_MAT4", "PF_MAT2", "layout_extents", "fold_many",
    "SampleExit", "pf_exp_hashes", "load_pfraw", "LockstepBatch", "batch_level_plan", "BatchLevelPlan", "plan_lockstep",
    "pf_many", "PfLockstepBatch", "pf_level_plan", "PF_PLAN_KERNELS", "pf_setup_host_hashes", "PF_SETUP_TABLES", "RangeError", "RANGE_LEVEL", "RANGE_ILOOP", "RANGE_PARTIAL", "RANGE_TAB", "RANGE_CF", "RANGE_EXIT_CODE",
    "il_prune_host", "IL_U", "share_roles", "ShareRoles", "SideRole",
]

_HERE = os.path.dirname(os.path.abspath(__file__))
# CCJ_LIB_VARIANT=dbg selects the bounds-checked debug build (libccj_hip_dbg.so); other variants
# (libccj_hip_<name>.so) are timing-only ablation builds made by tools/ablate.sh.
_VARIANT = os.environ.get("CCJ_LIB_VARIANT", "")
_LIB_PATH = os.path.join(_HERE, "lib", f"libccj_hip_{_VARIANT}.so" if _VARIANT else "libccj_hip.so")
PARAM_DIR = os.path.join(_HERE, "params")

# ccj.h enums
MAT4 = ["PK", "PL", "PR", "PM", "PO", "PfromL", "PfromR", "PfromM", "PfromMprime", "PfromO",
        "PLmloop00", "PLmloop01", "PLmloop10", "PRmloop00", "PRmloop01", "PRmloop10",
        "PMmloop00", "PMmloop01", "PMmloop10", "POmloop00", "POmloop01", "POmloop10"]
MAT2 = ["P", "WBP", "WPP", "V", "Vtype", "WM", "WMv", "WMp"]
HASH_NAMES = MAT4 + MAT2 + ["W"]
# ccj_pf.h enums (partition function)
PF_MAT4 = ["PK", "PL", "PR", "PM", "PO", "PfromL", "PfromR", "PfromM", "PfromO",
           "PLmloop00", "PLmloop01", "PLmloop10", "PRmloop00", "PRmloop01", "PRmloop10",
           "PMmloop00", "PMmloop01", "PMmloop10", "POmloop00", "POmloop01", "POmloop10"]
PF_MAT2 = ["V", "VM", "WM", "WMv", "WMp", "WBP", "WPP", "P"]
CCJ_E_PF_SAMPLE = 8  # include/ccj_pf.h
CCJ_E_PF_RANGE = 10

CCJ_OK, CCJ_E_ARG, CCJ_E_OOM, CCJ_E_HIP, CCJ_E_PARAMS, CCJ_E_BACKTRACK, CCJ_E_STATE, CCJ_E_INTER_EXIT = range(8)
CCJ_E_COMM = 9  # include/ccj.h: band-sharded exchange failed or timed out
CCJ_E_PARFILE = 8  # include/ccj_parfile.h
CCJ_E_RANGE = 11  # include/ccj.h: a 4-D value below -32768, no reference-identical result exists
# include/ccj.h CCJ_RANGE_*: the sites at which a fill saw such a value (W_final.range_flags, RangeError.flags)
RANGE_LEVEL, RANGE_ILOOP, RANGE_PARTIAL, RANGE_TAB, RANGE_CF = 1, 2, 4, 8, 16
RANGE_SITES = {"LEVEL": RANGE_LEVEL, "ILOOP": RANGE_ILOOP, "PARTIAL": RANGE_PARTIAL, "TAB": RANGE_TAB, "CF": RANGE_CF}
# The exit code of a refused fold in fold_many / fold_cli records.  The reference's own paths end
# with 0 (result, "NOT GOOD RESTR INTER"), 1 (EXIT_FAILURE) or 134 (assert): 3 is none of them.
RANGE_EXIT_CODE = 3

# name -> blob file (the reference's params/*.par sets, dumped to our table format)
PARAM_SETS = {
    "Turner04": "Turner04.ccjp", "rna_Turner04": "Turner04.ccjp",
    "DirksPierce09": "DirksPierce09.ccjp", "rna_DirksPierce09": "DirksPierce09.ccjp",
    "DirksPierce03": "DirksPierce03.ccjp", "rna_DirksPierce03": "DirksPierce03.ccjp",
    "CaoChen06": "CaoChen06.ccjp", "rna_CaoChen06": "CaoChen06.ccjp",
    "CaoChen09": "CaoChen09.ccjp", "rna_CaoChen09": "CaoChen09.ccjp",
    "Matthews04": "Matthews04.ccjp", "dna_Matthews04": "Matthews04.ccjp",
    "DNA_Mathews2004": "DNA_Mathews2004.ccjp", "default": "default.ccjp",
}


class CCJError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"ccj error {code}: {msg}")
        self.code = code
        self.msg = msg


class BacktrackExit(CCJError):
    """The reference would have terminated inside its backtrack (stderr text + exit code)."""

    def __init__(self, code: int, msg: str, exit_code: int, stdout: str):
        super().__init__(code, msg)
        self.exit_code = exit_code
        self.stdout = stdout


class RangeError(CCJError):
    """The fold leaves the domain in which a reference-identical result exists (CCJ_E_RANGE): some
    4-D value lies below -32768, where the reference's int16 store wraps.  ``flags``: the RANGE_* bits
    of the sites that saw one.  No structure or energy is reported; the context stays usable."""

    def __init__(self, code: int, msg: str, flags: int):
        super().__init__(code, msg)
        self.flags = flags


class _Problem(ctypes.Structure):
    _fields_ = [("seq", ctypes.c_char_p), ("dangles", ctypes.c_int), ("noGU", ctypes.c_int),
                ("params", ctypes.c_void_p), ("pen", ctypes.c_void_p)]


class _Penalties(ctypes.Structure):
    """include/ccj_params.h ccj_pk_penalties"""
    _fields_ = [(k, ctypes.c_int32) for k in ("PS", "PSM", "PSP", "PB", "PUP", "PPS", "a", "b", "c", "ap", "bp", "cp")] + \
               [("e_stP", ctypes.c_double), ("e_intP", ctypes.c_double)]


PEN_DEFAULT = (-138, 1007, 1500, 246, 6, 96, 339, 3, 2, 341, 56, 12, 0.89, 0.74)  # CCJ_PK_PENALTIES_DEFAULT


class _Options(ctypes.Structure):
    _fields_ = [("device", ctypes.c_int), ("overlap_d2h", ctypes.c_int), ("shard_world", ctypes.c_int),
                ("shard_rank", ctypes.c_int), ("shard_simulate", ctypes.c_int), ("host_traceback", ctypes.c_int),
                ("split_target", ctypes.c_int), ("share_splits", ctypes.c_int)]

class _Constraint(ctypes.Structure):
    """include/ccj.h ccj_constraint"""
    _fields_ = [("unpaired", ctypes.c_char_p), ("forbid", ctypes.POINTER(ctypes.c_int)), ("n_forbid", ctypes.c_int),
                ("allow_only", ctypes.POINTER(ctypes.c_int)), ("n_allow", ctypes.c_int)]


class Constraint:
    """Negative folding constraints for one sequence (include/ccj.h ccj_constraint):
    positions that must stay unpaired and pairs that must not form.  Pairs cannot be forced.

    ``unpaired``: a string of the sequence's length over ``.`` and ``x`` (the ViennaRNA convention);
    ``x`` at position p forbids every pair of p.  ``forbid``: 1-based pairs (i, j), i < j, that must
    not form.  ``allow_only``: if given, only the listed pairs may form at all (before the two above
    are applied).  ``Constraint("..xx..")`` and ``Constraint(forbid=[(2, 9)])`` both work.

    The checks that need no sequence run here (characters, i < j, i >= 1); ``check(n)`` runs the ones
    that need its length, and every call that takes a constraint does so before it touches a context.
    All of them raise ``CCJError(CCJ_E_ARG)``, the code the ABI refuses the same defects with."""

    def __init__(self, unpaired: Optional[str] = None, forbid=(), allow_only=None):
        if unpaired is not None:
            if not isinstance(unpaired, str):
                raise CCJError(CCJ_E_ARG, "constraint: the unpaired string must be a str")
            bad = sorted(set(unpaired) - set(".x"))
            if bad:
                raise CCJError(CCJ_E_ARG, f"constraint: unpaired string has characters other than '.' and 'x': {bad}")
        self.unpaired = unpaired
        self.forbid = self._pairs(forbid, "forbid")
        self.allow_only = None if allow_only is None else self._pairs(allow_only, "allow_only")

    @staticmethod
    def _pairs(pairs, name):
        out = []
        for pr in pairs:
            try:
                i, j = pr
                ok = int(i) == i and int(j) == j
            except (TypeError, ValueError):
                ok = False
            if not ok:
                raise CCJError(CCJ_E_ARG, f"constraint: {name} entry {pr!r} is not a pair of positions")
            i, j = int(i), int(j)
            if i < 1 or i >= j:
                raise CCJError(CCJ_E_ARG, f"constraint: {name} pair ({i}, {j}) is not 1 <= i < j")
            out.append((i, j))
        return tuple(out)

    @classmethod
    def parse(cls, text: str) -> "Constraint":
        """The string form: one character per position, ``.`` free, ``x`` unpaired."""
        return cls(unpaired=text.strip())

    def check(self, n: int) -> "Constraint":
        """Raise unless the constraint fits a sequence of length n."""
        if self.unpaired is not None and len(self.unpaired) != n:
            raise CCJError(CCJ_E_ARG, f"constraint: unpaired string of length {len(self.unpaired)}, sequence of {n}")
        for name, pairs in (("forbid", self.forbid), ("allow_only", self.allow_only or ())):
            for i, j in pairs:
                if j > n:
                    raise CCJError(CCJ_E_ARG, f"constraint: {name} pair ({i}, {j}) outside 1..{n}")
        return self

    def forbidden(self, n: int) -> set:
        """The set F of forbidden position pairs (i, j), i < j, for a sequence of length n."""
        self.check(n)
        F = set()
        if self.allow_only is not None:
            F = {(i, j) for i in range(1, n + 1) for j in range(i + 1, n + 1)} - set(self.allow_only)
        if self.unpaired:
            for p, ch in enumerate(self.unpaired, 1):
                if ch == "x":
                    F |= {(min(p, q), max(p, q)) for q in range(1, n + 1) if q != p}
        return F | set(self.forbid)

    def _c(self):
        """(the ccj_constraint, the buffers it points into)."""
        fb = (ctypes.c_int * max(1, 2 * len(self.forbid)))(*[v for pr in self.forbid for v in pr])
        ao = None
        if self.allow_only is not None:
            ao = (ctypes.c_int * max(1, 2 * len(self.allow_only)))(*[v for pr in self.allow_only for v in pr])
        c = _Constraint(self.unpaired.encode() if self.unpaired is not None else None,
                        ctypes.cast(fb, ctypes.POINTER(ctypes.c_int)), len(self.forbid),
                        ctypes.cast(ao, ctypes.POINTER(ctypes.c_int)) if ao is not None else None,
                        len(self.allow_only) if self.allow_only is not None else 0)
        return c, (fb, ao)

    def __repr__(self):
        return f"Constraint(unpaired={self.unpaired!r}, forbid={list(self.forbid)!r}, allow_only=" \
               f"{None if self.allow_only is None else list(self.allow_only)!r})"


def _cons_arg(constraint, n):
    """A ccj_constraint pointer (or None) for a call, with what must outlive the call."""
    if constraint is None:
        return None, None
    if isinstance(constraint, str):
        constraint = Constraint.parse(constraint)
    if not isinstance(constraint, Constraint):
        raise CCJError(CCJ_E_ARG, "constraint: expected a Constraint, its string form or None")
    c, keep = constraint.check(n)._c()
    return ctypes.byref(c), (c, keep)


COMM_ID_BYTES = 128
DEFAULT_SPLIT_TARGET = 9216  # ccj_host.cc create_impl (include/ccj.h ccj_options.split_target)


class LevelSchedule(tuple):
    """One level's launch regime for one rank (include/ccj.h ccj_level_schedule): sharing (bool),
    split (k_level4d: 1/2/4/8, 0 = no block), lead_split (k_level4d_lead: 2/4/8, 0 = no leader
    launch), g_lo, g_hi (the sharing range)."""
    __slots__ = ()
    sharing = property(lambda s: s[0])
    split = property(lambda s: s[1])
    lead_split = property(lambda s: s[2])
    g_lo = property(lambda s: s[3])
    g_hi = property(lambda s: s[4])
    regime = property(lambda s: (s[1], s[2]))


_lib = None


def lib() -> ctypes.CDLL:
    """Load libccj_hip.so (raises if it has not been built — no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(_LIB_PATH):
        raise CCJError(CCJ_E_STATE, f"{_LIB_PATH} missing: run __graft_entry__.build() first")
    L = ctypes.CDLL(_LIB_PATH)
    vp, ip, cp = ctypes.c_void_p, ctypes.c_int, ctypes.c_char_p
    L.ccj_create.argtypes = [ctypes.POINTER(_Problem), ctypes.POINTER(_Options), ctypes.POINTER(vp)]
    L.ccj_create.restype = ip
    for fn in ("ccj_fill", "ccj_fill_device", "ccj_sync_host", "ccj_n"):
        getattr(L, fn).argtypes = [vp]
        getattr(L, fn).restype = ip
    L.ccj_reset.argtypes = [vp, cp]
    L.ccj_reset.restype = ip
    L.ccj_create_cap.argtypes = [ctypes.POINTER(_Problem), ctypes.POINTER(_Options), ip, ctypes.POINTER(vp)]
    L.ccj_create_cap.restype = ip
    L.ccj_rebind.argtypes = [vp, cp]
    L.ccj_rebind.restype = ip
    L.ccj_capacity.argtypes = [vp]
    L.ccj_capacity.restype = ip
    if hasattr(L, "ccj_rebind_constrained"):  # not in a CCJ_LIB_VARIANT built from an older tree (A/B runs)
        consp = ctypes.POINTER(_Constraint)
        L.ccj_reset_constrained.argtypes = [vp, cp, consp]
        L.ccj_reset_constrained.restype = ip
        L.ccj_rebind_constrained.argtypes = [vp, cp, consp]
        L.ccj_rebind_constrained.restype = ip
        L.ccj_batch_bind_constrained.argtypes = [vp, ctypes.POINTER(cp), ctypes.POINTER(consp), ip]
        L.ccj_batch_bind_constrained.restype = ip
        L.ccj_constraint_count.argtypes = [vp]
        L.ccj_constraint_count.restype = ctypes.c_longlong
        L.ccj_il_prune_host_constrained.argtypes = [ctypes.POINTER(_Problem), consp, ctypes.POINTER(ctypes.c_longlong)] + [vp] * 6
        L.ccj_il_prune_host_constrained.restype = ip
        L.ccj_work_model_seq_constrained.argtypes = [cp, ip, consp, ctypes.POINTER(ctypes.c_double)]
        L.ccj_work_model_seq_constrained.restype = ip
    L.ccj_layout_extents.argtypes = [ip, ip, ip, ip, ip, ctypes.POINTER(ctypes.c_longlong), ip]
    L.ccj_layout_extents.restype = ip
    L.ccj_layout_extent_names.argtypes = []
    L.ccj_layout_extent_names.restype = cp
    L.ccj_fill_async.argtypes = [vp]
    L.ccj_fill_async.restype = ip
    L.ccj_fill_async_after.argtypes = [vp, vp]
    L.ccj_fill_async_after.restype = ip
    L.ccj_wait.argtypes = [vp, cp, ctypes.POINTER(ctypes.c_double), cp, ip]
    L.ccj_wait.restype = ip
    L.ccj_result.argtypes = [vp, cp, ctypes.POINTER(ctypes.c_double), cp, ip]
    L.ccj_result.restype = ip
    L.ccj_get4.argtypes = [vp, ip, ip, ip, ip, ip]
    L.ccj_get4.restype = ip
    L.ccj_get2.argtypes = [vp, ip, ip, ip]
    L.ccj_get2.restype = ip
    L.ccj_getW.argtypes = [vp, ip]
    L.ccj_getW.restype = ip
    L.ccj_hashes.argtypes = [vp, ctypes.POINTER(ctypes.c_uint64)]
    L.ccj_hashes.restype = ip
    L.ccj_last_timing.argtypes = [vp, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double)]
    L.ccj_last_timing.restype = ip
    L.ccj_last_error.argtypes = [vp]
    L.ccj_last_error.restype = cp
    L.ccj_range_flags.argtypes = [vp]
    L.ccj_range_flags.restype = ip
    L.ccj_destroy.argtypes = [vp]
    L.ccj_destroy.restype = None
    L.ccj_num_cells.argtypes = [ip]
    L.ccj_num_cells.restype = ctypes.c_uint64
    L.ccj_host_timing.argtypes = [vp, ctypes.POINTER(ctypes.c_double)]
    L.ccj_host_timing.restype = ip
    L.ccj_iloop_ms.argtypes = [vp]
    L.ccj_iloop_ms.restype = ctypes.c_double
    L.ccj_ppush_ms.argtypes = [vp]
    L.ccj_ppush_ms.restype = ctypes.c_double
    L.ccj_set_timing.argtypes = [vp, ip]
    L.ccj_set_timing.restype = ip
    L.ccj_comm_unique_id.argtypes = [cp]
    L.ccj_comm_unique_id.restype = ip
    L.ccj_comm_init.argtypes = [vp, cp]
    L.ccj_comm_init.restype = ip
    L.ccj_shard_blocks.argtypes = [ip, ip, ip, ip, ctypes.POINTER(ip), ip]
    L.ccj_shard_blocks.restype = ip
    L.ccj_group_create.argtypes = [ip, ctypes.POINTER(vp)]
    L.ccj_group_create.restype = ip
    L.ccj_group_destroy.argtypes = [vp]
    L.ccj_group_destroy.restype = None
    L.ccj_comm_init_local.argtypes = [vp, vp]
    L.ccj_comm_init_local.restype = ip
    L.ccj_level_layout.argtypes = [ip, ip, ip, ctypes.POINTER(ctypes.c_longlong), ctypes.POINTER(ip)]
    L.ccj_level_layout.restype = ip
    L.ccj_level_schedule.argtypes = [ip, ip, ip, ip, ip, ip, ctypes.POINTER(ip)]
    L.ccj_level_schedule.restype = ip
    L.ccj_ctx_level_schedule.argtypes = [vp, ip, ip, ctypes.POINTER(ip)]
    L.ccj_ctx_level_schedule.restype = ip
    if hasattr(L, "ccj_share_roles"):  # not in a CCJ_LIB_VARIANT built from an older tree (A/B runs)
        L.ccj_share_roles.argtypes = [ip, ip, ip, ip, ip, ctypes.POINTER(ip)]
        L.ccj_share_roles.restype = ip
    # lockstep batch
    L.ccj_batch_create.argtypes = [ctypes.POINTER(_Problem), ctypes.POINTER(_Options), ip, ip, ctypes.POINTER(vp)]
    L.ccj_batch_create.restype = ip
    L.ccj_batch_bind.argtypes = [vp, ctypes.POINTER(cp), ip]
    L.ccj_batch_bind.restype = ip
    for fn in ("ccj_batch_fold_async", "ccj_batch_wait", "ccj_batch_members", "ccj_batch_count"):
        getattr(L, fn).argtypes = [vp]
        getattr(L, fn).restype = ip
    L.ccj_batch_member.argtypes = [vp, ip]
    L.ccj_batch_member.restype = vp
    L.ccj_batch_fill_ms.argtypes = [vp]
    L.ccj_batch_fill_ms.restype = ctypes.c_double
    L.ccj_batch_last_error.argtypes = [vp]
    L.ccj_batch_last_error.restype = cp
    L.ccj_batch_level_plan.argtypes = [ctypes.POINTER(ip), ip, ip, ip, ctypes.POINTER(ip)]
    L.ccj_batch_level_plan.restype = ip
    L.ccj_batch_destroy.argtypes = [vp]
    L.ccj_batch_destroy.restype = None
    L.ccj_params_load_par.argtypes = [cp, cp, cp, cp, ip]
    L.ccj_params_load_par.restype = ip
    L.ccj_params_load_par_string.argtypes = [cp, cp, cp, cp, ip]
    L.ccj_params_load_par_string.restype = ip
    # partition function (include/ccj_pf.h)
    u64p, dp = ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_double)
    L.ccj_pf_create.argtypes = [ctypes.POINTER(_Problem), cp, ip, ctypes.POINTER(vp)]
    L.ccj_pf_create.restype = ip
    L.ccj_pf_destroy.argtypes = [vp]
    L.ccj_pf_destroy.restype = None
    # (a CCJ_LIB_VARIANT built from an older tree, as the A side of tools/pf_contexts_ab.py, has no
    # capacity entry points: calling one there is an AttributeError, not a fallback)
    if hasattr(L, "ccj_pf_create_cap"):
        L.ccj_pf_create_cap.argtypes = [ctypes.POINTER(_Problem), cp, ip, ip, ctypes.POINTER(vp)]
        L.ccj_pf_create_cap.restype = ip
        L.ccj_pf_rebind.argtypes = [vp, cp]
        L.ccj_pf_rebind.restype = ip
        L.ccj_pf_reset.argtypes = [vp, cp]
        L.ccj_pf_reset.restype = ip
        L.ccj_pf_capacity.argtypes = [vp]
        L.ccj_pf_capacity.restype = ip
        L.ccj_pf_n.argtypes = [vp]
        L.ccj_pf_n.restype = ip
        L.ccj_pf_keytab_info.argtypes = [vp, dp, ctypes.POINTER(ctypes.c_ulonglong)]
        L.ccj_pf_keytab_info.restype = ip
        L.ccj_pf_setup_hashes.argtypes = [vp, u64p, ip]
        L.ccj_pf_setup_hashes.restype = ip
        L.ccj_pf_setup_host_hashes.argtypes = [ctypes.POINTER(_Problem), cp, u64p, u64p]
        L.ccj_pf_setup_host_hashes.restype = ip
    # (likewise the lockstep batch of the partition function)
    if hasattr(L, "ccj_pf_batch_create"):
        L.ccj_pf_batch_create.argtypes = [ctypes.POINTER(_Problem), cp, ip, ip, ip, ctypes.POINTER(vp)]
        L.ccj_pf_batch_create.restype = ip
        L.ccj_pf_batch_bind.argtypes = [vp, ctypes.POINTER(cp), ip]
        L.ccj_pf_batch_bind.restype = ip
        for fn in ("ccj_pf_batch_fill", "ccj_pf_batch_members", "ccj_pf_batch_count", "ccj_pf_batch_launches"):
            getattr(L, fn).argtypes = [vp]
            getattr(L, fn).restype = ip
        L.ccj_pf_batch_result.argtypes = [vp, ip, dp]
        L.ccj_pf_batch_result.restype = ip
        L.ccj_pf_batch_member.argtypes = [vp, ip]
        L.ccj_pf_batch_member.restype = vp
        L.ccj_pf_batch_fill_ms.argtypes = [vp]
        L.ccj_pf_batch_fill_ms.restype = ctypes.c_double
        L.ccj_pf_batch_item_counts.argtypes = [vp, ip, ctypes.POINTER(ip)]
        L.ccj_pf_batch_item_counts.restype = ip
        L.ccj_pf_batch_last_error.argtypes = [vp]
        L.ccj_pf_batch_last_error.restype = cp
        L.ccj_pf_batch_destroy.argtypes = [vp]
        L.ccj_pf_batch_destroy.restype = None
        L.ccj_pf_level_plan_items.argtypes = [ctypes.POINTER(ip), ctypes.POINTER(ip), ip, ip, ctypes.POINTER(ip)]
        L.ccj_pf_level_plan_items.restype = ip
    # (likewise the candidate-list pruning, absent from an older tree's library)
    if hasattr(L, "ccj_il_counts"):
        L.ccj_il_counts.argtypes = [vp, ctypes.POINTER(ctypes.c_longlong)]
        L.ccj_il_counts.restype = ip
        L.ccj_il_prune_host.argtypes = [ctypes.POINTER(_Problem), ctypes.POINTER(ctypes.c_longlong)] + [vp] * 6
        L.ccj_il_prune_host.restype = ip
    L.ccj_pf_fill.argtypes = [vp, dp]
    L.ccj_pf_fill.restype = ip
    L.ccj_pf_W.argtypes = [vp, dp]
    L.ccj_pf_W.restype = ip
    L.ccj_pf_get2.argtypes = [vp, ip, dp]
    L.ccj_pf_get2.restype = ip
    L.ccj_pf_get4.argtypes = [vp, ip, ip, ip, ip, ip, ctypes.POINTER(ip)]
    L.ccj_pf_get4.restype = ip
    L.ccj_pf_hashes.argtypes = [vp, u64p, u64p]
    L.ccj_pf_hashes.restype = ip
    L.ccj_pf_exp_hashes.argtypes = [vp, u64p, ip]
    L.ccj_pf_exp_hashes.restype = ip
    L.ccj_pf_exp_hashes_params.argtypes = [cp, cp, vp, u64p, ip]
    L.ccj_pf_exp_hashes_params.restype = ip
    L.ccj_pf_exp_names.argtypes = []
    L.ccj_pf_exp_names.restype = cp
    L.ccj_pf_srand.argtypes = [vp, ctypes.c_uint]
    L.ccj_pf_srand.restype = ip
    L.ccj_pf_sample.argtypes = [vp, ip, cp, ctypes.POINTER(ip)]
    L.ccj_pf_sample.restype = ip
    L.ccj_pf_last_message.argtypes = [vp]
    L.ccj_pf_last_message.restype = cp
    L.ccj_pf_timing.argtypes = [vp, ctypes.POINTER(ctypes.c_float)]
    L.ccj_pf_timing.restype = ip
    L.ccj_pf_set_timing.argtypes = [vp, ip]
    L.ccj_pf_set_timing.restype = ip
    L.ccj_pf_kernel_ms.argtypes = [vp, ctypes.POINTER(ctypes.c_double)]
    L.ccj_pf_kernel_ms.restype = ip
    L.ccj_pf_work_model.argtypes = [vp, ctypes.POINTER(ctypes.c_double)]
    L.ccj_pf_work_model.restype = ip
    _lib = L
    return L


def num_cells(n: int) -> int:
    """4-D DP cells C(n+1,4) — the unit of work."""
    if n < 3:
        return 0
    m = n + 1
    return m * (m - 1) * (m - 2) * (m - 3) // 24


IL_U = 29  # ccj_engine.h IE_U: u1, u2 in [0, 28]


def il_prune_host(seq: str, params: str | bytes = "Turner04", dangle: int = 2, noGU: bool = False, pen=None,
                  windows: bool = True, constraint=None):
    """The candidate-list pruning rule on the host, no GPU (include/ccj.h ccj_il_prune_host).

    Returns a dict: ``counts`` = (il kept, il full, ilm kept, ilm full) and, with ``windows``, the numpy
    arrays ``e_il``, ``e_ilm`` (int16) and ``st_il``, ``st_ilm`` (uint8), each [w][p][u1][u2] with p in
    [0, n+2), and the planes ``est``, ``ie`` [w][p]: see the header for the status values.
    ``constraint``: the rule under a Constraint (ccj_il_prune_host_constrained)."""
    import numpy as np
    blob = params if isinstance(params, (bytes, bytearray)) else load_params(params)
    blob_buf = ctypes.create_string_buffer(bytes(blob), len(blob))
    seq_buf = ctypes.create_string_buffer(seq.encode())
    pk = None
    if pen is not None:
        pk = _Penalties(*[int(v) for v in pen[:12]], float(pen[12]), float(pen[13]))
    prob = _Problem(ctypes.cast(seq_buf, ctypes.c_char_p), dangle, 1 if noGU else 0, ctypes.cast(blob_buf, ctypes.c_void_p),
                    ctypes.cast(ctypes.pointer(pk), ctypes.c_void_p) if pk is not None else None)
    n = len(seq)
    counts = (ctypes.c_longlong * 4)()
    out = {}
    ptrs = [None] * 6
    if windows:
        shape = (n + 1, n + 2, IL_U, IL_U)
        for x, (name, dt, sh) in enumerate([("e_il", np.int16, shape), ("e_ilm", np.int16, shape), ("st_il", np.uint8, shape),
                                            ("st_ilm", np.uint8, shape), ("est", np.int16, shape[:2]), ("ie", np.int16, shape[:2])]):
            out[name] = np.zeros(sh, dtype=dt)
            ptrs[x] = out[name].ctypes.data_as(ctypes.c_void_p)
    consp, _keep = _cons_arg(constraint, len(seq))
    if consp is None:
        rc = lib().ccj_il_prune_host(ctypes.byref(prob), counts, *ptrs)
    else:
        rc = lib().ccj_il_prune_host_constrained(ctypes.byref(prob), consp, counts, *ptrs)
    if rc != CCJ_OK:
        raise CCJError(rc, "ccj_il_prune_host")
    out["counts"] = tuple(counts)
    return out


def param_path(name_or_path: str) -> str:
    """Bundled blob for a parameter-set name ("Turner04", "rna_Turner04.par", ...) or a .ccjp path."""
    if os.path.exists(name_or_path) and name_or_path.endswith(".ccjp"):
        return name_or_path
    base = os.path.basename(name_or_path)
    for suf in (".par", ".ccjp"):
        if base.endswith(suf):
            base = base[: -len(suf)]
    if base in PARAM_SETS:
        return os.path.join(PARAM_DIR, PARAM_SETS[base])
    raise CCJError(CCJ_E_ARG, f"unknown parameter set {name_or_path!r}")


class ParFileError(CCJError):
    """A .par file the reference loader rejects: it prints ``log`` on stderr and exits 1."""

    def __init__(self, log: str):
        super().__init__(CCJ_E_PARFILE, log)
        self.log = log


def load_par(path: str, base: bytes | None = None, text: bool = False):
    """Read a ViennaRNA v2.0 parameter file natively (include/ccj_parfile.h).

    ``base`` is the table state the file lands on (default: the reference's compiled-in
    defaults, ccj_amd/params/default.ccjp).  ``text=True`` treats ``path`` as the file contents
    (vrna_params_load_from_string).  Returns (applied, blob, log): applied is 1 when the file was
    parsed, 0 when it could not be opened or was empty (blob == base); log is what the reference
    prints on stderr.  Raises ParFileError where the reference exits 1.
    """
    if base is None:
        base = _read_blob(os.path.join(PARAM_DIR, "default.ccjp"))
    L = lib()
    out = ctypes.create_string_buffer(len(base))
    cap = 1 << 22
    log = ctypes.create_string_buffer(cap)
    fn = L.ccj_params_load_par_string if text else L.ccj_params_load_par
    rc = fn(path.encode(), bytes(base), out, log, cap)
    msg = log.value.decode(errors="replace")
    if rc == CCJ_E_PARFILE:
        raise ParFileError(msg)
    if rc < 0:
        raise CCJError(CCJ_E_ARG, "bad parameter base blob")
    return rc, out.raw, msg


def _read_blob(p: str) -> bytes:
    if p not in _PARAM_CACHE:
        with open(p, "rb") as f:
            _PARAM_CACHE[p] = f.read()
    return _PARAM_CACHE[p]


_PARAM_CACHE: dict = {}


def load_params(name_or_path: str = "DirksPierce09") -> bytes:
    """Scaled 37 C energy tables (include/ccj_params.h).

    An existing .par file is read natively over the compiled-in defaults (like the reference's
    vrna_params_load); an existing .ccjp is used as is; otherwise the name selects one of the
    bundled sets (Turner04, DirksPierce09, ... — dumps of the reference's own files).
    """
    if os.path.isfile(name_or_path) and not name_or_path.endswith(".ccjp"):
        key = ("par", os.path.abspath(name_or_path), os.path.getmtime(name_or_path))
        if key not in _PARAM_CACHE:
            _PARAM_CACHE[key] = load_par(name_or_path)[1]
        return _PARAM_CACHE[key]
    return _read_blob(param_path(name_or_path))


class W_final:
    """Mirror of the reference class W_final (src/W_final.hh:18-71).

    ``W_final(seq, dangle).ccj()`` fills every matrix on the GPU, runs W + backtrack on the host
    mirror and returns the MFE in kcal/mol; ``structure`` holds the dot-bracket string.
    """

    def __init__(self, seq: str, dangle: int = 2, params: str | bytes = "DirksPierce09",
                 noGU: bool = False, device: int = 0, overlap_d2h: bool = False, shard_world: int = 1,
                 shard_rank: int = 0, shard_simulate: bool = False, comm_id: Optional[bytes] = None,
                 host_traceback: bool = False, split_target: int = 0, share_splits: int = 0,
                 local_group: Optional["LocalGroup"] = None, pen=None, capacity: Optional[int] = None,
                 constraint: Optional["Constraint"] = None):
        """shard_world > 1: band-shard this one sequence over shard_world processes (one per GPU),
        exchanging each level over RCCL; every rank passes the same comm_id (from comm_unique_id()
        on one rank), or the same local_group when the ranks are contexts of this process.
        shard_simulate runs all shards in this one context without an exchange.
        host_traceback: run W and the traceback on the host over a mirror of every matrix (the
        same node logic, host executor; overlap_d2h streams that mirror during the fill) instead of on the GPU.
        split_target / share_splits: level-kernel tuning (include/ccj.h ccj_options; 0 = default,
        < 0 = never split a level / no split-point sharing).
        pen: the pseudoknot penalties (include/ccj_params.h ccj_pk_penalties), 14 values in the
        struct's order: PS PSM PSP PB PUP PPS a b c ap bp cp (ints) e_stP e_intP (floats); None =
        the reference's h_globals.hh defaults (PEN_DEFAULT).
        capacity: allocate for every length 1 .. capacity (include/ccj.h ccj_create_cap), so that
        rebind() can bind sequences of other lengths; None = the length of seq.
        constraint: a Constraint (or its string form) for this binding: positions that must stay
        unpaired, pairs that must not form (include/ccj.h ccj_rebind_constrained).  A band-sharded fold
        needs the same constraint on every rank.  The context is created on the unconstrained sequence
        and then rebound under the constraint (the ABI has no constrained constructor), so a constrained
        constructor pays the sequence setup, with its wait for the work-item counts, twice; reset() and
        rebind() with a constraint pay it once."""
        consp, _keep = _cons_arg(constraint, len(seq))  # a bad constraint is refused before anything is allocated
        self.seq = seq
        self.n = len(seq)
        self.dangle = dangle
        self._blob = params if isinstance(params, (bytes, bytearray)) else load_params(params)
        self._blob_buf = ctypes.create_string_buffer(bytes(self._blob), len(self._blob))
        self._seq_buf = ctypes.create_string_buffer(seq.encode())
        L = lib()
        self._pen = None
        if pen is not None:
            if len(pen) != 14:
                raise CCJError(CCJ_E_ARG, "pen needs the 14 values of ccj_pk_penalties")
            self._pen = _Penalties(*[int(v) for v in pen[:12]], float(pen[12]), float(pen[13]))
        prob = _Problem(ctypes.cast(self._seq_buf, ctypes.c_char_p), dangle, 1 if noGU else 0,
                        ctypes.cast(self._blob_buf, ctypes.c_void_p),
                        ctypes.cast(ctypes.pointer(self._pen), ctypes.c_void_p) if self._pen is not None else None)
        opts = _Options(device, 1 if overlap_d2h else 0, shard_world, shard_rank, 1 if shard_simulate else 0,
                        1 if host_traceback else 0, split_target, share_splits)
        h = ctypes.c_void_p()
        if capacity is None:
            rc = L.ccj_create(ctypes.byref(prob), ctypes.byref(opts), ctypes.byref(h))
        else:
            rc = L.ccj_create_cap(ctypes.byref(prob), ctypes.byref(opts), int(capacity), ctypes.byref(h))
        if rc != CCJ_OK:
            raise CCJError(rc, L.ccj_last_error(None).decode())
        self._h = h
        if consp is not None:
            self._check(L.ccj_rebind_constrained(h, seq.encode(), consp))
        if shard_world > 1 and not shard_simulate and local_group is not None:
            self._group = local_group  # keeps the group alive as long as this context
            self._check(L.ccj_comm_init_local(h, local_group._h))
        elif shard_world > 1 and not shard_simulate:
            if comm_id is None or len(comm_id) != COMM_ID_BYTES:
                raise CCJError(CCJ_E_ARG, "sharded context needs the 128-byte comm_id of rank 0")
            self._check(L.ccj_comm_init(h, comm_id))
        self.structure: Optional[str] = None
        self.energy: Optional[float] = None
        self.stdout_msgs = ""

    def reset(self, seq: str, constraint: Optional["Constraint"] = None) -> None:
        """Rebind this context to another sequence of the same length (include/ccj.h ccj_reset):
        the allocations are reused, only the sequence tables and work lists are rebuilt.  The binding
        carries `constraint` and nothing of an earlier one (None: an unconstrained fold)."""
        if len(seq) != self.n:
            raise CCJError(CCJ_E_ARG, f"reset: length {len(seq)} differs from n={self.n}")
        consp, _keep = _cons_arg(constraint, len(seq))
        if consp is None:
            self._check(lib().ccj_reset(self._h, seq.encode()))
        else:
            self._check(lib().ccj_reset_constrained(self._h, seq.encode(), consp))
        self.seq = seq
        self._seq_buf = ctypes.create_string_buffer(seq.encode())
        self.structure = None
        self.energy = None
        self.stdout_msgs = ""

    def rebind(self, seq: str, constraint: Optional["Constraint"] = None) -> None:
        """Bind this context to another sequence of any length up to its capacity (include/ccj.h
        ccj_rebind): nothing is allocated; with the bound length it is reset()."""
        consp, _keep = _cons_arg(constraint, len(seq))
        if consp is None:
            self._check(lib().ccj_rebind(self._h, seq.encode()))
        else:
            self._check(lib().ccj_rebind_constrained(self._h, seq.encode(), consp))
        self.seq = seq
        self.n = len(seq)
        self._seq_buf = ctypes.create_string_buffer(seq.encode())
        self.structure = None
        self.energy = None
        self.stdout_msgs = ""

    @property
    def capacity(self) -> int:
        """The longest sequence this context can be bound to (ccj_capacity)."""
        return lib().ccj_capacity(self._h)

    def constraint_count(self) -> int:
        """Pairs the binding's constraint forbids among those whose bases could pair
        (ccj_constraint_count); 0 for an unconstrained binding."""
        return lib().ccj_constraint_count(self._h)

    def _check(self, rc: int):
        if rc == CCJ_E_RANGE:
            raise RangeError(rc, lib().ccj_last_error(self._h).decode(), self.range_flags())
        if rc != CCJ_OK:
            raise CCJError(rc, lib().ccj_last_error(self._h).decode())

    def range_flags(self) -> int:
        """The RANGE_* bits of the last fill (include/ccj.h ccj_range_flags): 0 inside the domain of
        bit-identity.  Non-zero after a RangeError, and after a fold that CCJ_ALLOW_OUT_OF_RANGE=1 let
        complete under the engine's clamp-only semantics."""
        return lib().ccj_range_flags(self._h)

    def il_counts(self):
        """(il kept, il full, ilm kept, ilm full): entries of the last fill's interior-loop candidate
        lists after and before pruning (include/ccj.h ccj_il_counts; CCJ_IL_PRUNE=0 keeps them all)."""
        out = (ctypes.c_longlong * 4)()
        self._check(lib().ccj_il_counts(self._h, out))
        return tuple(out)

    def fill(self):
        self._check(lib().ccj_fill(self._h))

    def fill_device(self):
        self._check(lib().ccj_fill_device(self._h))

    def sync_host(self):
        self._check(lib().ccj_sync_host(self._h))

    def result(self):
        L = lib()
        buf = ctypes.create_string_buffer(self.n + 1)
        msgs = ctypes.create_string_buffer(1 << 16)
        e = ctypes.c_double()
        rc = L.ccj_result(self._h, buf, ctypes.byref(e), msgs, 1 << 16)
        self.stdout_msgs = msgs.value.decode()
        if rc == CCJ_E_BACKTRACK or rc == CCJ_E_INTER_EXIT:
            err = L.ccj_last_error(self._h).decode()
            exit_code = 0 if rc == CCJ_E_INTER_EXIT else (134 if "Assertion" in err else 1)
            raise BacktrackExit(rc, err, exit_code, self.stdout_msgs)
        self._check(rc)
        self.structure = buf.value.decode()
        self.energy = e.value
        return self.energy

    def ccj(self) -> float:
        """reference W_final::ccj (W_final.cc:58-105)"""
        self.fill()
        return self.result()

    def fill_async(self, after: Optional["W_final"] = None) -> None:
        """Enqueue fill + W + traceback and return at once (include/ccj.h ccj_fill_async); with
        `after`, the fill starts when that context's last enqueued fill has ended."""
        if after is None:
            self._check(lib().ccj_fill_async(self._h))
        else:
            self._check(lib().ccj_fill_async_after(self._h, after._h))

    def wait(self) -> float:
        """Finish a fill_async: same results (and exceptions) as ccj()."""
        L = lib()
        buf = ctypes.create_string_buffer(self.n + 1)
        msgs = ctypes.create_string_buffer(1 << 16)
        e = ctypes.c_double()
        rc = L.ccj_wait(self._h, buf, ctypes.byref(e), msgs, 1 << 16)
        self.stdout_msgs = msgs.value.decode()
        if rc == CCJ_E_BACKTRACK or rc == CCJ_E_INTER_EXIT:
            err = L.ccj_last_error(self._h).decode()
            exit_code = 0 if rc == CCJ_E_INTER_EXIT else (134 if "Assertion" in err else 1)
            raise BacktrackExit(rc, err, exit_code, self.stdout_msgs)
        self._check(rc)
        self.structure = buf.value.decode()
        self.energy = e.value
        return self.energy

    # ---- matrix access (reference getter semantics) ----
    def get4(self, mat, i, j, k, l) -> int:
        m = MAT4.index(mat) if isinstance(mat, str) else mat
        return lib().ccj_get4(self._h, m, i, j, k, l)

    def get2(self, mat, i, j) -> int:
        m = MAT2.index(mat) if isinstance(mat, str) else mat
        return lib().ccj_get2(self._h, m, i, j)

    def W(self, j) -> int:
        return lib().ccj_getW(self._h, j)

    def hashes(self) -> dict:
        out = (ctypes.c_uint64 * len(HASH_NAMES))()
        self._check(lib().ccj_hashes(self._h, out))
        return {name: "%016x" % out[x] for x, name in enumerate(HASH_NAMES)}

    def level_schedule(self, t: int, rank: int = -1) -> LevelSchedule:
        """The launch regime this context runs level t in (include/ccj.h ccj_ctx_level_schedule),
        from the split target and share flag it resolved (options and environment); rank: another
        rank's launches in a shard_simulate context (default: this context's own)."""
        out = (ctypes.c_int * 7)()
        self._check(lib().ccj_ctx_level_schedule(self._h, t, rank, out))
        return LevelSchedule((bool(out[0]), out[1], out[2], out[3], out[4]))

    def schedule_options(self):
        """(split_target, share) as this context resolved them (0 = never split)."""
        out = (ctypes.c_int * 7)()
        self._check(lib().ccj_ctx_level_schedule(self._h, 0, -1, out))
        return out[5], bool(out[6])

    def set_timing(self, mode: int) -> None:
        """What later ccj() calls time: 0 = the fill; 1 (default) = + level durations; 2 = + per-kernel
        family times (k_diag2d, k_iloop) from extra marker events, which slow the fill down."""
        self._check(lib().ccj_set_timing(self._h, mode))

    def timing(self) -> dict:
        f = ctypes.c_double()
        k = (ctypes.c_double * 3)()
        lib().ccj_last_timing(self._h, ctypes.byref(f), k)
        hst = (ctypes.c_double * 3)()
        lib().ccj_host_timing(self._h, hst)
        L = lib()
        return {"fill_ms": f.value, "level4d_ms": k[0], "iloop_ms": L.ccj_iloop_ms(self._h), "diag2d_ms": k[1],
                "ppush_ms": L.ccj_ppush_ms(self._h),
                "precompute_ms": k[2],
                "host_mirror_wait_ms": hst[0], "W_ms": hst[1], "backtrack_ms": hst[2]}

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            lib().ccj_destroy(self._h)  # ignores a lockstep batch's member: LockstepBatch.close frees it
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class BatchLevelPlan(tuple):
    """The batched k_level4d launch of one level (include/ccj.h ccj_batch_level_plan): split (1/2/4/8,
    0 = no member has the level), threads per block, dynamic LDS bytes, grid x, and per member
    (workgroups, 64-cell chunks per a-block)."""
    __slots__ = ()
    split = property(lambda s: s[0])
    threads = property(lambda s: s[1])
    lds = property(lambda s: s[2])
    grid_x = property(lambda s: s[3])
    members = property(lambda s: s[4])


def batch_level_plan(lengths, t: int, split_target: int = DEFAULT_SPLIT_TARGET) -> BatchLevelPlan:
    """The one launch a lockstep batch makes for level t of members of these lengths (no GPU needed).
    split_target is the resolved target: 0 = never split."""
    lengths = [int(x) for x in lengths]
    n = (ctypes.c_int * len(lengths))(*lengths)
    out = (ctypes.c_int * (4 + 2 * len(lengths)))()
    rc = lib().ccj_batch_level_plan(n, len(lengths), t, split_target, out)
    if rc != CCJ_OK:
        raise CCJError(rc, "bad plan arguments")
    return BatchLevelPlan((out[0], out[1], out[2], out[3],
                           tuple((out[4 + 2 * k], out[5 + 2 * k]) for k in range(len(lengths)))))


class LockstepBatch:
    """`members` capacity contexts folded in lockstep (include/ccj.h ccj_batch): bind(seqs) gives
    member k the k-th sequence, fold() runs every bound member's fill, W and traceback in one set of
    level launches.  Afterwards each bound member (a W_final over the borrowed context) has
    structure / energy / stdout_msgs set, or `exit` = its BacktrackExit where the reference's
    backtrack would have exited, or `refused` = its RangeError where the fold leaves the domain of
    bit-identity (the other members are untouched); result(), hashes(), W(), get2 and get4 work on it."""

    def __init__(self, capacity: int, members: int, dangle: int = 2, params: str | bytes = "DirksPierce09",
                 noGU: bool = False, device: int = 0, pen=None, **engine):
        self._blob = params if isinstance(params, (bytes, bytearray)) else load_params(params)
        self._blob_buf = ctypes.create_string_buffer(bytes(self._blob), len(self._blob))
        L = lib()
        self._pen = None
        if pen is not None:
            if len(pen) != 14:
                raise CCJError(CCJ_E_ARG, "pen needs the 14 values of ccj_pk_penalties")
            self._pen = _Penalties(*[int(v) for v in pen[:12]], float(pen[12]), float(pen[13]))
        prob = _Problem(None, dangle, 1 if noGU else 0, ctypes.cast(self._blob_buf, ctypes.c_void_p),
                        ctypes.cast(ctypes.pointer(self._pen), ctypes.c_void_p) if self._pen is not None else None)
        unknown = set(engine) - {"overlap_d2h", "shard_world", "shard_rank", "shard_simulate", "host_traceback",
                                 "split_target", "share_splits"}
        if unknown:
            raise TypeError(f"LockstepBatch: unknown options {sorted(unknown)}")
        opts = _Options(device, 1 if engine.get("overlap_d2h") else 0, engine.get("shard_world", 1), engine.get("shard_rank", 0),
                        1 if engine.get("shard_simulate") else 0, 1 if engine.get("host_traceback") else 0,
                        engine.get("split_target", 0), engine.get("share_splits", 0))
        h = ctypes.c_void_p()
        rc = L.ccj_batch_create(ctypes.byref(prob), ctypes.byref(opts), int(capacity), int(members), ctypes.byref(h))
        if rc != CCJ_OK:
            raise CCJError(rc, L.ccj_batch_last_error(None).decode())
        self._h = h
        self.capacity = int(capacity)
        self.dangle = dangle
        self._all = []
        for k in range(int(members)):
            wf = W_final.__new__(W_final)
            wf._h = ctypes.c_void_p(L.ccj_batch_member(h, k))
            wf._blob, wf._blob_buf, wf._pen = self._blob, self._blob_buf, self._pen
            wf.seq, wf.n, wf.dangle = "", 0, dangle
            wf.structure = wf.energy = wf.exit = wf.refused = None
            wf.stdout_msgs = ""
            self._all.append(wf)
        self.count = 0

    @property
    def members(self) -> list:
        """The bound members, in the order of the last bind()."""
        return self._all[: self.count]

    @property
    def size(self) -> int:
        return len(self._all)

    def _check(self, rc: int):
        if rc != CCJ_OK:
            raise CCJError(rc, lib().ccj_batch_last_error(self._h).decode())

    def bind(self, seqs, constraints=None) -> None:
        """Member k folds seqs[k]; constraints: None, or one entry per sequence, each a Constraint
        (or its string form) or None (include/ccj.h ccj_batch_bind_constrained)."""
        seqs = [str(s) for s in seqs]
        arr = (ctypes.c_char_p * max(len(seqs), 1))(*[s.encode() for s in seqs])
        if constraints is None:
            self._check(lib().ccj_batch_bind(self._h, arr, len(seqs)))
        else:
            constraints = list(constraints)
            if len(constraints) != len(seqs):
                raise CCJError(CCJ_E_ARG, f"bind: {len(constraints)} constraints for {len(seqs)} sequences")
            args = [_cons_arg(c, len(s)) for c, s in zip(constraints, seqs)]  # refused before any member moves
            carr = (ctypes.POINTER(_Constraint) * max(len(seqs), 1))(
                *[ctypes.pointer(keep[0]) if keep is not None else None for _, keep in args])
            self._check(lib().ccj_batch_bind_constrained(self._h, arr, carr, len(seqs)))
        self.count = len(seqs)
        for wf, s in zip(self._all, seqs):
            wf.seq, wf.n = s, len(s)
            wf._seq_buf = ctypes.create_string_buffer(s.encode())
            wf.structure = wf.energy = wf.exit = wf.refused = None
            wf.stdout_msgs = ""

    def fold_async(self) -> None:
        self._check(lib().ccj_batch_fold_async(self._h))

    def wait(self) -> None:
        self._check(lib().ccj_batch_wait(self._h))
        for wf in self.members:
            wf.exit = wf.refused = None
            try:
                wf.result()
            except BacktrackExit as ex:
                wf.structure = wf.energy = None
                wf.exit = ex
            except RangeError as ex:
                wf.structure = wf.energy = None
                wf.refused = ex

    def fold(self) -> None:
        self.fold_async()
        self.wait()

    def fill_ms(self) -> float:
        return lib().ccj_batch_fill_ms(self._h)

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            for wf in self._all:
                wf._h = ctypes.c_void_p()
            lib().ccj_batch_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def plan_lockstep(lengths, k: int) -> list:
    """The runs fold_many(lockstep=k) folds: the input indices sorted by length (ties in input
    order) and cut into runs of at most k neighbours, so that the members of one batch have similar
    lengths.  Pure; every index appears exactly once."""
    k = max(1, int(k))
    order = sorted(range(len(lengths)), key=lambda x: (lengths[x], x))
    return [order[p: p + k] for p in range(0, len(order), k)]


def comm_unique_id() -> bytes:
    """A fresh RCCL unique id for a sharded fold (broadcast it to every rank)."""
    buf = ctypes.create_string_buffer(COMM_ID_BYTES)
    rc = lib().ccj_comm_unique_id(buf)
    if rc != CCJ_OK:
        raise CCJError(rc, "ncclGetUniqueId failed")
    return buf.raw


def shard_blocks(n: int, t: int, world: int, rank: int):
    """a-blocks of 4-D level t that rank computes in a band-sharded fold, ascending (no GPU needed):
    block a belongs to rank (a // 4) % world on every level."""
    cap = t + 1
    buf = (ctypes.c_int * max(cap, 1))()
    cnt = lib().ccj_shard_blocks(n, t, world, rank, buf, cap)
    if cnt < 0:
        raise CCJError(-cnt, "bad shard arguments")
    return list(buf[:cnt])


class LocalGroup:
    """In-process exchange group for a band-sharded fold whose ranks are contexts of this process
    (include/ccj.h ccj_group): pass it as W_final(..., shard_world=N, shard_rank=r, local_group=g)
    and drive each rank's fill from its own thread."""

    def __init__(self, world: int):
        h = ctypes.c_void_p()
        rc = lib().ccj_group_create(world, ctypes.byref(h))
        if rc != CCJ_OK:
            raise CCJError(rc, "ccj_group_create failed")
        self._h = h
        self.world = world

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            lib().ccj_group_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def level_layout(n: int, t: int, world: int):
    """(C_t, M_t): per-matrix element stride of level t (padded to world equal chunks), a-block size."""
    C, M = ctypes.c_longlong(), ctypes.c_int()
    rc = lib().ccj_level_layout(n, t, world, ctypes.byref(C), ctypes.byref(M))
    if rc != CCJ_OK:
        raise CCJError(rc, "bad layout arguments")
    return C.value, M.value


def level_schedule(n: int, t: int, world: int = 1, rank: int = 0, split_target: int = DEFAULT_SPLIT_TARGET,
                   share: bool = True) -> LevelSchedule:
    """The launch regime of level t for one rank (no GPU needed; include/ccj.h ccj_level_schedule).
    split_target is the resolved target: 0 = never split (what the option's -1 means)."""
    out = (ctypes.c_int * 5)()
    rc = lib().ccj_level_schedule(n, t, world, rank, split_target, 1 if share else 0, out)
    if rc != CCJ_OK:
        raise CCJError(rc, "bad schedule arguments")
    return LevelSchedule((bool(out[0]), out[1], out[2], out[3], out[4]))


class SideRole(tuple):
    """One side (a-loop or b-loop) of a cell's split-point sharing (include/ccj.h ccj_share_roles):
    role (0 full scan, 1 leader, 2 follower), low, top (the split points 1 .. low and the top `top`
    of its range the cell scans itself), cuts (a leader's cut for followers r = 1, 2, 3)."""
    __slots__ = ()
    role = property(lambda s: s[0])
    low = property(lambda s: s[1])
    top = property(lambda s: s[2])
    cuts = property(lambda s: s[3])


class ShareRoles(tuple):
    """a-block a of level t: a_side, b_side (SideRole), in_lead (k_level4d_lead runs the block),
    sharing, g_lo, g_hi."""
    __slots__ = ()
    a_side = property(lambda s: s[0])
    b_side = property(lambda s: s[1])
    in_lead = property(lambda s: s[2])
    sharing = property(lambda s: s[3])
    g_lo = property(lambda s: s[4])
    g_hi = property(lambda s: s[5])


def share_roles(n: int, t: int, a: int, split_target: int = DEFAULT_SPLIT_TARGET, edges: bool = True) -> ShareRoles:
    """The sharing roles of a-block a of level t (no GPU needed; include/ccj.h ccj_share_roles).
    split_target is the resolved target: 0 = never split (what the option's -1 means)."""
    out = (ctypes.c_int * 16)()
    rc = lib().ccj_share_roles(n, t, a, split_target, 1 if edges else 0, out)
    if rc != CCJ_OK:
        raise CCJError(rc, "bad role arguments")
    sides = [SideRole((out[o], out[o + 1], out[o + 2], (out[o + 3], out[o + 4], out[o + 5]))) for o in (0, 6)]
    return ShareRoles((sides[0], sides[1], bool(out[12]), bool(out[13]), out[14], out[15]))


def layout_extents(n: int, split_target: int = DEFAULT_SPLIT_TARGET, share: bool = True, full4: bool = False,
                   as_capacity: bool = False) -> dict:
    """Element counts of every device buffer whose size depends on n (no GPU needed; include/ccj.h
    ccj_layout_extents): what a binding of n uses, or with as_capacity what a context of capacity n
    allocates.  split_target is the resolved target (0 = never split)."""
    L = lib()
    names = L.ccj_layout_extent_names().decode().split()
    out = (ctypes.c_longlong * len(names))()
    got = L.ccj_layout_extents(n, split_target, 1 if share else 0, 1 if full4 else 0, 1 if as_capacity else 0, out, len(names))
    if got != len(names):
        raise CCJError(CCJ_E_ARG, "bad layout arguments")
    return dict(zip(names, out))


def _fold_many_lockstep(seqs, k, dangle, params, noGU, device, capacity, pen, engine, constraints=None) -> list:
    runs = plan_lockstep([len(s) for s in seqs], k)
    cap = max(len(s) for s in seqs) if capacity is None else int(capacity)
    out: list = [None] * len(seqs)
    batch = LockstepBatch(cap, min(max(1, int(k)), len(seqs)), dangle, params=params, noGU=noGU, device=device, pen=pen, **engine)
    try:
        for run in runs:
            batch.bind([seqs[x] for x in run], None if constraints is None else [constraints[x] for x in run])
            batch.fold()
            for x, wf in zip(run, batch.members):
                if wf.refused is not None:
                    out[x] = (seqs[x], None, None, "", RANGE_EXIT_CODE, wf.refused.msg)
                elif wf.exit is None:
                    out[x] = (seqs[x], wf.structure, wf.energy, wf.stdout_msgs, 0, "")
                else:
                    out[x] = (seqs[x], None, None, wf.exit.stdout, wf.exit.exit_code, wf.exit.msg)
    finally:
        batch.close()
    return out


def fold_many(seqs, dangle: int = 2, params: str | bytes = "DirksPierce09", noGU: bool = False, device: int = 0,
              contexts: int = 2, capacity: Optional[int] = None, pen=None, lockstep: int = 0, constraints=None,
              **engine) -> list:
    """Fold sequences of mixed lengths through `contexts` capacity contexts (capacity: the longest
    sequence by default), kept in flight with rebind + fill_async / wait: while one context's
    traceback runs, the next context's fill has the GPU.  Returns one record per sequence, in input
    order: (seq, structure, energy, stdout_msgs, exit_code, stderr).  A reference backtrack exit is
    a record with structure and energy None, its exit code and stderr text; it does not disturb the
    other folds.  Neither does a fold refused with RangeError (possible under non-default pen only):
    its record is (seq, None, None, "", RANGE_EXIT_CODE, message).  engine: further W_final options (split_target, share_splits, host_traceback, ...).
    lockstep=K > 0: instead, sort by length, cut into runs of K neighbours (plan_lockstep) and fold each
    run as one LockstepBatch, which pays every level's launches once per run; the same records, in
    input order.
    constraints: None, or one entry per sequence (a Constraint, its string form, or None), on either
    path; every entry is checked against its sequence before the first fold starts."""
    seqs = list(seqs)
    if not seqs:
        return []
    if constraints is not None:
        constraints = [Constraint.parse(c) if isinstance(c, str) else c for c in constraints]
        if len(constraints) != len(seqs):
            raise CCJError(CCJ_E_ARG, f"fold_many: {len(constraints)} constraints for {len(seqs)} sequences")
        for c, s in zip(constraints, seqs):
            _cons_arg(c, len(s))
    if lockstep and int(lockstep) > 0:
        return _fold_many_lockstep(seqs, int(lockstep), dangle, params, noGU, device, capacity, pen, engine, constraints)
    cap = max(len(s) for s in seqs) if capacity is None else int(capacity)
    k = max(1, min(int(contexts), len(seqs)))
    out: list = [None] * len(seqs)
    ctx: list = []      # the contexts, created on their first sequence
    flying: list = []   # (context, input index) in enqueue order

    def finish(wf, x):
        try:
            e = wf.wait()
            out[x] = (seqs[x], wf.structure, e, wf.stdout_msgs, 0, "")
        except BacktrackExit as ex:
            out[x] = (seqs[x], None, None, ex.stdout, ex.exit_code, ex.msg)
        except RangeError as ex:
            out[x] = (seqs[x], None, None, "", RANGE_EXIT_CODE, ex.msg)

    try:
        for x, s in enumerate(seqs):
            if len(ctx) < k:
                wf = W_final(s, dangle, params=params, noGU=noGU, device=device, pen=pen, capacity=cap,
                             constraint=None if constraints is None else constraints[x], **engine)
                ctx.append(wf)
            else:
                wf, done = flying.pop(0)  # the oldest fold in flight: its context is the next free one
                finish(wf, done)
                wf.rebind(s, None if constraints is None else constraints[x])
            wf.fill_async()
            flying.append((wf, x))
        while flying:
            wf, done = flying.pop(0)
            finish(wf, done)
    finally:
        for wf, _ in flying:  # an error above: let the folds in flight end before their contexts close
            try:
                wf.wait()
            except CCJError:
                pass
        for wf in ctx:
            wf.close()
    return out


def ccj(seq: str, dangle: int = 2, params: str | bytes = "DirksPierce09", noGU: bool = False,
        device: int = 0):
    """reference ``std::string ccj(std::string seq, double &energy, int dangle)`` (CCJ.cc:44-49).

    Returns (structure, energy_kcal_per_mol).
    """
    wf = W_final(seq, dangle, params=params, noGU=noGU, device=device)
    try:
        energy = wf.ccj()
        return wf.structure, energy
    finally:
        wf.close()


def load_pfraw(name_or_path) -> Optional[bytes]:
    """Raw (unclamped) dangle / mismatch tables of a bundled set (ccj_amd/params/<set>.pfraw,
    include/ccj_pf.h ccj_pf_raw), or None (the engine then takes the pair-type-0 rows as INF)."""
    if not isinstance(name_or_path, str):
        return None
    if os.path.isfile(name_or_path) and not name_or_path.endswith(".ccjp"):
        return None  # a .par file read natively: no raw tables (type-0 rows taken as INF)
    try:
        p = param_path(name_or_path)
    except Exception:
        return None
    raw = p[:-5] + ".pfraw" if p.endswith(".ccjp") else None
    if raw and os.path.exists(raw):
        return _read_blob(raw)
    return None


def pf_exp_hashes(params: str | bytes = "DirksPierce09") -> dict:
    """FNV-1a of the partition function's Boltzmann tables for a parameter set (host only)."""
    blob = params if isinstance(params, (bytes, bytearray)) else load_params(params)
    raw = load_pfraw(params)
    names = lib().ccj_pf_exp_names().decode().split()
    out = (ctypes.c_uint64 * len(names))()
    got = lib().ccj_pf_exp_hashes_params(bytes(blob), raw, None, out, len(names))
    if got != len(names):
        raise CCJError(CCJ_E_ARG, "ccj_pf_exp_hashes_params")
    return {k: "%016x" % v for k, v in zip(names, out)}


class SampleExit(CCJError):
    """A Sample_* failure path of the reference (it prints ``stdout`` and calls exit(0))."""

    def __init__(self, msg: str, structures: list):
        super().__init__(CCJ_E_PF_SAMPLE, msg)
        self.stdout = msg
        self.structures = structures


PF_SETUP_TABLES = ["pt", "est", "hp", "items", "ieO", "ieI", "mO", "mI"]  # ccj_pf_setup_hashes


def _pf_problem(seq, dangle, params, noGU, pen):
    """A ccj_problem for the partition function and the buffers it points into (keep them alive)."""
    blob = params if isinstance(params, (bytes, bytearray)) else load_params(params)
    blob_buf = ctypes.create_string_buffer(bytes(blob), len(blob))
    seq_buf = ctypes.create_string_buffer(seq.encode()) if seq is not None else None
    pen_s = None
    if pen is not None:
        if len(pen) != 14:
            raise CCJError(CCJ_E_ARG, "pen needs the 14 values of ccj_pk_penalties")
        pen_s = _Penalties(*[int(v) for v in pen[:12]], float(pen[12]), float(pen[13]))
    prob = _Problem(ctypes.cast(seq_buf, ctypes.c_char_p) if seq_buf is not None else None, dangle, 1 if noGU else 0,
                    ctypes.cast(blob_buf, ctypes.c_void_p),
                    ctypes.cast(ctypes.pointer(pen_s), ctypes.c_void_p) if pen_s is not None else None)
    return prob, (blob_buf, seq_buf, pen_s)


def pf_setup_host_hashes(seq: str, dangle: int = 2, params: str | bytes = "DirksPierce09", noGU: bool = False,
                         pen=None) -> tuple:
    """No GPU: FNV hashes of a problem's setup tables (est, ieO, ieI, mO, mI; the windows over the
    intervals whose pair can pair) built two ways — one pow per entry, and through the key tables
    and the gather functions the setup kernels share (ccj_pf_setup_host_hashes).  (direct, keyed)."""
    prob, keep = _pf_problem(seq, dangle, params, noGU, pen)
    names = ["est", "ieO", "ieI", "mO", "mI"]
    a, b = (ctypes.c_uint64 * 5)(), (ctypes.c_uint64 * 5)()
    rc = lib().ccj_pf_setup_host_hashes(ctypes.byref(prob), load_pfraw(params), a, b)
    if rc != CCJ_OK:
        raise CCJError(rc, "ccj_pf_setup_host_hashes")
    return ({k: "%016x" % v for k, v in zip(names, a)}, {k: "%016x" % v for k, v in zip(names, b)})


def _pf_many_lockstep(seqs, k, dangle, params, noGU, device, capacity) -> list:
    runs = plan_lockstep([len(s) for s in seqs], k)
    cap = max(len(s) for s in seqs) if capacity is None else int(capacity)
    out: list = [None] * len(seqs)
    batch = PfLockstepBatch(cap, min(max(1, int(k)), len(seqs)), dangle, params=params, noGU=noGU, device=device)
    try:
        for run in runs:
            batch.bind([seqs[x] for x in run])
            batch.fill()
            for x, pf in zip(run, batch.members):
                out[x] = (seqs[x], None, pf.refused) if pf.refused is not None else (seqs[x], pf.energy, pf.W()[-1])
    finally:
        batch.close()
    return out


def pf_many(seqs, dangle: int = 2, params: str | bytes = "DirksPierce09", noGU: bool = False, device: int = 0,
            capacity: Optional[int] = None, lockstep: int = 0) -> list:
    """The partition function of every sequence through one capacity context (capacity: the longest
    sequence by default), rebind + fill each.  Returns one record per sequence, in input order:
    (seq, energy, W(n)).  A fold that fails (CCJ_E_PF_RANGE: the exactness guard) is recorded as
    (seq, None, CCJError) and does not disturb the others.
    lockstep=K > 0: instead, sort by length, cut into runs of K neighbours (plan_lockstep) and fill each
    run as one PfLockstepBatch, which pays every level's launches once per run; the same records, in
    input order."""
    seqs = list(seqs)
    if not seqs:
        return []
    if lockstep and int(lockstep) > 0:
        return _pf_many_lockstep(seqs, int(lockstep), dangle, params, noGU, device, capacity)
    cap = max(len(s) for s in seqs) if capacity is None else int(capacity)
    out: list = []
    pf = W_final_pf(seqs[0], dangle=dangle, params=params, noGU=noGU, device=device, capacity=cap)
    try:
        for x, s in enumerate(seqs):
            if x:
                pf.rebind(s)
            try:
                e = pf.ccj_pf()
                out.append((s, e, pf.W()[-1]))
            except CCJError as ex:
                if ex.code != CCJ_E_PF_RANGE:
                    raise
                out.append((s, None, ex))
    finally:
        pf.close()
    return out


class W_final_pf:
    """Mirror of the reference class W_final_pf (src/part_func.hh:28-194, part_func.cc).

    ``W_final_pf(seq, MFE_structure, MFE_energy, dangle, num_samples, PSplot).ccj_pf()`` runs the
    CCJ partition function on the GPU (include/ccj_pf.h) and returns the ensemble free energy in
    kcal/mol, bit-identical to the reference's part_func.cc evaluated without floating-point
    contraction.  MFE_structure, MFE_energy and PSplot are accepted and stored like the reference
    (which ignores them: pf_scale is forced to 1).  ``srand(seed)`` + ``sample(k)`` is the
    reference's stochastic traceback Sample_W(1, n) (stoch_backtrack.cc), drawing rand()/RAND_MAX
    like vrna_urn() in the reference build.
    """

    def __init__(self, seq: str, MFE_structure: str = "", MFE_energy: float = 0.0, dangle: int = 2,
                 num_samples: int = 0, PSplot: bool = False, params: str | bytes = "DirksPierce09",
                 noGU: bool = False, device: int = 0, pen=None, capacity: Optional[int] = None):
        """capacity=N: a context that folds any sequence of length 1..N (include/ccj_pf.h
        ccj_pf_create_cap); reset(seq) / rebind(seq) then bind the next sequence without allocating.
        pen: the 14 pseudoknot penalties, as for W_final."""
        self.seq = seq
        self.n = len(seq)
        self.MFE_structure = MFE_structure
        self.MFE_energy = MFE_energy
        self.num_samples = num_samples
        self.PSplot = PSplot
        self.structure = "." * self.n
        self.structures: dict = {}
        self._h = None
        L = lib()
        prob, self._keep = _pf_problem(seq, dangle, params, noGU, pen)
        h = ctypes.c_void_p()
        self._raw = load_pfraw(params)
        if capacity is None:
            rc = L.ccj_pf_create(ctypes.byref(prob), self._raw, device, ctypes.byref(h))
        else:
            rc = L.ccj_pf_create_cap(ctypes.byref(prob), self._raw, device, int(capacity), ctypes.byref(h))
        if rc != CCJ_OK:
            raise CCJError(rc, "ccj_pf_create failed (see stderr)")
        self._h = h
        self.energy: Optional[float] = None

    def _check(self, rc: int):
        if rc != CCJ_OK:
            raise CCJError(rc, lib().ccj_pf_last_message(self._h).decode())

    def _bound(self, seq: str) -> None:
        self.seq = seq
        self.n = len(seq)
        self.structure = "." * self.n
        self.energy = None

    def reset(self, seq: str) -> None:
        """Bind another sequence of the same length (ccj_pf_reset): the per-sequence tables are
        rebuilt on the GPU, nothing is allocated; the context holds no fill until ccj_pf()."""
        if len(seq) != self.n:
            raise CCJError(CCJ_E_ARG, f"reset: length {len(seq)} differs from n={self.n}")
        self._check(lib().ccj_pf_reset(self._h, seq.encode()))
        self._bound(seq)

    def rebind(self, seq: str) -> None:
        """Bind another sequence of any length up to the capacity (ccj_pf_rebind); with the bound
        length it is reset()."""
        self._check(lib().ccj_pf_rebind(self._h, seq.encode()))
        self._bound(seq)

    @property
    def capacity(self) -> int:
        """The longest sequence this context can be bound to (ccj_pf_capacity)."""
        return lib().ccj_pf_capacity(self._h)

    def keytab_info(self) -> tuple:
        """(host ms of this context's one-time key-table build, its device bytes)."""
        ms, b = ctypes.c_double(), ctypes.c_ulonglong()
        self._check(lib().ccj_pf_keytab_info(self._h, ctypes.byref(ms), ctypes.byref(b)))
        return ms.value, b.value

    def setup_hashes(self) -> dict:
        """FNV hashes of the bound sequence's setup tables on the device (ccj_pf_setup_hashes)."""
        out = (ctypes.c_uint64 * len(PF_SETUP_TABLES))()
        self._check(lib().ccj_pf_setup_hashes(self._h, out, len(PF_SETUP_TABLES)))
        return {k: "%016x" % v for k, v in zip(PF_SETUP_TABLES, out)}

    def ccj_pf(self) -> float:
        e = ctypes.c_double()
        self._check(lib().ccj_pf_fill(self._h, ctypes.byref(e)))
        self.energy = e.value
        return e.value

    def W(self) -> list:
        out = (ctypes.c_double * (self.n + 1))()
        self._check(lib().ccj_pf_W(self._h, out))
        return list(out)

    def get2(self, name: str) -> list:
        """One 2-D matrix in canonical order (i = 1..n, j = i..n)."""
        out = (ctypes.c_double * (self.n * (self.n + 1) // 2))()
        self._check(lib().ccj_pf_get2(self._h, PF_MAT2.index(name), out))
        return list(out)

    def get4(self, name: str, i: int, j: int, k: int, l: int) -> int:
        """Matrix4DPF::get: the stored int, 0 outside i <= j < k-1, k <= l."""
        v = ctypes.c_int()
        self._check(lib().ccj_pf_get4(self._h, PF_MAT4.index(name), i, j, k, l, ctypes.byref(v)))
        return v.value

    def hashes(self) -> dict:
        h4 = (ctypes.c_uint64 * len(PF_MAT4))()
        h2 = (ctypes.c_uint64 * len(PF_MAT2))()
        self._check(lib().ccj_pf_hashes(self._h, h4, h2))
        d = {k: "%016x" % v for k, v in zip(PF_MAT4, h4)}
        d.update({k: "%016x" % v for k, v in zip(PF_MAT2, h2)})
        return d

    def exp_hashes(self) -> dict:
        names = lib().ccj_pf_exp_names().decode().split()
        out = (ctypes.c_uint64 * len(names))()
        got = lib().ccj_pf_exp_hashes(self._h, out, len(names))
        if got != len(names):
            raise CCJError(CCJ_E_ARG, "ccj_pf_exp_hashes")
        return {k: "%016x" % v for k, v in zip(names, out)}

    def srand(self, seed: int) -> None:
        """srand(seed) for this context's vrna_urn() generator (rand()/RAND_MAX, like the reference build)."""
        self._check(lib().ccj_pf_srand(self._h, seed))

    def sample(self, count: int) -> list:
        """count x Sample_W(1, n) (stoch_backtrack.cc), continuing this context's rand() stream."""
        buf = ctypes.create_string_buffer(max(count, 1) * (self.n + 1))
        done = ctypes.c_int()
        rc = lib().ccj_pf_sample(self._h, count, buf, ctypes.byref(done))
        got = [buf.raw[s * (self.n + 1): s * (self.n + 1) + self.n].decode() for s in range(done.value)]
        if rc == CCJ_E_PF_SAMPLE:
            raise SampleExit(lib().ccj_pf_last_message(self._h).decode(), got)
        self._check(rc)
        return got

    def fill_ms(self) -> float:
        t = ctypes.c_float()
        self._check(lib().ccj_pf_timing(self._h, ctypes.byref(t)))
        return t.value

    @property
    def PF_KERNELS(self) -> tuple:
        """The four kernel families of kernel_ms / work_model.  Family 2, the P terms, is k_pf_ppush
        (pushed by level, the default) or k_pf_pterm (CCJ_PF_PULL=1); ccj_pf.cc reads the variable on
        every fill, so it is read here at call time too."""
        pull = os.environ.get("CCJ_PF_PULL", "0") not in ("", "0")
        return ("k_pf_iloop", "k_pf_level", "k_pf_pterm" if pull else "k_pf_ppush", "k_pf_diag")

    def set_timing(self, on: bool = True):
        """Event pairs around every launch of the following fills (ccj_pf_set_timing)."""
        self._check(lib().ccj_pf_set_timing(self._h, 1 if on else 0))

    def kernel_ms(self) -> dict:
        """Summed launch durations of the last timed fill per kernel family (ms)."""
        v = (ctypes.c_double * 4)()
        self._check(lib().ccj_pf_kernel_ms(self._h, v))
        return dict(zip(self.PF_KERNELS, v))

    def work_model(self) -> dict:
        """Algorithmic HBM bytes of one fill per kernel family (ccj_pf_work_model)."""
        v = (ctypes.c_double * 4)()
        self._check(lib().ccj_pf_work_model(self._h, v))
        return dict(zip(self.PF_KERNELS, v))

    def close(self):
        if getattr(self, "_h", None):
            lib().ccj_pf_destroy(self._h)  # ignores a lockstep batch's member: PfLockstepBatch.close frees it
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


PF_PLAN_KERNELS = ("k_pf_iloop", "k_pf_level", "k_pf_ppush", "k_pf_diag")


def pf_level_plan(lengths, t: int, item_counts=None) -> dict:
    """The launches a partition-function fill enqueues with level t for members of these lengths (no
    GPU needed; include/ccj_pf.h ccj_pf_level_plan): k_pf_iloop(t+2), k_pf_level(t), k_pf_ppush(t),
    k_pf_diag(t+3); t = -3, -2, -1 are the launches ahead of level 0.  Returns {kernel: (grid,
    members)}: grid = the one launch's (x, y, z), members = the grid each member would launch alone;
    (0, 0, 0) = no launch.  item_counts: each member's k_pf_iloop items of level t+2
    (PfLockstepBatch.item_counts); without them that family is (-1, -1, -1) wherever the level exists."""
    lengths = [int(x) for x in lengths]
    cnt = len(lengths)
    n = (ctypes.c_int * max(cnt, 1))(*lengths)
    items = None
    if item_counts is not None:
        if len(item_counts) != cnt:
            raise CCJError(CCJ_E_ARG, "pf_level_plan: one item count per member")
        items = (ctypes.c_int * max(cnt, 1))(*[int(x) for x in item_counts])
    out = (ctypes.c_int * (12 + 12 * max(cnt, 1)))()
    rc = lib().ccj_pf_level_plan_items(n, items, cnt, int(t), out)
    if rc != CCJ_OK:
        raise CCJError(rc, "bad plan arguments")
    g = [tuple(out[3 * q: 3 * q + 3]) for q in range(4 + 4 * cnt)]
    return {name: (g[f], tuple(g[4 + 4 * k + f] for k in range(cnt))) for f, name in enumerate(PF_PLAN_KERNELS)}


class PfLockstepBatch:
    """`members` capacity contexts of the partition function filled in lockstep (include/ccj_pf.h
    ccj_pf_batch): bind(seqs) gives member k the k-th sequence, fill() runs every bound member's fill
    in one set of level launches, then W and the energy per member.  Afterwards each bound member (a
    W_final_pf over the borrowed context) has `energy` set, or `refused` = its CCJError where the
    fold ended in CCJ_E_PF_RANGE (the other members are untouched); W(), hashes(), get2, get4,
    srand and sample work on it, its own rebind / reset / ccj_pf raise CCJ_E_STATE."""

    def __init__(self, capacity: int, members: int, dangle: int = 2, params: str | bytes = "DirksPierce09",
                 noGU: bool = False, device: int = 0, pen=None):
        L = lib()
        prob, self._keep = _pf_problem(None, dangle, params, noGU, pen)
        self._raw = load_pfraw(params)
        h = ctypes.c_void_p()
        rc = L.ccj_pf_batch_create(ctypes.byref(prob), self._raw, device, int(capacity), int(members), ctypes.byref(h))
        if rc != CCJ_OK:
            raise CCJError(rc, L.ccj_pf_batch_last_error(None).decode())
        self._h = h
        self.capacity = int(capacity)
        self.dangle = dangle
        self._all = []
        for k in range(int(members)):
            pf = W_final_pf.__new__(W_final_pf)
            pf._h = ctypes.c_void_p(L.ccj_pf_batch_member(h, k))
            pf._keep, pf._raw = self._keep, self._raw
            pf.MFE_structure, pf.MFE_energy, pf.num_samples, pf.PSplot, pf.structures = "", 0.0, 0, False, {}
            pf._bound("")
            pf.refused = None
            self._all.append(pf)
        self.count = 0

    @property
    def members(self) -> list:
        """The bound members, in the order of the last bind()."""
        return self._all[: self.count]

    @property
    def size(self) -> int:
        return len(self._all)

    def _check(self, rc: int):
        if rc != CCJ_OK:
            raise CCJError(rc, lib().ccj_pf_batch_last_error(self._h).decode())

    def bind(self, seqs) -> None:
        seqs = [str(s) for s in seqs]
        arr = (ctypes.c_char_p * max(len(seqs), 1))(*[s.encode() for s in seqs])
        self._check(lib().ccj_pf_batch_bind(self._h, arr, len(seqs)))
        self.count = len(seqs)
        for pf, s in zip(self._all, seqs):
            pf._bound(s)
            pf.refused = None

    def fill(self) -> None:
        L = lib()
        self._check(L.ccj_pf_batch_fill(self._h))
        e = ctypes.c_double()
        for k, pf in enumerate(self.members):
            rc = L.ccj_pf_batch_result(self._h, k, ctypes.byref(e))
            pf.energy, pf.refused = (e.value, None) if rc == CCJ_OK else (None, CCJError(rc, L.ccj_pf_last_message(pf._h).decode()))
            if rc not in (CCJ_OK, CCJ_E_PF_RANGE):
                raise pf.refused

    def item_counts(self, t: int) -> list:
        """Each bound member's k_pf_iloop work items of level t (0 where it has no such level)."""
        out = (ctypes.c_int * max(self.count, 1))()
        self._check(lib().ccj_pf_batch_item_counts(self._h, int(t), out))
        return list(out[: self.count])

    def fill_ms(self) -> float:
        return lib().ccj_pf_batch_fill_ms(self._h)

    def launches(self) -> int:
        """Kernel launches the last fill() enqueued."""
        return lib().ccj_pf_batch_launches(self._h)

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            for pf in self._all:
                pf._h = None
            lib().ccj_pf_batch_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
