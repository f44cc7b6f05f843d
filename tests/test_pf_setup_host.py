"""Partition function: the per-sequence setup tables as gathers from the key tables — on the CPU.

The setup kernels of ccj_pf.hip evaluate no transcendental: every get_e_intP / get_e_stP weight is
gathered from a table the host builds once per context with libm, keyed by exp_E_IntLoop's
arguments (ccj_pf_setup.h).  ccj_pf_setup_host_hashes builds a problem's tables both ways on the
host — one pow per entry, as ccj_pf_create did before, and through the key tables with the key and
gather functions the kernels share — and returns FNV hashes of est and, over every interval whose
pair can pair, the 29 masks and 29 x 29 compacted weights of ieO and ieI.  Equal hashes are the
exactness claim, before any GPU run; tests/test_gpu_pf_contexts.py holds the device tables against
the host builder.
"""
import json
import os

import pytest

GOLD = os.path.join(os.path.dirname(__file__), "golden", "pf_golden.json")

with open(GOLD) as _f:
    CASES = json.load(_f)["cases"]


def _both(*a, **k):
    import ccj_amd
    try:
        ccj_amd.lib()
    except ccj_amd.CCJError:
        pytest.skip("libccj_hip.so not built")
    return ccj_amd.pf_setup_host_hashes(*a, **k)


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_keyed_tables_equal_direct_pow(case):
    direct, keyed = _both(case["seq"], case["dangles"], case["params"])
    assert sorted(direct) == ["est", "ieI", "ieO", "mI", "mO"]
    assert keyed == direct


def test_keyed_tables_equal_direct_pow_noGU():
    """noGU removes the G-U pair types: other intervals pair, other masks."""
    c = next(c for c in CASES if c["name"] == "big60_default")
    assert "G" in c["seq"] and "U" in c["seq"]
    direct, keyed = _both(c["seq"], 2, c["params"], noGU=True)
    assert keyed == direct
    assert direct != _both(c["seq"], 2, c["params"])[0]


def test_keyed_tables_equal_direct_pow_other_exponents():
    """e_stP / e_intP are the exponents of the two pow() calls the key tables replace."""
    from ccj_amd import PEN_DEFAULT
    c = next(c for c in CASES if c["name"] == "big40_default")
    pen = list(PEN_DEFAULT)
    pen[12], pen[13] = 0.61, 1.13
    direct, keyed = _both(c["seq"], 2, c["params"], pen=pen)
    assert keyed == direct
    base = _both(c["seq"], 2, c["params"])[0]
    assert direct["est"] != base["est"] and direct["ieO"] != base["ieO"]
    assert direct["mO"] == base["mO"]  # the masks do not depend on the exponents


def test_keyed_tables_with_T():
    """T encodes as U."""
    c = next(c for c in CASES if c["name"] == "big40_default")
    direct, keyed = _both(c["seq"].replace("U", "T"), 2, c["params"])
    assert keyed == direct == _both(c["seq"], 2, c["params"])[0]
