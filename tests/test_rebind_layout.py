"""The layout extents a capacity context allocates from (include/ccj.h ccj_layout_extents), on the CPU.

ccj_create_cap sizes every n-dependent buffer from layout_extents(N, as_capacity=True) and nothing
else, and a rebind lays a length n <= N out inside those buffers.  So for every n up to the
capacity, under every split target, share flag and d4 width, a binding's extents must fit the
capacity's, entry by entry; and where an extent grows with n the capacity's value is the length-N
value itself, so a plain ccj_create (capacity = length) allocates what it always did.
"""
import pytest

from ccj_amd import DEFAULT_SPLIT_TARGET, layout_extents, level_schedule, num_cells

CAPACITIES = [40, 64, 120]
TARGETS = [DEFAULT_SPLIT_TARGET, 96, 200, 352, 0]  # 0: never split
# the sharing range moves with n and the target, and these three follow it; every other extent grows with n
FOLLOW_SHARING = {"acc", "lord", "lord_off"}
NAMES = ["d4", "rec", "rk", "rl", "acc", "d4x", "pmx", "lord", "lord_off", "plane", "il", "ilseg", "levels", "lx",
         "events", "icount", "ppush_span", "iloop_span"]


def _all(N, target, share, full4):
    return {n: layout_extents(n, target, share, bool(full4)) for n in range(1, N + 1)}


@pytest.mark.parametrize("full4", [0, 1])
@pytest.mark.parametrize("share", [True, False], ids=["share", "noshare"])
@pytest.mark.parametrize("target", TARGETS)
@pytest.mark.parametrize("N", CAPACITIES)
def test_every_binding_fits_its_capacity(N, target, share, full4):
    cap = layout_extents(N, target, share, bool(full4), as_capacity=True)
    assert list(cap) == NAMES
    use = _all(N, target, share, full4)
    for n, e in use.items():
        over = {k: (e[k], cap[k]) for k in NAMES if e[k] > cap[k]}
        assert not over, (n, over)
    # the capacity's value is the largest any length up to N uses: nothing is over-allocated either
    for k in NAMES:
        assert cap[k] == max(e[k] for e in use.values()), k


@pytest.mark.parametrize("full4", [0, 1])
@pytest.mark.parametrize("share", [True, False], ids=["share", "noshare"])
@pytest.mark.parametrize("target", TARGETS)
@pytest.mark.parametrize("N", CAPACITIES)
def test_capacity_equals_binding_where_the_extent_grows_with_n(N, target, share, full4):
    """A plain ccj_create is ccj_create_cap at capacity = length: same sizes as before."""
    use = _all(N, target, share, full4)
    for n in range(1, N + 1):
        cap = layout_extents(n, target, share, bool(full4), as_capacity=True)
        for k in NAMES:
            if k not in FOLLOW_SHARING:
                assert cap[k] == use[n][k], (n, k)
                assert n == 1 or use[n][k] >= use[n - 1][k], (n, k)
            else:
                assert cap[k] >= use[n][k], (n, k)


@pytest.mark.parametrize("full4", [0, 1])
@pytest.mark.parametrize("N", CAPACITIES)
def test_cell_carriers_are_cells_times_their_width(N, full4):
    """d4: 6 int16 slots per cell (12 bytes), all 22 in a full context (44); the three loop-record
    arrays one record of 8, 8 and 4 bytes per cell."""
    for n in range(1, N + 1):
        for as_cap in (False, True):
            e = layout_extents(n, full4=bool(full4), as_capacity=as_cap)
            assert e["d4"] == num_cells(n) * (22 if full4 else 6)
            assert e["rec"] == e["rk"] == e["rl"] == num_cells(n)


def test_sharing_extents_follow_the_schedule_getter():
    """acc, lord and lord_off are there exactly when the length shares (level_schedule's range, which moves
    with n and the target)."""
    for n in range(1, 65):
        s = level_schedule(n, 0, 1, 0, 96)
        e = layout_extents(n, 96)
        sharing = s.g_hi > s.g_lo
        assert (e["acc"] > 0) == (e["lord"] > 0) == (e["lord_off"] > 0) == sharing, n
        if sharing:
            assert e["lord_off"] == n + 1
            # every block of every sharing level, less the followers that take both sides from a record
            assert 0 < e["lord"] <= sum(t + 1 for t in range(s.g_lo, s.g_hi))
    assert layout_extents(64, 96, share=False)["acc"] == 0


def test_bad_arguments():
    from ccj_amd import CCJError
    for bad in [dict(n=0), dict(n=1024), dict(n=10, split_target=-1)]:
        with pytest.raises(CCJError):
            layout_extents(**bad)
