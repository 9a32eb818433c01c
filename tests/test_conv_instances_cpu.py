"""Completeness of the fp32 sparse-convolution instance table (tests/conv_instance_helpers.py), without a GPU.

The library's own dispatch (conv_select of csrc/sv_conv_select.h, the function sv_conv_fwd_acc launches by, asked through
sv_conv_select) is swept over both dispatch scales, K = 1 / 8 / 27, input and output widths from every list, every padded row count up to 136k, an
aligned and a misaligned `perm`, a first and a later pass.  The set of (instance, fast, ring, full) it can produce must be
exactly the set CASES pins on the GPU (tests/test_gpu_conv_instances.py): a candidate added to a list, or a moved
threshold, fails here until a row covers it.

Rows of the tile table (sv_conv_tile_info) that NO dispatch rule reaches - only SV_CONV_FORCE / SV_CONV_FORCE_RANGE /
SV_CONV_FORCE_DENSE select them, so they are out of scope here (whether to keep them is a separate question):

    <128, 4, 3>  <128, 2, 3>  <128, 1, 3>  <64, 2, 3>  <64, 1, 3>
    <128, 2, 2>  <128, 1, 2>  <64, 2, 2>   <64, 1, 2>  <16, 4, 2>

Forms the rules cannot produce on a reachable tile (the sweep never yields them): FAST on <32, 2, 2> (its list holds
no width that is a multiple of its 64 columns) and on the fused-3 tiles (Cin = 3); FULL on the tiles whose USE_FULL is
false; ring = 1 on <64, 4, 3>, <64, 4, 2>, <32, 4, 3> and <128, 4, 2> (PFD = 1: they have no ring form).
"""
import re

import pytest

import conv_instance_helpers as H

UNREACHABLE = {(128, 4, 3, 0), (128, 2, 3, 0), (128, 1, 3, 0), (64, 2, 3, 0), (64, 1, 3, 0),
               (128, 2, 2, 0), (128, 1, 2, 0), (64, 2, 2, 0), (64, 1, 2, 0), (16, 4, 2, 0)}


@pytest.fixture(scope="module")
def reachable():
    return H.sweep()


def _tile_of(name):
    m = re.fullmatch(r"conv_fwd_kernel<(\d+), (\d+), (\d+)(?:, fused (\d+))?>", name)
    return (int(m[1]), int(m[2]), int(m[3]), int(m[4] or 0)) if m else None


def _expected(c):
    return (c.name, c.fast, c.ring, c.full)


def test_tile_constants_as_convcfg_computes_them():
    """MR, TN, GK, KC, PFD, USE_FULL of the tiles the comments of csrc/sv_conv.hip speak of"""
    assert H.tile_cfg(64, 4, 3) == H.TileCfg(MR=4, TN=192, GK=1, KC=32, PFD=1, USE_FULL=False)
    assert H.tile_cfg(32, 4, 3) == H.TileCfg(MR=2, TN=192, GK=1, KC=64, PFD=1, USE_FULL=True)
    assert H.tile_cfg(16, 4, 3) == H.TileCfg(MR=1, TN=192, GK=1, KC=128, PFD=3, USE_FULL=True)
    assert H.tile_cfg(16, 4, 1) == H.TileCfg(MR=1, TN=64, GK=1, KC=128, PFD=8, USE_FULL=True)
    assert H.tile_cfg(128, 4, 2) == H.TileCfg(MR=8, TN=128, GK=1, KC=32, PFD=1, USE_FULL=False)
    assert H.tile_cfg(128, 1, 1) == H.TileCfg(MR=2, TN=16, GK=1, KC=64, PFD=4, USE_FULL=False)
    assert H.tile_cfg(64, 1, 1) == H.TileCfg(MR=1, TN=16, GK=1, KC=128, PFD=8, USE_FULL=True)
    assert H.tile_cfg(64, 2, 1, 3) == H.TileCfg(MR=2, TN=32, GK=27, KC=84, PFD=4, USE_FULL=False)
    assert H.tile_cfg(32, 2, 1, 32) == H.TileCfg(MR=1, TN=32, GK=4, KC=128, PFD=8, USE_FULL=True)
    assert H.tile_cfg(32, 4, 1, 64) == H.TileCfg(MR=2, TN=64, GK=2, KC=128, PFD=4, USE_FULL=False)
    assert len(H.INSTANTIATED) == 34 and len(set(H.INSTANTIATED)) == 34
    # (that every candidate of every list is a row of the table, and that a list's last entry takes whatever is left, is a
    #  static_assert beside the lists)


def test_every_reachable_combination_has_a_row_and_no_row_is_unreachable(reachable):
    pinned = {_expected(c) for c in H.CASES}
    assert not (pinned & H.KNOWN_UNPINNED)
    missing = set(reachable) - pinned - H.KNOWN_UNPINNED
    assert not missing, "reachable without a CASES row (first shape that reaches it: K, Cin, Cout, Vpad, has_plan, vec_a, " \
        f"buf_ok, acc_init, want_scale): { {k: reachable[k] for k in missing} }"
    stale = (pinned | H.KNOWN_UNPINNED) - set(reachable)
    assert not stale, f"pinned but no longer reachable: {stale}"


def test_every_row_expects_what_the_restatement_says():
    """(the name is from when a Python restatement of the rules answered; H.dispatch now asks the library)"""
    for c in H.CASES:
        assert c.V % H.PLAN_TILE == 67, c  # the partial last plan tile the GPU test relies on
        assert (c.kind, c.K) in (("dense", 1), ("up", 8), ("k3", 27)), c
        assert c.split is None or (c.kind == "k3" and 0 < c.split < 27), c
        assert c.reason in (None, "odd_cin", "cout_tail", "perm_misaligned"), c
        tile = _tile_of(c.name)
        assert tile is None or (c.reason == "odd_cin") == (c.Cin % 4 != 0), c
        assert c.reason != "perm_misaligned" or c.kind != "dense", c
        name, flags = H.dispatch(*H.case_inputs(c))
        assert (name, flags["fast"], flags["ring"], flags["full"]) == _expected(c), c
        if tile and c.reason == "cout_tail":
            assert c.Cout % H.tile_cfg(*tile).TN != 0, c
        if tile and c.reason in ("odd_cin", "perm_misaligned") and tile[3] != 3 and tile != (32, 2, 2, 0):
            assert c.Cout % H.tile_cfg(*tile).TN == 0, f"two reasons at once: {c}"
        if tile and c.fast == 0:
            assert c.reason is not None, c
    ids = [H.case_id(c) for c in H.CASES]
    assert len(set(ids)) == len(ids)


def test_every_listed_tile_has_a_row_with_a_real_plan_and_every_guard_reason_it_allows(reachable):
    tiles = {_tile_of(k[0]) for k in reachable if _tile_of(k[0])}  # the tiles the sweep reaches
    assert tiles == set(H.INSTANTIATED) - UNREACHABLE
    for tile in tiles:
        rows = [c for c in H.CASES if _tile_of(c.name) == tile]
        assert any(c.K > 1 for c in rows), f"{tile}: no row with a kernel map"
        reasons = {c.reason for c in rows if c.fast == 0}
        if tile[3] == 3:
            want = {"odd_cin"}                      # Cin = 3: guarded whatever else holds
        elif tile[3]:
            want = {"perm_misaligned"}              # Cin and Cout fixed by the rule that selects the fused list
        elif tile == (32, 2, 2, 0):
            want = {"cout_tail"}                    # its list holds no multiple of its 64 columns
        else:
            want = {"odd_cin", "cout_tail", "perm_misaligned"}
        assert reasons == want, (tile, reasons)


def test_conv_dispatch_restores_the_setting_it_found():
    """conv_dispatch blocks nest: leaving one re-applies the enclosing block's thresholds (the library default at the
    bottom), also when the block ends in an exception, and one thread's blocks leave another thread's answer alone.  Read
    through sv_conv_select with this thread's current dispatch on the 32 -> 32 3x3x3 layer at 8192 padded rows, which the
    default sends to conv_thin_kernel and conv_dispatch(1.0) to conv_thin_lds_kernel."""
    import threading

    from mrcc_amd import _lib

    flags = (_lib.SV_CONV_SEL_BUF_OK | _lib.SV_CONV_SEL_PLAN | _lib.SV_CONV_SEL_TILE_ORDER | _lib.SV_CONV_SEL_VEC_A |
             _lib.SV_CONV_SEL_W_ALIGNED)
    now = lambda: _lib._parse_instance(_lib.conv_instance(27, 32, 32, 8192, flags))[0]  # noqa: E731
    THIN, LDS = "conv_thin_kernel<32, 32>", "conv_thin_lds_kernel<32, 32>"
    assert now() == THIN
    with _lib.conv_dispatch(1.0):
        assert now() == LDS
        with _lib.conv_dispatch(0.25):
            assert now() == THIN
        assert now() == LDS, "leaving the inner block must bring the outer block's setting back"
        with pytest.raises(RuntimeError):
            with _lib.conv_dispatch(0.25):
                assert now() == THIN
                raise RuntimeError("the block ends in an exception")
        assert now() == LDS
        # a second thread starts from the default, sets its own dispatch and leaves this thread's untouched
        seen, inside, leave = {}, threading.Event(), threading.Event()

        def other():
            seen["before"] = now()
            with _lib.conv_dispatch(0.25):
                seen["inside"] = now()
                inside.set()
                leave.wait(30)
            seen["after"] = now()

        t = threading.Thread(target=other)
        t.start()
        assert inside.wait(30)
        assert now() == LDS
        leave.set()
        t.join(30)
        assert not t.is_alive() and seen == {"before": THIN, "inside": THIN, "after": THIN}
        assert now() == LDS

        def other_alone():
            with _lib.conv_dispatch(1.0):
                seen["alone"] = now()

        with _lib.conv_dispatch(0.25):
            t = threading.Thread(target=other_alone)
            t.start()
            t.join(30)
            assert seen["alone"] == LDS and now() == THIN
        assert now() == LDS
    assert now() == THIN
