"""What tests/test_gpu_conv_strided.py relies on, checked without a GPU: the chosen blobs give the strided maps the properties
the GPU tests are about (from strided_helpers.probe_ref alone), and every row of strided_helpers.STRIDED_CASES expects the
instance and form the library's own host-side dispatch (conv_instance_helpers.dispatch) answers for its shape."""
import numpy as np

import conv_instance_helpers as H
import strided_helpers as S


def _vpad(V):
    return (V + H.PLAN_TILE - 1) // H.PLAN_TILE * H.PLAN_TILE


def test_fine_maps_leave_a_67_row_last_plan_tile_and_hold_negative_coordinates():
    for name in S.FRAMES:
        c = S.frame_coords(name)
        assert len(c) == sum(V for V, _ in S.FRAMES[name]) and len(c) % H.PLAN_TILE == 67, name
    two = S.frame_coords("two")
    assert (two[two[:, 0] == 1][:, 1:] < 0).all(), "the second frame lies at negative coordinates"
    assert len({tuple(r) for r in (two[two[:, 0] == 1][:, 1:] % 2).tolist()}) == 8, "every parity class"


def test_map_kinds_have_the_row_counts_the_tests_are_about():
    for name in ("one", "two"):
        for kind, (ks, st, dil, transposed) in S.MAP_KINDS.items():
            nbr, V_in, V_out = S.kind_table(name, kind)
            assert nbr.shape == (ks ** 3, V_out)
            assert nbr.max() < V_in and (nbr >= 0).any()
            if transposed:
                assert V_out > V_in, (name, kind)
            elif kind in ("k3s2", "k3s3"):
                assert V_out < V_in, (name, kind)
            # nbr[k][o] = i on the forward map exactly when nbr_t[k][i] = o on the transposed one
            if transposed:
                fwd = S.kind_table(name, kind[:-2])[0]
                pairs_f = {(k, int(fwd[k, o]), o) for k, o in zip(*np.nonzero(fwd >= 0))}
                pairs_t = {(k, i, int(nbr[k, i])) for k, i in zip(*np.nonzero(nbr >= 0))}
                assert pairs_f == pairs_t, (name, kind)


def test_empty_tile_maps_have_whole_plan_tiles_without_any_neighbour():
    """At least half of the rows of k1s2_t and k3s2d2_t have no neighbour at all.  The plan is sorted by mask, so these rows
    are contiguous: 255 of them hold a whole 128-row tile wherever they start, and because the empty mask sorts first
    (sv_plan_build: rank 0 of the Gray order) the tile they end in mixes empty and live 16-row sub-tiles when their count
    leaves between 16 and 112 rows in it.  (The GPU test asserts both on the plan itself.)"""
    for name in ("one", "two", "big"):
        for kind in S.EMPTY_TILE_KINDS:
            if name == "big" and kind != "k1s2_t":
                continue
            nbr, V_in, V_out = S.kind_table(name, kind)
            n0 = int((nbr < 0).all(0).sum())
            assert 2 * n0 >= V_out and n0 >= 255, (name, kind, n0, V_out)
            assert name == "big" or 16 <= n0 % H.PLAN_TILE <= 112, (name, kind, n0)  # (the dual row needs no mixed tile)
            # a row has a neighbour exactly when all its coordinates are even (the output voxels of a stride-2 map)
            even = (S.frame_coords(name)[:, 1:] % 2 == 0).all(1)
            assert np.array_equal((nbr >= 0).any(0), even), (name, kind)


def test_row_edge_blobs_and_the_single_voxel_without_a_neighbour():
    for V in S.EDGE_V:
        c1 = S.canonical(S.compact_blob(V, origin=(1, 1, 1)))[0]
        nbr, V_in, V_out = S.kind_table_of(c1, "k3s2d2_t")
        assert V_out == V and V_in >= 1
        if V == 1:
            assert (nbr < 0).all(), "the only row of V = 1 has no neighbour"
        else:
            assert (nbr >= 0).any() and (nbr < 0).all(0).any(), V


def test_every_strided_row_expects_what_the_library_dispatches():
    """the literals of STRIDED_CASES against sv_conv_select, and the coverage the table promises"""
    for c in S.STRIDED_CASES:
        nbr, V_in, V_out = S.kind_table(c.frame, c.kind)
        K = nbr.shape[0]
        name, flags = H.dispatch(K, c.Cin, c.Cout, _vpad(V_out), True, c.Cin % 4 == 0, not c.mis, False,
                                 c.scale if c.scale is not None else H.WANT_SCALE_DEFAULT)
        assert (name, flags["fast"], flags["ring"], flags["full"]) == (c.name, c.fast, c.ring, c.full), c
        assert not c.name.startswith("linear_narrow"), c
        if _tile(c.name):  # a tiled row is guarded for a reason the row states: `perm`, odd Cin or a partial column tile
            assert c.fast == int(not c.mis and c.Cin % 4 == 0 and c.Cout % H.tile_cfg(*_tile(c.name)).TN == 0), c
    ids = [S.strided_case_id(c) for c in S.STRIDED_CASES]
    assert len(set(ids)) == len(ids)
    for name, flags, Cin, Cout, scale, mis in S.EDGE_SPECIAL:
        got, f = H.dispatch(27, Cin, Cout, 128, True, Cin % 4 == 0, not mis, False,
                            scale if scale is not None else H.WANT_SCALE_DEFAULT)
        assert (got, (f["fast"], f["ring"], f["full"])) == (name, flags)

    def covered(pred):
        kinds = {c.kind for c in S.STRIDED_CASES if pred(c)}
        return bool(kinds & set(S.EMPTY_TILE_KINDS)) and bool(kinds - {k for k in S.MAP_KINDS if k.endswith("_t")})

    K_of = lambda c: S.MAP_KINDS[c.kind][0] ** 3  # noqa: E731
    # each on at least one forward kind and on an empty-tile map
    for special in (S.FIRST_MFMA, S.FIRST_VALU, S.THIN, S.THIN_LDS):
        assert covered(lambda c: c.name == special), special
    for cin, cout in ((32, 64), (64, 64), (64, 128)):
        assert covered(lambda c: (c.Cin, c.Cout) == (cin, cout) and K_of(c) == 27 and "fused" in c.name), (cin, cout)
        assert covered(lambda c: (c.Cin, c.Cout) == (cin, cout) and K_of(c) == 1 and "fused" not in c.name), (cin, cout)
    assert covered(lambda c: (c.Cin, c.Cout) == (3, 64) and c.fast == 0)
    assert covered(lambda c: (c.Cin, c.Cout) == (256, 64) and K_of(c) == 1 and c.full == 1)
    assert covered(lambda c: (c.Cin, c.Cout) == (64, 256) and K_of(c) == 1)
    assert any(H.tile_cfg(*_tile(c.name)).TN == 128 for c in S.STRIDED_CASES if _tile(c.name))
    assert covered(lambda c: (c.Cin, c.Cout) == (512, 512) and K_of(c) == 27)
    assert covered(lambda c: (c.Cin, c.Cout) == (256, 384) and c.full == 1 and H.tile_cfg(*_tile(c.name)).TN == 192)
    assert any(c.name == S.DUAL and c.kind == "k1s2_t" and (c.Cin, c.Cout) == (148, 384) for c in S.STRIDED_CASES)
    for cout in (1, 3, 4):
        assert covered(lambda c: (c.Cin, c.Cout) == (148, cout) and K_of(c) == 1)
    assert {c.kind for c in S.STRIDED_CASES} == set(S.MAP_KINDS), "every kind runs at least once"
    assert {c.frame for c in S.STRIDED_CASES} == {"one", "two", "big"}


def _tile(name):
    import re

    m = re.fullmatch(r"conv_fwd_kernel<(\d+), (\d+), (\d+)(?:, fused (\d+))?>", name)
    return (int(m[1]), int(m[2]), int(m[3]), int(m[4] or 0)) if m else None


def test_the_dual_row_runs_its_tail_body_over_more_tiles_than_the_live_rows_fill():
    """the dual-body launch gives its 32-row tail body the tail128 cheapest plan tiles; on k1s2_t of the 24003-voxel blob the
    rows WITH a neighbour fill fewer tiles than the rest of the grid, so the tail can only consist of empty tiles"""
    nbr, V_in, V_out = S.kind_table("big", "k1s2_t")
    n128 = _vpad(V_out) // H.PLAN_TILE
    tail128 = int(n128 * H.TAIL_DEFAULT)
    live_tiles = -(-int((nbr >= 0).any(0).sum()) // H.PLAN_TILE) + 1  # the live rows, and the tile they share with empty ones
    assert 1 <= tail128 < n128 - live_tiles


def test_the_batch_frame_has_an_empty_index_and_different_bounds_at_the_two_strides():
    """what the batch-range tests split at: four batch indices, index 1 empty, the other three of different sizes at both
    strides, so that ranges of one and of two indices are different splits on the input and on the output side"""
    c1 = S.frame_coords("batch")
    b1, b2 = S.batch_bounds_ref(c1, 4), S.batch_bounds_ref(S.stride_map_ref(c1, 2)[0], 4)
    assert b1 == [0, 419, 419, 419 + 707, 1475]
    assert b2[1] == b2[2] and b2[0] == 0 and b2[1] > 0 and b2[3] > b2[2] and b2[4] > b2[3]
    assert b2 != b1 and b2[4] < b1[4]
    for kind in ("k3s2", "k1s2_t", "k1s2", "k3s2_t"):
        nbr, V_in, V_out = S.kind_table("batch", kind)
        bi, bo = (b2, b1) if kind.endswith("_t") else (b1, b2)
        assert (V_in, V_out) == (bi[4], bo[4])
        for c in range(4):  # the frames of a batch share no neighbours: a range's rows read its own input rows only
            rows = nbr[:, bo[c]:bo[c + 1]]
            assert ((rows < 0) | ((rows >= bi[c]) & (rows < bi[c + 1]))).all(), (kind, c)
