"""Plain numpy restatements of the PointNet++ training kernels (csrc/sv_pointnet_grad.hip), in the kernels' own float32
operation order, and the inputs the GPU edge tests run them on.  tests/test_pointnet_grad_cpu.py pins every function here
(to torch on the CPU, to a brute-force definition or to a float64 sum), so tests/test_gpu_pointnet_grad_edges.py compares
the kernels bit for bit with a checked emulation."""
import itertools

import numpy as np

SSG, MSG = 0, 1  # SV_GROUP_SSG / SV_GROUP_MSG
U = 2.0 ** -24  # unit roundoff of float32


def same_bits(got, want):
    """float32 arrays with the same bits; a NaN matches a NaN, the sign of zero counts"""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    if got.dtype != np.float32 or want.dtype != np.float32 or got.shape != want.shape:
        return False
    ng, nw = np.isnan(got), np.isnan(want)
    return np.array_equal(ng, nw) and np.array_equal(got.view(np.uint32)[~ng], want.view(np.uint32)[~nw])


# ---- references ----------------------------------------------------------------------------------------------------
def group_rows_ref(xyz, points, new_xyz, idx, order, ld):
    """sv_group_rows: xyz [B, N, 3], points [B, N, D] or None, new_xyz [B, S, 3], idx int64 [B, S, K] (None: group_all)
    -> float32 [B * S * K, ld].  SSG [xyz[j] - new_xyz[g], points[j]], MSG [points[j], xyz[j] - new_xyz[g]]; a row whose
    index is outside [0, N) is NaN in columns < 3 + D; columns 3 + D .. ld - 1 are +0.0."""
    xyz = np.asarray(xyz, dtype=np.float32)
    B, N, _ = xyz.shape
    D = 0 if points is None else points.shape[2]
    if idx is None:  # every point once, as it is
        out = np.zeros((B, N, ld), dtype=np.float32)
        out[:, :, :3] = xyz
        if D:
            out[:, :, 3:3 + D] = np.asarray(points, dtype=np.float32)
        return out.reshape(B * N, ld)
    idx = np.asarray(idx, dtype=np.int64)
    _, S, K = idx.shape
    ok = (idx >= 0) & (idx < N)
    j = np.where(ok, idx, 0)
    b = np.arange(B)[:, None, None]
    gx = xyz[b, j] - np.asarray(new_xyz, dtype=np.float32)[:, :, None, :]  # float32 - float32: one rounding
    parts = [gx]
    if D:
        feats = np.asarray(points, dtype=np.float32)[b, j]
        parts = [gx, feats] if order == SSG else [feats, gx]
    out = np.zeros((B, S, K, ld), dtype=np.float32)
    out[..., :3 + D] = np.concatenate(parts, axis=-1)
    out[..., :3 + D][~ok] = np.nan
    return out.reshape(B * S * K, ld)


def index_transpose_ref(idx, N):
    """sv_index_transpose: idx [B, M] (any integer type) -> (offsets int32 [B * N + 1], pos int32 [valid entries]).
    key = b * N + idx; entries outside [0, N) are dropped (compared in int64); pos is the stable argsort of the valid
    positions by key; offsets[t] is the lower bound of t in the sorted keys."""
    idx = np.asarray(idx)
    B = idx.shape[0]
    M = int(np.prod(idx.shape[1:]))
    v = idx.reshape(B, M).astype(np.int64)
    ok = (v >= 0) & (v < N)
    key = (np.arange(B, dtype=np.int64)[:, None] * N + v).reshape(-1)
    p = np.nonzero(ok.reshape(-1))[0]
    order = np.argsort(key[p], kind="stable")
    pos = p[order].astype(np.int32)
    offsets = np.searchsorted(key[p][order], np.arange(B * N + 1, dtype=np.int64), side="left").astype(np.int32)
    assert B * M < 2 ** 31
    return offsets, pos


def gather_transpose_ref(offsets, pos, w, rows, col0, C, per_row, order="ascending"):
    """sv_gather_transpose -> float32 [T, C]: acc = +0.0f, then for the positions p of target t in ascending order
    acc = fl(acc + fl(w[p] * v)) (fl(acc + v) without w) with v = rows[p // per_row, col0 + c].  order "descending"
    walks the same positions from the last to the first (used only to show that inputs are order-sensitive)."""
    assert order in ("ascending", "descending")
    offsets = np.asarray(offsets, dtype=np.int64)
    pos = np.asarray(pos, dtype=np.int64)
    rows = np.asarray(rows)
    assert rows.dtype == np.float32 and (w is None or w.dtype == np.float32)
    T = len(offsets) - 1
    cnt = np.diff(offsets)
    acc = np.zeros((T, C), dtype=np.float32)
    with np.errstate(all="ignore"):
        for step in range(int(cnt.max()) if T else 0):
            live = np.nonzero(cnt > step)[0]
            q = offsets[live] + step if order == "ascending" else offsets[live + 1] - 1 - step
            p = pos[q]
            v = rows[p // per_row, col0:col0 + C]
            if w is not None:
                v = w[p][:, None] * v  # float32 * float32 -> float32: one rounding
            acc[live] = acc[live] + v
    return acc


def group_max_ref(rows, nsample):
    """sv_group_max: rows [G * nsample, C] -> (values float32 [G, C], arg int32 [G, C]).  Start at k = 0; a later value
    replaces the current one only if the current is not NaN and the value is strictly greater or NaN."""
    rows = np.asarray(rows, dtype=np.float32)
    C = rows.shape[1]
    v = rows.reshape(-1, nsample, C)
    m = v[:, 0].copy()
    a = np.zeros(m.shape, dtype=np.int32)
    with np.errstate(all="ignore"):
        for k in range(1, nsample):
            x = v[:, k]
            take = ~np.isnan(m) & ((x > m) | np.isnan(x))
            m = np.where(take, x, m)
            a = np.where(take, np.int32(k), a)
    return m, a


def group_max_backward_ref(dpooled, arg, nsample):
    """sv_group_max_backward: drows [G * nsample, C] = dpooled[g, c] at row k = arg[g, c] (its bits), +0.0 elsewhere"""
    dpooled = np.asarray(dpooled, dtype=np.float32)
    G, C = dpooled.shape
    out = np.zeros((G, nsample, C), dtype=np.float32)
    g, c = np.meshgrid(np.arange(G), np.arange(C), indexing="ij")
    out[g, np.asarray(arg), c] = dpooled
    return out.reshape(G * nsample, C)


# ---- inputs of the gather-transpose tests ----------------------------------------------------------------------------
def wide_values(rng, shape):
    """normal * 10 ** uniform(-3, 3): six decades of magnitude, so a float32 sum depends on its order"""
    return (rng.standard_normal(shape) * 10.0 ** rng.uniform(-3, 3, shape)).astype(np.float32)


def table_with_counts(rng, counts, per_row):
    """a flat index table (int64, one cloud of len(counts) targets) that references target t counts[t] times, shuffled,
    with entries of -1 (dropped) mixed in so that its length is a multiple of per_row and some positions are skipped"""
    flat = np.repeat(np.arange(len(counts), dtype=np.int64), counts)
    pad = 5 + (-(len(flat) + 5)) % per_row
    flat = np.concatenate([flat, np.full(pad, -1, dtype=np.int64)])
    return flat[rng.permutation(len(flat))]


GATHER_T = 37  # T * C is no multiple of 256 for C = 1, 5, 64, 257
GATHER_GRID = [dict(weighted=wt, per_row=pr, col0=c0, C=C, pad_rows=padr, pad_out=pado)
               for wt, pr, c0, C, padr, pado in itertools.product((False, True), (1, 3), (0, 3), (1, 5, 64, 257), (0, 3),
                                                                  (0, 2))]
GATHER_BIG = [dict(weighted=wt, per_row=pr, col0=3, C=5, pad_rows=3, pad_out=2, big=1100)
              for wt, pr in ((False, 1), (True, 3))]


def gather_id(case):
    return "-".join(f"{k}{int(v)}" for k, v in case.items())


def gather_case(case, specials=True):
    """the arrays of one sv_gather_transpose case: dict(offsets, pos, w, rows, ld_rows, nan_targets, inf_targets, table,
    nan_at, inf_at).  Reference counts 0 .. 40 per target (target 1 has none; `big`: target 2 has that many); with
    `specials`, rows holds one NaN and one +inf (different rows), and nan_targets / inf_targets are the (target, column)
    pairs they must reach."""
    seed = sum((i + 1) * int(v) * 131 for i, v in enumerate(case.values()))
    rng = np.random.default_rng(seed)
    T, C, per_row, col0 = GATHER_T, case["C"], case["per_row"], case["col0"]
    counts = rng.integers(0, 41, T)
    counts[0], counts[1] = 40, 0
    if case.get("big"):
        counts[2] = case["big"]
    table = table_with_counts(rng, counts, per_row)
    M = len(table)
    ld_rows = col0 + C + case["pad_rows"]
    rows = wide_values(rng, (M // per_row, ld_rows))
    w = (rng.random(M) + 0.05).astype(np.float32) if case["weighted"] else None
    nan_at = inf_at = None
    if specials:
        valid = np.nonzero(table >= 0)[0]
        nan_at = (int(valid[3]) // per_row, int(rng.integers(0, C)))
        other = [int(p) // per_row for p in valid if int(p) // per_row != nan_at[0]]
        inf_at = (other[len(other) // 2], int(rng.integers(0, C)))
        rows[nan_at[0], col0 + nan_at[1]] = np.nan
        rows[inf_at[0], col0 + inf_at[1]] = np.inf
    offsets, pos = index_transpose_ref(table[None], T)
    d = dict(offsets=offsets, pos=pos, w=w, rows=rows, ld_rows=ld_rows, table=table, nan_at=nan_at, inf_at=inf_at)
    if specials:
        row_of = np.arange(M) // per_row
        d["nan_targets"] = {(int(t), nan_at[1]) for t in table[(row_of == nan_at[0]) & (table >= 0)]}
        d["inf_targets"] = {(int(t), inf_at[1]) for t in table[(row_of == inf_at[0]) & (table >= 0)]} - d["nan_targets"]
    return d


# ---- inputs of the autograd-Function tests ---------------------------------------------------------------------------
def group_rows_grad_case(order, D, seed=0):
    """a ball-query table over a small cloud (about six references per point, point 0 never referenced) and an upstream
    gradient of wide_values: dict(xyz, points, new_xyz, idx, drows, col0)"""
    rng = np.random.default_rng(1000 + 10 * D + order + seed)
    B, N, S, K = 2, 23, 9, 16
    return dict(xyz=rng.random((B, N, 3), dtype=np.float32), points=rng.standard_normal((B, N, D)).astype(np.float32),
                new_xyz=rng.random((B, S, 3), dtype=np.float32), idx=rng.integers(1, N, (B, S, K)).astype(np.int64),
                drows=wide_values(rng, (B * S * K, 3 + D)), col0=3 if order == SSG else 0)


def three_nn_grad_case(seed=0):
    """hand-made 3-NN tables: dict(points2 [B, S, C], idx int32 [B, N, 3], w [B, N, 3], dout [B, N, C])"""
    rng = np.random.default_rng(2000 + seed)
    B, N, S, C = 2, 40, 9, 5
    w = rng.random((B, N, 3), dtype=np.float32) + np.float32(0.05)
    return dict(points2=rng.standard_normal((B, S, C)).astype(np.float32),
                idx=rng.integers(0, S - 1, (B, N, 3)).astype(np.int32),  # source S - 1 is never referenced
                w=(w / w.sum(-1, keepdims=True)).astype(np.float32), dout=wide_values(rng, (B, N, C)))
