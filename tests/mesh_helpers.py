"""float64 numpy restatement of include/sv_hip.h block N3d (sv_mesh_sample, sv_sample_eliminate) and of the composition
utils/mesh.py load_cad_model runs.  It shares no code with the package: every expression is written out elementwise in
the order the header states, and the sums whose order is part of the contract are Python-level sequential loops."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
HAND_OBJ = os.path.join(GOLDEN, "hand_notblender.obj")
HAND_PCD = os.path.join(GOLDEN, "hand.pcd")
HAND_AREA = 0.05994213121136108  # m^2, measured once with an independent parser


def bits(a):
    """float64 array -> its bit patterns, so that NaN compares equal to NaN and -0.0 differs from 0.0"""
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def parse_obj(path):
    """a parser of its own for triangle-only OBJ files: `v` rows and three-corner `f` rows with positive indices"""
    verts, tris = [], []
    for line in open(path):
        if line.startswith("v "):
            verts.append([float(x) for x in line.split()[1:4]])
        elif line.startswith("f "):
            corners = line.split()[1:]
            assert len(corners) == 3
            tris.append([int(c.partition("/")[0]) - 1 for c in corners])
    return np.array(verts, dtype=np.float64), np.array(tris, dtype=np.int32)


def triangle_areas(verts, tris):
    """-> (a [F], c [F,3], len [F], ok [F]); a triangle with an index outside the vertex list has a = 0 and ok False"""
    tris = np.asarray(tris, dtype=np.int64)
    ok = ((tris >= 0) & (tris < len(verts))).all(axis=1)
    safe = np.where(ok[:, None], tris, 0)
    v0, v1, v2 = verts[safe[:, 0]], verts[safe[:, 1]], verts[safe[:, 2]]
    e1, e2 = v1 - v0, v2 - v0
    cx = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
    cy = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
    cz = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
    length = np.sqrt((cx * cx + cy * cy) + cz * cz)
    a = 0.5 * length
    a[~ok] = 0.0
    return a, np.stack([cx, cy, cz], axis=1), length, ok


def running_sums(a):
    out = np.empty(len(a), dtype=np.float64)
    s = 0.0
    for t, x in enumerate(a.tolist()):  # ascending t, one rounding per addition
        s = s + x
        out[t] = s
    return out


def mesh_sample(verts, tris, draws):
    """-> points [N,3], normals [N,3], tri int32 [N], area, number of triangles with a bad index"""
    verts, draws = np.asarray(verts, dtype=np.float64), np.asarray(draws, dtype=np.float64)
    a, c, length, ok = triangle_areas(verts, tris)
    cdf = running_sums(a)
    area = cdf[-1]
    N, F = len(draws), len(a)
    if not (np.isfinite(area) and area > 0):
        return np.full((N, 3), np.nan), np.full((N, 3), np.nan), np.full(N, -1, np.int32), area, int((~ok).sum())
    u, r1, r2 = draws[:, 0], draws[:, 1], draws[:, 2]
    t = np.minimum(np.searchsorted(cdf, u * area, side="right"), F - 1)
    assert ok[t].all(), "the clamp landed on a triangle with a bad index: outside what this helper restates"
    tri = np.asarray(tris, dtype=np.int64)[t]
    v0, v1, v2 = verts[tri[:, 0]], verts[tri[:, 1]], verts[tri[:, 2]]
    q = np.sqrt(r1)
    w0, w1, w2 = 1.0 - q, q * (1.0 - r2), q * r2
    points = (w0[:, None] * v0 + w1[:, None] * v1) + w2[:, None] * v2
    with np.errstate(invalid="ignore", divide="ignore"):
        normals = c[t] / length[t][:, None]
    return points, normals, t.astype(np.int32), area, int((~ok).sum())


def radii(area, n_points, n_keep):
    ratio = n_keep / n_points
    r_max = 2.0 * np.sqrt((area / n_keep) / (2.0 * np.sqrt(3.0)))
    r_min = r_max * 0.5 * (1.0 - ratio * np.sqrt(ratio))
    return float(r_max), float(r_min)


def neighbour_table(points, r_max, r_min, block=1 << 21):
    """-> (nbr, wts): per point its neighbours in ascending index and their pair weights.  The pairs that are tested are
    cut down first to those within 1.001 r_max along the cloud's longest axis: d2 < r_max * r_max implies |dx| < r_max
    for the rounded dx (rounding is monotone), and the margin of a thousandth covers the rounding of the window's own
    ends for coordinates below 1e12 r_max.  The test itself is the header's expression on every pair that is left."""
    p = np.asarray(points, dtype=np.float64)
    n = len(p)
    r2 = r_max * r_max
    spans = [np.ptp(p[np.isfinite(p[:, k]), k]) if np.isfinite(p[:, k]).any() else 0.0 for k in range(3)]
    axis = int(np.argmax(spans))
    perm = np.argsort(p[:, axis], kind="stable")
    xs = p[perm, axis]
    with np.errstate(invalid="ignore"):
        lo = np.searchsorted(xs, p[:, axis] - 1.001 * r_max, side="left")
        hi = np.searchsorted(xs, p[:, axis] + 1.001 * r_max, side="right")
        cnt = np.maximum(hi - lo, 0)
        csum = np.concatenate([[0], np.cumsum(cnt)])
        found_i, found_j, found_w = [], [], []
        a = 0
        while a < n:  # rows a .. b-1: about `block` candidate pairs at a time
            b = min(n, max(a + 1, int(np.searchsorted(csum, csum[a] + block, side="right")) - 1))
            c = cnt[a:b]
            ci = np.repeat(np.arange(a, b), c)
            cj = perm[np.repeat(lo[a:b], c) + (np.arange(int(c.sum())) - np.repeat(csum[a:b] - csum[a], c))]
            dx = p[cj, 0] - p[ci, 0]
            dy = p[cj, 1] - p[ci, 1]
            dz = p[cj, 2] - p[ci, 2]
            d2 = (dx * dx + dy * dy) + dz * dz
            hit = (d2 < r2) & (cj != ci)
            d = np.maximum(np.sqrt(d2[hit]), r_min)
            t = 1.0 - d / r_max
            w = t * t
            w = w * w
            w = w * w
            found_i.append(ci[hit])
            found_j.append(cj[hit])
            found_w.append(w)
            a = b
    fi, fj, fw = np.concatenate(found_i), np.concatenate(found_j), np.concatenate(found_w)
    by_row = np.lexsort((fj, fi))  # by i, then ascending j
    fi, fj, fw = fi[by_row], fj[by_row], fw[by_row]
    starts = np.searchsorted(fi, np.arange(n + 1))
    return ([fj[starts[k]:starts[k + 1]] for k in range(n)], [fw[starts[k]:starts[k + 1]] for k in range(n)])


def sample_eliminate(points, n_keep, r_max, r_min):
    """-> kept int32 [n_keep] ascending, order int32 [N - n_keep] in deletion order, the largest neighbour count"""
    n = len(points)
    nbr, wts = neighbour_table(points, r_max, r_min)
    nbr_l, wts_l = [x.tolist() for x in nbr], [x.tolist() for x in wts]
    alive = [True] * n

    def row_weight(i):
        s = 0.0
        for j, w in zip(nbr_l[i], wts_l[i]):  # ascending j, one rounding per addition
            if alive[j]:
                s = s + w
        return s

    weight = np.array([row_weight(i) for i in range(n)], dtype=np.float64)
    order = []
    for _ in range(n - n_keep):
        p = int(np.argmax(weight))  # the first maximum: the lowest index on a tie; deleted points sit at -1
        order.append(p)
        alive[p] = False
        weight[p] = -1.0
        for q in nbr_l[p]:
            if alive[q]:
                weight[q] = row_weight(q)
    kept = np.nonzero(np.array(alive))[0].astype(np.int32)
    return kept, np.array(order, dtype=np.int32), max((len(x) for x in nbr_l), default=0)


_CACHE = {}


def hand_mesh():
    if "mesh" not in _CACHE:
        _CACHE["mesh"] = parse_obj(HAND_OBJ)
    return _CACHE["mesh"]


def hand_samples(n, seed=0):
    """(points, normals, tri, area) of n samples of the hand mesh drawn with default_rng(seed); computed once per n"""
    key = ("samples", n, seed)
    if key not in _CACHE:
        verts, tris = hand_mesh()
        _CACHE[key] = mesh_sample(verts, tris, np.random.default_rng(seed).random((n, 3)))[:4]
    return _CACHE[key]


def hand_eliminated(n, n_keep, seed=0):
    """(kept, order, max degree) of hand_samples(n) thinned to n_keep; computed once per size"""
    key = ("eliminated", n, n_keep, seed)
    if key not in _CACHE:
        points, _, _, area = hand_samples(n, seed)
        _CACHE[key] = sample_eliminate(points, n_keep, *radii(area, n, n_keep))
    return _CACHE[key]


def cad_model(n_init=16384, n_points=8192, seed=0):
    """what load_cad_model(HAND_OBJ) must return: float32 points and normals of the thinned samples with x > 0"""
    points, normals, _, _ = hand_samples(n_init, seed)
    kept, _, _ = hand_eliminated(n_init, n_points, seed)
    points, normals = points[kept], normals[kept]
    mask = points[:, 0] > 0.0
    return points[mask].astype(np.float32), normals[mask].astype(np.float32)
