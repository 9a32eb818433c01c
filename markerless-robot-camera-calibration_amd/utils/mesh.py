"""The ICP model from a mesh file, with the reference's (Open3D's) names on libsvhip (include/sv_hip.h block N3d).

    mesh = read_triangle_mesh("hand_notblender.obj")            # utils/icp.py:20-24
    pcl = mesh.sample_points_uniformly(16384)                   # :26-28  (sv_mesh_sample)
    pcl = mesh.sample_points_poisson_disk(8192, pcl=pcl)        # :29-31  (sv_sample_eliminate)
    points, normals = load_cad_model("hand_notblender.obj")     # :17-40, what the matchers and the engine call

The readers are host code (a start-up step); sampling and elimination run on the device in float64.  Open3D draws from
its own generator, so the samples differ from Open3D's; the algorithm is Open3D's restated (parity by construction,
unverified).  The draws come from np.random.default_rng(0) unless given: one file gives one model at every start.
"""
import dataclasses
import math
import os
from ctypes import c_double, c_int, c_int64, c_size_t

import numpy as np
import torch

from .. import _lib
from .._lib import call, ptr, stream_ptr

MAX_TRIANGLES = 1 << 20
MAX_SAMPLES = 1 << 20
MAX_ELIMINATE = 65536
MAX_DEGREE = 1024
DEFAULT_DEGREE = 64


# ---- host readers ------------------------------------------------------------------------------------------------------
def _obj_index(token, n_vertices, path, lineno):
    """the vertex index of a face token i, i/j, i//k or i/j/k (1-based; negative = relative to the vertices read so far)"""
    try:
        i = int(token.split("/")[0])
    except ValueError:
        raise ValueError(f"{path}:{lineno}: bad face token {token!r}") from None
    if i == 0 or n_vertices + i < 0:
        raise ValueError(f"{path}:{lineno}: vertex index {i} outside the vertex list ({n_vertices} vertices so far)")
    return i - 1 if i > 0 else n_vertices + i


def read_triangle_mesh(path):
    """Wavefront OBJ -> TriangleMesh: `v x y z` (extra columns ignored) and `f` records (tokens i, i/j, i//k, i/j/k; negative
    indices relative; more than three corners fan-triangulated (0, k, k+1)); every other record is ignored."""
    path = os.fspath(path)
    vertices, triangles, lines = [], [], []
    with open(path, "r", errors="replace") as fh:
        for lineno, line in enumerate(fh, 1):
            parts = line.split()
            if not parts:
                continue
            if parts[0] == "v":
                try:
                    vertices.append((float(parts[1]), float(parts[2]), float(parts[3])))
                except (IndexError, ValueError):
                    raise ValueError(f"{path}:{lineno}: a vertex needs three numbers") from None
            elif parts[0] == "f":
                if len(parts) < 4:
                    raise ValueError(f"{path}:{lineno}: a face needs at least three corners, got {len(parts) - 1}")
                corners = [_obj_index(tok, len(vertices), path, lineno) for tok in parts[1:]]
                for k in range(1, len(corners) - 1):
                    triangles.append((corners[0], corners[k], corners[k + 1]))
                    lines.append(lineno)
    if not triangles:
        raise ValueError(f"{path}: no face record (not a triangle mesh)")
    for tri, lineno in zip(triangles, lines):  # a face may name a vertex that the file defines after it
        if max(tri) >= len(vertices):
            raise ValueError(f"{path}:{lineno}: vertex index {max(tri) + 1} outside the vertex list "
                             f"({len(vertices)} vertices)")
    return TriangleMesh(np.array(vertices, dtype=np.float64).reshape(-1, 3),
                        np.array(triangles, dtype=np.int32).reshape(-1, 3))


_PCD_TYPES = {("F", 4): "<f4", ("F", 8): "<f8", ("I", 1): "<i1", ("I", 2): "<i2", ("I", 4): "<i4", ("I", 8): "<i8",
              ("U", 1): "<u1", ("U", 2): "<u2", ("U", 4): "<u4", ("U", 8): "<u8"}


def read_point_cloud(path):
    """.pcd -> float64 [P,3]: the x, y, z fields of a `DATA ascii` or `DATA binary` file; other fields (a packed rgb,
    say) are skipped by their byte sizes."""
    path = os.fspath(path)
    with open(path, "rb") as fh:
        raw = fh.read()
    header, pos, data = {}, 0, None
    while pos < len(raw):
        end = raw.find(b"\n", pos)
        end = len(raw) if end < 0 else end
        line = raw[pos:end].decode("ascii", "replace").strip()
        pos = end + 1
        if not line or line.startswith("#"):
            continue
        key, _, rest = line.partition(" ")
        header[key.upper()] = rest.split()
        if key.upper() == "DATA":
            data = rest.strip().lower()
            break
    if data is None:
        raise ValueError(f"{path}: no DATA record (not a .pcd file)")
    if data == "binary_compressed":
        raise NotImplementedError(f"{path}: DATA binary_compressed is not supported (ascii and binary are)")
    if data not in ("ascii", "binary"):
        raise ValueError(f"{path}: unknown DATA kind {data!r}")
    try:
        fields = header["FIELDS"]
        sizes = [int(s) for s in header["SIZE"]]
        types = [t.upper() for t in header["TYPE"]]
        counts = [int(c) for c in header.get("COUNT", ["1"] * len(fields))]
        n = int(header["POINTS"][0]) if "POINTS" in header else int(header["WIDTH"][0]) * int(header["HEIGHT"][0])
    except (KeyError, IndexError, ValueError):
        raise ValueError(f"{path}: incomplete header (FIELDS, SIZE, TYPE, COUNT, POINTS)") from None
    if not len(fields) == len(sizes) == len(types) == len(counts):
        raise ValueError(f"{path}: FIELDS, SIZE, TYPE and COUNT disagree in length")
    for name in ("x", "y", "z"):
        if name not in fields or counts[fields.index(name)] != 1:
            raise ValueError(f"{path}: no scalar field {name!r}")
    if data == "ascii":
        columns = np.concatenate([[0], np.cumsum(counts)])
        rows = [ln.split() for ln in raw[pos:].decode("ascii", "replace").splitlines() if ln.strip()]
        if len(rows) < n or any(len(r) < columns[-1] for r in rows[:n]):
            raise ValueError(f"{path}: fewer than {n} complete rows of data")
        return np.array([[float(r[columns[fields.index(c)]]) for c in "xyz"] for r in rows[:n]],
                        dtype=np.float64).reshape(-1, 3)
    members = []
    for f, (name, size, typ, count) in enumerate(zip(fields, sizes, types, counts)):
        if (typ, size) not in _PCD_TYPES:
            raise ValueError(f"{path}: field {name!r} has unsupported TYPE {typ} SIZE {size}")
        members.append((f"f{f}", _PCD_TYPES[(typ, size)], (count,)))
    record = np.dtype(members)
    if len(raw) - pos < n * record.itemsize:
        raise ValueError(f"{path}: {len(raw) - pos} bytes of data, {n} points need {n * record.itemsize}")
    table = np.frombuffer(raw, dtype=record, count=n, offset=pos)
    return np.stack([table[f"f{fields.index(c)}"][:, 0].astype(np.float64) for c in "xyz"], axis=1)


# ---- device side -------------------------------------------------------------------------------------------------------
@dataclasses.dataclass
class PointCloud:
    """points, normals float64 [N,3] and triangle int32 [N] device tensors (the triangle each sample lies on);
    surface_area: the mesh's, a float."""
    points: torch.Tensor
    normals: torch.Tensor
    triangle: torch.Tensor
    surface_area: float

    def __len__(self):
        return self.points.shape[0]


def _draws(number_of_points, rng, draws):
    """-> float64 [N,3] host array of (u, r1, r2) in [0, 1), checked before anything moves"""
    if draws is None:
        n = int(number_of_points)
        if not 1 <= n <= MAX_SAMPLES:
            raise ValueError(f"number_of_points must lie in [1, 2^20], got {number_of_points!r}")
        rng = np.random.default_rng(0) if rng is None else rng
        return rng.random((n, 3))
    if torch.is_tensor(draws):
        raise ValueError("draws must be a host array [N, 3] of float64")
    shape = np.shape(draws)
    if len(shape) != 2 or shape[1] != 3 or not 1 <= shape[0] <= MAX_SAMPLES:
        raise ValueError(f"draws must be [N, 3] with N in [1, 2^20], got {shape}")
    if np.asarray(draws).dtype != np.float64:
        raise ValueError(f"draws must be float64, got {np.asarray(draws).dtype}")
    if number_of_points is not None and int(number_of_points) != shape[0]:
        raise ValueError(f"draws holds {shape[0]} rows, number_of_points is {number_of_points}")
    d = np.ascontiguousarray(draws)
    if not ((d >= 0.0) & (d < 1.0)).all():
        raise ValueError("draws must lie in [0, 1)")
    return d


def eliminate_radii(surface_area, n_points, n_keep):
    """(r_max, r_min) of Open3D's SamplePointsPoissonDisk: r_max = 2 sqrt((A / n) / (2 sqrt 3)), r_min = r_max * beta *
    (1 - ratio^gamma) with beta 0.5, gamma 1.5, ratio = n / N (ratio^1.5 written as a product)."""
    ratio = float(n_keep) / float(n_points)
    r_max = 2.0 * math.sqrt((float(surface_area) / float(n_keep)) / (2.0 * math.sqrt(3.0)))
    r_min = r_max * 0.5 * (1.0 - ratio * math.sqrt(ratio))
    return r_max, r_min


def _check_eliminate_args(shape, n_keep, r_max, r_min, max_degree):
    if len(shape) != 2 or shape[1] != 3:
        raise ValueError(f"points must be [N, 3], got {shape}")
    if not 1 <= shape[0] <= MAX_ELIMINATE:
        raise ValueError(f"points must hold 1 to 65536 rows, got {shape[0]}")
    if not 1 <= int(n_keep) <= shape[0]:
        raise ValueError(f"n_keep must lie in [1, {shape[0]}], got {n_keep!r}")
    if not (r_max > 0 and math.isfinite(r_max)):
        raise ValueError(f"r_max must be finite and positive, got {r_max!r}")
    if not 0 <= r_min <= r_max:
        raise ValueError(f"r_min must lie in [0, r_max], got {r_min!r}")
    if not 1 <= int(max_degree) <= MAX_DEGREE:
        raise ValueError(f"max_degree must lie in [1, {MAX_DEGREE}], got {max_degree!r}")


def sample_eliminate(points, n_keep, r_max, r_min, max_degree=DEFAULT_DEGREE, device="cuda"):
    """points float64 [N,3] (host array or device tensor) -> (kept int32 [n_keep] ascending, order int32 [N - n_keep] in
    deletion order) as host arrays, and the largest neighbour count.  The neighbour table has max_degree columns; when a
    point has more neighbours the call is repeated with twice as many (this is set-up code: the counter is read back)."""
    shape = tuple(points.shape) if hasattr(points, "shape") else np.shape(points)
    _check_eliminate_args(shape, n_keep, r_max, r_min, max_degree)
    dtype = getattr(points, "dtype", None)
    if not (dtype == torch.float64 if torch.is_tensor(points) else dtype == np.float64):
        raise ValueError(f"points must be float64, got {dtype}")
    dev = points.device if torch.is_tensor(points) and points.is_cuda else torch.device(device)
    pts = (points if torch.is_tensor(points) else torch.as_tensor(np.ascontiguousarray(points))).to(dev).contiguous()
    N, n_keep, max_degree = shape[0], int(n_keep), int(max_degree)
    kept = torch.empty(n_keep, dtype=torch.int32, device=dev)
    order = torch.empty(max(N - n_keep, 1), dtype=torch.int32, device=dev)
    counters = torch.zeros(1, dtype=torch.int32, device=dev)
    while True:
        ws_bytes = _lib.load().sv_sample_eliminate_workspace_bytes(c_int64(N), c_int(max_degree))
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        call("sv_sample_eliminate", ptr(pts), c_int64(N), c_int64(n_keep), c_double(r_max), c_double(r_min),
             c_int(max_degree), ptr(ws), c_size_t(ws_bytes), ptr(kept), ptr(order), ptr(counters), stream_ptr())
        degree = int(counters.item())
        if degree <= max_degree:
            return kept.cpu().numpy(), order[:N - n_keep].cpu().numpy(), degree
        if max_degree >= MAX_DEGREE:
            raise ValueError(f"a point has {degree} neighbours within r_max = {r_max!r}, more than the {MAX_DEGREE} "
                             "the table can hold: the cloud is far denser than the radius assumes")
        max_degree = min(2 * max_degree, MAX_DEGREE)


class TriangleMesh:
    """vertices float64 [Nv,3], triangles int32 [F,3] on the host."""

    def __init__(self, vertices, triangles):
        self.vertices = np.ascontiguousarray(vertices, dtype=np.float64)
        self.triangles = np.ascontiguousarray(triangles, dtype=np.int32)
        if self.vertices.ndim != 2 or self.vertices.shape[1] != 3 or self.vertices.shape[0] < 1:
            raise ValueError(f"vertices must be [Nv, 3] with Nv >= 1, got {self.vertices.shape}")
        if self.triangles.ndim != 2 or self.triangles.shape[1] != 3 or not 1 <= self.triangles.shape[0] <= MAX_TRIANGLES:
            raise ValueError(f"triangles must be [F, 3] with F in [1, 2^20], got {self.triangles.shape}")

    def sample_points_uniformly(self, number_of_points=None, rng=None, draws=None, device="cuda"):
        """number_of_points samples, each on a triangle chosen with probability proportional to its area and uniform on
        it, with the triangle's geometric normal.  draws float64 [N,3] in [0, 1) = (triangle, r1, r2) per sample, or
        rng.random((N, 3)); rng=None is np.random.default_rng(0)."""
        d = _draws(number_of_points, rng, draws)
        dev = torch.device(device)
        N, F, Nv = d.shape[0], self.triangles.shape[0], self.vertices.shape[0]
        verts, tris = torch.as_tensor(self.vertices).to(dev), torch.as_tensor(self.triangles).to(dev)
        draws_d = torch.as_tensor(d).to(dev)
        ws_bytes = _lib.load().sv_mesh_sample_workspace_bytes(c_int64(F))
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        points = torch.empty((N, 3), dtype=torch.float64, device=dev)
        normals = torch.empty((N, 3), dtype=torch.float64, device=dev)
        tri = torch.empty(N, dtype=torch.int32, device=dev)
        area = torch.empty(1, dtype=torch.float64, device=dev)
        counters = torch.zeros(1, dtype=torch.int32, device=dev)
        call("sv_mesh_sample", ptr(verts), c_int64(Nv), ptr(tris), c_int64(F), ptr(draws_d), c_int64(N), ptr(ws),
             c_size_t(ws_bytes), ptr(points), ptr(normals), ptr(tri), ptr(area), ptr(counters), stream_ptr())
        a = float(area.item())
        if not (a > 0 and math.isfinite(a)):
            raise ValueError(f"the mesh has no usable surface (area {a!r}, {int(counters.item())} of {F} triangles "
                             "with an index outside the vertex list)")
        return PointCloud(points, normals, tri, a)

    def sample_points_poisson_disk(self, number_of_points, init_factor=5, pcl=None, rng=None, device="cuda"):
        """The number_of_points rows of pcl (None: init_factor * number_of_points uniform samples) that weighted sample
        elimination leaves, in ascending order."""
        n = int(number_of_points)
        if n < 1:
            raise ValueError(f"number_of_points must be positive, got {number_of_points!r}")
        if pcl is None:
            if int(init_factor) < 1:
                raise ValueError(f"init_factor must be at least 1, got {init_factor!r}")
            pcl = self.sample_points_uniformly(int(init_factor) * n, rng=rng, device=device)
        N = len(pcl)
        if not n <= N <= MAX_ELIMINATE:
            raise ValueError(f"pcl must hold between number_of_points ({n}) and 65536 points, got {N}")
        r_max, r_min = eliminate_radii(pcl.surface_area, N, n)
        kept, _, _ = sample_eliminate(pcl.points, n, r_max, r_min, device=device)
        rows = torch.as_tensor(kept.astype(np.int64)).to(pcl.points.device)
        return PointCloud(pcl.points[rows], pcl.normals[rows], pcl.triangle[rows], pcl.surface_area)


def load_cad_model(cad_name, n_init=16384, n_points=8192, rng=None, device="cuda"):
    """utils/icp.py:17-40 -> (points float32 [M,3], normals float32 [M,3] or None) as host arrays.  A .pcd file gives its
    points as they are (no normals, no mask, no thinning, as the reference); anything else is read as a mesh, sampled
    (n_init), thinned (n_points) and masked."""
    cad_name = os.fspath(cad_name)
    if cad_name.endswith(".pcd"):
        return read_point_cloud(cad_name).astype(np.float32), None
    mesh = read_triangle_mesh(cad_name)
    pcl = mesh.sample_points_uniformly(n_init, rng=rng, device=device)
    pcl = mesh.sample_points_poisson_disk(n_points, pcl=pcl, device=device)
    points, normals = pcl.points.cpu().numpy(), pcl.normals.cpu().numpy()
    # the reference's mask, as written there: `0.0 * (z > -0.02)` is 0.0 for every row, so it keeps exactly x > 0
    mask = points[:, 0] > 0.0 * (points[:, 2] > -0.02)
    return points[mask].astype(np.float32), normals[mask].astype(np.float32)


def is_path(x):
    """what the matchers and the engine take as a CAD file name rather than as points"""
    return isinstance(x, (str, os.PathLike))
