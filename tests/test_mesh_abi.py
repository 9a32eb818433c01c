"""Argument checks of sv_mesh_sample and sv_sample_eliminate and of their Python wrappers (utils/mesh.py, the matchers
and the engine taking a CAD file's path): host code only, no GPU needed.  As tests/test_icp_batch_abi.py: every library
call here fails its checks before any HIP call, and the wrappers reject bad arguments before a tensor is moved, which the
`no_launch` fixture enforces."""
import ctypes

import numpy as np
import pytest

NAN, INF = float("nan"), float("inf")
NAMES = ("sv_mesh_sample_workspace_bytes", "sv_mesh_sample", "sv_sample_eliminate_workspace_bytes",
         "sv_sample_eliminate")


def _buf(n=64):
    """A host buffer standing in for a non-null pointer (never dereferenced: every call here fails its checks)."""
    return ctypes.create_string_buffer(n)


def test_symbols_are_exported_and_declared():
    import mrcc_amd

    lib = mrcc_amd._lib.load()
    for name in NAMES:
        assert name in mrcc_amd._lib.SIGNATURES
        assert getattr(lib, name) is not None
    assert len(mrcc_amd._lib.SIGNATURES["sv_mesh_sample"][1]) == 14
    assert len(mrcc_amd._lib.SIGNATURES["sv_sample_eliminate"][1]) == 12
    assert lib.sv_abi_version() == 4


def test_workspace_sizes_are_monotone():
    import mrcc_amd

    lib = mrcc_amd._lib.load()
    mesh, elim = lib.sv_mesh_sample_workspace_bytes, lib.sv_sample_eliminate_workspace_bytes
    assert mesh(1) >= 8 and mesh(2120) >= 2120 * 8 and mesh(1 << 20) >= (1 << 20) * 8
    sizes = [mesh(F) for F in (1, 31, 32, 33, 2120, 100000, 1 << 20)]
    assert sizes == sorted(sizes) and sizes[-1] > sizes[0]
    assert elim(16384, 64) >= 16384 * 64 * 4 + 16384 * 8
    by_n = [elim(N, 64) for N in (1, 2, 300, 4096, 16384, 16385, 65536)]
    assert by_n == sorted(by_n) and len(set(by_n)) == len(by_n)
    by_degree = [elim(4096, d) for d in (1, 8, 64, 128, 1024)]
    assert by_degree == sorted(by_degree) and len(set(by_degree)) == len(by_degree)
    assert elim(65536, 1024) >= 65536 * 1024 * 4  # computed in 64 bits


def test_mesh_sample_argument_checks_without_gpu():
    import mrcc_amd

    lib = mrcc_amd._lib.load()
    p = _buf()
    need = lib.sv_mesh_sample_workspace_bytes(10)

    def sample(Nv=8, F=10, N=5, ws_bytes=need, **ptrs):
        a = dict(verts=p, tris=p, draws=p, ws=p, points=p, normals=p, tri=p, area=p, counters=p)
        a.update(ptrs)
        return lib.sv_mesh_sample(a["verts"], Nv, a["tris"], F, a["draws"], N, a["ws"], ws_bytes, a["points"],
                                  a["normals"], a["tri"], a["area"], a["counters"], None)

    for kw in ({"F": 0}, {"F": -1}, {"F": (1 << 20) + 1}):
        assert sample(**kw) == -1 and b"triangles" in lib.sv_last_error(), kw
    for kw in ({"N": 0}, {"N": -3}, {"N": (1 << 20) + 1}):
        assert sample(**kw) == -1 and b"samples" in lib.sv_last_error(), kw
    for kw in ({"Nv": 0}, {"Nv": -1}):
        assert sample(**kw) == -1 and b"vertex" in lib.sv_last_error(), kw
    for name in ("verts", "tris", "draws", "ws", "points", "normals", "tri", "area", "counters"):
        assert sample(**{name: None}) == -1 and b"null pointer" in lib.sv_last_error(), name
    for ws_bytes in (0, 8, need - 1):
        assert sample(ws_bytes=ws_bytes) == -2 and b"workspace too small" in lib.sv_last_error(), ws_bytes
    assert b"sv_mesh_sample" in lib.sv_last_error()


def test_sample_eliminate_argument_checks_without_gpu():
    import mrcc_amd

    lib = mrcc_amd._lib.load()
    p = _buf()
    need = lib.sv_sample_eliminate_workspace_bytes(100, 8)

    def eliminate(N=100, n_keep=50, r_max=0.5, r_min=0.1, max_degree=8, ws_bytes=need, **ptrs):
        a = dict(points=p, ws=p, kept=p, order=p, counters=p)
        a.update(ptrs)
        return lib.sv_sample_eliminate(a["points"], N, n_keep, r_max, r_min, max_degree, a["ws"], ws_bytes, a["kept"],
                                       a["order"], a["counters"], None)

    for kw in ({"N": 0}, {"N": -1}, {"N": 65537}):
        assert eliminate(**kw) == -1 and b"1 to 65536 points" in lib.sv_last_error(), kw
    for kw in ({"n_keep": 0}, {"n_keep": -1}, {"n_keep": 101}):
        assert eliminate(**kw) == -1 and b"n_keep" in lib.sv_last_error(), kw
    for kw in ({"max_degree": 0}, {"max_degree": -8}, {"max_degree": 1025}):
        assert eliminate(**kw) == -1 and b"max_degree" in lib.sv_last_error(), kw
    for kw in ({"r_max": 0.0}, {"r_max": -0.5}, {"r_max": NAN}, {"r_max": INF}):
        assert eliminate(**kw) == -1 and b"r_max" in lib.sv_last_error(), kw
    for kw in ({"r_min": 0.6}, {"r_min": -0.1}, {"r_min": NAN}):
        assert eliminate(**kw) == -1 and b"r_min" in lib.sv_last_error(), kw
    for name in ("points", "ws", "kept", "order", "counters"):
        assert eliminate(**{name: None}) == -1 and b"null pointer" in lib.sv_last_error(), name
    for ws_bytes in (0, 256, need // 2, need - 1):
        assert eliminate(ws_bytes=ws_bytes) == -2 and b"workspace too small" in lib.sv_last_error(), ws_bytes
    assert b"sv_sample_eliminate" in lib.sv_last_error()
    # one size does not fit a larger table
    assert eliminate(max_degree=16) == -2 and eliminate(N=101, n_keep=50) == -2


@pytest.fixture
def no_launch(monkeypatch):
    """Replace the wrappers' library call and the tensor constructor they move data with: reaching either means a bad
    argument got past the checks."""
    from mrcc_amd.utils import mesh

    def fail(name, *args):
        raise AssertionError(f"{name} was called with arguments the wrapper should have rejected")

    def no_tensor(*args, **kw):
        raise AssertionError("a tensor was created for arguments the wrapper should have rejected")

    monkeypatch.setattr(mesh, "call", fail)
    monkeypatch.setattr(mesh.torch, "as_tensor", no_tensor)
    monkeypatch.setattr(mesh.torch, "empty", no_tensor)


def _mesh():
    from mrcc_amd.utils.mesh import TriangleMesh

    return TriangleMesh(np.array([[0.0, 0, 0], [1, 0, 0], [0, 1, 0]]), np.array([[0, 1, 2]]))


def test_triangle_mesh_rejects_bad_arrays():
    from mrcc_amd.utils.mesh import TriangleMesh

    v, t = np.zeros((3, 3)), np.array([[0, 1, 2]])
    for verts, tris, word in ((np.zeros((3, 2)), t, "vertices"), (np.zeros((0, 3)), t, "vertices"),
                              (np.zeros(9), t, "vertices"), (v, np.zeros((0, 3), int), "triangles"),
                              (v, np.array([[0, 1]]), "triangles"), (v, np.array([0, 1, 2]), "triangles")):
        with pytest.raises(ValueError, match=word):
            TriangleMesh(verts, tris)
    mesh = TriangleMesh(v.astype(np.float32), t.astype(np.int64))
    assert mesh.vertices.dtype == np.float64 and mesh.triangles.dtype == np.int32


def test_sampling_wrappers_reject_bad_arguments(no_launch):
    import torch

    mesh = _mesh()
    for n in (0, -1, (1 << 20) + 1):
        with pytest.raises(ValueError, match="number_of_points"):
            mesh.sample_points_uniformly(n)
    good = np.full((4, 3), 0.5)
    for draws, word in ((good[:, :2], "draws"), (good.ravel(), "draws"), (good[:0], "draws"),
                        (good.astype(np.float32), "float64"), (good * 2.0, r"\[0, 1\)"), (good - 1.0, r"\[0, 1\)"),
                        (np.full((4, 3), NAN), r"\[0, 1\)"), (torch.zeros(4, 3, dtype=torch.float64), "host array")):
        with pytest.raises(ValueError, match=word):
            mesh.sample_points_uniformly(draws=draws)
    with pytest.raises(ValueError, match="number_of_points"):
        mesh.sample_points_uniformly(5, draws=good)
    with pytest.raises(ValueError, match="number_of_points"):
        mesh.sample_points_poisson_disk(0)
    with pytest.raises(ValueError, match="init_factor"):
        mesh.sample_points_poisson_disk(8, init_factor=0)


def test_eliminate_wrapper_rejects_bad_arguments(no_launch):
    from mrcc_amd.utils.mesh import PointCloud, sample_eliminate

    pts = np.zeros((10, 3))
    for p, word in ((pts[:, :2], "points"), (pts.ravel(), "points"), (pts[:0], "rows"), (np.zeros((65537, 3)), "rows"),
                    (pts.astype(np.float32), "float64")):
        with pytest.raises(ValueError, match=word):
            sample_eliminate(p, 1, 0.5, 0.1)
    for kw, word in (({"n_keep": 0}, "n_keep"), ({"n_keep": 11}, "n_keep"), ({"r_max": 0.0}, "r_max"),
                     ({"r_max": -1.0}, "r_max"), ({"r_max": NAN}, "r_max"), ({"r_max": INF}, "r_max"),
                     ({"r_min": 0.6}, "r_min"), ({"r_min": -0.1}, "r_min"), ({"r_min": NAN}, "r_min"),
                     ({"max_degree": 0}, "max_degree"), ({"max_degree": 1025}, "max_degree")):
        args = {"n_keep": 5, "r_max": 0.5, "r_min": 0.1, "max_degree": 64}
        args.update(kw)
        with pytest.raises(ValueError, match=word):
            sample_eliminate(pts, **args)
    # a cloud given to sample_points_poisson_disk must hold at least the points asked for and at most 65536
    small = PointCloud(points=np.zeros((10, 3)), normals=np.zeros((10, 3)), triangle=np.zeros(10, np.int32),
                       surface_area=1.0)
    with pytest.raises(ValueError, match="pcl"):
        _mesh().sample_points_poisson_disk(11, pcl=small)


def test_matchers_and_engine_without_points_or_path_still_name_cad_points():
    from mrcc_amd.app.inference_engine import InferenceEngine
    from mrcc_amd.utils import icp as I
    from mrcc_amd.utils.config import Config

    for make in (I.get_point2point_matcher, I.get_point2plane_matcher, I.PointToPointMatcher, I.PointToPlaneMatcher):
        with pytest.raises(ValueError, match="cad_points"):
            make(None, device="cpu")
    Config.reset()
    assert Config()()["INFERENCE"]["cad_name"] is None and Config().INFERENCE.icp_enabled is False
    Config().update({"INFERENCE": {"icp_enabled": True}})
    try:
        with pytest.raises(ValueError, match="INFERENCE.icp_enabled needs cad_points"):
            InferenceEngine(calibration_only=True)
    finally:
        Config.reset()
    engine = InferenceEngine(calibration_only=True)
    assert engine.cad_points is None and engine.match_icp is None


def test_a_missing_cad_file_is_reported_by_name(tmp_path):
    from mrcc_amd.utils import icp as I
    from mrcc_amd.utils.mesh import load_cad_model

    for name in ("nothing.obj", "nothing.pcd"):
        with pytest.raises(FileNotFoundError, match=name):
            load_cad_model(tmp_path / name, device="cpu")
    with pytest.raises(FileNotFoundError, match="nothing.obj"):
        I.get_point2point_matcher(str(tmp_path / "nothing.obj"), device="cpu")


def test_pcd_model_loads_without_a_device():
    """the .pcd branch is host code: the file's points as float32, no normals, no mask"""
    import mesh_helpers as H
    from mrcc_amd.utils.mesh import load_cad_model, read_point_cloud

    points, normals = load_cad_model(H.HAND_PCD, device="cpu")
    assert normals is None and points.dtype == np.float32 and points.shape == (4480, 3)
    assert np.array_equal(points, read_point_cloud(H.HAND_PCD).astype(np.float32))
    assert (points[:, 0] <= 0).any()  # not masked
