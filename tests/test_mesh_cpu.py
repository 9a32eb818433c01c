"""The host readers of utils/mesh.py (read_triangle_mesh for Wavefront OBJ, read_point_cloud for .pcd) on files written
by the tests and on the two fixtures tests/golden/hand_notblender.obj and hand.pcd.  Host code only, no GPU needed."""
import struct

import numpy as np
import pytest

import mesh_helpers as H


def _write(tmp_path, name, text):
    path = tmp_path / name
    if isinstance(text, bytes):
        path.write_bytes(text)
    else:
        path.write_text(text)
    return path


def test_obj_face_token_forms_and_ignored_records(tmp_path):
    from mrcc_amd.utils.mesh import read_triangle_mesh

    path = _write(tmp_path, "forms.obj", """# a comment
mtllib nothing.mtl
o thing
v 0 0 0
v 1 0 0 1.0
v 0 1 0 0.5 0.5 0.5
v 0 0 1
vt 0.5 0.5
vn 0 0 1
g group
usemtl none
s off
f 1 2 3
f 1/1 2/1 4/1
f 1//1 3//1 4//1

f 2/1/1 3/1/1 4/1/1
l 1 2
""")
    mesh = read_triangle_mesh(path)  # a pathlib.Path is taken as well as a str
    assert mesh.vertices.dtype == np.float64 and mesh.triangles.dtype == np.int32
    assert np.array_equal(mesh.vertices, [[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]])  # extra columns ignored
    assert np.array_equal(mesh.triangles, [[0, 1, 2], [0, 1, 3], [0, 2, 3], [1, 2, 3]])
    assert np.array_equal(read_triangle_mesh(str(path)).triangles, mesh.triangles)


def test_obj_negative_indices_are_relative_to_the_vertices_so_far(tmp_path):
    from mrcc_amd.utils.mesh import read_triangle_mesh

    path = _write(tmp_path, "neg.obj", "v 0 0 0\nv 1 0 0\nv 0 1 0\nf -3 -2 -1\nv 0 0 1\nf -1 -2//7 -4/2/2\n")
    assert np.array_equal(read_triangle_mesh(path).triangles, [[0, 1, 2], [3, 2, 0]])


def test_obj_polygons_are_fan_triangulated(tmp_path):
    from mrcc_amd.utils.mesh import read_triangle_mesh

    text = "".join(f"v {np.cos(k)} {np.sin(k)} 0\n" for k in range(5)) + "f 1 2 3 4\nf 1//1 2//1 3//1 4//1 5//1\n"
    mesh = read_triangle_mesh(_write(tmp_path, "poly.obj", text))
    assert np.array_equal(mesh.triangles, [[0, 1, 2], [0, 2, 3], [0, 1, 2], [0, 2, 3], [0, 3, 4]])


@pytest.mark.parametrize("text, line, word", [
    ("v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 4\n", 4, "outside the vertex list"),
    ("v 0 0 0\nv 1 0 0\nv 0 1 0\n# c\nf 1 2 0\n", 5, "outside the vertex list"),
    ("v 0 0 0\nv 1 0 0\nv 0 1 0\nf -1 -2 -4\n", 4, "outside the vertex list"),
    ("v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 3\nf 1 2\n", 5, "at least three corners"),
    ("v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1\n", 4, "at least three corners"),
])
def test_obj_errors_name_the_file_and_the_line(tmp_path, text, line, word):
    from mrcc_amd.utils.mesh import read_triangle_mesh

    path = _write(tmp_path, "bad.obj", text)
    with pytest.raises(ValueError, match=word) as err:
        read_triangle_mesh(path)
    assert f"{path}:{line}:" in str(err.value)


def test_obj_without_a_face_is_an_error(tmp_path):
    from mrcc_amd.utils.mesh import read_triangle_mesh

    path = _write(tmp_path, "cloud.obj", "v 0 0 0\nv 1 0 0\nv 0 1 0\n")
    with pytest.raises(ValueError, match="no face") as err:
        read_triangle_mesh(path)
    assert str(path) in str(err.value)


def test_fixture_obj_counts_area_and_box():
    from mrcc_amd.utils.mesh import read_triangle_mesh

    mesh = read_triangle_mesh(H.HAND_OBJ)
    assert mesh.vertices.shape == (1115, 3) and mesh.triangles.shape == (2120, 3)
    verts, tris = H.parse_obj(H.HAND_OBJ)  # the helper's own parser reads the same mesh
    assert np.array_equal(H.bits(mesh.vertices), H.bits(verts)) and np.array_equal(mesh.triangles, tris)
    a = H.triangle_areas(mesh.vertices, mesh.triangles)[0]
    assert (a > 0).all()
    assert abs(H.running_sums(a)[-1] - H.HAND_AREA) <= 1e-12 * H.HAND_AREA
    assert np.allclose(mesh.vertices.min(0), [-0.0316, -0.1039, -0.0260], atol=2e-4)
    assert np.allclose(mesh.vertices.max(0), [0.0316, 0.1006, 0.0660], atol=2e-4)


def _pcd_header(fields, sizes, types, n, data):
    return ("# .PCD v0.7 - Point Cloud Data file format\nVERSION 0.7\n"
            f"FIELDS {' '.join(fields)}\nSIZE {' '.join(map(str, sizes))}\nTYPE {' '.join(types)}\n"
            f"COUNT {' '.join('1' for _ in fields)}\nWIDTH {n}\nHEIGHT 1\nVIEWPOINT 0 0 0 1 0 0 0\nPOINTS {n}\n"
            f"DATA {data}\n")


def test_pcd_ascii_round_trip(tmp_path):
    from mrcc_amd.utils.mesh import read_point_cloud

    pts = np.random.default_rng(3).normal(size=(17, 3))
    body = "".join(f"{i} {p[0]!r} {p[1]!r} {p[2]!r} 4.2e+06\n" for i, p in enumerate(pts.tolist()))
    path = _write(tmp_path, "a.pcd", _pcd_header(["id", "x", "y", "z", "rgb"], [4, 8, 8, 8, 4], "I F F F F".split(), 17,
                                                 "ascii") + body)
    got = read_point_cloud(path)
    assert got.dtype == np.float64 and np.array_equal(H.bits(got), H.bits(pts))


def test_pcd_binary_round_trip_skips_other_fields_by_size(tmp_path):
    from mrcc_amd.utils.mesh import read_point_cloud

    pts = np.random.default_rng(4).normal(size=(9, 3)).astype(np.float32)
    # x and z float32, y float64, between them a 2-byte label, a packed rgb and a 1-byte flag
    body = b"".join(struct.pack("<fHdIfB", p[0], 7 + i, float(p[1]), 0x00ff8040, p[2], i)
                    for i, p in enumerate(pts))
    head = _pcd_header(["x", "label", "y", "rgb", "z", "flag"], [4, 2, 8, 4, 4, 1], "F U F U F U".split(), 9, "binary")
    got = read_point_cloud(_write(tmp_path, "b.pcd", head.encode() + body))
    assert got.dtype == np.float64 and np.array_equal(got, pts.astype(np.float64))


def test_pcd_compressed_and_broken_files(tmp_path):
    from mrcc_amd.utils.mesh import read_point_cloud

    head = _pcd_header(["x", "y", "z"], [4, 4, 4], "F F F".split(), 2, "binary_compressed")
    with pytest.raises(NotImplementedError, match="binary_compressed"):
        read_point_cloud(_write(tmp_path, "c.pcd", head.encode() + b"\0" * 32))
    head = _pcd_header(["x", "y", "z"], [4, 4, 4], "F F F".split(), 3, "binary")
    with pytest.raises(ValueError, match="bytes of data"):
        read_point_cloud(_write(tmp_path, "short.pcd", head.encode() + b"\0" * 35))
    head = _pcd_header(["x", "y"], [4, 4], "F F".split(), 1, "ascii")
    with pytest.raises(ValueError, match="'z'"):
        read_point_cloud(_write(tmp_path, "xy.pcd", head + "0 0\n"))
    with pytest.raises(ValueError, match="DATA"):
        read_point_cloud(_write(tmp_path, "none.pcd", "FIELDS x y z\n"))


def test_fixture_pcd():
    from mrcc_amd.utils.mesh import read_point_cloud

    pts = read_point_cloud(H.HAND_PCD)
    assert pts.shape == (4480, 3) and pts.dtype == np.float64 and np.isfinite(pts).all()
    raw = open(H.HAND_PCD, "rb").read()
    data = raw[raw.index(b"DATA binary\n") + len(b"DATA binary\n"):]
    first = struct.unpack("<3f", data[:12])  # the first record: x y z, then 4 bytes of rgb
    last = struct.unpack("<3f", data[4479 * 16:4479 * 16 + 12])
    assert tuple(pts[0]) == first and tuple(pts[-1]) == last
    assert np.abs(pts).max() < 0.2  # a hand-sized cloud in metres


def test_eliminate_radii_match_the_restated_constants():
    from mrcc_amd.utils.mesh import eliminate_radii

    for area, n_points, n_keep in ((H.HAND_AREA, 16384, 8192), (256.0, 256, 128), (1.0, 300, 1), (2.5, 1024, 1024)):
        assert eliminate_radii(area, n_points, n_keep) == H.radii(area, n_points, n_keep)
    assert eliminate_radii(1.0, 10, 10)[1] == 0.0  # ratio 1: r_min = 0
