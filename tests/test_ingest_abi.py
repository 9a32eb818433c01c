"""Argument checks of sv_unpack_points and of its Python wrappers (utils/packed.py, the packed frame stream): host code
only, no GPU needed.  As tests/test_mesh_abi.py: every library call here fails its checks before any HIP call, and the
wrappers reject bad layouts before a tensor is moved, which the `no_launch` fixture enforces."""
import ctypes

import numpy as np
import pytest

NAN = float("nan")
NAMES = ("sv_unpack_points_workspace_bytes", "sv_unpack_points")
F32, F64 = 7, 8


def _buf(n=64):
    """A host buffer standing in for a non-null pointer (never dereferenced: every call here fails its checks)."""
    return ctypes.create_string_buffer(n)


def test_symbols_are_exported_and_declared():
    import mrcc_amd

    lib = mrcc_amd._lib.load()
    for name in NAMES:
        assert name in mrcc_amd._lib.SIGNATURES
        assert getattr(lib, name) is not None
    assert len(mrcc_amd._lib.SIGNATURES["sv_unpack_points"][1]) == 21
    assert lib.sv_abi_version() == 4
    L = mrcc_amd._lib
    assert (L.SV_FIELD_F32, L.SV_FIELD_F64) == (7, 8)
    assert (L.SV_UNPACK_BIGENDIAN, L.SV_UNPACK_KEEP_NONFINITE) == (1, 2)


def test_workspace_sizes_are_monotone_and_64_bit():
    import mrcc_amd

    ws = mrcc_amd._lib.load().sv_unpack_points_workspace_bytes
    sizes = [ws(n) for n in (1, 255, 256, 257, 70001, 307200, 1 << 24)]
    assert sizes == sorted(sizes) and sizes[-1] > sizes[0]
    assert ws(1) >= 4 and ws(307200) >= 1200 * 4 and ws(1 << 24) >= (1 << 16) * 4
    assert ws(0) == ws(-5) and ws(0) <= ws(1)
    assert ws(1 << 40) >= (1 << 32) * 4  # computed in 64 bits


def test_unpack_points_argument_checks_without_gpu():
    import mrcc_amd

    lib = mrcc_amd._lib.load()
    p = _buf()
    need = lib.sv_unpack_points_workspace_bytes(100)
    box_t = ctypes.c_double * 6

    def unpack(n=100, data_bytes=3200, width=100, step=32, row_step=3200, x=0, y=4, z=8, typ=F32, rgb_off=16, flags=0,
               box=None, ws_bytes=need, **ptrs):
        a = dict(data=p, lut=None, ws=p, points=p, rgb=p, src=p, count=p)
        a.update(ptrs)
        return lib.sv_unpack_points(a["data"], data_bytes, n, width, step, row_step, x, y, z, typ, rgb_off, flags,
                                    None if box is None else box_t(*box), a["lut"], a["ws"], ws_bytes, a["points"],
                                    a["rgb"], a["src"], a["count"], None)

    def rejected(word, **kw):
        assert unpack(**kw) == -1 and word in lib.sv_last_error(), (kw, lib.sv_last_error())

    for n in (0, -1, (1 << 24) + 1):
        rejected(b"records", n=n)
    for width in (0, -7):
        rejected(b"width", width=width)
    for step in (0, -32, 4097):
        rejected(b"point_step", step=step)
    for kw in ({"row_step": 3199}, {"row_step": 0}, {"row_step": -3200}, {"width": 1 << 62, "row_step": 1 << 40}):
        rejected(b"row_step", **kw)
    for typ in (0, 6, 9):
        rejected(b"xyz_type", typ=typ)
    for flags in (4, 8, -1):
        rejected(b"flags", flags=flags)
    for kw in ({"x": -1}, {"y": 29}, {"z": 32}, {"typ": F64, "x": 0, "y": 8, "z": 25}, {"x": 1 << 30}):
        rejected(b"outside the record", **kw)
    for rgb_off in (29, 32, 1 << 30):
        rejected(b"rgb field lies outside", rgb_off=rgb_off)
    for kw in ({"y": 0}, {"y": 2}, {"z": 5}, {"typ": F64, "x": 0, "y": 4, "z": 16, "rgb_off": 24}):
        rejected(b"x, y and z fields overlap", **kw)
    for kw in ({"rgb_off": 0}, {"rgb_off": 10}, {"rgb_off": 5}, {"typ": F64, "x": 0, "y": 8, "z": 16, "rgb_off": 20}):
        rejected(b"rgb field overlaps", **kw)
    # the last record must end inside the buffer: one row, several rows, row padding, a short last row
    for kw in ({"data_bytes": 3199}, {"data_bytes": 0}, {"data_bytes": -1},
               {"width": 10, "row_step": 332, "data_bytes": 9 * 332 + 319},
               {"n": 95, "width": 10, "row_step": 320, "data_bytes": 9 * 320 + 5 * 32 - 1},
               {"width": 1, "row_step": 1 << 50, "data_bytes": 1 << 40}):
        rejected(b"data_bytes", **kw)
    for box in ((NAN, 0, 0, 1, 1, 1), (0, 0, 0, 1, NAN, 1)):
        rejected(b"NaN", box=box)
    for box in ((2, 0, 0, 1, 1, 1), (0, 0, 1.5, 1, 1, 1)):
        rejected(b"lo <= hi", box=box)
    for name in ("data", "ws", "points", "rgb", "count"):
        rejected(b"null pointer", **{name: None})
    for ws_bytes in (0, 8, need - 1):
        assert unpack(ws_bytes=ws_bytes) == -2 and b"workspace too small" in lib.sv_last_error(), ws_bytes
    assert b"sv_unpack_points" in lib.sv_last_error()
    assert unpack(n=1 << 20, data_bytes=32 << 20, width=1 << 20, row_step=32 << 20) == -2  # one size does not fit more


@pytest.fixture
def no_launch(monkeypatch):
    """Replace the wrappers' library call and the tensor constructors they move data with: reaching either means a bad
    argument got past the checks."""
    from mrcc_amd.utils import packed

    def fail(name, *args):
        raise AssertionError(f"{name} was called with arguments the wrapper should have rejected")

    def no_tensor(*args, **kw):
        raise AssertionError("a tensor was created for arguments the wrapper should have rejected")

    monkeypatch.setattr(packed, "call", fail)
    monkeypatch.setattr(packed.torch, "empty", no_tensor)
    monkeypatch.setattr(packed.torch, "from_numpy", no_tensor)
    monkeypatch.setattr(packed.torch, "as_tensor", no_tensor)


def _fields(**over):
    from mrcc_amd.utils.packed import Field

    rows = {"x": ("x", 0, F32), "y": ("y", 4, F32), "z": ("z", 8, F32), "rgb": ("rgb", 16, F32)}
    rows.update(over)
    return [Field(*r) for r in rows.values() if r is not None]


def test_packed_frame_rejects_bad_layouts(no_launch):
    from mrcc_amd.utils.packed import PackedFrame

    data = bytes(3200)
    PackedFrame(data, 100, 1, 32, 3200, _fields())  # the layout the cases below break
    cases = [
        (dict(point_step=0), "point_step"), (dict(point_step=4097, row_step=409700), "point_step"),
        (dict(row_step=3199), "row_step"), (dict(width=-1), "negative"), (dict(width=1 << 13, height=1 << 12), "2\\^24"),
        (dict(width=101, row_step=3232), "last record ends"), (dict(height=2), "last record ends"),
        (dict(fields=_fields(x=None)), "no scalar field 'x'"), (dict(fields=_fields(z=("z", 8, F32, 2))), "no scalar field 'z'"),
        (dict(fields=_fields(y=("y", 4, 5))), "FLOAT32 or FLOAT64"), (dict(fields=_fields(y=("y", 4, 99))), "unknown datatype"),
        (dict(fields=_fields(y=("y", 24, F64))), "share one datatype"),
        (dict(fields=_fields(rgb=("rgb", 16, 2))), "4-byte"), (dict(fields=_fields(rgb=("rgb", 16, F32, 2))), "4-byte"),
        (dict(fields=_fields(rgb=("rgb", 30, F32))), "outside"), (dict(fields=_fields(x=("x", -1, F32))), "outside"),
        (dict(fields=_fields(y=("y", 2, F32))), "overlap"), (dict(fields=_fields(rgb=("rgb", 10, F32))), "overlap"),
    ]
    for change, word in cases:
        kw = dict(data=data, width=100, height=1, point_step=32, row_step=3200, fields=_fields())
        kw.update(change)
        with pytest.raises(ValueError, match=word):
            PackedFrame(**kw)
    with pytest.raises(ValueError, match="uint8"):
        PackedFrame(np.zeros(800, np.float32), 100, 1, 32, 3200, _fields())


def test_decode_wrappers_reject_bad_arguments(no_launch):
    from mrcc_amd._lib import SvHipError
    from mrcc_amd.utils.packed import PackedFrame

    frame = PackedFrame(bytes(3200), 100, 1, 32, 3200, _fields())
    for box, word in (((0, 0, 0, 1, 1), "6 values"), ((NAN, 0, 0, 1, 1, 1), "NaN"), ((2, 0, 0, 1, 1, 1), "lo <= hi")):
        for fn in (lambda: frame.decode_device("cuda:0", box=box), lambda: frame.decode_host(box=box),
                   lambda: frame.unpack(None, box=box)):
            with pytest.raises(ValueError, match=word):
                fn()
    with pytest.raises(SvHipError, match="no CPU fallback"):
        frame.decode_device("cpu")
    with pytest.raises(ValueError, match="color"):
        frame.decode_device("cuda:0", lut="uint8")
    with pytest.raises(ValueError, match="color"):
        frame.decode_host(color="rgb")
    with pytest.raises(IndexError):
        frame.take([100])
    with pytest.raises(ValueError, match="same length"):
        frame.scatter(np.zeros(3), np.zeros(4, np.int64))


def test_packed_stream_rejects_an_unknown_colour_convention_before_allocating(no_launch, monkeypatch):
    from mrcc_amd.app import pipeline

    def no_pipe(*a, **kw):
        raise AssertionError("streams were created for a colour convention the stream should have rejected")

    monkeypatch.setattr(pipeline, "FramePipeline", no_pipe)
    with pytest.raises(ValueError, match="float64"):
        pipeline.PackedFrameStream("cuda:0", 50, stage=None, color="bytes")
