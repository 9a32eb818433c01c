"""Helpers of the RGB-D ingest tests: duck-typed image messages, a direct caller of sv_rgbd_cloud that lays the images out
in device memory itself (random bytes between the rows and in front of the colour image, so that nothing can rely on
them), and the comparison of every output with the numpy restatement (RGBDFrame.decode_host / decode_host64 /
registered_host, which tests/test_rgbd_cpu.py pins to the reference's own functions on tests/golden/rgbd_ycb.npz)."""
import ctypes
from types import SimpleNamespace

import numpy as np

U16, F32 = 4, 7  # SV_DEPTH_*
ALIGNED, NEAREST, BGR = 1, 2, 4  # SV_RGBD_*
SIMPLE_K = np.array([[1.0, 0, 0], [0, 1.0, 0], [0, 0, 1]])  # x = u * d, y = v * d: exact in float32 for small integers


def tiles():
    """(rows, columns) of the filter kernel's tile and the pixels per compaction tile, as the package exports them"""
    from mrcc_amd.utils import rgbd

    return rgbd.FILTER_TILE, rgbd.COMPACT_TILE


def image_msg(array, encoding, row_pad=0, big=False, fill=0x5A):
    """a sensor_msgs/Image look-alike of a [H, W] or [H, W, 3] array: rows of `step` bytes, `row_pad` bytes of `fill` each"""
    a = np.ascontiguousarray(array)
    h, w = a.shape[:2]
    row = a.reshape(h, -1).view(np.uint8)
    data = np.full((h, row.shape[1] + row_pad), fill, dtype=np.uint8)
    data[:, :row.shape[1]] = row
    return SimpleNamespace(height=h, width=w, encoding=encoding, is_bigendian=int(big), step=data.shape[1],
                           data=data.tobytes())


def camera_info(K):
    return SimpleNamespace(K=tuple(float(x) for x in np.asarray(K).reshape(-1)))


def filter_frame(depth, size, thresh):
    """an aligned frame whose registered map is the filtered depth itself (unit scale)"""
    from mrcc_amd.utils.rgbd import RGBDFrame

    return RGBDFrame(np.asarray(depth, dtype=np.uint16), None, SIMPLE_K, depth_scale=1.0, filter_size=size,
                     filter_thresh=thresh)


def _padded(image, pad, rng):
    """[H, ...] array -> (flat uint8 bytes of its rows with `pad` random bytes after each, row bytes)"""
    h = image.shape[0]
    row = np.ascontiguousarray(image).reshape(h, -1).view(np.uint8)
    out = rng.integers(0, 256, size=(h, row.shape[1] + pad), dtype=np.uint8)
    out[:, :row.shape[1]] = row
    return out.reshape(-1), row.shape[1] + pad


def run(frame, device, box=None, lut=None, depth_pad=0, color_pad=0, color_shift=0, want64=True, want_src=True,
        want_registered=True, seed=0):
    """sv_rgbd_cloud on `frame`'s images -> dict(points, points64, rgb, src, registered, count) of numpy arrays sliced to
    the count (None where not asked for), plus `count_tensor`, the device tensor the entry wrote.  color_shift: bytes
    the colour image is moved from its 256-aligned place (1 = an odd address)."""
    import torch

    import mrcc_amd
    from mrcc_amd._lib import call, ptr, stream_ptr

    rng = np.random.default_rng(seed)
    n = frame.Hc * frame.Wc
    d_bytes, d_row = _padded(frame.depth, depth_pad, rng)
    parts, c_off, m_off, c_row = [d_bytes], None, None, 0
    size = len(d_bytes)
    if frame.color is not None:
        c_bytes, c_row = _padded(frame.color, color_pad, rng)
        c_off = -(-size // 256) * 256 + color_shift
        parts += [rng.integers(0, 256, size=c_off - size, dtype=np.uint8), c_bytes]
        size = c_off + len(c_bytes)
    if frame.mask is not None:
        m_off = size
        parts.append(frame.mask.reshape(-1))
    dev = torch.from_numpy(np.concatenate(parts)).to(device)
    assert dev.data_ptr() % 256 == 0
    at = lambda off: None if off is None else ctypes.c_void_p(dev.data_ptr() + off)  # noqa: E731
    ws_bytes = mrcc_amd._lib.load().sv_rgbd_cloud_workspace_bytes(frame.Hd, frame.Wd, frame.Hc, frame.Wc)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=device)
    # outputs start as a pattern no result holds: an element the entry should have written cannot pass by luck
    points = torch.full((n, 3), -7.5, dtype=torch.float32, device=device)
    points64 = torch.full((n, 3), -7.5, dtype=torch.float64, device=device) if want64 else None
    rgb = torch.full((n, 3), -7.5, dtype=torch.float32, device=device) if frame.color is not None else None
    src = torch.full((n,), -7, dtype=torch.int32, device=device) if want_src else None
    registered = torch.full((n,), -7.5, dtype=torch.float64, device=device) if want_registered else None
    count = torch.full((1,), -7, dtype=torch.int64, device=device)
    d_lut = None if lut is None else torch.from_numpy(np.asarray(lut, dtype=np.float32)).to(device)
    call("sv_rgbd_cloud", at(0), frame.depth_type, frame.Hd, frame.Wd, d_row, at(c_off), frame.Hc, frame.Wc, c_row,
         at(m_off), (ctypes.c_double * 21)(*frame.cam()), frame.filter_size, frame.filter_thresh, frame.flags(),
         None if box is None else (ctypes.c_double * 6)(*box), ptr(d_lut), ptr(ws), ws_bytes, ptr(points), ptr(points64),
         ptr(rgb), ptr(src), ptr(registered), ptr(count), stream_ptr())
    assert count.is_cuda
    k = int(count.item())
    assert 0 <= k <= n
    host = lambda t: None if t is None else t.cpu().numpy()  # noqa: E731
    out = {name: (None if t is None else host(t)[:k]) for name, t in
           (("points", points), ("points64", points64), ("rgb", rgb), ("src", src))}
    out["registered"] = None if registered is None else host(registered).reshape(frame.Hc, frame.Wc)
    out["count"], out["count_tensor"] = k, count
    return out


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    view = {4: np.int32, 8: np.int64}[a.dtype.itemsize] if a.dtype.kind == "f" else a.dtype
    return np.array_equal(a.view(view), b.view(view))


def check(frame, device, box=None, lut=None, **layout):
    """run() and compare every output with the restatement, exactly -> run()'s dict"""
    out = run(frame, device, box=box, lut=lut, **layout)
    p32, rgb, src = frame.decode_host(box=box, color="bytes", lut=None if lut is None else np.asarray(lut, np.float32))
    p64, src64 = frame.decode_host64(box=box)
    assert out["count"] == len(src) and np.array_equal(src, src64)
    assert same_bits(out["points"], p32)
    if out["points64"] is not None:
        assert same_bits(out["points64"], p64)
    if out["src"] is not None:
        assert out["src"].dtype == np.int32 and np.array_equal(out["src"], src)
    if frame.color is not None:
        assert same_bits(out["rgb"], rgb.astype(np.float32))
    if out["registered"] is not None:
        assert same_bits(out["registered"], frame.registered_host())
    return out
