"""Strided kernel maps, local pooling and instance normalisation without a GPU: the entries are declared and exported, and
their argument checks (host code, nothing launched, no device pointer touched) answer SV_ERR_INVALID / SV_ERR_WORKSPACE."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = ctypes.c_void_p(1 << 20)  # never dereferenced: every call below fails its host-side checks first
INVALID, WORKSPACE = -1, -2

NEW_ENTRIES = ("sv_stride_map_general_workspace_bytes", "sv_stride_map_general", "sv_kernel_map_probe", "sv_pool_local",
               "sv_pool_local_backward", "sv_instance_norm_workspace_bytes", "sv_instance_norm", "sv_instance_norm_backward")


@pytest.fixture(scope="module")
def lib():
    import mrcc_amd

    return mrcc_amd._lib.load()


def test_entries_declared_exported_and_bound(lib):
    import mrcc_amd

    text = open(os.path.join(ROOT, "include", "sv_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(sv_[a-z0-9_]+)\s*\(", text))
    for name in NEW_ENTRIES:
        assert name in declared, f"{name} is not declared in include/sv_hip.h"
        assert hasattr(lib, name), f"{name} is not exported by libsvhip.so"
        assert name in mrcc_amd._lib.SIGNATURES
    assert lib.sv_abi_version() == 4 == mrcc_amd._lib.ABI_VERSION
    m = re.search(r"#define\s+SV_NORM_CHUNK_ROWS\s+(\d+)", text)
    assert m and int(m.group(1)) == mrcc_amd._lib.SV_NORM_CHUNK_ROWS
    assert re.search(r"#define\s+SV_POOL_SUM\s+2\b", text) and re.search(r"#define\s+SV_ACT_GELU\s+3\b", text)


def _stride(lib, keys=FAKE, V=10, s_in=2, s_out=6, ws=FAKE, ws_bytes=None, keys_out=FAKE, vc=FAKE, parent=FAKE, counters=FAKE):
    if ws_bytes is None:
        ws_bytes = lib.sv_stride_map_general_workspace_bytes(V)
    return lib.sv_stride_map_general(keys, V, s_in, s_out, ws, ws_bytes, keys_out, vc, parent, counters, None)


def test_stride_map_general_checks(lib):
    for kw in ({"keys": None}, {"keys_out": None}, {"vc": None}, {"parent": None}, {"ws": None}):
        assert _stride(lib, **kw) == INVALID and b"null pointer" in lib.sv_last_error(), kw
    assert _stride(lib, counters=None) == INVALID and b"counters" in lib.sv_last_error()
    for s_in, s_out in ((2, 5), (4, 6), (3, 4), (64, 96)):
        assert _stride(lib, s_in=s_in, s_out=s_out) == INVALID and b"multiple" in lib.sv_last_error(), (s_in, s_out)
    for s_in, s_out in ((0, 6), (-2, 6), (6, 2), (2, 1 << 18)):
        assert _stride(lib, s_in=s_in, s_out=s_out) == INVALID, (s_in, s_out)
    assert _stride(lib, V=-1) == INVALID
    need = lib.sv_stride_map_general_workspace_bytes(1000)
    assert need >= 1000 * (8 + 8 + 4 + 4)
    for have in (0, 1000 * 8, need // 2):
        assert _stride(lib, V=1000, ws_bytes=have) == WORKSPACE and b"workspace too small" in lib.sv_last_error()
    last = 0
    for V in (0, 1, 255, 256, 257, 5000, 88113, 1 << 22):
        b = lib.sv_stride_map_general_workspace_bytes(V)
        assert b >= last
        last = b


def _probe(lib, q=FAKE, V_q=10, ks=3, step=2, t=FAKE, V_t=10, tk=FAKE, tv=FAKE, cap=32, nbr=FAKE, ld=10, mask=FAKE):
    return lib.sv_kernel_map_probe(q, V_q, ks, step, t, V_t, tk, tv, cap, nbr, ld, mask, None)


def test_kernel_map_probe_checks(lib):
    for kw in ({"q": None}, {"t": None}, {"tk": None}, {"tv": None}, {"nbr": None}, {"mask": None}):
        assert _probe(lib, **kw) == INVALID and b"null pointer" in lib.sv_last_error(), kw
    for ks in (2, 0, 5, -3):
        assert _probe(lib, ks=ks) == INVALID and b"kernel_size" in lib.sv_last_error(), ks
    assert _probe(lib, ld=9) == INVALID and b"ld < V_q" in lib.sv_last_error()
    assert _probe(lib, step=0) == INVALID and b"step" in lib.sv_last_error()
    assert _probe(lib, step=1 << 18) == INVALID and b"step" in lib.sv_last_error()
    assert _probe(lib, cap=24) == INVALID and b"power of two" in lib.sv_last_error()
    assert _probe(lib, cap=16) == INVALID and b"power of two" in lib.sv_last_error()  # < 2 * V_t
    assert _probe(lib, V_q=0, q=None, nbr=None, mask=None) == 0  # nothing to do, nothing launched


def _pool(lib, in_=FAKE, V_in=20, in_ld=8, C=8, nbr=FAKE, ld=10, K=8, V_out=10, mode=0, out=FAKE, out_ld=8, arg=FAKE):
    return lib.sv_pool_local(in_, V_in, in_ld, C, nbr, ld, K, V_out, mode, out, out_ld, arg, None)


def _pool_bwd(lib, dy=FAKE, V_out=10, dy_ld=8, C=8, nbr_t=FAKE, ld_t=20, K=8, V_in=20, mode=0, arg=FAKE, mask=FAKE, dx=FAKE,
              dx_ld=8):
    return lib.sv_pool_local_backward(dy, V_out, dy_ld, C, nbr_t, ld_t, K, V_in, mode, arg, mask, dx, dx_ld, None)


def test_pool_local_checks(lib):
    for kw in ({"in_": None}, {"nbr": None}, {"out": None}, {"arg": None}):
        assert _pool(lib, **kw) == INVALID and b"null pointer" in lib.sv_last_error(), kw
    assert _pool(lib, ld=9) == INVALID and b"ld < V_out" in lib.sv_last_error()
    for kw in ({"mode": 3}, {"mode": -1}, {"K": 0}, {"K": 33}, {"C": 0}, {"in_ld": 7}, {"out_ld": 7}):
        assert _pool(lib, **kw) == INVALID, kw
    for kw in ({"dy": None}, {"nbr_t": None}, {"dx": None}, {"arg": None}, {"mode": 1, "mask": None}):
        assert _pool_bwd(lib, **kw) == INVALID and b"null pointer" in lib.sv_last_error(), kw
    assert _pool_bwd(lib, ld_t=19) == INVALID and b"ld_t < V_in" in lib.sv_last_error()
    for kw in ({"mode": 3}, {"K": 0}, {"K": 33}, {"C": 0}, {"dy_ld": 7}, {"dx_ld": 7}):
        assert _pool_bwd(lib, **kw) == INVALID, kw


def _norm(lib, x=FAKE, V=100, ld=8, C=8, bs=FAKE, B=2, w=FAKE, b=FAKE, act=0, ws=FAKE, ws_bytes=None, y=FAKE, y_ld=8, mean=FAKE,
          inv=FAKE):
    if ws_bytes is None:
        ws_bytes = lib.sv_instance_norm_workspace_bytes(V, B, C)
    return lib.sv_instance_norm(x, V, ld, C, bs, B, w, b, ctypes.c_double(1e-8), act, ws, ws_bytes, y, y_ld, mean, inv, None)


def _norm_bwd(lib, x=FAKE, V=100, ld=8, C=8, bs=FAKE, B=2, w=FAKE, b=FAKE, mean=FAKE, inv=FAKE, act=0, dy=FAKE, dy_ld=8,
              ws=FAKE, ws_bytes=None, dx=FAKE, dx_ld=8):
    if ws_bytes is None:
        ws_bytes = lib.sv_instance_norm_workspace_bytes(V, B, C)
    return lib.sv_instance_norm_backward(x, V, ld, C, bs, B, w, b, mean, inv, act, dy, dy_ld, ws, ws_bytes, dx, dx_ld, FAKE, FAKE,
                                         None)


def test_instance_norm_checks(lib):
    for kw in ({"x": None}, {"bs": None}, {"w": None}, {"b": None}, {"ws": None}, {"y": None}, {"mean": None}, {"inv": None}):
        assert _norm(lib, **kw) == INVALID and b"null pointer" in lib.sv_last_error(), kw
    for kw in ({"act": 2}, {"act": 4}, {"C": 0}, {"ld": 7}, {"y_ld": 7}, {"B": 0}, {"B": 1025}, {"V": -1}):
        assert _norm(lib, **kw) == INVALID, kw
    for kw in ({"x": None}, {"bs": None}, {"w": None}, {"b": None}, {"ws": None}, {"dy": None}, {"dx": None}, {"mean": None},
               {"inv": None}):
        assert _norm_bwd(lib, **kw) == INVALID and b"null pointer" in lib.sv_last_error(), kw
    for kw in ({"act": 2}, {"C": 0}, {"ld": 7}, {"dy_ld": 7}, {"dx_ld": 7}, {"B": 0}):
        assert _norm_bwd(lib, **kw) == INVALID, kw
    chunk = 256
    need = lib.sv_instance_norm_workspace_bytes(10 * chunk, 3, 64)
    assert need >= 2 * (10 + 3) * 64 * 8 + 2 * 3 * 64 * 8  # two partial arrays of one slot per chunk, two [B][C] sums
    for have in (0, 64, need // 8):
        assert _norm(lib, V=10 * chunk, B=3, C=64, ld=64, y_ld=64, ws_bytes=have) == WORKSPACE
        assert b"workspace too small" in lib.sv_last_error()
        assert _norm_bwd(lib, V=10 * chunk, B=3, C=64, ld=64, dy_ld=64, dx_ld=64, ws_bytes=have) == WORKSPACE
        assert b"workspace too small" in lib.sv_last_error()
