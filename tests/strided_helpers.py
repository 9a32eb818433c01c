"""Helpers shared by the strided-map, local-pooling, instance-norm and ResNet tests: numpy restatements of the definitions
in include/sv_hip.h (block N8) and thin wrappers that call the library's entries on torch tensors."""
from ctypes import c_double, c_int, c_int64, c_size_t

import numpy as np

BIAS, BITS, LO, HI = 1 << 17, 18, -(1 << 17), (1 << 17) - 1
EMPTY_KEY = (1 << 64) - 1


# ---- numpy restatements -------------------------------------------------------------------------------------------------
def make_keys(coords):
    """key = batch << 54 | morton3(x + 2^17, y + 2^17, z + 2^17), x in bit 3j (include/sv_hip.h); python ints in an object
    array so that all 64 bits compare unsigned"""
    out = []
    for b, x, y, z in np.asarray(coords, np.int64).tolist():
        k = b << 54
        for j in range(BITS):
            k |= (((x + BIAS) >> j) & 1) << (3 * j) | (((y + BIAS) >> j) & 1) << (3 * j + 1) | (((z + BIAS) >> j) & 1) << (3 * j + 2)
        out.append(k)
    return out


def canonical(coords):
    """distinct voxels int32[V, 4] in canonical (ascending key) order, and their keys as int64 (the uint64 bit patterns)"""
    coords = np.unique(np.asarray(coords, np.int32).reshape(-1, 4), axis=0)
    keys = make_keys(coords)
    order = sorted(range(len(keys)), key=keys.__getitem__)
    keys = np.array([keys[i] for i in order], dtype=np.uint64).view(np.int64) if order else np.zeros(0, np.int64)
    return coords[order], keys


def in_range(b, x, y, z):
    return 0 <= b < 1024 and all(LO <= v <= HI for v in (x, y, z))


def stride_map_ref(coords, s_out):
    """(vcoords_out, keys_out, parent, bad) of sv_stride_map_general for a canonical input map: python's // floors towards
    minus infinity; a voxel whose floored coordinate leaves the key range is counted, keyed as (0,0,0,0) and gets parent -1"""
    rows, bad = [], []
    for b, x, y, z in coords.tolist():
        o = (b, x // s_out * s_out, y // s_out * s_out, z // s_out * s_out)
        ok = in_range(*o)
        bad.append(not ok)
        rows.append(o if ok else (0, 0, 0, 0))
    out, keys = canonical(rows) if rows else (np.zeros((0, 4), np.int32), np.zeros(0, np.int64))
    row_of = {tuple(r): i for i, r in enumerate(out.tolist())}
    parent = np.array([-1 if bd else row_of[r] for r, bd in zip(rows, bad)], np.int32).reshape(-1)
    return out, keys, parent, int(sum(bad))


def offsets(ks):
    return [(k % 3 - 1, (k // 3) % 3 - 1, k // 9 - 1) for k in range(27)] if ks == 3 else [(0, 0, 0)]


def probe_ref(coords_q, coords_t, ks, step):
    """nbr[k][o] = row in coords_t of coords_q[o] + d_k * step (dict lookup), -1 when absent or outside the key range"""
    row_of = {tuple(r): i for i, r in enumerate(coords_t.tolist())}
    offs = offsets(ks)
    nbr = np.full((len(offs), len(coords_q)), -1, np.int32)
    for o, (b, x, y, z) in enumerate(coords_q.tolist()):
        for k, (dx, dy, dz) in enumerate(offs):
            c = (b, x + dx * step, y + dy * step, z + dz * step)
            if in_range(*c):
                nbr[k, o] = row_of.get(c, -1)
    return nbr


def mask_of(nbr):
    return ((nbr >= 0).astype(np.int64) << np.arange(nbr.shape[0])[:, None]).sum(0).astype(np.uint32).view(np.int32)


def pool_ref(x, nbr, mode):
    """sv_pool_local in float32, ascending k: mode 0 max (first NaN wins and stays, ties to the lowest k; arg = input row),
    1 average over the present neighbours, 2 sum.  A row without neighbours: 0 and arg -1."""
    K, V = nbr.shape
    C = x.shape[1]
    out = np.zeros((V, C), np.float32)
    arg = np.full((V, C), -1, np.int32)
    for o in range(V):
        rows = [int(i) for i in nbr[:, o] if i >= 0]
        if not rows:
            continue
        if mode == 0:
            best, who = x[rows[0]].copy(), np.full(C, rows[0], np.int32)
            for i in rows[1:]:
                v = x[i]
                take = (v > best) | (np.isnan(v) & ~np.isnan(best))
                best[take], who[take] = v[take], i
            out[o], arg[o] = best, who
        else:
            acc = np.zeros(C, np.float32)
            for i in rows:
                acc = (acc + x[i]).astype(np.float32)
            out[o] = acc / np.float32(len(rows)) if mode == 1 else acc
    return out, arg


def pool_backward_ref(dy, nbr, mode, arg, V_in):
    """float64 input gradient of pool_ref from the FORWARD table"""
    K, V = nbr.shape
    dx = np.zeros((V_in, dy.shape[1]), np.float64)
    for o in range(V):
        rows = [int(i) for i in nbr[:, o] if i >= 0]
        for i in rows:
            if mode == 0:
                dx[i] += np.where(arg[o] == i, dy[o].astype(np.float64), 0.0)
            elif mode == 1:
                dx[i] += dy[o].astype(np.float64) / len(rows)
            else:
                dx[i] += dy[o].astype(np.float64)
    return dx


def gelu64(y):
    import torch

    t = torch.from_numpy(np.ascontiguousarray(y, np.float64))
    return (0.5 * t * (1.0 + torch.erf(t / np.sqrt(2.0)))).numpy()


def instance_norm_ref(x, starts, weight, bias, eps, act):
    """float64 instance norm per (frame, channel), biased variance from the second pass; act 0 none, 1 ReLU, 3 exact GELU"""
    x = x.astype(np.float64)
    y = np.zeros_like(x)
    for b in range(len(starts) - 1):
        s, e = starts[b], starts[b + 1]
        if e <= s:
            continue
        seg = x[s:e]
        mean = seg.sum(0) / (e - s)
        var = ((seg - mean) ** 2).sum(0) / (e - s)
        y[s:e] = (seg - mean) / np.sqrt(var + eps) * weight.astype(np.float64) + bias.astype(np.float64)
    if act == 1:
        y = np.maximum(y, 0.0)
    elif act == 3:
        y = gelu64(y)
    return y


# ---- library calls on torch tensors ----------------------------------------------------------------------------------
def _L():
    import mrcc_amd

    return mrcc_amd._lib


def gpu_stride_map_general(keys, s_in, s_out, dev):
    """sv_stride_map_general on int64 keys (numpy) -> (keys_out, vcoords_out, parent, counters) as numpy"""
    import torch

    L = _L()
    V = len(keys)
    k = torch.from_numpy(np.ascontiguousarray(keys)).to(dev)
    nbytes = L.load().sv_stride_map_general_workspace_bytes(c_int64(V))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    n1 = max(V, 1)
    ko = torch.full((n1,), -7, dtype=torch.int64, device=dev)
    vo = torch.full((n1, 4), -7, dtype=torch.int32, device=dev)
    parent = torch.full((n1,), -7, dtype=torch.int32, device=dev)
    counters = torch.full((4,), -7, dtype=torch.int32, device=dev)
    L.call("sv_stride_map_general", L.ptr(k), c_int64(V), c_int(s_in), c_int(s_out), L.ptr(ws), c_size_t(nbytes), L.ptr(ko),
           L.ptr(vo), L.ptr(parent), L.ptr(counters), L.stream_ptr())
    cnt = counters.cpu().numpy()
    Vo = int(cnt[0])
    return ko[:Vo].cpu().numpy(), vo[:Vo].cpu().numpy(), parent[:V].cpu().numpy(), cnt


def gpu_probe(coords_q, coords_t, keys_t, ks, step, dev, pad=3):
    """sv_hash_build on the table map + sv_kernel_map_probe -> (nbr int32[K][V_q], mask int32[V_q]) as numpy; the table is
    allocated with ld = V_q + pad and the padding must stay untouched"""
    import torch

    L = _L()
    Vq, Vt = len(coords_q), len(coords_t)
    cap = 2
    while cap < 2 * Vt:
        cap *= 2
    kt = torch.from_numpy(np.ascontiguousarray(keys_t)).to(dev)
    tk = torch.empty(cap, dtype=torch.int64, device=dev)
    tv = torch.empty(cap, dtype=torch.int32, device=dev)
    L.call("sv_hash_build", L.ptr(kt), c_int64(Vt), L.ptr(tk), L.ptr(tv), c_int64(cap), L.stream_ptr())
    q = torch.from_numpy(np.ascontiguousarray(coords_q, np.int32)).to(dev)
    t = torch.from_numpy(np.ascontiguousarray(coords_t, np.int32)).to(dev)
    K, ld = ks ** 3, Vq + pad
    nbr = torch.full((K, ld), -9, dtype=torch.int32, device=dev)
    mask = torch.full((ld,), -9, dtype=torch.int32, device=dev)
    L.call("sv_kernel_map_probe", L.ptr(q), c_int64(Vq), c_int(ks), c_int(step), L.ptr(t), c_int64(Vt), L.ptr(tk), L.ptr(tv),
           c_int64(cap), L.ptr(nbr), c_int64(ld), L.ptr(mask), L.stream_ptr())
    nbr, mask = nbr.cpu().numpy(), mask.cpu().numpy()
    assert (nbr[:, Vq:] == -9).all() and (mask[Vq:] == -9).all(), "the probe wrote past V_q"
    return nbr[:, :Vq], mask[:Vq]


def gpu_pool(x, nbr, mode):
    """sv_pool_local on torch tensors (x float32 [V_in, C], nbr int32 [K, V_out]) -> (out, arg or None)"""
    import torch

    L = _L()
    K, V_out = nbr.shape
    C = x.shape[1]
    out = torch.full((V_out, C), 7.0, dtype=torch.float32, device=x.device)
    arg = torch.full((V_out, C), -7, dtype=torch.int32, device=x.device) if mode == 0 else None
    L.call("sv_pool_local", L.ptr(x), c_int64(x.shape[0]), c_int64(x.stride(0)), c_int(C), L.ptr(nbr), c_int64(nbr.stride(0)),
           c_int(K), c_int64(V_out), c_int(mode), L.ptr(out), c_int64(C), L.ptr(arg), L.stream_ptr())
    return out, arg


def gpu_pool_backward(dy, nbr_t, mode, arg, mask_fwd):
    import torch

    L = _L()
    K, V_in = nbr_t.shape
    C = dy.shape[1]
    dx = torch.full((V_in, C), 7.0, dtype=torch.float32, device=dy.device)
    L.call("sv_pool_local_backward", L.ptr(dy), c_int64(dy.shape[0]), c_int64(dy.stride(0)), c_int(C), L.ptr(nbr_t),
           c_int64(nbr_t.stride(0)), c_int(K), c_int64(V_in), c_int(mode), L.ptr(arg), L.ptr(mask_fwd), L.ptr(dx), c_int64(C),
           L.stream_ptr())
    return dx


def gpu_instance_norm(x, starts, weight, bias, eps, act):
    """sv_instance_norm -> (y, mean, inv_std); starts int32 [B + 1] on the device"""
    import torch

    L = _L()
    V, C = x.shape
    B = starts.shape[0] - 1
    nbytes = L.load().sv_instance_norm_workspace_bytes(c_int64(V), c_int(B), c_int(C))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
    y = torch.full((max(V, 1), C), 7.0, dtype=torch.float32, device=x.device)
    mean = torch.empty((B, C), dtype=torch.float64, device=x.device)
    inv_std = torch.empty((B, C), dtype=torch.float64, device=x.device)
    L.call("sv_instance_norm", L.ptr(x), c_int64(V), c_int64(max(x.stride(0), C)), c_int(C), L.ptr(starts), c_int(B),
           L.ptr(weight), L.ptr(bias), c_double(eps), c_int(act), L.ptr(ws), c_size_t(nbytes), L.ptr(y), c_int64(C),
           L.ptr(mean), L.ptr(inv_std), L.stream_ptr())
    return y[:V], mean, inv_std


def blob_cloud(rng, n, centres, sigma, lo, hi):
    """n distinct integer voxels drawn from gaussian blobs around `centres`, clipped to the box [lo, hi) per axis"""
    lo, hi = np.asarray(lo), np.asarray(hi)
    pts = np.zeros((0, 3), np.int64)
    while len(pts) < n:
        c = np.asarray(centres)[rng.integers(0, len(centres), size=2 * n)]
        p = np.floor(c + rng.normal(0.0, sigma, size=(2 * n, 3))).astype(np.int64)
        p = p[np.all((p >= lo) & (p < hi), axis=1)]
        pts = np.unique(np.concatenate([pts, p]), axis=0)
    return pts[rng.permutation(len(pts))[:n]]
