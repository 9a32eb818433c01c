"""Helpers shared by the strided-map, local-pooling, instance-norm and ResNet tests: numpy restatements of the definitions
in include/sv_hip.h (block N8) and thin wrappers that call the library's entries on torch tensors; at the end the map kinds,
compact-blob frames and the case table of the convolution tests on these maps (tests/test_gpu_conv_strided.py)."""
from collections import namedtuple
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


def pool_features(rng, V, C, ties):
    """pooling inputs float32 [V, C].  ties: few distinct values, so every window has ties; NaNs in a few places, one whole
    NaN row, one +inf and one -inf.  Else standard normal."""
    if ties:
        x = rng.integers(-2, 3, size=(V, C)).astype(np.float32)
        x[rng.integers(0, V, size=12), rng.integers(0, C, size=12)] = np.nan
        x[V // 2] = np.nan
        x[3, 0], x[4, 0] = np.inf, -np.inf
    else:
        x = rng.standard_normal((V, C)).astype(np.float32)
    return x


def pool_backward_terms(dy, nbr_t, mode, arg, count):
    """the addends of sv_pool_local_backward per offset of the TRANSPOSED table, float32 [K, V_in, C] (0 where the offset has
    no output row): dy[o] (sum), dy[o] / count[o] rounded to float32 (avg; count = present neighbours of o in the FORWARD
    table), dy[o] where arg[o] is this input row (max)"""
    K, V_in = nbr_t.shape
    rows = np.arange(V_in)[:, None]
    terms = np.zeros((K, V_in, dy.shape[1]), np.float32)
    for k in range(K):
        o = nbr_t[k]
        oc = np.maximum(o, 0)
        g = dy[oc]
        if mode == 0:
            g = np.where(arg[oc] == rows, g, np.float32(0))
        elif mode == 1:
            with np.errstate(divide="ignore", invalid="ignore"):  # masked rows (o = -1) read row 0, whose count may be 0
                g = (g / count[oc].astype(np.float32)[:, None]).astype(np.float32)
        terms[k] = np.where((o >= 0)[:, None], g, np.float32(0))
    return terms


def pool_backward32_ref(dy, nbr_t, mode, arg, count):
    """sv_pool_local_backward in float32 in the defined order: ascending k over the transposed table, starting from 0"""
    terms = pool_backward_terms(dy, nbr_t, mode, arg, count)
    acc = np.zeros(terms.shape[1:], np.float32)
    for k in range(terms.shape[0]):
        acc = (acc + terms[k]).astype(np.float32)
    return acc


def pool_backward_bound(dy, nbr_t, mode, arg, count):
    """|float32 result - float64 result| per element: at most K float32 additions of correctly rounded terms, each addition
    off by at most 2^-24 of a partial sum that never exceeds sum_k |term|: K * 2^-24 * sum_k |term|; the average's terms
    carry one rounded division each, covered by K + 1"""
    terms = np.abs(pool_backward_terms(dy, nbr_t, mode, arg, count).astype(np.float64))
    K = terms.shape[0]
    return (K + (mode == 1)) * 2.0 ** -24 * terms.sum(0)


def gelu64(y):
    import torch

    t = torch.from_numpy(np.ascontiguousarray(y, np.float64))
    return (0.5 * t * (1.0 + torch.erf(t / np.sqrt(2.0)))).numpy()


def act_grad64(y, act):
    """derivative of the activation at the pre-activation y, float64: act 0 none, 1 ReLU (1 where y > 0), 3 exact GELU"""
    import torch

    if act == 1:
        return (y > 0.0).astype(np.float64)
    if act == 3:
        t = torch.from_numpy(np.ascontiguousarray(y, np.float64))
        return (0.5 * (1.0 + torch.erf(t / np.sqrt(2.0))) + t * torch.exp(-0.5 * t * t) / np.sqrt(2.0 * np.pi)).numpy()
    return np.ones_like(y)


def instance_norm_stats_ref(x, starts, eps):
    """(mean, inv_std) float64 [B, C] of instance_norm_ref; both 0 for an empty frame"""
    x = x.astype(np.float64)
    B = len(starts) - 1
    mean, inv_std = np.zeros((B, x.shape[1])), np.zeros((B, x.shape[1]))
    for b in range(B):
        s, e = starts[b], starts[b + 1]
        if e <= s:
            continue
        seg = x[s:e]
        mean[b] = seg.sum(0) / (e - s)
        with np.errstate(invalid="ignore", divide="ignore"):
            inv_std[b] = 1.0 / np.sqrt(((seg - mean[b]) ** 2).sum(0) / (e - s) + eps)
    return mean, inv_std


def instance_norm_backward_ref(x, starts, weight, bias, mean, inv_std, act, dy):
    """sv_instance_norm_backward's formula (include/sv_hip.h) in float64 with its three terms kept apart, from the SAME mean /
    inv_std the kernel is given: dx = inv_std * (g - mean_b(g) - xhat * mean_b(g xhat)), g = dy act'(pre) weight.
    Returns (dx, dweight, dbias, dx_noise, dweight_noise, dbias_noise): *_noise = the sum of the magnitudes of what is added
    up per element, inv_std * (|g| + |mean_b g| + |xhat mean_b(g xhat)|) and sum |dy' xhat|, sum |dy'| - what float64
    summation-order noise scales with.  Rows outside [starts[0], starts[-1]) get 0."""
    x, dy = x.astype(np.float64), dy.astype(np.float64)
    w, bs = weight.astype(np.float64), bias.astype(np.float64)
    dx, noise = np.zeros_like(x), np.zeros_like(x)
    C = x.shape[1]
    dw, db, dw_n, db_n = np.zeros(C), np.zeros(C), np.zeros(C), np.zeros(C)
    with np.errstate(invalid="ignore"):
        for b in range(len(starts) - 1):
            s, e = starts[b], starts[b + 1]
            if e <= s:
                continue
            xh = (x[s:e] - mean[b]) * inv_std[b]
            dyp = dy[s:e] * act_grad64(xh * w + bs, act)
            g = dyp * w
            t2 = g.sum(0) / (e - s)
            t3 = xh * ((g * xh).sum(0) / (e - s))
            dx[s:e] = inv_std[b] * (g - t2 - t3)
            noise[s:e] = np.abs(inv_std[b]) * (np.abs(g) + np.abs(t2) + np.abs(t3))
            dw, db = dw + (dyp * xh).sum(0), db + dyp.sum(0)
            dw_n, db_n = dw_n + np.abs(dyp * xh).sum(0), db_n + np.abs(dyp).sum(0)
    return dx, dw, db, noise, dw_n, db_n


def make_keys_np(coords):
    """make_keys on whole arrays: uint64 [V]"""
    c = np.asarray(coords, np.int64).reshape(-1, 4)
    k = c[:, 0].astype(np.uint64) << np.uint64(54)
    for a in range(3):
        v = (c[:, 1 + a] + BIAS).astype(np.uint64)
        for j in range(BITS):
            k |= ((v >> np.uint64(j)) & np.uint64(1)) << np.uint64(3 * j + a)
    return k


def canonical_np(coords):
    """canonical() on whole arrays, for maps of tens of thousands of voxels"""
    c = np.asarray(coords, np.int32).reshape(-1, 4)
    keys, first = np.unique(make_keys_np(c), return_index=True)
    return c[first], keys.view(np.int64)


def stride_map_ref_np(coords, s_out):
    """stride_map_ref on whole arrays (numpy's // floors towards minus infinity as python's does)"""
    c = np.asarray(coords, np.int64).reshape(-1, 4)
    o = np.concatenate([c[:, :1], c[:, 1:] // s_out * s_out], 1)
    bad = ~(((o[:, 1:] >= LO) & (o[:, 1:] <= HI)).all(1) & (o[:, 0] >= 0) & (o[:, 0] < 1024))
    o[bad] = 0
    out, keys = canonical_np(o)
    parent = np.searchsorted(keys.view(np.uint64), make_keys_np(o)).astype(np.int32)
    parent[bad] = -1
    return out, keys, parent, int(bad.sum())


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


SENTINEL, ARG_SENTINEL = 7.0, -7  # what the guarded buffers below are pre-filled with


def pool_takes_float4(x, out, arg, C):
    """the condition under which sv_pool_local runs its float4 kernel (csrc/sv_pool.hip), restated on the tensors passed"""
    return (C % 4 == 0 and x.stride(0) % 4 == 0 and out.stride(0) % 4 == 0 and x.data_ptr() % 16 == 0 and
            out.data_ptr() % 16 == 0 and (arg is None or arg.data_ptr() % 16 == 0))


def gpu_pool_guarded(x, nbr, mode, V_out=None, pad_cols=0, guard_rows=4):
    """sv_pool_local on the first V_out output rows of a table (default: all; ld stays the table's) into buffers pre-filled
    with a sentinel: out [V_out + guard_rows, C + pad_cols] with out_ld = C + pad_cols, arg [V_out + guard_rows, C], always
    passed (the entry ignores it unless the mode is max).  Asserts that every guard row, every padding column and, unless the
    mode is max, all of arg kept the sentinel.  Returns (out[:V_out, :C], arg[:V_out], float4) as numpy / bool, float4 =
    pool_takes_float4 of what was passed."""
    import torch

    L = _L()
    K = nbr.shape[0]
    V_out = nbr.shape[1] if V_out is None else V_out
    C = x.shape[1]
    out = torch.full((V_out + guard_rows, C + pad_cols), SENTINEL, dtype=torch.float32, device=x.device)
    arg = torch.full((V_out + guard_rows, C), ARG_SENTINEL, dtype=torch.int32, device=x.device)
    L.call("sv_pool_local", L.ptr(x), c_int64(x.shape[0]), c_int64(x.stride(0)), c_int(C), L.ptr(nbr), c_int64(nbr.stride(0)),
           c_int(K), c_int64(V_out), c_int(mode), L.ptr(out), c_int64(C + pad_cols), L.ptr(arg), L.stream_ptr())
    vec = pool_takes_float4(x, out, arg, C)
    out, arg = out.cpu().numpy(), arg.cpu().numpy()
    assert (out[V_out:] == SENTINEL).all() and (out[:, C:] == SENTINEL).all(), "sv_pool_local wrote outside out[:V_out, :C]"
    assert (arg[V_out if mode == 0 else 0:] == ARG_SENTINEL).all(), "sv_pool_local wrote outside arg[:V_out]"
    return out[:V_out, :C], arg[:V_out], vec


def gpu_pool_backward_guarded(dy, nbr_t, mode, arg, mask_fwd, pad_cols=3):
    """sv_pool_local_backward into dx [V_in + 4, C + pad_cols] pre-filled with a sentinel (dx_ld = C + pad_cols); dy may be a
    column view (dy_ld = its row stride).  Asserts that guard rows and padding columns kept the sentinel; dx[:V_in, :C] as
    numpy."""
    import torch

    L = _L()
    K, V_in = nbr_t.shape
    C = dy.shape[1]
    dx = torch.full((V_in + 4, C + pad_cols), SENTINEL, dtype=torch.float32, device=dy.device)
    L.call("sv_pool_local_backward", L.ptr(dy), c_int64(dy.shape[0]), c_int64(dy.stride(0)), c_int(C), L.ptr(nbr_t),
           c_int64(nbr_t.stride(0)), c_int(K), c_int64(V_in), c_int(mode), L.ptr(arg), L.ptr(mask_fwd), L.ptr(dx),
           c_int64(C + pad_cols), L.stream_ptr())
    dx = dx.cpu().numpy()
    assert (dx[V_in:] == SENTINEL).all() and (dx[:, C:] == SENTINEL).all(), "sv_pool_local_backward wrote outside dx[:V_in, :C]"
    return dx[:V_in, :C]


def gpu_instance_norm(x, starts, weight, bias, eps, act, y=None):
    """sv_instance_norm -> (y, mean, inv_std); starts int32 [B + 1] on the device.  x may be a column view (ld = its row
    stride); y: the [V, C] tensor or column view to write into (y_ld = its row stride), default a contiguous one pre-filled
    with a sentinel."""
    import torch

    L = _L()
    V, C = x.shape
    B = starts.shape[0] - 1
    nbytes = L.load().sv_instance_norm_workspace_bytes(c_int64(V), c_int(B), c_int(C))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
    if y is None:
        y = torch.full((max(V, 1), C), SENTINEL, dtype=torch.float32, device=x.device)
    mean = torch.full((B, C), SENTINEL, dtype=torch.float64, device=x.device)
    inv_std = torch.full((B, C), SENTINEL, dtype=torch.float64, device=x.device)
    L.call("sv_instance_norm", L.ptr(x), c_int64(V), c_int64(max(x.stride(0), C)), c_int(C), L.ptr(starts), c_int(B),
           L.ptr(weight), L.ptr(bias), c_double(eps), c_int(act), L.ptr(ws), c_size_t(nbytes), L.ptr(y),
           c_int64(max(y.stride(0), C)), L.ptr(mean), L.ptr(inv_std), L.stream_ptr())
    return y[:V], mean, inv_std


def gpu_instance_norm_backward(x, starts, weight, bias, mean, inv_std, act, dy, dx=None):
    """sv_instance_norm_backward -> (dx, dweight, dbias); x, dy and dx may be column views (ld = their row strides); dx
    defaults to a contiguous [V, C] tensor pre-filled with a sentinel"""
    import torch

    L = _L()
    V, C = x.shape
    B = starts.shape[0] - 1
    nbytes = L.load().sv_instance_norm_workspace_bytes(c_int64(V), c_int(B), c_int(C))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
    if dx is None:
        dx = torch.full((max(V, 1), C), SENTINEL, dtype=torch.float32, device=x.device)
    dw = torch.full((C,), SENTINEL, dtype=torch.float32, device=x.device)
    db = torch.full((C,), SENTINEL, dtype=torch.float32, device=x.device)
    L.call("sv_instance_norm_backward", L.ptr(x), c_int64(V), c_int64(max(x.stride(0), C)), c_int(C), L.ptr(starts), c_int(B),
           L.ptr(weight), L.ptr(bias), L.ptr(mean), L.ptr(inv_std), c_int(act), L.ptr(dy), c_int64(max(dy.stride(0), C)),
           L.ptr(ws), c_size_t(nbytes), L.ptr(dx), c_int64(max(dx.stride(0), C)), L.ptr(dw), L.ptr(db), L.stream_ptr())
    return dx[:V], dw, db


def dense_pool_ref(c_in, x, c_out, ks, st, mode, origin, size, dy=None):
    """Local pooling on a dense float64 grid with torch's own pooling operators - no kernel map: the cloud (canonical rows
    c_in, features x) lies in the cube of `size` cells from `origin` (a multiple of the output stride), an odd kernel is
    centred on the output cell (padding 1), kernel_size 2 starts at it.  max: max_pool3d with -inf at inactive cells;
    sum: avg_pool3d * ks^3; avg: that sum / the same sum of the occupancy mask (include/sv_hip.h: the number of present
    neighbours); an output row without neighbours gives 0.  Read back at the rows c_out.
    Returns a dict: out float64 [V_out, C]; count [V_out]; bound [V_out, C] = (K [+ 1 for avg]) 2^-24 * pooled sum of |x|
    [/ count], what K float32 additions [and one division] can be off; with dy also dx = d sum(out * dy) / dx by autograd and
    dx_terms = d sum(out * |dy|) / dx, the sum of the magnitudes of what is added into every dx element."""
    import torch
    import torch.nn.functional as F

    c_in, c_out = np.asarray(c_in, np.int64), np.asarray(c_out, np.int64)
    B, C, K, pad = int(c_in[:, 0].max()) + 1, x.shape[1], ks ** 3, 1 if ks == 3 else 0
    g = c_in[:, 1:] - np.asarray(origin)
    assert (g >= 0).all() and (g < size).all() and all(o % st == 0 for o in origin)
    at = (torch.from_numpy(c_in[:, 0]), slice(None), *(torch.from_numpy(np.ascontiguousarray(g[:, i])) for i in range(3)))
    go = (c_out[:, 1:] - np.asarray(origin)) // st
    at_out = (torch.from_numpy(c_out[:, 0]), slice(None), *(torch.from_numpy(np.ascontiguousarray(go[:, i])) for i in range(3)))
    leaf = torch.from_numpy(np.asarray(x, np.float64)).requires_grad_(dy is not None)

    def grid(vals, fill, channels=C):
        d = torch.full((B, channels, size, size, size), fill, dtype=torch.float64)
        d[at] = vals
        return d

    def window_sum(d):
        s = F.avg_pool3d(d, ks, st, padding=pad) * K
        assert s.shape[2] == size // st
        return s[at_out]

    count = window_sum(grid(torch.ones(len(c_in), 1, dtype=torch.float64), 0.0, 1))[:, 0].round()
    live = (count > 0)[:, None]
    safe = torch.where(count > 0, count, torch.ones_like(count))[:, None]
    abs_sum = window_sum(grid(leaf.detach().abs(), 0.0))
    if mode == 0:
        out = torch.where(live, F.max_pool3d(grid(leaf, -float("inf")), ks, st, padding=pad)[at_out], torch.zeros(()).double())
        bound = torch.zeros_like(abs_sum)
    elif mode == 1:
        out, bound = window_sum(grid(leaf, 0.0)) / safe, (K + 1) * 2.0 ** -24 * abs_sum / safe
    else:
        out, bound = window_sum(grid(leaf, 0.0)), K * 2.0 ** -24 * abs_sum
    res = {"out": out.detach().numpy(), "count": count.numpy().astype(np.int64), "bound": bound.numpy()}
    if dy is not None:
        dyt = torch.from_numpy(np.asarray(dy, np.float64))
        res["dx"] = torch.autograd.grad((out * dyt).sum(), leaf, retain_graph=True)[0].numpy()
        res["dx_terms"] = torch.autograd.grad((out * dyt.abs()).sum(), leaf)[0].numpy()
    return res


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


# ---- inputs shared by the edge tests and their CPU twin (tests/test_resnet_ops_edges_cpu.py) ---------------------------
# pooling shape -> (kernel_size, stride, dilation): what layer_maps(pooling=True) promises beyond the stem's k2 s2
POOL_SHAPES = {"k3s3": (3, 3, 1), "k1s2": (1, 2, 1), "k3s1": (3, 1, 1), "k3s1d2": (3, 1, 2), "k3s2d2": (3, 2, 2), "k1s1": (1, 1, 1),
               "k3s2": (3, 2, 1)}
_shared = {}


def two_frame_cloud(seed, n, centres, sigma, lo, hi):
    """[2 n, 4] integer voxels: frames 0 and 1 of n blob voxels each"""
    rng = np.random.default_rng(seed)
    return np.concatenate([np.concatenate([np.full((n, 1), b), blob_cloud(rng, n, centres, sigma, (lo,) * 3, (hi,) * 3)], 1)
                           for b in (0, 1)])


def pool_edge_cloud():
    """the cloud of tests/test_gpu_pool_local_edges.py: two frames of 300 voxels, negative coordinates present"""
    return two_frame_cloud(17, 300, [(-5, 2, 0), (6, -3, 4)], 1.4, -20, 20)


def pool_tables_ref(shape):
    """(forward table, transposed table, canonical input rows, canonical output rows) of a pooling shape on pool_edge_cloud,
    from stride_map_ref and probe_ref alone; computed once, read-only"""
    if shape not in _shared:
        ks, st, dil = POOL_SHAPES[shape]
        c_in = canonical(pool_edge_cloud())[0]
        c_out = stride_map_ref(c_in, st)[0] if st > 1 else c_in
        fwd, tr = probe_ref(c_out, c_in, ks, dil), probe_ref(c_in, c_out, ks, -dil)
        for a in (fwd, tr, c_in, c_out):
            a.setflags(write=False)
        _shared[shape] = (fwd, tr, c_in, c_out)
    return _shared[shape]


DENSE_ORIGIN, DENSE_SIZE = (-24, -24, -24), 48
DENSE_POOLS = ((3, 1), (3, 2), (3, 3), (2, 2))  # (kernel_size, stride) of the module tests against the dense grid


def dense_pool_cloud():
    """two frames of 260 voxels in the 48^3 box from DENSE_ORIGIN, a multiple of 6 (so of every stride used)"""
    return two_frame_cloud(23, 260, [(-7, 3, -2), (8, -6, 5)], 3.5, -24, 24)


def k2_table_ref(c_out, c_in):
    """the kernel_size 2 stride 2 map as a dict lookup: nbr[k][o] = row of c_out[o] + (k & 1, k >> 1 & 1, k >> 2), x fastest"""
    row_of = {tuple(r): i for i, r in enumerate(c_in.tolist())}
    nbr = np.full((8, len(c_out)), -1, np.int32)
    for o, (b, x, y, z) in enumerate(c_out.tolist()):
        for k in range(8):
            nbr[k, o] = row_of.get((b, x + (k & 1), y + (k >> 1 & 1), z + (k >> 2)), -1)
    return nbr


CANCEL_BASES = (4096.0, -65536.0, 1e6)
CANCEL_SIZES = (257, 773)


def ulp32(v):
    return float(np.spacing(np.float32(abs(v))))


def cancellation_case(C=7, seed=5):
    """(x float32 [V, C], starts, k int [V, C], base [B, C]): per (frame, channel) a base of CANCEL_BASES plus k ulp32(base),
    k in {0, 1, 2, 3}.  Every value is a float32 and every partial sum of the values and of k is exact in float64, so the mean
    has the same bits in any summation order, while the variance (about ulp32^2) is 2^-46 of the mean square: a one-pass
    E[x^2] - mean^2 loses it."""
    rng = np.random.default_rng(seed)
    starts = np.concatenate([[0], np.cumsum(CANCEL_SIZES)]).astype(np.int32)
    k = rng.integers(0, 4, size=(int(starts[-1]), C))
    base = np.array(CANCEL_BASES)[(np.arange(len(CANCEL_SIZES))[:, None] + np.arange(C)[None]) % len(CANCEL_BASES)]
    x = np.zeros(k.shape, np.float64)
    for b in range(len(CANCEL_SIZES)):
        s, e = starts[b], starts[b + 1]
        x[s:e] = base[b] + k[s:e] * np.array([ulp32(v) for v in base[b]])
    assert np.array_equal(x.astype(np.float32).astype(np.float64), x)
    return x.astype(np.float32), starts, k, base


def cancellation_exact(k, starts, base, weight, bias, eps):
    """the instance norm of cancellation_case from the small integers k alone (x - mean = (k - mean_k) ulp32, exactly), float64"""
    y = np.zeros(k.shape, np.float64)
    for b in range(len(starts) - 1):
        s, e = starts[b], starts[b + 1]
        u = np.array([ulp32(v) for v in base[b]])
        d = (k[s:e] - k[s:e].sum(0) / (e - s)) * u
        y[s:e] = d / np.sqrt((d * d).sum(0) / (e - s) + eps) * weight.astype(np.float64) + bias.astype(np.float64)
    return y


def norm_forward_bound(want):
    """|float32 result - float64 reference| of sv_instance_norm: one float32 rounding plus float64 summation-order noise"""
    return 2.0 ** -23 * np.abs(want) + 1e-12


def collapse_voxels(batch, n=9000, s_out=192, seed=3):
    """n distinct voxels of one batch index inside ONE cell of the stride-s_out lattice, the cell [-s_out, 0)^3"""
    rng = np.random.default_rng(seed)
    cells = rng.choice(s_out ** 3, size=n, replace=False)
    xyz = np.stack([cells % s_out, cells // s_out % s_out, cells // (s_out * s_out)], 1) - s_out
    return np.concatenate([np.full((n, 1), batch), xyz], 1)


def spread_voxels(batch, n=9000, s_out=3, seed=4):
    """n voxels of one batch index, each in a cell of its own of the stride-s_out lattice (cells drawn without replacement from
    24^3 around the origin, a random position inside each cell)"""
    rng = np.random.default_rng(seed)
    cells = rng.choice(24 ** 3, size=n, replace=False)
    xyz = (np.stack([cells % 24, cells // 24 % 24, cells // 576], 1) - 12) * s_out + rng.integers(0, s_out, size=(n, 3))
    return np.concatenate([np.full((n, 1), batch), xyz], 1)


# ---- the strided / dilated kernel-map kinds of the convolution tests ----------------------------------------------------
# (tests/test_conv_strided_cpu.py, tests/test_gpu_conv_strided.py, tests/test_gpu_conv_exact.py)
# kind -> (kernel_size, stride, dilation, transposed), all from tensor stride 1; "k3d2" is the dilated stride-1 3x3x3 map
MAP_KINDS = {"k3s2": (3, 2, 1, False), "k3s3": (3, 3, 1, False), "k1s2": (1, 2, 1, False), "k3s2d2": (3, 2, 2, False),
             "k3s2_t": (3, 2, 1, True), "k3s3_t": (3, 3, 1, True), "k1s2_t": (1, 2, 1, True), "k3s2d2_t": (3, 2, 2, True),
             "k3d2": (3, 1, 2, False)}
EMPTY_TILE_KINDS = ("k1s2_t", "k3s2d2_t")  # about 7 of 8 output rows have no neighbour at all


def compact_blob(V, batch=0, origin=(0, 0, 0)):
    """V integer voxels [V, 4] of a compact block (x fastest) centred on `origin`: V is exact and 3x3x3 neighbours exist"""
    if V == 0:
        return np.zeros((0, 4), np.int64)
    s = int(np.ceil(V ** (1.0 / 3.0)))
    while s ** 3 < V:
        s += 1
    i = np.arange(V, dtype=np.int64)
    c = np.stack([np.full(V, batch, np.int64), i % s, (i // s) % s, i // (s * s)], axis=1)
    c[:, 1:] += np.asarray(origin, np.int64) - s // 2
    return c


# frame name -> [(voxels, origin)] per batch index; every fine map has V % 128 == 67 (707; 835 + 640 = 1475; 24003, the
# size of the existing dual-body row); the second frame of "two" lies wholly at negative coordinates of mixed parity
FRAMES = {"one": [(707, (0, 0, 0))], "two": [(835, (1, 0, 0)), (640, (-37, -20, -9))], "big": [(24003, (0, 0, 0))],
          # four batch indices, one of them empty: the batch-range tests (ConvPlan.chunks)
          "batch": [(419, (0, 0, 0)), (0, (0, 0, 0)), (707, (-21, 3, -8)), (349, (5, -30, 2))]}
_coords, _tables = {}, {}


def frame_input(name):
    """the integer coordinates [N, 4] a frame's coordinate manager is built from"""
    return np.concatenate([compact_blob(V, b, o) for b, (V, o) in enumerate(FRAMES[name])])


def frame_coords(name):
    """canonical stride-1 coordinates of a frame (the device's row order), computed once"""
    if name not in _coords:
        _coords[name] = canonical(frame_input(name))[0]
    return _coords[name]


def batch_bounds_ref(coords, B):
    """first row of every batch index of canonical coordinates (rows ascend by batch first), [B + 1]"""
    return [int(np.searchsorted(coords[:, 0], b)) for b in range(B + 1)]


def kind_table_of(c1, kind):
    """(nbr int32[K][V_out], V_in, V_out) of a map kind on canonical stride-1 coordinates, from probe_ref alone: a forward
    kind's output rows probe the input map at +dilation, a transposed kind's rows (the input map) probe the output map at
    -dilation"""
    ks, st, dil, transposed = MAP_KINDS[kind]
    if st == 1:
        return probe_ref(c1, c1, ks, dil), len(c1), len(c1)
    cs = stride_map_ref(c1, st)[0]
    if transposed:
        return probe_ref(c1, cs, ks, -dil), len(cs), len(c1)
    return probe_ref(cs, c1, ks, dil), len(c1), len(cs)


def kind_table(name, kind):
    """kind_table_of on a named frame, computed once and never changed"""
    if (name, kind) not in _tables:
        nbr, V_in, V_out = kind_table_of(frame_coords(name), kind)
        nbr.setflags(write=False)
        _tables[(name, kind)] = (nbr, V_in, V_out)
    return _tables[(name, kind)]


def kind_plan(cm, kind):
    """the library's plan of a map kind on a coordinate manager (tensor stride 1)"""
    ks, st, dil, transposed = MAP_KINDS[kind]
    if st == 1:
        return cm.plan_k3(1, dil)
    return cm.plan_strided_t(1, ks, st, dil) if transposed else cm.plan_strided(1, ks, st, dil)


def plan_tile_census(plan):
    """(all_empty bool[tiles], mixed bool[tiles]) of a plan's 128-row tiles: all_empty = every row is a real output row
    (perm >= 0) and every submask word is zero; mixed = among the tile's 16-row sub-tiles that hold only real rows some have a
    neighbour at some offset and some have none"""
    perm = plan.perm.cpu().numpy().reshape(-1, 128)
    sub = plan.submask.cpu().numpy().reshape(perm.shape[0], plan.K).astype(np.int64) & 0xFF
    live = np.bitwise_or.reduce(sub, axis=1)                      # bit s: sub-tile s has a pair at some offset
    real = (perm.reshape(-1, 8, 16) >= 0).all(2)                  # [tiles, 8]: the sub-tile holds only real rows
    bits = (live[:, None] >> np.arange(8)[None]) & 1
    all_empty = (perm >= 0).all(1) & (sub == 0).all(1)
    mixed = ((bits == 1) & real).any(1) & ((bits == 0) & real).any(1)
    return all_empty, mixed


# ---- the table of tests/test_gpu_conv_strided.py (a): fp32 forward on the strided maps, bit-exact against the oracle ----
# frame, kind: the map; scale: None = the library's default dispatch, 1.0 = under conv_dispatch(1.0); mis: `perm` 4 bytes off
# a 16-byte boundary; name, fast, ring, full: what sv_conv_last_instance() must report, as literals
# (tests/test_conv_strided_cpu.py holds them to the library's own host-side answer)
StridedCase = namedtuple("StridedCase", "frame kind Cin Cout scale mis name fast ring full")

FIRST_MFMA, FIRST_VALU = "conv_first_mfma_kernel<3, 32>", "conv_first_layer_kernel<3, 32>"
THIN, THIN_LDS = "conv_thin_kernel<32, 32>", "conv_thin_lds_kernel<32, 32>"
DUAL = "conv_fwd_dual_kernel<64, 32, 4, 3>"
T16_64, T16_192 = "conv_fwd_kernel<16, 4, 1>", "conv_fwd_kernel<16, 4, 3>"
F32, F64 = "conv_fwd_kernel<16, 4, 1, fused 32>", "conv_fwd_kernel<16, 4, 1, fused 64>"
T64_16 = "conv_fwd_kernel<64, 1, 1>"

STRIDED_CASES = tuple(StridedCase(*r) for r in (
    # the 3 -> 32 first layer on the matrix pipe and, with a misaligned `perm`, on the vector ALU (K = 27 only)
    ("one", "k3s2", 3, 32, None, False, FIRST_MFMA, 1, 0, 1),
    ("one", "k3s2d2_t", 3, 32, None, False, FIRST_MFMA, 1, 0, 1),
    ("one", "k3s2", 3, 32, None, True, FIRST_VALU, 0, 0, 0),
    ("one", "k3s2d2_t", 3, 32, None, True, FIRST_VALU, 0, 0, 0),
    # the thin 32 -> 32 layer, and its LDS-weights kernel when the frame is alone on the GPU
    ("one", "k3s3", 32, 32, None, False, THIN, 1, 0, 1),
    ("one", "k3s2d2_t", 32, 32, None, False, THIN, 1, 0, 1),
    ("one", "k3s2", 32, 32, 1.0, False, THIN_LDS, 1, 0, 1),
    ("one", "k3s2d2_t", 32, 32, 1.0, False, THIN_LDS, 1, 0, 1),
    # the fused-offset tiles, FAST and guarded
    ("one", "k3s2", 32, 64, None, False, F32, 1, 1, 0),
    ("two", "k3s2d2_t", 32, 64, None, False, F32, 1, 1, 0),
    ("one", "k3s2d2_t", 32, 64, None, True, F32, 0, 1, 0),
    ("one", "k3d2", 64, 64, None, False, F64, 1, 1, 0),
    ("one", "k3s2d2_t", 64, 64, None, False, F64, 1, 1, 0),
    ("two", "k3s2_t", 64, 64, None, False, F64, 1, 1, 0),
    ("one", "k3s3_t", 64, 64, None, True, F64, 0, 1, 0),
    ("one", "k3s2d2", 64, 128, None, False, F64, 1, 1, 0),
    ("one", "k3s2d2_t", 64, 128, None, False, F64, 1, 1, 0),
    ("two", "k3s2d2_t", 64, 128, 1.0, True, F64, 0, 1, 0),
    # the same widths at K = 1 WITH a plan: the plain lists, not the fused ones
    ("one", "k1s2", 32, 64, None, False, T16_64, 1, 1, 0),
    ("one", "k1s2_t", 32, 64, None, False, T16_64, 1, 1, 0),
    ("one", "k1s2", 64, 64, None, False, T16_64, 1, 1, 0),
    ("two", "k1s2_t", 64, 64, None, False, T16_64, 1, 1, 0),
    ("one", "k1s2", 64, 128, None, False, T16_64, 1, 1, 0),
    ("one", "k1s2_t", 64, 128, None, False, T16_64, 1, 1, 0),
    ("one", "k1s2_t", 64, 128, None, True, T16_64, 0, 1, 0),
    # the ResNet stem 3 -> 64 (odd Cin: guarded) and other guarded widths (odd Cin at K = 1, a partial column tile)
    ("one", "k3s2", 3, 64, None, False, T16_64, 0, 1, 0),
    ("one", "k3s2d2_t", 3, 64, None, False, T16_64, 0, 1, 0),
    ("two", "k1s2_t", 131, 48, None, False, T16_64, 0, 1, 0),
    ("one", "k3s2d2_t", 148, 80, None, False, "conv_fwd_kernel<32, 2, 2>", 0, 1, 0),
    # a 64-column tile in FULL form
    ("one", "k1s2", 256, 64, None, False, T16_64, 1, 1, 1),
    ("one", "k1s2_t", 256, 64, None, False, T16_64, 1, 1, 1),
    # the Bottleneck downsample 64 -> 256 k1 s2: on maps this small the 128-column list ends on its 64-column tile; the same
    # layer's input gradient map at 24003 rows reaches a 128-column tile
    ("one", "k1s2", 64, 256, None, False, T16_64, 1, 1, 0),
    ("two", "k1s2_t", 64, 256, None, False, T16_64, 1, 1, 0),
    ("big", "k1s2_t", 64, 256, None, False, "conv_fwd_kernel<64, 4, 2>", 1, 0, 0),
    ("one", "k3s3", 512, 512, None, False, T16_64, 1, 1, 1),
    ("one", "k3s2d2_t", 512, 512, None, False, T16_64, 1, 1, 1),
    # a 192-column tile in FULL form
    ("two", "k3s2", 256, 384, None, False, T16_192, 1, 1, 1),
    ("one", "k1s2_t", 256, 384, None, False, T16_192, 1, 1, 1),
    # the dual-body launch: its 32-row tail body runs the cheapest plan tiles, which on this map are the empty ones
    ("big", "k1s2_t", 148, 384, None, False, DUAL, 1, 0, 0),
    # K = 1 with a plan and at most four outputs: NOT the narrow (dense-row) kernel
    ("one", "k1s2", 148, 1, None, False, T64_16, 0, 1, 0),
    ("one", "k1s2_t", 148, 1, None, False, T64_16, 0, 1, 0),
    ("one", "k1s2", 148, 3, None, False, T64_16, 0, 1, 0),
    ("one", "k1s2_t", 148, 3, None, False, T64_16, 0, 1, 0),
    ("one", "k1s2", 148, 4, None, False, T64_16, 0, 1, 0),
    ("one", "k1s2_t", 148, 4, None, False, T64_16, 0, 1, 0),
))


def strided_case_id(c):
    tile = c.name.replace("conv_", "").replace("_kernel", "").replace(" ", "")
    return (f"{tile}-f{c.fast}r{c.ring}u{c.full}-{c.frame}-{c.kind}-{c.Cin}x{c.Cout}" + ("-alone" if c.scale else "") +
            ("-perm_misaligned" if c.mis else ""))


# (b) the special kernels at row edges on the k3s2d2_t map of a V-voxel blob centred on (1, 1, 1), so that the only voxel of
# V = 1 has odd coordinates and no neighbour at all: (name, (fast, ring, full), Cin, Cout, scale, perm misaligned)
EDGE_V = (1, 15, 16, 17, 127, 128, 129)
EDGE_SPECIAL = ((THIN, (1, 0, 1), 32, 32, None, False), (THIN_LDS, (1, 0, 1), 32, 32, 1.0, False),
                (FIRST_MFMA, (1, 0, 1), 3, 32, None, False), (FIRST_VALU, (0, 0, 0), 3, 32, None, True))
