"""numpy mirrors of host-side arithmetic of the post-processing kernels (csrc/sv_common.h topk_key, csrc/sv_post.hip
sv_col_stats' slab split) and the special float32 bit patterns the edge tests plant.  tests/test_post_keys_cpu.py checks
the key mirror against the documented order without a GPU; tests/test_gpu_post_edges.py pins the kernels."""
import numpy as np

FLT_MAX = 0x7f7fffff
SIGN = 0x80000000
# name -> float32 bit pattern
NANS = {"nan": 0x7fc00000, "-nan": 0xffc00000, "nan_payload": 0x7fc00001, "nan_all_ones": 0xffffffff,
        "snan": 0x7f800001, "+nan_all_ones": 0x7fffffff}
NUMBERS = {"+inf": 0x7f800000, "-inf": 0xff800000, "+max": FLT_MAX, "-max": FLT_MAX | SIGN, "+0": 0x00000000,
           "-0": SIGN, "+denorm": 0x00000001, "-denorm": SIGN | 1, "+1": 0x3f800000, "-1": 0xbf800000}
SPECIALS = {**NANS, **NUMBERS}


def f32(bits):
    """float32 array with exactly these uint32 bit patterns (no arithmetic touches them: NaN signs and payloads stay)"""
    return np.asarray(bits, dtype=np.uint32).view(np.float32)


def bits_of(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def topk_key(bits, row):
    """csrc/sv_common.h topk_key on uint32 value bits and row indices -> uint64 keys"""
    u = np.asarray(bits, dtype=np.uint32).copy()
    row = np.asarray(row, dtype=np.uint64)
    u[(u & np.uint32(0x7fffffff)) > np.uint32(0x7f800000)] = np.uint32(0x7fc00000)  # every NaN: the quiet NaN's class
    u[u == np.uint32(SIGN)] = np.uint32(0)  # -0.0: the class of +0.0
    neg = (u & np.uint32(SIGN)) != 0
    u = np.where(neg, ~u, u | np.uint32(SIGN)).astype(np.uint32)
    return (u.astype(np.uint64) << np.uint64(32)) | (np.uint64(0xffffffff) - row)


def contract_before(bits_a, row_a, bits_b, row_b):
    """the documented order of sv_topk_indices (include/sv_hip.h), written from its words: does (value a, row a) come
    before (value b, row b)?  NaN above +inf, then the larger value, equal values (and any two NaNs) by the lower row."""
    a, b = np.float64(f32([bits_a])[0]), np.float64(f32([bits_b])[0])
    if np.isnan(a) != np.isnan(b):
        return bool(np.isnan(a))
    if not np.isnan(a) and a != b:  # -0.0 == +0.0
        return bool(a > b)
    return row_a < row_b


def stats_slabs(N):
    """(slabs, rows per slab) of sv_col_stats' first stage, as csrc/sv_post.hip computes them"""
    blocks = min((N + 4095) // 4096, 1024)
    return blocks, (N + blocks - 1) // blocks


def lattice(n, dtype=np.float32):
    """n points one unit apart on a line: with dist = 0.5 every point is a component of its own"""
    pts = np.zeros((n, 3), dtype)
    pts[:, 0] = np.arange(n)
    return pts


def link(pts, a, b, axis=1, step=0.25):
    """move point b to `step` beside point a (along another axis than the lattice's): the only link of b is a"""
    pts[b] = pts[a]
    pts[b, axis] += step


def non_finite_scene():
    """(float32 points, rows that hold a NaN or an infinity): three small clusters of a unit lattice (dist = 0.5) with
    non-finite rows between their members - a NaN, a +inf, both infinities, the same +inf row twice, an all-NaN row"""
    pts = lattice(40)
    for a, b in ((0, 5), (5, 9), (2, 30), (30, 31), (12, 39)):
        link(pts, a, b, axis=1 + (b % 2))
    bad = {3: (np.nan, 0, 0), 6: (6, np.inf, 0), 7: (np.inf, -np.inf, 0), 10: (np.inf, 1, 2), 11: (np.inf, 1, 2),
           20: (np.nan, np.nan, np.nan), 38: (-np.inf, 0, 0), 1: (1, np.nan, np.inf)}
    for r, v in bad.items():
        pts[r] = v
    return pts, sorted(bad)
