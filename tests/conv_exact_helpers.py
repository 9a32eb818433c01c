"""Exact integer references of the sparse convolution and its gradients (tests/test_conv_exact_cpu.py,
tests/test_gpu_conv_exact.py).

With small-integer operands every product is exact in fp32 (the operands are bf16-exact, |v| <= 256, and the products
stay below 2^24), and so is every partial sum in ANY summation order and in any matrix-core internal format, as long as
the sum of the absolute terms of an element stays below 2^24 (assert_exact_range).  A kernel must then return exactly
the integer result on every element: no tolerance, no sampling.

The references are int64 gather / index_add over the RAW kernel map (plan.raw[0], the unsorted neighbour table
nbr[k][o] = input row or -1), so they share no plan, no tiling and no arithmetic with the kernels.  The per-offset
product of two integer matrices runs as a float64 matmul rounded back to int64: every partial sum is an integer below
2^53, so it is exact (tests/test_conv_exact_cpu.py holds it to a plain int64 einsum)."""
import numpy as np
import torch

EXACT_LIMIT = 1 << 24          # integers below it are exact in fp32
OPERAND_LIMIT = 256            # integers up to it are exact in bf16 (8 significant bits)
SCALES = (-2.0, -1.0, -0.5, 0.5, 1.0, 2.0, 4.0)  # BN scales whose products with an integer are exact
LEAKY_SLOPE = 0.25


# ---------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------
def int_cloud(seed, n, span=24):
    """integer voxel coordinates [V, 3]: a spherical shell plus a slab (surfaces, as a depth camera sees them)"""
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(n, 3))
    shell = d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(span * 0.6, span * 0.7, size=(n, 1))
    slab = np.concatenate([rng.uniform(-span, span, size=(n // 2, 2)), rng.uniform(-2, 1, size=(n // 2, 1))], axis=1)
    c = np.unique(np.floor(np.concatenate([shell, slab])).astype(np.int64), axis=0)
    return c[rng.permutation(len(c))]


def scatter_cloud(seed, n, span=20):
    """mostly isolated voxels: uniform in a cube of side 2 span.  At span 20 and n ~ 1200 about six voxels in ten have no
    neighbour at all, so most 16-row sub-tiles (and whole 128-row tiles of an offset-range pass without the centre
    offset) hold no pair, while the rest still has a few"""
    rng = np.random.default_rng(seed)
    c = np.unique(rng.integers(-span, span, size=(n, 3)), axis=0)
    return c[rng.permutation(len(c))]


def int_tensor(shape, lo, hi, seed, zero_rows=0.0):
    """float32 tensor of integers in [lo, hi]; zero_rows: the share of whole rows (first dimension) set to zero"""
    g = torch.Generator().manual_seed(seed)
    t = torch.randint(lo, hi + 1, tuple(shape), generator=g).float()
    if zero_rows > 0.0:
        t[torch.rand(shape[0], generator=g) < zero_rows] = 0.0
    return t


def scale_tensor(n, seed):
    """per-channel scales drawn from SCALES"""
    g = torch.Generator().manual_seed(seed)
    return torch.tensor(SCALES)[torch.randint(0, len(SCALES), (n,), generator=g)]


# ---------------------------------------------------------------------------------------------------------------------
# int64 references
# ---------------------------------------------------------------------------------------------------------------------
def _int(t):
    """float tensor holding integers -> int64 (refuses anything else)"""
    if t.dtype == torch.int64:
        return t
    assert bool((t == t.round()).all()), "the exact references take integer-valued operands"
    return t.to(torch.int64)


def _imatmul(a, b):
    """a @ b of int64 matrices through float64 (exact: every partial sum is an integer far below 2^53)"""
    return (a.double() @ b.double()).round().to(torch.int64)


def _pairs(nbr, k, V_out):
    """(output rows o, input rows nbr[k][o]) of the pairs at offset k"""
    idx = nbr[k, :V_out].long()
    o = torch.nonzero(idx >= 0).flatten()
    return o, idx[o]


def dense_nbr(V, device="cpu"):
    """the neighbour table of dense rows (kernel_size 1 / Linear): one offset, row o reads row o"""
    return torch.arange(V, dtype=torch.int32, device=device)[None]


def ref_forward(x, W, nbr, V_out, acc0=None):
    """out[o] = acc0[o] + sum_k x[nbr[k][o]] @ W[k]: int64 [V_out, Cout]"""
    xi, Wi = _int(x), _int(W)
    out = torch.zeros((V_out, W.shape[2]), dtype=torch.int64, device=x.device) if acc0 is None else _int(acc0).clone()
    for k in range(W.shape[0]):
        o, i = _pairs(nbr, k, V_out)
        out.index_add_(0, o, _imatmul(xi[i], Wi[k]))
    return out


def ref_wgrad(x, dy, nbr, V_out):
    """dW[k][c][n] = sum over the pairs (i, o) at offset k of x[i][c] * dy[o][n]: int64 [K, Cin, Cout]"""
    xi, di = _int(x), _int(dy)
    K = nbr.shape[0]
    dW = torch.zeros((K, x.shape[1], dy.shape[1]), dtype=torch.int64, device=x.device)
    for k in range(K):
        o, i = _pairs(nbr, k, V_out)
        dW[k] = _imatmul(xi[i].t(), di[o])
    return dW


def ref_dgrad(dy, W, nbr, V_in, V_out):
    """dX[i] = sum over the pairs (i, o) at offset k of dy[o] @ W[k]^T: int64 [V_in, Cin]"""
    di, Wi = _int(dy), _int(W)
    dX = torch.zeros((V_in, W.shape[1]), dtype=torch.int64, device=dy.device)
    for k in range(W.shape[0]):
        o, i = _pairs(nbr, k, V_out)
        dX.index_add_(0, i, _imatmul(di[o], Wi[k].t()))
    return dX


def assert_exact_range(x, W_or_dy, nbr, V_out):
    """Precondition of an exact case, from the reference alone: the operands are bf16-exact integers and the largest sum
    of absolute terms of any element (the same reference on |operands|) is below 2^24.  W_or_dy: W [K, Cin, Cout] (the
    forward's sums) or dy [V_out, Cout] (the weight gradient's).  Returns that largest sum."""
    a, b = _int(x).abs(), _int(W_or_dy).abs()
    assert int(a.max()) <= OPERAND_LIMIT and int(b.max()) <= OPERAND_LIMIT, "operands beyond the bf16-exact integers"
    ref = ref_forward(a, b, nbr, V_out) if b.dim() == 3 else ref_wgrad(a, b, nbr, V_out)
    biggest = int(ref.max()) if ref.numel() else 0
    assert biggest < EXACT_LIMIT, f"largest sum of absolute terms {biggest} >= 2^24: the case is not exact in fp32"
    return biggest


def ref_epilogue(acc, scale=None, shift=None, residual=None, act=0, slope=LEAKY_SLOPE):
    """The fused epilogue y = act(acc * scale + shift + residual) in float64 on the integer accumulator, cast to
    float32.  With scale from SCALES, integer shift / residual and slope 0.25 every intermediate is a multiple of 1/8;
    the assertion keeps it below 2^21, so each of the kernel's fp32 roundings (fma, add, multiply) is exact as well.
    Zeros: an absent shift beside a scale adds +0 and relu(negative) is +0, as the kernels define them.
    act: 0 none, 1 ReLU, 2 leaky ReLU."""
    v = acc.double()
    bound = v.abs().max() if v.numel() else v.new_zeros(())
    if scale is not None:
        v = v * scale.double() + (shift.double() if shift is not None else 0.0)
        bound = bound * scale.abs().max().double()
    elif shift is not None:
        v = v + shift.double()
    if shift is not None:
        bound = bound + shift.abs().max().double()
    if residual is not None:
        v = v + residual.double()
        bound = bound + residual.abs().max().double()
    assert float(bound) * 8 < EXACT_LIMIT, f"epilogue magnitude {float(bound)} * 8 >= 2^24: not exact in fp32"
    if act == 1:
        v = torch.where(v < 0, torch.zeros_like(v), v)
    elif act == 2:
        v = torch.where(v > 0, v, v * slope)
    return v.float()


def same_bits(a, b):
    """float32 tensors equal as int32 bit patterns (signed zeros told apart)"""
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ---------------------------------------------------------------------------------------------------------------------
# fp32 -> bf16 rounding table
# ---------------------------------------------------------------------------------------------------------------------
TIES = (0x3F808000, 0x3F818000, 0xBF808000, 0x3F80C000)  # tie down to even, tie up to even, negative tie, above the tie
MAX_FINITE = 0x7F7FFFFF                                  # rounds to +Inf
P_INF, N_INF, Q_NAN = 0x7F800000, 0xFF800000, 0x7FC00000
ZEROS = (0x00000000, 0x80000000)
SUBNORMALS = (0x00000001, 0x00400000, 0x007F8000, 0x00018000, 0x00010000, 0x00008000, 0x80008001, 0x80400000, 0x807FFFFF)


def from_bits(bits):
    """float32 tensor with the given bit patterns"""
    return torch.from_numpy(np.asarray(bits, dtype=np.uint32).view(np.float32).copy())


def bits_of(t):
    """bit patterns of a float32 tensor as int64 (for messages)"""
    return (t.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF)


def rne_bf16(t):
    """fp32 -> bf16 -> fp32, round to nearest even (torch's CPU conversion)"""
    return t.cpu().to(torch.bfloat16).float()
