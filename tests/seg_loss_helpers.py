"""float64 numpy restatement of the segmentation criterion and step metrics (include/sv_hip.h N7 and the Python layer
over it), written from the definitions; tests/test_seg_loss_cpu.py pins it to torch on the CPU."""
import numpy as np


def argmax_rows(x):
    """torch's max(1) index: the first index among equal maxima; the first NaN of a row is its maximum"""
    x = np.asarray(x)
    nan = np.isnan(x)
    return np.where(nan.any(1), nan.argmax(1), np.where(nan, -np.inf, x).argmax(1)).astype(np.int64)


def counted(labels, C, ignore_index=-100):
    labels = np.asarray(labels)
    return (labels != ignore_index) & (labels >= 0) & (labels < C)


def n_invalid(labels, C, ignore_index=-100):
    labels = np.asarray(labels)
    return int(((labels != ignore_index) & ((labels < 0) | (labels >= C))).sum())


def _exp_shifted(x):
    """exp(x_c - m) with m the row maximum (NaN when the row holds one: np.max propagates it, as the first-NaN rule does)"""
    with np.errstate(invalid="ignore", over="ignore"):
        m = x.max(1, keepdims=True) if x.shape[0] else np.zeros((0, 1))
        return m[:, 0], np.exp(x - m)


def row_losses(x, labels, ignore_index=-100):
    """lse(x) - x[y] of the counted rows in float64 (0 elsewhere), lse = m + log(sum exp(x_c - m)), m the row maximum"""
    x = np.asarray(x, np.float64)
    labels = np.asarray(labels)
    N, C = x.shape
    ok = counted(labels, C, ignore_index)
    m, e = _exp_shifted(x)
    y = np.where(ok, labels, 0)
    with np.errstate(invalid="ignore", divide="ignore"):
        rl = (m + np.log(e.sum(1))) - x[np.arange(N), y]
    return np.where(ok, rl, 0.0)


def loss(x, labels, reduction, ignore_index=-100):
    """sum or mean over the counted rows; mean over no row: NaN; an invalid label: NaN"""
    x = np.asarray(x, np.float64)
    ok = counted(labels, x.shape[1], ignore_index)
    if n_invalid(labels, x.shape[1], ignore_index):
        return float("nan")
    total = row_losses(x, labels, ignore_index)[ok].sum() if ok.any() else 0.0
    if reduction == "sum":
        return float(total)
    return float(total / ok.sum()) if ok.any() else float("nan")


def grad_unscaled(x, labels, ignore_index=-100):
    """softmax - onehot of the counted rows, 0 for ignored rows, NaN for rows with an invalid label.  The label's column
    is -(sum of the other columns): p - 1 cancels when p is close to 1."""
    x = np.asarray(x, np.float64)
    labels = np.asarray(labels)
    N, C = x.shape
    ok = counted(labels, C, ignore_index)
    m, e = _exp_shifted(x)
    y = np.where(ok, labels, 0)
    onehot = np.arange(C)[None, :] == y[:, None]
    with np.errstate(invalid="ignore", divide="ignore"):
        s = e.sum(1, keepdims=True)
        others = np.where(onehot, 0.0, e).sum(1, keepdims=True)
        g = np.where(onehot, -(others / s), e / s)
    g[~ok] = 0.0
    g[~ok & (labels != ignore_index)] = np.nan
    return g


def grad(x, labels, reduction, ignore_index=-100, dloss=1.0):
    g = grad_unscaled(x, labels, ignore_index)
    if reduction == "mean":
        n = max(int(counted(labels, np.asarray(x).shape[1], ignore_index).sum()), 1)  # no counted row: the rows stay 0 / NaN
        g = g * (dloss * (1.0 / np.float64(n)))
    else:
        g = g * dloss
    return g


def confusion(x, labels, offsets, ignore_index=-100):
    """int64 [B, C, C]: [b][gt][pred] over the counted rows of frame b; ignored int64 [B]"""
    x = np.asarray(x)
    labels = np.asarray(labels)
    C = x.shape[1]
    B = len(offsets) - 1
    pred = argmax_rows(x)
    ok = counted(labels, C, ignore_index)
    cm = np.zeros((B, C, C), np.int64)
    ign = np.zeros(B, np.int64)
    for b in range(B):
        lo, hi = offsets[b], offsets[b + 1]
        sel = ok[lo:hi]
        np.add.at(cm[b], (labels[lo:hi][sel], pred[lo:hi][sel]), 1)
        ign[b] = int((labels[lo:hi] == ignore_index).sum())
    return cm, ign


def accuracies(x, labels, offsets):
    """the reference's compute_accuracies formula (train_segmentation.py:34-46), frame by frame, as Python floats"""
    pred = argmax_rows(x)
    labels = np.asarray(labels)
    return [float((pred[lo:hi] == labels[lo:hi]).sum()) / (hi - lo) for lo, hi in zip(offsets[:-1], offsets[1:])]


def topk_rows(col, k):
    """rows of the k largest entries, largest first, ties to the lower row, NaN above +inf; -1 padded to k"""
    col = np.asarray(col, np.float64)
    key = np.where(np.isnan(col), np.inf, col)
    rank = np.isnan(col).astype(np.int64)  # NaN before +inf
    order = np.lexsort((np.arange(len(col)), -key, -rank))  # last key first: NaN, then value descending, then row
    out = np.full(k, -1, np.int64)
    out[:min(k, len(col))] = order[:k]
    return out


def segment_topk(col, offsets, k):
    return np.stack([topk_rows(col[lo:hi], k) for lo, hi in zip(offsets[:-1], offsets[1:])])


def quaternion_matrix(q):
    """(w, x, y, z), not necessarily unit -> 3 x 3 (utils/transformation.py get_quaternion_rotation_matrix_torch)"""
    r, i, j, k = (np.float64(v) for v in q)
    s = 2.0 / (r * r + i * i + j * j + k * k)
    return np.array([[1 - s * (j * j + k * k), s * (i * j - k * r), s * (i * k + j * r)],
                     [s * (i * j + k * r), 1 - s * (i * i + k * k), s * (j * k - i * r)],
                     [s * (i * k - j * r), s * (j * k + i * r), 1 - s * (i * i + j * j)]])


def pred_centers(out, coords, offsets, quantization_size, ee_r=0.03, q=None):
    """float64 [B, 3]: mean of coords[:, 1:] * quantization_size over the frame's up to 8 highest out[:, 1], plus
    R(q[b]) @ (-ee_r, 0, 0); an empty frame: NaN"""
    out = np.asarray(out)
    B = len(offsets) - 1
    c = np.full((B, 3), np.nan)
    for b in range(B):
        lo, hi = offsets[b], offsets[b + 1]
        sel = topk_rows(out[lo:hi, 1], 8)
        sel = sel[sel >= 0]
        if len(sel):
            pts = np.asarray(coords)[lo:hi, 1:][sel].astype(np.float64) * quantization_size
            tot = np.zeros(3)
            for p in pts:
                tot += p
            c[b] = tot / len(sel)
        if q is not None:
            c[b] = c[b] + quaternion_matrix(np.asarray(q, np.float64)[b]) @ np.array([-ee_r, 0.0, 0.0])
    return c


def center_dists(out, labels, coords, poses, offsets, quantization_size, ee_r=0.03):
    """(dist float64 [B], valid bool [B]) of train_vote.py:48-65: distance of the moved centre to poses[b, :3]; valid = the
    frame has a row with label 1"""
    poses = np.asarray(poses, np.float64)
    c = pred_centers(out, coords, offsets, quantization_size, ee_r, poses[:, 3:7])
    d = c - poses[:, :3]
    dist = np.sqrt((d * d).sum(1))
    labels = np.asarray(labels)
    valid = np.array([(labels[lo:hi] == 1).any() for lo, hi in zip(offsets[:-1], offsets[1:])])
    return dist, valid
