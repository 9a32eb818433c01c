"""PointNet++ training on the HIP path (set_training_path(model, "hip")).

Kernels: sv_group_rows against torch's index_points + subtraction (bit for bit), the index transpose + gather transpose
against a float64 index_add, sv_group_max against torch.max (values, indices, NaN, ties), its backward against autograd,
sv_three_nn_gather against sv_three_nn_interpolate (bit for bit) and sv_three_nn against square_distance + topk.
Modules and networks: the HIP step in fp32 against a float64 replay of the same step in torch expressions that takes
the HIP run's argmax and 3-NN choices (_Ref), with a float32 replay of the same choices as the measure of conditioning:
per tensor e <= 2 e32 + 16e-7 ||sum|terms| of the last reduction|| / ||want|| and e <= 1e-4 wherever e32 <= 5e-5; per
element for the biases in front of a train-mode BatchNorm (exact gradient 0) against the rounding noise of that zero.
Details above _record."""
import copy

import numpy as np
import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
REL = 1e-4


@pytest.fixture(scope="module")
def mods():
    import mrcc_amd
    from mrcc_amd import profiling
    from mrcc_amd.model import pointnet2, pointnet2_utils

    mrcc_amd._lib.load()
    return pointnet2, pointnet2_utils, profiling


def _cloud(B, N, seed, C=3):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(B, N, C, generator=g).to(DEV)


# ---- kernels ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order,D", [(0, 5), (1, 5), (0, 0), (1, 0)])
def test_group_rows_equals_torch_gather(mods, order, D):
    _, U, _ = mods
    B, N, S, K = 3, 500, 40, 32
    xyz = _cloud(B, N, 1)
    pts = _cloud(B, N, 2, D) if D else None
    new_xyz = U.index_points(xyz, U.farthest_point_sample(xyz, S, start=torch.zeros(B, dtype=torch.long)))
    idx = U.query_ball_point(0.15, K, xyz, new_xyz)  # small radius: many balls padded with the first hit
    assert (idx[..., -1] == idx[..., 0]).any()
    rows = U.group_rows(xyz, pts, new_xyz, idx, order)
    want = U._group(xyz, pts, new_xyz, idx, order)
    assert torch.equal(rows.view(B, S, K, -1), want)


def test_group_rows_group_all(mods):
    _, U, _ = mods
    B, N, D = 2, 128, 7
    xyz, pts = _cloud(B, N, 3), _cloud(B, N, 4, D)
    rows = U.group_rows(xyz, pts, None, None, 0)
    assert torch.equal(rows.view(B, 1, N, -1), U.sample_and_group_all(xyz, pts)[1])
    rows0 = U.group_rows(xyz, None, None, None, 0)
    assert torch.equal(rows0.view(B, N, 3), xyz)


def test_index_transpose_and_gather_transpose(mods):
    _, U, _ = mods
    B, S, K, N, C = 3, 64, 16, 300, 11
    g = torch.Generator().manual_seed(5)
    idx = torch.randint(0, N // 2, (B, S, K), generator=g).to(DEV)  # points >= N/2 are never referenced
    drows = torch.randn(B * S * K, C + 3, generator=g).to(DEV)
    csr = U._csr(idx, N, None)
    offsets, pos = csr
    assert offsets[0].item() == 0 and offsets[-1].item() == B * S * K
    got = U._gather_transpose(csr, None, drows, 3, C, 1, B * N, None).view(B, N, C)
    want = torch.zeros(B * N, C, dtype=torch.float64, device=DEV)
    flat = (idx + torch.arange(B, device=DEV).view(B, 1, 1) * N).reshape(-1)
    want.index_add_(0, flat, drows[:, 3:].double())
    assert (got.double().view(-1, C) - want).abs().max().item() <= 1e-5 * want.abs().max().item()
    assert torch.all(got[:, N // 2:] == 0)
    # positions ascending per target
    o, p = offsets.cpu().numpy(), pos.cpu().numpy()
    for t in range(0, B * N, 37):
        seg = p[o[t]:o[t + 1]]
        assert np.all(np.diff(seg) > 0) and np.all(flat.cpu().numpy()[seg] == t)
    again = U._gather_transpose(U._csr(idx, N, None), None, drows, 3, C, 1, B * N, None).view(B, N, C)
    assert torch.equal(got, again)
    # int32 tables and weights (the 3-NN form, per_row 3)
    w = torch.rand(B * S * K, generator=g).to(DEV)
    rows3 = torch.randn(B * S * K // 2, C, generator=g).to(DEV)
    idx3 = idx.view(B, -1)[:, : S * K // 2 * 2].to(torch.int32).contiguous()
    got3 = U._gather_transpose(U._csr(idx3, N, None), w, rows3, 0, C, 2, B * N, None)
    flat3 = (idx3.long() + torch.arange(B, device=DEV).view(B, 1) * N).reshape(-1)
    want3 = torch.zeros(B * N, C, dtype=torch.float64, device=DEV)
    want3.index_add_(0, flat3, rows3.double().repeat_interleave(2, 0) * w[: flat3.numel()].double().view(-1, 1))
    assert (got3.double() - want3).abs().max().item() <= 1e-5 * want3.abs().max().item()


def test_group_max_values_indices_nan_ties(mods):
    _, U, _ = mods
    G, K, C = 50, 32, 19
    g = torch.Generator().manual_seed(6)
    rows = torch.randn(G * K, C, generator=g).to(DEV)
    out, arg = U.GroupMaxFunction.apply(rows, K, None)
    v, i = rows.view(G, K, C).max(dim=1)
    assert torch.equal(out, v) and torch.equal(arg.long(), i)
    # ties go to the lowest row; the first NaN wins
    r2 = rows.clone().view(G, K, C)
    r2[:, 5, 0] = 100.0
    r2[:, 9, 0] = 100.0
    r2[:, 7, 1] = float("nan")
    r2[:, 3, 1] = float("nan")
    r2[:, 0, 2] = float("nan")
    r2 = r2.view(G * K, C)
    out2, arg2 = U.GroupMaxFunction.apply(r2, K, None)
    assert torch.all(arg2[:, 0] == 5) and torch.all(out2[:, 0] == 100.0)
    assert torch.all(arg2[:, 1] == 3) and torch.all(torch.isnan(out2[:, 1]))
    assert torch.all(arg2[:, 2] == 0) and torch.all(torch.isnan(out2[:, 2]))
    # group_all sizes: one group of N rows, any N
    big = torch.randn(2 * 128, 1024, generator=g).to(DEV)
    o3, a3 = U.GroupMaxFunction.apply(big, 128, None)
    v3, i3 = big.view(2, 128, 1024).max(dim=1)
    assert torch.equal(o3, v3) and torch.equal(a3.long(), i3)


def test_group_max_backward_equals_autograd(mods):
    _, U, _ = mods
    G, K, C = 40, 16, 23
    g = torch.Generator().manual_seed(7)
    rows = torch.randn(G * K, C, generator=g).to(DEV).requires_grad_()
    dp = torch.randn(G, C, generator=g).to(DEV)
    U.group_max(rows, K).backward(dp)
    r2 = rows.detach().clone().requires_grad_()
    r2.view(G, K, C).max(dim=1)[0].backward(dp)
    assert torch.equal(rows.grad, r2.grad)


def test_three_nn_gather_equals_interpolate_and_topk(mods):
    _, U, _ = mods
    B, N, S, C = 2, 700, 300, 33
    x1, x2 = _cloud(B, N, 8), _cloud(B, S, 9)
    p2 = torch.randn(B, S, C, generator=torch.Generator().manual_seed(10)).to(DEV)
    idx, w = U.three_nn(x1, x2)
    got = U.three_nn_gather(p2, idx, w)
    ref = U.three_nn_interpolate(x1, x2, p2)
    assert torch.equal(got, ref), (got - ref).abs().max().item()
    d, i = U.square_distance(x1, x2).topk(3, dim=-1, largest=False, sorted=True)
    untied = (d[..., 1] - d[..., 0] > 1e-5) & (d[..., 2] - d[..., 1] > 1e-5)
    assert untied.float().mean().item() > 0.9, untied.float().mean().item()
    assert torch.equal(idx.long()[untied], i[untied]), (idx.long()[untied] != i[untied]).sum().item()
    recip = 1.0 / (d + 1e-8)
    werr = (w - recip / recip.sum(-1, keepdim=True))[untied].abs().max().item()
    assert werr < 5e-4, werr
    # backward: the transpose with the weights against a float64 index_add
    p2g = p2.clone().requires_grad_()
    dout = torch.randn(B, N, C, generator=torch.Generator().manual_seed(11)).to(DEV)
    U.three_nn_gather(p2g, idx, w).backward(dout)
    want = torch.zeros(B * S, C, dtype=torch.float64, device=DEV)
    flat = (idx.long() + torch.arange(B, device=DEV).view(B, 1, 1) * S).reshape(-1)
    want.index_add_(0, flat, dout.double().view(B * N, 1, C).expand(B * N, 3, C).reshape(-1, C) *
                    w.double().reshape(-1, 1))
    gerr = (p2g.grad.double().view(-1, C) - want).abs().max().item()
    assert gerr <= 1e-5 * want.abs().max().item(), (gerr, want.abs().max().item())


# ---- modules ----------------------------------------------------------------------------------------------------
# ---- replay of a HIP step with its discrete choices -----------------------------------------------------------------
# _Ref replays a module / network step with torch expressions (the reference's), in float64 or float32, taking the
# group-max argmax and the 3-NN (idx, w) the HIP run chose (recorded by _record); sampling and ball query are recomputed
# from the fp32 coordinates (the same indices).  An argmax whose maxima are within rounding of each other (a flip) or a
# 3-NN near-tie therefore cannot move a gradient row between the runs; the flips against the float64 choice are counted
# and printed.  Bounds, per tensor against the float64 replay, with e the relative Frobenius error and e32 the float32
# replay's (the torch expressions' error on the same choices: the conditioning of the step):
#   e <= 2 e32 + 16e-7 ||T|| / ||want||, T the last reduction's sum|terms| (|x|^T |dz| of a weight, sum |dy| of a BN
#        bias, sum |dy x_hat| of a BN weight; 0 elsewhere);
#   e <= 1e-4 wherever e32 <= 5e-5;
# and per element for the conv / linear biases in front of a train-mode BatchNorm, whose exact gradient is 0 for any
# upstream gradient: |got - want| <= 16e-7 * sum_i |g| / sigma (|dy_i| + |mean dy| + (|z_i| + |mean z|) / sigma
# |mean(dy x_hat)|), the sum|terms| of BatchNorm's backward summed over the rows.
def _record(monkeypatch, U):
    events = []
    three_nn = U.three_nn

    def rec_group_max(rows, nsample, module=None):
        out, arg = U.GroupMaxFunction.apply(rows, nsample, module)
        events.append(arg.detach().clone())
        return out

    def rec_three_nn(xyz1, xyz2, module=None):
        idx, w = three_nn(xyz1, xyz2, module)
        events.append((idx.clone(), w.clone()))
        return idx, w

    monkeypatch.setattr(U, "group_max", rec_group_max)
    monkeypatch.setattr(U, "three_nn", rec_three_nn)
    return events


class _Ref:
    def __init__(self, U, module, events, dtype):
        self.U, self.events, self.dt = U, events, dtype
        self.i = 0
        self.p = {n: t.detach().to(dtype).requires_grad_() for n, t in module.named_parameters()}
        self.bn_mod = {n: m for n, m in module.named_modules() if isinstance(m, nn.modules.batchnorm._BatchNorm)}
        self.stats, self.convs, self.bns, self.after = {}, {}, {}, {}
        self.last_conv = None
        self.flips = [0, 0, 0]  # argmax flips, argmax entries, 3-NN rows whose neighbour set differs

    def conv(self, rows, name):
        w = self.p[name + ".weight"]
        z = rows @ w.reshape(w.shape[0], -1).t() + self.p[name + ".bias"]
        z.retain_grad()
        self.convs[name] = (rows, z)
        self.last_conv = name
        return z

    def bn(self, z, name):
        m = self.bn_mod[name]
        g, b = self.p[name + ".weight"], self.p[name + ".bias"]
        mean, var = z.mean(0), z.var(0, unbiased=False)
        sigma = torch.sqrt(var + m.eps)
        xh = (z - mean) / sigma
        mom = m.momentum
        self.stats[name] = ((1 - mom) * m.running_mean.to(self.dt) + mom * mean.detach(),
                            (1 - mom) * m.running_var.to(self.dt) + mom * z.detach().var(0, unbiased=True))
        y = xh * g + b
        y.retain_grad()
        self.bns[name] = (z.detach(), mean.detach(), sigma.detach(), xh.detach(), y)
        self.after[self.last_conv] = name
        return y

    def relu(self, y):
        return y * (y.detach() > 0)

    def mlp(self, rows, convs, bns):
        for c, b in zip(convs, bns):
            rows = self.relu(self.bn(self.conv(rows, c), b))
        return rows

    def gmax(self, rows, K):
        arg = self.events[self.i].long()
        self.i += 1
        G, C = rows.shape[0] // K, rows.shape[1]
        v = rows.view(G, K, C)
        picked = v.detach().gather(1, arg.unsqueeze(1)).squeeze(1)
        self.flips[0] += int((picked < v.detach().max(1)[0]).sum())
        self.flips[1] += arg.numel()
        return v.gather(1, arg.unsqueeze(1)).squeeze(1)

    def sa(self, mod, pre, xyz, pts, fps_start=None):
        """PointNetSetAbstraction: xyz [B, N, 3], pts [B, N, D] or None -> new_xyz, pooled [B, S, C]"""
        U = self.U
        B, N, _ = xyz.shape
        if mod.group_all:
            new_xyz, S, K = torch.zeros(B, 1, 3, dtype=xyz.dtype, device=DEV), 1, N
            rows = torch.cat([xyz] + ([pts] if pts is not None else []), -1).reshape(B * N, -1)
        else:
            fps = U.farthest_point_sample(xyz.float(), mod.npoint, start=fps_start)
            new_xyz = U.index_points(xyz, fps)
            S, K = mod.npoint, mod.nsample
            idx = U.query_ball_point(mod.radius, K, xyz.float(), new_xyz.float())
            rows = self.group(xyz, pts, new_xyz, idx, msg=False)
        convs = [f"{pre}mlp_convs.{i}" for i in range(len(mod.mlp_convs))]
        bns = [f"{pre}mlp_bns.{i}" for i in range(len(mod.mlp_bns))]
        return new_xyz, self.gmax(self.mlp(rows, convs, bns), K).view(B, S, -1)

    def group(self, xyz, pts, new_xyz, idx, msg):
        U = self.U
        B, S, K = idx.shape
        gx = U.index_points(xyz, idx) - new_xyz.view(B, S, 1, 3)
        if pts is None:
            return gx.reshape(B * S * K, 3)
        gp = U.index_points(pts, idx)
        return torch.cat([gp, gx] if msg else [gx, gp], -1).reshape(B * S * K, -1)

    def msg(self, mod, pre, xyz, pts, fps_start=None):
        U = self.U
        B = xyz.shape[0]
        fps = U.farthest_point_sample(xyz.float(), mod.npoint, start=fps_start)
        new_xyz = U.index_points(xyz, fps)
        pooled = []
        for i, (r, K) in enumerate(zip(mod.radius_list, mod.nsample_list)):
            idx = U.query_ball_point(r, K, xyz.float(), new_xyz.float())
            convs = [f"{pre}conv_blocks.{i}.{j}" for j in range(len(mod.conv_blocks[i]))]
            bns = [f"{pre}bn_blocks.{i}.{j}" for j in range(len(mod.bn_blocks[i]))]
            rows = self.mlp(self.group(xyz, pts, new_xyz, idx, msg=True), convs, bns)
            pooled.append(self.gmax(rows, K).view(B, mod.npoint, -1))
        return new_xyz, torch.cat(pooled, -1)

    def fp(self, mod, pre, xyz1, xyz2, p1, p2):
        """PointNetFeaturePropagation: xyz1 [B, N, 3], xyz2 [B, S, 3], p1 [B, N, C1] or None, p2 [B, S, C2] -> [B, N, C]"""
        B, N, _ = xyz1.shape
        if xyz2.shape[1] == 1:
            interp = p2.repeat(1, N, 1)
        else:
            idx, w = self.events[self.i]
            self.i += 1
            idx = idx.long()
            _, want = self.U.square_distance(xyz1.double(), xyz2.double()).topk(3, dim=-1, largest=False, sorted=True)
            self.flips[2] += int((want.sort(-1)[0] != idx.sort(-1)[0]).any(-1).sum())
            interp = (self.U.index_points(p2, idx) * w.to(self.dt).unsqueeze(-1)).sum(2)
        new = interp if p1 is None else torch.cat([p1, interp], -1)
        convs = [f"{pre}mlp_convs.{i}" for i in range(len(mod.mlp_convs))]
        bns = [f"{pre}mlp_bns.{i}" for i in range(len(mod.mlp_bns))]
        return self.mlp(new.reshape(B * N, -1), convs, bns).view(B, N, -1)

    def ssg_head(self, pre, l0):  # l0 [B, N, 128] -> [B, N, classes]
        B, N, C = l0.shape
        x = self.relu(self.bn(self.conv(l0.reshape(B * N, C), pre + "conv1"), pre + "bn1"))
        return self.conv(x, pre + "conv2").view(B, N, -1)

    def msg_head(self, pre, x):
        x = self.relu(self.bn(self.conv(x, pre + "fc1"), pre + "bn1"))
        x = self.relu(self.bn(self.conv(x, pre + "fc2"), pre + "bn2"))
        return self.conv(x, pre + "fc3")

    def ssg_net(self, m, x, fps):  # x [B, 6, N] -> [B, N, classes]
        xyz = x[:, :3].permute(0, 2, 1)
        pts = x.permute(0, 2, 1)
        l1x, l1p = self.sa(m.sa1, "sa1.", xyz, pts, fps[0])
        l2x, l2p = self.sa(m.sa2, "sa2.", l1x, l1p, fps[1])
        l3x, l3p = self.sa(m.sa3, "sa3.", l2x, l2p, fps[2])
        l4x, l4p = self.sa(m.sa4, "sa4.", l3x, l3p, fps[3])
        l3p = self.fp(m.fp4, "fp4.", l3x, l4x, l3p, l4p)
        l2p = self.fp(m.fp3, "fp3.", l2x, l3x, l2p, l3p)
        l1p = self.fp(m.fp2, "fp2.", l1x, l2x, l1p, l2p)
        return self.ssg_head("", self.fp(m.fp1, "fp1.", xyz, l1x, None, l1p))

    def msg_net(self, m, x, fps):  # x [B, 6, N] -> [B, classes]
        xyz, nrm = x[:, :3].permute(0, 2, 1), x[:, 3:].permute(0, 2, 1)
        l1x, l1p = self.msg(m.sa1, "sa1.", xyz, nrm, fps[0])
        l2x, l2p = self.msg(m.sa2, "sa2.", l1x, l1p, fps[1])
        _, l3p = self.sa(m.sa3, "sa3.", l2x, l2p)
        return self.msg_head("", l3p.reshape(x.shape[0], -1))

    def terms(self):
        """after the backward: (T of the last reduction per parameter gradient, the per-element noise bound's sum of
        the BatchNorm-preceded biases)"""
        T, noise = {}, {}
        for name, (x, z) in self.convs.items():
            w = self.p[name + ".weight"]
            T[name + ".weight.grad"] = (z.grad.abs().t() @ x.detach().abs()).reshape(w.shape)
            T[name + ".bias.grad"] = z.grad.abs().sum(0)
        for name, (z, mean, sigma, xh, y) in self.bns.items():
            dy = y.grad
            T[name + ".weight.grad"] = (dy * xh).abs().sum(0)
            T[name + ".bias.grad"] = dy.abs().sum(0)
            g = self.p[name + ".weight"].detach().abs()
            noise[name] = (g / sigma * (dy.abs() + dy.mean(0).abs() +
                                        (z.abs() + mean.abs()) / sigma * (dy * xh).mean(0).abs())).sum(0)
        return T, {c + ".bias.grad": noise[b] for c, b in self.after.items()}


def _reference(U, module, events, run, inputs, loss, dtype):
    """the replay of `run(ref, *inputs)` in `dtype`; inputs that require grad get gradients.  Returns (values, T,
    noise, flips): values has "out", the parameter gradients ".grad", the running statistics and "input{i}.grad"."""
    ref = _Ref(U, module, events, dtype)
    leaves = [None if t is None else t.detach().to(dtype).requires_grad_(t.requires_grad) for t in inputs]
    out = run(ref, *leaves)
    loss(out).backward()
    d = {"out": out.detach()}
    d.update({n + ".grad": p.grad for n, p in ref.p.items()})
    for name, (rm, rv) in ref.stats.items():
        d[name + ".running_mean"], d[name + ".running_var"] = rm, rv
    d.update({f"input{i}.grad": t.grad for i, t in enumerate(leaves) if t is not None and t.requires_grad})
    T, noise = ref.terms()
    return d, T, noise, ref.flips


def _check(got, want, w32, T, noise, label=""):
    """the bounds above; returns {name: (e, e32)}"""
    bad, errs = [], {}
    for n in want:
        g, w, t32 = (x.detach().double() for x in (got[n], want[n], w32[n]))
        if n in noise:  # a bias in front of a train-mode BatchNorm: per element against the noise of its exact zero
            over = ((g - w).abs() > 16e-7 * noise[n].double()).sum().item()
            if over:
                bad.append((n, "elements over the noise bound", over))
            continue
        wn = max(w.norm().item(), 1e-300)
        e, e32 = (g - w).norm().item() / wn, (t32 - w).norm().item() / wn
        floor = 16e-7 * T[n].double().norm().item() / wn if n in T else 0.0
        errs[n] = (e, e32)
        if not (e <= 2 * e32 + floor and (e32 > 5e-5 or e <= REL)):
            bad.append((n, e, e32, floor))
    assert not bad, f"{label} (name, e, e32, floor): {bad}"
    return errs


def _module_got(mod, out, args, grad_inputs):
    d = {"out": out.detach()}
    d.update({n + ".grad": p.grad for n, p in mod.named_parameters()})
    d.update({n: b for n, b in mod.named_buffers() if b.is_floating_point()})
    d.update({f"input{i}.grad": args[i].grad for i in grad_inputs})
    return d


def _check_module_step(U, monkeypatch, mod, args32, grad_inputs, run, fps=None):
    """one train() forward + backward of `mod` on the HIP path (fp32), against the float64 / float32 replays of its
    choices"""
    events = _record(monkeypatch, U)
    ref_mod = copy.deepcopy(mod)  # the parameters and the running statistics the step starts from
    U.set_training_path(mod, "hip")
    mod.train()
    out = mod(*args32, **({} if fps is None else {"fps_start": fps}))
    out = out[1] if isinstance(out, tuple) else out
    gy = torch.randn(out.shape, generator=torch.Generator().manual_seed(99), dtype=torch.float64).to(DEV)
    (out * gy.float()).sum().backward()
    got = _module_got(mod, out, args32, grad_inputs)
    loss = lambda o: (o * gy.to(o.dtype).view(o.shape)).sum()  # noqa: E731
    want, T, noise, flips = _reference(U, ref_mod, events, run, args32, loss, torch.float64)
    w32 = _reference(U, ref_mod, events, run, args32, loss, torch.float32)[0]
    print("flips (argmax, of, 3-NN rows):", flips)
    got = {k: v.reshape(want[k].shape) for k, v in got.items()}
    _check(got, want, w32, T, noise)


SSG_SA = [(1024, 0.1, 32, 6 + 3, [32, 32, 64], 2048, 6), (256, 0.2, 32, 64 + 3, [64, 64, 128], 1024, 64),
          (64, 0.4, 32, 128 + 3, [128, 128, 256], 256, 128), (16, 0.8, 32, 256 + 3, [256, 256, 512], 64, 256)]


@pytest.mark.parametrize("cfg", SSG_SA, ids=["sa1", "sa2", "sa3", "sa4"])
def test_ssg_set_abstraction_layers(mods, monkeypatch, cfg):
    _, U, _ = mods
    S, r, K, cin, mlp, N, D = cfg
    B = 2
    torch.manual_seed(0)
    m = U.PointNetSetAbstraction(S, r, K, cin, mlp, False).to(DEV)
    xyz = _cloud(B, N, 20).permute(0, 2, 1).contiguous()
    pts = torch.randn(B, D, N, generator=torch.Generator().manual_seed(21)).to(DEV).requires_grad_()
    fps = torch.tensor([3, 7], device=DEV)
    run = lambda R, x, p: R.sa(m, "", x.permute(0, 2, 1), p.permute(0, 2, 1), fps)[1].permute(0, 2, 1)  # noqa: E731
    _check_module_step(U, monkeypatch, m, [xyz, pts], [1], run, fps=fps)


@pytest.mark.parametrize("layer", ["sa1", "sa2"])
def test_msg_set_abstraction_layers(mods, monkeypatch, layer):
    P, U, _ = mods
    B = 2
    torch.manual_seed(0)
    if layer == "sa1":
        m = U.PointNetSetAbstractionMsg(512, [0.1, 0.2, 0.4], [16, 32, 128], 3,
                                        [[32, 32, 64], [64, 64, 128], [64, 96, 128]]).to(DEV)
        N, D = 1024, 3
    else:
        m = U.PointNetSetAbstractionMsg(128, [0.2, 0.4, 0.8], [32, 64, 128], 320,
                                        [[64, 64, 128], [128, 128, 256], [128, 128, 256]]).to(DEV)
        N, D = 512, 320
    xyz = _cloud(B, N, 22).permute(0, 2, 1).contiguous()
    pts = torch.randn(B, D, N, generator=torch.Generator().manual_seed(23)).to(DEV).requires_grad_()
    fps = torch.tensor([0, 5], device=DEV)
    run = lambda R, x, p: R.msg(m, "", x.permute(0, 2, 1), p.permute(0, 2, 1), fps)[1].permute(0, 2, 1)  # noqa: E731
    _check_module_step(U, monkeypatch, m, [xyz, pts], [1], run, fps=fps)


def test_group_all_layer(mods, monkeypatch):
    _, U, _ = mods
    B, N, D = 4, 128, 640
    torch.manual_seed(0)
    m = U.PointNetSetAbstraction(None, None, None, D + 3, [256, 512, 1024], True).to(DEV)
    xyz = _cloud(B, N, 24).permute(0, 2, 1).contiguous()
    pts = torch.randn(B, D, N, generator=torch.Generator().manual_seed(25)).to(DEV).requires_grad_()
    run = lambda R, x, p: R.sa(m, "", x.permute(0, 2, 1), p.permute(0, 2, 1))[1].permute(0, 2, 1)  # noqa: E731
    _check_module_step(U, monkeypatch, m, [xyz, pts], [1], run)


FP = [(768, [256, 256], 64, 16, 256, 512), (384, [256, 256], 256, 64, 128, 256), (320, [256, 128], 1024, 256, 64, 256),
      (128, [128, 128, 128], 2048, 1024, 0, 128)]


@pytest.mark.parametrize("cfg", FP, ids=["fp4", "fp3", "fp2", "fp1"])
def test_feature_propagation_layers(mods, monkeypatch, cfg):
    _, U, _ = mods
    cin, mlp, N, S, C1, C2 = cfg
    B = 2
    torch.manual_seed(0)
    m = U.PointNetFeaturePropagation(cin, mlp).to(DEV)
    x1 = _cloud(B, N, 26).permute(0, 2, 1).contiguous()
    x2 = _cloud(B, S, 27).permute(0, 2, 1).contiguous()
    g = torch.Generator().manual_seed(28)
    p1 = torch.randn(B, C1, N, generator=g).to(DEV).requires_grad_() if C1 else None
    p2 = torch.randn(B, C2, S, generator=g).to(DEV).requires_grad_()

    def run(R, a, b, c, d):
        t = (lambda v: None if v is None else v.permute(0, 2, 1))
        return R.fp(m, "", t(a), t(b), t(c), t(d)).permute(0, 2, 1)

    _check_module_step(U, monkeypatch, m, [x1, x2, p1, p2], [3] + ([2] if C1 else []), run)


class _HeadSSG(nn.Module):
    """PointNet2SSG's head alone (conv1 / bn1 / relu / dropout / conv2) on the HIP path"""

    def __init__(self, m):
        super().__init__()
        self.conv1, self.bn1, self.drop1, self.conv2 = m.conv1, m.bn1, m.drop1, m.conv2
        self.training_path = "hip"

    def forward(self, l0):
        from mrcc_amd.model.pointnet2 import PointNet2SSG

        return PointNet2SSG._head_train(self, l0)


class _HeadMSG(nn.Module):
    def __init__(self, m):
        super().__init__()
        self.fc1, self.bn1, self.drop1, self.fc2, self.bn2, self.drop2, self.fc3 = (
            m.fc1, m.bn1, m.drop1, m.fc2, m.bn2, m.drop2, m.fc3)
        self.training_path = "hip"

    def forward(self, x):
        from mrcc_amd.model.pointnet2 import PointNet2MSGEncoder

        return PointNet2MSGEncoder._head_train(self, x)


def test_heads(mods, monkeypatch):
    P, U, _ = mods
    torch.manual_seed(0)
    ssg = P.PointNet2SSG(6, in_channels=6).to(DEV)
    ssg.drop1.p = 0.0
    x = torch.randn(2, 128, 300, generator=torch.Generator().manual_seed(29)).to(DEV).requires_grad_()
    _check_module_step(U, monkeypatch, _HeadSSG(ssg), [x], [0], lambda R, a: R.ssg_head("", a.permute(0, 2, 1)))
    enc = P.PointNet2MSGEncoder(7).to(DEV)
    enc.drop1.p = enc.drop2.p = 0.0
    x = torch.randn(16, 1024, generator=torch.Generator().manual_seed(30)).to(DEV).requires_grad_()
    _check_module_step(U, monkeypatch, _HeadMSG(enc), [x], [0], lambda R, a: R.msg_head("", a))


# ---- whole networks ---------------------------------------------------------------------------------------------
def _ssg_inputs(B=4, N=2048, seed=40):
    g = torch.Generator().manual_seed(seed)
    xyz = torch.rand(B, 3, N, generator=g)
    x = torch.cat([xyz, torch.randn(B, 3, N, generator=g)], 1).to(DEV)
    y = torch.randint(0, 6, (B, N), generator=g).to(DEV)
    fps = torch.randint(0, N, (4, B), generator=g).to(DEV)
    return x, y, fps


def _ssg_step(model, x, y, fps):
    model.zero_grad(set_to_none=True)
    out, _ = model(x, fps_starts=fps)
    loss = nn.functional.cross_entropy(out.reshape(-1, out.shape[-1]), y.reshape(-1))
    loss.backward()
    return loss.detach(), {n: p.grad.detach().clone() for n, p in model.named_parameters()}


def _msg_inputs(B=8, N=1024, seed=41):
    g = torch.Generator().manual_seed(seed)
    xyz = torch.rand(B, 3, N, generator=g)
    nrm = torch.nn.functional.normalize(torch.randn(B, 3, N, generator=g), dim=1)
    x = torch.cat([xyz, nrm], 1).to(DEV)
    y = torch.randn(B, 7, generator=g).to(DEV)
    fps = torch.randint(0, N, (2, B), generator=g).to(DEV)
    return x, y, fps


def _msg_step(model, x, y, fps):
    model.zero_grad(set_to_none=True)
    out, _ = model(x, fps_starts=fps)
    loss = nn.functional.mse_loss(out, y)
    loss.backward()
    return loss.detach(), {n: p.grad.detach().clone() for n, p in model.named_parameters()}


def _nets(P, which):
    torch.manual_seed(0)
    if which == "ssg":
        m = P.PointNet2SSG(6, in_channels=6)
        m.drop1.p = 0.0
        return m.to(DEV), _ssg_inputs(), _ssg_step
    m = P.PointNet2MSGEncoder(7)
    m.drop1.p = m.drop2.p = 0.0
    return m.to(DEV), _msg_inputs(), _msg_step


@pytest.mark.parametrize("which", ["ssg", "msg"])
def test_whole_network_gradients_against_float64(mods, monkeypatch, which):
    """every parameter gradient of a HIP step against the float64 replay of its choices, with the float32 replay's error
    as the conditioning (the bounds above the replay); the torch path's own error against a float64 torch step (its own
    argmax / 3-NN choices) is printed for comparison"""
    P, U, _ = mods
    m32, (x, y, fps), step = _nets(P, which)
    m64, mt, ref_mod = copy.deepcopy(m32).double(), copy.deepcopy(m32), copy.deepcopy(m32)
    events = _record(monkeypatch, U)
    U.set_training_path(m32, "hip")
    m32.train(), m64.train(), mt.train()
    _, g32 = step(m32, x, y, fps)
    _, g64 = step(m64, x.double(), y if which == "ssg" else y.double(), fps)
    _, gt = step(mt, x, y, fps)
    if which == "ssg":
        run = lambda R, a: R.ssg_net(ref_mod, a, fps)  # noqa: E731
        loss = lambda o: nn.functional.cross_entropy(o.reshape(-1, o.shape[-1]), y.reshape(-1))  # noqa: E731
    else:
        run = lambda R, a: R.msg_net(ref_mod, a, fps)  # noqa: E731
        loss = lambda o: nn.functional.mse_loss(o, y.to(o.dtype))  # noqa: E731
    want, T, noise, flips = _reference(U, ref_mod, events, run, [x], loss, torch.float64)
    w32 = _reference(U, ref_mod, events, run, [x], loss, torch.float32)[0]
    names = [n + ".grad" for n, _ in m32.named_parameters()]
    errs = _check({n: g32[n[:-5]] for n in names}, {n: want[n] for n in names}, {n: w32[n] for n in names}, T, noise,
                  which)
    print("flips (argmax, of, 3-NN rows):", flips)
    for n, (e, e32) in errs.items():
        w = g64[n[:-5]].double()
        e_torch = (gt[n[:-5]].double() - w).norm().item() / max(w.norm().item(), 1e-300)
        print(f"{n:36s} hip {e:.2e}  fp32 replay {e32:.2e}  torch path vs float64 torch {e_torch:.2e}")


@pytest.mark.parametrize("which", ["ssg", "msg"])
def test_two_identical_hip_steps_give_identical_gradient_bits(mods, which):
    P, U, _ = mods
    m, (x, y, fps), step = _nets(P, which)
    U.set_training_path(m, "hip")
    m.train()
    sd = copy.deepcopy(m.state_dict())
    l1, g1 = step(m, x, y, fps)
    m.load_state_dict(sd)
    l2, g2 = step(m, x, y, fps)
    assert torch.equal(l1, l2)
    assert all(torch.equal(g1[n], g2[n]) for n in g1)


def test_default_path_is_todays_torch_path(mods):
    """without the switch, train() is the torch path: two models, one never switched and one switched to "hip" and back,
    give the same bits (the torch path's own nondeterminism aside, their kernels are the same: no sv_ entry runs)"""
    P, U, prof = mods
    m, (x, y, fps), step = _nets(P, "ssg")
    m.train()
    prof.TRAIN_LOG = []
    try:
        step(m, x, y, fps)
        assert prof.TRAIN_LOG == []
        U.set_training_path(m, "hip")
        U.set_training_path(m, "torch")
        step(m, x, y, fps)
        assert prof.TRAIN_LOG == []
    finally:
        prof.TRAIN_LOG = None


def test_train_log_and_fallback(mods):
    P, U, prof = mods
    m, (x, y, fps), step = _nets(P, "ssg")
    U.set_training_path(m, "hip")
    m.train()
    prof.TRAIN_LOG = []
    try:
        step(m, x, y, fps)
        log = list(prof.TRAIN_LOG)
        prof.TRAIN_LOG = []
        xg = x.clone().requires_grad_()  # coordinates that require grad: sa1 takes the torch path for the call
        m.zero_grad()
        out, _ = m(xg, fps_starts=fps)
        out.sum().backward()
        log2 = list(prof.TRAIN_LOG)
    finally:
        prof.TRAIN_LOG = None
    for name, q in m.named_modules():  # every 1x1 conv once per op, under its own module
        if isinstance(q, (nn.Conv1d, nn.Conv2d)):
            assert [f for mod, op, f in log if mod is q and op == "fwd"] == ["sv_conv_fwd_acc"], name
            assert [f for mod, op, f in log if mod is q and op == "dw"] == ["sv_conv_wgrad"], name
            dx = [f for mod, op, f in log if mod is q and op == "dx"]
            assert dx == ([] if name == "sa1.mlp_convs.0" else ["sv_conv_fwd_acc"]), name  # sa1's rows need no dX
    assert all(mod is not None for mod, _, _ in log)
    ops = {(mod, op) for mod, op, _ in log}
    for name in ("sa1", "sa2", "sa3", "sa4"):
        assert (getattr(m, name), "group_rows") in ops and (getattr(m, name), "group_max") in ops
        assert (getattr(m, name), "group_max_backward") in ops
    for name in ("sa2", "sa3", "sa4"):  # sa1's features are the input, which needs no gradient
        assert (getattr(m, name), "gather_transpose") in ops
    for name in ("fp4", "fp3", "fp2", "fp1"):
        assert (getattr(m, name), "three_nn") in ops and (getattr(m, name), "three_nn_gather") in ops
        assert (getattr(m, name), "index_transpose") in ops
    assert (m.sa1, "fallback", "torch") in log2 and m.sa1.train_fallbacks == 1
    assert xg.grad is not None and torch.isfinite(xg.grad).all()


def test_no_vendor_gemm_or_convolution_kernel_in_a_step(mods):
    P, U, _ = mods
    m, (x, y, fps), step = _nets(P, "ssg")
    U.set_training_path(m, "hip")
    m.train()
    step(m, x, y, fps)  # warm
    torch.cuda.synchronize()
    with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
        step(m, x, y, fps)
        torch.cuda.synchronize()
    names = {e.key for e in prof.key_averages()}
    low = [n.lower() for n in names]
    assert any("group_max_kernel" in n for n in low) and any("conv" in n and "sv::" in n for n in low), sorted(names)
    vendor = ("cijk_", "igemm", "naive_conv", "miopenconv", "miopensp3asmconv", "gridwise_conv", "im2col", "winograd")
    assert not [n for n in names if any(v in n.lower() for v in vendor)]


def _key_point_crops(B, N, seed):
    """synthetic crops with per-point key-point labels (train_key_points.py: class = nearest of five key points, or
    background beyond a radius)"""
    g = torch.Generator().manual_seed(seed)
    xyz = torch.rand(B, 3, N, generator=g)
    kp = torch.rand(B, 5, 3, generator=g)
    d = ((xyz.permute(0, 2, 1)[:, :, None, :] - kp[:, None, :, :]) ** 2).sum(-1)  # [B, N, 5]
    dmin, near = d.min(-1)
    y = torch.where(dmin < 0.05, near + 1, torch.zeros_like(near))
    x = torch.cat([xyz, xyz - 0.5], 1)  # use_coordinates_as_features
    return x.to(DEV), y.to(DEV)


def test_train_key_points_loop_and_eval_after_training(mods):
    P, U, _ = mods
    torch.manual_seed(3)
    m = P.PointNet2SSG(6, in_channels=6).to(DEV)
    U.set_training_path(m, "hip")
    opt = torch.optim.Adam(m.parameters(), lr=1e-2)
    x, y = _key_point_crops(4, 1024, 50)
    fps = torch.zeros(4, 4, dtype=torch.long, device=DEV)
    losses = []
    m.train()
    for _ in range(25):
        opt.zero_grad()
        out, _ = m(x, fps_starts=fps)
        loss = nn.functional.cross_entropy(out.reshape(-1, 6), y.reshape(-1))
        loss.backward()
        opt.step()
        losses.append(loss.item())
    assert all(np.isfinite(losses)) and losses[-1] < 0.5 * losses[0], losses
    m.eval()
    with torch.no_grad():
        got, l4 = m(x, fps_starts=fps)
    fresh = P.PointNet2SSG(6, in_channels=6).to(DEV)
    fresh.load_state_dict(m.state_dict())
    fresh.eval()
    with torch.no_grad():
        want, l4w = fresh(x, fps_starts=fps)
    assert torch.equal(got, want) and torch.equal(l4, l4w)
