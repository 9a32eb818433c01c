"""Every (instance, fast, ring, full) combination the public fp32 sparse-convolution call can dispatch to, bit-exact
against oracle.conv, with the instance name AND the three form flags asserted (sv_conv_last_instance).

One test per row of conv_instance_helpers.CASES (tests/test_conv_instances_cpu.py shows the table is complete).  No
SV_CONV_FORCE* switch anywhere: what runs is what the library dispatches for the row's shape, scale and operands.

Each row runs the layer with the full epilogue (scale, shift, residual with its own row stride, ReLU) on a column slice
of a wider input buffer, into a column slice of a sentinel-filled wider output buffer whose other columns must keep the
sentinel.  Maps are compact blobs of integer coordinates, so V is exact and 3x3x3 neighbours exist; every V leaves the last
128-row plan tile with 67 rows (three live rows in its second 64-row tile, three dead 16-row sub-tiles).

Second part: every row's layer one plan tile smaller must dispatch as the restatement says (names and flags only), which
pins each threshold from its other side.  Third part: the row edges of the special kernels (thin, LDS-weights thin, first
layer on the matrix pipe and on the vector ALU, narrow linear) at V = 1 .. 129, where sub-tiles are fewer than waves and
workgroups find no work.
"""
import contextlib

import numpy as np
import pytest
import torch

import conv_instance_helpers as H

pytestmark = pytest.mark.gpu

SENTINEL = 7.0
# rows that share a shape are neighbours, so that the one-entry operand / oracle cache below serves them
ROWS = sorted(H.CASES, key=lambda c: (c.kind, c.V, c.Cin, c.Cout, H.case_id(c)))


def _blob(V):
    """V integer voxels of a compact block (x fastest), centred on the origin"""
    s = int(np.ceil(V ** (1.0 / 3.0)))
    while s ** 3 < V:
        s += 1
    i = np.arange(V, dtype=np.int64)
    c = np.stack([np.zeros(V, np.int64), i % s, (i // s) % s, i // (s * s)], axis=1)
    c[:, 1:] -= s // 2
    return c


@pytest.fixture(scope="module")
def maps(gpu, oracle):
    """V -> the GPU coordinate manager and the oracle's frame of the V-voxel blob, built on first use"""
    from mrcc_amd import MinkowskiEngine as ME

    cache = {}

    def get(V):
        if V not in cache:
            c4 = _blob(V)
            st = ME.SparseTensor(torch.zeros(V, 1), coordinates=torch.from_numpy(c4).int(), device=gpu)
            cm = st.coordinate_manager
            frame = oracle.Frame(oracle.voxelize(c4, coords_are_int=True)["coords"])
            assert cm.stride_map(1).V == V == len(frame.maps[1])
            cache[V] = (cm, frame)
        return cache[V]

    return get


@pytest.fixture(scope="module")
def shapes(oracle, maps):
    """(kind, K, Cin, Cout, V) -> host operands, the kernel map and the oracle's result; the last shape is kept"""
    last = {}

    def get(kind, K, Cin, Cout, V):
        key = (kind, K, Cin, Cout, V)
        if last.get("key") != key:
            last.clear()
            rng = np.random.default_rng([K, Cin, Cout, V])
            nbr, V_in = None, V
            if kind != "dense":
                cm, frame = maps(V)
                if kind == "up":
                    V_in = len(frame.down(1))
                    nbr = frame.kup(2)
                else:
                    nbr = frame.k3(1)
            # column slices of wider buffers: 16-byte aligned start and row stride wherever Cin allows float4 gathers
            in_off, in_ld = (4, Cin + 8) if Cin % 4 == 0 else (1, Cin + 2)
            xbuf = rng.standard_normal((V_in, in_ld), dtype=np.float32)
            W = rng.standard_normal((K, Cin, Cout), dtype=np.float32) * np.float32(0.1)
            scale = rng.uniform(0.5, 1.5, size=Cout).astype(np.float32)
            shift = rng.standard_normal(Cout, dtype=np.float32)
            resbuf = rng.standard_normal((V, Cout + 4), dtype=np.float32)
            x = np.ascontiguousarray(xbuf[:, in_off:in_off + Cin])
            res = np.ascontiguousarray(resbuf[:, :Cout])
            want = oracle.conv(x, W, nbr, V, scale, shift, res, oracle.ACT_RELU)
            last.update(key=key, xbuf=xbuf, in_off=in_off, W=W, scale=scale, shift=shift, resbuf=resbuf, want=want, V_in=V_in)
        return last

    return get


def _misaligned_perm(plan):
    """a copy of the plan whose `perm` starts 4 bytes off a 16-byte boundary (a plan carved from a workspace at an odd
    offset): the buffer-addressed epilogue cannot read it four entries at a time"""
    from mrcc_amd.sparse import ConvPlan

    buf = torch.empty(plan.Vpad + 1, dtype=torch.int32, device=plan.perm.device)
    buf[1:] = plan.perm
    perm = buf[1:1 + plan.Vpad]
    assert perm.data_ptr() % 16 == 4
    return ConvPlan(perm, plan.nbr_s, plan.submask, plan.tile_order, plan.V_out, plan.Vpad, plan.K)


def _plan(maps, kind, V, reason=None, split=None):
    if kind == "dense":
        return None
    cm, _ = maps(V)
    if kind == "up":
        cm.plan_down(1)
        plan = cm.plan_up(2)
    elif split is not None:
        return cm.plan_k3_split(1, split)
    else:
        plan = cm.plan_k3(1)
    assert plan.V_out == V and plan.Vpad == (V + 127) // 128 * 128
    return _misaligned_perm(plan) if reason == "perm_misaligned" else plan


def _run(gpu, ops, plan, Cin, Cout, V, scale=None):
    """(result, name, flags, the output buffer's other columns untouched) of one public call"""
    import mrcc_amd
    from mrcc_amd import nn as svnn

    t = lambda a: torch.from_numpy(a).to(gpu)  # noqa: E731
    x = t(ops["xbuf"])[:, ops["in_off"]:ops["in_off"] + Cin]
    res = t(ops["resbuf"])[:, :Cout]
    out_ld = (Cout + 3) // 4 * 4 + 8
    out_buf = torch.full((V, out_ld), SENTINEL, device=gpu)
    out = out_buf[:, 4:4 + Cout]  # 16-byte aligned start, row stride a multiple of four floats
    with (mrcc_amd._lib.conv_dispatch(scale) if scale is not None else contextlib.nullcontext()):
        svnn.conv_forward(x, t(ops["W"]), plan, V, t(ops["scale"]), t(ops["shift"]), res, 1, out=out)
        name, flags = mrcc_amd._lib.conv_last_instance()
    got = out.cpu().numpy()
    untouched = bool((out_buf[:, :4] == SENTINEL).all()) and bool((out_buf[:, 4 + Cout:] == SENTINEL).all())
    return got, name, flags, untouched


@pytest.mark.parametrize("case", ROWS, ids=H.case_id)
def test_dispatched_instance_and_form_bit_exact(gpu, oracle, maps, shapes, case):
    c = case
    ops = shapes(c.kind, c.K, c.Cin, c.Cout, c.V)
    plan = _plan(maps, c.kind, c.V, c.reason, c.split)
    got, name, flags, untouched = _run(gpu, ops, plan, c.Cin, c.Cout, c.V, c.scale)
    assert (name, flags) == (c.name, {"fast": c.fast, "ring": c.ring, "full": c.full})
    want = ops["want"]
    assert np.array_equal(got, want), f"{int((got != want).sum())} of {want.size} differ, max abs diff {np.abs(got - want).max()}"
    assert untouched, "columns beside the output slice were written"


# ---- the other side of every threshold ---------------------------------------------------------------------------
# A row sits at the smallest padded row count that reaches its combination, so it notices a threshold that moves UP.  The
# same layer one plan tile smaller notices one that moves DOWN: it must still dispatch as the restatement says (whose lists
# and thresholds the rows above pin against the library).  Names and flags only - no oracle, operands made on the device.
BELOW = sorted({(c.kind, c.K, c.Cin, c.Cout, c.V - 128, c.scale, c.reason, c.split) for c in H.CASES if c.V > 128},
               key=lambda b: (b[0], b[4], str(b)))


def _below_id(b):
    kind, K, Cin, Cout, V, scale, reason, split = b
    return f"{kind}-{Cin}x{Cout}-V{V}-{reason or 'plain'}" + ("-alone" if scale else "") + (f"-split{split}" if split else "")


@pytest.mark.parametrize("below", BELOW, ids=_below_id)
def test_one_plan_tile_below_a_row_dispatches_as_restated(gpu, maps, below):
    import mrcc_amd
    from mrcc_amd import nn as svnn

    kind, K, Cin, Cout, V, scale, reason, split = below
    probe = H.Case(kind, K, Cin, Cout, V, scale, reason, split, None, None, None, None)
    want_name, want_flags = H.dispatch(*H.case_inputs(probe))
    plan = _plan(maps, kind, V, reason, split)
    V_in = maps(V)[0].stride_map(2).V if kind == "up" else V
    g = torch.Generator(device=gpu).manual_seed(V + Cin)
    in_off, in_ld = (4, Cin + 8) if Cin % 4 == 0 else (1, Cin + 2)
    x = torch.randn((V_in, in_ld), device=gpu, generator=g)[:, in_off:in_off + Cin]
    W = torch.randn((K, Cin, Cout), device=gpu, generator=g) * 0.1
    with (mrcc_amd._lib.conv_dispatch(scale) if scale is not None else contextlib.nullcontext()):
        out = svnn.conv_forward(x, W, plan, V, act=1)
        name, flags = mrcc_amd._lib.conv_last_instance()
    assert (name, flags) == (want_name, want_flags)
    assert bool(torch.isfinite(out).all())


# ---- row edges of the special kernels ------------------------------------------------------------------------------
EDGE_V = (1, 15, 16, 17, 127, 128, 129)
# (expected name, flags, kind, K, Cin, Cout, dispatch scale, perm misaligned)
SPECIAL = [
    ("conv_thin_kernel<32, 32>", (1, 0, 1), "k3", 27, 32, 32, None, False),
    ("conv_thin_lds_kernel<32, 32>", (1, 0, 1), "k3", 27, 32, 32, 1.0, False),
    ("conv_first_mfma_kernel<3, 32>", (1, 0, 1), "k3", 27, 3, 32, None, False),
    ("conv_first_layer_kernel<3, 32>", (0, 0, 0), "k3", 27, 3, 32, None, True),
    ("linear_narrow_kernel<1>", (0, 0, 0), "dense", 1, 64, 1, None, False),
    ("linear_narrow_kernel<3>", (0, 0, 0), "dense", 1, 100, 3, None, False),
    ("linear_narrow_kernel<4>", (0, 0, 0), "dense", 1, 256, 4, None, False),
]


@pytest.mark.parametrize("V", EDGE_V)
@pytest.mark.parametrize("spec", SPECIAL, ids=lambda s: s[0].split("<")[0] + "-" + str(s[5]) + ("-alone" if s[6] else ""))
def test_special_kernels_at_row_edges(gpu, oracle, maps, shapes, spec, V):
    """V = 1 .. 17: fewer 16-row sub-tiles than a workgroup has waves, workgroups (and, on the LDS-weights kernel, whole
    queues) without work; 127 .. 129: the last plan tile full, one row short, and a second tile of one row"""
    name_want, (fast, ring, full), kind, K, Cin, Cout, scale, misaligned = spec
    ops = shapes(kind, K, Cin, Cout, V)
    plan = _plan(maps, kind, V, "perm_misaligned" if misaligned else None)
    got, name, flags, untouched = _run(gpu, ops, plan, Cin, Cout, V, scale)
    assert (name, flags) == (name_want, {"fast": fast, "ring": ring, "full": full})
    want = ops["want"]
    assert np.array_equal(got, want), f"V {V}: {int((got != want).sum())} of {want.size} differ, max abs diff {np.abs(got - want).max()}"
    assert untouched, "columns beside the output slice were written"
