"""sv_sinusoidal (ME.MinkowskiSinusoidal) against float64 at the bound of its definition (include/sv_hip.h):

    |coef_n| ((Cin + 2) u (sum_k |x_k K_kn| + |b_n|) + u) + u |want|,   u = 2^-24

- the fp32 argument's rounding (Cin products and sums, the bias), one rounding for the sine of that argument, one for the
product with coef.  A fast-math sine fails it at the inputs scaled by 5000 (arguments of tens of thousands).  Inputs and
outputs are column views of wider buffers whose other columns hold a sentinel."""
import pytest
import torch

import field_helpers as FH

pytestmark = pytest.mark.gpu

NS = (0, 1, 63, 64, 65, 1000)
SCALES = (1.0, 100.0, 5000.0)


def _inputs(N, cin, cout, scale, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(N, cin, generator=g) * scale, torch.randn(cin, cout, generator=g), torch.randn(cout, generator=g),
            torch.randn(cout, generator=g))


@pytest.mark.parametrize("cout", [1, 32, 33, 64])
@pytest.mark.parametrize("cin", [1, 3, 35, 67])
def test_sinusoidal_within_the_bound(gpu, cin, cout):
    worst = 0.0
    for N in NS:
        for scale in SCALES:
            x, k, b, c = _inputs(N, cin, cout, scale, seed=cin * 1000 + cout)
            got = FH.run_sinusoidal(gpu, x, k, b, c)
            assert got.shape == (N, cout)
            if N == 0:
                continue
            want = FH.sinusoidal_ref(x.double(), k.double(), b.double(), c.double())
            ratio = float(((got.double() - want).abs() / FH.sinusoidal_bound(x, k, b, c, want)).max())
            worst = max(worst, ratio)
            assert ratio <= 1.0, f"N = {N}, scale = {scale}: error / bound = {ratio:.3f}"
            assert torch.equal(FH.bits(FH.run_sinusoidal(gpu, x, k, b, c)), FH.bits(got)), "two calls differ"
    print(f"sv_sinusoidal Cin = {cin}, Cout = {cout}: largest error / bound = {worst:.3f}")


def test_arguments_up_to_2_pow_20(gpu):
    """one input channel, kernel 1, bias 0, coef 1: the result is the correctly rounded sine of the float32 input, up to the
    double rounding (error <= u |want| (1 + 2^-28))"""
    g = torch.Generator().manual_seed(9)
    x = torch.cat([(torch.rand(4000, 1, generator=g) * 2 - 1) * 2.0 ** 20, torch.tensor([[2.0 ** 20], [-2.0 ** 20], [1048575.9375]])])
    got = FH.run_sinusoidal(gpu, x, torch.ones(1, 1), torch.zeros(1), torch.ones(1))
    want = torch.sin(x.double())
    assert float(((got.double() - want).abs() / want.abs()).max()) <= FH.U * (1 + 2.0 ** -28)


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), -float("inf")])
def test_a_non_finite_input_stays_in_its_row(gpu, bad):
    x, k, b, c = _inputs(130, 35, 64, 1.0, seed=4)
    clean = FH.run_sinusoidal(gpu, x, k, b, c)
    x[77, 20] = bad
    got = FH.run_sinusoidal(gpu, x, k, b, c)
    assert torch.isnan(got[77]).all()
    keep = torch.arange(130) != 77
    assert torch.equal(FH.bits(got[keep]), FH.bits(clean[keep]))


def test_module_on_a_field_and_on_a_sparse_tensor(gpu):
    """MinkowskiSinusoidal in eval() returns the same kind of tensor on the same coordinates, the values sv_sinusoidal's;
    batch norm, ReLU, leaky ReLU and linear take a field as well"""
    import numpy as np

    from mrcc_amd import MinkowskiEngine as ME

    torch.manual_seed(2)
    layer = ME.MinkowskiSinusoidal(3, 32).to(gpu).eval()
    pts = FH.stage_cloud()
    g = torch.Generator().manual_seed(3)
    F = torch.randn(len(pts), 3, generator=g)
    with torch.no_grad():
        field = ME.TensorField(F, torch.from_numpy(pts.astype(np.float32) + np.float32(0.25)), device=gpu)
        out = layer(field)
        assert isinstance(out, ME.TensorField) and out.C is field.C
        want = FH.run_sinusoidal(gpu, F, layer.kernel.detach().cpu(), layer.bias.detach().cpu().reshape(-1),
                                 layer.coef.detach().cpu().reshape(-1))
        assert torch.equal(FH.bits(out.F.cpu()), FH.bits(want))
        st = field.sparse()
        sout = layer(st)
        assert isinstance(sout, ME.SparseTensor) and sout.coordinate_manager is st.coordinate_manager and sout.F.shape == (len(st), 32)
        chain = [ME.MinkowskiBatchNorm(32), ME.MinkowskiReLU(), ME.MinkowskiLeakyReLU(0.1), ME.MinkowskiLinear(32, 32)]
        y = out
        for m in chain:
            y = m.to(gpu).eval()(y)
            assert isinstance(y, ME.TensorField) and y.F.shape == (len(pts), 32)
        ref = torch.nn.functional.leaky_relu(torch.relu(chain[0].bn.cpu().double()(want.double())), 0.1)
        ref = ref @ chain[3].linear.weight.detach().cpu().double().t() + chain[3].linear.bias.detach().cpu().double()
        assert float((y.F.cpu().double() - ref).abs().max() / ref.abs().max()) <= 1e-4
        # the derived fields share one voxelisation: their tensors live on one manager
        assert y.sparse().coordinate_manager is out.sparse().coordinate_manager
