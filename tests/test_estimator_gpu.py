"""'Next' row f-1: the fused evaluation of the weight estimator (channel-major GEMMs + one HIP pass for
InstanceNorm+LeakyReLU) against the stock PyTorch module with the same parameters.  GPU box only."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def relerr(a, b):
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


@pytest.mark.parametrize("C,R,N", [(64, 5, 100), (1024, 3, 100), (7, 2, 8), (16, 4, 500)])
def test_inorm_lrelu_kernel_matches_torch(dfepe, C, R, N):
    g = torch.Generator().manual_seed(C + N)
    Y = (torch.randn(C, R, N, generator=g) * 3 + 1).to(DEV).requires_grad_(True)
    gamma = (1 + 0.2 * torch.randn(C, generator=g)).to(DEV).requires_grad_(True)
    beta = (0.3 * torch.randn(C, generator=g)).to(DEV).requires_grad_(True)
    G = torch.randn(C, R, N, generator=g).to(DEV)
    A = dfepe.ops.inorm_lrelu(Y, gamma, beta, 1e-5, 0.01)
    (A * G).sum().backward()
    Yr, gr, br = (t.detach().clone().double().requires_grad_(True) for t in (Y, gamma, beta))
    x = Yr.permute(1, 0, 2)  # [R, C, N] = (batch, channels, points)
    ref = torch.nn.functional.leaky_relu(torch.nn.functional.instance_norm(x, weight=gr, bias=br, eps=1e-5), 0.01).permute(1, 0, 2)
    (ref * G.double()).sum().backward()
    assert relerr(A.detach().double(), ref.detach()) < 1e-5
    assert relerr(Y.grad.double(), Yr.grad) < 1e-4
    assert relerr(gamma.grad.double(), gr.grad) < 1e-4
    assert relerr(beta.grad.double(), br.grad) < 1e-4


def test_inorm_lrelu_rejects_unsupported_shapes(dfepe):
    with pytest.raises(dfepe.DfepeError):
        dfepe.ops.inorm_lrelu(torch.zeros(4, 2, 10, device=DEV), torch.ones(4, device=DEV), torch.zeros(4, device=DEV))  # N % 4 != 0


@pytest.mark.parametrize("cin", [4, 7])
def test_fused_estimator_equals_stock_module(dfepe, cin):
    B, N = 6, 100
    EE = dfepe.compat.ErrorEstimators
    stock = EE.ErrorEstimator(cin).to(DEV)
    dfepe.synth.fill_params_deterministic(stock, seed=3)
    fused = EE.FusedErrorEstimator(cin).to(DEV)
    fused.load_state_dict(stock.state_dict())
    assert list(fused.state_dict().keys()) == list(stock.state_dict().keys())
    g = torch.Generator().manual_seed(0)
    x = torch.rand(B, cin, N, generator=g).to(DEV)
    G = torch.randn(B, 1, N, generator=g).to(DEV)
    xa, xb = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
    ya, yb = stock(xa), fused(xb)
    assert yb.shape == ya.shape == (B, 1, N)
    assert relerr(yb.detach(), ya.detach()) < 2e-4
    (ya * G).sum().backward()
    (yb * G).sum().backward()
    assert relerr(xb.grad, xa.grad) < 2e-3
    pa, pb = dict(stock.named_parameters()), dict(fused.named_parameters())
    for name in pa:
        # every parameter takes part in the graph (DistributedDataParallel needs that; the optimizer state then matches the
        # reference's): the biases that cancel in an InstanceNorm get the exact zero the stock module computes numerically
        assert pb[name].grad is not None, name
        if pb[name].grad.abs().max().item() == 0.0:
            assert name.endswith(".bias") and pa[name].grad.abs().max().item() < 1e-3 * max(1.0, G.abs().sum().item()) * 1e-3
            continue
        assert relerr(pb[name].grad, pa[name].grad) < 5e-3, name


def test_batchnorm_variant_is_not_chunked_in_training_mode(dfepe):
    """Batch statistics span the whole batch: the chunked evaluation (MIOpen work-around) only applies without BatchNorm in
    training mode."""
    EE = dfepe.compat.ErrorEstimators
    net = EE.ErrorEstimator(4, if_bn=True).to(DEV)
    net.max_chunk = 4
    x = torch.rand(10, 4, 20, device=DEV)
    net.train()
    y = net(x)
    ref = net.fw(x)
    assert y.shape == (10, 1, 20) and torch.isfinite(y).all() and relerr(y.detach(), ref.detach()) < 1e-5


# ---- inorm_lrelu held per element (tests/est_norm_ref.py, tests/est_norm_cases.py) and the native-fp32 stack's backward ------------------
import os  # noqa: E402
import sys  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import est_norm_cases as cs  # noqa: E402
import est_norm_ref as nref  # noqa: E402


@pytest.mark.parametrize("case", cs.INORM, ids=cs.case_id)
def test_inorm_lrelu_against_the_fp64_restatement(dfepe, case):
    """ops.inorm_lrelu forward and backward, every template (2 / 4 / 8 float4 per lane) on each side of N = 128 and 256, row counts around
    the 16 rows of a workgroup: every element within TOL times its own bound of the restatement; a second call bit for bit."""
    _, N, C, R = case
    Y, gamma, beta, G = (t.to(DEV) for t in cs.inorm_inputs(case))

    def call():
        y, gm, bt = (t.clone().requires_grad_(True) for t in (Y, gamma, beta))
        A = dfepe.ops.inorm_lrelu(y, gm, bt, cs.EPS, 0.01)
        (A * G).sum().backward()
        return A.detach(), y.grad, gm.grad, bt.grad

    A, gY, gg, gb = call()
    # the statistics the backward kernel was given: the forward kernel's own, from a direct call on the same input
    stats = torch.full((C * R, 2), float("nan"), device=DEV)
    A2 = torch.empty_like(Y)
    assert dfepe._lib.lib().dfepe_inorm_lrelu_fwd(Y.data_ptr(), gamma.data_ptr(), beta.data_ptr(), C, R, N, cs.EPS, 0.01, A2.data_ptr(), stats.data_ptr(), None) == 0
    torch.cuda.synchronize()
    assert torch.equal(A2, A)
    worst = cs.check_inorm(case, Y, gamma, beta, 0.01, A, stats, G, gY, gg, gb)
    for a, b in zip(call(), (A, gY, gg, gb)):
        assert torch.equal(a, b)
    print("ESTNORM inorm_lrelu parts", {k: round(v, 3) for k, v in worst.items()})
    print(f"ESTNORM inorm_lrelu case={cs.case_id(case)} worst={max(worst.values()):.3f}")
    assert max(worst.values()) <= nref.TOL


@pytest.mark.parametrize("N", cs.INORM_REFUSED)
def test_inorm_lrelu_refuses_rows_it_cannot_hold(dfepe, N):
    with pytest.raises(dfepe.DfepeError):
        dfepe.ops.inorm_lrelu(torch.zeros(4, 2, N, device=DEV), torch.ones(4, device=DEV), torch.zeros(4, device=DEV))


def test_native_fp32_stack_forward_and_backward_at_200_points(dfepe):
    """FusedErrorEstimator with split_bf16 = False (channel-major fp32 GEMMs + inorm_lrelu, its NV = 4 template at N = 200) against the
    stock module in float64, forward and backward.  The guard and the classes are test_whole_estimator_at_other_point_counts' (tests/
    test_estimator_mfma_gpu.py), set there for the two-plane stack, which keeps fewer digits than this one: logits to 1e-5; every
    gradient to 1e-4 of its norm when the float64 run keeps each pre-activation 2e-6 away from the LeakyReLU kink, 2e-3 otherwise."""
    cin, B, N = 7, 3, 200
    EE = dfepe.compat.ErrorEstimators
    stock = EE.ErrorEstimator(cin)
    dfepe.synth.fill_params_deterministic(stock, seed=9)
    fused = EE.FusedErrorEstimator(cin).to(DEV)
    fused.load_state_dict(stock.state_dict())
    fused.split_bf16 = False
    stock = stock.double()
    margin = [float("inf")]
    hooks = [m.register_forward_hook(lambda _m, _i, o: margin.__setitem__(0, min(margin[0], float(o.abs().min()))))
             for m in stock.fw if isinstance(m, torch.nn.InstanceNorm1d)]
    g = torch.Generator().manual_seed(N)
    x = torch.rand(B, cin, N, generator=g)
    G = torch.randn(B, 1, N, generator=g)
    xa = x.double().requires_grad_(True)
    xb = x.to(DEV).requires_grad_(True)
    ya = stock(xa)
    for h in hooks:
        h.remove()
    yb = fused(xb)
    assert yb.shape == (B, 1, N) and not type(yb.grad_fn).__name__.startswith("_Estimator")  # the native-fp32 path, not the planes'
    assert float((yb.detach().cpu().double() - ya.detach()).abs().max()) < 1e-5
    (ya * G.double()).sum().backward()
    (yb * G.to(DEV)).sum().backward()
    strict = margin[0] > 2e-6
    pa, pb = dict(stock.named_parameters()), dict(fused.named_parameters())
    for name, got, want in [("input", xb.grad.cpu().double(), xa.grad)] + [(n, pb[n].grad.cpu().double(), pa[n].grad) for n in pa]:
        if float(want.norm()) < 1e-9:  # biases that cancel in an InstanceNorm
            assert float(got.abs().max()) < 1e-6, name
            continue
        err = float((got - want).norm() / want.norm())
        assert err < (1e-4 if strict else 2e-3), (name, err, margin[0])
