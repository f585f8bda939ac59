"""The PPO update's fused backward kernels with the Tanh activation (HS_ACT_TANH): hs_dgrad_act
(ppo_mlp.hip dgrad_mask_*_kernel<.., ACT>: input gradient times 1 - x^2 with the bias sum's first pass),
hs_act_grad_colsum (relu_colsum_kernel<ACT>) and the autograd nodes built on them (_MLPChainFn,
_SplitKLinearReLUFn), against float64 formulas and plain torch autograd at the bars of their ReLU
counterparts in tests/test_gpu_ppo.py."""
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("B,K", [(100, 256), (10000, 256), (37, 21), (5, 1)])
def test_dgrad_act_tanh_matches_float64(B, K):
    """hs_dgrad_act with HS_ACT_TANH == (g @ w) * (1 - x^2) in float64 at test_dgrad_mask_matches_torch's
    bar, 1e-5 (1 + max |ref|) elementwise, and its column sums through colsum_pair: the MFMA instance
    with a partial tile (100 rows) and with two row blocks plus a partial (10000), the VALU head
    instances (21 actions, 1 value) with ragged rows.  Where x is exactly +-1 the gradient is exactly 0."""
    from mujocoposelearning_amd._lib import HS_ACT_TANH
    from mujocoposelearning_amd.ppo_ops import colsum_pair, dgrad_mask
    gen = torch.Generator(device="cuda").manual_seed(B + K)
    g = torch.randn(B, K, device="cuda", generator=gen)
    w = torch.randn(K, 256, device="cuda", generator=gen) * 0.06
    x = torch.tanh(torch.randn(B, 256, device="cuda", generator=gen))
    sat = [(0, 0, 1.0), (B - 1, 255, -1.0), (B // 2, 17, 1.0), (B // 3, 130, -1.0)]
    for r, c, v in sat:
        x[r, c] = v
    gx, part = dgrad_mask(g, w, x, act=HS_ACT_TANH)
    ref = (g.double() @ w.double()) * (1 - x.double() ** 2)
    tol = 1e-5 * (1 + float(ref.abs().max()))
    err = float((gx.double() - ref).abs().max())
    print(f"B {B} K {K}: max |gx - ref| {err:.3e}, bar {tol:.3e}")
    assert err < tol
    for r, c, _ in sat:
        assert float(gx[r, c]) == 0.0, (r, c)
    _, s1 = colsum_pair(torch.zeros(1, 1, device="cuda"), part)
    assert torch.allclose(s1.double(), ref.sum(0), rtol=1e-5, atol=tol * B ** 0.5)
    # the activation is selected, not ignored: the ReLU result on the same operands differs
    gr, _ = dgrad_mask(g, w, x)
    assert torch.equal(gr, torch.where(x > 0, gr, torch.zeros_like(gr))) and not torch.equal(gr, gx)


def test_dgrad_act_tanh_unaligned_operands():
    """hs_dgrad_act (Tanh) on X and W views one float into wider rows, as test_dgrad_mask_unaligned_operands:
    the element-load instance gives bitwise the aligned call's results."""
    from mujocoposelearning_amd._lib import HS_ACT_TANH
    from mujocoposelearning_amd.ppo_ops import dgrad_mask
    gen = torch.Generator(device="cuda").manual_seed(256)
    B, K = 3000, 256
    g = torch.randn(B, K, device="cuda", generator=gen)
    w = (torch.randn(K, 261, device="cuda", generator=gen) * 0.06)[:, 1:257]
    x = torch.tanh(torch.randn(B, 259, device="cuda", generator=gen))[:, 3:259]
    gx, part = dgrad_mask(g, w, x, act=HS_ACT_TANH)
    ga, pa = dgrad_mask(g, w.contiguous(), x.contiguous(), act=HS_ACT_TANH)
    ref = (g.double() @ w.double()) * (1 - x.double() ** 2)
    assert float((gx.double() - ref).abs().max()) < 1e-5 * (1 + float(ref.abs().max()))
    assert torch.equal(gx, ga) and torch.equal(part, pa)


@pytest.mark.parametrize("rows,cols", [(4096, 64), (100, 7)])
def test_act_grad_colsum_tanh(rows, cols):
    """hs_act_grad_colsum with HS_ACT_TANH: |gm - g (1 - y^2)| in float64 <= 1e-6 (1 + max |g|) (three
    fp32 roundings, ~1.8e-7 relative to |g|, times five), and the partial sums finished by colsum_pair
    at the bar of test_relu_grad_colsum_and_pair."""
    from mujocoposelearning_amd._lib import HS_ACT_TANH
    from mujocoposelearning_amd.ppo_ops import colsum_pair, relu_grad_colsum
    gen = torch.Generator(device="cuda").manual_seed(rows + cols)
    g = torch.randn(rows, cols, device="cuda", generator=gen)
    y = torch.tanh(torch.randn(rows, cols, device="cuda", generator=gen))
    gm, part = relu_grad_colsum(g, y, act=HS_ACT_TANH)
    ref = g.double() * (1 - y.double() ** 2)
    err = float((gm.double() - ref).abs().max())
    print(f"rows {rows} cols {cols}: max |gm - ref| {err:.3e}")
    assert err <= 1e-6 * (1 + float(g.abs().max()))
    p2 = torch.randn(16, 3 * cols, device="cuda", generator=gen)
    s0, s1 = colsum_pair(p2, part)
    assert torch.allclose(s0, p2.double().sum(0).float(), rtol=1e-5, atol=1e-5)
    assert torch.allclose(s1, ref.sum(0).float(), rtol=1e-5, atol=1e-5 * rows ** 0.5)


@pytest.mark.parametrize("depth", [1, 2])
def test_mlp_chain_node_tanh_gradients_match_autograd(depth):
    """_MLPChainFn with Tanh == plain torch.tanh(F.linear(...)) autograd on the same parameters: outputs,
    every parameter gradient and the input gradient at the bar of
    test_mlp_chain_node_gradients_match_autograd, at the smallest batch that takes the node."""
    from mujocoposelearning_amd import ppo_ops as O
    F = torch.nn.functional
    torch.manual_seed(13 + depth)
    B, D = 2 * O._SPLITK_ROWS, 352
    for A, need_gx in ((21, False), (1, True)):
        mods = []
        for li in range(depth):
            mods += [O.Linear(D if li == 0 else 256, 256), torch.nn.Tanh()]
        seq = torch.nn.Sequential(*mods).cuda()
        head = O.Linear(256, A).cuda()
        params = list(seq.parameters()) + list(head.parameters())
        x = torch.randn(B, D, device="cuda", requires_grad=need_gx)
        gout = torch.randn(B, A, device="cuda")
        res = {}
        for fused in (True, False):
            for p in params:
                p.grad = None
            x.grad = None
            with torch.enable_grad():
                if fused:
                    out = O.mlp_head_forward(seq, head, x)
                    assert "MLPChainFn" in type(out.grad_fn).__name__, type(out.grad_fn).__name__
                else:
                    h = x
                    for m in seq[0::2]:
                        h = torch.tanh(F.linear(h, m.weight, m.bias))
                    out = F.linear(h, head.weight, head.bias)
                out.backward(gout)
            res[fused] = [out.detach()] + [p.grad.clone() for p in params]
            if need_gx:
                res[fused].append(x.grad.clone())
        for a, b in zip(res[True], res[False]):
            assert a.shape == b.shape
            assert torch.allclose(a, b, rtol=1e-4, atol=1e-4 * (1 + float(b.abs().max()))), float((a - b).abs().max())


def test_mlp_forward_tanh_pairs_match_the_modules():
    """mlp_forward on a [64, 64] Tanh Sequential runs each (Linear, Tanh) pair as a _SplitKLinearReLUFn
    node (hs_act_grad_colsum in its backward) and equals the modules' own forward / backward."""
    from mujocoposelearning_amd import ppo_ops as O
    torch.manual_seed(5)
    B, D = 2 * O._SPLITK_ROWS, 352
    seq = torch.nn.Sequential(O.Linear(D, 64), torch.nn.Tanh(), O.Linear(64, 64), torch.nn.Tanh()).cuda()
    params = list(seq.parameters())
    x = torch.randn(B, D, device="cuda", requires_grad=True)
    gout = torch.randn(B, 64, device="cuda")
    res = {}
    for fused in (True, False):
        for p in params:
            p.grad = None
        x.grad = None
        with torch.enable_grad():
            if fused:
                out = O.mlp_forward(seq, x)
                assert "SplitKLinearReLUFn" in type(out.grad_fn).__name__, type(out.grad_fn).__name__
            else:
                h = x
                for m in seq:
                    h = torch.nn.Linear.forward(m, h) if isinstance(m, torch.nn.Linear) else m(h)
                out = h
            out.backward(gout)
        res[fused] = [out.detach()] + [p.grad.clone() for p in params] + [x.grad.clone()]
    for a, b in zip(res[True], res[False]):
        assert a.shape == b.shape
        assert torch.allclose(a, b, rtol=1e-4, atol=1e-4 * (1 + float(b.abs().max()))), float((a - b).abs().max())
