"""The VisualLoss kernels around the convolutions (csrc/vgg.hip): MaxPool2d(2, 2) forward / backward, the input
normalisation and its backward, the feature MSE and its gradient -- each against an fp64 / torch CPU reference, with
bounds derived from the number formats (nothing comes from what the kernels return)."""
import pytest
import torch
import torch.nn.functional as F

from visual_ref import BF16, EPS32, F32, F64, MEAN, STD, nchw_to_nhwc, nhwc_to_nchw, normalise64

pytestmark = pytest.mark.gpu


def relu_like(shape, seed):
    """Multiples of 1/4 in [-2, 2], about 40 % zeros (as after a ReLU): exact in bf16, many tied windows."""
    g = torch.Generator().manual_seed(seed)
    v = torch.randint(-8, 9, shape, generator=g).to(F32) / 4
    return torch.where(torch.rand(shape, generator=g) < 0.4, torch.zeros(()), v)


@pytest.mark.parametrize("shape", [(1, 2, 2, 8), (3, 6, 10, 24), (2, 32, 32, 64)], ids=str)
def test_maxpool_forward_backward_exact(shape):
    """Bit-exact against F.max_pool2d and its autograd on the CPU, on the same bf16 values; >= 10 % of the windows have
    a tied maximum (asserted from the input alone), so the first-maximum rule decides the gradient's position."""
    from stcgan_amd import ops
    B, H, W, C = shape
    x = relu_like((B, C, H, W), 11)
    win = F.unfold(x.reshape(B * C, 1, H, W), 2, stride=2)  # [B*C, 4, windows]
    tied = ((win == win.amax(1, keepdim=True)).sum(1) > 1).double().mean()
    assert tied >= 0.10, tied
    xr = x.clone().requires_grad_(True)
    y_ref = F.max_pool2d(xr, 2, 2)
    g = torch.Generator().manual_seed(12)
    gy = (torch.randint(-8, 9, y_ref.shape, generator=g).to(F32) / 8)
    (gx_ref,) = torch.autograd.grad(y_ref, xr, gy)
    xd = nchw_to_nhwc(x).to(device="cuda", dtype=BF16)
    y = ops.maxpool2(xd)
    gx = ops.maxpool2_backward(xd, nchw_to_nhwc(gy).to(device="cuda", dtype=BF16))
    assert torch.equal(nhwc_to_nchw(y.cpu().float()), y_ref.detach())
    assert torch.equal(nhwc_to_nchw(gx.cpu().float()), gx_ref)


def _norm_inputs():
    g = torch.Generator().manual_seed(21)
    dense = torch.rand((2, 3, 6, 10), generator=g) * 2 - 1
    mask = torch.rand((2, 1, 6, 10), generator=g) * 2 - 1
    cl = (torch.rand((2, 6, 10, 3), generator=g) * 2 - 1)
    return {"dense": lambda d: dense.to(d), "expanded": lambda d: mask.to(d).expand(-1, 3, -1, -1),
            "channels_last": lambda d: cl.to(d).permute(0, 3, 1, 2)}


@pytest.mark.parametrize("kind", ["dense", "expanded", "channels_last"])
def test_normalise_forward(kind):
    """Within the bf16 half-ulp of the fp64 value (at most 2^-8 relative: 8 significant bits) plus 4 * 2^-23
    relative; a stride-0 expanded [B, 1, H, W] input and a channels-last-strided one are read in place."""
    from stcgan_amd import ops
    src = _norm_inputs()[kind]("cuda")
    if kind == "expanded":
        assert src.stride(1) == 0
    if kind == "channels_last":
        assert src.stride(1) == 1
    B, _, H, W = src.shape
    dst = torch.full((B, H, W, 8), float("nan"), dtype=BF16, device="cuda")
    ops.vgg_normalise(src, dst)
    ref = nchw_to_nhwc(normalise64(src.cpu()))
    out = dst.cpu().double()
    assert not out[..., 3:].any()
    err = (out[..., :3] - ref).abs()
    bound = ref.abs() * (2.0 ** -8 * 1.001 + 4 * EPS32) + 2.0 ** -133
    print(f"normalise {kind}: worst error/bound {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all())


def test_normalise_backward():
    """g * 0.5 / std_c, exact to 2 * 2^-23 relative."""
    from stcgan_amd import ops
    g = torch.Generator().manual_seed(22)
    gv = torch.randn((2, 5, 7, 8), generator=g).to(BF16)
    out = ops.vgg_normalise_backward(gv.cuda()).cpu().double()
    assert out.shape == (2, 3, 5, 7) and out.is_contiguous()
    k = torch.tensor([0.5 / s for s in STD], dtype=F64)[None, :, None, None]
    ref = nhwc_to_nchw(gv.double()[..., :3]) * k
    assert bool(((out - ref).abs() <= 2 * EPS32 * ref.abs()).all())


@pytest.mark.parametrize("n", [8, 4096 + 8, 2 * 128 * 4 * 4], ids=str)
def test_feature_mse(n):
    """Value within (m + 8) * 2^-23 * sum(terms) / N with m = stc_feat_mse_chain() (the longest chain of fp32 additions
    the kernel documents); gradient = the RNE of fp64 gout * 2 d / N to within one fp32 rounding before it; the same
    call twice and on a side stream is bit-identical."""
    from stcgan_amd import _lib as L, ops
    g = torch.Generator().manual_seed(30 + n % 7)
    fp = torch.relu(torch.randn(n, generator=g)).to(BF16)
    ft = torch.relu(torch.randn(n, generator=g)).to(BF16)
    gout = torch.tensor(0.37, dtype=F32)
    fpd, ftd, goutd = fp.cuda(), ft.cuda(), gout.cuda()
    m = L.lib().stc_feat_mse_chain()
    assert 1 <= m <= 64
    val = ops.feature_mse(fpd, ftd)
    grad = ops.feature_mse_backward(fpd, ftd, goutd)
    d = fp.double() - ft.double()
    terms = d * d
    ref = terms.sum() / n
    assert val.dtype == F32 and val.dim() == 0
    assert abs(float(val.double().cpu()) - float(ref)) <= (m + 8) * EPS32 * float(terms.sum()) / n
    gref = float(gout) * 2.0 * d / n
    lo = (gref * (1 - EPS32)).to(F32).to(BF16)
    hi = (gref * (1 + EPS32)).to(F32).to(BF16)
    mid = gref.to(F32).to(BF16)
    gc = grad.cpu()
    assert bool(((gc == mid) | (gc == lo) | (gc == hi)).all())
    masked = ops.feature_mse_backward(fpd, ftd, goutd, relu_mask=True).cpu()
    assert torch.equal(masked.float(), torch.where(fp.float() > 0, gc.float(), torch.zeros(())))
    # bit-identical twice and on a side stream
    val2, grad2 = ops.feature_mse(fpd, ftd), ops.feature_mse_backward(fpd, ftd, goutd)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        val3, grad3 = ops.feature_mse(fpd, ftd), ops.feature_mse_backward(fpd, ftd, goutd)
    torch.cuda.current_stream().wait_stream(side)
    for a, b in ((val, val2), (val, val3)):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    for a, b in ((grad, grad2), (grad, grad3)):
        assert torch.equal(a.view(torch.int16), b.view(torch.int16))
