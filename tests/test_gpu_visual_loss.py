"""VisualLoss on the GPU: cfg E at 1/4 width (vgg19_bn_features(widths=(16, 32, 64, 128)), [:40]) with seeded random
weights at B = 2, 64 x 64 and 32 x 96, and a no-BatchNorm Sequential of two convs and a pool at 16 x 16.

Layer-wise (the discriminating check): every tensor one call stored (loss.TRACE) against an fp64 computation from
the STORED input of that step -- conv outputs and input-gradient conv outputs within round_bound (fp32 accumulation
of K products in any order, one bf16 rounding), pools and pool gradients exactly, the normalise and MSE steps as in
tests/test_gpu_vgg_ops.py.  End to end (guards the wiring): against the fp64 torch.nn reference, with the error of a
rounding-point emulation (visual_ref.emulate, reference-only) as the yardstick."""
import functools

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from visual_ref import (BF16, EPS32, F32, F64, STD, emulate, images, nchw_to_nhwc, nhwc_to_nchw, normalise64,
                        quarter_vgg, reference64, rel_l2, rne_bf16, round_bound, seed_features)

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def small_seq():
    return seed_features(nn.Sequential(nn.Conv2d(3, 16, 3, padding=1), nn.ReLU(), nn.Conv2d(16, 24, 3, padding=1, bias=False),
                                       nn.ReLU(), nn.MaxPool2d(2, 2)), 5).requires_grad_(False).eval()


CASES = {"q64": (quarter_vgg, (2, 3, 64, 64)), "q32x96": (quarter_vgg, (2, 3, 32, 96)), "small16": (small_seq, (2, 3, 16, 16))}


@functools.lru_cache(maxsize=None)
def module(name):
    from stcgan_amd.loss import VisualLoss
    return VisualLoss(CASES[name][0]())


@functools.lru_cache(maxsize=None)
def inputs(name):
    shape = CASES[name][1]
    return images(shape, 100), images(shape, 101)


@functools.lru_cache(maxsize=None)
def refs(name):
    """(fp64 loss, fp64 gradient, E_loss, E_grad, rms of the last fp64 feature map) -- computed once, never modified."""
    seq = CASES[name][0]()
    yp, yt = inputs(name)
    loss, grad, feat = reference64(seq, yp, yt)
    el, eg = emulate(seq, yp, yt)
    rms = float(feat.pow(2).mean().sqrt())
    assert 0.05 <= rms <= 20, rms  # (from the fp64 reference alone: the seeded weights keep activations O(1))
    return loss, grad, abs(float(el - loss)) / float(loss), rel_l2(eg, grad), rms


def run_traced(name):
    from stcgan_amd import loss as LS
    yp, yt = inputs(name)
    ypd = yp.cuda().requires_grad_(True)
    LS.TRACE = tr = {}
    try:
        out = module(name)(ypd, yt.cuda())
        out.backward()
        torch.cuda.synchronize()
    finally:
        LS.TRACE = None
    return tr, out.detach(), ypd.grad


@pytest.mark.parametrize("name", list(CASES))
def test_layerwise_from_stored_tensors(name):
    """Error/bound per layer is printed (pytest -s).  Measured on an MI355X (profiles/visual_loss/test_ratios.log), worst
    ratios: q64 -- normalise 0.994, conv0..11 0.991 ... 0.807, dgrad11..0 0.799 ... 0.974; q32x96 -- normalise 0.993,
    conv 0.990 ... 0.835, dgrad 0.741 ... 0.986; small16 -- normalise 0.970, conv 0.976, dgrad 0.959 / 0.947.  The
    ratios sit just below 1 because the bound is dominated by the one bf16 rounding, whose error reaches its half-ulp
    somewhere in every tensor; the fp32 accumulation part is a few percent of it.  Pools, pool gradients, the packed
    operands: exact."""
    from stcgan_amd import _lib as L
    mod = module(name)
    tr, loss, grad = run_traced(name)
    yp, yt = inputs(name)
    B = yp.shape[0]
    fold = mod.folded()
    wq = [rne_bf16(w) for w, _ in fold]
    bq = [b.double() for _, b in fold]
    worst = {}

    def ratio(tag, err, bound):
        r = float((err / bound).max())
        worst[tag] = max(worst.get(tag, 0.0), r)
        print(f"{name} {tag}: error/bound {r:.3f}")
        assert r <= 1.0, (tag, r)

    # the normalised input (pred | target batch), channels 3..7 zero
    xin = tr["input"].cpu().double()
    ref = nchw_to_nhwc(normalise64(torch.cat([yp, yt])))
    assert not xin[..., 3:].any()
    ratio("normalise", (xin[..., :3] - ref).abs(), ref.abs() * (2.0 ** -8 * 1.001 + 4 * EPS32) + 2.0 ** -133)
    # the operands as packed
    for k, (pf, pd) in enumerate(tr["packed"]):
        co, ci = wq[k].shape[:2]
        flat = wq[k].reshape(co, ci, 9)
        assert torch.equal(pf.cpu().double()[:co, :, :ci], flat.permute(0, 2, 1))
        assert torch.equal(pd.cpu().double()[:ci, :, :co], flat.flip(2).permute(1, 2, 0))
    # forward chain, each step from its stored input
    prev = tr["input"]
    for i, it in enumerate(tr["items"]):
        x = nhwc_to_nchw(prev.cpu().double())
        y = nhwc_to_nchw(tr["acts"][i].cpu().double())
        if it[0] == "pool":
            assert torch.equal(y, F.max_pool2d(x, 2, 2)), f"pool {i}"
        else:
            k = it[1]
            ci = wq[k].shape[1]
            assert not x[:, ci:].any()
            r = torch.relu(F.conv2d(x[:, :ci], wq[k], bq[k], 1, 1))
            mag = F.conv2d(x[:, :ci].abs(), wq[k].abs(), bq[k].abs(), 1, 1)
            ratio(f"conv{k}", (y - r).abs(), round_bound(r, mag, 9 * ci) + 2.0 ** -133)
        prev = tr["acts"][i]
    # the MSE of the stored features
    f = tr["acts"][-1].cpu().double()
    d = f[:B] - f[B:]
    m = L.lib().stc_feat_mse_chain()
    assert abs(float(tr["loss"].detach().cpu().double()) - float((d * d).mean())) <= (m + 8) * EPS32 * float((d * d).mean())
    gref = 2.0 * d / d.numel() * (f[:B] > 0)
    gf = tr["g_feat"].cpu()
    assert bool(((gf == gref.to(F32).to(BF16)) | (gf == (gref * (1 - EPS32)).to(F32).to(BF16))
                 | (gf == (gref * (1 + EPS32)).to(F32).to(BF16))).all())
    # backward chain, each step from its stored incoming gradient and stored mask / pool input
    n = len(tr["items"])
    for i in reversed(range(n)):
        gin = nhwc_to_nchw((tr["grads"][i + 1] if i + 1 < n else tr["g_feat"]).cpu().double())
        got = nhwc_to_nchw(tr["grads"][i].cpu().double())
        x = nhwc_to_nchw((tr["acts"][i - 1] if i > 0 else tr["input"]).cpu().double())[:B]
        if tr["items"][i][0] == "pool":
            xx = x.clone().requires_grad_(True)
            (want,) = torch.autograd.grad(F.max_pool2d(xx, 2, 2), xx, gin)
            assert torch.equal(got, want), f"pool gradient {i}"
        else:
            k = tr["items"][i][1]
            co, ci = wq[k].shape[:2]
            mask = (x[:, :ci] > 0) if i > 0 else torch.ones_like(x[:, :ci], dtype=torch.bool)
            r = F.conv_transpose2d(gin[:, :co], wq[k], None, 1, 1) * mask
            mag = F.conv_transpose2d(gin[:, :co].abs(), wq[k].abs(), None, 1, 1) * mask
            assert not got[:, ci:].any()
            ratio(f"dgrad{k}", (got[:, :ci] - r).abs(), round_bound(r, mag, 9 * co) + 2.0 ** -140)
    # the fp32 gradient of the input
    g0 = nhwc_to_nchw(tr["grads"][0].cpu().double())[:, :3]
    kk = torch.tensor([0.5 / s for s in STD], dtype=F64)[None, :, None, None]
    assert bool(((tr["g_input"].cpu().double() - g0 * kk).abs() <= 2 * EPS32 * (g0 * kk).abs()).all())
    assert torch.equal(tr["g_input"], grad)
    print(f"{name} worst ratios: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


@pytest.mark.parametrize("name", list(CASES))
def test_end_to_end_against_fp64(name):
    """Loss within 3 x (the largest emulation loss error of the file's cases), gradient relative L2 within 1.5 x the
    emulation's of this case; the measured values are printed (pytest -s) and kept in profiles/visual_loss/.
    Measured on an MI355X: q64 -- loss 3.6e-4 of fp64 (emulation 5.1e-4; 3 x file max = 1.2e-2: ratio 0.030), gradient
    relative L2 0.3318 (emulation 0.3320: ratio 0.666 to 1.5 x); q32x96 -- loss 3.0e-3 (emulation 3.9e-3, ratio 0.258),
    gradient 0.2759 (0.2776, 0.663); small16 -- loss 1.2e-5 (1.2e-5, 0.001), gradient 0.0591 (0.0591, 0.667)."""
    ref_loss, ref_grad, _, e_grad, rms = refs(name)
    e_loss_max = max(refs(n)[2] for n in CASES)
    yp, yt = inputs(name)
    ypd = yp.cuda().requires_grad_(True)
    out = module(name)(ypd, yt.cuda())
    out.backward()
    assert out.dtype == F32 and out.dim() == 0
    k_loss = abs(float(out.detach().double().cpu()) - float(ref_loss)) / float(ref_loss)
    k_grad = rel_l2(ypd.grad.cpu(), ref_grad)
    print(f"{name}: feature rms {rms:.3f}; loss rel err {k_loss:.3e} (emulation {refs(name)[2]:.3e}, file max "
          f"{e_loss_max:.3e}, ratio to 3 x max {k_loss / (3 * e_loss_max):.3f}); gradient rel L2 {k_grad:.4f} "
          f"(emulation {e_grad:.4f}, ratio to 1.5 x {k_grad / (1.5 * e_grad):.3f})")
    assert k_loss <= 3 * e_loss_max
    assert k_grad <= 1.5 * e_grad


def test_expanded_mask_form_and_target_gradient():
    """vis1: a [B, 1, H, W] prediction expanded to 3 channels (stride 0, read in place) receives the channel sum of the
    3-channel gradient of the materialised input, bit for bit; the target never receives a gradient."""
    mod = module("small16")
    g = torch.Generator().manual_seed(3)
    mp = torch.tanh(torch.randn((2, 1, 16, 16), generator=g)).cuda().requires_grad_(True)
    mt = torch.tanh(torch.randn((2, 1, 16, 16), generator=g)).cuda().requires_grad_(True)
    l1 = mod(mp.expand(-1, 3, -1, -1), mt.expand(-1, 3, -1, -1))
    l1.backward()
    assert mt.grad is None and mp.grad.shape == (2, 1, 16, 16)
    full = mp.detach().expand(-1, 3, -1, -1).contiguous().requires_grad_(True)
    l2 = mod(full, mt.detach().expand(-1, 3, -1, -1).contiguous())
    l2.backward()
    assert torch.equal(l1.detach(), l2.detach())
    assert torch.equal(mp.grad, full.grad.sum(dim=1, keepdim=True))


def test_no_grad_repeat_and_side_stream_bit_identical():
    mod = module("q64")
    yp, yt = (t.cuda() for t in inputs("q64"))

    def call():
        p = yp.clone().requires_grad_(True)
        out = mod(p, yt)
        out.backward()
        return out.detach(), p.grad

    l1, g1 = call()
    l2, g2 = call()
    with torch.no_grad():
        l0 = mod(yp, yt)
    l00 = mod(yp, yt)  # (grad enabled, nothing requires it)
    assert not l0.requires_grad and not l00.requires_grad
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        l3, g3 = call()
    torch.cuda.current_stream().wait_stream(side)
    for a in (l2, l0, l00, l3):
        assert torch.equal(l1.view(torch.int32), a.view(torch.int32))
    for a in (g2, g3):
        assert torch.equal(g1.view(torch.int32), a.view(torch.int32))


def test_indivisible_size_raises_before_any_launch():
    mod = module("q64")
    x = torch.zeros((1, 3, 40, 64), device="cuda")
    with pytest.raises(ValueError, match="divisible by 16"):
        mod(x, x)
    with pytest.raises(ValueError, match="divisible by 16"):
        mod(x.transpose(2, 3), x.transpose(2, 3))
