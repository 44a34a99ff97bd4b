"""Helpers and fp64 references shared by the VisualLoss tests (tests/test_visual_loss_cpu.py, test_gpu_conv3_exact.py,
test_gpu_vgg_ops.py, test_gpu_visual_loss.py, test_gpu_visual_loss_trainer.py).  Nothing here calls the code under
test: seeded operand makers, layout helpers, error bounds, and a rounding-point emulation of the bf16 chain."""
import functools

import torch
import torch.nn as nn
import torch.nn.functional as F

F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16
EPS32 = 2.0 ** -23
MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)
QUARTER = (16, 32, 64, 128)  # cfg E at 1/4 width


def rne_bf16(t):
    """Round-to-nearest-even to bf16 of an fp64 / fp32 tensor, returned in fp64 (through fp32: the values used here
    are either exact in fp32 or the double rounding is inside the bounds that use it)."""
    return t.to(F32).to(BF16).to(F64)


def round_bound(ref, mag, K):
    """fp32 accumulation of K products (+ bias) in any order, then one rounding to bf16: with
    d = (K + 8) * 2^-23 * mag (mag = sum |a||w| + |b|), |error| <= d + (|ref| + d) * 2^-8 * 1.001
    (round_bound of tests/test_gpu_instance_norm.py)."""
    d = (K + 8) * EPS32 * mag
    return d + (ref.abs() + d) * 2.0 ** -8 * 1.001


def nchw_to_nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def nhwc_to_nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


# ---------------------------------------------------------------- seeded random VGG weights
def seed_features(seq, seed):
    """He-scaled conv weights N(0, 2/(9 Cin)), bias N(0, 0.1^2), BN gamma in [0.5, 1.5], beta N(0, 0.2^2),
    running_mean N(0, 0.2^2), running_var in [0.5, 1.5]: activations stay O(1) through 12 layers."""
    g = torch.Generator().manual_seed(int(seed))
    with torch.no_grad():
        for m in seq:
            if isinstance(m, nn.Conv2d):
                m.weight.copy_(torch.randn(m.weight.shape, generator=g) * (2.0 / (9 * m.in_channels)) ** 0.5)
                if m.bias is not None:
                    m.bias.copy_(torch.randn(m.bias.shape, generator=g) * 0.1)
            elif isinstance(m, nn.BatchNorm2d):
                m.weight.copy_(torch.rand(m.weight.shape, generator=g) + 0.5)
                m.bias.copy_(torch.randn(m.bias.shape, generator=g) * 0.2)
                m.running_mean.copy_(torch.randn(m.running_mean.shape, generator=g) * 0.2)
                m.running_var.copy_(torch.rand(m.running_var.shape, generator=g) + 0.5)
    return seq


def images(shape, seed):
    """Smooth-ish fp32 images in the tanh range (-1, 1)."""
    g = torch.Generator().manual_seed(int(seed))
    return torch.tanh(torch.randn(shape, generator=g)).float()


def fold64(seq):
    """Per conv (w' fp64, b' fp64) by the fp64 formula s = gamma / sqrt(running_var + eps), w' = w s,
    b' = (b - running_mean) s + beta, with the |terms| of b' (for the fp32 bound)."""
    out, mods, i = [], list(seq), 0
    while i < len(mods):
        m = mods[i]
        if isinstance(m, nn.Conv2d):
            w = m.weight.detach().to(F64)
            b = m.bias.detach().to(F64) if m.bias is not None else torch.zeros(w.shape[0], dtype=F64)
            babs = b.abs()
            if i + 1 < len(mods) and isinstance(mods[i + 1], nn.BatchNorm2d):
                bn = mods[i + 1]
                s = bn.weight.detach().to(F64) / torch.sqrt(bn.running_var.detach().to(F64) + bn.eps)
                w = w * s[:, None, None, None]
                rm = bn.running_mean.detach().to(F64)
                babs = (b.abs() + rm.abs()) * s.abs() + bn.bias.detach().to(F64).abs()
                b = (b - rm) * s + bn.bias.detach().to(F64)
            out.append((w, b, babs))
        i += 1
    return out


def normalise64(y):
    """((y * 0.5 + 0.5) - mean) / std of an fp32 / fp64 NCHW image, in fp64."""
    y = y.to(F64)
    mean = torch.tensor(MEAN, dtype=F64)[None, :, None, None]
    std = torch.tensor(STD, dtype=F64)[None, :, None, None]
    return ((y * 0.5 + 0.5) - mean) / std


def structure(seq):
    """[("conv", k) | ("pool",)] of a Sequential of the VisualLoss grammar (k = conv index)."""
    out, k = [], 0
    for m in seq:
        if isinstance(m, nn.Conv2d):
            out.append(("conv", k))
            k += 1
        elif isinstance(m, nn.MaxPool2d):
            out.append(("pool",))
    return out


def reference64(seq, y_pred, y_target):
    """The fp64 torch.nn reference: the same Sequential in fp64 (eval mode), F.mse_loss.  Returns (loss, gradient
    with respect to y_pred, the pred feature map)."""
    import copy
    ref = copy.deepcopy(seq).double().eval()
    mean = torch.tensor(MEAN, dtype=F64)[None, :, None, None]
    std = torch.tensor(STD, dtype=F64)[None, :, None, None]
    yp = y_pred.detach().to(F64).clone().requires_grad_(True)
    fp = ref(((yp * 0.5 + 0.5) - mean) / std)
    with torch.no_grad():
        ft = ref(((y_target.to(F64) * 0.5 + 0.5) - mean) / std)
    loss = F.mse_loss(fp, ft)
    (g,) = torch.autograd.grad(loss, yp)
    return loss.detach(), g, fp.detach()


def emulate(seq, y_pred, y_target, sums=F64):
    """Rounding-point emulation of the bf16 chain, a reference-only computation: sums in ``sums`` precision (fp64 or
    fp32) with bf16 roundings at the documented points -- the normalised input, the folded weights, each
    conv+bias+ReLU output, each pool output (exact), g = 2 (f_p - f_t) / N, each input-gradient conv output after the
    ReLU mask -- and the fp32 output gradient g0 * 0.5 / std.  Returns (loss, gradient)."""
    fold = fold64(seq)
    st = structure(seq)
    wq = [rne_bf16(w).to(sums) for w, _, _ in fold]
    bq = [b.to(F32).to(sums) for _, b, _ in fold]

    def chain(y, keep):
        x = rne_bf16(normalise64(y).to(F32)).to(sums)
        saved = []
        for it in st:
            if it[0] == "conv":
                saved.append(("conv", it[1], x))
                x = rne_bf16(torch.relu(F.conv2d(x, wq[it[1]], bq[it[1]], 1, 1))).to(sums)
            else:
                saved.append(("pool", None, x))
                x = F.max_pool2d(x, 2, 2)
        return (x, saved) if keep else x

    fp, saved = chain(y_pred, True)
    ft = chain(y_target, False)
    d = (fp - ft).to(F64)
    loss = (d * d).mean()
    g = rne_bf16(2.0 * d / d.numel()).to(sums)
    g = g * (fp > 0)
    for kind, k, x in reversed(saved):
        if kind == "pool":
            xx = x.clone().requires_grad_(True)
            (g,) = torch.autograd.grad(F.max_pool2d(xx, 2, 2), xx, g)
        else:
            g = F.conv_transpose2d(g, wq[k], None, 1, 1)
            if k > 0:
                g = g * (x > 0)
            g = rne_bf16(g).to(sums)
    k = torch.tensor([float(torch.tensor(0.5 / s, dtype=F32)) for s in STD], dtype=F64)[None, :, None, None]
    return loss, (g.to(F64) * k)


def rel_l2(a, b):
    return float((a.to(F64) - b.to(F64)).norm() / b.to(F64).norm())


# ---------------------------------------------------------------- NaN-surrounded device buffers
class Boxed:
    """An NHWC bf16 device tensor [B, H, W, C] placed inside a NaN-filled buffer [B, H + 2, W + 2, C + extra] at
    pixel offset (1, 1) and channel offset ``co`` (0 <= co <= extra, multiple of 8), with the stc_view that addresses
    it in place."""

    def __init__(self, B, H, W, C, co=8, extra=16, device="cuda", value=None):
        from stcgan_amd import _lib as L
        self.shape = (B, H, W, C)
        self.co = co
        Cw = C + extra
        self.buf = torch.full((B, H + 2, W + 2, Cw), float("nan"), dtype=BF16, device=device)
        if value is not None:
            self.inner().copy_(value.to(device=device, dtype=BF16))
        p = self.buf.data_ptr() + ((W + 2) * Cw + Cw) * 2
        self.view = L.View(p, H, W, (H + 2) * (W + 2) * Cw, (W + 2) * Cw, Cw, co, 1, 0)
        self.view._keep = self.buf

    def inner(self):
        B, H, W, C = self.shape
        return self.buf[:, 1:H + 1, 1:W + 1, self.co:self.co + C]

    def surroundings_untouched(self):
        """Every element outside the view is still NaN."""
        B, H, W, C = self.shape
        keep = torch.ones_like(self.buf, dtype=torch.bool)
        keep[:, 1:H + 1, 1:W + 1, self.co:self.co + C] = False
        return bool(torch.isnan(self.buf[keep]).all())


@functools.lru_cache(maxsize=None)
def quarter_vgg(seed=7):
    """cfg E at 1/4 width ([:40], ending with pool4) with seeded random weights.  Cached: never modify it."""
    from stcgan_amd.loss import vgg19_bn_features
    return seed_features(vgg19_bn_features(widths=QUARTER), seed)
