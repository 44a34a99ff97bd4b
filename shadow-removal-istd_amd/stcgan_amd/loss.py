"""Drop-in replacement for the loss modules of STCGAN/loss.py on the ST-CGAN path.

DataLoss (STCGAN/loss.py:14-26) and AdversarialLoss (STCGAN/loss.py:59-86) run as
HIP reduction kernels (deterministic two-level sums) with hand-written gradients.
VisualLoss (src/loss.py:29-56) runs an eval-mode vgg19_bn feature chain in bf16 on the
HIP 3x3 MFMA conv kernels.  SoftAdapt is not on the path.
"""
import ctypes

import torch
import torch.nn as nn

from . import _lib as L
from ._lib import check, lib, ptr, stream


class _LossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, kind, c, pred, target):
        pred = pred.contiguous()
        if pred.dtype != torch.float32:
            raise TypeError("stcgan_amd losses take fp32 inputs")
        if not pred.is_cuda:
            raise RuntimeError("stcgan_amd losses run on the GPU only")
        if target is not None:
            target = target.contiguous()
            if target.shape != pred.shape:
                raise ValueError(f"loss: target shape {tuple(target.shape)} != prediction {tuple(pred.shape)}")
        n = pred.numel()
        part = torch.empty(max(1, lib().stc_loss_parts(n)), dtype=torch.float32, device=pred.device)
        out = torch.empty((), dtype=torch.float32, device=pred.device)
        check(lib().stc_loss_fwd(kind, ptr(pred), ptr(target), float(c), n, ptr(part), ptr(out), stream()),
              "stc_loss_fwd")
        ctx.kind, ctx.c = kind, c
        ctx.save_for_backward(pred, target if target is not None else pred)
        ctx.has_t = target is not None
        return out

    @staticmethod
    def backward(ctx, gout):
        pred, target = ctx.saved_tensors
        t = target if ctx.has_t else None
        grad = torch.empty_like(pred)
        gout = gout.contiguous().float()
        check(lib().stc_loss_bwd(ctx.kind, ptr(pred), ptr(t), float(ctx.c), pred.numel(), ptr(gout), ptr(grad),
                                 stream()), "stc_loss_bwd")
        return None, None, grad, None


def _arr(ctype, vals):
    return (ctype * len(vals))(*vals)


class _ObjectiveFn(torch.autograd.Function):
    """Four loss terms and the scalar arithmetic combining them as one node: two launches forward, one
    backward (stc_loss_multi_*), instead of 4 loss nodes and ~6 torch scalar ops with their own launches
    and autograd nodes.  Values bit-identical to the per-term path (same reductions, same fp32 rounding
    order).  forward -> (objective, parts): parts = the named sub-losses, not differentiable."""

    @staticmethod
    def forward(ctx, mode, kinds, consts, w, wab, *tensors):
        preds = [t.contiguous() for t in tensors[:4]]
        targets = [t.contiguous() if t is not None else None for t in tensors[4:]]
        for p_, t_ in zip(preds, targets):
            if p_.dtype != torch.float32 or not p_.is_cuda:
                raise TypeError("stcgan_amd losses take fp32 CUDA inputs")
            if t_ is not None and t_.shape != p_.shape:
                raise ValueError(f"loss: target shape {tuple(t_.shape)} != prediction {tuple(p_.shape)}")
        dev = preds[0].device
        numels = [p_.numel() for p_ in preds]
        l = lib()
        n_arr = _arr(ctypes.c_int64, numels)
        part = torch.empty(l.stc_loss_multi_parts(4, n_arr), dtype=torch.float32, device=dev)
        vals = torch.empty(6, dtype=torch.float32, device=dev)  # the 4 terms, then D1, D2 (mode D)
        total = torch.empty((), dtype=torch.float32, device=dev)
        args = (4, _arr(ctypes.c_int32, kinds), _arr(ctypes.c_float, consts),
                _arr(ctypes.c_void_p, [p_.data_ptr() for p_ in preds]),
                _arr(ctypes.c_void_p, [t_.data_ptr() if t_ is not None else None for t_ in targets]), n_arr)
        check(l.stc_loss_multi_fwd(*args, mode, _arr(ctypes.c_float, list(w) + [0.0] * (3 - len(w))), ptr(part),
                                   ptr(vals), ptr(total), stream()), "stc_loss_multi_fwd")
        ctx.args, ctx.wab = args, wab
        ctx.save_for_backward(*preds, *[t_ if t_ is not None else preds[0] for t_ in targets])
        ctx.mark_non_differentiable(vals)
        ctx.set_materialize_grads(False)  # no zero-filled gradient for the non-differentiable parts
        return total, vals

    @staticmethod
    def backward(ctx, gout, _gparts):
        if gout is None:
            return (None,) * 13
        preds = ctx.saved_tensors[:4]
        need = ctx.needs_input_grad[5:9]
        grads = [torch.empty_like(p_) if nd else None for p_, nd in zip(preds, need)]
        wa, wb = ctx.wab
        gout = gout.contiguous().float()
        check(lib().stc_loss_multi_bwd(*ctx.args, _arr(ctypes.c_float, wa), _arr(ctypes.c_float, wb), ptr(gout),
                                       _arr(ctypes.c_void_p, [g.data_ptr() if g is not None else None
                                                              for g in grads]), stream()), "stc_loss_multi_bwd")
        return (None,) * 5 + tuple(grads) + (None,) * 4


def d_objective(adv, C1_fake, C1_real, C2_fake, C2_real, lambda2, lambda3):
    """The D objective of STCGAN/stcgan.py:240-251 (loss type "normal"):
    D1 = (adv(C1_fake, fake) + adv(C1_real, real)) * 0.5, D2 likewise, D = lambda2*D1 + lambda3*D2.
    Returns (D, D1, D2)."""
    real, fake = adv._labels
    k = L.LOSS_BCE_CONST if adv.ls else L.LOSS_MSE_CONST
    total, parts = _ObjectiveFn.apply(L.LOSS_COMBINE_D, [k] * 4, [fake, real, fake, real], [lambda2, lambda3],
                                      ([lambda2, lambda2, lambda3, lambda3], [0.5] * 4),
                                      C1_fake, C1_real, C2_fake, C2_real, None, None, None, None)
    return total, parts[4], parts[5]


def d_term_grad(adv, C, lam, gout, real=True):
    """d_objective's gradient with respect to one of its four logits tensors, lam * 0.5 * adv'(C, label) (label: real
    or fake) scaled by the objective's incoming gradient ``gout`` (fp32 device scalar) -- the same per-term kernel
    arithmetic as that node's backward (stc_loss_multi_bwd), available as soon as C is: with loss type normal each
    term involves one logits tensor only, so each discriminator call's backward need not wait for the other calls
    (STCGAN.train_step runs them early; the objective then takes the logits detached)."""
    label = adv._labels[0] if real else adv._labels[1]
    k = L.LOSS_BCE_CONST if adv.ls else L.LOSS_MSE_CONST
    p_ = C.contiguous()
    if p_.dtype != torch.float32 or not p_.is_cuda:
        raise TypeError("stcgan_amd losses take fp32 CUDA inputs")
    g = torch.empty_like(p_)
    check(lib().stc_loss_multi_bwd(1, _arr(ctypes.c_int32, [k]), _arr(ctypes.c_float, [label]),
                                   _arr(ctypes.c_void_p, [p_.data_ptr()]), _arr(ctypes.c_void_p, [None]),
                                   _arr(ctypes.c_int64, [p_.numel()]), _arr(ctypes.c_float, [lam]),
                                   _arr(ctypes.c_float, [0.5]), ptr(gout), _arr(ctypes.c_void_p, [g.data_ptr()]),
                                   stream()), "stc_loss_multi_bwd")
    return g


def g_objective(adv, m_pred, m, y_pred, y, C1_fake, C2_fake, lambda1, lambda2, lambda3):
    """The G objective of STCGAN/stcgan.py:291-299 (loss type "normal"): G1 = adv(C1_fake, real),
    G2 = adv(C2_fake, real), data1 = L1(m_pred, m), data2 = L1(y_pred, y),
    G = data1 + lambda1*data2 + lambda2*G1 + lambda3*G2.  Returns (G, G1, G2, data1, data2)."""
    real = adv._labels[0]
    k = L.LOSS_BCE_CONST if adv.ls else L.LOSS_MSE_CONST
    total, v = _ObjectiveFn.apply(L.LOSS_COMBINE_G, [L.LOSS_L1, L.LOSS_L1, k, k], [0.0, 0.0, real, real],
                                  [lambda1, lambda2, lambda3], ([1.0, lambda1, lambda2, lambda3], [1.0] * 4),
                                  m_pred, y_pred, C1_fake, C2_fake, m, y, None, None)
    return total, v[2], v[3], v[0], v[1]


def l1_loss(pred, target):
    """F.l1_loss(pred, target, reduction='mean')."""
    return _LossFn.apply(L.LOSS_L1, 0.0, pred, target)


def mse_const(pred, value):
    """F.mse_loss(pred, full_like(pred, value))."""
    return _LossFn.apply(L.LOSS_MSE_CONST, float(value), pred, None)


def bce_logits_const(pred, value):
    """F.binary_cross_entropy_with_logits(pred, full_like(pred, value))."""
    return _LossFn.apply(L.LOSS_BCE_CONST, float(value), pred, None)


class DataLoss(nn.Module):
    """Loss between shadow parameters: L1, mean reduction (STCGAN/loss.py:14-26)."""
    __slots__ = ["reduction", "norm"]

    def __init__(self, norm=None, reduction: str = 'mean'):
        super().__init__()
        if reduction != 'mean' or (norm is not None and norm is not torch.nn.functional.l1_loss):
            raise NotImplementedError("stcgan_amd DataLoss: only F.l1_loss with reduction='mean' is on the path")
        self.reduction = reduction

    def forward(self, y_pred, y_target):
        return l1_loss(y_pred, y_target)


class AdversarialLoss(nn.Module):
    """Objective of a conditional GAN (STCGAN/loss.py:59-86).

    ls=False: labels real=1 / fake=0 and F.mse_loss -- the branch the reference
    always takes (its constructor compares against the misspelt 'leastsqure',
    STCGAN/stcgan.py:111-112).  ls=True: labels 1 / -1 and BCE-with-logits,
    exactly as the reference (inverted) branches."""

    def __init__(self, ls=False, rel=False, avg=False):
        super().__init__()
        if not ls:
            self.register_buffer('real_label', torch.tensor(1.0))
            self.register_buffer('fake_label', torch.tensor(0.0))
        else:
            self.register_buffer('real_label', torch.tensor(1.0))
            self.register_buffer('fake_label', torch.tensor(-1.0))
        self.ls = ls
        self.rel = rel
        self.avg = avg
        self._labels = (1.0, -1.0 if ls else 0.0)

    def forward(self, D_out, is_real):
        target = self._labels[0] if is_real else self._labels[1]
        if not self.ls:
            return mse_const(D_out, target)
        return bce_logits_const(D_out, target)


class RelativisticAdversarialLoss(nn.Module):
    """The ``src/`` line's AdversarialLoss (src/loss.py:59-112): SGAN / RpGAN (rel) / RaGAN
    (rel + avg) objectives over a (C_real, C_fake) pair, for the discriminator (``D_loss=True``)
    or the generator; labels real=1, fake=0 (MSE) or 1 / -1 with ``ls=True`` (BCE-with-logits),
    as the reference.  The reductions and their gradients run in the HIP loss kernels; the
    relativistic differences (C_real - C_fake, C - mean over dim 0) are torch ops on the
    [B, 1, 30, 30] logits."""

    def __init__(self, ls=False, rel=False, avg=False):
        super().__init__()
        self.register_buffer('real_label', torch.tensor(1.0))
        self.register_buffer('fake_label', torch.tensor(-1.0 if ls else 0.0))
        self.ls, self.rel, self.avg = ls, rel, avg
        self._labels = (1.0, -1.0 if ls else 0.0)

    def cal_loss(self, C_out, label):
        return bce_logits_const(C_out, label) if self.ls else mse_const(C_out, label)

    def forward(self, C_real, C_fake, D_loss=True):
        real, fake = self._labels
        if self.rel and self.avg:  # RaGAN
            if D_loss:
                return (self.cal_loss(C_real - C_fake.mean(dim=0), real)
                        + self.cal_loss(C_fake - C_real.mean(dim=0), fake)) * 0.5
            return (self.cal_loss(C_real - C_fake.mean(dim=0), fake)
                    + self.cal_loss(C_fake - C_real.mean(dim=0), real)) * 0.5
        if self.rel:  # RpGAN
            return self.cal_loss(C_real - C_fake, real) if D_loss else self.cal_loss(C_fake - C_real, real)
        if D_loss:  # SGAN
            return (self.cal_loss(C_real, real) + self.cal_loss(C_fake, fake)) * 0.5
        return self.cal_loss(C_fake, real)


# ---------------------------------------------------------------------------------------------------------------
# VisualLoss (src/loss.py:29-56 of the reference's src/ line): MSE between the features of an eval-mode vgg19_bn.
# bf16 activations and weights, fp32 accumulation, fp32 loss sums -- also under the fp32-parity trainer.
# Rounding points, in order: the normalised input; the folded weights; each conv+bias+ReLU output; each pool output
# (exact); g = gout * 2 (f_p - f_t) / N; each input-gradient conv output (after the ReLU mask).  The fp32 gradient of
# the input is g0 * 0.5 / std_c.

# When a dict: one VisualLoss call records every tensor it stored (tests; like engine.TRACE).  forward: "input" (the
# normalised pred | target batch, NHWC bf16 [2B, H, W, 8]), "items" (("conv", layer index) / ("pool",) per module
# group), "acts" (each item's output, [2B, ...]), "packed" ([(fwd, dgrad)] per conv as packed), "biases", "loss";
# backward: "g_feat" (the MSE gradient), "grads" (the gradient each item passes to its input, in item order),
# "g_input" (fp32 [B, 3, H, W]).
TRACE = None

_VGG19_WIDTHS = (64, 128, 256, 512)


def vgg19_bn_features(state_dict=None, upto=40, widths=_VGG19_WIDTHS):
    """torchvision's ``vgg19_bn().features[:upto]`` from plain torch.nn (cfg E: convs at 0, 3, 7, 10, 14, 17, 20, 23,
    27, 30, 33, 36, ..., BatchNorm at +1, ReLU at +2, pools at 6, 13, 26, 39, 52; [:40] ends with pool4).
    state_dict: a torchvision vgg19_bn state_dict -- its ``features.N.*`` entries with N < upto are loaded, the
    ``classifier.*`` and later entries ignored.  widths: the four block widths (block 5 has the fourth), for a
    scaled-down network of the same shape."""
    w1, w2, w3, w4 = widths
    cfg = [w1, w1, "M", w2, w2, "M", w3, w3, w3, w3, "M", w4, w4, w4, w4, "M", w4, w4, w4, w4, "M"]
    mods, cin = [], 3
    for v in cfg:
        if v == "M":
            mods.append(nn.MaxPool2d(kernel_size=2, stride=2))
        else:
            mods += [nn.Conv2d(cin, v, kernel_size=3, padding=1), nn.BatchNorm2d(v), nn.ReLU(inplace=True)]
            cin = v
    seq = nn.Sequential(*mods[:upto])
    if state_dict is not None:
        own = seq.state_dict()
        sub = {}
        for k, v in state_dict.items():
            if k.startswith("features.") and k[len("features."):] in own:
                sub[k[len("features."):]] = v
        seq.load_state_dict(sub, strict=True)
    return seq.requires_grad_(False).eval()


def _pad8(c):
    return -(-c // 8) * 8


def _parse_features(features):
    """The Sequential grammar: (Conv2d k3 s1 p1 zeros [BatchNorm2d] ReLU | MaxPool2d(2, 2))*."""
    if not isinstance(features, nn.Sequential):
        raise NotImplementedError(f"stcgan_amd VisualLoss: features must be an nn.Sequential, got {type(features).__name__}")
    mods = list(features)
    items, i, cin = [], 0, 3

    def two(v):
        return tuple(v) if isinstance(v, (tuple, list)) else (v, v)

    while i < len(mods):
        m = mods[i]
        if isinstance(m, nn.MaxPool2d):
            if two(m.kernel_size) != (2, 2) or two(m.stride) != (2, 2) or two(m.padding) != (0, 0) \
                    or two(m.dilation) != (1, 1) or m.ceil_mode or m.return_indices:
                raise NotImplementedError(f"stcgan_amd VisualLoss: only MaxPool2d(2, 2) is on the path, got {m}")
            items.append(("pool",))
            i += 1
            continue
        if isinstance(m, nn.Conv2d):
            if m.kernel_size != (3, 3) or m.stride != (1, 1) or m.padding != (1, 1) or m.dilation != (1, 1) \
                    or m.groups != 1 or m.padding_mode != "zeros" or m.in_channels != cin or m.out_channels % 8 != 0:
                raise NotImplementedError("stcgan_amd VisualLoss: only Conv2d(k=3, s=1, p=1, zero padding) with "
                                          f"{cin} input channels and a multiple of 8 output channels is on the path, got {m}")
            bn = None
            j = i + 1
            if j < len(mods) and isinstance(mods[j], nn.BatchNorm2d):
                bn = mods[j]
                if not bn.track_running_stats or bn.running_mean is None:
                    raise NotImplementedError(f"stcgan_amd VisualLoss: BatchNorm2d needs running statistics, got {bn}")
                j += 1
            if j >= len(mods) or not isinstance(mods[j], nn.ReLU):
                got = mods[j] if j < len(mods) else "the end of the Sequential"
                raise NotImplementedError(f"stcgan_amd VisualLoss: a ReLU must follow {m}, got {got}")
            items.append(("conv", m, bn))
            cin = m.out_channels
            i = j + 1
            continue
        raise NotImplementedError(f"stcgan_amd VisualLoss: module {i} is not on the path: {m}")
    if not any(it[0] == "conv" for it in items):
        raise NotImplementedError("stcgan_amd VisualLoss: features has no Conv2d")
    return items


class _VisualFn(torch.autograd.Function):
    """The whole loss as one node: normalise, the feature chain on the pred | target batch, the MSE."""

    @staticmethod
    def forward(ctx, mod, y_pred, y_target):
        from . import ops
        tr = TRACE if isinstance(TRACE, dict) else None
        if y_pred.dtype != torch.float32 or y_target.dtype != torch.float32 or not y_pred.is_cuda \
                or not y_target.is_cuda:
            raise TypeError("stcgan_amd VisualLoss takes fp32 CUDA inputs")
        if y_pred.dim() != 4 or y_pred.shape[1] != 3 or y_target.shape != y_pred.shape:
            raise ValueError(f"VisualLoss: [B, 3, H, W] inputs of one shape are required, got {tuple(y_pred.shape)} "
                             f"and {tuple(y_target.shape)}")
        B, _, H, W = y_pred.shape
        div = 1 << mod.num_pools
        if H % div or W % div:
            raise ValueError(f"VisualLoss: H={H} and W={W} must be divisible by {div} ({mod.num_pools} max-pools)")
        dev = y_pred.device
        packs, biases = mod.prepare(dev)
        keep = ctx.needs_input_grad[1]
        x = torch.empty((2 * B, H, W, 8), dtype=torch.bfloat16, device=dev)
        ops.vgg_normalise(y_pred.detach(), x[:B])
        ops.vgg_normalise(y_target.detach(), x[B:])
        if tr is not None:
            tr.update(input=x, items=[], acts=[], packed=packs, biases=biases)
        saved, relu_in, li = [], False, 0
        for it in mod.items:
            if it[0] == "pool":
                y = ops.maxpool2(x)
                saved.append(("pool", x[:B], None))
            else:
                wf = packs[li][0]
                y = torch.empty((2 * B, x.shape[1], x.shape[2], wf.shape[0]), dtype=torch.bfloat16, device=dev)
                ops.conv3(x, wf, y, bias=biases[li], relu=True)
                saved.append(("conv", x[:B], li, relu_in))
                relu_in = True
                li += 1
            if tr is not None:
                tr["items"].append(("conv", li - 1) if it[0] == "conv" else ("pool",))
                tr["acts"].append(y)
            x = y
        fp, ft = x[:B], x[B:]
        loss = ops.feature_mse(fp, ft)
        if tr is not None:
            tr["loss"] = loss
        if keep:
            ctx.mod, ctx.saved, ctx.feat, ctx.feat_relu = mod, saved, (fp, ft), relu_in
        return loss

    @staticmethod
    def backward(ctx, gout):
        from . import ops
        tr = TRACE if isinstance(TRACE, dict) else None
        packs, _ = ctx.mod.prepare(gout.device)
        fp, ft = ctx.feat
        g = ops.feature_mse_backward(fp, ft, gout.contiguous().float(), relu_mask=ctx.feat_relu)
        grads = []
        if tr is not None:
            tr["g_feat"] = g
        for rec in reversed(ctx.saved):
            xin = rec[1]
            if rec[0] == "pool":
                g = ops.maxpool2_backward(xin, g)
            else:
                gin = torch.empty_like(xin)
                ops.conv3(g, packs[rec[2]][1], gin, bias=None, relu=False, mask=xin if rec[3] else None)
                g = gin
            grads.append(g)
        dx = ops.vgg_normalise_backward(g)
        if tr is not None:
            tr["grads"] = grads[::-1]
            tr["g_input"] = dx
        return None, dx, None


class VisualLoss(nn.Module):
    """Perceptual loss of the reference's ``src/`` line (src/loss.py:29-56): F.mse_loss between the features of an
    eval-mode, frozen ``vgg19_bn().features[:40]`` of the two images, each first mapped from the tanh range to the
    ImageNet-normalised one.  ``features``: an nn.Sequential in torchvision's layout (``vgg19_bn_features``) made of
    Conv2d(k=3, s=1, p=1) [+ BatchNorm2d] + ReLU groups and MaxPool2d(2, 2).  BatchNorm is folded into the conv at
    construction (``refresh()`` folds again after loading weights); the chain runs in bf16 on the HIP 3x3 MFMA
    kernels with fp32 accumulation.  Only ``y_pred`` receives a gradient.  The module holds no parameter and no
    state_dict entry, and stays in eval mode whatever ``.train()`` is called on it."""

    def __init__(self, features, norm=None, reduction: str = 'mean'):
        super().__init__()
        if reduction != 'mean' or (norm is not None and norm is not torch.nn.functional.mse_loss):
            raise NotImplementedError("stcgan_amd VisualLoss: only F.mse_loss with reduction='mean' is on the path")
        items = _parse_features(features)
        features.requires_grad_(False).eval()
        # (not a registered submodule: no parameter, no state_dict entry, nothing for .to() / the checkpoints)
        self.__dict__["features"] = features
        self.__dict__["items"] = items
        self.reduction = reduction
        self.num_pools = sum(1 for it in items if it[0] == "pool")
        self.refresh()
        super().train(False)

    def train(self, mode: bool = True):
        return super().train(False)

    def refresh(self):
        """Fold the BatchNorms into the convs again (after weights were loaded into ``features``), in fp32:
        s = gamma / sqrt(running_var + eps), w' = w * s, b' = (b - running_mean) * s + beta (b = 0 without a bias)."""
        folded = []
        with torch.no_grad():
            for it in self.items:
                if it[0] != "conv":
                    continue
                conv, bn = it[1], it[2]
                w = conv.weight.detach().float().cpu()
                b = conv.bias.detach().float().cpu() if conv.bias is not None else torch.zeros(w.shape[0])
                if bn is not None:
                    gamma = bn.weight.detach().float().cpu() if bn.weight is not None else torch.ones(w.shape[0])
                    beta = bn.bias.detach().float().cpu() if bn.bias is not None else torch.zeros(w.shape[0])
                    s = gamma / torch.sqrt(bn.running_var.detach().float().cpu() + bn.eps)
                    w = w * s[:, None, None, None]
                    b = (b - bn.running_mean.detach().float().cpu()) * s + beta
                folded.append((w.contiguous(), b.contiguous()))
        self.__dict__["_folded"] = folded
        self.__dict__["_packs"] = {}

    def folded(self):
        """Per conv layer (w' fp32 [Co, Ci, 3, 3], b' fp32 [Co])."""
        return list(self._folded)

    def prepare(self, device):
        """The packed bf16 operands and fp32 biases on ``device`` (packed once per device and refresh())."""
        from . import ops
        key = str(device)
        hit = self._packs.get(key)
        if hit is None:
            ws = [w.to(device) for w, _ in self._folded]
            hit = self._packs[key] = (ops.pack_conv3(ws), [b.to(device) for _, b in self._folded])
        return hit

    def forward(self, y_pred, y_target):
        return _VisualFn.apply(self, y_pred, y_target)
