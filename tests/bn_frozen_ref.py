"""fp64 reference of a BatchNorm2d layer that normalises with its running statistics ("frozen"), forward and backward,
fused with the LeakyReLU / ReLU of its consumers.  Written from the definitions, not from csrc/bn.hip:

    rstd_run = 1 / sqrt(running_var + eps)        scale = gamma * rstd_run        shift = beta - running_mean * scale
    n  = scale * x + shift                                                       (the layer output; buffers untouched)
    dn = g1 * f * act'(n, s1) [+ g2 * act'(n, s2)]      act'(n, s) = 1 if n > 0 else s;  f = keep / (1 - p) under a
                                                        dropout level between the norm and the activation, else 1
    dx = scale * dn         dbeta = sum dn         dgamma = sum dn * xhat,   xhat = (x - running_mean) * rstd_run

Tensors are channels-last [B, H, W, C] (the kernels' layout); sums run over B, H, W.  Everything is torch.float64 on
the CPU, computed from the values handed in (the caller passes exactly what it uploads: fp32, or bf16-rounded).
"""
import numpy as np
import torch

from dropout_ref import keep_view, scale32


def slope32(s):
    """A slope as the C-ABI receives it (float)."""
    return float(np.float32(s))


def tables(gamma, beta, running_mean, running_var, eps):
    """(scale, shift, rstd_run) in fp64."""
    g, b, rm, rv = (t.double() for t in (gamma, beta, running_mean, running_var))
    rstd = 1.0 / torch.sqrt(rv + float(eps))
    scale = g * rstd
    return scale, b - rm * scale, rstd


def forward(x, scale, shift):
    return x.double() * scale.double() + shift.double()


def dact(n, slope):
    return torch.where(n > 0, 1.0, slope32(slope)).double()


def drop_factor(seed, offset, level, extent, hw, p):
    """keep / (1 - p) (as the kernels hold 1 / (1 - p): the fp32 of it) or 0, over the top-left ``hw`` view of the
    full extent (B, FH, FW, C) the mask's logical index runs over; fp64 [B, H, W, C]."""
    return keep_view(seed, offset, level, extent, hw, p).double() * float(scale32(p))


def backward(x, scale, shift, running_mean, rstd, g1=None, s1=0.0, g2=None, s2=0.0, factor=None):
    """dict(n, dn, mag, dx, dbeta, dgamma, mag_beta, mag_gamma): the definitions above; mag = sum of the absolute
    values of dn's terms per element, mag_beta / mag_gamma the per-channel sums of the absolute values of the terms
    of dbeta / dgamma (what an accumulation-error bound scales with).  factor: drop_factor's result, applied to g1."""
    xd = x.double()
    n = forward(xd, scale, shift)
    dn = torch.zeros_like(n)
    mag = torch.zeros_like(n)
    if g1 is not None:
        t = g1.double() * (factor if factor is not None else 1.0) * dact(n, s1)
        dn, mag = dn + t, mag + t.abs()
    else:
        assert factor is None, "a dropout level acts on g1"
    if g2 is not None:
        t = g2.double() * dact(n, s2)
        dn, mag = dn + t, mag + t.abs()
    xhat = (xd - running_mean.double()) * rstd.double()
    dims = (0, 1, 2)
    return dict(n=n, dn=dn, mag=mag, xhat=xhat, dx=scale.double() * dn, dbeta=dn.sum(dims),
                dgamma=(dn * xhat).sum(dims), mag_beta=mag.sum(dims), mag_gamma=(mag * xhat.abs()).sum(dims))


def chunk_sums(ref, nch):
    """part[chunk][c] = {sum dn, sum dn * xhat} and the sums of the terms' absolute values, over the chunk's
    per = ceil(P / nch) consecutive pixels (pixel index = (b * H + y) * W + x); fp64 [nch, C, 2] each."""
    dn, xh, mag = ref["dn"], ref["xhat"], ref["mag"]
    C = dn.shape[-1]
    dn, xh, mag = dn.reshape(-1, C), xh.reshape(-1, C), mag.reshape(-1, C)
    P = dn.shape[0]
    per = -(-P // nch)
    val = torch.zeros((nch, C, 2), dtype=torch.float64)
    absv = torch.zeros((nch, C, 2), dtype=torch.float64)
    for k in range(nch):
        a, b = k * per, min(P, (k + 1) * per)
        if a >= b:
            continue
        val[k, :, 0], val[k, :, 1] = dn[a:b].sum(0), (dn[a:b] * xh[a:b]).sum(0)
        absv[k, :, 0], absv[k, :, 1] = mag[a:b].sum(0), (mag[a:b] * xh[a:b].abs()).sum(0)
    return val, absv
