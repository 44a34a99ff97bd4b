"""Reflect padding of the 4x4 convs (padding_mode="reflect"): fp64 references of the conv, its
input gradient and its weight gradient written from the index map, the input-gradient formulation the kernels use
(frame, then fold) restated, and a plain torch.nn restatement of both networks with reflect convs (helper of the
reflect tests; not a test module).

The index map.  A Conv2d k4 p1 with padding_mode="reflect" reads x[R(s*oy + kh - 1), R(s*ox + kw - 1)] with
R(j) = -j for j < 0 and 2(H - 1) - j for j >= H; only R(-1) = 1 and R(H) = H - 2 occur.

The adjoint.  Input pixel row 1 also receives what a virtual row -1 would receive, row H - 2 what row H would.  The
kernels run the padding-free transposed conv over the extended grid -1 .. H, -1 .. W (the "frame", index a + 1) and
then fold frame (a, b) into (R(a), R(b)): ``frame`` and ``fold`` below, ``dgrad_frame_fold`` their composition.

The networks.  ``ReflectG`` / ``ReflectD`` subclass the restatements of tests/inorm_ref.py (so inorm_ref.sign_margin
and activation_inputs work on them) and take the options the reflect model tests combine: no_conv_t (the Upsample +
Conv2d(3, 1, 1) pair of tests/upconv_ref.py, zero padding), the output activation, and dropout masks handed in by
the test ({level: NCHW keep / (1 - p)}, applied after the up-norm over the full extent).  Their state_dict keys are
the project's networks'."""
import functools

import torch
import torch.nn as nn
import torch.nn.functional as F

import conv_exact_ref as R
from inorm_ref import RefBlock, RefD
from upconv_ref import up_pair

F64 = torch.float64
# (stride, H, W) of the small planes every formulation is checked on: both reflections landing in a two-wide plane,
# a plane one reflection wide in one dimension only, odd extents for the stride-1 conv
SMALL = [(2, 2, 2), (2, 2, 6), (2, 4, 6), (1, 5, 6), (1, 2, 3), (1, 3, 2)]


def rmap(j, H):
    """R(j) for a plane of extent H."""
    if j < 0:
        return -j
    if j >= H:
        return 2 * (H - 1) - j
    return j


def out_extent(h, stride):
    return (h + 2 - 4) // stride + 1


def pad_reflect(x):
    """x [B, C, H, W] with a one-wide reflected border, by the index map."""
    H, W = x.shape[2], x.shape[3]
    if H < 2 or W < 2:
        raise RuntimeError("Padding size should be less than the corresponding input dimension")
    iy = torch.tensor([rmap(j, H) for j in range(-1, H + 1)])
    ix = torch.tensor([rmap(j, W) for j in range(-1, W + 1)])
    return x[:, :, iy][:, :, :, ix]


def conv(x, w, stride, bias=None):
    """fp64 y[oy, ox] = sum x[R(s oy + kh - 1), R(s ox + kw - 1)] w[kh, kw] (+ bias), tap by tap."""
    x, w = x.to(F64), w.to(F64)
    xp = pad_reflect(x)
    Ho, Wo = out_extent(x.shape[2], stride), out_extent(x.shape[3], stride)
    y = torch.zeros(x.shape[0], w.shape[0], Ho, Wo, dtype=F64)
    for kh in range(4):
        for kw in range(4):
            win = xp[:, :, kh:kh + stride * (Ho - 1) + 1:stride, kw:kw + stride * (Wo - 1) + 1:stride]
            y += torch.einsum("bchw,oc->bohw", win, w[:, :, kh, kw])
    if bias is not None:
        y += bias.to(F64)[None, :, None, None]
    return y


def wgrad(x, dy, stride):
    """fp64 dW[o, c, kh, kw] = sum dy[b, o, oy, ox] x[b, c, R(s oy + kh - 1), R(s ox + kw - 1)]."""
    x, dy = x.to(F64), dy.to(F64)
    xp = pad_reflect(x)
    Ho, Wo = dy.shape[2], dy.shape[3]
    dW = torch.zeros(dy.shape[1], x.shape[1], 4, 4, dtype=F64)
    for kh in range(4):
        for kw in range(4):
            win = xp[:, :, kh:kh + stride * (Ho - 1) + 1:stride, kw:kw + stride * (Wo - 1) + 1:stride]
            dW[:, :, kh, kw] = torch.einsum("bohw,bchw->oc", dy, win)
    return dW


def dgrad(dy, w, stride, H, W):
    """fp64 input gradient, product by product: dx[R(a), R(b)] += dy[oy, ox] w[kh, kw] with a = s oy + kh - 1."""
    dy, w = dy.to(F64), w.to(F64)
    dx = torch.zeros(dy.shape[0], w.shape[1], H, W, dtype=F64)
    for oy in range(dy.shape[2]):
        for ox in range(dy.shape[3]):
            for kh in range(4):
                for kw in range(4):
                    a, b = rmap(stride * oy + kh - 1, H), rmap(stride * ox + kw - 1, W)
                    dx[:, :, a, b] += torch.einsum("bo,oc->bc", dy[:, :, oy, ox], w[:, :, kh, kw])
    return dx


def frame(dy, w, stride, H, W):
    """The padding-free transposed conv over the extended grid: fr[a + 1, b + 1] for a in -1 .. H, b in -1 .. W, what
    pixel (a, b) of the zero-extended plane receives.  (For an odd H under stride 2 row H receives nothing.)"""
    full = F.conv_transpose2d(dy.to(F64), w.to(F64), None, stride, 0)  # extent s (Ho - 1) + 4 <= H + 2
    fr = torch.zeros(dy.shape[0], w.shape[1], H + 2, W + 2, dtype=F64)
    fr[:, :, :full.shape[2], :full.shape[3]] = full
    return fr


def fold(fr, H, W):
    """dx[y, x] = the frame pixels that reflect onto (y, x), added in the kernel's fixed order: its own, row -1 for
    y == 1, row H for y == H - 2; per row its own column, column -1 for x == 1, column W for x == W - 2."""
    dx = torch.zeros(*fr.shape[:2], H, W, dtype=fr.dtype)
    for y in range(H):
        rows = [y + 1] + ([0] if y == 1 else []) + ([H + 1] if y == H - 2 else [])
        for x in range(W):
            cols = [x + 1] + ([0] if x == 1 else []) + ([W + 1] if x == W - 2 else [])
            for ry in rows:
                for rx in cols:
                    dx[:, :, y, x] += fr[:, :, ry, rx]
    return dx


def dgrad_frame_fold(dy, w, stride, H, W):
    return fold(frame(dy, w, stride, H, W), H, W)


def abs_bound(x, w, stride, dy):
    """(sum |x||w| of the forward, of the input gradient, of the weight gradient): conv_exact_ref.require_exact's
    argument for a reflect case."""
    return (conv(x.abs(), w.abs(), stride), dgrad_frame_fold(dy.abs(), w.abs(), stride, x.shape[2], x.shape[3]),
            wgrad(x.abs(), dy.abs(), stride))


@functools.lru_cache(maxsize=None)
def case(stride, B, Cin, Cout, H, W, seed=0):
    """One integer-valued case (conv_exact_ref's operand makers): x, w [Cout, Cin, 4, 4], dy and the three fp64
    references (y, dx, dW), the exactness precondition asserted for each.  Cached and shared: never modified."""
    x = R.acts((B, Cin, H, W), 7000 + seed, 16 if Cin == 8 else 8)
    w = R.weights((Cout, Cin, 4, 4), 8000 + seed)
    dy = R.acts((B, Cout, out_extent(H, stride), out_extent(W, stride)), 9000 + seed)
    for A in abs_bound(x, w, stride, dy):
        R.require_exact(A)
    y = conv(x, w, stride)
    if H * W <= 64:
        dx = dgrad(dy, w, stride, H, W)
        assert torch.equal(dx, dgrad_frame_fold(dy, w, stride, H, W))
    else:  # (integers: every order of the sum is exact, the two formulations agree to the bit -- the small planes show it)
        dx = dgrad_frame_fold(dy, w, stride, H, W)
    return x, w, dy, y, dx, wgrad(x, dy, stride)


# ---------------------------------------------------------------- the networks
ACTS = {"none": lambda v: v, "tanh": torch.tanh, "sigmoid": torch.sigmoid, "htanh": lambda v: v.clamp(-1.0, 1.0)}


class ReflectBlock(RefBlock):
    """RefBlock whose 4x4 down conv pads by reflection; optionally the resize-convolution up pair, another output
    activation, a dropout module (a key-less module at the end, as the project's block) and a mask."""

    def __init__(self, *args, level=0, no_conv_t=False, use_dropout=False, activation="tanh", padding_mode="reflect",
                 **kwargs):
        super().__init__(*args, **kwargs)
        layers = list(self.model)
        for i, m in enumerate(layers):
            if isinstance(m, nn.Conv2d):
                layers[i] = nn.Conv2d(m.in_channels, m.out_channels, 4, 2, 1, bias=False, padding_mode=padding_mode)
            elif isinstance(m, nn.ConvTranspose2d) and no_conv_t:
                layers[i] = up_pair(m.in_channels, m.out_channels, m.bias is not None)
        if self.outermost:
            layers = layers[:4] + ([nn.Identity()] if activation != "none" else [])  # (no keys either way)
        if use_dropout:
            layers.append(nn.Dropout(0.5))
        self.model = nn.Sequential(*layers)
        self.level, self.act, self.mask = level, ACTS[activation], None

    def forward(self, x):
        m = self.model
        if self.outermost:
            return self.act(m[3](F.relu(m[1](m[0](x)))))
        assert x.shape[2] % 2 == 0 and x.shape[3] % 2 == 0, "reflect restatement: even levels only"
        a = F.leaky_relu(x, 0.2)
        d = m[1](a)
        u = m[4](m[3](F.relu(d))) if self.innermost else m[6](m[5](F.relu(m[3](m[2](d)))))
        if self.mask is not None:
            u = u * self.mask.to(u.dtype)
        return torch.cat([a, u], 1)


class ReflectG(nn.Module):
    def __init__(self, in_c, out_c, ngf=64, num_downs=8, norm_layer=nn.BatchNorm2d, **kw):
        super().__init__()
        drop = kw.pop("use_dropout", False)
        level = num_downs - 1
        blk = ReflectBlock(ngf * 8, ngf * 8, innermost=True, norm_layer=norm_layer, level=level, **kw)
        for _ in range(num_downs - 5):
            level -= 1
            blk = ReflectBlock(ngf * 8, ngf * 8, submodule=blk, norm_layer=norm_layer, level=level, use_dropout=drop,
                               **kw)
        for mult in (4, 2, 1):
            level -= 1
            blk = ReflectBlock(ngf * mult, ngf * mult * 2, submodule=blk, norm_layer=norm_layer, level=level, **kw)
        self.model = ReflectBlock(out_c, ngf, input_nc=in_c, submodule=blk, outermost=True, norm_layer=norm_layer, **kw)

    def set_masks(self, masks):
        """{level: NCHW keep / (1 - p)} applied after that level's up-norm (None / {}: no dropout)."""
        for m in self.modules():
            if isinstance(m, ReflectBlock):
                m.mask = (masks or {}).get(m.level)
        return self

    def forward(self, x):
        return self.model(x)


class ReflectD(RefD):
    def __init__(self, in_c, ndf=64, n_layers=3, norm_layer=nn.BatchNorm2d, padding_mode="reflect"):
        super().__init__(in_c, ndf, n_layers, norm_layer)
        seq = list(self.model)
        for i, m in enumerate(seq):
            if isinstance(m, nn.Conv2d):
                seq[i] = nn.Conv2d(m.in_channels, m.out_channels, 4, m.stride, 1, bias=m.bias is not None,
                                   padding_mode=padding_mode)
        self.model = nn.Sequential(*seq)


# ---------------------------------------------------------------- the GPU kernel cases (tests/test_gpu_reflect_exact.py)
# (stride, B, Cin, Cout, H, W): the smallest planes at which each thing can break -- 2 x 2 (both reflections land in a
# two-wide plane), 2 x 6 and 4 x 6, 34 x 30 (tiles that straddle rows, M no tile multiple) for stride 2; 2 x 3, 3 x 2,
# 5 x 6 and 31 x 31 for stride 1; Cin in {8, 24, 64}, Cout in {1, 8, 40, 72}, B in {1, 2}; and an odd plane under stride
# 2 (31 x 15: the discriminator on odd extents -- the last row / column is never reflected, the frame's tail stays zero)
EXACT_CASES = [
    (2, 1, 24, 8, 31, 15),
    (2, 1, 8, 8, 2, 2), (2, 2, 24, 40, 2, 6), (2, 2, 64, 72, 4, 6), (2, 1, 24, 8, 34, 30), (2, 2, 64, 1, 34, 30),
    (2, 2, 8, 72, 34, 30),
    (1, 2, 8, 1, 2, 3), (1, 1, 24, 8, 3, 2), (1, 2, 64, 40, 5, 6), (1, 1, 64, 72, 31, 31), (1, 2, 24, 1, 31, 31),
]
# per direction, cases whose plan (read from the new queries by the GPU test) has split-K / pixel splits > 1 in both
# dtypes: forward K = 16 * 64; input gradient K = 16 * 72 (stride 1) and K = 4 * 128 per phase (stride 2: four phases,
# the slabs behind the frame, the reduction writing frame rows); weight gradient P = 900 pixels
SPLIT_CASES = {"fwd": (2, 2, 64, 72, 4, 6), "dgrad": (1, 1, 64, 72, 31, 31), "dgrad_s2": (2, 2, 64, 128, 4, 6),
               "wgrad": (1, 1, 64, 72, 31, 31)}
