"""Resize-convolution up path (no_conv_t / --NN-upconv): a plain torch.nn restatement of the generator whose up layers
are ``nn.Sequential(nn.Upsample(2, "nearest"), nn.Conv2d(3, 1, 1))``, and numpy restatements of the weight identity
(helper of the upconv tests; not a test module).

The restatement subclasses the blocks of tests/inorm_ref.py, so ``inorm_ref.sign_margin`` and ``activation_inputs``
work on it; its forward is RefBlock's (the pair is called where the ConvTranspose2d was).

The identity.  Nearest 2x upsampling followed by a zero-padded 3x3 convolution is the ConvTranspose2d(4, 2, 1) with
    W4[ci][co][k][l] = sum_{a in ROWS[k]} sum_{b in ROWS[l]} w3[co][ci][a][b]           ROWS = ({2}, {1, 2}, {0, 1}, {0})
and its adjoint dw3[co][ci][a][b] = sum_{k : a in ROWS[k]} sum_{l : b in ROWS[l]} dW4[ci][co][k][l].  ``expand`` and
``collapse`` evaluate them in fp32 in the order the C-ABI documents (include/stcgan_hip.h): the outer index ascending
outside, the inner one inside, summed left to right from the first term, additions only -- so a kernel must match them
bit for bit.  ``M`` is the 4x3 matrix of the map (W4 = M w3 M^T per channel pair) for the fp64 einsum checks."""
import numpy as np
import torch
import torch.nn as nn

from inorm_ref import RefBlock

ROWS = ((2,), (1, 2), (0, 1), (0,))
M = np.zeros((4, 3))
for _k, _r in enumerate(ROWS):
    M[_k, list(_r)] = 1.0
SHAPES = [(2, 5, 3, 1, 1), (2, 8, 16, 2, 3), (1, 4, 4, 7, 5), (3, 16, 8, 16, 16)]  # (B, Ci, Co, H, W)


def expand(w3):
    """fp32 [Co, Ci, 3, 3] -> fp32 [Ci, Co, 4, 4], in the documented order."""
    w3 = np.ascontiguousarray(w3, dtype=np.float32)
    Co, Ci = w3.shape[:2]
    out = np.empty((Ci, Co, 4, 4), dtype=np.float32)
    wt = w3.transpose(1, 0, 2, 3)
    for k in range(4):
        for l in range(4):
            acc = None
            for a in ROWS[k]:
                for b in ROWS[l]:
                    term = wt[:, :, a, b]
                    acc = term.copy() if acc is None else (acc + term).astype(np.float32)
            out[:, :, k, l] = acc
    return out


def collapse(dW4):
    """fp32 [Ci, Co, 4, 4] -> fp32 [Co, Ci, 3, 3], in the documented order (k outside, l inside)."""
    dW4 = np.ascontiguousarray(dW4, dtype=np.float32)
    Ci, Co = dW4.shape[:2]
    out = np.empty((Co, Ci, 3, 3), dtype=np.float32)
    gt = dW4.transpose(1, 0, 2, 3)
    for a in range(3):
        for b in range(3):
            acc = None
            for k in range(4):
                if a not in ROWS[k]:
                    continue
                for l in range(4):
                    if b not in ROWS[l]:
                        continue
                    term = gt[:, :, k, l]
                    acc = term.copy() if acc is None else (acc + term).astype(np.float32)
            out[:, :, a, b] = acc
    return out


def expand_t(w3):
    """``expand`` on a torch fp32 tensor (CPU result)."""
    return torch.from_numpy(expand(w3.detach().cpu().float().numpy()))


def collapse_t(dW4):
    return torch.from_numpy(collapse(dW4.detach().cpu().float().numpy()))


def up_pair(cin, cout, bias):
    return nn.Sequential(nn.Upsample(scale_factor=2, mode="nearest"), nn.Conv2d(cin, cout, 3, 1, 1, bias=bias))


class UpRefBlock(RefBlock):
    """RefBlock with its ConvTranspose2d replaced, at the same index, by the Upsample + Conv2d pair."""

    def __init__(self, *args, use_dropout=False, **kwargs):
        super().__init__(*args, **kwargs)
        layers = list(self.model)
        for i, m in enumerate(layers):
            if isinstance(m, nn.ConvTranspose2d):
                layers[i] = up_pair(m.in_channels, m.out_channels, m.bias is not None)
        if use_dropout:  # (a key-less module at the end, as the reference's block; the forward does not apply it)
            layers.append(nn.Dropout(0.5))
        self.model = nn.Sequential(*layers)


class UpRefG(nn.Module):
    def __init__(self, in_c, out_c, ngf=64, num_downs=8, norm_layer=nn.BatchNorm2d, use_dropout=False):
        super().__init__()
        blk = UpRefBlock(ngf * 8, ngf * 8, innermost=True, norm_layer=norm_layer)
        for _ in range(num_downs - 5):
            blk = UpRefBlock(ngf * 8, ngf * 8, submodule=blk, norm_layer=norm_layer, use_dropout=use_dropout)
        for mult in (4, 2, 1):
            blk = UpRefBlock(ngf * mult, ngf * mult * 2, submodule=blk, norm_layer=norm_layer)
        self.model = UpRefBlock(out_c, ngf, input_nc=in_c, submodule=blk, outermost=True, norm_layer=norm_layer)

    def forward(self, x):
        return self.model(x)
