"""The generator's output head (activation = "none" / "tanh" / "sigmoid" / "htanh"): fp64 references, exactly
representable backward operands and a plain torch.nn restatement with a replaceable head (helper of the head tests; not
a test module).

Forward.  ``head(act, q)``: none q, tanh, sigmoid 1 / (1 + exp(-q)), htanh clamp(q, -1, 1) -- in fp64, or in the dtype
given (htanh and none only move or clamp values: they are exact in any dtype).

Backward, from the stored output y alone (include/stcgan_hip.h, stc_head_bwd):
  none     dq = gy
  tanh     dq = gy * (1 - y^2)
  sigmoid  omy = 1 - y;  dq = gy * (y * omy)
  htanh    dq = gy where -1 < y < 1, else 0   (torch's hardtanh_backward: y is exactly +-1 where q is at or outside)
``dq_torch`` evaluates the same formulas with torch fp32 elementwise ops in that order -- no multiply feeds an add in
the sigmoid form, so nothing can contract to an FMA and a kernel must give the same bits.

Exact operands, in the style of edge_loss_ref.tanh_operands: y and gy on coarse binary grids, so that every dq is a
multiple of 1/256 of magnitude <= 4 and every chunk sum of ``require_exact``'s size is exact in fp32 in any order."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from edge_loss_ref import LIMIT, quarters, tanh_operands
from upconv_ref import UpRefG

F64, F32 = torch.float64, torch.float32
HEADS = ("none", "tanh", "sigmoid", "htanh")
CODES = {"none": 0, "tanh": 1, "sigmoid": 2, "htanh": 3}  # STC_HEAD_*


def head(act, q):
    """y = act(q) in q's dtype (fp64 for a reference)."""
    if act == "none":
        return q.clone()
    if act == "tanh":
        return torch.tanh(q)
    if act == "sigmoid":
        return 1.0 / (1.0 + torch.exp(-q))
    if act == "htanh":
        return q.clamp(-1.0, 1.0)
    raise ValueError(act)


def dhead(act, y):
    """act'(q) expressed in the output y, in y's dtype."""
    if act == "none":
        return torch.ones_like(y)
    if act == "tanh":
        return 1.0 - y * y
    if act == "sigmoid":
        return y * (1.0 - y)
    if act == "htanh":
        return ((y > -1.0) & (y < 1.0)).to(y.dtype)
    raise ValueError(act)


def dq_torch(act, y, gy):
    """dq in torch fp32 elementwise ops, in the documented order (the bits a kernel must produce)."""
    assert y.dtype == F32 and gy.dtype == F32
    if act == "none":
        return gy.clone()
    if act == "sigmoid":
        omy = 1.0 - y
        return gy * (y * omy)
    if act == "htanh":
        return torch.where((y > -1.0) & (y < 1.0), gy, torch.zeros_like(gy))
    raise ValueError(f"{act}: no FMA-free torch form")


def head_bwd_ref(act, y, gy):
    """(dq NCHW fp64, its per-channel sum) -- exact on ``operands``."""
    dq = gy.to(F64) * dhead(act, y.to(F64))
    return dq, dq.sum(dim=(0, 2, 3))


def operands(act, B, C, H, W, seed):
    """(y, gy) fp64 NCHW whose dq is exact in fp32: gy multiples of 1/4 in [-4, 4];
    sigmoid: y multiples of 1/8 in (0, 1) -- y * (1 - y) a multiple of 1/64, dq of 1/256, |dq| <= 1;
    htanh:   y multiples of 1/8 in [-1, 1], both +1 and -1 present (planted where the draw has none) -- dq is gy or 0;
    none:    y is not read (drawn as for htanh), dq = gy;   tanh: edge_loss_ref.tanh_operands."""
    if act == "tanh":
        return tanh_operands(B, C, H, W, seed)
    g = torch.Generator().manual_seed(int(seed))
    gy = quarters((B, C, H, W), seed + 1, -4, 4)
    if act == "sigmoid":
        y = torch.randint(1, 8, (B, C, H, W), generator=g).to(F64) / 8.0
        assert float(y.min()) > 0 and float(y.max()) < 1
    else:
        y = torch.randint(-8, 9, (B, C, H, W), generator=g).to(F64) / 8.0
        flat = y.view(-1)
        flat[0], flat[-1] = 1.0, -1.0
        if flat.numel() > 4:
            flat[flat.numel() // 2], flat[flat.numel() // 2 + 1] = -1.0, 1.0
        assert bool((y == 1).any()) and bool((y == -1).any()) and float(y.abs().max()) == 1
    dq = head_bwd_ref(act, y, gy)[0]
    assert bool((dq * 256 == (dq * 256).round()).all()) and float(dq.abs().max()) <= 4
    assert torch.equal(dq.to(F32).to(F64), dq) and torch.equal(y.to(F32).to(F64), y)
    return y, gy


def require_exact(dq, chunk_pixels):
    """Every fp32 sum over one chunk's pixels is an integer number of 1/256 below 2^24 whatever its order."""
    assert chunk_pixels * max(float(dq.abs().max()), 2.0 ** -8) * 256 < LIMIT, (chunk_pixels, float(dq.abs().max()))


class HeadRefG(UpRefG):
    """upconv_ref.UpRefG (the no_conv_t restatement; same keys) whose output head is ``act`` instead of tanh.
    ``pre`` returns the pre-activation q."""

    def __init__(self, *args, act="tanh", **kwargs):
        super().__init__(*args, **kwargs)
        self.act = act

    def pre(self, x):
        m = self.model.model
        return m[3](F.relu(m[1](m[0](x))))

    def forward(self, x):
        return head(self.act, self.pre(x))


def head_module(act):
    """The module the reference appends for ``act`` (src/models/opt_layers.py:7-18), None for "none"."""
    return {"none": None, "tanh": nn.Tanh(), "sigmoid": nn.Sigmoid(),
            "htanh": nn.Hardtanh(min_val=-1.0, max_val=1.0, inplace=True)}[act]
