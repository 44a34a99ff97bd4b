"""Integer-valued operands and fp64 references for the bit-exact conv tests (tests/test_gpu_conv_exact.py; checked
without a GPU by tests/test_conv_exact_cpu.py).

Small integers are exact in bf16 and their products are exact in fp32, so while sum |x||w| stays below 2^24 every
partial sum of a convolution is an integer below 2^24 and therefore exact in fp32 -- in any summation order, tile
shape, split-K slab or MFMA chain.  The fp32 accumulator then equals the mathematical result: an fp32 output equals
the fp64 reference bit for bit, a bf16 output is its round-to-nearest-even rounding (one rounding of an exact
value), and one missing, duplicated or misplaced product fails torch.equal at any K.  ``require_exact`` asserts the
precondition for every case; a case that violates it is a mistake in the test, not in the kernel.

Operands exclude zero, so leaving out any single product changes the result (``drop_one_product``).

Geometry names follow the C-ABI kinds: conv_s2 / conv_s1 (Conv2d k4 p1, weight [Cout][Cin][4][4]), convT_s2
(ConvTranspose2d k4 s2 p1, weight [Cin][Cout][4][4]) and s1_dgrad (the stride-1 conv's input gradient,
conv_transpose2d with stride 1 of the CONV weight [Cin][Cout][4][4] where Cin is the GEMM's reduction).
"""
import functools

import torch
import torch.nn.functional as F

F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16
LIMIT = float(2 ** 24)
EPS32 = 2.0 ** -23
KINDS = ("conv_s2", "conv_s1", "convT_s2", "s1_dgrad")


# ---------------------------------------------------------------- operand makers (CPU, seeded)
def ints(shape, seed, r, nonzero=True):
    """fp64 tensor of integers uniform in [-r, r] (without 0 when ``nonzero``)."""
    g = torch.Generator().manual_seed(int(seed))
    if nonzero:
        v = torch.randint(1, r + 1, tuple(shape), generator=g)
        s = torch.randint(0, 2, tuple(shape), generator=g) * 2 - 1
        return (v * s).to(F64)
    return torch.randint(-r, r + 1, tuple(shape), generator=g).to(F64)


def acts(shape, seed, r=8):
    """Integer activations / gradients in [-r, r] \\ {0} (r = 16 for the 8-channel stem)."""
    return ints(shape, seed, r)


def weights(shape, seed, r=8):
    return ints(shape, seed, r)


def biases(n, seed):
    """Integer biases in [-64, 64] \\ {0}."""
    return ints((n,), seed, 64)


def pro_table(C, seed):
    """A prologue table: scale in {1, -1, 2, -2, 0.5} per channel, integer shift in [-4, 4] (zero allowed).  With
    integer x the prologue value x*scale+shift is a half-integer of magnitude <= 2r+4, and slope 0.5 makes it a
    quarter-integer: exact in fp32 and in bf16 (at most 7 significant bits)."""
    g = torch.Generator().manual_seed(int(seed))
    choices = torch.tensor([1.0, -1.0, 2.0, -2.0, 0.5], dtype=F64)
    sc = choices[torch.randint(0, 5, (C,), generator=g)]
    sh = torch.randint(-4, 5, (C,), generator=g).to(F64)
    return sc, sh


def prologue(x, table, slope):
    """act(x*scale+shift, slope) per channel of NCHW x in fp64 (table / slope None: skipped)."""
    v = x
    if table is not None:
        sc, sh = table
        v = v * sc[None, :, None, None] + sh[None, :, None, None]
    if slope is not None:
        v = torch.where(v > 0, v, v * float(slope))
    return v


# ---------------------------------------------------------------- fp64 references
def conv_ref(kind, x, w, bias=None):
    """fp64 result (NCHW) of one forward kind on NCHW ``x``."""
    x, w = x.to(F64), w.to(F64)
    b = None if bias is None else bias.to(F64)
    if kind == "conv_s2":
        return F.conv2d(x, w, b, 2, 1)
    if kind == "conv_s1":
        return F.conv2d(x, w, b, 1, 1)
    if kind == "convT_s2":
        return F.conv_transpose2d(x, w, b, 2, 1)
    if kind == "s1_dgrad":
        return F.conv_transpose2d(x, w, b, 1, 1)
    raise ValueError(kind)


def conv_abs(kind, x, w, bias=None):
    """A = conv(|x|, |w|) + |bias|: the largest magnitude any partial sum of any order can reach."""
    return conv_ref(kind, x.abs(), w.abs(), None if bias is None else bias.abs())


def wgrad_ref(role, stride, x, dy):
    """fp64 weight gradient by autograd.  role "conv": y = conv2d(x, w, stride) -> dW [Cout][Cin][4][4];
    role "convT": y = conv_transpose2d(x, w, 2) -> dW [Cin][Cout][4][4].  ``x`` NCHW input, ``dy`` NCHW output
    gradient."""
    x, dy = x.to(F64), dy.to(F64)
    if role == "conv":
        w = torch.zeros(dy.shape[1], x.shape[1], 4, 4, dtype=F64, requires_grad=True)
        y = F.conv2d(x, w, None, stride, 1)
    elif role == "convT":
        w = torch.zeros(x.shape[1], dy.shape[1], 4, 4, dtype=F64, requires_grad=True)
        y = F.conv_transpose2d(x, w, None, 2, 1)
    else:
        raise ValueError(role)
    assert y.shape == dy.shape, (y.shape, dy.shape)
    (gw,) = torch.autograd.grad(y, w, dy)
    return gw


def wgrad_abs(role, stride, x, dy):
    """sum |D||G| per weight element."""
    return wgrad_ref(role, stride, x.abs(), dy.abs())


def require_exact(A, unit=1.0):
    """The precondition: every partial sum is a multiple of ``unit`` (a power of two <= 1) below 2^24 units."""
    m = float(A.max()) / unit
    assert m < LIMIT, f"sum|x||w| reaches {m:.0f} units >= 2^24: the case is not exact in fp32 (a mistake in the test)"
    return m


def expect_f32(ref64):
    out = ref64.float()
    assert torch.equal(out.double(), ref64), "the reference is not representable in fp32"
    return out


def expect_bf16(ref64):
    """Round-to-nearest-even of the exact value (exact in fp32, so there is no double rounding)."""
    return expect_f32(ref64).to(BF16)


def act_bf16(v, slope):
    """bf16(v > 0 ? v : fp32(slope) * v) of bf16 ``v``: the activation epilogue on the bf16-rounded conv value, one
    fp32 multiply, one rounding."""
    v32 = v.float()
    s = torch.tensor(float(slope), dtype=F32)
    return torch.where(v32 > 0, v32, v32 * s).to(BF16)


def dact(x, slope):
    """act'(x, slope) in fp32: 1 where x > 0, else fp32(slope)."""
    one = torch.ones((), dtype=F32)
    return torch.where(x.float() > 0, one, torch.tensor(float(slope), dtype=F32))


def rounding_shares(ref64):
    """(share of values that are not bf16-representable, share that are exact bf16 ties) of an exact fp32 tensor."""
    f = expect_f32(ref64).contiguous()
    low = f.view(torch.int32) & 0xFFFF
    return float((low != 0).double().mean()), float((low == 0x8000).double().mean())


def require_shares(ref64, what=""):
    """For bf16-output cases with K >= 1024: >= 25 % of the reference values need rounding and >= 5 % are ties, so
    the store's rounding mode is exercised (a condition on the inputs)."""
    nr, tie = rounding_shares(ref64)
    assert nr >= 0.25 and tie >= 0.05, f"{what}: {nr:.1%} need rounding, {tie:.1%} ties: the case went soft"
    return nr, tie


def drop_one_product(kind, x, w, idx=None):
    """Sensitivity of the expected tensor to the products of one input element x[idx] (default: the last element, a
    border pixel).  Returns (output elements that change when x[idx] is zeroed, output elements that change when
    only the single product x[idx] * w[last weight element] is removed -- 0 or 1, by linearity the support of that
    product alone).  Operands are non-zero, so the first is positive, and the second is 1 wherever the padding
    lets that tap reach an output."""
    x = x.to(F64)
    idx = tuple(d - 1 for d in x.shape) if idx is None else idx
    assert float(x[idx]) != 0.0
    full = conv_ref(kind, x, w)
    x2 = x.clone()
    x2[idx] = 0.0
    all_w = int((conv_ref(kind, x2, w) != full).sum())
    # a single product: zero one weight element and restrict x to the chosen element
    one = torch.zeros_like(x)
    one[idx] = x[idx]
    w1 = torch.zeros_like(w, dtype=F64)
    flat = w.to(F64).reshape(-1)
    assert float(flat[-1]) != 0.0
    w1.reshape(-1)[-1] = flat[-1]
    single = int((conv_ref(kind, one, w1) != 0).sum())
    return all_w, single


# ---------------------------------------------------------------- statistics
def stats_ref(y64):
    """Per-channel (mean, biased variance, count) of NCHW fp64 ``y64`` over exactly its extent."""
    P = y64.shape[0] * y64.shape[2] * y64.shape[3]
    return y64.mean(dim=(0, 2, 3)), y64.var(dim=(0, 2, 3), unbiased=False), P


def merge_partials(part):
    """Chan merge in fp64 of conv_stats partials [chunks][C][4] = {n, S1, S2, shift} (chunk mean = shift + S1/n,
    chunk M2 = max(S2 - S1^2/n, 0)): (total count per channel, mean, biased variance)."""
    p = part.detach().cpu().double()
    n, S1, S2, sh = p[..., 0], p[..., 1], p[..., 2], p[..., 3]
    live = n > 0
    nn = torch.where(live, n, torch.ones_like(n))
    N = n.sum(0)
    mi = sh + S1 / nn
    m2i = (S2 - S1 * S1 / nn).clamp_min(0.0)
    mean = (n * mi).sum(0) / N
    M2 = (live * (m2i + n * (mi - mean[None]) ** 2)).sum(0)
    return N, mean, M2 / N


def stats_bounds(y64, m):
    """fp32 error bounds (mean, variance) per channel for shifted one-pass chunk statistics whose longest fp32
    accumulation chain has ``m`` steps (rows summed per lane + the lane / wave merges + the roundings inside a
    term), merged in fp64.  With R = max - min of the channel (every shifted term |x - shift| <= R, the shift being
    one of the chunk's values) and A = max |x|:
      chunk mean  = shift + S1/n:  |error| <= m*EPS32*R (the sum) + 4*EPS32*A (forming and merging means);
      the merged mean is a weighted average of chunk means, so the same bound holds for it;
      chunk M2    = S2 - S1^2/n:   |error| <= n*m*EPS32*R^2 (S2) + 2*n*m*EPS32*R^2 (S1 in S1^2/n);
      the between-chunk term n*(mean_i - mean)^2 moves by <= 2*n*R*(mean bound);
      so the variance is within 5*m*EPS32*R^2 + 8*EPS32*A*R.
    Nothing here comes from the kernel under test."""
    mx = y64.amax(dim=(0, 2, 3))
    mn = y64.amin(dim=(0, 2, 3))
    R = (mx - mn)
    A = torch.maximum(mx.abs(), mn.abs())
    bm = m * EPS32 * R + 4 * EPS32 * A
    bv = 5 * m * EPS32 * R * R + 8 * EPS32 * A * R
    return bm, bv


def one_pixel_margin(y64, bm, bv):
    """The one-pixel condition: for every channel, the statistics with one pixel of that channel left out (the
    pixel farthest from the channel mean) differ from the full ones by more than the bounds.  Returns the smallest
    (difference / bound) over channels for (mean, variance); both must exceed 1 for the bounds to see one pixel."""
    B, C, H, W = y64.shape
    P = B * H * W
    v = y64.permute(1, 0, 2, 3).reshape(C, P)
    mean = v.mean(1)
    var = v.var(1, unbiased=False)
    k = (v - mean[:, None]).abs().argmax(1)
    xk = v[torch.arange(C), k]
    s1 = v.sum(1) - xk
    mean1 = s1 / (P - 1)
    var1 = ((v - mean1[:, None]) ** 2).sum(1) - (xk - mean1) ** 2
    var1 = var1 / (P - 1)
    rm = ((mean1 - mean).abs() / bm).min()
    rv = ((var1 - var).abs() / bv).min()
    return float(rm), float(rv)


# ---------------------------------------------------------------- fused BatchNorm backward (fp64)
def bn_tables(C, seed):
    """BatchNorm state as the backward reads it: fp32 (scale, shift, mean, rstd, gamma), positive and negative
    scales / gammas."""
    g = torch.Generator().manual_seed(int(seed))
    scale = (torch.rand(C, generator=g) + 0.5)
    scale[1::3] *= -1.0
    shift = (torch.rand(C, generator=g) - 0.5) * 0.6  # |shift| < 0.3 <= |x * scale| - 0.2 for integer x != 0
    mean = torch.randn(C, generator=g) * 0.1
    rstd = torch.rand(C, generator=g) + 0.5
    gamma = torch.rand(C, generator=g) + 0.5
    gamma[2::5] *= -1.0
    return tuple(t.float() for t in (scale, shift, mean, rstd, gamma))


def bn_backward_ref(v, x, go, tables, s_self, s_other):
    """fp64 reference of the fused BatchNorm backward from NHWC fp64 tensors: ``v`` the conv output at the BN channels
    AS THE KERNEL READS IT (the bf16-rounded value), ``x`` the BN input, ``go`` the second gradient or None.
      nn = x*scale + shift (the sign decides the activation branch; evaluated as the kernel does, one fp32 fma);
      dn = v*act'(nn, s_self) + go*act'(nn, s_other);  xhat = (x - mean)*rstd;
      dbeta = sum dn;  dgamma = sum dn*xhat;  dx = gamma*rstd*(dn - dbeta/P - xhat*dgamma/P).
    Returns {name: (value, sum |terms|)} for dbeta / dgamma and (dx, |terms| of dx)."""
    scale, shift, mean, rstd, gamma = tables
    nn = x * scale.double() + shift.double()
    # the kernel's fp32 fma can decide another branch only where nn is within rounding of zero: no such element
    assert float(nn.abs().min()) > 1e-4 * float(nn.abs().max()), "an activation input too close to zero"
    pos = nn > 0
    ss, so = (float(torch.tensor(float(s), dtype=F32)) for s in (s_self, s_other))  # as the C-ABI receives them
    dn = v * torch.where(pos, 1.0, ss)
    dn_abs = v.abs() * torch.where(pos, 1.0, abs(ss))
    if go is not None:
        dn = dn + go * torch.where(pos, 1.0, so)
        dn_abs = dn_abs + go.abs() * torch.where(pos, 1.0, abs(so))
    xhat = (x - mean.double()) * rstd.double()
    P = x.shape[0] * x.shape[1] * x.shape[2]
    dbeta = dn.sum(dim=(0, 1, 2))
    dgamma = (dn * xhat).sum(dim=(0, 1, 2))
    dbeta_abs = dn_abs.sum(dim=(0, 1, 2))
    dgamma_abs = (dn_abs * xhat.abs()).sum(dim=(0, 1, 2))
    k = gamma.double() * rstd.double()
    dx = k * (dn - dbeta / P - xhat * dgamma / P)
    dx_abs = k.abs() * (dn_abs + dbeta_abs / P + xhat.abs() * dgamma_abs / P)
    return {"dbeta": (dbeta, dbeta_abs), "dgamma": (dgamma, dgamma_abs), "dx": (dx, dx_abs), "dn": (dn, dn_abs)}


@functools.lru_cache(maxsize=None)
def fwd_case(kind, B, Cin, Cout, GH, GW, seed=0, r=8, bias=False):
    """One forward case from its GEMM geometry (grid GH x GW: the output of conv_s2 / conv_s1 / s1_dgrad, the input
    of convT_s2): (x NCHW, w torch layout, bias or None, ref64 NCHW), all fp64, precondition asserted.  Cached: a
    reference is computed once and shared (never modify the returned tensors)."""
    assert kind in KINDS
    in_hw = {"conv_s2": (2 * GH, 2 * GW), "conv_s1": (GH + 1, GW + 1), "convT_s2": (GH, GW),
             "s1_dgrad": (GH - 1, GW - 1)}[kind]
    x = acts((B, Cin, *in_hw), 1000 + seed, r)
    wshape = (Cout, Cin, 4, 4) if kind in ("conv_s2", "conv_s1") else (Cin, Cout, 4, 4)
    w = weights(wshape, 2000 + seed, r)
    b = biases(Cout, 3000 + seed) if bias else None
    require_exact(conv_abs(kind, x, w, b))
    return x, w, b, conv_ref(kind, x, w, b)


@functools.lru_cache(maxsize=None)
def wgrad_case(role, stride, B, Cin, Cout, H, W, seed=0):
    """One weight-gradient case: (x NCHW [B, Cin, H, W], dy NCHW, dW fp64), precondition asserted.  Cached."""
    x = acts((B, Cin, H, W), 4000 + seed)
    if role == "conv":
        Ho, Wo = (H + 2 - 4) // stride + 1, (W + 2 - 4) // stride + 1
    else:
        Ho, Wo = 2 * H, 2 * W
    dy = acts((B, Cout, Ho, Wo), 5000 + seed)
    require_exact(wgrad_abs(role, stride, x, dy))
    return x, dy, wgrad_ref(role, stride, x, dy)
