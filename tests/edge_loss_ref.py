"""fp64 references, exactly-summable operands and derived error bounds for the kernels of csrc/eltwise.hip
(tests/test_gpu_edge_loss_family.py; checked without a GPU by tests/test_edge_loss_ref_cpu.py).

Plain torch / numpy on the CPU; nothing here calls the HIP library.

Exact operands.  Multiples of 1/4 (losses) and of 1/8 (tanh backward) keep every product and every partial sum of
every order exact in fp32, so a correct kernel must EQUAL the fp64 result rounded once to the output type; one
element left out or counted twice fails torch.equal.  Every generator asserts its precondition (``require_*``); a
case that violates it is a mistake of the test, not of the kernel.

Bounds.  What cannot be exact (BCE-with-logits, the gradient scale) is compared with fp64 within bounds derived from
the number of fp32 roundings of the documented formulas (include/stcgan_hip.h); EPS = 2^-24 is the relative error of
one rounding.  Nothing here is tuned to the output of a kernel.
"""
import numpy as np
import torch

F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16
EPS = 2.0 ** -24          # relative error of one fp32 rounding (half an ulp)
TINY = 2.0 ** -126        # smallest normal fp32: below it a rounding is absolute, not relative
LIMIT = float(2 ** 24)
L1, MSE, BCE = 0, 1, 2    # STC_LOSS_L1 / STC_LOSS_MSE_CONST / STC_LOSS_BCE_CONST
LOSS_PER_BLOCK = 4096     # elements of one fp32 partial sum: 16 serial additions per thread, then an 8-level tree
BLOCK_SERIAL, BLOCK_TREE = 16, 8

# U: the error budget of expf followed by log1pf (and of expf followed by the reciprocal of the sigmoid), in units
# of EPS relative to the result.  Origin: the ROCm tree this suite was written against ships no max-ulp table for
# its device math library, so U is measured: the worst error of torch's fp32 CPU evaluation of
# log1p(exp(-|x|)) and 1 / (1 + exp(-x)) against fp64 over the inputs of every BCE case of the GPU file (1.94 EPS),
# times 4 to allow for a different libm (7.75), rounded up.  tests/test_edge_loss_ref_cpu.py re-measures it and
# asserts 4 x measured <= U.  It is never derived from a kernel's output.
U = 8.0

BCE_FIXED = (0.0, 1e-8, -1e-8, 1.0, -1.0, 20.0, -20.0, 88.0, -88.0, 89.0, -89.0, 104.0, -104.0, 1e4, -1e4)


def f32(v):
    """The fp32 value of a Python float, as a Python float (what a ``float`` C argument receives)."""
    return float(np.float32(v))


# ---------------------------------------------------------------- layout references
def gather_ref(srcs, cpad):
    """torch.cat(dim=1) of NCHW sources, zero channels up to ``cpad``, NHWC: fp64 [B, H, W, cpad]."""
    x = torch.cat([s.to(F64) for s in srcs], 1)
    B, C, H, W = x.shape
    assert C <= cpad
    x = torch.cat((x, torch.zeros(B, cpad - C, H, W, dtype=F64)), 1)
    return x.permute(0, 2, 3, 1).contiguous()


def scatter_ref(src_nhwc, chans, H, W):
    """The backward of the gather: per channel range an NCHW fp64 [B, c, H, W] of the top-left H x W extent."""
    out, c0 = [], 0
    for c in chans:
        out.append(src_nhwc[:, :H, :W, c0:c0 + c].to(F64).permute(0, 3, 1, 2).contiguous())
        c0 += c
    return out


def tanh_bwd_ref(y, gy):
    """dq = gy * (1 - y^2) (NCHW fp64) and its per-channel sum."""
    dq = gy.to(F64) * (1.0 - y.to(F64) ** 2)
    return dq, dq.sum(dim=(0, 2, 3))


# ---------------------------------------------------------------- loss references (fp64)
def loss_elem(kind, p, t):
    p, t = p.to(F64), torch.as_tensor(t, dtype=F64)
    if kind == L1:
        return (p - t).abs()
    if kind == MSE:
        return (p - t) ** 2
    return p.clamp_min(0.0) - p * t + torch.log1p(torch.exp(-p.abs()))


def loss_dgrad(kind, p, t):
    """d elem / d p."""
    p, t = p.to(F64), torch.as_tensor(t, dtype=F64)
    if kind == L1:
        return torch.sign(p - t)
    if kind == MSE:
        return 2.0 * (p - t)
    return torch.sigmoid(p) - t


def loss_value(kind, p, t):
    """The mean loss in fp64 (a 0-d tensor)."""
    return loss_elem(kind, p, t).sum() / p.numel()


def value_f32(kind, p, t):
    """float32(fp64 mean): what a kernel whose partial sums are exact must return."""
    return loss_value(kind, p, t).to(F32)


def grad_scale(gout, wa, wb, n):
    """((gout * wa) * wb) / n of the fp32 arguments, in fp64."""
    return f32(gout) * f32(wa) * f32(wb) / float(n)


def grad_scale_f32(gout, wa=None, wb=None, n=1):
    """The same in fp32, one rounding per operation in the documented order (single-term form: gout / n)."""
    g = torch.tensor(gout, dtype=F32)
    if wa is not None:
        g = (g * torch.tensor(wa, dtype=F32)) * torch.tensor(wb, dtype=F32)
    return g / torch.tensor(float(n), dtype=F32)


def loss_grad_ref(kind, p, t, scale):
    return scale * loss_dgrad(kind, p, t)


def combine_d(v, l2, l3):
    """D1 = (fake1 + real1) * 0.5, D2 = (fake2 + real2) * 0.5, D = l2 * D1 + l3 * D2 on fp32 values v[0..3]: fp32,
    one rounding per operation, in that order -> (D, D1, D2)."""
    v = [torch.as_tensor(x, dtype=F32) for x in v]
    half, w0, w1 = torch.tensor(0.5, dtype=F32), torch.tensor(l2, dtype=F32), torch.tensor(l3, dtype=F32)
    d1 = (v[0] + v[1]) * half
    d2 = (v[2] + v[3]) * half
    return d1 * w0 + d2 * w1, d1, d2


def combine_g(v, l1, l2, l3):
    """G = ((data1 + l1 * data2) + l2 * G1) + l3 * G2 on fp32 values, one rounding per operation."""
    v = [torch.as_tensor(x, dtype=F32) for x in v]
    w = [torch.tensor(x, dtype=F32) for x in (l1, l2, l3)]
    return ((v[0] + v[1] * w[0]) + v[2] * w[1]) + v[3] * w[2]


# ---------------------------------------------------------------- weight-pack reference
PACK_CONV_FWD, PACK_CONV_DGRAD, PACK_CONV_S1_DGRAD, PACK_CONVT_FWD, PACK_CONVT_DGRAD = 0, 1, 2, 3, 4
PACK_MODES = (0, 1, 2, 3, 4)
PHASED = (PACK_CONV_DGRAD, PACK_CONVT_FWD)
N_IS_P = (PACK_CONV_FWD, PACK_CONVT_DGRAD)


def pack_ref(mode, W, n_pad, c_pad):
    """out[phase][N_pad][tap][C_pad] of a weight W[P][Q][4][4] from the layout comment of include/stcgan_hip.h:
    n = p for CONV_FWD / CONVT_DGRAD and n = q for the other modes (c the other index); the unphased modes have one
    phase and tap = kh * 4 + kw; the phased ones have phase = ph * 2 + pw and 4 taps with kh = (1 - ph) + 2 (t >> 1),
    kw = (1 - pw) + 2 (t & 1), i.e. ph = 1 - kh % 2, t = 2 (kh / 2) + kw / 2.  Every other entry is zero."""
    W = W.to(F64)
    P, Q = W.shape[0], W.shape[1]
    phased = mode in PHASED
    out = torch.zeros((4 if phased else 1, n_pad, 4 if phased else 16, c_pad), dtype=F64)
    p, q, kh, kw = (torch.from_numpy(a) for a in np.indices((P, Q, 4, 4)))
    n, c = (p, q) if mode in N_IS_P else (q, p)
    assert int(n.max()) < n_pad and int(c.max()) < c_pad
    if phased:
        z = (1 - kh % 2) * 2 + (1 - kw % 2)
        t = (kh // 2) * 2 + kw // 2
    else:
        z = torch.zeros_like(kh)
        t = kh * 4 + kw
    out[z, n, t, c] = W[p, q, kh, kw]
    return out


def bf16_exact_ints(count):
    """The first ``count`` positive integers that bf16 holds exactly (8 significant bits), ascending: 1..256, then
    258, 260, ..."""
    vals, e = list(range(1, 128)), 0
    while len(vals) < count:
        vals += [m << e for m in range(128, 256)]
        e += 1
    return torch.tensor(vals[:count], dtype=F64)


def pack_weights(P, Q, seed, unique=True):
    """Integer weights, exact in bf16, in a seeded random order.  ``unique``: every element differs from every other
    one (+-1, +-2, ...; below 2^8 in magnitude while P*Q*16 <= 510), so that any misplaced element is seen.  Without it
    (tensors with more elements than bf16 has values) the magnitudes repeat with an odd period, so neighbouring taps,
    rows and columns still differ."""
    n = P * Q * 16
    g = torch.Generator().manual_seed(int(seed))
    if unique:
        mag = bf16_exact_ints((n + 1) // 2)
        v = torch.cat((mag, -mag))[:n]
        v = v[torch.randperm(n, generator=g)]
        assert len(set(v.tolist())) == n
    else:
        mag = bf16_exact_ints(12799)
        k = torch.arange(n)
        v = mag[k % 12799] * (1 - 2 * ((k // 12799) % 2)).to(F64)
    v = v.reshape(P, Q, 4, 4)
    assert torch.equal(v.to(BF16).to(F64), v) and torch.equal(v.to(F32).to(F64), v) and float(v.abs().min()) >= 1
    return v


# ---------------------------------------------------------------- exactly-summable operands
def quarters(shape, seed, lo, hi):
    """fp64 multiples of 1/4 uniform in [lo, hi]."""
    g = torch.Generator().manual_seed(int(seed))
    return torch.randint(int(lo * 4), int(hi * 4) + 1, tuple(shape), generator=g).to(F64) / 4.0


def require_loss_exact(elem):
    """Every element loss is a multiple of 1/16 and at most 64, so a 4096-element block sums to fewer than 2^24 units
    of 1/16: every fp32 partial sum of any order is exact."""
    assert bool((elem * 16 == (elem * 16).round()).all()), "loss elements must be multiples of 1/16"
    assert float(elem.max()) <= 64.0, float(elem.max())
    assert float(elem.max()) * 16 * LOSS_PER_BLOCK < LIMIT


def loss_operands(kind, n, seed, const=None, runs=True):
    """(p, t) for an L1 / MSE term: p and t multiples of 1/4 in [-4, 4] (|p - t| <= 8); with ``const`` t is that
    constant (0, 1 or -1).  L1 with ``runs``: stretches with p == t, where the gradient must be exactly 0 (one at the
    start, one across the first block boundary, one just before the end when n allows).  The last element always
    has a nonzero loss: where n = k * 4096 + 1 it is a partial sum of its own, and a zero there would hide a last
    block that is never added."""
    p = quarters((n,), seed, -4, 4)
    if const is not None:
        assert float(const) * 4 == round(float(const) * 4)
        t = torch.full((n,), float(const), dtype=F64)
        if p[-1] == t[-1]:
            p[-1] = p[-1] - 2.0
    else:
        t = quarters((n,), seed + 1, -4, 4)
        if kind == L1 and runs and n >= 8:
            for a, b in ((0, 3), (min(n, LOSS_PER_BLOCK) - 3, min(n - 1, LOSS_PER_BLOCK + 3)), (n - 3, n - 1)):
                t[a:b] = p[a:b]
        if p[-1] == t[-1]:
            t[-1] = p[-1] - 1.0 if p[-1] > 0 else p[-1] + 1.0
    assert float((p - t).abs().max()) <= 8.0 and p[-1] != t[-1]
    require_loss_exact(loss_elem(kind, p, t))
    return p, t


def tanh_operands(B, C, H, W, seed):
    """y: multiples of 1/8 in (-1, 1); gy: multiples of 1/4 in [-4, 4].  1 - y^2 is a multiple of 1/64 and
    dq = gy * (1 - y^2) a multiple of 1/256 of magnitude <= 4: exact in fp32 (at most 11 significant bits, so the
    bf16 output is a real rounding)."""
    g = torch.Generator().manual_seed(int(seed))
    y = torch.randint(-7, 8, (B, C, H, W), generator=g).to(F64) / 8.0
    gy = quarters((B, C, H, W), seed + 1, -4, 4)
    dq = tanh_bwd_ref(y, gy)[0]
    assert bool((dq * 256 == (dq * 256).round()).all()) and float(y.abs().max()) < 1
    assert torch.equal(dq.to(F32).to(F64), dq)
    return y, gy


def require_tanh_exact(dq, chunk_pixels):
    """Every fp32 sum over one chunk's pixels is an integer number of 1/256 below 2^24 whatever its order."""
    assert chunk_pixels * float(dq.abs().max()) * 256 < LIMIT, (chunk_pixels, float(dq.abs().max()))


def bce_inputs(n, seed):
    """A Gaussian bulk (fp32 values) with BCE_FIXED written at the start, in the middle and at the end."""
    k = len(BCE_FIXED)
    assert n >= 4 * k
    g = torch.Generator().manual_seed(int(seed))
    x = torch.randn(n, generator=g, dtype=F32).to(F64)
    fixed = torch.tensor(BCE_FIXED, dtype=F32).to(F64)
    for a in (0, (n - k) // 2, n - k):
        x[a:a + k] = fixed
    return x


def bce_fixed_positions(n):
    k = len(BCE_FIXED)
    return [a + i for a in (0, (n - k) // 2, n - k) for i in range(k)]


# ---------------------------------------------------------------- derived bounds
def bce_parts(x, t):
    x, t = x.to(F64), torch.as_tensor(t, dtype=F64)
    return x.clamp_min(0.0).abs(), (x * t).abs(), torch.log1p(torch.exp(-x.abs()))


def bce_elem_bound(x, t):
    """|fp32 element - fp64 element| <= (3 + U) EPS (|max(x, 0)| + |x t| + |log1p term|) + TINY: the product, the
    subtraction and the addition round once each relative to magnitudes that the sum of the three terms bounds,
    expf + log1pf contribute U EPS of the log1p term; a log1p term below the smallest normal number (|x| > 87.3) is
    outside the format's relative precision and carries an absolute error of up to TINY instead."""
    a, b, c = bce_parts(x, t)
    return (3.0 + U) * EPS * (a + b + c) + TINY


def bce_mean_bound(x, t):
    """The per-element bounds, plus (16 + 8) EPS sum |elem| for the 16 serial and 8 tree fp32 additions of a block
    (the block sums are added in fp64), all over n, plus the final rounding to fp32.  The elements the block adds
    are the finished fp32 ones, of magnitude at most |elem| + the element's own bound; the final rounding is
    relative to the computed mean, at most |mean| + the error accumulated so far."""
    n = x.numel()
    elem = loss_elem(BCE, x, t)
    eb = bce_elem_bound(x, t)
    tot = (eb.sum() + (BLOCK_SERIAL + BLOCK_TREE) * EPS * (elem.abs() + eb).sum()) / n
    return tot + EPS * (float(elem.sum().abs() / n) + tot)


def grad_bound(kind, p, t, scale, r):
    """|fp32 gradient - fp64 gradient| <= (r + 1) EPS |gradient|, r the fp32 roundings of the documented formula (2:
    gout / n and the product, single-term; 4: the ((gout wa) wb) / n chain and the product, multi-term).  BCE adds the
    sigmoid's error U EPS s + TINY times |scale|, absolute because s - t cancels (TINY: where exp(-x) overflows, or
    s is below the smallest normal number, s is known only to that absolute error), and TINY for a gradient that
    is itself below the normal range."""
    ref = loss_grad_ref(kind, p, t, scale).abs()
    b = (r + 1) * EPS * ref + TINY
    if kind == BCE:
        s = torch.sigmoid(p.to(F64))
        b = b + abs(scale) * (U * EPS * s + TINY)
    return b


def measure_u(x):
    """Worst error, in EPS relative to the result, of torch's fp32 CPU log1p(exp(-|x|)) and 1 / (1 + exp(-x))
    against fp64, over the normal-range results."""
    x32 = x.to(F32)
    x = x32.to(F64)
    worst = 0.0
    for got, ref in ((torch.log1p(torch.exp(-x32.abs())), torch.log1p(torch.exp(-x.abs()))),
                     (1.0 / (1.0 + torch.exp(-x32)), torch.sigmoid(x))):
        m = ref >= TINY
        worst = max(worst, float((((got.to(F64) - ref).abs() / ref)[m]).max() / EPS))
    return worst
