"""stc_in_fwd / stc_in_bwd (csrc/inorm.hip) against fp64 references of the same operations.

Every reference is evaluated on the CPU in fp64 from exactly the values uploaded (fp32, or bf16-rounded
activations; fp32 gamma / beta / mean / rstd).  Shapes: the planes 1x2 ... 127x129 of the issue with 1, 3 and 64
channel vectors and B of 1 and 3, thinned so that every regime of stc_in_plan (tiny / resident / streamed) meets
every layout (dense, low / high half of a 2C-wide buffer, cropped), plus the plane sizes on either side of each
regime threshold, found by probing stc_in_plan.  NaN fills everything outside the views and must stay.

Bounds (EPS = 2^-23, m = the accumulation length stc_in_plan reports + 8 for the roundings inside one term),
never taken from what the kernels return:
  plane sum      within m * EPS * sum|terms|
  mean           the sum runs over x - shift with the shift an element of the plane, |shift| <= max|x|:
                 d_mean = m * EPS * (mean|x| + max|x|) + 4 * EPS * |mean|
  variance       the centred sum around a mean that is off by at most d_mean, merged over chunks:
                 d_var = m * EPS * (var + d_mean^2) + 2 * sqrt(var) * d_mean + 2 * d_mean^2
  rstd           d_rstd = d_var / (2 * (var + eps - d_var)^1.5) + 4 * EPS * rstd
  n              d_n = |gamma| * (d_mean * rstd + |x - mean| * d_rstd) + 4 * EPS * (|xhat * gamma| + |beta| + |n|)
  y = act(n, s)  act is Lipschitz with constant max(1, |s|): d_y = max(1, |s|) * d_n, then round-to-nearest-even for
                 bf16 (8 significant bits: relative 2^-8)
  backward       from the uploaded mean / rstd: s1 = sum dn within m * EPS * sum|dn|, s2 = sum dn * xhat within
                 m * EPS * sum|dn * xhat|; dx = gamma * rstd * (dn - s1/P - xhat * s2/P) within
                 |gamma * rstd| * (d_s1/P + |xhat| * d_s2/P) + 8 * EPS * |gamma * rstd| * (|dn| + |s1|/P + |xhat * s2|/P),
                 then the bf16 rounding; dgamma / dbeta = the sums over b of s2 / s1, within the sum of their bounds
                 + B * EPS * sum|.|.  The incoming gradients are zeroed where |n| is within 64 * EPS of the magnitude of its
                 terms (act' is discontinuous at 0), so a rounding of n cannot flip a term.
A raw-moment variance (E[x^2] - E[x]^2) misses d_rstd on the cancellation planes (mean 64, standard deviation 1/16)
by more than an order of magnitude.

Measured worst error / bound on an MI355X: see the docstrings of the tests (every printed line: profiles/inorm/).
"""

import numpy as np
import pytest
import torch

from stcgan_amd import _lib as L
from stcgan_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, BF16 = torch.float32, torch.bfloat16
NAN = float("nan")
EPS32 = 2.0 ** -23
IN_EPS = float(np.float32(1e-5))
LAYOUTS = ["dense", "lo", "hi", "crop"]
# (B, H, W, channel vectors)
SHAPES = [(3, 1, 2, 3), (3, 2, 2, 64), (1, 3, 3, 1),
          (3, 8, 8, 64), (1, 5, 13, 3), (3, 31, 31, 3), (1, 64, 64, 1), (1, 8, 8, 1),
          (3, 31, 31, 64), (1, 64, 64, 3), (1, 17, 241, 1), (3, 17, 241, 3), (1, 127, 129, 3), (1, 64, 64, 64)]
WORST = {}


def dtname(dt):
    return "f32" if dt == F32 else "bf16"


def note(key, err, bound):
    err, bound = torch.as_tensor(err, dtype=torch.float64), torch.as_tensor(bound, dtype=torch.float64)
    ratio = float((err / bound.clamp_min(1e-300)).max())
    WORST[key] = max(WORST.get(key, 0.0), ratio)
    print(f"[instance_norm] {key}: error/bound {ratio:.4f}")
    assert bool((err <= bound).all()), f"{key}: error/bound {ratio:.4f} (max err {float(err.max()):.3e})"


def stored(t, dt):
    return t.float() if dt == F32 else t.float().to(BF16).float()


def round_bound(ref, d, dt):
    """Bound on a stored element whose fp32 value is within d of ref."""
    if dt == F32:
        return d + EPS32 * ref.abs()
    return d + (ref.abs() + d) * 2.0 ** -8 * 1.001 + 1e-38


def plan(dt, B, H, W, C):
    return ops.in_plan(B, H, W, C, dt)


def thresholds(dt, cv):
    """Plane widths (H = 1) on either side of each regime change of stc_in_plan for cv channel vectors."""
    C = cv * ops.vec(dt)
    out, prev = [], plan(dt, 1, 1, 2, C)[0]
    w = 2
    while prev < 2 and w < (1 << 16):
        lo, hi = w, w
        while plan(dt, 1, 1, hi, C)[0] == prev:  # gallop, then bisect
            lo, hi = hi, hi * 2
        while hi - lo > 1:
            mid = (lo + hi) // 2
            lo, hi = (mid, hi) if plan(dt, 1, 1, mid, C)[0] == prev else (lo, mid)
        out += [lo, hi]
        prev, w = plan(dt, 1, 1, hi, C)[0], hi
    return out


CASES = [pytest.param(s, id="x".join(map(str, s))) for s in SHAPES] + ["thresholds-cv1", "thresholds-cv64"]


def shapes_of(case, dt):
    """The shapes of one parametrised case: a shape of the list, or the four plane sizes around the two thresholds."""
    if isinstance(case, tuple):
        return [case]
    cv = int(case.rsplit("cv", 1)[1])
    return [(1 + (i % 2) * 2, 1, w, cv) for i, w in enumerate(thresholds(dt, cv))]


def all_shapes(dt):
    return [sv for c in SHAPES + ["thresholds-cv1", "thresholds-cv64"] for sv in shapes_of(c, dt)]


# ---------------------------------------------------------------- layouts (as tests/test_gpu_bn_family.py)
def _full(shape, mode):
    B, H, W, C = shape
    return {"dense": (B, H, W, C), "lo": (B, H, W, 2 * C), "hi": (B, H, W, 2 * C), "crop": (B, H + 1, W + 3, C)}[mode]


def _region(buf, shape, mode):
    B, H, W, C = shape
    if mode == "dense":
        return buf
    if mode in ("lo", "hi"):
        c0 = 0 if mode == "lo" else C
        return buf[..., c0:c0 + C]
    return buf[:, :H, :W, :]


def _view(buf, shape, mode):
    B, H, W, C = shape
    if mode == "dense":
        return L.nhwc_view(buf)
    if mode in ("lo", "hi"):
        return L.nhwc_view(buf, 0 if mode == "lo" else C)
    return L.nhwc_view(buf, 0, H, W)


def new_buf(shape, dt, mode):
    return torch.full(_full(shape, mode), NAN, device=DEV, dtype=dt)


def place(vals, dt, mode):
    shape = tuple(vals.shape)
    buf = new_buf(shape, dt, mode)
    _region(buf, shape, mode).copy_(vals.to(dt))
    return buf, _view(buf, shape, mode)


def read_back(buf, shape, mode):
    got = _region(buf, shape, mode).detach().clone()
    if mode != "dense":
        rest = buf.detach().clone()
        _region(rest, shape, mode).fill_(NAN)
        assert bool(torch.isnan(rest).all()), f"{mode}: an element outside the view was written"
    return got.cpu().double()


class Norm:
    """Stand-in of nn.InstanceNorm2d for ops.in_forward / in_backward: eps and optional randomised weight / bias."""

    def __init__(self, C, affine, seed):
        self.eps = 1e-5
        self.weight = self.bias = None
        self.g64 = torch.ones(C, dtype=torch.float64)
        self.b64 = torch.zeros(C, dtype=torch.float64)
        if affine:
            g = torch.Generator().manual_seed(seed)
            w = torch.rand(C, generator=g) + 0.5
            w[1::3] *= -1.0
            b = torch.randn(C, generator=g) * 0.3
            self.weight, self.bias = w.to(DEV), b.to(DEV)
            self.g64, self.b64 = w.double(), b.double()


def values(shape, dt, seed, kind="normal"):
    """Plane values [B, H, W, C] as the storage type holds them (fp32 on the CPU)."""
    g = torch.Generator().manual_seed(seed)
    B, H, W, C = shape
    if kind == "cancel":  # mean 64, standard deviation 1/16
        v = 64.0 + torch.randn(shape, generator=g) / 16.0
    elif kind == "const":
        v = (torch.randn((B, 1, 1, C), generator=g) * 3.0).expand(shape).clone()
    else:
        v = torch.randn(shape, generator=g) * (0.5 + torch.rand((B, 1, 1, C), generator=g) * 2.0) \
            + torch.randn((B, 1, 1, C), generator=g) * 2.0
    return stored(v, dt)


# ---------------------------------------------------------------- fp64 references + bounds
def fwd_ref(x, norm, m):
    """x fp64 [B, H, W, C] -> dict of reference values and bounds (module docstring)."""
    P = x.shape[1] * x.shape[2]
    mean = x.mean((1, 2), keepdim=True)
    var = ((x - mean) ** 2).mean((1, 2), keepdim=True)
    rstd = 1.0 / torch.sqrt(var + IN_EPS)
    d_mean = m * EPS32 * (x.abs().mean((1, 2), keepdim=True) + x.abs().amax((1, 2), keepdim=True)) \
        + 4 * EPS32 * mean.abs()
    d_var = m * EPS32 * (var + d_mean ** 2) + 2 * var.sqrt() * d_mean + 2 * d_mean ** 2
    assert bool((d_var < 0.5 * (var + IN_EPS)).all()), "bound degenerate: the variance bound exceeds half the variance"
    d_rstd = d_var / (2 * (var + IN_EPS - d_var) ** 1.5) + 4 * EPS32 * rstd
    xhat = (x - mean) * rstd
    n = xhat * norm.g64 + norm.b64
    d_n = norm.g64.abs() * (d_mean * rstd + (x - mean).abs() * d_rstd) \
        + 4 * EPS32 * ((xhat * norm.g64).abs() + norm.b64.abs() + n.abs())
    return dict(P=P, mean=mean, rstd=rstd, d_mean=d_mean, d_rstd=d_rstd, n=n, d_n=d_n, xhat=xhat)


def act64(n, s):
    return torch.where(n > 0, n, n * s)


def run_fwd(shape, dt, mode, x_cpu, norm, slopes, crop_apply=False):
    """One stc_in_fwd: x in layout ``mode`` (crop: the statistics run over the whole (H+1) x (W+3) buffer and the
    outputs cover its top-left H x W).  Returns (mean, rstd, [outputs fp64], raw output buffers)."""
    B, H, W, C = shape
    if mode == "crop":
        xbuf = x_cpu.to(dt).to(DEV)  # [B, H+1, W+3, C], all of it valid
        xv, av = L.nhwc_view(xbuf), L.nhwc_view(xbuf, 0, H, W)
    else:
        xbuf, xv = place(x_cpu, dt, mode)
        av = xv
    outs = [new_buf(shape, dt, mode) for _ in slopes]
    ov = [_view(o, shape, mode) for o in outs]
    mean, rstd = ops.in_forward(B, xv, C, dt, norm, av, ov[0], slopes[0], ov[1] if len(slopes) > 1 else None,
                                slopes[1] if len(slopes) > 1 else 0.0)
    torch.cuda.synchronize()
    return mean, rstd, [read_back(o, shape, mode) for o in outs], outs


def check_fwd(tag, shape, dt, mode, x_cpu, norm, slopes, streams=False):
    B, H, W, C = shape
    sh_stats = tuple(x_cpu.shape)
    m = plan(dt, B, sh_stats[1], sh_stats[2], C)[3] + 8
    r = fwd_ref(x_cpu.double(), norm, m)
    mean, rstd, ys, raw = run_fwd(shape, dt, mode, x_cpu, norm, slopes)
    note(f"{tag} mean", (mean.cpu().double() - r["mean"].reshape(B, C)).abs(), r["d_mean"].reshape(B, C))
    note(f"{tag} rstd", (rstd.cpu().double() - r["rstd"].reshape(B, C)).abs(), r["d_rstd"].reshape(B, C))
    n, d_n = r["n"][:, :H, :W], r["d_n"][:, :H, :W]
    for y, s in zip(ys, slopes):
        s = float(np.float32(s))
        ref = act64(n, s)
        note(f"{tag} y(slope {s:g})", (y - ref).abs(), round_bound(ref, max(1.0, abs(s)) * d_n, dt))
    if streams:  # the same call again, and on a side stream: bit-identical
        mean2, rstd2, _, raw2 = run_fwd(shape, dt, mode, x_cpu, norm, slopes)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            mean3, rstd3, _, raw3 = run_fwd(shape, dt, mode, x_cpu, norm, slopes)
        torch.cuda.synchronize()
        for a, b_, c in zip([mean, rstd] + raw, [mean2, rstd2] + raw2, [mean3, rstd3] + raw3):
            assert torch.equal(a.view(torch.uint8), b_.view(torch.uint8)), f"{tag}: a second call differs"
            assert torch.equal(a.view(torch.uint8), c.view(torch.uint8)), f"{tag}: the side-stream call differs"
    return r


def stats_shape(shape, mode):
    B, H, W, C = shape
    return (B, H + 1, W + 3, C) if mode == "crop" else shape


def _mk(shape_v, dt):
    B, H, W, cv = shape_v
    return (B, H, W, cv * ops.vec(dt))


# ================================================================ forward
@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("mode", LAYOUTS)
@pytest.mark.parametrize("dt", [F32, BF16], ids=dtname)
def test_forward(dt, mode, case):
    """Every shape of the cross: two outputs (LeakyReLU 0.2 + ReLU) with randomised gamma / beta, one output (identity)
    without; the first form also twice and on a side stream (bit-identical).
    Measured worst error / bound on an MI355X: fp32 mean 0.034, rstd 0.015, outputs 0.030; bf16 mean 0.027, rstd 0.019,
    outputs 0.99 (the bound there is the half-ulp of the bf16 rounding itself)."""
    for i, sv in enumerate(shapes_of(case, dt)):
        shape = _mk(sv, dt)
        tag = f"fwd {dtname(dt)} {mode} {'x'.join(map(str, sv))}"
        x = values(stats_shape(shape, mode), dt, 100 + i)
        check_fwd(tag + " affine", shape, dt, mode, x, Norm(shape[3], True, 7 + i), (0.2, 0.0), streams=True)
        check_fwd(tag + " plain", shape, dt, mode, x, Norm(shape[3], False, 0), (1.0,))


@pytest.mark.parametrize("hw", [(31, 31), (64, 64)], ids=lambda v: f"{v[0]}x{v[1]}")
@pytest.mark.parametrize("cv", [3, 64])
def test_forward_cancellation(hw, cv):
    """Planes with mean 64 and standard deviation 1/16, fp32: the same bound formula as every other case (a raw-moment
    variance misses it: E[x^2] ~ 4096 carries an absolute error of m * EPS * 4096 against a variance of 1/256).
    Measured worst error / bound on an MI355X: mean 0.012, rstd 0.0004, outputs 0.012."""
    shape = (2, hw[0], hw[1], cv * 4)
    x = values(shape, F32, 5, "cancel")
    for affine in (False, True):
        check_fwd(f"fwd cancel {hw[0]}x{hw[1]} cv{cv} affine={affine}", shape, F32, "dense", x,
                  Norm(shape[3], affine, 3), (0.2, 0.0))


@pytest.mark.parametrize("dt", [F32, BF16], ids=dtname)
def test_constant_plane(dt):
    """A constant plane: the output within the bound of act(beta), and with a plane-constant incoming gradient dx
    within the bound of 0.  Measured worst error / bound on an MI355X: fp32 outputs 0.0003, dx 0.034 (mean exact);
    bf16 outputs 0.72 (the bf16 rounding of act(beta))."""
    for sv in [(2, 2, 2, 3), (2, 8, 8, 64), (2, 31, 31, 3), (1, 64, 64, 3)]:
        shape = _mk(sv, dt)
        B, H, W, C = shape
        x = values(shape, dt, 9, "const")
        norm = Norm(C, True, 11)
        r = check_fwd(f"const {dtname(dt)} {sv}", shape, dt, "dense", x, norm, (0.2,))
        assert float((r["n"] - norm.b64).abs().max()) < 1e-9  # the reference output is beta
        g = stored((torch.randn((B, 1, 1, C), generator=torch.Generator().manual_seed(3))).expand(shape).clone(), dt)
        dx, dg, db, ref = run_bwd(shape, dt, "dense", x, norm, [(g, 1.0)], r["mean"], r["rstd"])
        m = plan(dt, B, H, W, C)[3] + 8
        k = (norm.g64 * ref["rstd"]).abs()
        bound = k * (m * EPS32 * g.double().abs().sum((1, 2), keepdim=True) / (H * W)) + 8 * EPS32 * k * 2 * g.double().abs()
        note(f"const {dtname(dt)} {sv} dx", dx.abs(), round_bound(torch.zeros_like(dx), bound, dt))


# ================================================================ backward
def run_bwd(shape, dt, mode, x_cpu, norm, grads, mean64, rstd64, keep=False):
    """One stc_in_bwd from the fp32-rounded reference mean / rstd.  grads: [(g values, slope)].  Returns
    (dx fp64, dgamma, dbeta, reference dict of the uploaded statistics)."""
    B, H, W, C = shape
    mean32 = mean64.reshape(B, C).float().to(DEV)
    rstd32 = rstd64.reshape(B, C).float().to(DEV)
    _, xv = place(x_cpu, dt, mode)
    gv = [place(g, dt, mode)[1] for g, _ in grads]
    dxb = new_buf(shape, dt, mode)
    kw = {}
    if len(grads) > 1:
        kw = dict(g2=gv[1], s2=grads[1][1])
    dg, db = ops.in_backward(B, xv, C, dt, _view(dxb, shape, mode), norm, (mean32, rstd32), g1=gv[0], s1=grads[0][1],
                             **kw)
    torch.cuda.synchronize()
    ref = dict(mean=mean32.cpu().double().reshape(B, 1, 1, C), rstd=rstd32.cpu().double().reshape(B, 1, 1, C))
    out = (read_back(dxb, shape, mode), None if dg is None else dg.cpu().double(),
           None if db is None else db.cpu().double(), ref)
    return out + ((dxb, dg, db),) if keep else out


def check_bwd(tag, shape, dt, mode, seed, norm, slopes, streams=False):
    B, H, W, C = shape
    P = H * W
    m = plan(dt, B, H, W, C)[3] + 8
    x = values(shape, dt, seed)
    fr = fwd_ref(x.double(), norm, m)
    gen = torch.Generator().manual_seed(seed + 1)
    # the statistics as uploaded (fp32), and n from them; gradients zeroed where a rounding of n could flip act'
    mean = fr["mean"].float().double()
    rstd = fr["rstd"].float().double()
    xhat = (x.double() - mean) * rstd
    n = xhat * norm.g64 + norm.b64
    safe = n.abs() > 64 * EPS32 * ((xhat * norm.g64).abs() + norm.b64.abs() + 1e-30)
    grads = [(stored(torch.randn(shape, generator=gen), dt) * safe, float(np.float32(s))) for s in slopes]
    dn = sum(g.double() * torch.where(n > 0, 1.0, s) for g, s in grads)
    s1 = dn.sum((1, 2), keepdim=True)
    s2 = (dn * xhat).sum((1, 2), keepdim=True)
    d_s1 = m * EPS32 * dn.abs().sum((1, 2), keepdim=True)
    d_s2 = m * EPS32 * (dn * xhat).abs().sum((1, 2), keepdim=True)
    k = norm.g64 * rstd
    dx_ref = k * (dn - s1 / P - xhat * s2 / P)
    d_dx = k.abs() * (d_s1 / P + xhat.abs() * d_s2 / P) \
        + 8 * EPS32 * k.abs() * (dn.abs() + s1.abs() / P + (xhat * s2).abs() / P)
    res = run_bwd(shape, dt, mode, x, norm, grads, mean, rstd, keep=True)
    dx, dg, db = res[0], res[1], res[2]
    note(f"{tag} dx", (dx - dx_ref).abs(), round_bound(dx_ref, d_dx, dt))
    if norm.weight is not None:
        note(f"{tag} dbeta", (db - s1.sum(0).reshape(C)).abs(),
             (d_s1.sum(0) + B * EPS32 * s1.abs().sum(0)).reshape(C) + 1e-30)
        note(f"{tag} dgamma", (dg - s2.sum(0).reshape(C)).abs(),
             (d_s2.sum(0) + B * EPS32 * s2.abs().sum(0)).reshape(C) + 1e-30)
    else:
        assert dg is None and db is None
    if streams:
        again = run_bwd(shape, dt, mode, x, norm, grads, mean, rstd, keep=True)[4]
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            other = run_bwd(shape, dt, mode, x, norm, grads, mean, rstd, keep=True)[4]
        torch.cuda.synchronize()
        for a, b_, c in zip(res[4], again, other):
            if a is not None:
                assert torch.equal(a.view(torch.uint8), b_.view(torch.uint8)), f"{tag}: a second call differs"
                assert torch.equal(a.view(torch.uint8), c.view(torch.uint8)), f"{tag}: the side-stream call differs"


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("mode", LAYOUTS)
@pytest.mark.parametrize("dt", [F32, BF16], ids=dtname)
def test_backward(dt, mode, case):
    """Every shape of the cross: g1 + g2 (ReLU + LeakyReLU 0.2) with randomised gamma / beta (dx, dgamma, dbeta; also
    twice and on a side stream, bit-identical), g1 only (LeakyReLU) without.
    Measured worst error / bound on an MI355X: fp32 dx 0.13, dgamma 0.072, dbeta 0.061; bf16 dx 0.99 (the half-ulp of the
    bf16 rounding), dgamma 0.063, dbeta 0.052."""
    for i, sv in enumerate(shapes_of(case, dt)):
        shape = _mk(sv, dt)
        tag = f"bwd {dtname(dt)} {mode} {'x'.join(map(str, sv))}"
        check_bwd(tag + " affine", shape, dt, mode, 300 + i, Norm(shape[3], True, 17 + i), (0.0, 0.2), streams=True)
        check_bwd(tag + " plain", shape, dt, mode, 400 + i, Norm(shape[3], False, 0), (0.2,))


@pytest.mark.parametrize("dt", [F32, BF16], ids=dtname)
def test_every_regime_in_the_cross(dt):
    """The shape list puts each regime under test (every shape runs under every layout), and both sides of each
    threshold the plan query reveals are in it."""
    regimes = {}
    for sv in all_shapes(dt):
        regimes.setdefault(plan(dt, *_mk(sv, dt))[0], []).append(sv)
    assert sorted(regimes) == [0, 1, 2], regimes
    for cv in (1, 64):
        th = thresholds(dt, cv)
        assert len(th) == 4
        C = cv * ops.vec(dt)
        assert [plan(dt, 1, 1, w, C)[0] for w in th] == [0, 1, 1, 2]
        assert th[1] == th[0] + 1 and th[3] == th[2] + 1
    # a multi-slab resident shape and a multi-slab streamed shape (64 vectors: more than one slab)
    assert any(plan(dt, *_mk(sv, dt))[0] == 1 and plan(dt, *_mk(sv, dt))[1] < _mk(sv, dt)[3] for sv in SHAPES)
    assert any(plan(dt, *_mk(sv, dt))[0] == 2 and plan(dt, *_mk(sv, dt))[1] < _mk(sv, dt)[3] for sv in SHAPES)


def test_missing_workspace_is_refused():
    lib = L.lib()
    x = torch.zeros((1, 127, 129, 8), device=DEV)
    v = L.nhwc_view(x)
    st = torch.zeros((1, 8), device=DEV)
    rc = lib.stc_in_fwd(0, 1, v, 8, None, None, 1e-5, L.ptr(st), L.ptr(st), v, v, 0.0, L.NULL_VIEW, 0.0, None, 0,
                        L.stream())
    assert rc != 0 and b"workspace" in lib.stc_last_error()
    rc = lib.stc_in_bwd(0, 1, v, 8, None, None, L.ptr(st), L.ptr(st), v, 0.0, L.NULL_VIEW, 0.0, v, None, None, None,
                        0, L.stream())
    assert rc != 0 and b"workspace" in lib.stc_last_error()
