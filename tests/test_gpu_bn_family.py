"""The BatchNorm kernel family of csrc/bn.hip against fp64 references of the same operations.

chan_stats / bn_finalize / bn_eval_table / bn_apply / bn_bwd_reduce / bn_bwd_apply / chan_sum are what the fused
epilogue tests, the dropout tests and the stem tests compare against, so they are pinned here on their own: every
reference is evaluated on the CPU in fp64 (the chunk merge in long double) from exactly the values uploaded to the
device -- fp32 or bf16-rounded activations and fp32 tables -- at the shapes that select each host / kernel branch:
thread layouts CG = C/N of 1, 3, 24 and 256, the chunk-count groups of both finalize kernels, empty tail chunks
(P = 65537), the streaming (DENSE) and the general-addressing element-wise forms, channel-offset and cropped views
with a NaN surround, both grid caps, and both pixel-index divisions.

Bounds come from the accumulation lengths and the number formats, never from what the kernels return (EPS32 = 2^-23):
a chunk holds per = ceil(P / nch) pixels and each thread sums ceil(per / RL) of them (RL = 256 // CG pixel lanes),
then RL lane totals are added, so a per-channel fp32 sum is within m * EPS32 * sum|terms| of the exact one with
m = ceil(per / RL) + RL + 8 (the 8: the roundings inside one term).  Everything downstream of the fp64 merge is
within 4 * EPS32 of the sum of the absolute values of the terms that form it.  Element-wise results are within one
fp32 ulp (fp32) or are the round-to-nearest-even bf16 of a value within one fp32 ulp (bf16).

Measured worst error / bound over this file on an MI355X: see each test's docstring.
"""
import functools
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from stcgan_amd import _lib as L
from stcgan_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, BF16 = torch.float32, torch.bfloat16
NAN = float("nan")
EPS32 = 2.0 ** -23
MOM = float(np.float32(0.1))      # momentum and eps as the C-ABI receives them (float)
BN_EPS = float(np.float32(1e-5))

WORST = {}


def note(key, err, bound):
    """Largest error / bound of one quantity (printed, so that a run with -s records the measured ratios);
    asserts err <= bound element-wise."""
    err, bound = torch.as_tensor(err, dtype=torch.float64), torch.as_tensor(bound, dtype=torch.float64)
    ratio = float((err / bound.clamp_min(1e-300)).max())
    WORST[key] = max(WORST.get(key, 0.0), ratio)
    print(f"[bn_family] {key}: error/bound {ratio:.4f}")
    assert bool((err <= bound).all()), f"{key}: error/bound {ratio:.4f} (max err {float(err.max()):.3e})"


def dtname(dt):
    return "f32" if dt == F32 else "bf16"


def stored(t, dt):
    """fp32 CPU values as the storage type holds them."""
    return t.float() if dt == F32 else t.float().to(BF16).float()


def ulp32(t):
    a = np.abs(t.detach().double().numpy().astype(np.float32))
    return torch.from_numpy(np.spacing(a).astype(np.float64))


def slope32(s):
    return float(np.float32(s))


def stat_chunks(P):
    return max(1, min(1024, (P + 63) // 64))


def acc_len(P, C, dt):
    """m of the module docstring for a per-channel reduction over P pixels of C channels."""
    rl = 256 // (C // ops.vec(dt))
    per = -(-P // stat_chunks(P))
    return -(-per // rl) + rl + 8


# ---------------------------------------------------------------- layouts
# dense: the tensor itself; lo / hi: channels [0, C) / [C, 2C) of a 2C-wide buffer; crop: the top-left H x W of a
# [B, H+1, W+3, C] buffer.  Everything outside the view is NaN.
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
    B, H, W, C = shape
    full = {"dense": (B, H, W, C), "lo": (B, H, W, 2 * C), "hi": (B, H, W, 2 * C), "crop": (B, H + 1, W + 3, C)}[mode]
    return torch.full(full, NAN, device=DEV, dtype=dt)


def place(vals, dt, mode):
    """Upload the CPU values [B, H, W, C] in the layout ``mode``: (buffer, view)."""
    shape = tuple(vals.shape)
    buf = new_buf(shape, dt, mode)
    _region(buf, shape, mode).copy_(vals.to(dt))
    return buf, _view(buf, shape, mode)


def read_back(buf, shape, mode):
    """The view's elements as fp64 on the CPU, after asserting that everything outside the view is still NaN."""
    got = _region(buf, shape, mode).detach().clone()
    if mode != "dense":
        rest = buf.detach().clone()
        _region(rest, shape, mode).fill_(NAN)
        assert bool(torch.isnan(rest).all()), f"{mode}: an element outside the view was written"
    return got.cpu().double()


# ---------------------------------------------------------------- BatchNorm module stand-in
class _BN:
    def __init__(self, C, seed):
        g = torch.Generator().manual_seed(seed)
        w = torch.rand(C, generator=g) + 0.5
        w[1::3] *= -1.0  # negative gammas too
        self.host = {"weight": w, "bias": torch.randn(C, generator=g) * 0.1,
                     "running_mean": torch.randn(C, generator=g) * 0.1, "running_var": torch.rand(C, generator=g) + 0.5}
        for k, v in self.host.items():
            setattr(self, k, v.to(DEV))
        self.num_batches_tracked = torch.zeros((), dtype=torch.long, device=DEV)
        self.momentum, self.eps = 0.1, 1e-5

    def buffers(self):
        return self.running_mean.clone(), self.running_var.clone(), self.num_batches_tracked.clone()


def _same_buffers(a, b):
    return all(torch.equal(p, q) for p, q in zip(a, b))


# ================================================================ A. stc_bn_finalize on synthetic partials
def make_partials(nch, C, single=None):
    """part[nch][C][4] = {n, S1, S2, shift} (fp32) of hand-made chunks: about 10 % empty, channel 1 constant,
    channel 2 with S2 - S1^2/n a few ulps below zero in every chunk."""
    rs = np.random.RandomState(977 * nch + C)
    f32 = lambda a: np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)  # noqa: E731
    n = rs.randint(1, 4097, size=(nch, C)).astype(np.float64)
    n[rs.rand(nch, C) < 0.1] = 0.0
    n[0] = np.maximum(n[0], 1.0)  # every channel has data
    if nch == 1:
        n[0, 0] = 1.0  # N = 1: the running variance takes the biased form
    if single is not None:
        keep = np.maximum(n[single], 2.0)
        n[:] = 0.0
        n[single] = keep
    live = n > 0
    nn = np.where(live, n, 1.0)
    sig = 0.5 + 3.0 * rs.rand(nch, C)
    m = 1.5 + 3.0 * rs.randn(nch, C)
    M2 = np.maximum(n - 1.0, 0.0) * sig ** 2 * (0.5 + rs.rand(nch, C))
    shift = f32(m + np.sqrt(M2 / nn) * rs.uniform(-3.0, 3.0, size=(nch, C)))
    S1 = f32(n * (m - shift))
    S2 = f32(M2 + S1 * S1 / nn)
    # channel 1: a constant channel
    shift[:, 1] = 2.25
    S1[:, 1] = 0.0
    S2[:, 1] = 0.0
    # channel 2: S2 two fp32 steps below S1^2/n (as after rounding of an almost constant chunk)
    d = rs.uniform(0.5, 2.0, size=nch) * np.where(rs.rand(nch) < 0.5, -1.0, 1.0)
    s1 = f32(n[:, 2] * d)
    s2 = (s1 * s1 / nn[:, 2]).astype(np.float32)
    s2 = np.nextafter(np.nextafter(s2, np.float32(0)), np.float32(0)).astype(np.float64)
    shift[:, 2] = f32(1.5 + 0.25 * rs.randn(nch))
    S1[:, 2], S2[:, 2] = s1, s2
    part = np.stack([n, S1, S2, shift], axis=-1) * live[..., None]
    return part.astype(np.float32)


def finalize_ref(part, bn):
    """The two-pass merge of csrc/bn.hip's header comment in long double: {name: (value, sum|terms|)}, fp64."""
    ld = np.longdouble
    p = part.astype(ld)
    n, S1, S2, sh = p[..., 0], p[..., 1], p[..., 2], p[..., 3]
    live = n > 0
    nn = np.where(live, n, ld(1))
    N = n.sum(0)
    mean = (n * sh + S1).sum(0) / N
    mean_abs = (np.abs(n * sh) + np.abs(S1)).sum(0) / N
    r = S1 / nn
    q = np.maximum(S2 - S1 * r, ld(0))  # the stated contract: a negative chunk M2 counts as 0
    d = sh + r - mean
    M2 = (live * (q + n * d * d)).sum(0)
    var = M2 / N
    eps, mom = ld(BN_EPS), ld(MOM)
    rstd = 1 / np.sqrt(var + eps)
    unb = np.where(N > 1, M2 / np.maximum(N - 1, ld(1)), var)
    g, b, rm, rv = (bn.host[k].numpy().astype(ld) for k in ("weight", "bias", "running_mean", "running_var"))
    scale = g * rstd
    out = {"mean": (mean, mean_abs), "rstd": (rstd, np.abs(rstd)), "scale": (scale, np.abs(scale)),
           "shift": (b - mean * scale, np.abs(b) + np.abs(mean * scale)),
           "running_mean": ((1 - mom) * rm + mom * mean, np.abs((1 - mom) * rm) + np.abs(mom * mean_abs)),
           "running_var": ((1 - mom) * rv + mom * unb, np.abs((1 - mom) * rv) + np.abs(mom * unb))}
    return {k: (torch.from_numpy(v.astype(np.float64)), torch.from_numpy(a.astype(np.float64)))
            for k, (v, a) in out.items()}


def check_finalize(part, nch, C, tag):
    bn = _BN(C, 500 + C)
    ref = finalize_ref(part, bn)
    pd = torch.from_numpy(part).to(DEV)
    tab = torch.full((2, C), NAN, device=DEV)
    mean, rstd = ops.bn_finalize_part(pd, nch, C, bn, tab[0], tab[1])
    got = {"mean": mean, "rstd": rstd, "scale": tab[0], "shift": tab[1], "running_mean": bn.running_mean,
           "running_var": bn.running_var}
    for k, (val, mag) in ref.items():
        err = (got[k].cpu().double() - val).abs()
        note(f"A.{k}", err, 4 * EPS32 * mag)
        if k in ("mean", "rstd"):
            note(f"A.{k}.ulp", err, ulp32(val))
    assert int(bn.num_batches_tracked) == 1
    # a second call on the same input: the same bits
    bn2 = _BN(C, 500 + C)
    tab2 = torch.full((2, C), NAN, device=DEV)
    mean2, rstd2 = ops.bn_finalize_part(pd, nch, C, bn2, tab2[0], tab2[1])
    assert torch.equal(mean2, mean) and torch.equal(rstd2, rstd) and torch.equal(tab2, tab), tag
    assert _same_buffers(bn2.buffers(), bn.buffers()), tag
    # update_running=False leaves the three buffers alone; the deferred update then equals the immediate one
    bn3 = _BN(C, 500 + C)
    before = bn3.buffers()
    tab3 = torch.full((2, C), NAN, device=DEV)
    mean3, rstd3 = ops.bn_finalize_part(pd, nch, C, bn3, tab3[0], tab3[1], update_running=False)
    assert _same_buffers(bn3.buffers(), before), tag
    assert torch.equal(mean3, mean) and torch.equal(rstd3, rstd) and torch.equal(tab3, tab), tag
    ops.bn_running_update(pd, nch, C, bn3)
    assert _same_buffers(bn3.buffers(), bn.buffers()), tag
    assert int(bn3.num_batches_tracked) == 1


FINALIZE_NCH = [1, 2, 64, 65, 256, 257, 512, 513, 1024, 1025, 2048, 2049, 4096, 4097, 9001]


@pytest.mark.parametrize("C", [3, 4, 5])
@pytest.mark.parametrize("nch", FINALIZE_NCH)
def test_finalize_synthetic_partials(nch, C):
    """bn_finalize_kernel<WaveMerge> (nch <= 256 / 512 / 1024, and its c >= C guard at C = 3, 5) and
    bn_finalize_kernel<BlockMerge> (nch <= 2048 / 4096 and the loop above) on hand-made partials with empty chunks, a
    constant channel and a channel of slightly negative chunk M2; running buffers, update_running=False and bn_running_update.
    Measured worst error / bound (MI355X): mean 0.104, rstd 0.116, scale 0.179, shift 0.220, running_mean 0.194,
    running_var 0.200 of 4 * EPS32 * sum|terms|; mean and rstd 0.50 of one fp32 ulp."""
    check_finalize(make_partials(nch, C), nch, C, f"nch={nch} C={C}")


@pytest.mark.parametrize("nch,single", [(65, 37), (1025, 1024), (4097, 2500)])
def test_finalize_single_live_chunk(nch, single):
    """Every chunk but one empty: the merge equals that chunk's own statistics."""
    check_finalize(make_partials(nch, 4, single=single), nch, 4, f"nch={nch} only chunk {single}")


@pytest.mark.parametrize("C", [1, 5, 256, 257])
def test_eval_table(C):
    """bn_eval_table_kernel: scale = gamma / sqrt(running_var + eps) within 2 fp32 ulp, shift = beta -
    running_mean * scale (of the device's own scale) within 2 fp32 ulp; running_var from 1e-6 to 1e3, negative
    gammas, a partial last block (C = 257).  Measured worst (MI355X): scale 1.67 ulp, shift 0.50 ulp.  (The fp32
    formula add, sqrt, divide, multiply has no 2-ulp guarantee: an fp32 emulation reaches 2.35 ulp over 2e6 random
    draws; the fixed inputs here stay below 2.)"""
    g = torch.Generator().manual_seed(40 + C)
    bn = _BN(C, 41 + C)
    rv = (10.0 ** (torch.rand(C, generator=g) * 9.0 - 6.0)).float()
    rv[0] = 1e-6
    rv[-1] = 1e3
    rm = (torch.randn(C, generator=g) * 2.0).float()
    bn.running_var, bn.running_mean = rv.to(DEV), rm.to(DEV)
    tab = torch.full((2, C), NAN, device=DEV)
    ops.bn_eval_table(C, bn, tab[0], tab[1])
    sc, sh = tab[0].cpu().double(), tab[1].cpu().double()
    ref_sc = bn.host["weight"].double() / torch.sqrt(rv.double() + BN_EPS)
    note("A.eval.scale", (sc - ref_sc).abs(), 2 * ulp32(ref_sc))
    ref_sh = bn.host["bias"].double() - rm.double() * sc
    note("A.eval.shift", (sh - ref_sh).abs(), 2 * ulp32(ref_sh))


# ================================================================ B. stc_chan_stats + finalize
STAT_SHAPES = {
    F32: [(2, 1, 1, 4), (1, 5, 13, 8), (1, 1, 63, 96), (1, 8, 8, 96), (1, 5, 13, 1024), (3, 15, 20, 128),
          (1, 257, 255, 4), (1, 1, 65537, 4)],
    BF16: [(2, 1, 1, 8), (1, 5, 13, 24), (1, 1, 65, 64), (1, 5, 13, 2048), (3, 15, 20, 128), (1, 257, 255, 8),
           (1, 1, 65537, 8)],
}
CROP_SHAPES = {F32: [(1, 5, 13, 8), (3, 15, 20, 128), (1, 8, 8, 96)], BF16: [(1, 5, 13, 24), (3, 15, 20, 128)]}


def _sid(shape):
    return "x".join(str(v) for v in shape)


def _layout_params(kinds=("std",)):
    out = []
    for dt in (F32, BF16):
        for shape in STAT_SHAPES[dt]:
            modes = ["dense", "lo", "hi"] + (["crop"] if shape in CROP_SHAPES[dt] else [])
            for mode in modes:
                out.append(pytest.param(dt, shape, "std" if dt == F32 else "bf", mode,
                                        id=f"{dtname(dt)}-{_sid(shape)}-{mode}"))
            if dt == F32 and "ill" in kinds:
                for mode in ["dense"] + (["crop"] if shape == (3, 15, 20, 128) else []):
                    out.append(pytest.param(dt, shape, "ill", mode, id=f"f32-{_sid(shape)}-{mode}-ill"))
    return out


@functools.lru_cache(maxsize=None)
def stats_case(shape, dt, kind):
    """(stored values x [B, H, W, C] fp32, fp64 per-channel mean / biased variance / max|x - mean| / sum|x| / sum)."""
    B, H, W, C = shape
    g = torch.Generator().manual_seed(71 + 3 * B + 5 * H + 7 * W + 11 * C)
    r = torch.randn(shape, generator=g)
    if kind == "std":
        x, const = r * 3 + 1.5, 2.5
    elif kind == "ill":  # mean / sigma = 1e4: what the shifted sums exist for
        x, const = 100.0 + 0.01 * r, 100.0
    else:
        x, const = 8.0 + r, 8.0
    x[..., 1] = const
    x = stored(x, dt)
    xd = x.double()
    mean = xd.mean(dim=(0, 1, 2))
    dev = (xd - mean).abs().amax(dim=(0, 1, 2))
    var = ((xd - mean) ** 2).mean(dim=(0, 1, 2))
    return x, {"mean": mean, "var": var, "dev": dev, "sum": xd.sum(dim=(0, 1, 2)),
               "abs": xd.abs().sum(dim=(0, 1, 2))}


@pytest.mark.parametrize("dt,shape,kind,mode", _layout_params(kinds=("std", "ill")))
def test_chan_stats_train_table(dt, shape, kind, mode):
    """chan_stats_kernel + finalize through ops.bn_train_table: thread layouts CG = 1, 2, 3, 8, 16, 24, 32, 256,
    one pixel per chunk up to 65 per chunk, P = 65535 / 65537 (empty tail chunks), dense, channel-offset (the other
    half NaN) and cropped (NaN surround) views, a constant channel, and the ill-conditioned 100 + 0.01 * randn.
    |mean - ref| <= ulp32(ref) + m * EPS32 * max|x - mean|; variance (from rstd) within 1e-5 relative, plus the
    2 * EPS32 * (var + eps) that rstd's own fp32 rounding moves it; running buffers as in section A with the mean /
    variance bounds carried through.  Measured worst error / bound (MI355X): mean 0.490, var 0.350,
    running_mean 0.216, running_var 0.175, scale 0.122, shift 0.124."""
    B, H, W, C = shape
    P = B * H * W
    x, ref = stats_case(shape, dt, kind)
    buf, xv = place(x, dt, mode)
    bn = _BN(C, 300 + C)
    tab = torch.full((2, C), NAN, device=DEV)
    assert ops.stats_chunks(B, H, W) == stat_chunks(P)
    mean, rstd = ops.bn_train_table(B, xv, C, dt, bn, tab[0], tab[1])
    mean, rstd = mean.cpu().double(), rstd.cpu().double()
    m = acc_len(P, C, dt)
    mean_b = ulp32(ref["mean"]) + m * EPS32 * ref["dev"]
    note("B.mean", (mean - ref["mean"]).abs(), mean_b)
    var_b = 1e-5 * ref["var"] + 2 * EPS32 * (ref["var"] + BN_EPS)
    note("B.var", (1.0 / (rstd * rstd) - BN_EPS - ref["var"]).abs(), var_b)
    rm0, rv0 = bn.host["running_mean"].double(), bn.host["running_var"].double()
    rm_ref = (1 - MOM) * rm0 + MOM * ref["mean"]
    note("B.running_mean", (bn.running_mean.cpu().double() - rm_ref).abs(),
         4 * EPS32 * (((1 - MOM) * rm0).abs() + (MOM * ref["mean"]).abs()) + MOM * mean_b)
    unb = ref["var"] * (P / (P - 1.0) if P > 1 else 1.0)
    rv_ref = (1 - MOM) * rv0 + MOM * unb
    note("B.running_var", (bn.running_var.cpu().double() - rv_ref).abs(),
         4 * EPS32 * (((1 - MOM) * rv0).abs() + MOM * unb) + MOM * 1e-5 * unb)
    assert int(bn.num_batches_tracked) == 1
    # the table, from the device's own mean / rstd
    gam, bet = bn.host["weight"].double(), bn.host["bias"].double()
    sc = tab[0].cpu().double()
    note("B.scale", (sc - gam * rstd).abs(), 4 * EPS32 * (gam * rstd).abs())
    note("B.shift", (tab[1].cpu().double() - (bet - mean * sc)).abs(), 4 * EPS32 * (bet.abs() + (mean * sc).abs()))
    read_back(buf, shape, mode)  # (the input's surround untouched)


# ================================================================ E. stc_chan_sum
@pytest.mark.parametrize("dt,shape,kind,mode", _layout_params())
def test_chan_sum(dt, shape, kind, mode):
    """chan_sum_kernel + chan_sum_final_kernel on the layouts of section B, all channels and Cout < C (the
    outputs past Cout stay untouched): within m * EPS32 * sum|x|.  Measured worst error / bound (MI355X): 0.034."""
    B, H, W, C = shape
    x, ref = stats_case(shape, dt, kind)
    _, xv = place(x, dt, mode)
    m = acc_len(B * H * W, C, dt)
    for cout in (C, C - 1):
        out = torch.full((C,), NAN, device=DEV)
        got = ops.chan_sum(B, xv, C, cout, dt, DEV, out=out[:cout])
        note("E.chan_sum", (got.cpu().double() - ref["sum"][:cout]).abs(), m * EPS32 * ref["abs"][:cout])
        assert bool(torch.isnan(out[cout:]).all())


# ================================================================ C. stc_bn_apply
BIG = (1, 1, 70000, 128)  # fp32: past the 2048-block (streaming) and 8192-block (general) grid caps
APPLY_SHAPES = {F32: STAT_SHAPES[F32] + [BIG], BF16: STAT_SHAPES[BF16]}


@functools.lru_cache(maxsize=None)
def apply_case(shape, dt, table):
    """Inputs built from the activations backwards: |n| in [0.1, 3] with random sign, |scale| in [0.5, 1.25] with
    every third channel negative, shift in [-0.5, 0.5], x = (n - shift) / scale in the storage type.  Returns
    (x, scale, shift, n_ref fp64); no ReLU / LeakyReLU decision of n_ref is rounding-sensitive (asserted)."""
    B, H, W, C = shape
    g = torch.Generator().manual_seed(13 + 3 * B + 5 * H + 7 * W + 11 * C)
    n = (0.1 + 2.9 * torch.rand(shape, generator=g)) * torch.where(torch.rand(shape, generator=g) < 0.5, -1.0, 1.0)
    if table:
        sc = (0.5 + 0.75 * torch.rand(C, generator=g)).float()
        sc[::3] *= -1.0
        sh = (torch.rand(C, generator=g) - 0.5).float()
        x = stored((n - sh) / sc, dt)
        nref = x.double() * sc.double() + sh.double()
    else:
        sc = sh = None
        x = stored(n, dt)
        nref = x.double()
    assert float(nref.abs().min()) >= 0.09, float(nref.abs().min())
    return x, sc, sh, nref


def act_ref(n, slope):
    return n if slope == 1.0 else torch.where(n > 0, n, n * slope32(slope))


def check_elementwise(key, got, ref, dt, tol=None):
    """fp32: |got - ref| <= tol (default: one fp32 ulp, 2^-23 |ref|).  bf16: got lies between the bf16 roundings of
    ref -/+ tol (default: of the fp32 neighbours of fp32(ref)), i.e. it is the round-to-nearest-even of an fp32
    value that close to ref; ratio reported in units of the allowed interval."""
    if dt == F32:
        note(key, (got - ref).abs(), EPS32 * ref.abs() if tol is None else tol)
        return
    if tol is None:
        r32 = ref.float()
        lo = torch.nextafter(r32, torch.full_like(r32, -math.inf))
        hi = torch.nextafter(r32, torch.full_like(r32, math.inf))
    else:
        lo, hi = (ref - tol).float(), (ref + tol).float()
    lo, hi = lo.to(BF16).double(), hi.to(BF16).double()
    mid, half = 0.5 * (lo + hi), 0.5 * (hi - lo)
    # (an exact hit of a degenerate interval is ratio 0; any miss of it is > 1)
    err = (got - mid).abs()
    note(key, torch.where(err <= half, err / half.clamp_min(1e-300), torch.full_like(err, 2.0)).nan_to_num(0.0),
         torch.ones_like(err))


SLOPES = [(0.2, 0.0), (0.0, 0.2), (0.2, None), (0.0, None), (1.0, None)]
# view mixes (x, y1, y2): all dense; the generator's cat[k] pattern (y1 into the second half of a 2C buffer,
# streaming with ps = 2C); cropped x and y1 (general addressing)
MIXES = {"dense": ("dense", "dense", "dense"), "cat": ("dense", "hi", "dense"), "crop": ("crop", "crop", "dense")}


def _apply_params():
    return [pytest.param(dt, shape, id=f"{dtname(dt)}-{_sid(shape)}") for dt in (F32, BF16)
            for shape in APPLY_SHAPES[dt]]


@pytest.mark.parametrize("table", [True, False], ids=["table", "identity"])
@pytest.mark.parametrize("mix", list(MIXES))
@pytest.mark.parametrize("dt,shape", _apply_params())
def test_bn_apply(dt, shape, mix, table):
    """bn_apply_kernel<T, DENSE> for both types, with and without a table and a second output, slopes 0.2 / 0 / 1:
    streaming (dense, and y1 at channel offset C of a 2C buffer), general addressing (cropped x / y1; C = 96 fp32
    and C = 24 bf16 by the 256 % CG rule), both grid caps (70000 x 128).  fp32 within 2^-23 |ref|; bf16 the
    round-to-nearest-even of the fp32 value; everything outside the written views stays NaN.
    Measured worst error / bound (MI355X): fp32 0.874; bf16 every element inside its interval."""
    x, sc, sh, nref = apply_case(shape, dt, table)
    mx, m1, m2 = MIXES[mix]
    _, xv = place(x, dt, mx)
    tab = (sc.to(DEV), sh.to(DEV)) if table else None
    B, _, _, C = shape
    for s1, s2 in (SLOPES if shape != BIG else [(0.2, 0.0), (1.0, None)]):
        y1 = new_buf(shape, dt, m1)
        y2 = new_buf(shape, dt, m2) if s2 is not None else None
        ops.bn_apply(B, xv, C, dt, tab, _view(y1, shape, m1), s1,
                     _view(y2, shape, m2) if y2 is not None else None, s2 if s2 is not None else 1.0)
        check_elementwise(f"C.apply.{dtname(dt)}", read_back(y1, shape, m1), act_ref(nref, s1), dt)
        if y2 is not None:
            check_elementwise(f"C.apply.{dtname(dt)}", read_back(y2, shape, m2), act_ref(nref, s2), dt)


# ================================================================ D. stc_bn_bwd_reduce / stc_bn_bwd_apply
def dact_ref(n, slope):
    return torch.where(n > 0, 1.0, slope32(slope)).double()


def grads_for(shape, dt, seed):
    g = torch.Generator().manual_seed(seed)
    return stored(torch.randn(shape, generator=g), dt), stored(torch.randn(shape, generator=g), dt)


def dn_terms(nref, g1, s1, g2, s2):
    """dn = g1 * act1'(n) + g2 * act2'(n) and |g1 act1'| + |g2 act2'| in fp64 (an absent gradient is None)."""
    dn = torch.zeros_like(nref)
    mag = torch.zeros_like(nref)
    for g, s in ((g1, s1), (g2, s2)):
        if g is not None:
            t = g.double() * dact_ref(nref, s)
            dn, mag = dn + t, mag + t.abs()
    return dn, mag


def dx_bound(k1, k2, k0, dn, x):
    """E of the kernel's dx = k1 * dn - k0 - k2 * x: 16 fp32 roundings (the k's and the two fmas) of the terms."""
    return 16 * EPS32 * ((k1 * dn).abs() + (k2 * x).abs() + k0.abs())


# configurations (g1 present, g2 present, slope1, slope2)
BWD_CFG = [(True, True, 0.0, 0.2), (True, False, 0.2, 0.0), (False, True, 0.0, 0.2), (True, True, 0.2, 0.0)]
# view mixes (x, g1, g2, dx): dense; g1 a channel-offset view (the ch_off use of the fused tests) and dx into the
# second half of a 2C buffer; cropped x and dx
BWD_MIXES = {"dense": ("dense", "dense", "dense", "dense"), "off": ("dense", "hi", "dense", "hi"),
             "crop": ("crop", "dense", "lo", "crop")}


@pytest.mark.parametrize("mix", list(BWD_MIXES))
@pytest.mark.parametrize("dt,shape", _apply_params())
def test_bn_backward_algebraic(dt, shape, mix):
    """ops.bn_backward with a hand-made state (scale, shift, mean, rstd, gamma -- unrelated to the data's own
    statistics): bn_bwd_reduce_kernel (every thread layout, empty chunks at P = 65537), both backward finalize
    kernels (<= 256 chunks: P <= 16384; above: P = 65535 / 65537 / 70000), bn_bwd_apply_kernel<T, DENSE> streaming
    and general, g1 / g2 present or absent, g1 at a channel offset, cropped x / dx, NaN outside the written view,
    repeated calls bit-identical.  dgamma / dbeta within m * EPS32 * sum|terms|; dx (with the device's own
    dgamma / dbeta in the reference's coefficients) within E = 16 * EPS32 * (|k1 dn| + |k2 x| + |k0|), bf16 between
    the roundings of ref -/+ E.  Measured worst error / bound (MI355X): dbeta 0.022, dgamma 0.023, dx fp32 0.228,
    dx bf16 every element inside its interval."""
    x, sc, sh, nref = apply_case(shape, dt, True)
    B, H, W, C = shape
    P = B * H * W
    g = torch.Generator().manual_seed(90 + C)
    mean = (1.0 + 0.5 * torch.randn(C, generator=g)).float()
    rstd = (0.3 + 0.9 * torch.rand(C, generator=g)).float()
    gam = (0.5 + torch.rand(C, generator=g)).float()
    gam[2::3] *= -1.0
    state = tuple(t.to(DEV) for t in (sc, sh, mean, rstd, gam))
    g1, g2 = grads_for(shape, dt, 91 + C)
    mx, mg1, mg2, mdx = BWD_MIXES[mix]
    _, xv = place(x, dt, mx)
    _, g1v = place(g1, dt, mg1)
    _, g2v = place(g2, dt, mg2)
    xd = x.double()
    xh = (xd - mean.double()) * rstd.double()
    m = acc_len(P, C, dt)
    k1 = gam.double() * rstd.double()
    for i, (has1, has2, s1, s2) in enumerate(BWD_CFG if shape != BIG else BWD_CFG[:1]):
        dxb = new_buf(shape, dt, mdx)
        dg, db = ops.bn_backward(B, xv, C, dt, _view(dxb, shape, mdx), g1=g1v if has1 else None, s1=s1,
                                 g2=g2v if has2 else None, s2=s2, bn_state=state)
        dn, mag = dn_terms(nref, g1 if has1 else None, s1, g2 if has2 else None, s2)
        dgd, dbd = dg.cpu().double(), db.cpu().double()
        note("D.dbeta", (dbd - dn.sum(dim=(0, 1, 2))).abs(), m * EPS32 * mag.sum(dim=(0, 1, 2)))
        note("D.dgamma", (dgd - (dn * xh).sum(dim=(0, 1, 2))).abs(), m * EPS32 * (mag * xh.abs()).sum(dim=(0, 1, 2)))
        k2 = k1 * rstd.double() * dgd / P
        k0 = k1 * (dbd / P - mean.double() * rstd.double() * dgd / P)
        check_elementwise(f"D.dx.{dtname(dt)}", read_back(dxb, shape, mdx), k1 * dn - k0 - k2 * xd, dt,
                          tol=dx_bound(k1, k2, k0, dn, xd))
        if i == 0:  # the same call again: the same bits
            dxb2 = new_buf(shape, dt, mdx)
            dg2, db2 = ops.bn_backward(B, xv, C, dt, _view(dxb2, shape, mdx), g1=g1v, s1=s1, g2=g2v, s2=s2,
                                       bn_state=state)
            assert torch.equal(dg2, dg) and torch.equal(db2, db)
            assert torch.equal(_region(dxb2, shape, mdx), _region(dxb, shape, mdx))


@pytest.mark.parametrize("mix", list(BWD_MIXES))
@pytest.mark.parametrize("dt,shape", _apply_params())
def test_act_backward_no_bn_family(dt, shape, mix):
    """bn_backward(bn_state=None): dx = g1 * act1'(x) + g2 * act2'(x), exact up to the rounding of the 0.2 product
    and of the sum -- EPS32 * (|g1 act1'| + |g2 act2'|), two half-ulp roundings (bf16: the rounding of a value
    that close).  Measured worst error / bound (MI355X): fp32 0.50."""
    x, _, _, nref = apply_case(shape, dt, False)
    B, _, _, C = shape
    g1, g2 = grads_for(shape, dt, 95 + C)
    mx, mg1, mg2, mdx = BWD_MIXES[mix]
    _, xv = place(x, dt, mx)
    _, g1v = place(g1, dt, mg1)
    _, g2v = place(g2, dt, mg2)
    for has1, has2, s1, s2 in (BWD_CFG[:3] if shape != BIG else BWD_CFG[:1]):
        dxb = new_buf(shape, dt, mdx)
        ops.bn_backward(B, xv, C, dt, _view(dxb, shape, mdx), g1=g1v if has1 else None, s1=s1,
                        g2=g2v if has2 else None, s2=s2)
        dn, mag = dn_terms(nref, g1 if has1 else None, s1, g2 if has2 else None, s2)
        check_elementwise(f"D.nobn.{dtname(dt)}", read_back(dxb, shape, mdx), dn, dt, tol=EPS32 * mag)


AUTOGRAD_SHAPES = [(2, 1, 1, 8), (1, 5, 13, 8), (3, 15, 20, 128), (4, 16, 16, 64), (1, 257, 255, 8)]


@functools.lru_cache(maxsize=None)
def autograd_case(shape, dt):
    """randn * 3 + 1.5 data conditioned so that no BN output of its true statistics lies within 1e-2 of zero: up to
    8 rounds of 'recompute the fp64 statistics, add 0.08 sigma to the elements with |n| < 1e-2'."""
    B, H, W, C = shape
    g = torch.Generator().manual_seed(61 + 3 * B + 5 * H + 7 * W + 11 * C)
    x = stored(torch.randn(shape, generator=g) * 3 + 1.5, dt)
    gam = (0.5 + torch.rand(C, generator=g)).float()
    gam[1::3] *= -1.0
    bet = (torch.randn(C, generator=g) * 0.1).float()
    for _ in range(8):
        xd = x.double()
        mean = xd.mean(dim=(0, 1, 2))
        var = ((xd - mean) ** 2).mean(dim=(0, 1, 2))
        n = (xd - mean) / torch.sqrt(var + BN_EPS) * gam.double() + bet.double()
        near = n.abs() < 1e-2
        if not bool(near.any()):
            break
        x = stored(torch.where(near, xd + 0.08 * torch.sqrt(var), xd), dt)
    assert not bool(near.any()), "conditioning did not converge"
    assert float(n.abs().min()) >= 1e-2
    return x, gam, bet


@pytest.mark.parametrize("dt", [F32, BF16], ids=dtname)
@pytest.mark.parametrize("shape", AUTOGRAD_SHAPES, ids=_sid)
def test_bn_backward_autograd(shape, dt):
    """bn_train_table + bn_backward against fp64 autograd of F.batch_norm + relu / leaky_relu on the stored values
    (this pins the backward formula itself, not only its evaluation).  dgamma / dbeta within m * EPS32 *
    sum|terms|; dx within E plus what those two bounds move it by, |k1| * (bound_dbeta + |xhat| bound_dgamma) / P.
    Measured worst error / bound (MI355X): dbeta 0.004, dgamma 0.009, dx fp32 0.072, dx bf16 inside."""
    x, gam, bet = autograd_case(shape, dt)
    B, H, W, C = shape
    P = B * H * W
    g1, g2 = grads_for(shape, dt, 63 + C)
    bn = _BN(C, 64)
    bn.weight, bn.bias = gam.to(DEV), bet.to(DEV)
    _, xv = place(x, dt, "dense")
    tab = torch.empty((2, C), device=DEV)
    mean, rstd = ops.bn_train_table(B, xv, C, dt, bn, tab[0], tab[1])
    _, g1v = place(g1, dt, "dense")
    _, g2v = place(g2, dt, "dense")
    m = acc_len(P, C, dt)
    for has2, s1, s2 in ((True, 0.0, 0.2), (False, 0.2, 0.0)):
        xr = x.double().permute(0, 3, 1, 2).contiguous().requires_grad_(True)
        gr, br = gam.double().requires_grad_(True), bet.double().requires_grad_(True)
        nrm = F.batch_norm(xr, None, None, gr, br, True, 0.0, BN_EPS)
        a1 = F.relu(nrm) if s1 == 0.0 else F.leaky_relu(nrm, slope32(s1))
        out = (a1 * g1.double().permute(0, 3, 1, 2)).sum()
        if has2:
            out = out + (F.leaky_relu(nrm, slope32(s2)) * g2.double().permute(0, 3, 1, 2)).sum()
        gx, gg, gb = torch.autograd.grad(out, (xr, gr, br))
        gx = gx.permute(0, 2, 3, 1)
        dxb = new_buf(shape, dt, "dense")
        dg, db = ops.bn_backward(B, xv, C, dt, L.nhwc_view(dxb), g1=g1v, s1=s1, g2=g2v if has2 else None, s2=s2,
                                 bn_state=(tab[0], tab[1], mean, rstd, bn.weight))
        nref = nrm.detach().permute(0, 2, 3, 1)
        dn, mag = dn_terms(nref, g1, s1, g2 if has2 else None, s2)
        xd = x.double()
        mu = xd.mean(dim=(0, 1, 2))
        rs = 1.0 / torch.sqrt(((xd - mu) ** 2).mean(dim=(0, 1, 2)) + BN_EPS)
        xh = (xd - mu) * rs
        b_db = m * EPS32 * mag.sum(dim=(0, 1, 2))
        b_dg = m * EPS32 * (mag * xh.abs()).sum(dim=(0, 1, 2))
        note("D.auto.dbeta", (db.cpu().double() - gb).abs(), b_db)
        note("D.auto.dgamma", (dg.cpu().double() - gg).abs(), b_dg)
        k1 = gam.double() * rs
        k2 = k1 * rs * gg / P
        k0 = k1 * (gb / P - mu * rs * gg / P)
        tol = dx_bound(k1, k2, k0, dn, xd) + k1.abs() * (b_db + xh.abs() * b_dg) / P
        check_elementwise(f"D.auto.dx.{dtname(dt)}", read_back(dxb, shape, "dense"), gx, dt, tol=tol)


# ================================================================ F. pixel-index boundary
@pytest.mark.parametrize("H", [4095, 4096], ids=["P=2^24-1_float_reciprocal", "P=2^24+4096_integer"])
def test_pixel_index_boundary(H):
    """pix_bxy on both sides of 2^24 pixels (bf16, C = 8, identity table, ReLU, cropped views so the general
    addressing runs): the op is exact, so the result equals torch.relu of the same view, and the NaN surround
    of the output is intact."""
    W, C = 4097, 8
    g = torch.Generator(device=DEV).manual_seed(5)
    src = torch.full((1, H + 1, W + 3, C), NAN, device=DEV, dtype=BF16)
    src[:, :H, :W] = torch.randn((1, H, W, C), device=DEV, generator=g).to(BF16)
    dst = torch.full_like(src, NAN)
    ops.bn_apply(1, L.nhwc_view(src, 0, H, W), C, BF16, None, L.nhwc_view(dst, 0, H, W), 0.0)
    assert torch.equal(dst[:, :H, :W], torch.relu(src[:, :H, :W]))
    assert bool(torch.isnan(dst[:, H:]).all()) and bool(torch.isnan(dst[:, :, W:]).all())


# ================================================================ G. refusals
def test_refusals_write_nothing():
    """Arguments the element-wise kernels cannot take raise through ops.check and launch nothing."""
    B, H, W = 1, 3, 5
    x6 = torch.randn(B, H, W, 6, device=DEV)
    x16 = torch.randn(B, H, W, 16, device=DEV)
    sc = torch.ones(8, device=DEV)

    def refused(fn, *outs):
        with pytest.raises(RuntimeError, match="stc_"):
            fn()
        torch.cuda.synchronize()
        for o in outs:
            assert bool(torch.isnan(o).all())

    y = torch.full((B, H, W, 6), NAN, device=DEV)  # C not a multiple of the 16-byte vector
    refused(lambda: ops.bn_apply(B, L.nhwc_view(x6), 6, F32, None, L.nhwc_view(y), 0.0), y)
    refused(lambda: ops.bn_backward(B, L.nhwc_view(x6), 6, F32, L.nhwc_view(y), g1=L.nhwc_view(x6)), y)
    part = torch.full((1, 6, 4), NAN, device=DEV)
    refused(lambda: ops.check(L.lib().stc_chan_stats(L.F32, B, L.nhwc_view(x6), 6, L.ptr(part), 1, L.stream()),
                              "stc_chan_stats"), part)
    y8 = torch.full((B, H, W, 16), NAN, device=DEV)  # channel offset not a multiple of the vector
    refused(lambda: ops.bn_apply(B, L.nhwc_view(x16, 2), 8, F32, None, L.nhwc_view(y8), 0.0), y8)
    refused(lambda: ops.bn_apply(B, L.nhwc_view(x16), 8, F32, None, L.nhwc_view(y8, 6), 0.0), y8)
    refused(lambda: ops.bn_backward(B, L.nhwc_view(x16), 8, F32, L.nhwc_view(y8, 2), g1=L.nhwc_view(x16, 8)), y8)
    # y1 null; scale without shift and the reverse
    refused(lambda: ops.bn_apply(B, L.nhwc_view(x16), 8, F32, None, L.NULL_VIEW, 0.0, y2=L.nhwc_view(y8)), y8)
    refused(lambda: ops.bn_apply(B, L.nhwc_view(x16), 8, F32, (sc, None), L.nhwc_view(y8), 0.0), y8)  # scale alone
    refused(lambda: ops.bn_apply(B, L.nhwc_view(x16), 8, F32, (None, sc), L.nhwc_view(y8), 0.0), y8)
