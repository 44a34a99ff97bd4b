"""The conv GEMM family pinned bit-exactly with integer-valued operands (tests/conv_exact_ref.py).

csrc/igemm_bf16.*, halo_bf16.hip, narrow_bf16.hip, stem_bf16.hip, wgrad_bf16.hip and the fp32 igemm.hip / wgrad.hip
on operands that are small integers (half- and quarter-integers after a prologue): every product and every partial
sum of every order is exact in fp32 (precondition sum |x||w| < 2^24, asserted per case), so an fp32 output must
EQUAL the fp64 reference and a bf16 output must be exactly its round-to-nearest-even rounding -- torch.equal, no
tolerance, at any K.  One missing, duplicated or misplaced product fails, and a mismatch is reported with the
rows / columns / channels of the wrong elements.  Every output buffer is pre-filled with NaN (nothing outside the
output view may be written, everything inside must be); where the input is a channel slice of a wider buffer the
other channels are NaN, so a read outside the view poisons the output.

The shapes are the small ones of test_gpu_igemm_bf16.py, test_gpu_halo.py and test_gpu_kernels.py (none of the
B = 32 ones), on the plans those files force.

Section 4 (the fused BatchNorm statistics, the fused BatchNorm-backward sums) is not bit-exact: the accumulators
are exact but the epilogue's fp32 sums of them round.  Those are checked against fp64 references of the exact
output with bounds derived from the accumulation lengths (conv_exact_ref.stats_bounds; ``stats_steps`` below), and
every statistics case first proves on the CPU that its bounds see ONE pixel left out of one channel.

What this file does not cover: the tanh epilogue and real-valued summation error, which stay with the Gaussian
tests of the files above.
"""
import functools

import pytest
import torch

import conv_exact_ref as R
from stcgan_amd import _lib as L
from stcgan_amd import ops
from test_gpu_halo import CASES as HALO_CASES, S1CASES as HALO_S1CASES, TCASES as HALO_TCASES
from test_gpu_igemm_bf16 import CASES as IG_CASES, CFGS as IG_CFGS, NARROW, NARROW_STREAM, WGRAD, WGRAD_FORCED
from test_gpu_kernels import CONV_CASES

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF, F32 = torch.bfloat16, torch.float32
NAN = float("nan")
KNAME = {L.CONV_S2: "conv_s2", L.CONV_S1: "conv_s1", L.CONVT_S2: "convT_s2", L.CONV_S1_DGRAD: "s1_dgrad"}
PACK = {L.CONV_S2: L.PACK_CONV_FWD, L.CONV_S1: L.PACK_CONV_FWD, L.CONVT_S2: L.PACK_CONVT_FWD,
        L.CONV_S1_DGRAD: L.PACK_CONV_S1_DGRAD}
HALO = ops.HALO_CFG

WORST = {}


def note(key, err, bound):
    """Largest error / bound of one quantity (printed: a run with -s records the measured ratios); asserts
    err <= bound element-wise."""
    err, bound = torch.as_tensor(err, dtype=torch.float64), torch.as_tensor(bound, dtype=torch.float64)
    ratio = float((err / bound.clamp_min(1e-300)).max())
    WORST[key] = max(WORST.get(key, 0.0), ratio)
    print(f"[conv_exact] {key}: error/bound {ratio:.4f}")
    assert bool((err <= bound).all()), f"{key}: error/bound {ratio:.4f} (max err {float(err.max()):.3e})"


def fid(f):
    return "auto" if f is None else f"cfg{f[0]}_ks{f[1]}"


def cid(c):
    return "x".join(map(str, c))


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def assert_same(got, exp, what):
    """torch.equal with a report of where the wrong elements are (NHWC or any 4-d layout: dims named d0..d3)."""
    got, exp = got.detach().cpu(), exp.detach().cpu()
    assert got.shape == exp.shape and got.dtype == exp.dtype, (what, got.shape, exp.shape, got.dtype, exp.dtype)
    if torch.equal(got, exp):
        return
    bad = (got != exp) | torch.isnan(got.float())
    idx = bad.nonzero()
    dims = ", ".join(f"d{d}: {sorted(set(idx[:, d].tolist()))[:12]}" for d in range(idx.shape[1]))
    first = tuple(idx[0].tolist())
    raise AssertionError(f"{what}: {len(idx)} of {bad.numel()} elements differ (shape {tuple(got.shape)}); indices by "
                         f"dim -- {dims}; first {first}: got {float(got[first])} expected {float(exp[first])}; "
                         f"NaN (unwritten / poisoned): {int(torch.isnan(got.float()).sum())}")


def place(vals, dt, mode):
    """Upload NHWC CPU values as a dense tensor or as the low / high channel half of a twice-as-wide NaN buffer:
    (buffer, view)."""
    C = vals.shape[-1]
    if mode == "dense":
        buf = vals.to(DEV, dt).contiguous()
        return buf, L.nhwc_view(buf)
    c0 = 0 if mode == "lo" else C
    buf = torch.full((*vals.shape[:-1], 2 * C), NAN, device=DEV, dtype=dt)
    buf[..., c0:c0 + C] = vals.to(DEV, dt)
    return buf, L.nhwc_view(buf, c0)


def out_buf(shape, dt, mode):
    """A NaN output buffer [B, H, W, C] (dense) or [B, H, W, 2C] with the view on one half: (buffer, view, c0)."""
    B, H, W, C = shape
    if mode == "dense":
        buf = torch.full(shape, NAN, device=DEV, dtype=dt)
        return buf, L.nhwc_view(buf), 0
    c0 = 0 if mode == "lo" else C
    buf = torch.full((B, H, W, 2 * C), NAN, device=DEV, dtype=dt)
    return buf, L.nhwc_view(buf, c0), c0


def read_out(buf, C, c0, what):
    """The view's channels on the CPU after asserting that every other channel of the buffer is still NaN."""
    got = buf[..., c0:c0 + C].contiguous().cpu()
    if buf.shape[-1] != C:
        rest = torch.cat((buf[..., :c0], buf[..., c0 + C:]), -1)
        assert bool(torch.isnan(rest.float()).all()), f"{what}: an element outside the output view was written"
    return got


def out_hw(kind, GH, GW):
    return (2 * GH, 2 * GW) if kind == L.CONVT_S2 else (GH, GW)


@functools.lru_cache(maxsize=None)
def operands(kind, case, seed=0, bias=False):
    """(x NHWC fp64, w, bias, expected bf16 NHWC, expected fp32 NHWC, ref64 NCHW) of a forward case; 8-channel
    inputs take the [-16, 16] range.  Cached and shared: never modified."""
    B, Cin, Cout, GH, GW = case
    x, w, b, ref = R.fwd_case(KNAME[kind], B, Cin, Cout, GH, GW, seed, 16 if Cin == 8 else 8, bias)
    if 16 * Cin // (4 if kind == L.CONVT_S2 else 1) >= 1024:
        R.require_shares(ref, f"{KNAME[kind]} {case}")
    return nhwc(x), w, b, nhwc(R.expect_bf16(ref)), nhwc(R.expect_f32(ref)), ref


# ================================================================ section 4a: the fused statistics
def reduce_steps(rows, N):
    """Longest fp32 chain of splitk_reduce_stats_kernel for ``rows`` GEMM rows of N channels: a thread sums
    ceil(rows_per_block / RL) rows (RL = 256 // (N / 8) row lanes), then RL lane totals are added; + 8 for the
    roundings inside a term and of the chunk's own mean / M2."""
    rl = max(1, 256 // (N // 8))
    blocks = min(1024, max(1, rows // max(rl, 4)))
    per = -(-rows // blocks)
    return -(-per // rl) + rl + 8


def tile_steps(BM, WM):
    """Longest fp32 chain of the tile epilogue (igemm_bf16.hpp tile_stats): a lane sums its BM / WM / 4 rows of a
    column, two lane merges, WM wave merges (Chan); + 8 as above."""
    return BM // WM // 4 + 2 + WM + 8


TILE_STEPS_MAX = 44  # BM = 256, WM = 2: the largest of every tile configuration (the halo blocks: WM >= 2)


def stats_steps(kind, case, plan, inlaunch):
    B, Cin, Cout, GH, GW = case
    BM, BN, ks, _, cfg = plan
    if cfg == HALO:
        return TILE_STEPS_MAX
    if ks > 1 and not inlaunch:
        return reduce_steps((4 if kind == L.CONVT_S2 else 1) * B * GH * GW, Cout)
    return tile_steps(BM, ops._BF16_TILES[cfg][2])


def check_stats(kind, case, part, ref, plan, inlaunch, what):
    """Measured worst error / bound over this file's 466 statistics launches (MI355X): mean 0.0045, variance 0.0013
    (the bounds are worst-case chains; one left-out pixel moves the reference mean by at least 11 and its variance by
    at least 1.1 bounds in every case, tests/test_conv_exact_cpu.py).
    The statistics partials against the fp64 statistics of the exact output (with the bias) over exactly its
    extent: counts sum to B*H*W exactly; mean and variance within the derived bounds -- after proving that those
    bounds see one pixel of one channel left out."""
    m = stats_steps(kind, case, plan, inlaunch)
    bm, bv = R.stats_bounds(ref, m)
    rm, rv = R.one_pixel_margin(ref, bm, bv)
    assert rm > 1 and rv > 1, f"{what}: the bounds (m = {m}) do not see one pixel: margins {rm:.2f} / {rv:.2f}"
    mean_r, var_r, P = R.stats_ref(ref)
    N, mean, var = R.merge_partials(part)
    assert bool((N == P).all()), f"{what}: pixel counts {sorted(set(N.tolist()))[:8]} != B*H*W = {P}"
    note("stats.mean", (mean - mean_r).abs(), bm)
    note("stats.var", (var - var_r).abs(), bv)


def run_stats(kind, case, force, in_mode="dense", out_mode="dense", bias=False, inlaunch=True, seed=0, stats=True):
    """stc_conv_fwd_ex with statistics into a NaN buffer: output exact (bf16 RNE of the fp64 reference), nothing
    outside the view written, statistics within the derived bounds.  Returns the plan."""
    B, Cin, Cout, GH, GW = case
    x, w, b, exp, _, ref = operands(kind, case, seed, bias)
    what = f"{KNAME[kind]} {case} {fid(force)} in={in_mode} out={out_mode} inlaunch={inlaunch}"
    xb, xv = place(x, BF, in_mode)
    wp = ops.pack(PACK[kind], w.float().to(DEV), Cout, Cin, BF)
    Ho, Wo = out_hw(kind, GH, GW)
    old = ops.set_splitk_inlaunch(inlaunch)
    try:
        _, nq, plan = ops.conv_query(kind, B, GH, GW, Cin, Cout, BF, force=force)
        yb, yv, c0 = out_buf((B, Ho, Wo, Cout), BF, out_mode)
        part, nch = ops.conv_stats(kind, B, xv, Cin, wp, Cout, yv, BF, bias=None if b is None else b.float().to(DEV),
                                   force=force)
        torch.cuda.synchronize()
    finally:
        ops.set_splitk_inlaunch(old)
    assert nq == nch
    assert_same(read_out(yb, Cout, c0, what), exp, what)
    if stats:
        check_stats(kind, case, part, ref, plan, inlaunch, what)
    return plan


# ================================================================ section 2: forward and input-gradient GEMMs
def _ig_params(cfgs):
    out = []
    for f in cfgs:
        if f is None or f[1] == 1:
            out.append((f, True))
        else:
            out += [(f, True), (f, False)]
    return out


IG_T_CFGS = [None, (0, 1), (1, 1), (3, 1), (5, 2), (8, 1), (9, 1), (13, 1), (11, 2), (14, 1), (15, 1), (16, 1), (17, 2),
             (18, 1), (19, 1), (29, 1), (30, 2), (31, 1), (32, 1), (33, 1), (34, 1), (35, 1)]  # test_convT_s2's list
# the Cin = 8 cases at full size hold too many pixels for the one-pixel condition of the statistics (see
# check_stats): the statistics are checked on the shrunk (2, 8, 64, 32, 32) / (2, 8, 64, 16, 16) beside them
IG_SMALL8 = {L.CONV_S2: (2, 8, 64, 32, 32), L.CONVT_S2: (2, 8, 64, 16, 16)}


@pytest.mark.parametrize("force,inlaunch", _ig_params(IG_CFGS), ids=lambda v: fid(v) if not isinstance(v, bool) else
                         ("inlaunch" if v else "reduce"))
@pytest.mark.parametrize("case", IG_CASES, ids=cid)
def test_im2col_conv_s2(case, force, inlaunch):
    """Conv2d k4 s2 on every im2col tile of test_gpu_igemm_bf16.CFGS (ragged M / N, Cin = 8, split-K 2 and 4 both
    in the launch and by the reduction launch): bf16 output exact, statistics within the derived bounds."""
    big8 = case[1] == 8
    run_stats(L.CONV_S2, case, force, inlaunch=inlaunch, stats=not big8)
    if big8 and force in (None, (0, 1), (0, 2), (5, 4)):
        run_stats(L.CONV_S2, IG_SMALL8[L.CONV_S2], force, inlaunch=inlaunch)


@pytest.mark.parametrize("force,inlaunch", _ig_params(IG_T_CFGS), ids=lambda v: fid(v) if not isinstance(v, bool) else
                         ("inlaunch" if v else "reduce"))
@pytest.mark.parametrize("case", IG_CASES, ids=cid)
def test_im2col_convT_s2(case, force, inlaunch):
    """ConvTranspose2d k4 s2 (4 phases) on the im2col tiles of test_gpu_igemm_bf16.test_convT_s2."""
    big8 = case[1] == 8
    run_stats(L.CONVT_S2, case, force, inlaunch=inlaunch, stats=not big8)
    if big8 and force in (None, (0, 1), (5, 2)):
        run_stats(L.CONVT_S2, IG_SMALL8[L.CONVT_S2], force, inlaunch=inlaunch)


@pytest.mark.parametrize("force,inlaunch", _ig_params([None, (0, 1), (6, 1), (0, 4), (14, 1), (17, 1)]),
                         ids=lambda v: fid(v) if not isinstance(v, bool) else ("inlaunch" if v else "reduce"))
def test_im2col_conv_s1_and_dgrad(force, inlaunch):
    """The stride-1 pair at H = 17 (K = 4096 and 8192): forward 17 x 17 -> 16 x 16, input gradient 16 x 16 -> 17 x 17."""
    run_stats(L.CONV_S1, (2, 256, 512, 16, 16), force, inlaunch=inlaunch)
    run_stats(L.CONV_S1_DGRAD, (2, 512, 256, 17, 17), force, inlaunch=inlaunch)


@pytest.mark.parametrize("force", [None, (1, 1), (0, 2)], ids=fid)
@pytest.mark.parametrize("in_mode,out_mode", [("dense", "hi"), ("hi", "lo"), ("lo", "hi")])
def test_im2col_views_and_bias(force, in_mode, out_mode):
    """Input from / output into channel halves of NaN-filled concat buffers, integer bias."""
    run_stats(L.CONV_S2, (2, 128, 128, 16, 16), force, in_mode=in_mode, out_mode=out_mode, bias=True)


F32_CFGS = [None, (0, 1), (1, 1), (3, 1), (4, 1), (5, 1), (6, 1), (13, 1), (14, 1), (19, 1), (29, 1), (31, 1), (35, 1)]


@pytest.mark.parametrize("force", F32_CFGS, ids=fid)
@pytest.mark.parametrize("case", IG_CASES, ids=cid)
@pytest.mark.parametrize("kind", [L.CONV_S2, L.CONVT_S2], ids=["conv_s2", "convT_s2"])
def test_im2col_f32_output(kind, case, force):
    """The element-store epilogue (out_f32, no tanh): the fp32 accumulators themselves, equal to the fp64 reference."""
    B, Cin, Cout, GH, GW = case
    x, w, b, _, exp, _ = operands(kind, case, 0, True)
    what = f"f32 out {KNAME[kind]} {case} {fid(force)}"
    xb, xv = place(x, BF, "dense")
    wp = ops.pack(PACK[kind], w.float().to(DEV), Cout, Cin, BF)
    Ho, Wo = out_hw(kind, GH, GW)
    yb, yv, c0 = out_buf((B, Ho, Wo, Cout), F32, "hi")
    ops.conv(kind, B, xv, Cin, wp, Cout, yv, BF, bias=b.float().to(DEV), out_f32=True, force=force)
    torch.cuda.synchronize()
    assert_same(read_out(yb, Cout, c0, what), exp, what)


@pytest.mark.parametrize("force", [None, (0, 1), (6, 1), (14, 1), (17, 1)], ids=fid)
@pytest.mark.parametrize("kind,case", [(L.CONV_S1, (2, 256, 512, 16, 16)), (L.CONV_S1_DGRAD, (2, 512, 256, 17, 17))],
                         ids=["conv_s1", "s1_dgrad"])
def test_im2col_f32_output_s1(kind, case, force):
    """The stride-1 pair at H = 17 with the fp32 element-store epilogue (dense output)."""
    B, Cin, Cout, GH, GW = case
    x, w, _, _, exp, _ = operands(kind, case, 0, False)
    what = f"f32 out {KNAME[kind]} {case} {fid(force)}"
    wp = ops.pack(PACK[kind], w.float().to(DEV), Cout, Cin, BF)
    yb, yv, _ = out_buf((B, GH, GW, Cout), F32, "dense")
    ops.conv(kind, B, place(x, BF, "dense")[1], Cin, wp, Cout, yv, BF, out_f32=True, force=force)
    torch.cuda.synchronize()
    assert_same(yb, exp, what)


# ---------------------------------------------------------------- halo kernels
@pytest.mark.parametrize("shape", [1, 2, 3, 4], ids=["8wave", "4wave", "n64", "n64w8"])
@pytest.mark.parametrize("case", HALO_CASES, ids=cid)
def test_halo_conv_s2(case, shape):
    plan = run_stats(L.CONV_S2, case, (HALO, shape))
    assert plan[4] == HALO and plan[0] == 256


HALO_T = [(c, s) for c in HALO_TCASES for s in (1, 2, 6)] + [(c, 5) for c in HALO_TCASES if c[2] <= 64]


@pytest.mark.parametrize("case,shape", HALO_T, ids=lambda v: cid(v) if isinstance(v, tuple) else f"shape{v}")
def test_halo_convT(case, shape):
    """ConvT on the 8-wave / 4-wave blocks, the phase pair (6) and, for N <= 64, one phase per block (5)."""
    plan = run_stats(L.CONVT_S2, case, (HALO, shape))
    assert plan[4] == HALO


@pytest.mark.parametrize("shape", [1, 2], ids=["8wave", "4wave"])
@pytest.mark.parametrize("case", HALO_S1CASES, ids=cid)
def test_halo_conv_s1(case, shape):
    """32 x 32 -> 31 x 31 on the 32 x 32 grid with the last row / column masked: the masked points are neither
    stored nor counted (counts sum to B * 31 * 31 exactly)."""
    B, Cin, Cout = case
    plan = run_stats(L.CONV_S1, (B, Cin, Cout, 31, 31), (HALO, shape))
    assert plan[4] == HALO


@pytest.mark.parametrize("shape", [1, 2], ids=["8wave", "4wave"])
@pytest.mark.parametrize("case", [c for c in HALO_S1CASES if c[2] % 64 == 0], ids=cid)
def test_halo_conv_s1_dgrad(case, shape):
    B, Cin, Cout = case  # of the conv: the GEMM reduces over Cout
    plan = run_stats(L.CONV_S1_DGRAD, (B, Cout, Cin, 32, 32), (HALO, shape))
    assert plan[4] == HALO


@pytest.mark.parametrize("shape", [1, 2, 3, 4], ids=["8wave", "4wave", "n64", "n64w8"])
@pytest.mark.parametrize("in_mode,out_mode", [("hi", "hi"), ("lo", "lo")])
def test_halo_views_and_bias(shape, in_mode, out_mode):
    plan = run_stats(L.CONV_S2, (2, 64, 128, 8, 32), (HALO, shape), in_mode=in_mode, out_mode=out_mode, bias=True)
    assert plan[4] == HALO


# ---------------------------------------------------------------- narrow kernels
NARROW_SMALL = [c for c in NARROW if c[1] < 32]
STREAM_SMALL = [c for c in NARROW_STREAM if c[0] < 32]
NARROW_RUNS = ([(("convT" if c[0] == "convT" else "conv_s1",) + tuple(c[1:]), None) for c in NARROW_SMALL] +
               [(("convT",) + tuple(c), f) for c in STREAM_SMALL for f in (None, (4, 1))])


@pytest.mark.parametrize("out", ["nhwc_bf16", "nchw_f32"])
@pytest.mark.parametrize("case,force", NARROW_RUNS, ids=lambda v: "_".join(map(str, v)) if isinstance(v, tuple) and
                         isinstance(v[0], str) else fid(v))
def test_narrow(case, force, out):
    """csrc/narrow_bf16.hip (N <= 8): the tiled K-split kernel, the streaming ConvT kernel and the two-pass logits
    form, bf16 NHWC output with bias and fp32 NCHW output without tanh (both exact)."""
    kname, B, Cin, N, GH, GW = case
    kind = L.CONVT_S2 if kname == "convT" else L.CONV_S1
    assert ops.plan_of(kind, B, GH, GW, Cin, N, BF)[3] == 1
    if kname == "convT" and force is None and (B, Cin, N, GH, GW) in STREAM_SMALL:
        assert ops.kernel_name(kind, B, GH, GW, Cin, N, BF)[0].startswith("narrow_stream_kernel")
    x, w, b, exp_bf, exp_f32, _ = operands(kind, (B, Cin, N, GH, GW), 7, True)
    what = f"narrow {case} {fid(force)} {out}"
    xb, xv = place(x, BF, "dense")
    wp = ops.pack(PACK[kind], w.float().to(DEV), N, Cin, BF)
    Ho, Wo = out_hw(kind, GH, GW)
    bg = b.float().to(DEV)
    if out == "nchw_f32":
        y = torch.full((B, N, Ho, Wo), NAN, device=DEV)
        ops.conv(kind, B, xv, Cin, wp, N, L.nchw_view(y), BF, bias=bg, tanh=False, out_f32=True, force=force)
        torch.cuda.synchronize()
        assert_same(y.permute(0, 2, 3, 1).contiguous(), exp_f32, what)
    else:
        y = torch.full((B, Ho, Wo, N), NAN, device=DEV, dtype=BF)
        ops.conv(kind, B, xv, Cin, wp, N, L.nhwc_view(y), BF, bias=bg, force=force)
        torch.cuda.synchronize()
        assert_same(y, exp_bf, what)


def test_narrow_stream_offset_view():
    """The streaming kernel writing 3 channels at offset 4 of an 8-channel NaN buffer."""
    B, Cin, N, GH, GW = 2, 128, 3, 16, 64
    x, w, _, exp, _, _ = operands(L.CONVT_S2, (B, Cin, N, GH, GW), 8, False)
    wp = ops.pack(L.PACK_CONVT_FWD, w.float().to(DEV), N, Cin, BF)
    buf = torch.full((B, 2 * GH, 2 * GW, 8), NAN, device=DEV, dtype=BF)
    ops.conv(L.CONVT_S2, B, place(x, BF, "dense")[1], Cin, wp, N, L.nhwc_view(buf, c0=4), BF)
    torch.cuda.synchronize()
    assert_same(read_out(buf, N, 4, "narrow stream offset"), exp, "narrow stream offset")


# ---------------------------------------------------------------- stem
@pytest.mark.parametrize("nout,s1,s2", [(1, 0.2, 0.0), (1, 0.0, 0.0), (2, 0.2, 0.0), (2, 0.0, 0.2)],
                         ids=["one_lrelu", "one_relu", "two_lrelu_relu", "two_relu_lrelu"])
def test_stem_conv_act(nout, s1, s2):
    """csrc/stem_bf16.hip through ops.conv_act at (B = 2, W = 256), integer bias: the activation is applied to the
    bf16-rounded conv value v = bf16(ref) (as the kernel's header states), y = bf16(v > 0 ? v : fp32(slope) * v)."""
    B, W = 2, 256
    case = (B, 8, 64, W // 2, W // 2)
    x, w, b, v, _, _ = operands(L.CONV_S2, case, 9, True)
    xb, xv = place(x, BF, "dense")
    wp = ops.pack(L.PACK_CONV_FWD, w.float().to(DEV), 64, 8, BF)
    y1b, y1v, _ = out_buf((B, W // 2, W // 2, 64), BF, "dense")
    y2b, y2v, c2 = out_buf((B, W // 2, W // 2, 64), BF, "hi")
    assert ops.conv_act(L.CONV_S2, B, xv, 8, wp, 64, y1v, s1, BF, y2v if nout == 2 else None, s2,
                        bias=b.float().to(DEV))
    torch.cuda.synchronize()
    assert_same(y1b, R.act_bf16(v, s1), f"stem y1 slope {s1}")
    if nout == 2:
        assert_same(read_out(y2b, 64, c2, "stem y2"), R.act_bf16(v, s2), f"stem y2 slope {s2}")
    else:
        assert bool(torch.isnan(y2b.float()).all())


# ---------------------------------------------------------------- fp32 path and prologues
def _pro_runs():
    out = []
    for dt in (F32, BF):
        v = ops.vec(dt)
        for case in CONV_CASES:
            B, Cin, Cout, H, W = case
            if Cin < v:
                continue
            for kname, slope in (("conv_s2", 0.5), ("conv_s2", 0.0), ("conv_s1", 0.5), ("conv_s1", 0.0)):
                out.append((dt, kname, case, True, slope))
            if (4 * Cin) % (32 if dt == F32 else 64) == 0:
                out += [(dt, "convT_s2", case, True, 0.5), (dt, "convT_s2", case, False, 0.0)]
    return out


@functools.lru_cache(maxsize=None)
def pro_operands(kname, case, table, slope):
    """A prologue case of test_gpu_kernels.CONV_CASES (B, Cin, Cout, input H, W): x, w, bias, the prologue table and
    the fp64 reference of conv(act(x*scale+shift, slope)) -- quarter-integers, precondition in units of 1/4."""
    B, Cin, Cout, H, W = case
    r = 16 if Cin <= 8 else 8
    x = R.acts((B, Cin, H, W), 6000, r)
    wshape = (Cin, Cout, 4, 4) if kname == "convT_s2" else (Cout, Cin, 4, 4)
    w = R.weights(wshape, 6001, r)
    b = R.biases(Cout, 6002)
    tab = R.pro_table(Cin, 6003) if table else None
    xa = R.prologue(x, tab, slope)
    R.require_exact(R.conv_abs(kname, xa, w, b), unit=0.25)
    return x, w, b, tab, nhwc(R.expect_f32(R.conv_ref(kname, xa, w, b)))


@pytest.mark.parametrize("dt,kname,case,table,slope", _pro_runs(),
                         ids=lambda v: {F32: "f32", BF: "bf16"}.get(v, cid(v) if isinstance(v, tuple) else str(v)))
def test_prologue_paths(dt, kname, case, table, slope):
    """csrc/igemm.hip (fp32) and the bf16 general kernel (which takes over when a prologue is given): per-channel
    scale in {+-1, +-2, 0.5}, integer shift, slope 0.5 / 0, integer bias, fp32 NHWC output into a NaN buffer's
    channel half.  Every prologue value is a small quarter-integer, exact in fp32 and bf16."""
    B, Cin, Cout, H, W = case
    kind = {"conv_s2": L.CONV_S2, "conv_s1": L.CONV_S1, "convT_s2": L.CONVT_S2}[kname]
    x, w, b, tab, exp = pro_operands(kname, case, table, slope)
    what = f"prologue {dt} {kname} {case} table={table} slope={slope}"
    xb, xv = place(nhwc(x), dt, "hi")
    wp = ops.pack(PACK[kind], w.float().to(DEV), Cout, Cin, dt)
    yb, yv, c0 = out_buf(tuple(exp.shape), F32, "lo")
    pro = None if tab is None else (tab[0].float().to(DEV), tab[1].float().to(DEV))
    ops.conv(kind, B, xv, Cin, wp, Cout, yv, dt, pro=pro, slope=slope, bias=b.float().to(DEV), out_f32=True)
    torch.cuda.synchronize()
    assert_same(read_out(yb, Cout, c0, what), exp, what)


# ================================================================ section 3: weight gradients
def run_wgrad(case, dt=BF, force=None, d_mode="dense", g_mode="dense", cg_out=None, seed=0):
    role, s, B, Cin, Cout, H, W = case
    x, dy, gw = R.wgrad_case(role, s, B, Cin, Cout, H, W, seed)
    D, G = (dy, x) if role == "conv" else (x, dy)
    Rr, Cg = D.shape[1], G.shape[1]
    cg_out = Cg if cg_out is None else cg_out
    db, dv = place(nhwc(D), dt, d_mode)
    gb, gv = place(nhwc(G), dt, g_mode)
    out = torch.full((Rr, cg_out, 4, 4), NAN, device=DEV)
    dW = ops.wgrad(B, s, dv, Rr, gv, Cg, cg_out, dt, device=DEV, force=force, out=out)
    torch.cuda.synchronize()
    assert_same(dW, R.expect_f32(gw)[:, :cg_out].contiguous(), f"wgrad {case} {fid(force)} D={d_mode} G={g_mode} "
                                                              f"Cg_out={cg_out}")


@pytest.mark.parametrize("case", WGRAD, ids=lambda c: "_".join(map(str, c)))
def test_wgrad_bf16(case):
    """csrc/wgrad_bf16.hip on its automatic plans: the fp32 dW equals the fp64 reference."""
    run_wgrad(case)


@pytest.mark.parametrize("case,cfg,ns", WGRAD_FORCED, ids=lambda c: "_".join(map(str, c)) if isinstance(c, tuple) else str(c))
def test_wgrad_bf16_forced(case, cfg, ns):
    """Tile configurations 0-8 with every pixel-split count of test_gpu_igemm_bf16.WGRAD_FORCED."""
    run_wgrad(case, force=(cfg, ns))


WGRAD_VIEWS = [(("conv", 2, 2, 64, 128, 32, 32), None), (("conv", 2, 2, 64, 128, 32, 32), (8, 3)),
               (("convT", 2, 2, 128, 64, 16, 16), None), (("convT", 2, 2, 128, 64, 16, 16), (7, 2)),
               (("conv", 1, 2, 256, 512, 17, 17), None), (("conv", 2, 3, 32, 96, 10, 14), (3, 3)),
               (("conv", 2, 2, 16, 64, 40, 24), None)]


@pytest.mark.parametrize("d_mode,g_mode", [("lo", "hi"), ("hi", "lo"), ("hi", "hi")])
@pytest.mark.parametrize("case,force", WGRAD_VIEWS, ids=lambda v: "_".join(map(str, v)) if isinstance(v, tuple) and
                         isinstance(v[0], str) else fid(v))
def test_wgrad_bf16_views(case, force, d_mode, g_mode):
    """D and G as the low / high half of twice-as-wide NaN buffers (the U-Net's concat buffers): a read outside a
    view poisons dW."""
    run_wgrad(case, force=force, d_mode=d_mode, g_mode=g_mode)


@pytest.mark.parametrize("case,force", WGRAD_VIEWS, ids=lambda v: "_".join(map(str, v)) if isinstance(v, tuple) and
                         isinstance(v[0], str) else fid(v))
def test_wgrad_bf16_cg_out(case, force):
    """Cg_out < Cg: only the first Cg_out channels of G get a gradient (padded input channels)."""
    Cg = case[3] if case[0] == "conv" else case[4]
    run_wgrad(case, force=force, cg_out=Cg // 2)
    run_wgrad(case, force=force, g_mode="hi", cg_out=Cg - 8)


ROWS_CASES = [(4, 512, 31, 31, 1, BF), (2, 64, 9, 13, 2, BF), (3, 128, 17, 5, 1, F32), (1, 64, 6, 7, 2, F32)]


@functools.lru_cache(maxsize=None)
def rows_operands(B, Cin, H, W, rows):
    """(x NCHW, dy NCHW with 8 channels of which ``rows`` are non-zero, dW fp32) of a rows-kernel case."""
    x = R.acts((B, Cin, H, W), 7100)
    dy = torch.zeros((B, 8, H - 1, W - 1), dtype=torch.float64)
    dy[:, :rows] = R.acts((B, rows, H - 1, W - 1), 7101)
    R.require_exact(R.wgrad_abs("conv", 1, x, dy))
    gw = R.expect_f32(R.wgrad_ref("conv", 1, x, dy))
    assert float(gw[rows:].abs().max()) == 0.0 and float(gw[:rows].abs().max()) > 0.0
    return x, dy, gw


@pytest.mark.parametrize("B,Cin,H,W,rows,dt", ROWS_CASES)
def test_wgrad_rows(B, Cin, H, W, rows, dt):
    """stc_conv_wgrad_rows (1-2 real channels of D padded to 8): real rows exact, padded rows exactly zero."""
    x, dy, gw = rows_operands(B, Cin, H, W, rows)
    dW = ops.wgrad(B, 1, place(nhwc(dy), dt, "dense")[1], 8, place(nhwc(x), dt, "dense")[1], Cin, Cin, dt, device=DEV,
                   rows=rows, rows_kernel=True)
    torch.cuda.synchronize()
    assert_same(dW, gw, f"wgrad rows {(B, Cin, H, W, rows, dt)}")
    assert float(dW[rows:].abs().max()) == 0.0


def _wgrad_f32_runs():
    out = []
    for case in CONV_CASES[:6]:
        for role, s in (("conv", 2), ("conv", 1), ("convT", 2)):
            for pro in (False, True):
                out.append((role, s, case, pro))
    return out


@functools.lru_cache(maxsize=None)
def wgrad_f32_operands(role, s, case, pro):
    """(D NCHW, G NCHW, D table, G table, dW fp32) of an fp32 weight-gradient case of CONV_CASES (B, Cin, Cout, input
    H, W); with ``pro`` a prologue on D (table, slope 0.5) and on G (table, slope 0): quarter- and half-integer
    operands, products multiples of 1/8, precondition in units of 1/16."""
    B, Cin, Cout, H, W = case
    x = R.acts((B, Cin, H, W), 7200)
    if role == "conv":
        Ho, Wo = (H + 2 - 4) // s + 1, (W + 2 - 4) // s + 1
    else:
        Ho, Wo = 2 * H, 2 * W
    dy = R.acts((B, Cout, Ho, Wo), 7201)
    D, G = (dy, x) if role == "conv" else (x, dy)
    dtab = R.pro_table(D.shape[1], 7202) if pro else None
    gtab = R.pro_table(G.shape[1], 7203) if pro else None
    Da = R.prologue(D, dtab, 0.5 if pro else None)
    Ga = R.prologue(G, gtab, 0.0 if pro else None)
    xa, dya = (Ga, Da) if role == "conv" else (Da, Ga)
    R.require_exact(R.wgrad_abs(role, s, xa, dya), unit=1.0 / 16)
    return D, G, dtab, gtab, R.expect_f32(R.wgrad_ref(role, s, xa, dya))


@pytest.mark.parametrize("role,s,case,pro", _wgrad_f32_runs(), ids=lambda v: cid(v) if isinstance(v, tuple) else str(v))
def test_wgrad_f32(role, s, case, pro):
    """csrc/wgrad.hip (fp32) for both roles with and without prologues on D and G: dW exact.  D and G sit in channel
    halves of NaN buffers."""
    B = case[0]
    D, G, dtab, gtab, gw = wgrad_f32_operands(role, s, case, pro)
    db, dv = place(nhwc(D), F32, "hi")
    gb, gv = place(nhwc(G), F32, "lo")
    dev = lambda t: None if t is None else (t[0].float().to(DEV), t[1].float().to(DEV))  # noqa: E731
    dW = ops.wgrad(B, s, dv, D.shape[1], gv, G.shape[1], G.shape[1], F32, dpro=dev(dtab), dslope=0.5 if pro else None,
                   gpro=dev(gtab), gslope=0.0 if pro else None, device=DEV)
    torch.cuda.synchronize()
    assert_same(dW, gw, f"wgrad f32 {role} s{s} {case} pro={pro}")


# ================================================================ section 4b: fused BatchNorm / activation backward
# (kind, B, Cin, Cout, GH, GW, BN channels C, ch_off, second gradient, wanted plan): the smallest shapes found whose
# AUTOMATIC plan (these entry points take no forced plan) is a halo kernel (>= 256 blocks), an im2col tile without
# split-K, and an in-launch split-K plan (2-4 splits, one statistics chunk per tile)
BNB_CASES = [
    (L.CONVT_S2, 4, 64, 256, 32, 32, 128, 128, True, "halo"),
    (L.CONVT_S2, 2, 128, 64, 16, 16, 64, 0, True, "tile"),
    (L.CONV_S2, 2, 64, 256, 16, 16, 128, 128, False, "splitk"),
    (L.CONVT_S2, 4, 256, 128, 8, 8, 128, 0, True, "splitk"),
]


def assert_plan(kind, case, want):
    B, Cin, Cout, GH, GW = case
    _, nch, plan = ops.conv_query(kind, B, GH, GW, Cin, Cout, BF)
    if want == "halo":
        assert plan[4] == HALO, plan
    elif want == "tile":
        assert plan[4] != HALO and plan[4] >= 0 and plan[2] == 1, plan
    else:
        nphase = 4 if kind == L.CONVT_S2 else 1
        assert plan[4] != HALO and 2 <= plan[2] <= 4 and nch == nphase * -(-B * GH * GW // plan[0]), (plan, nch)
    return plan


def bnb_steps(plan):
    """Longest fp32 chain of the BN-backward epilogue (igemm_bf16.hpp): a thread adds its BM * CPR / T rows of an
    8-channel chunk (CPR = BN / 8 chunks per row, T threads), then T / CPR thread totals are added in order; + 8
    for the roundings inside a term (the slope products, x - mean, * rstd).  The chunks are merged in fp64
    (bn_bwd_finalize).  The halo blocks have 4 or 8 waves: the longer chain of the two."""
    BM, BN, _, _, cfg = plan
    cpr = BN // 8
    ts = (256, 512) if cfg == HALO else (64 * ops._BF16_TILES[cfg][2] * ops._BF16_TILES[cfg][3],)
    return max(BM * cpr // t + t // cpr for t in ts) + 8


def between_bf16(key, got, ref, tol):
    """got (bf16) lies between the bf16 roundings of ref -/+ tol: it is the rounding of a value that close."""
    lo, hi = (ref - tol).float().to(BF).double(), (ref + tol).float().to(BF).double()
    mid, half = 0.5 * (lo + hi), 0.5 * (hi - lo)
    err = (got.double() - mid).abs()
    note(key, torch.where(err <= half, err / half.clamp_min(1e-300), torch.full_like(err, 2.0)).nan_to_num(0.0),
         torch.ones_like(err))


@pytest.mark.parametrize("case", BNB_CASES, ids=lambda c: f"{KNAME[c[0]]}-{cid(c[1:9])}-{c[9]}")
def test_conv_bn_backward(case):
    """stc_conv_bwd_bn_apply on a halo plan, an im2col tile and an in-launch split-K plan (asserted).  The kernels
    form dn from the bf16-ROUNDED conv value (the staged bf16 tile, igemm_bf16.hpp; the reduction launch re-reads
    its rounded store), so the reference is evaluated in fp64 from v = bf16(exact conv): the conv output itself
    torch.equal; dbeta = sum dn and dgamma = sum dn * xhat within (chain + 8) * EPS32 * sum |terms| (bnb_steps); dx
    (with the device's dgamma / dbeta in the coefficients, as tests/test_gpu_bn_family.py) between the bf16 roundings
    of ref -/+ 16 * EPS32 * sum |terms|.  Measured worst error / bound (MI355X): dbeta 0.0053, dgamma 0.0047, dx every
    element inside its interval."""
    kind, B, Cin, Cout, GH, GW, C, ch_off, other, want = case
    plan = assert_plan(kind, (B, Cin, Cout, GH, GW), want)
    x, w, _, exp, _, _ = operands(kind, (B, Cin, Cout, GH, GW), 0, False)
    Ho, Wo = out_hw(kind, GH, GW)
    P = B * Ho * Wo
    bx = nhwc(R.acts((B, C, Ho, Wo), 8100))                       # the BN input: integers, exact in bf16
    go = nhwc(R.acts((B, C, Ho, Wo), 8101)) if other else None    # the second gradient
    tabs = R.bn_tables(C, 8102)
    s_self, s_other = 0.2, 0.0
    v = exp[..., ch_off:ch_off + C].double()
    ref = R.bn_backward_ref(v, bx, go, tabs, s_self, s_other)
    scale, shift, mean, rstd, gamma = (t.to(DEV) for t in tabs)
    wp = ops.pack(PACK[kind], w.float().to(DEV), Cout, Cin, BF)
    what = f"bn backward {KNAME[kind]} {case[1:]}"
    yb, yv, _ = out_buf((B, Ho, Wo, Cout), BF, "dense")
    dxb, dxv, c0 = out_buf((B, Ho, Wo, C), BF, "hi")
    dg, db = ops.conv_bn_backward(kind, B, place(x, BF, "dense")[1], Cin, wp, Cout, yv, BF, bn_x=place(bx, BF, "dense")[1],
                                  C=C, bn_state=(scale, shift, mean, rstd), gamma=gamma, s_self=s_self, ch_off=ch_off,
                                  g_other=None if go is None else place(go, BF, "dense")[1], s_other=s_other, dxv=dxv)
    torch.cuda.synchronize()
    assert_same(yb, exp, what + " conv output")
    m = bnb_steps(plan)
    dgd, dbd = dg.cpu().double(), db.cpu().double()
    note("bnb.dbeta", (dbd - ref["dbeta"][0]).abs(), m * R.EPS32 * ref["dbeta"][1])
    note("bnb.dgamma", (dgd - ref["dgamma"][0]).abs(), m * R.EPS32 * ref["dgamma"][1])
    dn, dn_abs = ref["dn"]
    k1 = gamma.cpu().double() * rstd.cpu().double()
    k2 = k1 * rstd.cpu().double() * dgd / P
    k0 = k1 * (dbd / P - mean.cpu().double() * rstd.cpu().double() * dgd / P)
    tol = 16 * R.EPS32 * ((k1 * dn_abs).abs() + (k2 * bx).abs() + k0.abs())
    between_bf16("bnb.dx", read_out(dxb, C, c0, what), k1 * dn - k0 - k2 * bx, tol)


ACTB_CASES = [(4, 64, 256, 32, 32, True), (4, 64, 256, 32, 32, False), (2, 64, 512, 32, 32, True)]


@pytest.mark.parametrize("case", ACTB_CASES, ids=cid)
def test_conv_act_backward(case):
    """stc_conv_bwd_act (the halo kernels' epilogue): out = bf16(g_other * act'(x, 0) + v * act'(x, 0.2)) with
    v = bf16(exact conv) and x holding exact zeros (the slope branch).  g_other * act'(x, 0) is exact, so the fp32
    value is ONE rounding of g + v * s when the compiler contracts the multiply-add, and the rounded product plus g
    otherwise: both tensors are computed on the CPU and the output must EQUAL one of them as a whole (without
    g_other there is a single product and the two coincide)."""
    B, Cin, Cout, GH, GW, other = case
    kind = L.CONVT_S2
    assert_plan(kind, (B, Cin, Cout, GH, GW), "halo")
    x, w, _, exp, _, _ = operands(kind, (B, Cin, Cout, GH, GW), 0, False)
    Ho, Wo = 2 * GH, 2 * GW
    ax = nhwc(R.ints((B, Cout, Ho, Wo), 8200, 8, nonzero=False))  # the activation's input, zeros included
    assert int((ax == 0).sum()) > 0
    go = nhwc(R.acts((B, Cout, Ho, Wo), 8201)) if other else None
    s_self, s_other = 0.2, 0.0
    v = exp.float()
    d_self = R.dact(ax, s_self)
    g_term = torch.zeros_like(v) if go is None else go.float() * R.dact(ax, s_other)
    sep = (g_term + v * d_self).to(BF)                                       # rounded product, then the sum
    fma = (g_term.double() + v.double() * d_self.double()).float().to(BF)    # one rounding (the sum is exact in fp64)
    if go is None:
        assert torch.equal(sep, fma)
    wp = ops.pack(PACK[kind], w.float().to(DEV), Cout, Cin, BF)
    yb, yv, _ = out_buf((B, Ho, Wo, Cout), BF, "dense")
    assert ops.conv_act_backward(kind, B, place(x, BF, "dense")[1], Cin, wp, Cout, yv, BF,
                                 act_x=place(ax, BF, "dense")[1], s_self=s_self,
                                 g_other=None if go is None else place(go, BF, "dense")[1], s_other=s_other)
    torch.cuda.synchronize()
    got = yb.cpu()
    which = "contracted" if torch.equal(got, fma) else "separate"
    print(f"[conv_exact] act backward {case}: {which} multiply-add; the two conventions differ in "
          f"{int((sep != fma).sum())} elements")
    assert_same(got, fma if which == "contracted" else sep, f"act backward {case} ({which})")


# ================================================================ the case registry (tests/test_conv_exact_cpu.py)
def forward_cases():
    """Every (kind, case, seed, bias) that ``operands`` is called with above."""
    out = set()
    for kind in (L.CONV_S2, L.CONVT_S2):
        for c in IG_CASES:
            out.add((kind, c, 0, False))
            out.add((kind, c, 0, True))
        out.add((kind, IG_SMALL8[kind], 0, False))
    out |= {(L.CONV_S1, (2, 256, 512, 16, 16), 0, False), (L.CONV_S1_DGRAD, (2, 512, 256, 17, 17), 0, False),
            (L.CONV_S2, (2, 128, 128, 16, 16), 0, True), (L.CONV_S2, (2, 64, 128, 8, 32), 0, True)}
    out |= {(L.CONV_S2, c, 0, False) for c in HALO_CASES} | {(L.CONVT_S2, c, 0, False) for c in HALO_TCASES}
    out |= {(L.CONV_S1, (B, ci, co, 31, 31), 0, False) for (B, ci, co) in HALO_S1CASES}
    out |= {(L.CONV_S1_DGRAD, (B, co, ci, 32, 32), 0, False) for (B, ci, co) in HALO_S1CASES if co % 64 == 0}
    for case, _ in NARROW_RUNS:
        out.add((L.CONVT_S2 if case[0] == "convT" else L.CONV_S1, tuple(case[1:]), 7, True))
    out.add((L.CONVT_S2, (2, 128, 3, 16, 64), 8, False))
    out.add((L.CONV_S2, (2, 8, 64, 128, 128), 9, True))
    out |= {(c[0], tuple(c[1:6]), 0, False) for c in BNB_CASES}
    out |= {(L.CONVT_S2, tuple(c[:5]), 0, False) for c in ACTB_CASES}
    return sorted(out)


def stats_cases():
    """Every (kind, case, seed, bias) whose statistics are checked (run_stats with stats=True)."""
    extra = {(c[0], tuple(c[1:6])) for c in BNB_CASES} | {(L.CONVT_S2, tuple(c[:5])) for c in ACTB_CASES}
    out = [c for c in forward_cases() if c[2] == 0 and c[1][2] >= 16 and (c[0], c[1]) not in extra]
    big8 = {(L.CONV_S2, IG_CASES[4]), (L.CONVT_S2, IG_CASES[4])}
    ran = set()
    for kind in (L.CONV_S2, L.CONVT_S2):
        ran |= {(kind, c, 0, False) for c in IG_CASES if (kind, c) not in big8}
        ran.add((kind, IG_SMALL8[kind], 0, False))
    ran |= {c for c in out if c[0] in (L.CONV_S1, L.CONV_S1_DGRAD)}
    ran |= {(L.CONV_S2, (2, 128, 128, 16, 16), 0, True), (L.CONV_S2, (2, 64, 128, 8, 32), 0, True)}
    ran |= {(L.CONV_S2, c, 0, False) for c in HALO_CASES} | {(L.CONVT_S2, c, 0, False) for c in HALO_TCASES}
    return sorted(ran)
