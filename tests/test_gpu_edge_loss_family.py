"""csrc/eltwise.hip pinned to exact references (tests/edge_loss_ref.py): the NCHW <-> NHWC gather / scatter, the
tanh + bias backward, the L1 / MSE / BCE losses, the fused D and G objectives and the weight packer.

Layout kernels move values, so their outputs must EQUAL the fp64 reference cast once to the output type.  The tanh
backward and the L1 / MSE losses run on exactly-summable operands (multiples of 1/8 and 1/4; preconditions asserted
per case), so they must equal the reference too: one element left out or counted twice fails torch.equal.  What
cannot be exact -- BCE-with-logits and the gradient scale -- is held to bounds derived from the fp32 roundings of the
documented formulas (edge_loss_ref: U, bce_*_bound, grad_bound); each such comparison prints error / bound.  Every
output is allocated inside a larger NaN-filled buffer: everything inside the view must be written, nothing outside
it.  tests/test_edge_loss_ref_cpu.py plants a missing, a doubled, a sign-flipped and a misplaced element in the
expected tensors of these cases and shows that the comparison functions of this file reject each.

Which case reaches which kernel, by the dispatch conditions of stc_gather_nchw, stc_tanh_bias_bwd etc. as they stand.
``gather_path`` and ``tanh_path`` restate those conditions in Python and the cases assert that PREDICTION, not which
kernel ran: if the dispatch in csrc/eltwise.hip changes, a case can stop reaching its kernel and stay green, so the two
functions and this map have to be revised with it.
  gather4_kernel       test_gather4, test_gather_grid_stride[gather4]   (W % 4 == 0, 16-byte aligned sources)
  gather_vec_kernel    test_gather_vec (W in {10, 7}; W = 8 with a source at a 4-byte offset), ..._grid_stride[vec]
  gather_kernel        test_gather_scalar (Cpad 24 > 16; bf16 Cpad 4 and fp32 Cpad 6 are no multiple of the vector)
  scatter_kernel       test_scatter, test_scatter_grid_stride
  tanh_bwd4_kernel     test_tanh_bias_bwd[quad shapes];  tanh_bwd_kernel: [pixel shapes] and [y at a 4-byte offset]
  chunk_sum_kernel     every tanh case with a dbias;  test_tanh_no_dbias: not launched
  loss_partial_kernel / loss_final_kernel  test_l1_mse (n around 256 and 4096; n = 256*4096 +- 1: more than 256
                       partials), test_loss_tensor_target, test_bce
  loss_bwd_kernel      the same tests; strided: test_loss_grad_grid_stride (n = 8192*256 + 4097)
  loss_multi_*         test_d_objective_exact (unequal terms 900 / 4096 / 4097 / 1), test_g_objective_exact (L1 term
                       of 2048*256 + 1 elements: the backward strides), test_multi_bwd_null_grads (1 and 8 terms, NULL
                       first / middle / last), test_d_term_grad, test_objectives_bce, test_multi_fwd_many_partials
                       (a term of 257 partials: the strided pass of loss_multi_final_kernel)
  pack_kernel          test_pack_weight;  pack_multi_kernel: test_pack_weights (1, 2, STC_PACK_MAX descriptors) and
                       test_pack_weights_strided (N_pad * C_pad = 528 * 512 > 1024 * 256)

Deliberately not covered: the 64-bit-index instantiation of gather4_kernel (it needs B*H*W/4 >= 2^31, i.e. 2^33
pixels: out of reach), and the real-valued summation error of L1 / MSE, which stays with test_gpu_kernels.test_losses.
"""
import ctypes
import math

import pytest
import torch

import edge_loss_ref as R
from stcgan_amd import _lib as L
from stcgan_amd import loss as SL
from stcgan_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
NAN = float("nan")
GUARD = 64  # elements of NaN on either side of an output (a multiple of 16 bytes for both dtypes)
GOUTS = (3.0, 1.0 / 3.0)  # the second is no power of two: the scale chain really rounds

WORST = {}


def note(key, err, bound):
    """Largest error / bound of one quantity (printed: a run with -s records the measured ratios); asserts
    err <= bound element-wise and that the value is finite."""
    err, bound = torch.as_tensor(err, dtype=F64).cpu(), torch.as_tensor(bound, dtype=F64).cpu()
    assert bool(torch.isfinite(err).all()), f"{key}: not finite"
    ratio = float((err / bound.clamp_min(1e-300)).max())
    WORST[key] = max(WORST.get(key, 0.0), ratio)
    print(f"[edge_loss] {key}: error/bound {ratio:.4f}")
    assert bool((err <= bound).all()), f"{key}: error/bound {ratio:.4f} (max err {float(err.max()):.3e}); first at " \
                                       f"{tuple((err > bound).nonzero()[0].tolist()) if err.dim() else ()}"


def assert_same(got, exp, what):
    """torch.equal with a report of where the wrong elements are (dims named d0..); a NaN in ``exp`` (poison that must
    survive) matches only a NaN."""
    got, exp = got.detach().cpu(), exp.detach().cpu()
    assert got.shape == exp.shape and got.dtype == exp.dtype, (what, got.shape, exp.shape, got.dtype, exp.dtype)
    if torch.equal(got, exp):
        return
    g, e = got.double(), exp.double()
    bad = ~((g == e) | (torch.isnan(g) & torch.isnan(e)))
    if not bool(bad.any()):
        return
    if bad.dim() == 0:
        raise AssertionError(f"{what}: got {float(g)!r} expected {float(e)!r}")
    idx = bad.nonzero()
    dims = ", ".join(f"d{d}: {sorted(set(idx[:, d].tolist()))[:12]}" for d in range(idx.shape[1]))
    first = tuple(idx[0].tolist())
    raise AssertionError(f"{what}: {len(idx)} of {bad.numel()} elements differ (shape {tuple(got.shape)}); indices by "
                         f"dim -- {dims}; first {first}: got {float(g[first])!r} expected {float(e[first])!r}; "
                         f"NaN (unwritten / poisoned): {int(torch.isnan(g).sum())}")


def arena(shape, dt):
    """A NaN-filled flat buffer with the output view in its middle: (buffer, view)."""
    n = math.prod(shape)
    buf = torch.full((n + 2 * GUARD,), NAN, dtype=dt, device=DEV)
    return buf, buf[GUARD:GUARD + n].view(shape)


def guards_intact(buf, what):
    g = torch.cat((buf[:GUARD], buf[-GUARD:])).float()
    assert bool(torch.isnan(g).all()), f"{what}: memory next to the output was written"


def offset_by_one(t):
    """The same values on the device at a storage offset of one element of a flat buffer: 4-byte aligned, not 16."""
    flat = torch.empty(t.numel() + 1, dtype=t.dtype, device=DEV)
    v = flat[1:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


def dn(dt):
    return "f32" if dt == F32 else "bf16"


# ================================================================== a. gather
CHANS = [(3,), (3, 1), (3, 1, 3), (4,), (3, 1, 3, 1)]


def cpad_for(chans, dt):
    v = ops.vec(dt)
    return -(-sum(chans) // v) * v


def gather_case(chans, B, H, W, dt, cpad, seed=0):
    """(NCHW fp32 sources, expected NHWC [B, H, W, cpad] of dt): Gaussian values, so the bf16 cast really rounds."""
    g = torch.Generator().manual_seed(1000 + seed)
    srcs = [torch.randn((B, c, H, W), generator=g, dtype=F32) for c in chans]
    return srcs, R.gather_ref(srcs, cpad).to(dt)


def gather_path(dt, cpad, H, W, ptrs):
    """The kernel stc_gather_nchw takes for a dense NHWC destination."""
    n = ops.vec(dt)
    if cpad > 16 or cpad % n:
        return "scalar"
    if W % 4 == 0 and H * W < 2 ** 31 and all(p % 16 == 0 for p in ptrs):
        return "gather4"
    return "vec"


def run_gather(srcs, exp, dt, path, what, offset=None):
    dev = [offset_by_one(s) if k == offset else s.to(DEV) for k, s in enumerate(srcs)]
    B, H, W, cpad = exp.shape
    buf, dst = arena(exp.shape, dt)
    assert gather_path(dt, cpad, H, W, [d.data_ptr() for d in dev]) == path, (what, path)
    ops.gather(dev, dst, dt)
    torch.cuda.synchronize()
    assert_same(dst, exp, what)  # (the padding channels of exp are zeros)
    guards_intact(buf, what)


@pytest.mark.parametrize("dt", [F32, BF], ids=dn)
@pytest.mark.parametrize("B,H,W", [(3, 6, 8), (2, 5, 12)], ids=["3x6x8", "2x5x12"])
@pytest.mark.parametrize("chans", CHANS, ids=lambda c: "c" + "_".join(map(str, c)))
def test_gather4(chans, B, H, W, dt):
    srcs, exp = gather_case(chans, B, H, W, dt, cpad_for(chans, dt))
    run_gather(srcs, exp, dt, "gather4", f"gather4 {chans} {B}x{H}x{W} {dn(dt)}")


@pytest.mark.parametrize("dt", [F32, BF], ids=dn)
@pytest.mark.parametrize("W,offset", [(10, None), (7, None), (8, 0), (8, -1)], ids=["w10", "w7", "w8_off_first", "w8_off_last"])
@pytest.mark.parametrize("chans", CHANS, ids=lambda c: "c" + "_".join(map(str, c)))
def test_gather_vec(chans, W, offset, dt):
    B, H = 3, 6
    srcs, exp = gather_case(chans, B, H, W, dt, cpad_for(chans, dt), seed=W)
    off = None if offset is None else offset % len(chans)
    run_gather(srcs, exp, dt, "vec", f"gather_vec {chans} W={W} offset={off} {dn(dt)}", offset=off)


@pytest.mark.parametrize("chans,cpad,dt", [((20,), 24, F32), ((20,), 24, BF), ((3,), 4, BF), ((3, 1), 6, F32)],
                         ids=["c20_cpad24_f32", "c20_cpad24_bf16", "c3_cpad4_bf16", "c3_1_cpad6_f32"])
@pytest.mark.parametrize("B,H,W", [(3, 6, 8), (2, 5, 7)], ids=["3x6x8", "2x5x7"])
def test_gather_scalar(chans, cpad, dt, B, H, W):
    srcs, exp = gather_case(chans, B, H, W, dt, cpad, seed=5)
    run_gather(srcs, exp, dt, "scalar", f"gather scalar {chans}->{cpad} {dn(dt)}")


@pytest.mark.parametrize("path,B,H,W", [("vec", 1, 1449, 1449), ("gather4", 5, 1024, 1024)], ids=["vec", "gather4"])
def test_gather_grid_stride(path, B, H, W):
    """Just over the launch cap of each kernel (8192*256 pixels / 4096*256 quads): the grid-stride loop runs twice
    for the first threads.  One channel into Cpad 4, fp32."""
    assert (B * H * W > 8192 * 256) if path == "vec" else (B * H * W // 4 > 4096 * 256)
    src = torch.randn((B, 1, H, W), generator=torch.Generator().manual_seed(77), dtype=F32)
    buf, dst = arena((B, H, W, 4), F32)
    dev = src.to(DEV)
    assert gather_path(F32, 4, H, W, [dev.data_ptr()]) == path
    ops.gather([dev], dst, F32)
    torch.cuda.synchronize()
    got = dst.cpu()
    assert torch.equal(got[..., 0], src[:, 0]), f"{path}: {int((got[..., 0] != src[:, 0]).sum())} pixels differ"
    assert torch.equal(got[..., 1:], torch.zeros_like(got[..., 1:]))
    guards_intact(buf, path)


# ================================================================== b. scatter
SCATTER_DIMS = [(2, 10, 12, 7, 9), (3, 6, 8, 6, 8)]  # B, Ha, Wa (allocated), H, W (logical)
SCATTER_SPLITS = [([3, 1, 3], 8, ()), ([3, 1, 3], 8, (0,)), ([3, 1, 3], 8, (1,)), ([3, 1, 3], 8, (2,)), ([1], 4, ())]


def scatter_case(chans, cpad, dims, dt, seed=0):
    """(NHWC source of dt [B, Ha, Wa, cpad], expected NCHW fp32 [B, c, H, W] per range)."""
    B, Ha, Wa, H, W = dims
    g = torch.Generator().manual_seed(2000 + seed)
    src = torch.randn((B, Ha, Wa, cpad), generator=g, dtype=F32).to(dt)
    return src, [e.to(F32) for e in R.scatter_ref(src, chans, H, W)]  # (bf16 -> fp32 is exact)


@pytest.mark.parametrize("dt", [F32, BF], ids=dn)
@pytest.mark.parametrize("dims", SCATTER_DIMS, ids=["crop7x9_of_10x12", "full6x8"])
@pytest.mark.parametrize("chans,cpad,skip", SCATTER_SPLITS, ids=["all", "none_first", "none_middle", "none_last", "c1"])
def test_scatter(chans, cpad, skip, dims, dt):
    src, exp = scatter_case(chans, cpad, dims, dt)
    B, Ha, Wa, H, W = dims
    slots = [arena((B, c, H, W), F32) for c in chans]
    ops.scatter(src.to(DEV), [None if k in skip else v for k, (_, v) in enumerate(slots)], chans, dt, H, W)
    torch.cuda.synchronize()
    for k, (buf, v) in enumerate(slots):
        what = f"scatter {chans} {dims} {dn(dt)} range {k}"
        if k in skip:
            assert bool(torch.isnan(buf).all()), f"{what}: a skipped destination was written"
        else:
            assert_same(v, exp[k], what)
            guards_intact(buf, what)


def test_scatter_grid_stride():
    B, H, W = 1, 1449, 1449
    assert B * H * W > 8192 * 256
    src = torch.randn((B, H, W, 4), generator=torch.Generator().manual_seed(78), dtype=F32)
    buf, v = arena((B, 1, H, W), F32)
    ops.scatter(src.to(DEV), [v], [1], F32)
    torch.cuda.synchronize()
    assert torch.equal(v.cpu()[:, 0], src[..., 0])
    guards_intact(buf, "scatter grid stride")


# ================================================================== c. tanh + bias backward
TANH_SHAPES = [("quad", 3, 10, 12), ("quad", 2, 4, 8), ("pixel", 2, 6, 10), ("pixel", 1, 3, 5), ("offset", 3, 10, 12)]


def tanh_case(B, C, H, W, dt, seed=0):
    """(y, gy fp32 NCHW, expected dq NHWC [B, H, W, Cpad] of dt, expected dbias fp32 [C], exact dq fp64)."""
    y, gy = R.tanh_operands(B, C, H, W, 3000 + seed)
    dq, db = R.tanh_bwd_ref(y, gy)
    return y.to(F32), gy.to(F32), R.gather_ref([dq], ops.vec(dt)).to(dt), db.to(F32), dq


def tanh_path(H, W, y, gy):
    return "quad" if W % 4 == 0 and y.data_ptr() % 16 == 0 and gy.data_ptr() % 16 == 0 else "pixel"


@pytest.mark.parametrize("dt", [F32, BF], ids=dn)
@pytest.mark.parametrize("C", [1, 3, 4])
@pytest.mark.parametrize("path,B,H,W", TANH_SHAPES, ids=lambda v: str(v))
def test_tanh_bias_bwd(path, B, H, W, C, dt):
    y, gy, exp_dq, exp_db, dq = tanh_case(B, C, H, W, dt, seed=C)
    nch = ops.stats_chunks(B, H, W)
    R.require_tanh_exact(dq, -(-B * H * W // nch) + 3)
    yd = offset_by_one(y) if path == "offset" else y.to(DEV)
    gd = gy.to(DEV)
    assert tanh_path(H, W, yd, gd) == ("quad" if path == "quad" else "pixel")
    buf, dqt = arena(exp_dq.shape, dt)
    bbuf, db = arena((C,), F32)
    ops.tanh_bias_bwd(yd, gd, L.nhwc_view(dqt), dt, dbias=db)
    torch.cuda.synchronize()
    what = f"tanh_bias_bwd {path} {B}x{C}x{H}x{W} {dn(dt)}"
    assert_same(dqt, exp_dq, what + " dq")
    assert_same(db, exp_db, what + " dbias")
    guards_intact(buf, what + " dq")
    guards_intact(bbuf, what + " dbias")


@pytest.mark.parametrize("dt", [F32, BF], ids=dn)
def test_tanh_no_dbias(dt):
    """dbias == NULL: dq as before, no sum launched -- the buffer a sum would have written keeps its NaN."""
    B, C, H, W = 3, 3, 10, 12
    y, gy, exp_dq, _, _ = tanh_case(B, C, H, W, dt, seed=9)
    nch = ops.stats_chunks(B, H, W)
    buf, dqt = arena(exp_dq.shape, dt)
    pbuf, part = arena((nch, C), F32)
    yd, gd = y.to(DEV), gy.to(DEV)
    L.check(L.lib().stc_tanh_bias_bwd(L.dtype_code(dt), B, C, H, W, L.ptr(yd), L.ptr(gd), L.nhwc_view(dqt), None,
                                      L.ptr(part), nch, L.stream()), "stc_tanh_bias_bwd")
    torch.cuda.synchronize()
    assert_same(dqt, exp_dq, "tanh no dbias dq")
    guards_intact(buf, "tanh no dbias dq")
    guards_intact(pbuf, "tanh no dbias partials")  # (the would-be dbias right behind the partials included)
    assert not bool(torch.isnan(part).any())


# ================================================================== d. single-term losses
NS = [1, 255, 256, 257, 4095, 4096, 4097, 8193, 256 * 4096 - 1, 256 * 4096 + 1]
FORMS = [("l1", R.L1, None), ("mse0", R.MSE, 0.0), ("mse1", R.MSE, 1.0), ("mse-1", R.MSE, -1.0)]
STRIDE_N = 8192 * 256 + 4097


def raw_loss(kind, p, t, c, gout):
    """stc_loss_fwd / stc_loss_bwd through the C API (the forms loss.py does not wrap: a tensor target for MSE /
    BCE), NaN-filled outputs: (value 0-d, gradient)."""
    n = p.numel()
    lib = L.lib()
    part = torch.full((lib.stc_loss_parts(n),), NAN, device=DEV)
    vbuf, out = arena((1,), F32)
    gbuf, grad = arena((n,), F32)
    go = torch.tensor([gout], dtype=F32, device=DEV)
    L.check(lib.stc_loss_fwd(kind, L.ptr(p), L.ptr(t), float(c), n, L.ptr(part), L.ptr(out), L.stream()), "stc_loss_fwd")
    L.check(lib.stc_loss_bwd(kind, L.ptr(p), L.ptr(t), float(c), n, L.ptr(go), L.ptr(grad), L.stream()), "stc_loss_bwd")
    torch.cuda.synchronize()
    guards_intact(vbuf, "loss value")
    guards_intact(gbuf, "loss gradient")
    return out[0], grad


def wrapped_loss(kind, p, t, c):
    if kind == R.L1:
        return SL.l1_loss(p, t)
    return SL.mse_const(p, c) if kind == R.MSE else SL.bce_logits_const(p, c)


def check_grad(key, got, kind, p, t, gout, n, r=2, wa=None, wb=None):
    """A gradient against fp64 within grad_bound; for the exact kinds also bit-equal to the fp32 formula, and exactly
    0 where p == t."""
    scale = R.grad_scale(gout, 1.0 if wa is None else wa, 1.0 if wb is None else wb, n)
    ref = R.loss_grad_ref(kind, p, t, scale)
    got = got.detach().cpu().reshape(-1)
    note(key, (got.double() - ref).abs(), R.grad_bound(kind, p, t, scale, r))
    if kind != R.BCE:
        zero = ref == 0
        assert bool((got[zero] == 0).all()), f"{key}: gradient not exactly 0 where p == t"
        # fp32 division on the card is correctly rounded (profiles/edge_loss/README.md), so the gradient also equals
        # the fp32 formula evaluated by torch on the CPU, bit for bit
        g32 = R.grad_scale_f32(gout, wa, wb, n)
        assert_same(got, g32 * R.loss_dgrad(kind, p, t).to(F32), key + " (fp32 formula)")


def grad_of(v, p, gout):
    (g,) = torch.autograd.grad(v, p, grad_outputs=torch.tensor(gout, dtype=F32, device=DEV), retain_graph=True)
    torch.cuda.synchronize()
    return g


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("name,kind,const", FORMS, ids=[f[0] for f in FORMS])
def test_l1_mse(name, kind, const, n):
    p, t = R.loss_operands(kind, n, seed=n, const=const)
    pd = p.to(F32).to(DEV).requires_grad_(True)
    v = wrapped_loss(kind, pd, t.to(F32).to(DEV) if const is None else None, const)
    assert_same(v, R.value_f32(kind, p, t), f"{name} n={n} value")
    for gout in GOUTS:
        check_grad(f"{name} n={n} gout={gout:.3g} grad", grad_of(v, pd, gout), kind, p, t, gout, n)


@pytest.mark.parametrize("n", [257, 4097])
def test_loss_tensor_target(n):
    """A tensor target for the MSE and BCE kinds (the C API allows it; loss.py has no such form)."""
    p, t = R.loss_operands(R.MSE, n, seed=3 * n)
    v, g = raw_loss(R.MSE, p.to(F32).to(DEV), t.to(F32).to(DEV), 7.0, GOUTS[1])  # (the constant must be ignored)
    assert_same(v, R.value_f32(R.MSE, p, t), f"mse tensor target n={n} value")
    check_grad(f"mse tensor target n={n} grad", g, R.MSE, p, t, GOUTS[1], n)
    x = R.bce_inputs(n, seed=n)
    lab = torch.tensor([R.f32(c) for c in (1.0, -1.0, 0.0, 0.9)], dtype=F64)[torch.arange(n) % 4]
    v, g = raw_loss(R.BCE, x.to(F32).to(DEV), lab.to(F32).to(DEV), 7.0, GOUTS[1])
    note(f"bce tensor target n={n} value", (v.double().cpu() - R.loss_value(R.BCE, x, lab)).abs(), R.bce_mean_bound(x, lab))
    check_grad(f"bce tensor target n={n} grad", g, R.BCE, x, lab, GOUTS[1], n)


@pytest.mark.parametrize("name,kind,const", [FORMS[0], FORMS[2]], ids=["l1", "mse1"])
def test_loss_grad_grid_stride(name, kind, const):
    """n = 8192*256 + 4097: loss_bwd_kernel's grid is capped, every thread strides (and 513 partials forward)."""
    n = STRIDE_N
    p, t = R.loss_operands(kind, n, seed=11, const=const)
    pd = p.to(F32).to(DEV).requires_grad_(True)
    v = wrapped_loss(kind, pd, t.to(F32).to(DEV) if const is None else None, const)
    assert_same(v, R.value_f32(kind, p, t), f"{name} n={n} value")
    check_grad(f"{name} n={n} grad", grad_of(v, pd, GOUTS[1]), kind, p, t, GOUTS[1], n)


BCE_LABELS = [1.0, -1.0, 0.0, 0.9]
BCE_NS = [1000, 9000]


def check_bce_extremes(key, got, x, label, g32):
    """At x = +-1e4 the sigmoid is exactly 1 / 0: the gradient is exactly (1 - t) or (0 - t) times the fp32 scale."""
    got = got.detach().cpu().reshape(-1)
    t32 = torch.tensor(label, dtype=F32)
    for i in (x == 1e4).nonzero().flatten().tolist():
        assert_same(got[i], g32 * (torch.tensor(1.0, dtype=F32) - t32), f"{key} x=1e4 at {i}")
    for i in (x == -1e4).nonzero().flatten().tolist():
        assert_same(got[i], g32 * (torch.tensor(0.0, dtype=F32) - t32), f"{key} x=-1e4 at {i}")


@pytest.mark.parametrize("n", BCE_NS)
@pytest.mark.parametrize("label", BCE_LABELS)
def test_bce(label, n):
    x = R.bce_inputs(n, seed=n + 1)
    t = R.f32(label)
    xd = x.to(F32).to(DEV).requires_grad_(True)
    v = SL.bce_logits_const(xd, label)
    note(f"bce label={label} n={n} value", (v.detach().double().cpu() - R.loss_value(R.BCE, x, t)).abs(),
         R.bce_mean_bound(x, t))
    for gout in GOUTS:
        g = grad_of(v, xd, gout)
        check_grad(f"bce label={label} n={n} gout={gout:.3g} grad", g, R.BCE, x, t, gout, n)
        check_bce_extremes(f"bce label={label} n={n} gout={gout:.3g}", g, x, label, R.grad_scale_f32(gout, n=n))


# ================================================================== e. fused objectives
LAMBDAS = (5.0, 0.1, 0.3)  # lambda1, lambda2, lambda3: none a power of two
D_SHAPES = [(1, 1, 30, 30), (4096,), (4097,), (1,)]
G_SHAPES = [(4097,), (2048 * 256 + 1,), (1, 1, 30, 30), (1,)]  # data1, data2 (strided backward), G1, G2


def d_case(ls, seed=0):
    """Four logits tensors (fake1, real1, fake2, real2) of unequal size and their constant targets."""
    kind = R.BCE if ls else R.MSE
    consts = [-1.0 if ls else 0.0, 1.0] * 2
    if ls:
        ps = [R.bce_inputs(max(60, math.prod(s)), 40 + seed + k) for k, s in enumerate(((900,), (4096,), (4097,), (60,)))]
    else:
        ps = [R.loss_operands(kind, math.prod(s), 40 + seed + k, const=c)[0].reshape(s)
              for k, (s, c) in enumerate(zip(D_SHAPES, consts))]
    return kind, ps, consts


def g_case(ls, seed=0):
    """(preds, targets, kinds, consts) of data1, data2, G1, G2."""
    kind = R.BCE if ls else R.MSE
    d1 = R.loss_operands(R.L1, math.prod(G_SHAPES[0]), 50 + seed)
    d2 = R.loss_operands(R.L1, math.prod(G_SHAPES[1]), 52 + seed)
    if ls:
        c1, c2 = R.bce_inputs(900, 54 + seed), R.bce_inputs(60, 55 + seed)
    else:
        c1 = R.loss_operands(kind, 900, 54 + seed, const=1.0)[0].reshape(G_SHAPES[2])
        c2 = R.loss_operands(kind, 1, 55 + seed, const=1.0)[0]
    return [d1[0], d2[0], c1, c2], [d1[1], d2[1], 1.0, 1.0], [R.L1, R.L1, kind, kind]


def check_value(key, got, kind, p, t):
    """A sub-loss: exact kinds must equal float32(fp64 mean), BCE is held to bce_mean_bound."""
    if kind == R.BCE:
        note(key, (got.detach().double().cpu() - R.loss_value(kind, p, t)).abs(), R.bce_mean_bound(p, t))
    else:
        assert_same(got.detach().reshape(()), R.value_f32(kind, p, t), key)


def up(p, grad=True):
    return p.to(F32).to(DEV).requires_grad_(grad)


def run_d(ls):
    l1, l2, l3 = LAMBDAS
    kind, ps, consts = d_case(ls)
    adv = SL.AdversarialLoss(ls=ls)
    dev = [up(p) for p in ps]
    D, D1, D2 = SL.d_objective(adv, *dev, l2, l3)
    vals = raw_multi_fwd([kind] * 4, consts, [d.detach() for d in dev], [None] * 4, L.LOSS_COMBINE_D, (l2, l3))
    tag = "D bce" if ls else "D mse"
    for k in range(4):
        check_value(f"{tag} vals[{k}]", vals[k], kind, ps[k], consts[k])
    # the documented fp32 operation sequence on the sub-losses (for the exact kinds these equal the reference means)
    eD, e1, e2 = R.combine_d(vals[:4].cpu(), l2, l3)
    if not ls:
        eD, e1, e2 = R.combine_d([R.value_f32(kind, p, c) for p, c in zip(ps, consts)], l2, l3)
    for got, exp, nm in ((D, eD, "D"), (D1, e1, "D1"), (D2, e2, "D2"), (vals[6], eD, "D (C API)"), (vals[4], e1, "vals[4]"),
                         (vals[5], e2, "vals[5]")):
        assert_same(got.detach().reshape(()), exp, f"{tag} {nm}")
    for gout in GOUTS:
        gs = torch.autograd.grad(D, dev, grad_outputs=torch.tensor(gout, dtype=F32, device=DEV), retain_graph=True)
        torch.cuda.synchronize()
        for k, g in enumerate(gs):
            check_grad(f"{tag} grad[{k}] gout={gout:.3g}", g, kind, ps[k].reshape(-1), consts[k], gout, ps[k].numel(), r=4,
                       wa=(l2, l2, l3, l3)[k], wb=0.5)


def raw_multi_fwd(kinds, consts, preds, targets, mode, w):
    """stc_loss_multi_fwd through the C API with NaN-filled outputs: [vals[0..5], D or G] (unwritten ones stay NaN)."""
    lib = L.lib()
    n_arr = SL._arr(ctypes.c_int64, [p.numel() for p in preds])
    part = torch.full((lib.stc_loss_multi_parts(4, n_arr),), NAN, device=DEV)
    vbuf, vals = arena((6,), F32)
    obuf, out = arena((1,), F32)
    L.check(lib.stc_loss_multi_fwd(4, SL._arr(ctypes.c_int32, kinds), SL._arr(ctypes.c_float, consts),
                                   SL._arr(ctypes.c_void_p, [p.data_ptr() for p in preds]),
                                   SL._arr(ctypes.c_void_p, [None if t is None else t.data_ptr() for t in targets]), n_arr,
                                   mode, SL._arr(ctypes.c_float, list(w) + [0.0] * (3 - len(w))), L.ptr(part), L.ptr(vals),
                                   L.ptr(out), L.stream()), "stc_loss_multi_fwd")
    torch.cuda.synchronize()
    guards_intact(vbuf, "multi vals")
    guards_intact(obuf, "multi out")
    assert not bool(torch.isnan(part).any())
    return torch.cat((vals, out))


def test_d_objective_exact():
    run_d(False)


def test_multi_fwd_many_partials():
    """A term of 256 * 4096 + 1 elements: loss_multi_final_kernel's strided second pass over its 257 partials, the
    last of them a single element; the other terms start right behind it in the block map."""
    sizes, consts = (256 * 4096 + 1, 1, 4097, 255), [0.0, 1.0, 0.0, 1.0]
    ps = [R.loss_operands(R.MSE, n, 90 + k, const=c)[0] for k, (n, c) in enumerate(zip(sizes, consts))]
    vals = raw_multi_fwd([R.MSE] * 4, consts, [up(p, False) for p in ps], [None] * 4, L.LOSS_COMBINE_D, LAMBDAS[1:])
    exp = [R.value_f32(R.MSE, p, c) for p, c in zip(ps, consts)]
    eD, e1, e2 = R.combine_d(exp, *LAMBDAS[1:])
    for k, e in enumerate(exp + [e1, e2, eD]):
        assert_same(vals[k].reshape(()), e, f"many partials vals[{k}]")


def run_g(ls):
    l1, l2, l3 = LAMBDAS
    preds, targets, kinds = g_case(ls)
    adv = SL.AdversarialLoss(ls=ls)
    dev = [up(p) for p in preds]
    tdev = [up(t, False) if torch.is_tensor(t) else None for t in targets]
    G, G1, G2, data1, data2 = SL.g_objective(adv, dev[0], tdev[0], dev[1], tdev[1], dev[2], dev[3], l1, l2, l3)
    vals = raw_multi_fwd(kinds, [0.0, 0.0, 1.0, 1.0], [d.detach() for d in dev], tdev, L.LOSS_COMBINE_G, LAMBDAS)
    tag = "G bce" if ls else "G mse"
    for k, got in enumerate((data1, data2, G1, G2)):
        check_value(f"{tag} term {k}", got, kinds[k], preds[k], targets[k])
        assert_same(vals[k].reshape(()), got.detach().reshape(()), f"{tag} vals[{k}] (C API)")
    assert bool(torch.isnan(vals[4:6]).all()), "G writes four sub-losses"
    eG = R.combine_g(vals[:4].cpu(), *LAMBDAS)
    if not ls:
        eG = R.combine_g([R.value_f32(k, p, t) for k, p, t in zip(kinds, preds, targets)], *LAMBDAS)
    assert_same(G.detach().reshape(()), eG, f"{tag} G")
    assert_same(vals[6].reshape(()), eG, f"{tag} G (C API)")
    for gout in GOUTS:
        gs = torch.autograd.grad(G, dev, grad_outputs=torch.tensor(gout, dtype=F32, device=DEV), retain_graph=True)
        torch.cuda.synchronize()
        for k, g in enumerate(gs):
            t = targets[k].reshape(-1) if torch.is_tensor(targets[k]) else targets[k]
            check_grad(f"{tag} grad[{k}] gout={gout:.3g}", g, kinds[k], preds[k].reshape(-1), t, gout, preds[k].numel(),
                       r=4, wa=(1.0, l1, l2, l3)[k], wb=1.0)


def test_g_objective_exact():
    run_g(False)


@pytest.mark.parametrize("which", ["D", "G"])
def test_objectives_bce(which):
    """ls=True: BCE with labels 1 / -1 on the extreme logits of section d."""
    (run_d if which == "D" else run_g)(True)


def test_objective_partial_grads():
    """The objective node with only some inputs requiring a gradient (NULL pointers inside the term list)."""
    l1, l2, l3 = LAMBDAS
    kind, ps, consts = d_case(False, seed=7)
    adv = SL.AdversarialLoss(ls=False)
    for need in ((False, True, True, False), (True, False, True, True)):
        dev = [up(p, nd) for p, nd in zip(ps, need)]
        D, _, _ = SL.d_objective(adv, *dev, l2, l3)
        wanted = [d for d, nd in zip(dev, need) if nd]
        gs = iter(torch.autograd.grad(D, wanted, grad_outputs=torch.tensor(GOUTS[1], dtype=F32, device=DEV)))
        torch.cuda.synchronize()
        for k, nd in enumerate(need):
            if nd:
                check_grad(f"D partial {need} grad[{k}]", next(gs), kind, ps[k].reshape(-1), consts[k], GOUTS[1],
                           ps[k].numel(), r=4, wa=(l2, l2, l3, l3)[k], wb=0.5)


@pytest.mark.parametrize("n", [900, 2048 * 256 + 1])
@pytest.mark.parametrize("real", [True, False])
def test_d_term_grad(real, n):
    """stc_loss_multi_bwd with one term (loss.d_term_grad), also over its 2048-block cap."""
    adv = SL.AdversarialLoss(ls=False)
    c = 1.0 if real else 0.0
    p = R.loss_operands(R.MSE, n, seed=60 + n % 7, const=c)[0]
    go = torch.tensor(GOUTS[1], dtype=F32, device=DEV)
    g = SL.d_term_grad(adv, up(p, False), LAMBDAS[1], go, real=real)
    torch.cuda.synchronize()
    check_grad(f"d_term_grad real={real} n={n}", g, R.MSE, p, c, GOUTS[1], n, r=4, wa=LAMBDAS[1], wb=0.5)


MULTI8_N = [1, 255, 257, 4096, 4097, 900, 133, 5000]
MULTI8_KIND = [R.L1, R.MSE, R.MSE, R.L1, R.BCE, R.MSE, R.BCE, R.L1]
MULTI8_WA = [1.0, 5.0, 0.1, 0.3, 0.1, 0.3, 5.0, 0.7]
MULTI8_WB = [1.0, 0.5, 0.5, 1.0, 0.5, 0.5, 1.0, 0.3]


def multi8_case():
    """8 terms of mixed kinds and sizes: (kinds, consts, preds, targets or None)."""
    preds, targets, consts = [], [], []
    for k, (n, kind) in enumerate(zip(MULTI8_N, MULTI8_KIND)):
        if kind == R.BCE:
            preds.append(R.bce_inputs(n, 70 + k))
            targets.append(None)
            consts.append(-1.0 if k == 4 else 0.9)
        elif kind == R.MSE and k == 2:  # a tensor target for an MSE term
            p, t = R.loss_operands(R.MSE, n, 70 + k)
            preds.append(p)
            targets.append(t)
            consts.append(7.0)
        elif kind == R.MSE:
            preds.append(R.loss_operands(R.MSE, n, 70 + k, const=1.0)[0])
            targets.append(None)
            consts.append(1.0)
        else:
            p, t = R.loss_operands(R.L1, n, 70 + k)
            preds.append(p)
            targets.append(t)
            consts.append(0.0)
    return MULTI8_KIND, consts, preds, targets


@pytest.mark.parametrize("nterm,null", [(1, ()), (8, ()), (8, (0, 3, 7)), (8, (1, 2, 4, 5, 6))],
                         ids=["one", "eight", "eight_null_first_middle_last", "eight_only_first_middle_last"])
def test_multi_bwd_null_grads(nterm, null):
    """stc_loss_multi_bwd with 1 and 8 terms; NULL gradient pointers skip a term: the other gradients are right and
    the poisoned buffers standing where the skipped ones would be are untouched."""
    kinds, consts, preds, targets = (x[:nterm] for x in multi8_case())
    gout = GOUTS[1]
    pd = [up(p, False) for p in preds]
    td = [None if t is None else up(t, False) for t in targets]
    slots = [arena((p.numel(),), F32) for p in preds]
    go = torch.tensor([gout], dtype=F32, device=DEV)
    A = SL._arr
    L.check(L.lib().stc_loss_multi_bwd(
        nterm, A(ctypes.c_int32, kinds), A(ctypes.c_float, consts), A(ctypes.c_void_p, [p.data_ptr() for p in pd]),
        A(ctypes.c_void_p, [None if t is None else t.data_ptr() for t in td]),
        A(ctypes.c_int64, [p.numel() for p in pd]), A(ctypes.c_float, MULTI8_WA[:nterm]),
        A(ctypes.c_float, MULTI8_WB[:nterm]), L.ptr(go),
        A(ctypes.c_void_p, [None if k in null else v.data_ptr() for k, (_, v) in enumerate(slots)]), L.stream()),
        "stc_loss_multi_bwd")
    torch.cuda.synchronize()
    for k, (buf, v) in enumerate(slots):
        what = f"multi_bwd nterm={nterm} null={null} term {k}"
        if k in null:
            assert bool(torch.isnan(buf).all()), f"{what}: a skipped gradient was written"
            continue
        guards_intact(buf, what)
        t = consts[k] if targets[k] is None else targets[k]
        check_grad(what, v, kinds[k], preds[k], t, gout, preds[k].numel(), r=4, wa=MULTI8_WA[k], wb=MULTI8_WB[k])


# ================================================================== f. weight packer
PACK_SHAPES = [(3, 5), (8, 8), (17, 33), (64, 4)]


def pack_pads(mode, P, Q, wide):
    """N_pad: the next multiple of 16 (64 when ``wide``), C_pad: of 8 (32)."""
    n, c = (P, Q) if mode in R.N_IS_P else (Q, P)
    a, b = (64, 32) if wide else (16, 8)
    return -(-n // a) * a, -(-c // b) * b


def pack_case(mode, P, Q, wide, dt, seed=0, unique=True):
    """(weight fp32 [P, Q, 4, 4], expected packed operand of dt, N_pad, C_pad)."""
    W = R.pack_weights(P, Q, 80 + seed, unique)
    n_pad, c_pad = pack_pads(mode, P, Q, wide)
    return W.to(F32), R.pack_ref(mode, W, n_pad, c_pad).to(dt), n_pad, c_pad


@pytest.mark.parametrize("dt", [F32, BF], ids=dn)
@pytest.mark.parametrize("wide", [False, True], ids=["pad16x8", "pad64x32"])
@pytest.mark.parametrize("P,Q", PACK_SHAPES, ids=lambda v: str(v))
@pytest.mark.parametrize("mode", R.PACK_MODES)
def test_pack_weight(mode, P, Q, wide, dt):
    W, exp, n_pad, c_pad = pack_case(mode, P, Q, wide, dt)
    buf, out = arena(exp.shape, dt)
    Wd = W.to(DEV)
    L.check(L.lib().stc_pack_weight(L.dtype_code(dt), mode, L.ptr(Wd), P, Q, L.ptr(out), n_pad, c_pad, L.stream()),
            "stc_pack_weight")
    torch.cuda.synchronize()
    what = f"pack mode {mode} {P}x{Q} -> {n_pad}x{c_pad} {dn(dt)}"
    assert_same(out, exp, what)  # (pad rows and columns of exp are zeros)
    guards_intact(buf, what)
    if not wide and dt == F32:  # the wrapper the engine uses
        assert_same(ops.pack(mode, Wd, n_pad, c_pad, dt), exp, what + " (ops.pack)")


def run_pack_multi(jobs, dt, what):
    """jobs: [(mode, P, Q, wide, unique)] as one stc_pack_weights launch."""
    cases = [pack_case(m, P, Q, wide, dt, seed=i, unique=u) for i, (m, P, Q, wide, u) in enumerate(jobs)]
    Ws = [c[0].to(DEV) for c in cases]
    outs = [arena(c[1].shape, dt) for c in cases]
    descs = (L.PackDesc * len(jobs))(*[L.PackDesc(j[0], j[1], j[2], c[2], c[3], 0, w.data_ptr(), o[1].data_ptr())
                                       for j, c, w, o in zip(jobs, cases, Ws, outs)])
    L.check(L.lib().stc_pack_weights(L.dtype_code(dt), len(jobs), descs, L.stream()), "stc_pack_weights")
    torch.cuda.synchronize()
    for i, (c, (buf, out)) in enumerate(zip(cases, outs)):
        assert_same(out, c[1], f"{what} descriptor {i} {jobs[i]}")
        guards_intact(buf, f"{what} descriptor {i}")


def multi_jobs(n):
    return [(i % 5, *PACK_SHAPES[(i // 5 + i) % 4], bool(i % 3 == 1), True) for i in range(n)]


@pytest.mark.parametrize("dt", [F32, BF], ids=dn)
@pytest.mark.parametrize("n", [1, 2, L.PACK_MAX])
def test_pack_weights(n, dt):
    run_pack_multi(multi_jobs(n), dt, f"pack_weights n={n} {dn(dt)}")


@pytest.mark.parametrize("dt", [F32, BF], ids=dn)
def test_pack_weights_strided(dt):
    """One descriptor over its 1024-block share (N_pad * C_pad = 528 * 512 > 1024 * 256: the first blocks stride)
    between two small ones."""
    jobs = [(R.PACK_CONV_FWD, 3, 5, False, True), (R.PACK_CONVT_FWD, 512, 520, False, False),
            (R.PACK_CONV_DGRAD, 17, 33, False, True)]
    assert math.prod(pack_pads(*jobs[1][:4])) > 1024 * 256
    run_pack_multi(jobs, dt, f"pack_weights strided {dn(dt)}")
