"""The reflect-padding kernels pinned bit-exactly with integer-valued operands (tests/reflect_ref.py,
tests/conv_exact_ref.py): forward, input gradient and weight gradient of a Conv2d k4 s2 / s1 p1 with
padding_mode="reflect" through stc_conv_pad_fwd / _dgrad / _wgrad, fp32 and bf16.

Every product and every partial sum of every order is exact in fp32 (sum |x||w| < 2^24, asserted per case on the CPU:
tests/test_reflect_ref_cpu.py), so an fp32 output EQUALS the fp64 reference and a bf16 output is exactly its
round-to-nearest-even rounding -- torch.equal, no tolerance.  That also pins the rounding rule of the input gradient:
the frame is fp32 and the fold adds before the one rounding (a frame stored in bf16 would fail here).  Output buffers
are pre-filled with NaN; channel-offset views live in twice-as-wide NaN buffers, so a read or write outside a view
shows."""
import ctypes

import pytest
import torch

import conv_exact_ref as R
import reflect_ref as P
from stcgan_amd import _lib as L
from stcgan_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF, F32 = torch.bfloat16, torch.float32
NAN = float("nan")
DTYPES = [F32, BF]
cid = lambda c: "x".join(map(str, c))  # noqa: E731
did = lambda d: "bf16" if d == BF else "fp32"  # noqa: E731


def kind_of(stride):
    return L.CONV_S2 if stride == 2 else L.CONV_S1


def nhwc(t, cpad=None):
    """NCHW fp64 -> NHWC, channels zero-padded to cpad."""
    v = t.permute(0, 2, 3, 1).contiguous()
    if cpad is not None and cpad > v.shape[-1]:
        v = torch.cat((v, torch.zeros(*v.shape[:-1], cpad - v.shape[-1], dtype=v.dtype)), -1)
    return v


def place(vals, dt, offset):
    """Upload NHWC values dense, or as the high channel half of a twice-as-wide NaN buffer: (buffer, view)."""
    C = vals.shape[-1]
    if not offset:
        buf = vals.to(DEV, dt).contiguous()
        return buf, L.nhwc_view(buf)
    buf = torch.full((*vals.shape[:-1], 2 * C), NAN, device=DEV, dtype=dt)
    buf[..., C:] = vals.to(DEV, dt)
    return buf, L.nhwc_view(buf, C)


def out_buf(shape, dt, offset):
    B, H, W, C = shape
    buf = torch.full((B, H, W, 2 * C if offset else C), NAN, device=DEV, dtype=dt)
    return buf, L.nhwc_view(buf, 0)  # (offset: the low half of the wider buffer -- pixel stride 2C)


def read_out(buf, C, what):
    got = buf[..., :C].contiguous().cpu()
    if buf.shape[-1] != C:
        assert bool(torch.isnan(buf[..., C:].float()).all()), f"{what}: an element outside the output view was written"
    return got


def same(got, exp, what):
    got, exp = got.detach().cpu(), exp.detach().cpu()
    assert got.shape == exp.shape and got.dtype == exp.dtype, (what, got.shape, exp.shape, got.dtype, exp.dtype)
    if not torch.equal(got, exp):
        bad = ((got != exp) | torch.isnan(got.float())).nonzero()
        first = tuple(bad[0].tolist())
        dims = ", ".join(f"d{d}: {sorted(set(bad[:, d].tolist()))[:10]}" for d in range(bad.shape[1]))
        raise AssertionError(f"{what}: {len(bad)} of {got.numel()} elements differ; {dims}; first {first}: got "
                             f"{float(got[first])} expected {float(exp[first])}; NaN: {int(torch.isnan(got.float()).sum())}")


def expect(ref64, dt):
    return R.expect_bf16(ref64) if dt == BF else R.expect_f32(ref64)


def cpad(c, dt):
    v = ops.vec(dt)
    return -(-c // v) * v


def forward(case, dt, pad=L.PAD_REFLECT, offset=False, bias=False):
    stride, B, Cin, Cout, H, W = case
    x, w, _, y, _, _ = P.case(*case)
    b = R.biases(Cout, 77) if bias else None
    xb, xv = place(nhwc(x), dt, offset)
    wp = ops.pack(L.PACK_CONV_FWD, w.float().to(DEV), Cout, Cin, dt)
    yb, yv = out_buf((B, y.shape[2], y.shape[3], Cout), dt, offset)
    ops.conv_pad(kind_of(stride), B, xv, Cin, wp, Cout, yv, dt, pad, bias=None if b is None else b.float().to(DEV))
    torch.cuda.synchronize()
    return read_out(yb, Cout, f"forward {case}"), (y if b is None else y + b[None, :, None, None])


def dgrad(case, dt, pad=L.PAD_REFLECT, offset=False):
    stride, B, Cin, Cout, H, W = case
    _, w, dy, _, dx, _ = P.case(*case)
    Cd = cpad(Cout, dt)  # the output gradient's channels, zero-padded to whole 16-byte chunks
    db, dv = place(nhwc(dy, Cd), dt, offset)
    mode = L.PACK_CONV_DGRAD if stride == 2 else L.PACK_CONV_S1_DGRAD
    wp = ops.pack(mode, w.float().to(DEV), Cin, Cd, dt)
    gb, gv = out_buf((B, H, W, Cin), dt, offset)
    kind = L.CONVT_S2 if stride == 2 else L.CONV_S1_DGRAD
    ops.conv_pad(kind, B, dv, Cd, wp, Cin, gv, dt, pad)
    torch.cuda.synchronize()
    return read_out(gb, Cin, f"input gradient {case}"), dx


def wgrad(case, dt, pad=L.PAD_REFLECT, offset=False):
    stride, B, Cin, Cout, H, W = case
    x, _, dy, _, _, dW = P.case(*case)
    Cd = cpad(Cout, dt)
    xb, xv = place(nhwc(x), dt, offset)
    db, dv = place(nhwc(dy, Cd), dt, offset)
    out = ops.wgrad(B, stride, dv, Cd, xv, Cin, Cin, dt, device=DEV, pad=pad)
    torch.cuda.synchronize()
    assert bool((out[Cout:] == 0).all()), "weight-gradient rows of the zero padding channels"
    return out[:Cout].cpu(), dW


RUN = {"fwd": forward, "dgrad": dgrad, "wgrad": wgrad}


@pytest.mark.parametrize("dt", DTYPES, ids=did)
@pytest.mark.parametrize("case", P.EXACT_CASES, ids=cid)
@pytest.mark.parametrize("what", ["fwd", "dgrad", "wgrad"])
def test_exact(what, case, dt):
    got, ref = RUN[what](case, dt)
    same(got, R.expect_f32(ref) if what == "wgrad" else nhwc(expect(ref, dt)), f"{what} {case} {did(dt)}")


@pytest.mark.parametrize("dt", DTYPES, ids=did)
@pytest.mark.parametrize("key", ["fwd", "dgrad", "dgrad_s2", "wgrad"])
def test_exact_split_k(key, dt):
    """Per direction (the input gradient in both strides) a case whose plan, read from the new query, splits the
    reduction."""
    case, what = P.SPLIT_CASES[key], key.split("_")[0]
    stride, B, Cin, Cout, H, W = case
    k, Cd = kind_of(stride), cpad(Cout, dt)
    if what == "fwd":
        ws, _, plan = ops.conv_pad_query(k, B, H, W, Cin, Cout, dt, L.PAD_REFLECT)
        splits = plan[2]
    elif what == "dgrad":
        ws, plan = ops.conv_pad_dgrad_query(k, B, H, W, Cd, Cin, dt, L.PAD_REFLECT)
        splits = plan[2]
    else:
        ws, plan = ops.wgrad_pad_query(stride, B, P.out_extent(H, stride), P.out_extent(W, stride), Cd, Cin, dt,
                                       L.PAD_REFLECT)
        splits = plan[3]
    assert splits > 1 and ws > 0, (what, case, plan)
    got, ref = RUN[what](case, dt)
    same(got, R.expect_f32(ref) if what == "wgrad" else nhwc(expect(ref, dt)), f"split {what} {case} {did(dt)}")


@pytest.mark.parametrize("dt", DTYPES, ids=did)
@pytest.mark.parametrize("case", [(2, 2, 24, 40, 2, 6), (2, 2, 8, 72, 34, 30), (1, 2, 64, 40, 5, 6)], ids=cid)
@pytest.mark.parametrize("what", ["fwd", "dgrad", "wgrad"])
def test_exact_channel_offset_views(what, case, dt):
    """Operands in the high channel half of NaN-filled wider buffers, the output in the low half of one (pixel stride
    twice the channel count): nothing outside a view is read or written."""
    got, ref = RUN[what](case, dt, offset=True)
    same(got, R.expect_f32(ref) if what == "wgrad" else nhwc(expect(ref, dt)), f"views {what} {case} {did(dt)}")


@pytest.mark.parametrize("dt", DTYPES, ids=did)
def test_exact_bias_and_f32_output(dt):
    """The epilogue's integer bias, and the fp32 output of a bf16 conv (the discriminator's logits layer form)."""
    case = (1, 2, 24, 1, 31, 31)
    got, ref = forward(case, dt, bias=True)
    same(got, nhwc(expect(ref, dt)), f"bias {did(dt)}")
    stride, B, Cin, Cout, H, W = case
    x, w, _, y, _, _ = P.case(*case)
    xb, xv = place(nhwc(x), dt, False)
    wp = ops.pack(L.PACK_CONV_FWD, w.float().to(DEV), Cout, Cin, dt)
    out = torch.full((B, Cout, H - 1, W - 1), NAN, device=DEV, dtype=F32)
    ops.conv_pad(L.CONV_S1, B, xv, Cin, wp, Cout, L.nchw_view(out), dt, L.PAD_REFLECT, out_f32=True)
    torch.cuda.synchronize()
    same(out, R.expect_f32(y), f"NCHW fp32 output {did(dt)}")


def old_ex(kind, B, xv, cin, wp, cout, yv, dt):
    """stc_conv_fwd_ex as the new entry points call it under STC_PAD_ZEROS: no bias, no statistics, force_plan NULL,
    the workspace of its own query."""
    gh, gw = (xv.H, xv.W) if kind == L.CONVT_S2 else (yv.H, yv.W)
    nbytes, _, _ = ops.conv_query(kind, B, gh, gw, cin, cout, dt)
    ws = torch.empty(max(int(nbytes), 1), dtype=torch.uint8, device=DEV)
    L.check(L.lib().stc_conv_fwd_ex(L.dtype_code(dt), kind, B, xv, cin, L.ptr(wp), cout, yv, None, 0, 0, None, 0, None,
                                    L.ptr(ws), int(nbytes), L.stream()), "stc_conv_fwd_ex")


@pytest.mark.parametrize("dt", DTYPES, ids=did)
@pytest.mark.parametrize("case", [(2, 2, 64, 72, 4, 6), (2, 1, 24, 8, 34, 30), (1, 1, 64, 72, 31, 31), (1, 2, 8, 1, 2, 3)],
                         ids=cid)
def test_zeros_is_the_old_entry_point(case, dt):
    """STC_PAD_ZEROS through each new entry point equals the old entry point bit for bit (Gaussian operands: real
    rounding, every summation order visible)."""
    stride, B, Cin, Cout, H, W = case
    k, Cd = kind_of(stride), cpad(Cout, dt)
    Ho, Wo = P.out_extent(H, stride), P.out_extent(W, stride)
    g = torch.Generator().manual_seed(5)
    x = torch.randn(B, H, W, Cin, generator=g).to(DEV, dt)
    dy = torch.randn(B, Ho, Wo, Cd, generator=g).to(DEV, dt)
    w = torch.randn(Cout, Cin, 4, 4, generator=g).to(DEV)
    xv, dv = L.nhwc_view(x), L.nhwc_view(dy)
    wp = ops.pack(L.PACK_CONV_FWD, w, Cout, Cin, dt)
    ya, yb = (torch.full((B, Ho, Wo, Cout), NAN, device=DEV, dtype=dt) for _ in range(2))
    ops.conv_pad(k, B, xv, Cin, wp, Cout, L.nhwc_view(ya), dt, L.PAD_ZEROS)
    old_ex(k, B, xv, Cin, wp, Cout, L.nhwc_view(yb), dt)
    mode, dk = (L.PACK_CONV_DGRAD, L.CONVT_S2) if stride == 2 else (L.PACK_CONV_S1_DGRAD, L.CONV_S1_DGRAD)
    wd = ops.pack(mode, w, Cin, Cd, dt)
    ga, gb = (torch.full((B, H, W, Cin), NAN, device=DEV, dtype=dt) for _ in range(2))
    ops.conv_pad(dk, B, dv, Cd, wd, Cin, L.nhwc_view(ga), dt, L.PAD_ZEROS)
    old_ex(dk, B, dv, Cd, wd, Cin, L.nhwc_view(gb), dt)
    wa = ops.wgrad(B, stride, dv, Cd, xv, Cin, Cin, dt, device=DEV, pad=L.PAD_ZEROS)
    wb = ops.wgrad(B, stride, dv, Cd, xv, Cin, Cin, dt, device=DEV)
    torch.cuda.synchronize()
    for a, b, what in ((ya, yb, "forward"), (ga, gb, "input gradient"), (wa, wb, "weight gradient")):
        assert not bool(torch.isnan(a.float()).any())
        same(a, b, f"zeros {what} {case} {did(dt)}")


def test_zeros_entry_point_against_stc_conv_fwd():
    """stc_conv_pad_fwd(STC_PAD_ZEROS), called directly, writes what ops.conv (stc_conv_fwd, the engine's default call)
    writes for the same operands."""
    h = L.lib()
    x = torch.randn(1, 4, 4, 8).to(DEV, BF)
    w = ops.pack(L.PACK_CONV_FWD, torch.randn(8, 8, 4, 4, device=DEV), 8, 8, BF)
    a, b = (torch.empty(1, 2, 2, 8, device=DEV, dtype=BF) for _ in range(2))
    ws = ctypes.c_int64()
    ops.conv(L.CONV_S2, 1, L.nhwc_view(x), 8, w, 8, L.nhwc_view(a), BF)
    assert h.stc_conv_pad_fwd(L.BF16, L.CONV_S2, L.PAD_ZEROS, 1, L.nhwc_view(x), 8, L.ptr(w), 8, L.nhwc_view(b), None, 0,
                              0, None, 0, None, None, 0, L.stream()) == 0
    torch.cuda.synchronize()
    same(a, b, "stc_conv_fwd against stc_conv_pad_fwd(zeros)")


@pytest.mark.parametrize("dt", DTYPES, ids=did)
@pytest.mark.parametrize("what", ["fwd", "dgrad", "wgrad"])
def test_twice_gives_identical_bits(what, dt):
    """Gaussian operands (so that an order change would show), the split-K case of each direction, run twice."""
    stride, B, Cin, Cout, H, W = P.SPLIT_CASES[what]
    k, Cd = kind_of(stride), cpad(Cout, dt)
    Ho, Wo = P.out_extent(H, stride), P.out_extent(W, stride)
    g = torch.Generator().manual_seed(9)
    x = torch.randn(B, H, W, Cin, generator=g).to(DEV, dt)
    dy = torch.randn(B, Ho, Wo, Cd, generator=g).to(DEV, dt)
    w = torch.randn(Cout, Cin, 4, 4, generator=g).to(DEV)
    outs = []
    for _ in range(2):
        if what == "fwd":
            o = torch.full((B, Ho, Wo, Cout), NAN, device=DEV, dtype=dt)
            ops.conv_pad(k, B, L.nhwc_view(x), Cin, ops.pack(L.PACK_CONV_FWD, w, Cout, Cin, dt), Cout, L.nhwc_view(o), dt,
                         L.PAD_REFLECT)
        elif what == "dgrad":
            o = torch.full((B, H, W, Cin), NAN, device=DEV, dtype=dt)
            mode, dk = (L.PACK_CONV_DGRAD, L.CONVT_S2) if stride == 2 else (L.PACK_CONV_S1_DGRAD, L.CONV_S1_DGRAD)
            ops.conv_pad(dk, B, L.nhwc_view(dy), Cd, ops.pack(mode, w, Cin, Cd, dt), Cin, L.nhwc_view(o), dt, L.PAD_REFLECT)
        else:
            o = ops.wgrad(B, stride, L.nhwc_view(dy), Cd, L.nhwc_view(x), Cin, Cin, dt, device=DEV, pad=L.PAD_REFLECT)
        torch.cuda.synchronize()
        assert not bool(torch.isnan(o.float()).any())
        outs.append(o.clone())
    same(outs[0], outs[1], f"twice {what} {did(dt)}")
