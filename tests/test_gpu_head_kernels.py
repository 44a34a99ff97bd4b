"""The output-head codes of the conv epilogues (stc_conv_fwd / stc_conv_fwd_ex, STC_HEAD_*) and stc_head_bwd on the GPU.

Forward.  One smallest ragged ConvTranspose2d shape per kernel an activation can reach -- a non-zero code takes the
route tanh takes -- with the route asserted from ops.plan_of / ops.kernel_name and the eligibility rules restated here:
  smalln_kernel         fp32 and bf16, B 2, Cin 16, N 1 and 3, grid 5 x 7
  narrow_tiled_kernel   fp32, B 2, Cin 32, N 3, grid 17 x 9
  narrow_wk_kernel      bf16, (2,128,3,20,24) and (2,128,1,16,16) of test_gpu_igemm_bf16.NARROW (N = 1: its reduction)
  narrow_stream_kernel  bf16, (2,128,3,32,64) and (3,128,1,16,128) of NARROW_STREAM; with force (4, 1) the tiled kernel
  igemm_kernel<float>   N 3, B 1, grid 4 x 4, Cin 1368 -- the smallest multiple of 4 with N*K*4 > 64 KB (K = 4 Cin), where
                        use_smalln is false; split-K there, so the epilogue is splitk_reduce_kernel's.  Beyond the issue's
                        list: N 12, Cin 16 (no split), the tile's own epilogue.
Each case writes both output forms the call takes with tanh today (NCHW fp32; NHWC of the compute type) into NaN-filled
buffers with guards.  Checks: act="tanh" equals tanh=True bit for bit; "none" against fp64 F.conv_transpose2d at
test_gpu_igemm_bf16's bounds (fp32 outputs 2e-5 * max(scale, 1) + 1e-5, bf16 outputs 8e-3 * scale); "htanh" equals
clamp(y_none, -1, 1) bit for bit (rounding to bf16 is monotonic and keeps +-1, so also on bf16 outputs); "sigmoid" on
fp32 outputs within 1e-5 of the fp64 sigmoid of y_none -- the project's allowance for the activation epilogue on fp32
outputs -- and on bf16 outputs within that plus one bf16 rounding of a value in (0, 1), 2^-9, of the fp64 sigmoid of the
fp32 y_none; an invalid code raises.  Weights are scaled to a unit-variance pre-activation, and every case asserts, from
the reference alone, that at least 5 % of it lies beyond +-1 and at least 5 % inside.

Backward.  The quad and pixel shapes of test_gpu_edge_loss_family.test_tanh_bias_bwd, C 1-4, fp32 and bf16 dq, y at a
4-byte offset, with and without dbias: dq and dbias of none / sigmoid / htanh equal the exact reference
(tests/head_ref.py), and stc_head_bwd(act = 1) equals stc_tanh_bias_bwd bit for bit."""
import pytest
import torch
import torch.nn.functional as F

import head_ref as R
import test_gpu_edge_loss_family as E
from edge_loss_ref import gather_ref
from stcgan_amd import _lib as L
from stcgan_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
WORST = {}

# (id, dtype, B, Cin, N, grid H, grid W, force, kernel)
FWD = [
    ("smalln_f32_n1", F32, 2, 16, 1, 5, 7, None, "smalln"),
    ("smalln_f32_n3", F32, 2, 16, 3, 5, 7, None, "smalln"),
    ("smalln_bf16_n1", BF, 2, 16, 1, 5, 7, None, "smalln"),
    ("smalln_bf16_n3", BF, 2, 16, 3, 5, 7, None, "smalln"),
    ("narrow_tiled_f32", F32, 2, 32, 3, 17, 9, None, "narrow_tiled"),
    ("narrow_wk_n3", BF, 2, 128, 3, 20, 24, None, "narrow_wk"),
    ("narrow_wk_n1", BF, 2, 128, 1, 16, 16, None, "narrow_wk"),
    ("narrow_stream_n3", BF, 2, 128, 3, 32, 64, None, "narrow_stream"),
    ("narrow_stream_n1", BF, 3, 128, 1, 16, 128, None, "narrow_stream"),
    ("narrow_forced_n3", BF, 2, 128, 3, 32, 64, (4, 1), "narrow_forced"),
    ("narrow_forced_n1", BF, 3, 128, 1, 16, 128, (4, 1), "narrow_forced"),
    ("fp_tile_splitk", F32, 1, 1368, 3, 4, 4, None, "fp_tile_splitk"),
    ("fp_tile_direct", F32, 2, 16, 12, 5, 7, None, "fp_tile_direct"),
]


def use_smalln(dt, N, K):  # csrc/igemm.hip
    return N <= 8 and N * K * (4 if dt == F32 else 2) <= 64 * 1024


def assert_route(dt, B, Cin, N, GH, GW, kernel):
    plan = ops.plan_of(L.CONVT_S2, B, GH, GW, Cin, N, dt)
    name = ops.kernel_name(L.CONVT_S2, B, GH, GW, Cin, N, dt)[0]
    K = 4 * Cin
    narrow_tiled = Cin % (32 if dt == F32 else 64) == 0  # narrow_tiled_eligible; bf16: the bf16 narrow kernels first
    if kernel.startswith("fp_tile"):
        assert not use_smalln(dt, N, K) and plan[3] == 0 and name.startswith("igemm_kernel<float"), (plan, name)
        assert (plan[2] > 1) == (kernel == "fp_tile_splitk"), plan
        if kernel == "fp_tile_splitk":  # the smallest Cin (a multiple of 4) past the small-N limit
            assert use_smalln(dt, N, 4 * (Cin - 4))
        return
    assert use_smalln(dt, N, K) and plan[3] == 1, plan
    if kernel == "smalln":
        assert not narrow_tiled
    elif kernel == "narrow_tiled":
        assert dt == F32 and narrow_tiled and name == "narrow_tiled_kernel"
    elif kernel == "narrow_wk":
        assert dt == BF and name.startswith("narrow_wk_kernel"), name
    else:
        assert dt == BF and name.startswith("narrow_stream_kernel"), name


def run_conv(dt, B, xg, Cin, wp, N, GH, GW, bias, form, force, **kw):
    """One ConvT into a NaN arena; returns the output as NCHW on the CPU (fp32 outputs as they are, bf16 as bf16)."""
    if form == "nchw_f32":
        buf, y = E.arena((B, N, 2 * GH, 2 * GW), F32)
        ops.conv(L.CONVT_S2, B, L.nhwc_view(xg), Cin, wp, N, L.nchw_view(y), dt, bias=bias, out_f32=True, force=force,
                 **kw)
        out = y
    else:
        buf, y = E.arena((B, 2 * GH, 2 * GW, N), dt)
        ops.conv(L.CONVT_S2, B, L.nhwc_view(xg), Cin, wp, N, L.nhwc_view(y), dt, bias=bias, force=force, **kw)
        out = y.permute(0, 3, 1, 2)
    torch.cuda.synchronize()
    E.guards_intact(buf, f"{form} {kw}")
    out = out.contiguous().cpu()
    assert not bool(torch.isnan(out.float()).any()), f"{form} {kw}: unwritten outputs"
    return out


@pytest.mark.parametrize("case", FWD, ids=lambda c: c[0])
def test_forward_heads(case):
    name, dt, B, Cin, N, GH, GW, force, kernel = case
    assert_route(dt, B, Cin, N, GH, GW, kernel)
    g = torch.Generator().manual_seed(500 + len(name) + Cin + N)
    rnd = (lambda *s: torch.randn(s, generator=g)) if dt == F32 else (lambda *s: torch.randn(s, generator=g).to(BF).float())
    x = rnd(B, Cin, GH, GW)
    w = rnd(Cin, N, 4, 4) / (4 * Cin) ** 0.5  # 4 taps per output: a unit-variance pre-activation
    if dt == BF:
        w = w.to(BF).float()
    b = torch.randn(N, generator=g) * 0.25
    q64 = F.conv_transpose2d(x.double(), w.double(), b.double(), 2, 1)
    beyond = float((q64.abs() > 1).double().mean())
    assert beyond >= 0.05 and 1 - beyond >= 0.05, f"{name}: {beyond:.3f} of the pre-activation beyond +-1"
    scale = float(q64.abs().max())
    xg = x.permute(0, 2, 3, 1).contiguous().to(DEV, dt)
    wp = ops.pack(L.PACK_CONVT_FWD, w.to(DEV), N, Cin, dt)
    bg = b.to(DEV)
    args = (dt, B, xg, Cin, wp, N, GH, GW, bg)
    q32 = None
    for form in ("nchw_f32", "nhwc"):
        f32_out = form == "nchw_f32" or dt == F32
        y = {a: run_conv(*args, form, force, act=a) for a in R.HEADS}
        E.assert_same(y["tanh"], run_conv(*args, form, force, tanh=True), f"{name} {form} act='tanh' against tanh=True")
        E.assert_same(run_conv(*args, form, force, act=None), y["none"], f"{name} {form} act=None against 'none'")
        err = float((y["none"].double() - q64).abs().max())
        bound = 2e-5 * max(scale, 1.0) + 1e-5 if f32_out else 8e-3 * scale
        print(f"[head] {name} {form} none: max err {err:.3e}, bound {bound:.3e}")
        assert err <= bound, f"{name} {form} none: {err:.3e} > {bound:.3e}"
        E.assert_same(y["htanh"], y["none"].clamp(-1.0, 1.0), f"{name} {form} htanh against clamp(none)")
        clamped = float((y["htanh"].float().abs() == 1).double().mean())
        assert 0.05 <= clamped <= 0.95, clamped
        if f32_out:
            q32 = y["none"] if q32 is None else q32
            serr = float((y["sigmoid"].double() - R.head("sigmoid", y["none"].double())).abs().max())
            sbound = 1e-5
        else:  # a bf16 output: one rounding of a value in (0, 1) on top, against the fp32 pre-activation of this case
            serr = float((y["sigmoid"].double() - R.head("sigmoid", q32.double())).abs().max())
            sbound = 1e-5 + 2.0 ** -9
        key = f"{kernel} {'fp32' if f32_out else 'bf16'} output"
        WORST[key] = max(WORST.get(key, 0.0), serr)
        print(f"[head] {name} {form} sigmoid: max err {serr:.3e}, bound {sbound:.3e} (worst of {key}: {WORST[key]:.3e})")
        assert serr <= sbound, f"{name} {form} sigmoid: {serr:.3e} > {sbound:.3e}"
        terr = float((y["tanh"].double() - torch.tanh(y["none"].double() if f32_out else q32.double())).abs().max())
        assert terr <= sbound, f"{name} {form} tanh: {terr:.3e}"
        for bad in (4, -1):
            with pytest.raises(RuntimeError, match="epilogue code"):
                run_conv(*args, form, force, act=bad)


def test_conv_tanh_flag_and_act_must_agree():
    with pytest.raises(ValueError, match="tanh=True"):
        ops.conv(L.CONVT_S2, 1, None, 16, torch.empty(1, device=DEV), 1, None, F32, tanh=True, act="sigmoid")


# ================================================================== backward
def head_case(act, B, C, H, W, dt, seed):
    y, gy = R.operands(act, B, C, H, W, 4000 + seed)
    dq, db = R.head_bwd_ref(act, y, gy)
    return y.to(F32), gy.to(F32), gather_ref([dq], ops.vec(dt)).to(dt), db.to(F32), dq


@pytest.mark.parametrize("dt", [F32, BF], ids=E.dn)
@pytest.mark.parametrize("C", [1, 2, 3, 4])
@pytest.mark.parametrize("path,B,H,W", E.TANH_SHAPES, ids=lambda v: str(v))
@pytest.mark.parametrize("act", ["none", "sigmoid", "htanh"])
def test_head_bwd(act, path, B, H, W, C, dt):
    y, gy, exp_dq, exp_db, dq = head_case(act, B, C, H, W, dt, seed=C)
    nch = ops.stats_chunks(B, H, W)
    R.require_exact(dq, -(-B * H * W // nch) + 3)
    yd = E.offset_by_one(y) if path == "offset" else y.to(DEV)
    gd = gy.to(DEV)
    assert E.tanh_path(H, W, yd, gd) == ("quad" if path == "quad" else "pixel")
    what = f"head_bwd {act} {path} {B}x{C}x{H}x{W} {E.dn(dt)}"
    # with a dbias
    buf, dqt = E.arena(exp_dq.shape, dt)
    bbuf, db = E.arena((C,), F32)
    ops.head_bwd(yd, gd, L.nhwc_view(dqt), dt, act, dbias=db)
    torch.cuda.synchronize()
    E.assert_same(dqt, exp_dq, what + " dq")
    E.assert_same(db, exp_db, what + " dbias")
    E.guards_intact(buf, what + " dq")
    E.guards_intact(bbuf, what + " dbias")
    if act != "none":  # the torch fp32 form in the documented order: the same bits
        E.assert_same(dqt[..., :C].float(), R.dq_torch(act, y, gy).permute(0, 2, 3, 1).to(dt).float(), what + " torch form")
    # without: dq as before, no sum launched
    buf, dqt = E.arena(exp_dq.shape, dt)
    pbuf, part = E.arena((nch, C), F32)
    L.check(L.lib().stc_head_bwd(L.dtype_code(dt), R.CODES[act], B, C, H, W, L.ptr(yd), L.ptr(gd), L.nhwc_view(dqt),
                                 None, L.ptr(part), nch, L.stream()), "stc_head_bwd")
    torch.cuda.synchronize()
    E.assert_same(dqt, exp_dq, what + " dq, no dbias")
    E.guards_intact(buf, what + " dq, no dbias")
    E.guards_intact(pbuf, what + " partials")
    assert not bool(torch.isnan(part).any())


@pytest.mark.parametrize("dt", [F32, BF], ids=E.dn)
@pytest.mark.parametrize("C", [1, 2, 3, 4])
@pytest.mark.parametrize("path,B,H,W", E.TANH_SHAPES, ids=lambda v: str(v))
def test_head_bwd_tanh_is_tanh_bias_bwd(path, B, H, W, C, dt):
    """stc_head_bwd(act = 1) and stc_tanh_bias_bwd: the same bits, on real-valued operands (so the roundings count) and
    on the exact ones (equal to the reference)."""
    g = torch.Generator().manual_seed(77 + C)
    cases = [(torch.tanh(torch.randn((B, C, H, W), generator=g) * 1.5), torch.randn((B, C, H, W), generator=g), None)]
    ye, ge, exp_dq, exp_db, _ = head_case("tanh", B, C, H, W, dt, seed=C)
    cases.append((ye, ge, (exp_dq, exp_db)))
    for y, gy, exact in cases:
        yd = E.offset_by_one(y) if path == "offset" else y.to(DEV)
        gd = gy.to(DEV)
        outs = []
        for fn in (lambda *a, **k: ops.head_bwd(*a, "tanh", **k), ops.tanh_bias_bwd):
            buf, dqt = E.arena((B, H, W, ops.vec(dt)), dt)
            bbuf, db = E.arena((C,), F32)
            if fn is ops.tanh_bias_bwd:
                fn(yd, gd, L.nhwc_view(dqt), dt, dbias=db)
            else:
                ops.head_bwd(yd, gd, L.nhwc_view(dqt), dt, "tanh", dbias=db)
            torch.cuda.synchronize()
            E.guards_intact(buf, "dq")
            E.guards_intact(bbuf, "dbias")
            outs.append((dqt.clone(), db.clone()))
        what = f"head_bwd(tanh) against tanh_bias_bwd {path} {B}x{C}x{H}x{W} {E.dn(dt)}"
        E.assert_same(outs[0][0], outs[1][0], what + " dq")
        E.assert_same(outs[0][1], outs[1][1], what + " dbias")
        assert not bool(torch.isnan(outs[0][0].float()).any())
        if exact is not None:
            E.assert_same(outs[0][0], exact[0], what + " dq, exact")
            E.assert_same(outs[0][1], exact[1], what + " dbias, exact")


def test_head_bwd_invalid_code():
    y = torch.zeros((1, 1, 4, 4), device=DEV)
    dq = torch.zeros((1, 4, 4, 4), device=DEV)
    for bad in (4, -1):
        with pytest.raises(RuntimeError, match="stc_head_bwd: act="):
            ops.head_bwd(y, y, L.nhwc_view(dq), F32, bad)
