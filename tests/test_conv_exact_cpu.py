"""The integer-operand helper of the bit-exact conv tests (tests/conv_exact_ref.py), checked without a GPU: the
preconditions and rounding shares of every case tests/test_gpu_conv_exact.py launches, torch's own fp32 CPU
convolution reproducing the fp64 reference bit for bit on these operands, the sensitivity of the expected tensors to
a single removed product, and the one-pixel condition of every statistics case."""
import pytest
import torch
import torch.nn.functional as F

import conv_exact_ref as R
import test_gpu_conv_exact as G
from stcgan_amd import _lib as L

FWD = G.forward_cases()
WG = sorted({c for c in G.WGRAD} | {c for c, _, _ in G.WGRAD_FORCED} | {c for c, _ in G.WGRAD_VIEWS})


def _ids(c):
    return f"{G.KNAME[c[0]]}-{G.cid(c[1])}-s{c[2]}-{'bias' if c[3] else 'nobias'}"


def _conv32(kname, x, w, b):
    x, w = x.float(), w.float()
    b = None if b is None else b.float()
    if kname in ("conv_s2", "conv_s1"):
        return F.conv2d(x, w, b, 2 if kname == "conv_s2" else 1, 1)
    return F.conv_transpose2d(x, w, b, 2 if kname == "convT_s2" else 1, 1)


@pytest.mark.parametrize("c", FWD, ids=_ids)
def test_forward_case(c):
    """Precondition and (K >= 1024) rounding shares hold -- asserted inside ``operands`` --, the operands are
    integers in range without zeros and exact in bf16, the expected tensors are the exact fp32 value and its
    round-to-nearest-even bf16, and torch's fp32 CPU convolution equals the fp64 reference bit for bit."""
    kind, case, seed, bias = c
    x, w, b, exp_bf, exp_f32, ref = G.operands(kind, case, seed, bias)
    r = 16 if case[1] == 8 else 8
    for t, lim in ((x, r), (w, r)) + (((b, 64),) if bias else ()):
        assert bool((t == t.round()).all()) and float(t.abs().max()) <= lim and float(t.abs().min()) >= 1
        assert torch.equal(t.to(torch.bfloat16).double(), t)
    assert torch.equal(exp_f32.double(), G.nhwc(ref))
    assert torch.equal(exp_bf, exp_f32.to(torch.bfloat16))
    x_nchw = x.permute(0, 3, 1, 2)
    assert torch.equal(_conv32(G.KNAME[kind], x_nchw, w, b).double(), ref)


def test_share_figures():
    """The shares quoted in DESIGN.md: at Cin = 64 / 128 (conv-s2) and at the 8-channel [-16, 16] stem well over a
    quarter of the reference values need rounding and well over 5 % are exact ties."""
    for kind, case in ((L.CONV_S2, (2, 64, 128, 32, 32)), (L.CONV_S2, (2, 128, 256, 16, 16)),
                       (L.CONV_S2, (2, 8, 64, 64, 64)), (L.CONV_S2, (4, 512, 512, 4, 4))):
        nr, tie = R.rounding_shares(G.operands(kind, case, 0, False)[5])
        print(f"{G.KNAME[kind]} {case}: {nr:.1%} need rounding, {tie:.1%} ties")
        assert nr >= 0.4 and tie >= 0.1


@pytest.mark.parametrize("kname", R.KINDS)
def test_one_removed_product_changes_the_expected_tensor(kname):
    """Operands exclude zero, so zeroing one input element changes every output it reaches and removing a single
    product changes exactly one expected element."""
    x, w, b, ref = R.fwd_case(kname, 1, 8, 16, 6, 6, 0, 8, False)
    changed, single = R.drop_one_product(kname, x, w, idx=(0, 7, 2, 2))  # (the last weight element belongs to input channel 7)
    assert changed >= 16 and single == 1
    # ... and the bf16 expectation sees it too wherever the change survives rounding: check one explicitly
    x2 = x.clone()
    x2[0, 7, 2, 2] = 0.0
    assert not torch.equal(R.expect_bf16(R.conv_ref(kname, x2, w)), R.expect_bf16(ref))


def test_precondition_rejects_an_inexact_case():
    with pytest.raises(AssertionError):
        R.require_exact(torch.tensor([2.0 ** 24]))
    with pytest.raises(AssertionError):
        R.require_exact(torch.tensor([2.0 ** 22]), unit=0.25)
    R.require_exact(torch.tensor([2.0 ** 24 - 1]))
    with pytest.raises(AssertionError):
        R.expect_f32(torch.tensor([2.0 ** 24 + 1], dtype=torch.float64))


def test_bf16_expectation_rounds_to_nearest_even():
    # spacing 2 from 256, 4 from 512: 257, 259, 514 and 518 are ties (to the even mantissa), 513 and 515 are not
    v = torch.tensor([256.0, 257.0, 259.0, 513.0, 514.0, 515.0, 518.0, -513.0], dtype=torch.float64)
    exp = torch.tensor([256.0, 256.0, 260.0, 512.0, 512.0, 516.0, 520.0, -512.0])
    assert torch.equal(R.expect_bf16(v).float(), exp)
    nr, tie = R.rounding_shares(v)
    assert nr == 0.875 and tie == 0.5


def test_activation_expectations():
    v = torch.tensor([3.0, -3.0, -257.0, 0.0, -1.0], dtype=torch.bfloat16)
    s = torch.tensor(0.2, dtype=torch.float32)
    got = R.act_bf16(v, 0.2).float()
    assert torch.equal(got[:2], torch.tensor([3.0, float((torch.tensor(-3.0) * s).to(torch.bfloat16))]))
    assert torch.equal(R.act_bf16(v, 0.0).float(), torch.tensor([3.0, -0.0, -0.0, 0.0, -0.0]))
    assert torch.equal(R.dact(v, 0.2), torch.where(v.float() > 0, torch.tensor(1.0), s))


@pytest.mark.parametrize("c", G.stats_cases(), ids=_ids)
def test_statistics_bounds_see_one_pixel(c):
    """The one-pixel condition with the longest accumulation chain any plan of the case can have (the largest tile,
    or the split-K reduction launch over the case's rows): the bounds the GPU test derives are never wider."""
    kind, case, seed, bias = c
    B, Cin, Cout, GH, GW = case
    ref = G.operands(kind, case, seed, bias)[5]
    m = max(G.TILE_STEPS_MAX, G.reduce_steps((4 if kind == L.CONVT_S2 else 1) * B * GH * GW, Cout))
    bm, bv = R.stats_bounds(ref, m)
    rm, rv = R.one_pixel_margin(ref, bm, bv)
    print(f"m = {m}: one pixel moves the mean by {rm:.1f} and the variance by {rv:.1f} bounds")
    assert rm > 1 and rv > 1
    # the fp64 merge of exact per-row partials reproduces the reference statistics
    rows = G.nhwc(ref).reshape(-1, Cout)
    part = torch.stack((torch.ones_like(rows), torch.zeros_like(rows), torch.zeros_like(rows), rows), -1)
    N, mean, var = R.merge_partials(part)
    mr, vr, P = R.stats_ref(ref)
    assert bool((N == P).all())
    assert float((mean - mr).abs().max()) <= 1e-9 * float(ref.abs().max())
    assert float(((var - vr).abs() / vr).max()) <= 1e-9


@pytest.mark.parametrize("case", WG, ids=lambda c: "_".join(map(str, c)))
def test_wgrad_case(case):
    """Weight-gradient operands: precondition (asserted in wgrad_case), the fp32 reference exact."""
    role, s, B, Cin, Cout, H, W = case
    x, dy, gw = R.wgrad_case(role, s, B, Cin, Cout, H, W)
    assert torch.equal(R.expect_f32(gw).double(), gw)
    assert float(gw.abs().max()) > 0


def test_wgrad_fp32_cpu_matches_fp64():
    for case in (("conv", 2, 2, 64, 128, 32, 32), ("convT", 2, 2, 128, 64, 16, 16), ("conv", 1, 1, 64, 8, 9, 11)):
        role, s, B, Cin, Cout, H, W = case
        x, dy, gw = R.wgrad_case(role, s, B, Cin, Cout, H, W)
        if role == "conv":
            w = torch.zeros(Cout, Cin, 4, 4, requires_grad=True)
            y = F.conv2d(x.float(), w, None, s, 1)
        else:
            w = torch.zeros(Cin, Cout, 4, 4, requires_grad=True)
            y = F.conv_transpose2d(x.float(), w, None, 2, 1)
        (g32,) = torch.autograd.grad(y, w, dy.float())
        assert torch.equal(g32.double(), gw)


def test_prologue_values_are_exact():
    """scale in {+-1, +-2, 0.5}, integer shift, slope 0.5 / 0: quarter-integers, exact in bf16 and fp32."""
    x = R.acts((2, 32, 5, 5), 1, 16)
    tab = R.pro_table(32, 2)
    assert set(tab[0].tolist()) <= {1.0, -1.0, 2.0, -2.0, 0.5}
    for slope in (0.5, 0.0):
        v = R.prologue(x, tab, slope)
        assert bool((v * 4 == (v * 4).round()).all())
        assert torch.equal(v.to(torch.bfloat16).double(), v)
    for dt, kname, case, table, slope in G._pro_runs():  # (precondition asserted inside, in units of 1/4)
        x, w, b, tab, exp = G.pro_operands(kname, case, table, slope)
        assert bool((exp * 4 == (exp * 4).round()).all())


def test_rows_and_fp32_wgrad_operands():
    """The rows-kernel and fp32 weight-gradient cases: preconditions (asserted inside), padded rows zero, exact."""
    for B, Cin, H, W, rows, _ in G.ROWS_CASES:
        x, dy, gw = G.rows_operands(B, Cin, H, W, rows)
        assert float(dy[:, rows:].abs().max()) == 0.0 and gw.shape == (8, Cin, 4, 4)
    for role, s, case, pro in G._wgrad_f32_runs():
        D, Gt, dtab, gtab, gw = G.wgrad_f32_operands(role, s, case, pro)
        assert (dtab is not None) == pro and float(gw.abs().max()) > 0
        assert bool((gw * 8 == (gw * 8).round()).all())


def test_bn_backward_reference_matches_autograd():
    """conv_exact_ref.bn_backward_ref with tables that ARE the batch statistics of x equals autograd through
    F.batch_norm and the two activations (fp64)."""
    B, H, W, C = 3, 5, 4, 8
    x = R.acts((B, H, W, C), 11)
    v = R.acts((B, H, W, C), 12, 64)
    go = R.acts((B, H, W, C), 13)
    gamma = torch.linspace(-1.5, 1.5, C, dtype=torch.float64)
    beta = torch.linspace(-0.3, 0.3, C, dtype=torch.float64) + 0.01
    eps = 1e-5
    mean = x.mean(dim=(0, 1, 2))
    rstd = (x.var(dim=(0, 1, 2), unbiased=False) + eps).rsqrt()
    scale = gamma * rstd
    shift = beta - mean * scale
    ref = R.bn_backward_ref(v, x, go, (scale, shift, mean, rstd, gamma), 0.2, 0.0)
    xr = x.permute(0, 3, 1, 2).clone().requires_grad_(True)
    g, b = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    n = F.batch_norm(xr, None, None, g, b, True, 0.0, eps)
    s = float(torch.tensor(0.2, dtype=torch.float32))
    out = (F.leaky_relu(n, s) * v.permute(0, 3, 1, 2)).sum() + (F.relu(n) * go.permute(0, 3, 1, 2)).sum()
    gx, gg, gb = torch.autograd.grad(out, (xr, g, b))
    assert float((ref["dbeta"][0] - gb).abs().max()) <= 1e-9 * float(ref["dbeta"][1].max())
    assert float((ref["dgamma"][0] - gg).abs().max()) <= 1e-9 * float(ref["dgamma"][1].max())
    assert float((ref["dx"][0] - gx.permute(0, 2, 3, 1)).abs().max()) <= 1e-9 * float(ref["dx"][1].max())
    tabs = R.bn_tables(64, 5)
    assert float(tabs[0].abs().min()) >= 0.5 and float(tabs[1].abs().max()) < 0.3 and bool((tabs[0] < 0).any())
