"""stc_conv3_fwd (Conv2d k3 s1 p1 forward and input gradient, csrc/conv3_bf16.hip) bit-exactly, with integer-valued
operands (tests/conv_exact_ref.py: operands in [-8, 8] without 0, integer biases; sum |x||w| < 2^24, so every partial
sum is exact in fp32 in any order and the bf16 output must equal the RNE of the exact value under torch.equal).

Forward reference: fp64 F.conv2d(padding=1) + bias, ReLU.  Input-gradient reference: fp64 F.conv_transpose2d(stride 1,
padding 1) times the mask [a > 0] of an integer ``a`` that contains zeros and negatives.  Every case runs on a dense
tensor and on a channel-offset view of a wider NaN-filled buffer with a NaN border (which must stay NaN).

Shapes: the fixed list, plus -- for H = 1, Cin = Cout = 64 -- the widths on either side of every M-tile boundary and the
Cout on either side of every N-tile boundary that stc_conv3_plan reports (probed, as
test_gpu_instance_norm.py::thresholds does)."""
import pytest
import torch
import torch.nn.functional as F

from conv_exact_ref import F64, BF16, acts, biases, expect_bf16, ints, require_exact, weights
from visual_ref import Boxed, nchw_to_nhwc

pytestmark = pytest.mark.gpu

FIXED = [(1, 1, 1, 8, 8), (2, 2, 2, 8, 64), (1, 3, 5, 16, 24), (3, 16, 16, 64, 64), (1, 8, 40, 128, 64),
         (2, 17, 33, 8, 128), (1, 24, 24, 192, 192), (1, 4, 4, 512, 512)]


def plan(B, H, W, cin, cout):
    from stcgan_amd import ops
    return ops.conv3_plan(B, H, W, cin, cout)


def thresholds():
    """(widths, couts) on either side of every tile boundary the plan reports for H = 1, Cin = Cout = 64."""
    ws, ns = [], []
    for w in range(1, 70):
        if plan(1, 1, w, 64, 64)[6] != plan(1, 1, w + 1, 64, 64)[6]:
            ws += [w, w + 1]
    for n in range(8, 200, 8):
        if plan(1, 1, 20, 64, n)[7] != plan(1, 1, 20, 64, n + 8)[7]:
            ns += [n, n + 8]
    return ws, ns


def all_cases():
    ws, ns = thresholds()
    return FIXED + [(1, 1, w, 64, 64) for w in ws] + [(1, 1, 20, 64, n) for n in ns]


CASES = all_cases()


def place(t_nhwc, layout):
    """Device bf16 tensor / view of an fp64 NHWC tensor: ("dense": contiguous, "boxed": NaN surroundings)."""
    from stcgan_amd import _lib as L
    B, H, W, C = t_nhwc.shape
    if layout == "dense":
        t = t_nhwc.to(device="cuda", dtype=BF16).contiguous()
        return t, L.nhwc_view(t), None
    bx = Boxed(B, H, W, C, value=t_nhwc)
    return bx.inner(), bx.view, bx


def out_buffer(B, H, W, C, layout):
    from stcgan_amd import _lib as L
    if layout == "dense":
        t = torch.full((B, H, W, C), float("nan"), dtype=BF16, device="cuda")
        return t, L.nhwc_view(t), None
    bx = Boxed(B, H, W, C)
    return bx.inner(), bx.view, bx


def run_fwd(case, layout, seed=0):
    from stcgan_amd import ops
    B, H, W, cin, cout = case
    x = acts((B, cin, H, W), 100 + seed)
    w = weights((cout, cin, 3, 3), 200 + seed)
    b = biases(cout, 300 + seed)
    require_exact(F.conv2d(x.abs(), w.abs(), b.abs(), 1, 1))
    ref = torch.relu(F.conv2d(x, w, b, 1, 1))
    (wf, _), = ops.pack_conv3([w.float().cuda()])
    _, xv, _ = place(nchw_to_nhwc(x), layout)
    y, yv, ybox = out_buffer(B, H, W, cout, layout)
    ops.conv3(xv, wf, yv, bias=b.float().cuda(), relu=True, B=B)
    torch.cuda.synchronize()
    return y, expect_bf16(nchw_to_nhwc(ref)), ybox


def run_dgrad(case, layout, seed=0):
    """(B, H, W, Cin, Cout) of the FORWARD layer: the GEMM reduces over Cout and produces Cin channels."""
    from stcgan_amd import ops
    B, H, W, cin, cout = case
    dy = acts((B, cout, H, W), 400 + seed)
    w = weights((cout, cin, 3, 3), 500 + seed)
    a = ints((B, cin, H, W), 600 + seed, 2, nonzero=False)
    assert bool((a == 0).any()) or a.numel() < 16
    require_exact(F.conv_transpose2d(dy.abs(), w.abs(), None, 1, 1))
    ref = F.conv_transpose2d(dy, w, None, 1, 1) * (a > 0)
    (_, wd), = ops.pack_conv3([w.float().cuda()])
    _, gv, _ = place(nchw_to_nhwc(dy), layout)
    _, av, _ = place(nchw_to_nhwc(a), layout)
    y, yv, ybox = out_buffer(B, H, W, cin, layout)
    ops.conv3(gv, wd, yv, bias=None, relu=False, mask=av, B=B)
    torch.cuda.synchronize()
    return y, expect_bf16(nchw_to_nhwc(ref)), ybox


@pytest.mark.parametrize("layout", ["dense", "boxed"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c)))
def test_forward_bit_exact(case, layout):
    y, want, box = run_fwd(case, layout)
    assert torch.equal(y.cpu(), want)
    assert box is None or box.surroundings_untouched()


@pytest.mark.parametrize("layout", ["dense", "boxed"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c)))
def test_input_gradient_bit_exact(case, layout):
    y, want, box = run_dgrad(case, layout)
    assert torch.equal(y.cpu(), want)
    assert box is None or box.surroundings_untouched()


def test_first_layer_gradient_without_mask():
    """The first layer's gradient: 8 output channels, no mask."""
    from stcgan_amd import ops
    B, H, W, cin, cout = 2, 9, 20, 8, 64
    dy = acts((B, cout, H, W), 41)
    w = weights((cout, cin, 3, 3), 42)
    ref = F.conv_transpose2d(dy, w, None, 1, 1)
    (_, wd), = ops.pack_conv3([w.float().cuda()])
    g = nchw_to_nhwc(dy).to(device="cuda", dtype=BF16)
    out = torch.full((B, H, W, cin), float("nan"), dtype=BF16, device="cuda")
    ops.conv3(g, wd, out, bias=None, relu=False)
    assert torch.equal(out.cpu(), expect_bf16(nchw_to_nhwc(ref)))


def test_pack_layouts_and_channel_padding():
    """fwd[n][t][c] = W[n][c][t], dgrad[m][t][k] = W[k][m][8 - t]; a 3-channel weight is padded to 8 with zeros."""
    from stcgan_amd import ops
    w = weights((16, 3, 3, 3), 77)
    (wf, wd), = ops.pack_conv3([w.float().cuda()])
    assert tuple(wf.shape) == (16, 9, 8) and tuple(wd.shape) == (8, 9, 16)
    wf, wd = wf.cpu().double(), wd.cpu().double()
    flat = w.reshape(16, 3, 9)
    assert torch.equal(wf[:, :, :3], flat.permute(0, 2, 1)) and not wf[:, :, 3:].any()
    assert torch.equal(wd[:3], flat.flip(2).permute(1, 2, 0)) and not wd[3:].any()


def test_cases_meet_every_path():
    """Every (path, K split) the plan can report over a wide sweep of shapes is met by CASES, and CASES has whole,
    partial and multiple tiles in M and in N."""
    can = set()
    for B in (1, 3, 64):
        for H, W in ((1, 1), (1, 17), (7, 5), (16, 16), (32, 32), (224, 224), (256, 256)):
            for cin in (8, 16, 64, 512):
                for cout in (8, 64, 72, 512):
                    p = plan(B, H, W, cin, cout)
                    can.add((p[0], p[5]))
    met = {(plan(*c)[0], plan(*c)[5]) for c in CASES}
    assert met == can
    TH, TW, BN = plan(1, 1, 1, 8, 8)[1:4]
    assert any(c[1] % TH and c[1] > TH for c in CASES) and any(c[2] % TW == 0 for c in CASES)
    assert any(c[2] % TW and c[2] > TW for c in CASES)
    assert any(c[4] > BN and c[4] % BN for c in CASES) and any(c[4] % BN == 0 for c in CASES)
    assert any(plan(*c)[6] > 1 for c in CASES) and any(plan(*c)[7] > 1 for c in CASES)
    assert any(c[3] % plan(*c)[4] for c in CASES)  # a Cin that is no multiple of the K chunk


def test_repeat_and_side_stream_bit_identical():
    case = (3, 16, 16, 64, 64)
    y1, want, _ = run_fwd(case, "dense")
    y2, _, _ = run_fwd(case, "dense")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        y3, _, _ = run_fwd(case, "dense")
        g3, gwant, _ = run_dgrad(case, "dense")
    torch.cuda.current_stream().wait_stream(side)
    g1, _, _ = run_dgrad(case, "dense")
    for a, b in ((y1, y2), (y1, y3), (g1, g3)):
        assert torch.equal(a.view(torch.int16), b.view(torch.int16))
    assert torch.equal(y1.cpu(), want) and torch.equal(g1.cpu(), gwant)
