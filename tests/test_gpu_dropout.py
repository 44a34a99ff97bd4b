"""use_dropout=True on the GPU: the mask export against the numpy restatement of the mask function, the dropout-aware
BatchNorm apply / backward kernels against the plain kernels fed torch-made masks (bit for bit), and the generator
against a functional torch U-Net with the same masks inserted after the three up-norms."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from fixture_init import fixture_state, normal, uniform
from oracle import stcgan_ref as ref
from test_dropout_cpu import dropout_mask as np_mask

pytestmark = pytest.mark.gpu
DEV = "cuda"
DT = {"fp32": torch.float32, "bf16": torch.bfloat16}
SEED, OFFSET = 0x1234ABCD5678, (1 << 32) + 7  # (both high words in use)


def _state(seed=SEED, offset=OFFSET):
    from stcgan_amd import ops
    return ops.dropout_state_tensor(seed, offset, DEV)


# ----------------------------------------------------------------------------- the mask
@pytest.mark.parametrize("p", [0.5, 0.2])
@pytest.mark.parametrize("shape,level", [((3, 4, 6, 64), 5), ((2, 16, 16, 512), 4)])
def test_mask_bit_exact(shape, level, p):
    from stcgan_amd import ops
    got = ops.dropout_mask(_state(), level, shape, p=p).cpu().numpy()
    want = np_mask(SEED, OFFSET, level, shape, p)
    assert got.dtype == np.uint8 and got.shape == tuple(shape)
    assert np.array_equal(got, want), f"{int((got != want).sum())} of {got.size} elements differ"


def test_dropout_next_copies_and_advances():
    from stcgan_amd import ops
    st = _state()
    a = ops.dropout_next(st)
    b = ops.dropout_next(st)
    assert a.tolist() == [SEED, OFFSET] and b.tolist() == [SEED, OFFSET + 1] and st.tolist() == [SEED, OFFSET + 2]


# ----------------------------------------------------------------------------- the kernels
B, C, FH, FW, H, W, LEVEL = 3, 64, 4, 6, 3, 5, 5  # a 4 x 6 ConvT extent cropped to 3 x 5


class _Case:
    """Raw ConvT output x (full extent), train-mode BatchNorm tables from its cropped extent, a gradient g."""

    def __init__(self, dt):
        from stcgan_amd import _lib as L
        from stcgan_amd import ops
        g = torch.Generator().manual_seed(21)
        self.dt = dt
        self.x = (torch.randn((B, FH, FW, C), generator=g) * 1.5 + 0.3).to(DEV, dt)
        self.g = torch.randn((B, FH, FW, 2 * C), generator=g).to(DEV, dt)  # (the BN channels: the second half)
        self.bn = torch.nn.BatchNorm2d(C).to(DEV)
        with torch.no_grad():
            self.bn.weight.copy_(torch.rand(C, generator=g) + 0.5)
            self.bn.bias.copy_(torch.randn(C, generator=g) * 0.3)
        self.xv = L.nhwc_view(self.x, 0, H, W)
        self.tab = torch.empty((2, C), dtype=torch.float32, device=DEV)
        self.mean, self.rstd = ops.bn_train_table(B, self.xv, C, dt, self.bn, self.tab[0], self.tab[1])
        self.state = _state()
        self.mask = ops.dropout_mask(self.state, LEVEL, (B, FH, FW, C))  # p = 0.5
        # (the reference of the tests below is built from this mask: it is the numpy restatement's, not only the GPU's)
        assert np.array_equal(self.mask.cpu().numpy(), np_mask(SEED, OFFSET, LEVEL, (B, FH, FW, C), 0.5))

    def drop(self, p):
        return (self.state, LEVEL, p, FH, FW)


def _apply(case, drop, dt):
    """bn_apply into y1 (ReLU, a channel-offset view of a concat buffer) and y2 (LeakyReLU)."""
    from stcgan_amd import _lib as L
    from stcgan_amd import ops
    cat = torch.zeros((B, H, W, 2 * C), dtype=dt, device=DEV)
    y2 = torch.zeros((B, H, W, C), dtype=dt, device=DEV)
    ops.bn_apply(B, case.xv, C, dt, (case.tab[0], case.tab[1]), L.nhwc_view(cat, C), 0.0, L.nhwc_view(y2), 0.2,
                 drop=drop)
    torch.cuda.synchronize()
    assert not cat[..., :C].any()  # nothing outside the view
    return cat[..., C:].clone(), y2


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_apply_kernel_bit_exact(dtype):
    dt = DT[dtype]
    case = _Case(dt)
    p1, p2 = _apply(case, None, dt)
    d1, d2 = _apply(case, case.drop(0.5), dt)
    m2 = (case.mask[:, :H, :W, :].to(dt) * 2)  # keep / (1 - p): an exact factor
    assert 0.3 < float(case.mask.float().mean()) < 0.7 and p1.any() and (p2 < 0).any()
    assert torch.equal(d1, p1 * m2) and torch.equal(d2, p2 * m2)
    z1, z2 = _apply(case, case.drop(0.0), dt)
    assert torch.equal(z1, p1) and torch.equal(z2, p2)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_backward_kernel_bit_exact(dtype):
    from stcgan_amd import _lib as L
    from stcgan_amd import ops
    dt = DT[dtype]
    case = _Case(dt)
    bn_state = (case.tab[0], case.tab[1], case.mean, case.rstd, case.bn.weight)

    def run(g, drop):
        dx = torch.zeros((B, FH, FW, C), dtype=dt, device=DEV)
        dg, db = ops.bn_backward(B, case.xv, C, dt, L.nhwc_view(dx, 0, H, W), g1=L.nhwc_view(g, C, H, W), s1=0.0,
                                 bn_state=bn_state, drop=drop)
        torch.cuda.synchronize()
        return dx, dg, db

    gm = case.g.clone()
    gm[..., C:] = case.g[..., C:] * (case.mask.to(dt) * 2)  # g * mask * 2 premultiplied (exact)
    want = run(gm, None)
    got = run(case.g, case.drop(0.5))
    assert want[0].any() and not torch.equal(want[0], run(case.g, None)[0])
    for a, b, name in zip(got, want, ("dx", "dgamma", "dbeta")):
        assert torch.equal(a, b), (name, float((a.float() - b.float()).abs().max()))
    for a, b in zip(run(case.g, case.drop(0.0)), run(case.g, None)):  # p = 0: the plain kernels' result
        assert torch.equal(a, b)


def test_bad_arguments_fail_loudly():
    from stcgan_amd import _lib as L
    from stcgan_amd import ops
    case = _Case(torch.float32)
    y = torch.zeros((B, H, W, C), device=DEV)
    with pytest.raises(RuntimeError, match="outside"):
        ops.bn_apply(B, case.xv, C, torch.float32, (case.tab[0], case.tab[1]), L.nhwc_view(y), 0.0,
                     drop=(case.state, LEVEL, 1.0, FH, FW))
    with pytest.raises(RuntimeError, match="dropout extent"):
        ops.bn_apply(B, case.xv, C, torch.float32, (case.tab[0], case.tab[1]), L.nhwc_view(y), 0.0,
                     drop=(case.state, LEVEL, 0.5, H - 1, W))


# ----------------------------------------------------------------------------- the generator
NGF, ND = 8, 8
# Input seed of the gradient comparison, chosen (among 1..12, on the torch U-Net below with these masks) so that no
# activation input at 32 x 32 and below sits within 1e-5 of zero: a ReLU decision there is fp32-rounding-sensitive and
# flips a whole gradient term, with or without dropout (the plain generator shows the same at other seeds; the
# golden vectors' inputs are picked the same way, tests/test_gpu_model.py).  The test asserts the margin;
# scripts/pick_dropout_test_seed.py (CPU only) prints the margin of every candidate and the choice.
X_SEED = 9


def _bn(st, prefix, x, train):
    out = F.batch_norm(x, st[prefix + "running_mean"], st[prefix + "running_var"], st[prefix + "weight"],
                       st[prefix + "bias"], train, 0.1, 1e-5)
    if train:
        st[prefix + "num_batches_tracked"] += 1
    return out


def _note(margins, level, t):
    """Record how close a deep level's activation inputs come to zero (exact zeros: dropped elements)."""
    if margins is not None and level >= 3:
        nz = t.detach()[t.detach() != 0].abs()
        margins.append((level, float(nz.min()) if nz.numel() else float("inf")))


def _block(st, x, level, train, masks, margins=None):
    """A non-outermost U-Net block (pad / crop at odd sizes), masks[level] (NCHW, keep/(1-p)) after its up-norm."""
    p = ref.gen_block_prefix(level)
    h, w = x.shape[2], x.shape[3]
    xin = F.pad(x, (0, w % 2, 0, h % 2))
    _note(margins, level, x)
    d = F.conv2d(F.leaky_relu(xin, 0.2), st[p + "1.weight"], None, 2, 1)
    if level == ND - 1:
        _note(margins, level, d)
        u = _bn(st, p + "4.", F.conv_transpose2d(F.relu(d), st[p + "3.weight"], None, 2, 1), train)
    else:
        c = _block(st, _bn(st, p + "2.", d, train), level + 1, train, masks, margins)
        u = _bn(st, p + "6.", F.conv_transpose2d(F.relu(c), st[p + "5.weight"], None, 2, 1), train)
    if level in masks:
        u = u * masks[level]  # over the full ConvT extent, before the crop
    _note(margins, level, u)
    return torch.cat([x, u[:, :, :h, :w]], 1)  # (the parent applies ReLU: ReLU(LeakyReLU(v)) = ReLU(v))


def unet(st, x, train, masks, margins=None):
    """margins (a list): collects (level, min nonzero |v|) over the inputs of every activation at 32 x 32 and below."""
    p = ref.gen_block_prefix(0)
    c = _block(st, F.conv2d(x, st[p + "0.weight"], None, 2, 1), 1, train, masks, margins)
    return torch.tanh(F.conv_transpose2d(F.relu(c), st[p + "3.weight"], st[p + "3.bias"], 2, 1))


def _params(st):
    return {k: v.clone().requires_grad_(v.is_floating_point() and not ref._is_buffer(k)) for k, v in st.items()}


def _masks(net, seed, offset, Bn, Hn, Wn, p=0.5):
    """{level: NCHW fp32 keep/(1-p)} of the call that starts at {seed, offset}, from the library's mask export."""
    from stcgan_amd import engine, ops
    S = engine._sizes(Hn, Wn, ND)
    out = {}
    for k in range(ND - 1 - (ND - 5), ND - 1):
        fh, fw = engine._pad2(S, k)
        m = ops.dropout_mask(ops.dropout_state_tensor(seed, offset, DEV), k, (Bn, fh, fw, NGF * 8), p=p)
        out[k] = m.permute(0, 3, 1, 2).float().cpu() / (1 - p)
    return out


def _net(dtype="fp32", seed=12, **kw):
    from stcgan_amd import networks
    net = networks.get_generator(4, 3, ngf=NGF, num_downs=ND, **kw)
    st = fixture_state(net.state_dict(), seed, "one")
    net.load_state_dict(st)
    net.to(DEV).set_compute_dtype(dtype)
    return net, st


def test_reference_unet_matches_oracle():
    """The test's own U-Net, with no masks, is the oracle's generator (train mode: output, buffers; eval)."""
    _, st = _net()
    x = uniform((2, 4, 256, 256), 5)
    for train in (True, False):
        a, b = _params(st), _params(st)
        with torch.no_grad():
            ya, yb = unet(a, x, train, {}), ref.generator_forward(b, x, train)
        assert float((ya - yb).abs().max()) <= 1e-6
        for k in a:
            if ref._is_buffer(k):
                assert torch.allclose(a[k].float(), b[k].float(), atol=1e-6, rtol=1e-6), k
    x = uniform((1, 4, 480, 640), 6)
    with torch.no_grad():
        assert float((unet(_params(st), x, True, {}) - ref.generator_forward(_params(st), x, True)).abs().max()) <= 1e-6


def test_model_parity_fp32():
    """Output, input gradient, parameter gradients and BatchNorm buffers of a train-mode forward / backward against the
    torch U-Net with the same masks (the tolerances of tests/test_gpu_model.py at this width without dropout)."""
    net, st = _net(use_dropout=True)
    net.set_dropout_seed(SEED, OFFSET).train()
    x = uniform((2, 4, 256, 256), X_SEED)
    xg = x.to(DEV).requires_grad_(True)
    out = net(xg)
    r = normal(tuple(out.shape), 212)
    (out * r.to(DEV)).sum().backward()
    torch.cuda.synchronize()
    assert net.dropout_state() == (SEED, OFFSET + 1)
    masks = _masks(net, SEED, OFFSET, 2, 256, 256)
    assert sorted(masks) == [4, 5, 6] and [tuple(masks[k].shape[2:]) for k in (4, 5, 6)] == [(16, 16), (8, 8), (4, 4)]
    ps = _params(st)
    xr = x.clone().requires_grad_(True)
    margins = []
    yr = unet(ps, xr, True, masks, margins)
    assert min(m for _, m in margins) >= 1e-5, sorted(margins, key=lambda t: t[1])[:3]  # (see X_SEED)
    (yr * r).sum().backward()
    err = float((out.detach().cpu() - yr.detach()).abs().max())
    # the masks matter: without them the reference is far away
    with torch.no_grad():
        far = float((unet(_params(st), x, True, {}) - yr).abs().max())
    print(f"output max-abs {err:.3e} (no masks: {far:.3e})")
    assert err <= 1e-4 and far > 100 * 1e-4
    gi = xr.grad
    e = (xg.grad.cpu() - gi).abs()
    print(f"input grad max-abs {float(e.max()):.3e}")
    assert bool((e <= 2e-5 + 2e-3 * gi.abs()).all())
    for k, p in net.named_parameters():
        g = ps[k].grad
        scale = float(g.abs().max())
        e = (p.grad.cpu() - g).abs()
        assert bool((e <= 2e-4 * scale + 1e-6 + 2e-3 * g.abs()).all()), (k, float(e.max()), scale)
    for k, b in net.named_buffers():
        e = (b.cpu().double() - ps[k].double()).abs()
        assert bool((e <= 1e-5 + 1e-4 * ps[k].double().abs()).all()), (k, float(e.max()))


def test_model_480x640_forward():
    """Odd intermediate sizes: level 5 drops over its padded 16 x 20 extent, cropped to 15 x 20 afterwards."""
    net, st = _net(use_dropout=True)
    net.set_dropout_seed(SEED, 3).train()
    x = uniform((1, 4, 480, 640), 6)
    with torch.no_grad():
        y = net(x.to(DEV)).cpu()
        masks = _masks(net, SEED, 3, 1, 480, 640)
        assert tuple(masks[5].shape[2:]) == (16, 20)
        yr = unet(_params(st), x, True, masks)
    err = float((y - yr).abs().max())
    print(f"480x640 output max-abs {err:.3e}")
    assert err <= 1e-4


def test_model_bf16_output():
    net, st = _net("bf16", use_dropout=True)
    net.set_dropout_seed(SEED, OFFSET).train()
    x = uniform((2, 4, 256, 256), 777)
    with torch.no_grad():
        y = net(x.to(DEV)).cpu()
        yr = unet(_params(st), x, True, _masks(net, SEED, OFFSET, 2, 256, 256))
    err = float((y - yr).abs().max())
    print(f"bf16 output max-abs {err:.3e}")
    assert err <= 2e-2


def _fwd_bwd(net, x, r):
    net.zero_grad(set_to_none=True)
    out = net(x)
    (out * r).sum().backward()
    torch.cuda.synchronize()
    return out.detach().clone(), [p.grad.clone() for p in net.parameters()]


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_p0_is_the_plain_net(dtype):
    """drop_rate = 0 keeps everything: outputs and parameter gradients of the plain generator, bit for bit.  The
    equality holds by path selection: GenPlan keeps a p = 0 level on the plain path (nothing to drop, nothing drawn),
    so this test does not reach the dropout kernels -- their p = 0 behaviour is what test_apply_kernel_bit_exact and
    test_backward_kernel_bit_exact check."""
    plain, _ = _net(dtype)
    zero, _ = _net(dtype, use_dropout=True, drop_rate=0.0)
    x = uniform((2, 4, 256, 256), 5).to(DEV)
    r = normal((2, 3, 256, 256), 212).to(DEV)
    plain.train()
    zero.train()
    ya, ga = _fwd_bwd(plain, x, r)
    yb, gb = _fwd_bwd(zero, x, r)
    assert torch.equal(ya, yb)
    for a, b in zip(ga, gb):
        assert torch.equal(a, b)


def test_determinism_and_counter():
    net, st = _net(use_dropout=True)
    plain, _ = _net()
    x = uniform((2, 4, 256, 256), 5).to(DEV)
    r = normal((2, 3, 256, 256), 212).to(DEV)
    net.train()
    net.set_dropout_seed(99, 5)
    y0, g0 = _fwd_bwd(net, x, r)
    assert net.dropout_state() == (99, 6)
    y1, _ = _fwd_bwd(net, x, r)  # the next offset: another mask
    assert net.dropout_state() == (99, 7) and not torch.equal(y0, y1)
    net.load_state_dict(st)  # (the BatchNorm buffers of the first call)
    net.set_dropout_seed(99, 5)
    y2, g2 = _fwd_bwd(net, x, r)
    assert torch.equal(y0, y2) and all(torch.equal(a, b) for a, b in zip(g0, g2))
    # train mode without a graph: the counter still advances
    with torch.no_grad():
        net(x)
    assert net.dropout_state() == (99, 7)
    # eval mode: the identity -- the plain net's output, and no state change
    net.load_state_dict(st)
    net.eval()
    plain.eval()
    with torch.no_grad():
        ye, yp = net(x), plain(x)
    assert torch.equal(ye, yp) and net.dropout_state() == (99, 7)
