"""UnetGenerator(activation=...) on the GPU: ngf 8, batch 2, 4 -> 3 channels, at 256 x 256 and at the odd 258 x 270.

Setup.  Built as test_gpu_upconv_model.build builds (no_conv_t=True, its SEEDS).  Nothing upstream of the head depends
on the head, so those seeds keep their sign margins (inorm_ref.sign_margin, asserted again).  The output layer's weight
is multiplied by 16 so that the heads saturate on a real share of the elements, and the running statistics are set to
one batch's (a momentum-1 train forward of the fp32 restatement) so that eval and frozen modes see the same scale; the
condition -- at least 5 % of the pre-activation q at or beyond +-1 and at least 5 % inside -- is asserted on the fp64
restatement in train and eval mode, and again on the q each comparison uses.

Default unchanged.  get_generator(...) and get_generator(..., activation="tanh") agree bit for bit: output, input
gradient, every parameter gradient, buffers; train and eval, fp32 and bf16.

Equivalence to the "none" net with the same weights, for sigmoid and htanh, fp32 and bf16, train / eval / frozen: the
output equals the head applied to q (htanh bit for bit, sigmoid within 1e-5 of the fp64 sigmoid), and a backward with
gy equals the "none" net's backward with gy * act'(y) formed by torch fp32 elementwise ops in the documented order
(head_ref.dq_torch) -- bit for bit in the input gradient, every parameter gradient (dbias included) and the running
statistics.  Once each with use_dropout=True (the same dropout seed) and with nn.InstanceNorm2d, at 256 x 256.

Parity.  "none" and "sigmoid" add no decision points: fp32 against the fp64 restatement whose head is replaced
(head_ref.HeadRefG), at the project's model tolerances (tests/test_gpu_model.py): output atol 1e-4; input gradient atol
2e-5, rtol 2e-3; parameter gradients atol 2e-4 * max|g| + 1e-6, rtol 2e-3."""
import functools

import pytest
import torch
import torch.nn as nn

import head_ref as R
import test_gpu_upconv_model as M
from fixture_init import normal, uniform
from inorm_ref import sign_margin

pytestmark = pytest.mark.gpu
DEV = "cuda"
OUT_W = "model.model.3.1.weight"
GAIN = 16.0
SHAPES = M.SHAPES


def shares(q):
    """(share of q at or beyond +-1, share strictly inside)."""
    out = float((q.detach().abs() >= 1).double().mean())
    return out, 1.0 - out


def require_saturation(q, what):
    out, inside = shares(q)
    assert out >= 0.05 and inside >= 0.05, f"{what}: {out:.3f} of q clamped, {inside:.3f} not"


@functools.lru_cache(maxsize=None)
def setup(shape, norm=None):
    """(state_dict with the scaled output weight and one batch's running statistics, x, r): once per shape, from the
    restatement alone."""
    kw = {} if norm is None else {"norm_layer": norm}
    net = M.build(M.SEEDS[(shape[2], shape[3])], **kw)
    sd = {k: v.clone() for k, v in net.state_dict().items()}
    sd[OUT_W] = sd[OUT_W] * GAIN
    x = uniform(shape, 44)
    r = normal((shape[0], 3, shape[2], shape[3]), 45)

    def fresh(act="none"):
        m = R.HeadRefG(4, 3, 8, 8, act=act, **kw)
        m.load_state_dict(sd)
        return m

    if norm is None:
        margin = sign_margin(fresh, x)
        assert margin >= M.MARGIN, f"seed of {shape}: an activation decision within fp32 rounding ({margin:.2f})"
        mover = fresh().train()
        for m in mover.modules():
            if isinstance(m, nn.BatchNorm2d):
                m.momentum = 1.0
        with torch.no_grad():
            mover(x)
        for k, v in mover.state_dict().items():
            if k.endswith(("running_mean", "running_var")):
                sd[k] = v.clone()
    ref = fresh().double()
    with torch.no_grad():
        require_saturation(ref.train().pre(x.double()), f"{shape} reference, train")
        if norm is None:
            ref.load_state_dict(sd)  # (the train forward moved its running statistics)
            require_saturation(ref.eval().pre(x.double()), f"{shape} reference, eval")
    return sd, x, r


def make(act, sd, dtype, **kw):
    from stcgan_amd import networks
    extra = {} if act is None else {"activation": act}
    net = networks.get_generator(4, 3, ngf=8, no_conv_t=True, **extra, **kw)
    net.load_state_dict(sd)
    return net.to(DEV).set_compute_dtype(dtype)


def run(net, x, gy_of, mode, seed=None):
    """One forward and a backward with the output gradient gy_of(output): (output, gy, input gradient)."""
    for p in net.parameters():
        p.grad = None
    net.train(mode != "eval")
    if mode == "frozen":
        net.freeze_norm()
    if seed is not None:
        net.set_dropout_seed(seed)
    xg = x.clone().requires_grad_(True)
    out = net(xg)
    gy = gy_of(out.detach())
    out.backward(gy)
    torch.cuda.synchronize()
    return out.detach(), gy, xg.grad


def compare_state(tag, a, b):
    pa, pb = dict(a.named_parameters()), dict(b.named_parameters())
    assert set(pa) == set(pb)
    for k in pa:
        assert pa[k].grad is not None and pb[k].grad is not None, k
        M.same(f"{tag} grad {k}", pa[k].grad, pb[k].grad)
    ba, bb = dict(a.named_buffers()), dict(b.named_buffers())
    assert set(ba) == set(bb)
    for k in ba:
        M.same(f"{tag} buffer {k}", ba[k], bb[k])


# ---------------------------------------------------------------- the default is what it was
@pytest.mark.parametrize("mode", ["train", "eval"])
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[2]}x{s[3]}")
def test_default_is_tanh(shape, dtype, mode):
    sd, x, r = setup(shape)
    a, b = make(None, sd, dtype), make("tanh", sd, dtype)
    assert a.activation == b.activation == "tanh" and a._make_plan().head == b._make_plan().head == "tanh"
    xg, rg = x.to(DEV), r.to(DEV)
    ya, _, ga = run(a, xg, lambda y: rg, mode)
    yb, _, gb = run(b, xg, lambda y: rg, mode)
    tag = f"{shape[2]}x{shape[3]} {dtype} {mode} default"
    M.same(f"{tag} output", ya, yb)
    M.same(f"{tag} input gradient", ga, gb)
    compare_state(tag, a, b)
    assert float(ya.abs().max()) <= 1.0 and not bool(torch.isnan(ya).any())


# ---------------------------------------------------------------- a head net is the "none" net plus the head
def check_equivalence(shape, dtype, mode, act, norm=None, **kw):
    sd, x, r = setup(shape, norm)
    if norm is not None:
        kw["norm_layer"] = norm
    h, n = make(act, sd, dtype, **kw), make("none", sd, dtype, **kw)
    assert h._make_plan().head == act and n._make_plan().head == "none" and len(n.model.model) == 4
    xg, rg = x.to(DEV), r.to(DEV)
    seed = 99 if kw.get("use_dropout") else None
    yh, _, gh = run(h, xg, lambda y: rg, mode, seed)
    # the "none" net: its output is q; its output gradient is gy * act'(y) in torch fp32 ops, from the head net's y
    q, gq, gn = run(n, xg, lambda q_: R.dq_torch(act, yh, rg), mode, seed)
    tag = f"{shape[2]}x{shape[3]} {dtype} {mode} {act} {sorted(kw)}"
    require_saturation(q, tag)
    if act == "htanh":
        M.same(f"{tag} output against clamp(q)", yh, q.clamp(-1.0, 1.0))
        zero = float((gq == 0).double().mean())
        assert zero >= 0.05, f"{tag}: {zero:.3f} of the gradient stopped by the clamp"
    else:
        err = float((yh.double() - R.head(act, q.double())).abs().max())
        print(f"[head_model] {tag} output against sigmoid(q): max err {err:.3e}")
        assert err <= 1e-5, f"{tag} output: {err:.3e}"
    M.same(f"{tag} input gradient", gh, gn)
    compare_state(tag, h, n)
    if mode == "train" and norm is None:
        assert any(float(v.abs().max()) > 0 for k, v in h.named_buffers() if k.endswith("running_mean"))


@pytest.mark.parametrize("act", ["sigmoid", "htanh"])
@pytest.mark.parametrize("mode", ["train", "eval", "frozen"])
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[2]}x{s[3]}")
def test_equivalence(shape, dtype, mode, act):
    check_equivalence(shape, dtype, mode, act)


@pytest.mark.parametrize("act", ["sigmoid", "htanh"])
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_equivalence_dropout(dtype, act):
    check_equivalence(SHAPES[0], dtype, "train", act, use_dropout=True)


@pytest.mark.parametrize("act", ["sigmoid", "htanh"])
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_equivalence_instance_norm(dtype, act):
    check_equivalence(SHAPES[0], dtype, "train", act, norm=nn.InstanceNorm2d)


# ---------------------------------------------------------------- parity with fp64 torch
@functools.lru_cache(maxsize=None)
def reference(shape, act):
    sd, x, r = setup(shape)
    ref = R.HeadRefG(4, 3, 8, 8, act=act)
    ref.load_state_dict(sd)
    ref = ref.double().train()
    x64 = x.double().requires_grad_(True)
    out = ref(x64)
    (out * r.double()).sum().backward()
    grads = {k: p.grad.clone() for k, p in ref.named_parameters()}
    ref.load_state_dict(sd)
    ref.eval()
    with torch.no_grad():
        out_eval = ref(x.double())
    return out.detach(), x64.grad.clone(), grads, out_eval


@pytest.mark.parametrize("act", ["none", "sigmoid"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[2]}x{s[3]}")
def test_parity_fp32(shape, act):
    sd, x, r = setup(shape)
    out_ref, gx_ref, grads, out_eval = reference(shape, act)
    net = make(act, sd, "fp32")
    rg = r.to(DEV)
    out, _, gx = run(net, x.to(DEV), lambda y: rg, "train")
    tag = f"G4 {act} {shape[0]}x{shape[2]}x{shape[3]}"
    fails = []
    M.close(f"{tag} train output", out, out_ref, 1e-4, 0.0, fails)
    M.close(f"{tag} input grad", gx, gx_ref, 2e-5, 2e-3, fails)
    params = dict(net.named_parameters())
    assert set(params) == set(grads)
    for k, g in grads.items():
        M.close(f"{tag} grad {k}", params[k].grad, g, 2e-4 * float(g.abs().max()) + 1e-6, 2e-3, fails)
    net.load_state_dict(sd)
    net.eval()
    with torch.no_grad():
        M.close(f"{tag} eval output", net(x.to(DEV)), out_eval, 1e-4, 0.0, fails)
    assert not fails, fails
