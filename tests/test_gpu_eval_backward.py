"""Backward through eval-mode networks and through train-mode networks with frozen BatchNorm statistics, against the
CPU oracle (oracle.stcgan_ref with train=False under torch.autograd) at ngf / ndf 8, batch size 2, fixture_state
weights (non-trivial running statistics).

Tolerances are those of tests/test_gpu_model.py for the train-mode goldens: output 1e-4 max-abs; input gradient atol
2e-5, rtol 2e-3; parameter gradients atol 2e-4 * max|g| + 1e-6, rtol 2e-3.  No element is excluded.

Input seeds.  A ReLU / LeakyReLU decision within fp32 rounding of zero flips a whole gradient term in any fp32
implementation, so the inputs are chosen on the CPU (the method of tests/golden/make_goldens.py pick_input_seed): the
first seed of base, base + 1000, ... at which no activation input of the reference lies within 1e-5 of zero.  Every
activation input is looked at, at every level, in the restated networks below (asserted equal to the oracle); the
margin of each chosen seed is asserted again by the test that uses it.
"""
import functools

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from fixture_init import fixture_state, normal, uniform
from oracle import stcgan_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
NGF, BS = 8, 2
MARGIN = 1e-5
SEED, OFFSET = 0x1234ABCD5678, (1 << 32) + 7


# ----------------------------------------------------------------------------- restated networks (CPU, torch)
def _bn(st, prefix, x, batch_stats):
    out = F.batch_norm(x, st[prefix + "running_mean"], st[prefix + "running_var"], st[prefix + "weight"],
                       st[prefix + "bias"], batch_stats, 0.1, 1e-5)
    if batch_stats:
        st[prefix + "num_batches_tracked"] += 1
    return out


def _see(acts, t):
    if acts is not None:
        acts.append(t.detach())


def _block(st, x, level, nd, batch_stats, masks, acts):
    """A non-outermost U-Net block (pad / crop at odd sizes); masks[level] (NCHW, keep / (1 - p)) after its up-norm,
    over the full ConvT extent.  acts collects every activation input: x (LeakyReLU into the conv, ReLU into the
    skip), the innermost conv output, the (masked) up-norm output."""
    p = ref.gen_block_prefix(level)
    h, w = x.shape[2], x.shape[3]
    _see(acts, x)
    d = F.conv2d(F.leaky_relu(F.pad(x, (0, w % 2, 0, h % 2)), 0.2), st[p + "1.weight"], None, 2, 1)
    if level == nd - 1:
        _see(acts, d)
        u = _bn(st, p + "4.", F.conv_transpose2d(F.relu(d), st[p + "3.weight"], None, 2, 1), batch_stats)
    else:
        c = _block(st, _bn(st, p + "2.", d, batch_stats), level + 1, nd, batch_stats, masks, acts)
        u = _bn(st, p + "6.", F.conv_transpose2d(F.relu(c), st[p + "5.weight"], None, 2, 1), batch_stats)
    if level in masks:
        u = u * masks[level]
    u = u[:, :, :h, :w]
    _see(acts, u)
    return torch.cat([x, u], 1)  # (the parent applies ReLU: ReLU(LeakyReLU(v)) = ReLU(v))


def unet(st, x, nd, batch_stats, masks=None, acts=None):
    """The U-Net generator with separate switches: batch_stats (BatchNorm on batch or running statistics) and masks
    ({level: factor}; the dropout of a train-mode call, none in eval mode)."""
    p = ref.gen_block_prefix(0)
    c = _block(st, F.conv2d(x, st[p + "0.weight"], None, 2, 1), 1, nd, batch_stats, masks or {}, acts)
    return torch.tanh(F.conv_transpose2d(F.relu(c), st[p + "3.weight"], st[p + "3.bias"], 2, 1))


def patchgan(st, x, batch_stats, acts=None):
    h = F.conv2d(x, st["model.0.weight"], st["model.0.bias"], 2, 1)
    _see(acts, h)
    h = F.leaky_relu(h, 0.2)
    idx = 2
    for n in range(1, 4):
        h = _bn(st, f"model.{idx + 1}.", F.conv2d(h, st[f"model.{idx}.weight"], None, 2 if n < 3 else 1, 1),
                batch_stats)
        _see(acts, h)
        h = F.leaky_relu(h, 0.2)
        idx += 3
    return F.conv2d(h, st[f"model.{idx}.weight"], st[f"model.{idx}.bias"], 1, 1)


def margin_of(acts):
    """Smallest |v| over every activation input (exact zeros, the elements a dropout mask removed, aside)."""
    out = float("inf")
    for t in acts:
        nz = t[t != 0].abs()
        if nz.numel():
            out = min(out, float(nz.min()))
    return out


def _params(st):
    return {k: v.clone().requires_grad_(v.is_floating_point() and not ref._is_buffer(k)) for k, v in st.items()}


# ----------------------------------------------------------------------------- cases
# name: (kind, in channels, out channels, num_downs, H, W, fixture seed, input seed)
CASES = {
    "G-3to1-64": ("G", 3, 1, 6, 64, 64, 11, None),
    "G-4to3-64": ("G", 4, 3, 6, 64, 64, 12, None),
    "G-4to3-60x44": ("G", 4, 3, 6, 60, 44, 12, None),  # an odd inner level, 15 x 11
    "G-4to3-256-full": ("G", 4, 3, 8, 256, 256, 12, None),
    "D-4-64": ("D", 4, 1, 0, 64, 64, 13, None),
    "D-7-64": ("D", 7, 1, 0, 64, 64, 14, None),
}
# input seeds: the first of base, base + 1000, ... with margin >= 1e-5 (pick_seed below; base = 100 + fixture seed).
# The full-depth 256 x 256 case has a million activation inputs, about 70 of them within 1e-5 of zero at every seed
# (and none of 400 seeds clears 1e-5 even over the tensors of <= 65536 elements that pick_input_seed looks at): its
# seed is chosen by the other method the golden tests use, tests/inorm_ref.py sign_margin -- every activation input
# of the fp64 restatement at least 8 of its own fp32 errors away from zero (sign_margin below; the first seed has 14).
X_SEED = {"G-3to1-64": 111111, "G-4to3-64": 366112, "G-4to3-60x44": 9112, "G-4to3-256-full": 112, "D-4-64": 113,
          "D-7-64": 3114}
SIGN_MARGIN = 8.0
X_SEED_DROP = 92112  # G-4to3-64 with use_dropout and the level-4 mask of {SEED, OFFSET}, p = 0.5


def make_net(case, dtype="fp32", **kw):
    from stcgan_amd import networks
    kind, cin, cout, nd, _, _, wseed, _ = CASES[case]
    net = (networks.get_generator(cin, cout, ngf=NGF, num_downs=nd, **kw) if kind == "G" else
           networks.get_discriminator(cin, ndf=NGF, **kw))
    st = fixture_state(net.state_dict(), wseed, "one")
    net.load_state_dict(st)
    return net, st


def ref_forward(case, st, x, batch_stats=False, masks=None, acts=None):
    kind, _, _, nd = CASES[case][:4]
    return unet(st, x, nd, batch_stats, masks, acts) if kind == "G" else patchgan(st, x, batch_stats, acts)


def oracle_forward(case, st, x):
    kind, _, _, nd = CASES[case][:4]
    return ref.generator_forward(st, x, False, num_downs=nd) if kind == "G" else ref.discriminator_forward(st, x, False)


def case_input(case, seed):
    _, cin, _, _, H, W = CASES[case][:6]
    return uniform((BS, cin, H, W), seed)


def pick_seed(case, st, masks_of=None, tries=200):
    """(seed, margin): the first seed of base, base + 1000, ... whose every activation input keeps |v| >= MARGIN."""
    base = 100 + CASES[case][6]
    for t in range(tries):
        seed = base + 1000 * t
        acts = []
        with torch.no_grad():
            ref_forward(case, _params(st), case_input(case, seed), False, masks_of, acts)
        m = margin_of(acts)
        if m >= MARGIN:
            return seed, m
    raise RuntimeError(f"{case}: no input seed with margin >= {MARGIN}")


def sign_margin(case, st, x):
    """The smallest |n| / e over every activation input n of the fp64 restatement, e the larger of that element's
    |fp32 - fp64| difference and the rms of that difference over its tensor (tests/inorm_ref.py sign_margin)."""
    rec = {}
    for dt in (torch.float64, torch.float32):
        acts = []
        sd = {k: (v.to(dt) if v.is_floating_point() else v.clone()) for k, v in st.items()}
        with torch.no_grad():
            ref_forward(case, sd, x.to(dt), False, None, acts)
        rec[dt] = [a.double() for a in acts]
    margin = float("inf")
    for a, b in zip(rec[torch.float64], rec[torch.float32]):
        d = (a - b).abs()
        e = torch.maximum(d, d.pow(2).mean().sqrt().expand_as(d)).clamp_min(1e-30)
        margin = min(margin, float((a.abs() / e).min()))
    return margin


def assert_margin(case, st, x, masks=None):
    if case == "G-4to3-256-full":
        m = sign_margin(case, st, x)
        assert m >= SIGN_MARGIN, f"{case}: an activation decision within fp32 rounding (sign margin {m:.2f})"
        return
    acts = []
    with torch.no_grad():
        ref_forward(case, _params(st), x, False, masks, acts)
    m = margin_of(acts)
    assert m >= MARGIN, f"{case}: an activation input within {m:.3e} of zero"


def check_grads(tag, net, xg, ps, xr):
    gi = xr.grad
    e = (xg.grad.cpu() - gi).abs()
    print(f"[eval_backward] {tag}: input grad error/bound {float((e / (2e-5 + 2e-3 * gi.abs())).max()):.4f}")
    assert bool((e <= 2e-5 + 2e-3 * gi.abs()).all()), (tag, float(e.max()))
    worst = 0.0
    for k, p in net.named_parameters():
        g = ps[k].grad
        assert p.grad is not None and g is not None, k
        scale = float(g.abs().max())
        e = (p.grad.cpu() - g).abs()
        bound = 2e-4 * scale + 1e-6 + 2e-3 * g.abs()
        worst = max(worst, float((e / bound).max()))
        assert bool((e <= bound).all()), (tag, k, float(e.max()), scale)
    print(f"[eval_backward] {tag}: parameter grad error/bound {worst:.4f}")


def buffers_of(net):
    return {k: b.detach().clone() for k, b in net.named_buffers()}


def assert_buffers_unchanged(net, before):
    for k, b in net.named_buffers():
        assert torch.equal(b, before[k]), k


def fwd_bwd(net, x, r):
    net.zero_grad(set_to_none=True)
    xg = x.detach().clone().requires_grad_(True)
    out = net(xg)
    (out * r).sum().backward()
    torch.cuda.synchronize()
    return out.detach(), xg, [None if p.grad is None else p.grad.clone() for p in net.parameters()]


@pytest.mark.parametrize("case", list(CASES))
def test_eval_backward_vs_oracle(case):
    """net.eval(); out = net(x); (out * r).sum().backward() against the oracle in eval mode under autograd: output,
    input gradient, every parameter gradient; buffers and num_batches_tracked untouched; a second call bit-identical;
    with the parameters not requiring gradients the same input gradient bit for bit and no parameter gradient."""
    net, st = make_net(case)
    net.to(DEV).eval()
    x = case_input(case, X_SEED[case])
    assert_margin(case, st, x)
    ps = _params(st)
    xr = x.clone().requires_grad_(True)
    with torch.no_grad():  # the restatement whose activation inputs the margin is taken from is the oracle
        assert float((ref_forward(case, _params(st), x) - oracle_forward(case, _params(st), x)).abs().max()) <= 1e-6
    yr = oracle_forward(case, ps, xr)
    r = normal(tuple(yr.shape), 212)
    (yr * r).sum().backward()
    before = buffers_of(net)
    out, xg, grads = fwd_bwd(net, x.to(DEV), r.to(DEV))
    err = float((out.cpu() - yr.detach()).abs().max())
    print(f"[eval_backward] {case}: output max-abs {err:.3e}")
    assert err <= 1e-4
    check_grads(case, net, xg, ps, xr)
    assert_buffers_unchanged(net, before)
    for k in st:  # (the oracle's copy too: eval mode moves nothing)
        if ref._is_buffer(k):
            assert torch.equal(ps[k], st[k]), k
    out2, xg2, grads2 = fwd_bwd(net, x.to(DEV), r.to(DEV))
    assert torch.equal(out2, out) and torch.equal(xg2.grad, xg.grad)
    assert all(torch.equal(a, b) for a, b in zip(grads, grads2))
    # gradients through a fixed network: no parameter gradient wanted
    net.requires_grad_(False)
    out3, xg3, grads3 = fwd_bwd(net, x.to(DEV), r.to(DEV))
    assert torch.equal(out3, out) and torch.equal(xg3.grad, xg.grad)
    assert all(g is None for g in grads3) and all(p.grad is None for p in net.parameters())
    assert_buffers_unchanged(net, before)


def test_frozen_norm_with_dropout():
    """A use_dropout generator in .train() after freeze_norm(): BatchNorm on running statistics, dropout active.
    Against the restated U-Net with batch_stats=False and the masks of the call (ops.dropout_mask): output and
    gradients; the offset advances by one per forward, the buffers stay; .eval() afterwards gives the plain eval
    output."""
    from stcgan_amd import engine, ops
    case, nd, level = "G-4to3-64", 6, 4
    net, st = make_net(case, use_dropout=True)
    net.to(DEV).train()
    net.freeze_norm()
    net.set_dropout_seed(SEED, OFFSET)
    assert [k for k, m in net.named_modules() if isinstance(m, nn.Dropout) and m.training]
    fh, fw = engine._pad2(engine._sizes(64, 64, nd), level)
    keep = ops.dropout_mask(ops.dropout_state_tensor(SEED, OFFSET, DEV), level, (BS, fh, fw, NGF * 8), p=0.5)
    masks = {level: keep.permute(0, 3, 1, 2).float().cpu() / 0.5}
    assert 0.2 < float(keep.float().mean()) < 0.8
    x = case_input(case, X_SEED_DROP)
    assert_margin(case, st, x, masks)
    ps = _params(st)
    xr = x.clone().requires_grad_(True)
    yr = unet(ps, xr, nd, False, masks)
    r = normal(tuple(yr.shape), 212)
    (yr * r).sum().backward()
    before = buffers_of(net)
    out, xg, _ = fwd_bwd(net, x.to(DEV), r.to(DEV))
    assert net.dropout_state() == (SEED, OFFSET + 1)
    err = float((out.cpu() - yr.detach()).abs().max())
    with torch.no_grad():
        far = float((unet(_params(st), x, nd, False) - yr).abs().max())       # without the masks
        far_bs = float((unet(_params(st), x, nd, True, masks) - yr).abs().max())  # with batch statistics
    print(f"[eval_backward] frozen+dropout: output max-abs {err:.3e} (no masks {far:.3e}, batch statistics {far_bs:.3e})")
    # (one 4 x 4 dropout level deep inside moves the output by little; the gradients below tell the masks apart)
    assert err <= 1e-4 and far > 2 * 1e-4 and far_bs > 100 * 1e-4
    check_grads("frozen+dropout", net, xg, ps, xr)
    p0 = _params(st)
    (unet(p0, x, nd, False) * r).sum().backward()
    key = ref.gen_block_prefix(level - 1) + "5.weight"  # the ConvT that reads the masked level
    gap = float((p0[key].grad - ps[key].grad).abs().max())
    assert gap > 100 * (2e-4 * float(ps[key].grad.abs().max()) + 1e-6), gap  # the masks matter
    assert_buffers_unchanged(net, before)
    with torch.no_grad():
        net(x.to(DEV))
    assert net.dropout_state() == (SEED, OFFSET + 2)
    # the same call state again: the same bits
    net.set_dropout_seed(SEED, OFFSET)
    out2, xg2, _ = fwd_bwd(net, x.to(DEV), r.to(DEV))
    assert torch.equal(out2, out) and torch.equal(xg2.grad, xg.grad)
    # eval mode: the plain generator's eval output, and no state change
    plain, _ = make_net(case)
    plain.to(DEV).eval()
    net.eval()
    with torch.no_grad():
        assert torch.equal(net(x.to(DEV)), plain(x.to(DEV)))
    assert net.dropout_state() == (SEED, OFFSET + 1)
    assert_buffers_unchanged(net, before)


@pytest.mark.parametrize("case", ["G-4to3-64", "G-4to3-60x44", "D-7-64"])
def test_instance_norm_eval_backward_is_the_train_backward(case):
    """Instance norm computes the same thing in train and eval mode: so does its backward, bit for bit."""
    net, _ = make_net(case, norm_layer=functools.partial(nn.InstanceNorm2d, affine=True))
    g = torch.Generator().manual_seed(5)
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, nn.InstanceNorm2d):
                m.weight.copy_(torch.rand(m.weight.shape, generator=g) + 0.5)
                m.bias.copy_(torch.randn(m.bias.shape, generator=g) * 0.2)
    net.to(DEV)
    x = case_input(case, 5).to(DEV)
    with torch.no_grad():
        shape = tuple(net.eval()(x).shape)
    r = normal(shape, 212).to(DEV)
    a = fwd_bwd(net.train(), x, r)
    b = fwd_bwd(net.eval(), x, r)
    c = fwd_bwd(net.train().freeze_norm(), x, r)
    for other in (b, c):
        assert torch.equal(a[0], other[0]) and torch.equal(a[1].grad, other[1].grad)
        assert all(torch.equal(p, q) for p, q in zip(a[2], other[2]))


def test_mixed_norm_modes_raise():
    for case in ("G-4to3-64", "D-4-64"):
        net, _ = make_net(case)
        net.to(DEV).train()
        bns = [m for m in net.modules() if isinstance(m, nn.BatchNorm2d)]
        bns[-1].eval()
        before = buffers_of(net)
        with pytest.raises(NotImplementedError, match="mixed modes"):
            net(case_input(case, 5).to(DEV))
        torch.cuda.synchronize()
        assert_buffers_unchanged(net, before)
        net.freeze_norm()  # all of them: accepted
        with torch.no_grad():
            net(case_input(case, 5).to(DEV))
        assert_buffers_unchanged(net, before)


def _record_ops(fn):
    """The names of the stcgan_amd.ops functions the engine calls during fn(), in call order."""
    from stcgan_amd import ops
    names, saved = [], {}
    for k, v in list(vars(ops).items()):
        if callable(v) and getattr(v, "__module__", None) == ops.__name__ and not k.startswith("_"):
            saved[k] = v
            setattr(ops, k, (lambda k, v: lambda *a, **kw: (names.append(k), v(*a, **kw))[1])(k, v))
    try:
        fn()
        torch.cuda.synchronize()
    finally:
        for k, v in saved.items():
            setattr(ops, k, v)
    return names


@pytest.mark.parametrize("case", ["G-4to3-64", "D-7-64"])
def test_train_mode_call_sequence_is_untouched(case):
    """A plain .train() forward + backward reaches none of the frozen-statistics calls, and the sequence of library
    wrappers it goes through is the one recorded on the commit before this feature (_train_sequence, taken there
    with this same recorder); an eval-mode call with a backward differs from it only by the frozen forms."""
    net, _ = make_net(case)
    net.to(DEV)
    x = case_input(case, 5).to(DEV)
    r = normal(tuple(net.eval()(x).shape), 212).to(DEV)
    fwd_bwd(net.train(), x, r)  # (plans and packs made)
    names = _record_ops(lambda: fwd_bwd(net.train(), x, r))
    frozen_only = {"bn_backward_frozen", "bn_running_rstd", "bn_eval_table"}
    assert not frozen_only & set(names)
    assert names == _train_sequence(case), names
    ev = _record_ops(lambda: fwd_bwd(net.eval(), x, r))
    n_bn = sum(isinstance(m, nn.BatchNorm2d) for m in net.modules())
    assert ev.count("bn_backward_frozen") == n_bn == ev.count("bn_running_rstd") == ev.count("bn_eval_table")
    assert "conv_bn_act" not in ev and "conv_bn_backward" not in ev


def _train_sequence(case):
    """Recorded with _record_ops on the commit before this feature (one train-mode forward + backward, fp32, after
    a first call has made plans and packs): tests/golden/train_call_sequence.json."""
    import json
    import os
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "train_call_sequence.json")) as f:
        return json.load(f)[case]


# ----------------------------------------------------------------------------- bf16, layer by layer
def _f(t, c=None):
    """NHWC (bf16 / fp32) -> NCHW fp32 (first c channels)."""
    x = t.float().permute(0, 3, 1, 2)
    return (x if c is None else x[:, :c]).contiguous()


def _q(t):
    return t.to(torch.bfloat16).float()


class _Checker:
    """The two bounds of tests/test_gpu_c3_layers.py: a bf16 tensor within 1e-2 relative L2 and 0.02 of its largest
    magnitude in the worst element; an fp32 parameter gradient within 1e-2 relative L2."""

    def __init__(self):
        self.fails, self.worst = [], {}

    @staticmethod
    def rel(a, b):
        a, b = a.double().reshape(-1), b.double().reshape(-1)
        return float((a - b).norm() / (b.norm() + 1e-30))

    def fp32(self, what, got, want, tol=1e-2):
        e = self.rel(got, want)
        self.worst[what] = e
        if not e <= tol:
            self.fails.append((what, e))

    def bf16(self, what, got, want):
        e = self.rel(got, want)
        m = float((got.float() - want.float()).abs().max() / (want.float().abs().max() + 1e-30))
        self.worst[what] = e
        if not (e <= 1e-2 and m <= 0.02):
            self.fails.append((what, e, m))


def _frozen_ref(raw, sc, sh, mean, rstd, dn_of):
    """dx, dgamma, dbeta of one frozen layer from its own saved inputs (NCHW fp32 on the device)."""
    bc = lambda t: t[None, :, None, None]  # noqa: E731
    dn = dn_of((raw.double() * bc(sc).double() + bc(sh).double()).float())  # (one rounding, as the kernels' fma)
    return bc(sc) * dn, (dn * (raw - bc(mean)) * bc(rstd)).sum(dim=(0, 2, 3)), dn.sum(dim=(0, 2, 3))


def _check_tables(C, what, bn, tab, st):
    rstd = torch.rsqrt(bn.running_var.double() + bn.eps)
    gam, bet = bn.weight.detach().double(), bn.bias.detach().double()
    assert st[0] is bn.running_mean
    C.fp32(f"{what} rstd_run", st[1], rstd, 1e-6)
    C.fp32(f"{what} scale", tab[0], gam * rstd, 1e-6)
    C.fp32(f"{what} shift", tab[1], bet - bn.running_mean.double() * gam * rstd, 1e-6)


@pytest.mark.parametrize("case,mode", [("G-4to3-64", "eval"), ("G-4to3-60x44", "frozen"), ("G-4to3-256-full", "eval")])
def test_bf16_frozen_generator_layers(case, mode):
    """bf16: every frozen BatchNorm layer's dx and dgamma / dbeta against torch on that layer's own saved inputs
    (engine.TRACE), so no error amplification enters the bounds."""
    from stcgan_amd import engine
    net, _ = make_net(case)
    net.to(DEV).set_compute_dtype("bf16")
    net.eval() if mode == "eval" else net.train().freeze_norm()
    x = case_input(case, 5).to(DEV)
    engine.TRACE = {}
    try:
        y = net(x)
        y.backward((normal(tuple(y.shape), 212) * 1e-3).to(DEV))
        torch.cuda.synchronize()
        tr = engine.TRACE["G"][0]
    finally:
        engine.TRACE = None
    sv, plan = tr["saved"], net._plan
    assert sv["frozen"]
    S, rd, rq = sv["S"], sv["rd"], sv["rq"]
    Lv, co = plan.L, plan.co
    C = _Checker()
    for k in range(Lv - 1):  # BN_up[k + 1]: the gradient is the second half of gcat[k], over the padded extent
        bn = plan.bnu[k + 1]
        _check_tables(C, f"bn_u{k + 1}", bn, sv["tab_u"][k + 1], sv["st_u"][k + 1])
        g = _f(tr[("gcat", k)])[:, co[k]:]
        dx, dgam, dbet = _frozen_ref(_f(rq[k + 1]), *sv["tab_u"][k + 1], *sv["st_u"][k + 1], lambda n: g * (n > 0))
        C.bf16(f"bn_u{k + 1} input grad", _f(tr[("dq", k + 1)]), _q(dx))
        C.fp32(f"bn_u{k + 1} gamma grad", bn.weight.grad, dgam)
        C.fp32(f"bn_u{k + 1} beta grad", bn.bias.grad, dbet)
    for k in range(Lv - 1, 1, -1):  # BN_down[k - 1]: the skip half (ReLU) + conv_k's input gradient (LeakyReLU)
        bn = plan.bnd[k - 1]
        _check_tables(C, f"bn_d{k - 1}", bn, sv["tab_d"][k - 1], sv["st_d"][k - 1])
        h, w = S[k]
        g1 = _f(tr[("gcat", k - 1)])[:, :co[k - 1], :h, :w]
        ga = _f(tr[("ga", k)])[:, :, :h, :w]
        dx, dgam, dbet = _frozen_ref(_f(rd[k - 1]), *sv["tab_d"][k - 1], *sv["st_d"][k - 1],
                                     lambda n: g1 * (n > 0) + ga * torch.where(n > 0, 1.0, 0.2))
        C.bf16(f"bn_d{k - 1} input grad", _f(tr[("dr", k - 1)]), _q(dx))
        C.fp32(f"bn_d{k - 1} gamma grad", bn.weight.grad, dgam)
        C.fp32(f"bn_d{k - 1} beta grad", bn.bias.grad, dbet)
    print(f"[eval_backward] bf16 {case} {mode}: {len(C.worst)} layer checks; worst",
          sorted(C.worst.items(), key=lambda kv: -kv[1])[:4])
    assert len(C.worst) == 6 * (len(plan.bnu) + len(plan.bnd)) and not C.fails, C.fails[:10]


@pytest.mark.parametrize("mode", ["eval", "frozen"])
def test_bf16_frozen_discriminator_layers(mode):
    from stcgan_amd import engine
    net, _ = make_net("D-7-64")
    net.to(DEV).set_compute_dtype("bf16")
    net.eval() if mode == "eval" else net.train().freeze_norm()
    x = case_input("D-7-64", 5).to(DEV).requires_grad_(True)
    engine.TRACE = {}
    try:
        y = net(x)
        y.backward((normal(tuple(y.shape), 212) * 1e-3).to(DEV))
        torch.cuda.synchronize()
        tr = engine.TRACE["D"][0]
    finally:
        engine.TRACE = None
    sv, plan = tr["saved"], net._plan
    assert sv["frozen"]
    C = _Checker()
    for i in range(plan.n - 1, 0, -1):  # conv_i's input gradient ga, through LeakyReLU and the BN of layer i - 1
        if sv["tabs"][i] is None:
            continue
        bn = plan.bns[i - 2]
        _check_tables(C, f"bn{i - 1}", bn, sv["tabs"][i], sv["stats"][i])
        ga = _f(tr[("ga", i)])
        dx, dgam, dbet = _frozen_ref(_f(sv["raw"][i]), *sv["tabs"][i], *sv["stats"][i],
                                     lambda n: ga * torch.where(n > 0, 1.0, 0.2))
        C.bf16(f"bn{i - 1} input grad", _f(tr[("g", i - 1)]), _q(dx))
        C.fp32(f"bn{i - 1} gamma grad", bn.weight.grad, dgam)
        C.fp32(f"bn{i - 1} beta grad", bn.bias.grad, dbet)
    print(f"[eval_backward] bf16 D {mode}: {len(C.worst)} layer checks; worst",
          sorted(C.worst.items(), key=lambda kv: -kv[1])[:4])
    assert len(C.worst) == 6 * len(plan.bns) and not C.fails, C.fails[:10]
