"""weight_decay (coupled and decoupled) and amsgrad inside the fused Adam + repack launch (stc_adam_pack_step_ex).

One step from a seeded state against an fp64 restatement, on the CPU, of torch's _single_tensor_adam on exactly the
uploaded values, with bounds from the fp32 roundings of the formulas (u = 2^-24; |g'| = |g| + wd |p| with coupled
decay, |g| otherwise):
    |dm| <= 8u (|m| + |g'|)        |dv| <= 8u (v + |g'|^2)
    |dp| <= u (4 |p| + 16 s (|m| + |g'|) / d),   s = lr / (1 - b1^t),  d the fp64 denominator
(4u|p|: the roundings of c, p * c and the final add; the rest: m', the quotient and the product.  torch.optim.Adam /
AdamW in fp32 on the CPU stay at <= 0.49 of the p bound and <= 0.27 of the state bounds over this grid.)  Then the
exact properties -- max_exp_avg_sq, the decoupled factor, the packed operands -- the agreement of the step paths bit
for bit, and torch's edge cases.  Each case prints its error / bound ratios."""
import numpy as np
import pytest
import torch

from stcgan_amd import _lib as L
from stcgan_amd import ops
from stcgan_amd.optim import Adam, AdamW

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
U = 2.0 ** -24
EPS = 1e-8

# (shape, packed modes, operand dtype): ragged 16x16 tiles with bf16 operands, fp32 operands, and flat tensors on
# either side of the 1024-element block
TENSORS = [
    ((17, 33, 4, 4), (L.PACK_CONV_FWD, L.PACK_CONV_S1_DGRAD), torch.bfloat16),
    ((24, 40, 4, 4), (L.PACK_CONVT_FWD, L.PACK_CONVT_DGRAD), torch.float32),
    ((1,), (), None),
    ((1023,), (), None),
    ((1025,), (), None),
]


def _seeded(shape, seed):
    """p ~ N(0,1), g ~ N(0,1), m ~ 0.3 N, v = (0.5 N)^2 + 1e-3, vmax = v U(0.5, 1.5) (fp32, CPU)."""
    g = torch.Generator().manual_seed(seed)
    p = torch.randn(shape, generator=g)
    gr = torch.randn(shape, generator=g)
    m = 0.3 * torch.randn(shape, generator=g)
    v = (0.5 * torch.randn(shape, generator=g)) ** 2 + 1e-3
    x = v * (0.5 + torch.rand(shape, generator=g))
    return p, gr, m, v, x


def _pads(shape, mode):
    P, Q = shape[:2]
    swapped = mode in (L.PACK_CONV_DGRAD, L.PACK_CONV_S1_DGRAD, L.PACK_CONVT_FWD)
    return ((Q if swapped else P) + 7) // 8 * 8, ((P if swapped else Q) + 7) // 8 * 8


def decay_factor(lr, lam):
    """c = (float)(1 - lr * lam), in double from the float lr the call receives."""
    return np.float32(1.0 - float(np.float32(lr)) * float(lam))


def reference(p, g, m, v, x, t, lr, betas, lam, dec, ams):
    """fp64 _single_tensor_adam of the uploaded values (lr, betas, eps as the floats the kernel receives) and the
    bounds.  Returns (p', m', v', x'), (bound p, bound m, bound v)."""
    p, g, m, v, x = (a.double() for a in (p, g, m, v, x))
    lr, b1, b2, eps = (float(np.float32(a)) for a in (lr, betas[0], betas[1], EPS))
    ga, p0 = g.abs(), p
    if lam != 0 and not dec:
        g = g + lam * p
        ga = ga + lam * p.abs()
    if lam != 0 and dec:
        p0 = p * float(decay_factor(lr, lam))
    m1 = m + (1.0 - b1) * (g - m)
    v1 = b2 * v + (1.0 - b2) * g * g
    x1 = torch.maximum(x, v1) if ams else x
    s = lr / (1.0 - b1 ** t)
    d = (x1 if ams else v1).sqrt() / np.sqrt(1.0 - b2 ** t) + eps
    p1 = p0 - s * m1 / d
    bounds = (U * (4 * p.abs() + 16 * s * (m.abs() + ga) / d), 8 * U * (m.abs() + ga), 8 * U * (v + ga * ga))
    return (p1, m1, v1, x1), bounds


class Case:
    """The tensors of TENSORS on the device with their forward operands packed, an optimiser over them and the
    seeded state written into it."""

    def __init__(self, t, lr, betas, lam, dec, ams, seed=0, cls=Adam, zero_gm=False):
        self.host, self.params, self.cache, self.packs = [], [], {}, []
        for i, (shape, modes, dt) in enumerate(TENSORS):
            p, g, m, v, x = _seeded(shape, 1000 * seed + i)
            if zero_gm:
                g, m = torch.zeros_like(g), torch.zeros_like(m)
            self.host.append((p, g, m, v, x))
            w = torch.nn.Parameter(p.to(DEV))
            w.grad = g.to(DEV)
            self.params.append(w)
            self.packs.append([(md, *_pads(shape, md), dt, ops.packed(self.cache, w, md, *_pads(shape, md), dt))
                               for md in modes])
        kw = dict(lr=lr, betas=betas, eps=EPS, weight_decay=lam, amsgrad=ams)
        self.opt = cls(self.params, **kw) if cls is AdamW else cls(self.params, decoupled_weight_decay=dec, **kw)
        for w, (p, g, m, v, x) in zip(self.params, self.host):
            self.opt.state[w] = dict(step=torch.tensor(float(t - 1)), exp_avg=m.to(DEV), exp_avg_sq=v.to(DEV),
                                     max_exp_avg_sq=x.to(DEV))

    def check_packs(self, tag=""):
        """Every packed operand == ops.pack of the updated weight, written in place by the step."""
        for w, packs in zip(self.params, self.packs):
            for (md, npad, cpad, dt, out) in packs:
                fresh = ops.packed(self.cache, w, md, npad, cpad, dt)  # no repack if the step wrote it
                assert fresh.data_ptr() == out.data_ptr(), (tag, md)
                want = ops.pack(md, w, npad, cpad, dt)
                it = torch.int16 if dt == torch.bfloat16 else torch.int32
                assert torch.equal(fresh.view(it), want.view(it)), (tag, md)


GRID = [(lam, dec, ams, t, lr, betas)
        for lam in (0.0, 1e-2, 0.3) for dec in (False, True) for ams in (False, True) for t in (1, 7)
        for (lr, betas) in ((5e-5, (0.5, 0.999)), (2e-3, (0.9, 0.99)))]


@pytest.mark.parametrize("lam,dec,ams,t,lr,betas", GRID)
def test_one_step_against_fp64(lam, dec, ams, t, lr, betas):
    c = Case(t, lr, betas, lam, dec, ams, seed=t)
    c.opt.step()
    torch.cuda.synchronize()
    worst = [0.0, 0.0, 0.0]
    for w, (p, g, m, v, x) in zip(c.params, c.host):
        (p1, m1, v1, x1), bounds = reference(p, g, m, v, x, t, lr, betas, lam, dec, ams)
        st = c.opt.state[w]
        assert float(st["step"]) == float(t)
        got = (w.detach().cpu(), st["exp_avg"].cpu(), st["exp_avg_sq"].cpu())
        for k, (a, r, b) in enumerate(zip(got, (p1, m1, v1), bounds)):
            worst[k] = max(worst[k], float(((a.double() - r).abs() / b).max()))
        # exact: max_exp_avg_sq = max(before, the exp_avg_sq the step wrote); untouched without amsgrad
        want_x = torch.maximum(x, got[2]) if ams else x
        assert torch.equal(st["max_exp_avg_sq"].cpu(), want_x)
    print(f"adam options lam={lam} dec={int(dec)} ams={int(ams)} t={t} lr={lr}: err/bound p {worst[0]:.3f} "
          f"m {worst[1]:.3f} v {worst[2]:.3f}")
    assert worst[0] <= 1.0 and worst[1] <= 1.0 and worst[2] <= 1.0, worst
    c.check_packs()


@pytest.mark.parametrize("ams", [False, True])
@pytest.mark.parametrize("lam", [1e-2, 0.3])
@pytest.mark.parametrize("lr", [5e-5, 2e-3])
def test_decoupled_factor_is_one_fp32_multiply(lam, lr, ams):
    """g = 0 and m = 0: the Adam term is exactly zero, and what is left is p * c, an fp32 product."""
    c = Case(3, lr, (0.5, 0.999), lam, True, ams, seed=9, zero_gm=True)
    c.opt.step()
    cf = torch.tensor(decay_factor(lr, lam))
    assert float(cf) < 1.0
    for w, (p, g, m, v, x) in zip(c.params, c.host):
        assert torch.equal(w.detach().cpu(), p * cf)
        assert not c.opt.state[w]["exp_avg"].any()
    c.check_packs()


# ---------------------------------------------------------------------------------------------- the step paths
STEPS, LR0, LR1 = 4, 2e-3, 7e-4


def _grad(shape, step, i):
    return torch.randn(shape, generator=torch.Generator().manual_seed(77 + 10 * step + i)).to(DEV)


def _run_path(path):
    c = Case(1, LR0, (0.5, 0.999), 1e-2, True, True, seed=5, cls=AdamW)
    opt = c.opt
    calls = {"full": 0}
    full = opt._full_step

    def counted(*a, **kw):
        calls["full"] += 1
        return full(*a, **kw)
    opt._full_step = counted
    for s in range(STEPS):
        for i, w in enumerate(c.params):
            w.grad.copy_(_grad(w.shape, s, i))  # in place: the steady-state table holds the gradients' addresses
        if path == "general" and s:
            opt._fast.clear()  # no steady-state record: the general path
        if path in ("device", "device_buckets") and s == 1:
            opt.device_step(True)
        if path in ("buckets", "device_buckets") and s >= 1:
            opt._bucket_ready([c.params[0], c.params[3]], None, None)
            opt._bucket_ready([c.params[1]], None, None)
            assert sorted(opt._ov_done[0]) == [0, 1, 3]
        opt.step()  # (after buckets: the rest of the group, and the join of the side stream)
        if s == 1:  # a scheduler step
            opt.param_groups[0]["lr"] = LR1
            opt.sync_lr()
    torch.cuda.synchronize()
    opt.sync_steps()
    assert calls["full"] == (STEPS if path == "general" else 1), (path, calls)
    out = []
    for w, packs in zip(c.params, c.packs):
        st = opt.state[w]
        assert float(st["step"]) == float(STEPS)
        out.append([w.detach().clone(), st["exp_avg"].clone(), st["exp_avg_sq"].clone(),
                    st["max_exp_avg_sq"].clone()] + [pk[4].clone() for pk in packs])
    if path.startswith("device"):  # the decay factor the device formed from the pushed lr
        coef = opt._dev[0]["coef"].cpu()
        assert coef.numel() == 4 and float(coef[2]) == float(decay_factor(LR1, 1e-2))
    c.check_packs(path)  # (at the end only: ops.pack makes new operand buffers, which ends the steady state)
    return out, c


def test_step_paths_agree_bit_for_bit():
    """AdamW + amsgrad, 4 steps, an lr change after step 2: the general path every step, the steady-state path, the
    device-resident step (lr pushed by sync_lr), per-bucket updates over two subsets (+ the rest in step()), and
    the buckets with the device-resident step -- parameters, the three moments and the packed operands."""
    base, c = _run_path("general")
    # (not vacuous: the general path itself against the fp64 reference run step by step on the CPU)
    for i, (w0, (p, g, m, v, x)) in enumerate(zip(base, c.host)):
        for s in range(STEPS):
            lr = LR0 if s < 2 else LR1
            (p, m, v, x), _ = reference(p, _grad(p.shape, s, i).cpu(), m, v, x, s + 1, lr, (0.5, 0.999), 1e-2, True,
                                        True)
        assert float((w0[0].cpu().double() - p).abs().max()) < 1e-5
        assert float((w0[3].cpu().double() - x).abs().max()) < 1e-5
    for path in ("steady", "device", "buckets", "device_buckets"):
        got, _ = _run_path(path)
        for i, (a, b) in enumerate(zip(base, got)):
            for k, (ta, tb) in enumerate(zip(a, b)):
                it = torch.int16 if ta.dtype == torch.bfloat16 else torch.int32
                assert torch.equal(ta.view(it), tb.view(it)), (path, i, k)


# ---------------------------------------------------------------------------------------------- torch's edge cases
def test_parameter_without_gradient_is_skipped():
    c = Case(2, 2e-3, (0.9, 0.99), 0.3, True, True, seed=3)
    c.params[1].grad = None
    c.params[3].grad = None
    for _ in range(2):  # (the second step: the steady-state path)
        c.opt.step()
    for i in (1, 3):
        p, g, m, v, x = c.host[i]
        st = c.opt.state[c.params[i]]
        assert torch.equal(c.params[i].detach().cpu(), p)  # no decay either, as torch
        assert torch.equal(st["exp_avg"].cpu(), m) and torch.equal(st["max_exp_avg_sq"].cpu(), x)
        assert float(st["step"]) == 1.0
    assert not torch.equal(c.params[0].detach().cpu(), c.host[0][0])
    assert float(c.opt.state[c.params[0]]["step"]) == 3.0


def test_two_groups_with_different_options():
    """Options are per group (each group is its own launch): coupled decay without amsgrad beside AdamW-style decay
    with amsgrad, and a default group, in one optimiser."""
    shapes = [((17, 33, 4, 4), 0), ((1025,), 1), ((24, 40, 4, 4), 2), ((1023,), 3), ((5,), 4)]
    host = [_seeded(sh, 500 + i) for sh, i in shapes]
    params = [torch.nn.Parameter(h[0].to(DEV)) for h in host]
    for w, h in zip(params, host):
        w.grad = h[1].to(DEV)
    conf = [dict(weight_decay=0.3), dict(weight_decay=1e-2, decoupled_weight_decay=True, amsgrad=True, lr=2e-3), {}]
    opt = Adam([dict(params=params[0:2], **conf[0]), dict(params=params[2:4], **conf[1]),
                dict(params=params[4:], **conf[2])], lr=5e-5, betas=(0.5, 0.999), eps=EPS)
    t = 4
    for w, (p, g, m, v, x) in zip(params, host):
        opt.state[w] = dict(step=torch.tensor(float(t - 1)), exp_avg=m.to(DEV), exp_avg_sq=v.to(DEV))
    opt.step()
    for gi, group in enumerate(opt.param_groups):
        for w in group["params"]:
            p, g, m, v, x = host[[id(q) for q in params].index(id(w))]
            ams = group["amsgrad"]
            (p1, m1, v1, x1), (bp, bm, bv) = reference(p, g, m, v, torch.zeros_like(v), t, group["lr"], (0.5, 0.999),
                                                       group["weight_decay"], group["decoupled_weight_decay"], ams)
            st = opt.state[w]
            assert ("max_exp_avg_sq" in st) == ams  # created (as zeros) where a group asks for it
            assert bool(((w.detach().cpu().double() - p1).abs() <= bp).all()), gi
            assert bool(((st["exp_avg"].cpu().double() - m1).abs() <= bm).all()), gi
            assert bool(((st["exp_avg_sq"].cpu().double() - v1).abs() <= bv).all()), gi
            if ams:
                assert torch.equal(st["max_exp_avg_sq"], st["exp_avg_sq"])


def test_amsgrad_switched_on_later():
    """The flags are read at every step: amsgrad set on a group that has already stepped leaves the steady-state
    path for one step and starts max_exp_avg_sq from zeros."""
    c = Case(1, 5e-5, (0.5, 0.999), 0.0, False, False, seed=6)
    for w in c.params:
        del c.opt.state[w]["max_exp_avg_sq"]
    c.opt.step()
    c.opt.step()
    c.opt.param_groups[0]["amsgrad"] = True
    c.opt.step()
    for w in c.params:
        st = c.opt.state[w]
        assert torch.equal(st["max_exp_avg_sq"], st["exp_avg_sq"])
    c.check_packs()
