"""The perceptual terms in the trainer (args.lambda4 / args.lambda5 / args.visual_loss): STCGAN at ngf 8, batch 2,
256 x 256, bf16 and fp32 trainer dtype, with the 1/4-width VGG of tests/visual_ref.py (always bf16)."""
import types

import pytest
import torch

from visual_ref import quarter_vgg

pytestmark = pytest.mark.gpu

NETS = ("G1", "G2", "D1", "D2")


def _visual():
    from stcgan_amd.loss import VisualLoss
    return VisualLoss(quarter_vgg())


def _trainer(dtype, lambda4=0.0, lambda5=0.0, **kw):
    from stcgan_amd.stcgan import STCGAN
    vl = _visual() if lambda4 > 0 or lambda5 > 0 else None  # (before the seed: building the VGG draws random numbers)
    torch.manual_seed(7)
    a = types.SimpleNamespace(devices=["cuda:0"], tasks=["train"], lr_G=5e-5, lr_D=2e-5, beta1=0.5, beta2=0.999,
                              D_loss_fn="standard", D_loss_type="normal", ngf=8, dtype=dtype,
                              load_weights_g1=None, load_weights_g2=None, load_weights_d1=None,
                              load_weights_d2=None, lambda4=lambda4, lambda5=lambda5, **kw)
    if vl is not None:
        a.visual_loss = vl
    return STCGAN(a)


def _batch(seed, B=2):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    x = torch.rand((B, 3, 256, 256), generator=g, device="cuda") * 2 - 1
    m = (torch.rand((B, 1, 256, 256), generator=g, device="cuda") < 0.5).float() * 2 - 1
    y = torch.rand((B, 3, 256, 256), generator=g, device="cuda") * 2 - 1
    return x, m, y


def _state(tr, nets=NETS, optims=("optim_G", "optim_D")):
    torch.cuda.synchronize()
    st = {n: {k: v.detach().clone() for k, v in getattr(tr, n).state_dict().items()} for n in nets}
    for oname in optims:
        o = getattr(tr, oname)
        o.sync_steps()
        st[oname] = [(float(o.state[p]["step"]), o.state[p]["exp_avg"].clone(), o.state[p]["exp_avg_sq"].clone())
                     for g in o.param_groups for p in g["params"]]
    return st


def _same(a, b):
    bad = []
    for n in a:
        if n.startswith("optim"):
            for i, (x, y) in enumerate(zip(a[n], b[n])):
                if x[0] != y[0] or not torch.equal(x[1], y[1]) or not torch.equal(x[2], y[2]):
                    bad.append((n, i))
        else:
            bad += [(n, k) for k in a[n] if not torch.equal(a[n][k], b[n][k])]
    return bad


def _hand_step(tw, x, m, y, vl, lambda4, lambda5):
    """One train step from the public pieces on a trainer built with lambda = 0: the D step (d_objective), then the G
    step with g_objective + lambda4 * vis1 + lambda5 * vis2 formed by torch scalar ops, .backward(), optim_G.step().
    (The statistics-only real-input discriminator calls of the G step are left out: they touch the discriminators'
    running statistics only.)"""
    from stcgan_amd.loss import d_objective, g_objective
    tw.optim_D.zero_grad()
    tw.optim_G.zero_grad()
    tw.D1.requires_grad_(True)
    tw.D2.requires_grad_(True)
    tw._exchange(("D1", "D2"), 2)
    C1_real = tw.D1([x, m])
    C2_real = tw.D2([x, m, y])
    m_pred = tw.G1(x)
    C1_fake = tw.D1([x, m_pred.detach()])
    y_pred = tw.G2([x, m_pred])
    C2_fake = tw.D2([x, m_pred.detach(), y_pred.detach()])
    D_loss = d_objective(tw.adv_loss, C1_fake, C1_real, C2_fake, C2_real, tw.lambda2, tw.lambda3)[0]
    D_loss.backward()
    tw._finish_exchange(("D2", "D1"))
    tw.optim_D.step()
    tw.optim_G.zero_grad()
    tw.D1.requires_grad_(False)
    tw.D2.requires_grad_(False)
    C1_fake = tw.D1([x, m_pred])
    C2_fake = tw.D2([x, m_pred, y_pred])
    G_loss = g_objective(tw.adv_loss, m_pred, m, y_pred, y, C1_fake, C2_fake, tw.lambda1, tw.lambda2, tw.lambda3)[0]
    if lambda4 > 0:
        G_loss = G_loss + lambda4 * vl(m_pred.expand(-1, 3, -1, -1), m.expand(-1, 3, -1, -1))
    if lambda5 > 0:
        G_loss = G_loss + lambda5 * vl(y_pred, y)
    tw._exchange(("G1", "G2"), 1)
    G_loss.backward()
    tw._finish_exchange(("G2", "G1"))
    tw.optim_G.step()


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_step_with_visual_terms(dtype):
    x, m, y = _batch(3)
    l4, l5 = 0.25, 0.5
    plain = _trainer(dtype)
    assert plain.visual_loss is None and plain.lambda4 == 0.0 and plain.lambda5 == 0.0
    v0 = plain.train_step(x, m, y)
    assert not any(k.startswith("vis") for k in v0)
    tr = _trainer(dtype, l4, l5)
    v = tr.train_step(x, m, y)
    assert set(v) == set(v0) | {"vis1", "vis2"}
    assert all(t.dtype == torch.float32 and t.dim() == 0 for t in v.values())
    # G = ((the existing objective) + lambda4 * vis1) + lambda5 * vis2, fp32 torch scalar ops in this order
    base = v["data1"] + tr.lambda1 * v["data2"] + tr.lambda2 * v["G1"] + tr.lambda3 * v["G2"]
    want = base + l4 * v["vis1"] + l5 * v["vis2"]
    assert torch.equal(v["G"].view(torch.int32), want.view(torch.int32))
    assert float(v["vis1"]) > 0 and float(v["vis2"]) > 0
    # the terms before the G update do not depend on the lambdas
    for k in ("D", "D1", "D2", "G1", "G2", "data1", "data2"):
        assert torch.equal(v[k], v0[k]), k
    # the D step is untouched
    assert not _same(_state(tr, ("D1", "D2"), ("optim_D",)), _state(plain, ("D1", "D2"), ("optim_D",)))
    # G1 / G2 and their Adam moments equal a hand-built step from the public pieces on a twin
    twin = _trainer(dtype)
    _hand_step(twin, x, m, y, tr.visual_loss, l4, l5)
    bad = _same(_state(tr, ("G1", "G2"), ("optim_G",)), _state(twin, ("G1", "G2"), ("optim_G",)))
    assert not bad, bad[:8]
    # ... and differ from the step without the terms
    assert _same(_state(tr, ("G1", "G2"), ("optim_G",)), _state(plain, ("G1", "G2"), ("optim_G",)))


def test_validation_epoch_reports_enabled_terms():
    tr = _trainer("bf16", 0.0, 0.5)
    tr.valid_loader = [("a",) + _batch(5), ("b",) + _batch(6)]
    before = _state(tr, ("G1", "G2"), ())
    out = tr.run_epoch(training=False)["Loss"]
    assert "vis2" in out and "vis1" not in out and out["vis2"] > 0
    assert out["total"] == pytest.approx(out["G"] * 0.8 + out["D"] * 0.2, rel=1e-12)
    both = _trainer("bf16", 0.25, 0.5)
    both.valid_loader = tr.valid_loader
    out2 = both.run_epoch(training=False)["Loss"]
    assert out2["vis1"] > 0 and out2["vis2"] == out["vis2"]
    after = _state(tr, ("G1", "G2"), ())
    assert not [k for n in ("G1", "G2") for k in before[n] if not torch.equal(before[n][k], after[n][k])]


def test_captured_step_with_visual_term_is_bit_identical():
    """On the pattern of tests/test_gpu_graph.py::test_captured_step_is_bit_identical, with lambda5 > 0."""
    x, m, y = _batch(9)
    eager = _trainer("bf16", 0.0, 0.5)
    graphed = _trainer("bf16", 0.0, 0.5)
    replay = graphed.capture(x, m, y, warmup=1)  # 3 eager steps inside
    for _ in range(3):
        eager.train_step(x, m, y)
    assert not _same(_state(eager), _state(graphed))
    for i in range(3):
        eager.train_step(x, m, y)
        replay()
        bad = _same(_state(eager), _state(graphed))
        assert not bad, (i, bad[:8])
