"""norm="instance" through the trainer (ngf 8, batch 2, 256x256, fp32): the first step's losses against an fp64
torch.nn restatement, stream schedules and a checkpoint resume bit for bit, and no discriminator call made for
running statistics that do not exist."""
import types

import pytest
import torch

from inorm_ref import RefD, RefG
from oracle import stcgan_ref as ref

pytestmark = pytest.mark.gpu

NETS = ("G1", "G2", "D1", "D2")


def _trainer(norm="instance", **kw):
    from stcgan_amd.stcgan import STCGAN
    torch.manual_seed(7)
    a = types.SimpleNamespace(devices=["cuda:0"], tasks=["train"], lr_G=5e-5, lr_D=2e-5, beta1=0.5, beta2=0.999,
                              D_loss_fn="standard", D_loss_type="normal", ngf=8, dtype="fp32",
                              load_weights_g1=None, load_weights_g2=None, load_weights_d1=None,
                              load_weights_d2=None, norm=norm, **kw)
    return STCGAN(a)


def _state(tr):
    torch.cuda.synchronize()
    st = {n: {k: v.detach().clone() for k, v in getattr(tr, n).state_dict().items()} for n in NETS}
    for oname in ("optim_G", "optim_D"):
        o = getattr(tr, oname)
        o.sync_steps()
        st[oname] = [(float(o.state[p]["step"]), o.state[p]["exp_avg"].clone(), o.state[p]["exp_avg_sq"].clone())
                     for g in o.param_groups for p in g["params"]]
    return st


def _same(a, b):
    bad = []
    for n in NETS:
        for k in a[n]:
            if not torch.equal(a[n][k], b[n][k]):
                bad.append((n, k))
    for oname in ("optim_G", "optim_D"):
        for i, (x, y) in enumerate(zip(a[oname], b[oname])):
            if x[0] != y[0] or not torch.equal(x[1], y[1]) or not torch.equal(x[2], y[2]):
                bad.append((oname, i))
    return bad


def _batch(seed=3, B=2):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    x = torch.rand((B, 3, 256, 256), generator=g, device="cuda") * 2 - 1
    m = (torch.rand((B, 1, 256, 256), generator=g, device="cuda") < 0.5).float() * 2 - 1
    y = torch.rand((B, 3, 256, 256), generator=g, device="cuda") * 2 - 1
    return x, m, y


def test_trainer_builds_instance_norm_networks():
    tr = _trainer()
    for n in NETS:
        net = getattr(tr, n)
        assert net.norm_kind == "instance" and not list(net.buffers())
        assert len(net.state_dict()) == (17 if n.startswith("G") else 7)
    assert _trainer("batch").D1.norm_kind == "batch"
    with pytest.raises(ValueError, match="norm"):
        _trainer("group")


def test_first_step_losses_against_fp64():
    """The eight losses of the first train_step (D update between the two phases, as the reference's run_epoch)
    within 2e-5 + 2e-4 * |want| of the fp64 restatement.  Measured on an MI355X: worst error / bound 0.001."""
    tr = _trainer()
    x, m, y = _batch()
    nl = torch.nn.InstanceNorm2d
    R = dict(G1=RefG(3, 1, 8, 8, nl), G2=RefG(4, 3, 8, 8, nl), D1=RefD(4, 8, 3, nl), D2=RefD(7, 8, 3, nl))
    for n, r in R.items():
        r.double().load_state_dict({k: v.cpu() for k, v in getattr(tr, n).state_dict().items()})
        r.train()
    got = {k: float(v) for k, v in tr.train_step(x, m, y).items()}
    x, m, y = x.cpu().double(), m.cpu().double(), y.cpu().double()
    opt_d = torch.optim.Adam(list(R["D1"].parameters()) + list(R["D2"].parameters()), lr=2e-5, betas=(0.5, 0.999))
    cat = torch.cat
    m_pred = R["G1"](x)
    y_pred = R["G2"](cat((x, m_pred), 1))
    c1r, c1f = R["D1"](cat((x, m), 1)), R["D1"](cat((x, m_pred.detach()), 1))
    c2r, c2f = R["D2"](cat((x, m, y), 1)), R["D2"](cat((x, m_pred.detach(), y_pred.detach()), 1))
    adv = ref.adversarial_loss
    d1 = (adv(c1f, False) + adv(c1r, True)) * 0.5
    d2 = (adv(c2f, False) + adv(c2r, True)) * 0.5
    d = 0.1 * d1 + 0.1 * d2
    d.backward()
    opt_d.step()
    g1 = adv(R["D1"](cat((x, m_pred), 1)), True)
    g2 = adv(R["D2"](cat((x, m_pred, y_pred), 1)), True)
    data1, data2 = ref.data_loss(m_pred, m), ref.data_loss(y_pred, y)
    want = dict(D1=d1, D2=d2, D=d, G1=g1, G2=g2, data1=data1, data2=data2, G=data1 + 5 * data2 + 0.1 * g1 + 0.1 * g2)
    assert sorted(got) == sorted(want)
    bad = []
    for k, w in want.items():
        w = float(w)
        print(f"[instance_norm_trainer] {k}: got {got[k]:.8f} want {w:.8f} "
              f"error/bound {abs(got[k] - w) / (2e-5 + 2e-4 * abs(w)):.3f}")
        if not abs(got[k] - w) <= 2e-5 + 2e-4 * abs(w):
            bad.append((k, got[k], w))
    assert not bad, bad


def test_stream_schedules_bit_identical():
    x, m, y = _batch()
    res = []
    for streams in (True, False):
        tr = _trainer(streams=streams)
        for _ in range(3):
            tr.train_step(x, m, y)
        res.append(_state(tr))
    bad = _same(*res)
    assert not bad, bad[:8]


def test_checkpoint_resume(tmp_path):
    x, m, y = _batch()
    tr = _trainer()
    tr.train_step(x, m, y)
    tr.train_step(x, m, y)
    path = str(tmp_path / "ck.tar")
    tr.save_checkpoint(2, path)
    tr.train_step(x, m, y)
    fresh = _trainer()
    fresh.load_checkpoint(path)
    fresh.train_step(x, m, y)
    bad = _same(_state(tr), _state(fresh))
    assert not bad, bad[:8]


def test_no_discriminator_call_for_absent_running_statistics(monkeypatch):
    """Loss type "normal": the G step's real-input discriminator calls exist only to advance BatchNorm running
    statistics.  norm="batch" issues them (8 discriminator forwards per step), norm="instance" does not (6)."""
    from stcgan_amd import engine
    orig = engine.NetFn
    calls = []

    class Counting:
        @staticmethod
        def apply(ctrl, *tensors):
            calls.append((ctrl[1], bool(ctrl[8])))
            return orig.apply(ctrl, *tensors)

    x, m, y = _batch()
    counts = {}
    for norm in ("instance", "batch"):
        tr = _trainer(norm)
        tr.train_step(x, m, y)  # (plans and packs made)
        monkeypatch.setattr(engine, "NetFn", Counting)
        calls.clear()
        tr.train_step(x, m, y)
        torch.cuda.synchronize()
        monkeypatch.setattr(engine, "NetFn", orig)
        counts[norm] = (sum(k == "G" for k, _ in calls), sum(k == "D" for k, _ in calls),
                        sum(k == "D" and so for k, so in calls))
    assert counts["instance"] == (2, 6, 0), counts
    assert counts["batch"] == (2, 8, 2), counts
