"""args.optimizer / args.weight_decay / args.amsgrad through the trainer (the configuration of
test_gpu_dropout_trainer.py: ngf 8, bf16): a checkpoint resume and a captured graph's replays are the uninterrupted
eager steps bit for bit -- parameters, moments and max_exp_avg_sq -- and the defaults leave the optimisers as before."""
import types

import pytest
import torch

pytestmark = pytest.mark.gpu

NETS = ("G1", "G2", "D1", "D2")
MOMENTS = ("exp_avg", "exp_avg_sq", "max_exp_avg_sq")


def _args(**kw):
    return types.SimpleNamespace(devices=["cuda:0"], tasks=["train"], lr_G=5e-5, lr_D=2e-5, beta1=0.5, beta2=0.999,
                                 D_loss_fn="standard", D_loss_type="normal", ngf=8, dtype="bf16",
                                 load_weights_g1=None, load_weights_g2=None, load_weights_d1=None,
                                 load_weights_d2=None, use_dropout=True, dropout_seed=4242, **kw)


def _trainer(**kw):
    from stcgan_amd.stcgan import STCGAN
    torch.manual_seed(7)
    return STCGAN(_args(optimizer="adamw", weight_decay=0.01, amsgrad=True, **kw))


def _state(tr):
    torch.cuda.synchronize()
    st = {n: {k: v.detach().clone() for k, v in getattr(tr, n).state_dict().items()} for n in NETS}
    for oname in ("optim_G", "optim_D"):
        o = getattr(tr, oname)
        o.sync_steps()
        st[oname] = [(float(o.state[p]["step"]),) + tuple(o.state[p][k].clone() for k in MOMENTS)
                     for g in o.param_groups for p in g["params"]]
    return st


def _same(a, b):
    bad = []
    for n in NETS:
        for k in a[n]:
            if not torch.equal(a[n][k], b[n][k]):
                bad.append((n, k))
    for oname in ("optim_G", "optim_D"):
        assert len(a[oname]) == len(b[oname]) > 0
        for i, (x, y) in enumerate(zip(a[oname], b[oname])):
            if x[0] != y[0] or any(not torch.equal(s, t) for s, t in zip(x[1:], y[1:])):
                bad.append((oname, i))
    return bad


def _batch(seed=3, B=2):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    x = torch.rand((B, 3, 256, 256), generator=g, device="cuda") * 2 - 1
    m = (torch.rand((B, 1, 256, 256), generator=g, device="cuda") < 0.5).float() * 2 - 1
    y = torch.rand((B, 3, 256, 256), generator=g, device="cuda") * 2 - 1
    return x, m, y


def test_trainer_builds_the_optimisers():
    from stcgan_amd.optim import AdamW
    tr = _trainer()
    for o in (tr.optim_G, tr.optim_D):
        assert isinstance(o, AdamW)
        g, = o.param_groups
        assert g["weight_decay"] == 0.01 and g["amsgrad"] is True and g["decoupled_weight_decay"] is True


def test_options_change_the_step():
    """(the comparisons below are not vacuous: the options reach the update)"""
    from stcgan_amd.stcgan import STCGAN
    x, m, y = _batch()
    a = _trainer()
    torch.manual_seed(7)
    b = STCGAN(_args())
    a.train_step(x, m, y)
    b.train_step(x, m, y)
    pa, pb = next(a.G1.parameters()), next(b.G1.parameters())
    assert not torch.equal(pa, pb)
    assert "max_exp_avg_sq" in a.optim_G.state[pa] and "max_exp_avg_sq" not in b.optim_G.state[pb]


def test_checkpoint_resume(tmp_path):
    x, m, y = _batch()
    tr = _trainer()
    for _ in range(3):
        tr.train_step(x, m, y)
    path = str(tmp_path / "ck.tar")
    tr.save_checkpoint(1, path)
    for _ in range(2):
        tr.train_step(x, m, y)
    fresh = _trainer()
    fresh.load_checkpoint(path)
    for _ in range(2):
        fresh.train_step(x, m, y)
    a, b = _state(tr), _state(fresh)
    assert a["optim_G"][0][0] == 5.0
    bad = _same(a, b)
    assert not bad, bad[:8]


def test_captured_step_replays_the_eager_steps():
    x, m, y = _batch()
    eager, graphed = _trainer(), _trainer()
    replay = graphed.capture(x, m, y, warmup=1)  # 3 eager steps inside
    for _ in range(3):
        eager.train_step(x, m, y)
    assert not _same(_state(eager), _state(graphed))
    for i in range(2):
        eager.train_step(x, m, y)
        replay()
        bad = _same(_state(eager), _state(graphed))
        assert not bad, (i, bad[:8])
    # a scheduler step: replay() pushes the new lr (sync_lr), and the decay factor 1 - lr * weight_decay follows it
    # inside the graph
    for tr in (eager, graphed):
        for o in (tr.optim_G, tr.optim_D):
            o.param_groups[0]["lr"] *= 0.8
    eager.train_step(x, m, y)
    replay()
    bad = _same(_state(eager), _state(graphed))
    assert not bad, bad[:8]
    assert float(graphed.optim_G.state[next(graphed.G1.parameters())]["step"]) == 6.0


def test_defaults_are_adam_without_options():
    from stcgan_amd.optim import Adam, AdamW
    from stcgan_amd.stcgan import STCGAN
    torch.manual_seed(7)
    tr = STCGAN(_args())
    for o in (tr.optim_G, tr.optim_D):
        assert isinstance(o, Adam) and not isinstance(o, AdamW)
        g, = o.param_groups
        assert g["weight_decay"] == 0 and g["amsgrad"] is False and g["decoupled_weight_decay"] is False
        assert Adam._options(g) == (None, False)  # the calls without options
    for bad in (dict(optimizer="sgd"), dict(weight_decay=-0.1), dict(amsgrad="yes")):
        with pytest.raises(ValueError):
            STCGAN(_args(**bad))
