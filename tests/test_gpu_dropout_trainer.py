"""use_dropout=True through the trainer: the masks depend on logical indices and a device-resident counter only, so
every stream schedule, a captured graph's replays and a checkpoint resume draw the eager steps' masks -- parameters,
BatchNorm buffers and Adam moments bit for bit."""
import types

import pytest
import torch

pytestmark = pytest.mark.gpu

NETS = ("G1", "G2", "D1", "D2")


def _trainer(dtype="bf16", **kw):
    from stcgan_amd.stcgan import STCGAN
    torch.manual_seed(7)
    a = types.SimpleNamespace(devices=["cuda:0"], tasks=["train"], lr_G=5e-5, lr_D=2e-5, beta1=0.5, beta2=0.999,
                              D_loss_fn="standard", D_loss_type="normal", ngf=8, dtype=dtype,
                              load_weights_g1=None, load_weights_g2=None, load_weights_d1=None,
                              load_weights_d2=None, use_dropout=True, dropout_seed=4242, **kw)
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


def test_trainer_builds_dropout_generators():
    tr = _trainer(droprate=0.2)
    assert tr.G1._make_plan().drop == {4: 0.2, 5: 0.2, 6: 0.2} and tr.G2._make_plan().drop == tr.G1._make_plan().drop
    # one mask stream per generator
    assert tr.G1.dropout_state() == (4242, 0) and tr.G2.dropout_state() == (4243, 0)


def test_droprate_is_ignored_without_dropout():
    """use_dropout off: args.droprate is not read, whatever it holds, and no generator has a dropout level."""
    from stcgan_amd.stcgan import STCGAN
    a = types.SimpleNamespace(devices=["cuda:0"], tasks=["train"], lr_G=5e-5, lr_D=2e-5, beta1=0.5, beta2=0.999,
                              D_loss_fn="standard", D_loss_type="normal", ngf=8, dtype="bf16",
                              load_weights_g1=None, load_weights_g2=None, load_weights_d1=None,
                              load_weights_d2=None, use_dropout=False, droprate=7.0)
    tr = STCGAN(a)
    assert tr.G1._make_plan().drop == {} and tr.G2._make_plan().drop == {}


def test_stream_schedules_bit_identical():
    x, m, y = _batch()
    res = []
    for streams in (True, False):
        tr = _trainer(streams=streams)
        for _ in range(2):
            tr.train_step(x, m, y)
        res.append(_state(tr))
        assert tr.G1.dropout_state() == (4242, 2) and tr.G2.dropout_state() == (4243, 2)
    bad = _same(*res)
    assert not bad, bad[:8]


def test_dropout_changes_the_step():
    """(the comparisons above are not vacuous: another seed is another result)"""
    x, m, y = _batch()
    a, b = _trainer(), _trainer()
    b.G1.set_dropout_seed(1)
    a.train_step(x, m, y)
    b.train_step(x, m, y)
    assert _same(_state(a), _state(b))


def test_captured_step_draws_the_eager_masks():
    x, m, y = _batch(B=2)
    eager, graphed = _trainer(), _trainer()
    replay = graphed.capture(x, m, y, warmup=1)  # 3 eager steps inside
    for _ in range(3):
        eager.train_step(x, m, y)
    assert not _same(_state(eager), _state(graphed))
    assert graphed.G1.dropout_state() == eager.G1.dropout_state() == (4242, 3)
    before = _state(graphed)
    deltas = []
    for i in range(2):
        eager.train_step(x, m, y)
        replay()
        now = _state(graphed)
        bad = _same(_state(eager), now)
        assert not bad, (i, bad[:8])
        # the replay advanced the device counter: a fresh mask, the one the eager step drew
        assert graphed.G1.dropout_state() == eager.G1.dropout_state() == (4242, 4 + i)
        assert graphed.G2.dropout_state() == eager.G2.dropout_state() == (4243, 4 + i)
        k = "model.model.1.model.3.model.3.model.3.model.5.weight"  # a ConvT right below a dropout level
        deltas.append(now["G2"][k] - before["G2"][k])
        before = now
    assert not torch.equal(deltas[0], deltas[1])


def test_checkpoint_resume(tmp_path):
    x, m, y = _batch()
    tr = _trainer()
    tr.train_step(x, m, y)
    path = str(tmp_path / "ck.tar")
    tr.save_checkpoint(1, path)
    tr.train_step(x, m, y)
    fresh = _trainer()
    fresh.G1.set_dropout_seed(5)  # (overwritten by the load)
    fresh.load_checkpoint(path)
    assert fresh.G1.dropout_state() == (4242, 1) and fresh.G2.dropout_state() == (4243, 1)
    fresh.train_step(x, m, y)
    bad = _same(_state(tr), _state(fresh))
    assert not bad, bad[:8]
    # a checkpoint without the key (written before dropout existed) still loads; the generators keep their state
    ck = torch.load(path, map_location="cpu", weights_only=True)
    del ck["dropout"]
    torch.save(ck, path)
    other = _trainer()
    other.load_checkpoint(path)
    assert other.G1.dropout_state() == (4242, 0)
