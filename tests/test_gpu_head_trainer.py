"""args.activation through the trainer (ngf 8, batch 2, 256 x 256, synthetic triplets): absent and "tanh" are the same
step bit for bit -- parameters, BatchNorm buffers, Adam moments, losses; with "sigmoid" and "htanh" two steps are
finite, the one-stream schedule and a captured graph's replays give the eager default-schedule steps bit for bit (as
tests/test_gpu_upconv_trainer.py checks them), and a checkpoint round trip continues bit-identically."""
import math
import types

import pytest
import torch
import torch.nn as nn

from test_gpu_upconv_trainer import _batch, _same, _state

pytestmark = pytest.mark.gpu
HEADS = {"tanh": nn.Tanh, "sigmoid": nn.Sigmoid, "htanh": nn.Hardtanh}


def _trainer(dtype="bf16", loss_type="normal", **kw):
    from stcgan_amd.stcgan import STCGAN
    torch.manual_seed(7)
    a = dict(devices=["cuda:0"], tasks=["train"], lr_G=5e-5, lr_D=2e-5, beta1=0.5, beta2=0.999,
             D_loss_fn="standard", D_loss_type=loss_type, ngf=8, dtype=dtype, load_weights_g1=None,
             load_weights_g2=None, load_weights_d1=None, load_weights_d2=None)
    return STCGAN(types.SimpleNamespace(**{**a, **kw}))


def _steps(tr, n, batch):
    out = []
    for _ in range(n):
        vals = tr.train_step(*batch)
        torch.cuda.synchronize()
        out.append({k: float(v) for k, v in vals.items()})
    return out


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_absent_is_tanh(dtype):
    batch = _batch()
    a, b = _trainer(dtype), _trainer(dtype, activation="tanh")
    assert a.activation == b.activation == "tanh"
    for g in (a.G1, a.G2, b.G1, b.G2):
        assert g.activation == "tanh" and g._make_plan().head == "tanh" and type(g.model.model[4]) is nn.Tanh
    la, lb = _steps(a, 2, batch), _steps(b, 2, batch)
    assert la == lb, (la, lb)
    bad = _same(_state(a), _state(b))
    assert not bad, bad[:8]


def test_trainer_validates_the_option():
    from stcgan_amd.stcgan import STCGAN
    for bad in ("relu", None, 1):
        ns = types.SimpleNamespace(devices=["cuda:0"], tasks=["train"], ngf=8, activation=bad)
        with pytest.raises(ValueError, match="'none', 'sigmoid', 'tanh'"):
            STCGAN(ns)
    tr = _trainer(activation="none")
    assert tr.activation == "none" and len(tr.G1.model.model) == 4 and tr.G2._make_plan().head == "none"


@pytest.mark.parametrize("act", ["sigmoid", "htanh"])
def test_two_steps_finite_and_schedules_bit_identical(act):
    batch = _batch()
    res, losses = [], []
    for streams in (True, False):
        tr = _trainer(activation=act, streams=streams)
        for g in (tr.G1, tr.G2):
            assert g.activation == act and g._make_plan().head == act and type(g.model.model[4]) is HEADS[act]
        losses.append(_steps(tr, 2, batch))
        res.append(_state(tr))
    assert all(math.isfinite(v) for run in losses for s in run for v in s.values()), losses
    assert losses[0] == losses[1], losses
    assert losses[0][0]["G"] != losses[0][1]["G"]  # (the second step starts from other weights)
    bad = _same(*res)
    assert not bad, bad[:8]
    for n in ("G1", "G2", "D1", "D2"):
        assert all(bool(torch.isfinite(v.float()).all()) for v in res[0][n].values()), n
    # (not vacuous: another head is another step)
    ref = _trainer()
    _steps(ref, 2, batch)
    sr = _state(ref)
    assert any(not torch.equal(sr["G2"][k], res[0]["G2"][k]) for k in sr["G2"])


@pytest.mark.parametrize("act", ["sigmoid", "htanh"])
def test_captured_step_is_bit_identical(act):
    """tests/test_gpu_upconv_trainer.py::test_captured_step_is_bit_identical (fp32, rel_avg) with a non-default head."""
    x, m, y = _batch(B=2)
    eager = _trainer("fp32", "rel_avg", activation=act)
    graphed = _trainer("fp32", "rel_avg", activation=act)
    replay = graphed.capture(x, m, y, warmup=1)  # 3 eager steps inside (warm-up + two in device-step mode)
    for _ in range(3):
        eager.train_step(x, m, y)
    assert not _same(_state(eager), _state(graphed))
    for i in range(2):
        eager.train_step(x, m, y)
        replay()
        bad = _same(_state(eager), _state(graphed))
        assert not bad, (i, bad[:8])
    g = torch.Generator(device="cuda").manual_seed(11)
    x.copy_(torch.rand((2, 3, 256, 256), generator=g, device="cuda") * 2 - 1)  # new contents in place
    eager.train_step(x, m, y)
    replay()
    assert not _same(_state(eager), _state(graphed))


@pytest.mark.parametrize("act", ["sigmoid", "htanh"])
def test_checkpoint_round_trip(act, tmp_path):
    batch = _batch()
    tr = _trainer(activation=act)
    tr.train_step(*batch)
    path = str(tmp_path / "ck.tar")
    tr.save_checkpoint(1, path)
    tr.train_step(*batch)
    fresh = _trainer(activation=act)
    fresh.load_checkpoint(path)
    fresh.train_step(*batch)
    bad = _same(_state(tr), _state(fresh))
    assert not bad, bad[:8]
    # no head has parameters: the checkpoint loads across heads (and then steps differently)
    other = _trainer()
    other.load_checkpoint(path)
    a, b = other.G2.state_dict(), fresh.G2.state_dict()
    assert list(a) == list(b)
