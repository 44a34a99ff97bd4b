"""args.padding_mode="reflect" through the trainer (ngf 8, batch 2, 256 x 256, synthetic triplets), fp32 and bf16: two
train steps are finite; the multi-stream step equals the one-stream step, overlap_optim on equals off, and a captured
graph's replays equal the eager steps -- parameters, BatchNorm buffers and Adam moments bit for bit (nothing host-side
is baked into a reflect launch); the forward after an optimiser step equals a fresh network loaded from the
state_dict (the packed operands are the existing pack modes, rewritten by the fused Adam + repack step).

The default trainer goes through the same sequence of stcgan_amd.ops calls as on the commit before this feature:
tests/golden/reflect_default_trainer_ops.json was recorded there with ``record_ops`` below."""
import json
import math
import os
import types

import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu
NETS = ("G1", "G2", "D1", "D2")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reflect_default_trainer_ops.json")


def trainer(dtype="bf16", loss_type="normal", **kw):
    from stcgan_amd.stcgan import STCGAN
    torch.manual_seed(7)
    a = dict(devices=["cuda:0"], tasks=["train"], lr_G=5e-5, lr_D=2e-5, beta1=0.5, beta2=0.999,
             D_loss_fn="standard", D_loss_type=loss_type, ngf=8, dtype=dtype, load_weights_g1=None,
             load_weights_g2=None, load_weights_d1=None, load_weights_d2=None)
    return STCGAN(types.SimpleNamespace(**{**a, **kw}))


def reflect(dtype="bf16", loss_type="normal", **kw):
    tr = trainer(dtype, loss_type, padding_mode="reflect", **kw)
    assert tr.padding_mode == "reflect"
    for n in NETS:
        k4 = [m for m in getattr(tr, n).modules() if isinstance(m, nn.Conv2d) and tuple(m.kernel_size) == (4, 4)]
        assert len(k4) == (8 if n[0] == "G" else 5) and all(m.padding_mode == "reflect" for m in k4), n
    return tr


def state(tr):
    torch.cuda.synchronize()
    st = {n: {k: v.detach().clone() for k, v in getattr(tr, n).state_dict().items()} for n in NETS}
    for oname in ("optim_G", "optim_D"):
        o = getattr(tr, oname)
        o.sync_steps()
        st[oname] = [(float(o.state[p]["step"]), o.state[p]["exp_avg"].clone(), o.state[p]["exp_avg_sq"].clone())
                     for g in o.param_groups for p in g["params"]]
    return st


def differing(a, b):
    bad = [(n, k) for n in NETS for k in a[n] if not torch.equal(a[n][k], b[n][k])]
    for oname in ("optim_G", "optim_D"):
        bad += [(oname, i) for i, (x, y) in enumerate(zip(a[oname], b[oname]))
                if x[0] != y[0] or not torch.equal(x[1], y[1]) or not torch.equal(x[2], y[2])]
    return bad


def batch(seed=3, B=2):
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.rand((B, 3, 256, 256), generator=g, device="cuda") * 2 - 1
    m = (torch.rand((B, 1, 256, 256), generator=g, device="cuda") < 0.5).float() * 2 - 1
    y = torch.rand((B, 3, 256, 256), generator=g, device="cuda") * 2 - 1
    return x, m, y


def steps(tr, n, b):
    out = []
    for _ in range(n):
        vals = tr.train_step(*b)
        torch.cuda.synchronize()
        out.append({k: float(v) for k, v in vals.items()})
    return out


def test_trainer_validates_the_option():
    from stcgan_amd.stcgan import STCGAN
    for bad in ("replicate", "circular", None, 1):
        ns = types.SimpleNamespace(devices=["cuda:0"], tasks=["train"], ngf=8, padding_mode=bad)
        with pytest.raises(ValueError, match="zeros.*reflect"):
            STCGAN(ns)
    assert trainer().padding_mode == "zeros" and trainer(padding_mode="zeros").padding_mode == "zeros"


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_two_steps_and_schedules_bit_identical(dtype):
    b = batch()
    res, losses = [], []
    for streams in (True, False):
        tr = reflect(dtype, streams=streams)
        losses.append(steps(tr, 2, b))
        res.append(state(tr))
    assert all(math.isfinite(v) for run in losses for s in run for v in s.values()), losses
    assert losses[0] == losses[1], losses
    assert losses[0][0]["G"] != losses[0][1]["G"]  # (the second step starts from other weights)
    bad = differing(*res)
    assert not bad, bad[:8]
    for n in NETS:
        assert all(bool(torch.isfinite(v.float()).all()) for v in res[0][n].values()), n
    ref = trainer(dtype)  # (not vacuous: zero padding is another step)
    steps(ref, 2, b)
    sr = state(ref)
    assert any(not torch.equal(sr["D1"][k], res[0]["D1"][k]) for k in sr["D1"])


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_overlap_optim_bit_identical(dtype):
    b = batch()
    res = []
    for on in (True, False):
        tr = reflect(dtype, overlap_optim=on)
        steps(tr, 2, b)
        res.append(state(tr))
    bad = differing(*res)
    assert not bad, bad[:8]


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_captured_step_is_bit_identical(dtype):
    """As tests/test_gpu_head_trainer.py::test_captured_step_is_bit_identical, with reflect padding."""
    x, m, y = batch(B=2)
    eager = reflect(dtype, "rel_avg")
    graphed = reflect(dtype, "rel_avg")
    replay = graphed.capture(x, m, y, warmup=1)  # 3 eager steps inside (warm-up + two in device-step mode)
    for _ in range(3):
        eager.train_step(x, m, y)
    assert not differing(state(eager), state(graphed))
    for i in range(2):
        eager.train_step(x, m, y)
        replay()
        bad = differing(state(eager), state(graphed))
        assert not bad, (i, bad[:8])
    g = torch.Generator(device="cuda").manual_seed(11)
    x.copy_(torch.rand((2, 3, 256, 256), generator=g, device="cuda") * 2 - 1)  # new contents in place
    eager.train_step(x, m, y)
    replay()
    assert not differing(state(eager), state(graphed))


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_forward_after_a_step_equals_a_fresh_network(dtype):
    from stcgan_amd import networks
    b = batch()
    tr = reflect(dtype)
    steps(tr, 2, b)
    x = torch.cat((b[0], b[1]), 1)
    for name, make in (("G2", lambda: networks.get_generator(4, 3, ngf=8, padding_mode="reflect")),
                       ("D1", lambda: networks.get_discriminator(4, ndf=8, padding_mode="reflect"))):
        net = getattr(tr, name)
        fresh = make()
        fresh.load_state_dict(net.state_dict())
        fresh.to("cuda").set_compute_dtype(dtype)
        was = net.training
        net.eval(), fresh.eval()
        with torch.no_grad():
            ya, yb = net(x), fresh(x)
        net.train(was)
        torch.cuda.synchronize()
        assert torch.equal(ya, yb), (name, float((ya - yb).abs().max()))


# ---------------------------------------------------------------- the default trainer's call sequence
def record_ops(fn):
    """The names of the stcgan_amd.ops functions called during fn(), in call order (the recorder of
    tests/test_gpu_eval_backward.py)."""
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


def default_sequence(dtype):
    """The ops calls of the third step of a default trainer (plans, packs and optimiser state made by the first two)."""
    tr = trainer(dtype)
    b = batch()
    steps(tr, 2, b)
    return record_ops(lambda: tr.train_step(*b))


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_default_trainer_call_sequence_is_untouched(dtype):
    with open(GOLDEN) as f:
        want = json.load(f)[dtype]
    got = default_sequence(dtype)
    assert len(want) > 100 and got == want, [(i, a, b) for i, (a, b) in enumerate(zip(got, want)) if a != b][:5]
    new = {"conv_pad", "conv_pad_query", "conv_pad_dgrad_query", "wgrad_pad_query"}
    assert not new & set(got)
    tr = reflect(dtype)
    b = batch()
    steps(tr, 2, b)
    seq = record_ops(lambda: tr.train_step(*b))
    assert seq.count("conv_pad") >= 2 * (8 + 8 + 5 + 5) and "conv_bn_backward" in seq  # (the up path stays fused)
    assert "conv_act" not in seq and "conv_act_backward" not in seq
