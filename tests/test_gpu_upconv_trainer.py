"""args.NN_upconv=True through the trainer (ngf 16, batch 2, 256 x 256): both generators run resize-convolution up
layers; the stream schedule, the overlapped optimiser, a captured graph's replays and a checkpoint resume give the
eager steps' parameters, BatchNorm buffers and Adam moments bit for bit; save() writes state_dicts the torch.nn
restatement (tests/upconv_ref.py) loads; infer() writes its PNGs."""
import math
import os
import types

import numpy as np
import pytest
import torch
import torch.nn as nn

import upconv_ref as U

pytestmark = pytest.mark.gpu

NETS = ("G1", "G2", "D1", "D2")


def _trainer(dtype="bf16", loss_type="normal", upconv=True, **kw):
    from stcgan_amd.stcgan import STCGAN
    torch.manual_seed(7)
    a = dict(devices=["cuda:0"], tasks=["train"], lr_G=5e-5, lr_D=2e-5, beta1=0.5, beta2=0.999,
             D_loss_fn="standard", D_loss_type=loss_type, ngf=16, dtype=dtype, load_weights_g1=None,
             load_weights_g2=None, load_weights_d1=None, load_weights_d2=None, NN_upconv=upconv)
    return STCGAN(types.SimpleNamespace(**{**a, **kw}))


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


def test_trainer_builds_upconv_generators():
    tr = _trainer()
    for g in (tr.G1, tr.G2):
        assert g.no_conv_t and g._make_plan().upconv
        assert not any(isinstance(m, nn.ConvTranspose2d) for m in g.modules())
    assert tr.NN_upconv is True
    off = _trainer(upconv=False)
    assert off.NN_upconv is False and not off.G1._make_plan().upconv
    assert sum(isinstance(m, nn.ConvTranspose2d) for m in off.G2.modules()) == 8
    from stcgan_amd.stcgan import STCGAN
    bad = types.SimpleNamespace(devices=["cuda:0"], tasks=["train"], ngf=16, NN_upconv="yes")
    with pytest.raises(ValueError, match="args.NN_upconv must be a bool"):
        STCGAN(bad)


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_three_steps_finite_and_moving(dtype):
    x, m, y = _batch()
    tr = _trainer(dtype)
    seen = []
    for _ in range(3):
        vals = tr.train_step(x, m, y)
        torch.cuda.synchronize()
        seen.append({k: float(v) for k, v in vals.items()})
    assert all(math.isfinite(v) for s in seen for v in s.values()), seen
    for k in ("G", "D", "data1", "data2"):  # every step starts from other weights
        assert seen[0][k] != seen[1][k] and seen[1][k] != seen[2][k], (k, seen)
    # the 3x3 weights moved, and the next forward reads them
    start = _trainer(dtype)  # (the same seed: the initial weights)
    k = "model.model.1.model.5.1.weight"
    for g in ("G1", "G2"):
        assert not torch.equal(getattr(tr, g).state_dict()[k], getattr(start, g).state_dict()[k])


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


def test_overlap_optim_bit_identical():
    x, m, y = _batch()
    res = []
    for on in (True, False):
        tr = _trainer(overlap_optim=on)
        for _ in range(3):
            tr.train_step(x, m, y)
        res.append(_state(tr))
    bad = _same(*res)
    assert not bad, bad[:8]


def test_upconv_changes_the_step():
    """(the comparisons above are not vacuous: another generator is another discriminator update)"""
    x, m, y = _batch()
    a, b = _trainer(), _trainer(upconv=False)
    a.train_step(x, m, y)
    b.train_step(x, m, y)
    sa, sb = _state(a), _state(b)
    assert any(not torch.equal(sa["D1"][k], sb["D1"][k]) for k in sa["D1"])


def test_captured_step_is_bit_identical():
    """tests/test_gpu_graph.py::test_captured_step_is_bit_identical, fp32 row (fp32, ngf 16, rel_avg), with NN_upconv:
    the refresh launches are part of the graph and rewrite the operands the captured convs read."""
    x, m, y = _batch(B=2)
    eager = _trainer("fp32", "rel_avg")
    graphed = _trainer("fp32", "rel_avg")
    replay = graphed.capture(x, m, y, warmup=1)  # 3 eager steps inside (warm-up + two in device-step mode)
    for _ in range(3):
        eager.train_step(x, m, y)
    assert not _same(_state(eager), _state(graphed))
    for i in range(3):
        eager.train_step(x, m, y)
        replay()
        bad = _same(_state(eager), _state(graphed))
        assert not bad, (i, bad[:8])
    g = torch.Generator(device="cuda").manual_seed(11)
    x.copy_(torch.rand((2, 3, 256, 256), generator=g, device="cuda") * 2 - 1)  # new contents in place
    eager.train_step(x, m, y)
    replay()
    assert not _same(_state(eager), _state(graphed))
    assert float(graphed.optim_G.state[next(graphed.G1.parameters())]["step"]) == 7.0


def test_checkpoint_resume(tmp_path):
    x, m, y = _batch()
    tr = _trainer()
    tr.train_step(x, m, y)
    path = str(tmp_path / "ck.tar")
    tr.save_checkpoint(1, path)
    tr.train_step(x, m, y)
    fresh = _trainer()
    fresh.load_checkpoint(path)
    fresh.train_step(x, m, y)
    bad = _same(_state(tr), _state(fresh))
    assert not bad, bad[:8]
    with pytest.raises(RuntimeError, match="Missing key|Unexpected key"):  # the keys differ, as in torch
        _trainer(upconv=False).load_checkpoint(path)


def test_save_files_load_into_the_restatement(tmp_path):
    x, m, y = _batch()
    tr = _trainer(weights=str(tmp_path))
    tr.train_step(x, m, y)
    tr.save()
    for name, (ic, oc) in (("G1", (3, 1)), ("G2", (4, 3))):
        sd = torch.load(os.path.join(str(tmp_path), f"{name}-latest.pt"), map_location="cpu", weights_only=True)
        ref = U.UpRefG(ic, oc, 16, 8)
        ref.load_state_dict(sd)  # strict
        assert tuple(sd["model.model.3.1.weight"].shape) == (oc, 32, 3, 3)
    # and init_weight reads them back
    again = _trainer(load_weights_g1=os.path.join(str(tmp_path), "G1-latest.pt"))
    a, b = again.G1.state_dict(), tr.G1.state_dict()
    assert all(torch.equal(a[k], b[k]) for k in b)


def test_infer_writes_pngs(tmp_path):
    from PIL import Image
    from stcgan_amd.stcgan import STCGAN
    torch.manual_seed(3)
    a = types.SimpleNamespace(devices=["cuda:0"], tasks=["infer", "train"], lr_G=5e-5, lr_D=2e-5, beta1=0.5,
                              beta2=0.999, ngf=16, dtype="fp32", infered=str(tmp_path), load_weights_g1=None,
                              load_weights_g2=None, load_weights_d1=None, load_weights_d2=None, NN_upconv=True)
    tr = STCGAN(a)
    x = torch.rand((2, 3, 256, 256)) * 2 - 1
    tr.valid_loader = [(["a", "b"], x, None, None)]
    res = tr.infer()
    assert [r[0] for r in res] == ["a", "b"]
    for i, name in enumerate(["a", "b"]):
        mk = np.asarray(Image.open(tmp_path / "mask" / f"{name}.png"))
        sl = np.asarray(Image.open(tmp_path / "shadowless" / f"{name}.png"))[:, :, ::-1]
        assert mk.shape == (192, 256) and sl.shape == (192, 256, 3)
        np.testing.assert_array_equal(mk, res[i][1])
        np.testing.assert_array_equal(sl, res[i][2])
        assert len(np.unique(sl)) > 1
