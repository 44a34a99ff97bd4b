"""VisualLoss without a GPU: the vgg19_bn feature layout and state_dict loading, the Sequential grammar, the fp32
BatchNorm fold, eval / frozen behaviour, argument validation of the new C-ABI calls, and the trainer's configuration."""
import types

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from visual_ref import EPS32, F64, QUARTER, fold64, seed_features

CONVS = (0, 3, 7, 10, 14, 17, 20, 23, 27, 30, 33, 36)
POOLS = (6, 13, 26, 39)


def test_feature_layout_is_torchvisions():
    from stcgan_amd.loss import vgg19_bn_features
    seq = vgg19_bn_features()
    assert len(seq) == 40 and isinstance(seq[39], nn.MaxPool2d)
    for i, m in enumerate(seq):
        if i in CONVS:
            assert isinstance(m, nn.Conv2d) and m.kernel_size == (3, 3) and m.padding == (1, 1)
            assert isinstance(seq[i + 1], nn.BatchNorm2d) and isinstance(seq[i + 2], nn.ReLU)
        elif i in POOLS:
            assert isinstance(m, nn.MaxPool2d) and m.kernel_size == 2 and m.stride == 2
    assert [seq[i].out_channels for i in CONVS] == [64, 64, 128, 128, 256, 256, 256, 256, 512, 512, 512, 512]
    assert seq[0].in_channels == 3
    assert not seq.training and not any(p.requires_grad for p in seq.parameters())
    full = vgg19_bn_features(upto=53)
    assert len(full) == 53 and isinstance(full[52], nn.MaxPool2d) and isinstance(full[40], nn.Conv2d)
    q = vgg19_bn_features(widths=QUARTER)
    assert [q[i].out_channels for i in CONVS] == [16, 16, 32, 32, 64, 64, 64, 64, 128, 128, 128, 128]


def test_torchvision_state_dict_loads():
    """A synthetic state_dict with torchvision's key names (all 16 conv groups and the classifier) loads; later
    features.* and classifier.* keys are ignored."""
    from stcgan_amd.loss import vgg19_bn_features
    src = seed_features(vgg19_bn_features(upto=53, widths=QUARTER), 3)
    sd = {"features." + k: v.clone() for k, v in src.state_dict().items()}
    sd.update({"classifier.0.weight": torch.zeros(4, 4), "classifier.0.bias": torch.zeros(4),
               "classifier.6.weight": torch.zeros(2, 4)})
    seq = vgg19_bn_features(sd, widths=QUARTER)
    assert len(seq) == 40
    for k, v in seq.state_dict().items():
        assert torch.equal(v, sd["features." + k]), k
    with pytest.raises(RuntimeError):  # a state_dict that lacks an entry is not loaded silently
        vgg19_bn_features({k: v for k, v in sd.items() if k != "features.3.weight"}, widths=QUARTER)


@pytest.mark.parametrize("bad,word", [
    (lambda: [nn.Conv2d(3, 8, 5, padding=2), nn.ReLU()], "Conv2d"),
    (lambda: [nn.Conv2d(3, 8, 3, stride=2, padding=1), nn.ReLU()], "Conv2d"),
    (lambda: [nn.Conv2d(3, 8, 3, padding=1, padding_mode="reflect"), nn.ReLU()], "reflect"),
    (lambda: [nn.Conv2d(3, 8, 3, padding=1), nn.ReLU(), nn.MaxPool2d(3)], "MaxPool2d"),
    (lambda: [nn.Conv2d(3, 8, 3, padding=1), nn.ReLU(), nn.Sigmoid()], "Sigmoid"),
    (lambda: [nn.Conv2d(3, 8, 3, padding=1), nn.Sigmoid()], "Sigmoid"),
])
def test_grammar_refusals_name_the_module(bad, word):
    from stcgan_amd.loss import VisualLoss
    with pytest.raises(NotImplementedError, match=word):
        VisualLoss(nn.Sequential(*bad()))


def test_norm_and_reduction_refusals():
    from stcgan_amd.loss import VisualLoss
    seq = nn.Sequential(nn.Conv2d(3, 8, 3, padding=1), nn.ReLU())
    VisualLoss(seq, norm=F.mse_loss)
    for kw in (dict(norm=F.l1_loss), dict(reduction="sum"), dict(reduction="none")):
        with pytest.raises(NotImplementedError, match="mse_loss"):
            VisualLoss(seq, **kw)


def test_fold_matches_fp64_formula():
    """folded() is within 4 * 2^-23 * (|w s| resp. the |terms| of b') of the fp64 formula; refresh() folds again."""
    from stcgan_amd.loss import VisualLoss, vgg19_bn_features
    seq = seed_features(vgg19_bn_features(widths=QUARTER), 9)
    mod = VisualLoss(seq)
    want = fold64(seq)
    got = mod.folded()
    assert len(got) == 12
    for (w, b), (w64, b64, babs) in zip(got, want):
        assert w.dtype == torch.float32 and b.dtype == torch.float32 and w.shape == w64.shape
        assert bool(((w.double() - w64).abs() <= 4 * EPS32 * w64.abs()).all())
        assert bool(((b.double() - b64).abs() <= 4 * EPS32 * babs).all())
    before = got[0][0].clone()
    with torch.no_grad():
        seq[1].weight.mul_(2.0)
    assert torch.equal(mod.folded()[0][0], before)
    mod.refresh()
    assert torch.equal(mod.folded()[0][0], before * 2.0)
    # without BatchNorm and without a bias: w itself and zeros
    plain = nn.Sequential(nn.Conv2d(3, 8, 3, padding=1, bias=False), nn.ReLU())
    (w, b), = VisualLoss(plain).folded()
    assert torch.equal(w, plain[0].weight.detach()) and not b.any()


def test_always_eval_and_frozen():
    from stcgan_amd.loss import VisualLoss, vgg19_bn_features
    seq = vgg19_bn_features(widths=QUARTER)
    seq.train().requires_grad_(True)
    mod = VisualLoss(seq)
    assert not mod.training and not seq.training
    assert mod.train() is mod and not mod.training and not mod.train(True).training
    assert list(mod.parameters()) == [] and list(mod.buffers()) == [] and len(mod.state_dict()) == 0
    assert not any(p.requires_grad for p in seq.parameters())


def test_cpu_inputs_fail_loudly():
    from stcgan_amd.loss import VisualLoss
    mod = VisualLoss(nn.Sequential(nn.Conv2d(3, 8, 3, padding=1), nn.ReLU()))
    with pytest.raises(TypeError, match="CUDA"):
        mod(torch.zeros(1, 3, 8, 8), torch.zeros(1, 3, 8, 8))


def test_c_abi_argument_validation_before_any_launch():
    """The error text comes back through stc_last_error; nothing is launched (no GPU here)."""
    from stcgan_amd import _lib
    lib = _lib.lib()
    null = _lib.View(None, 4, 4, 0, 0, 8, 0, 1, 0)
    fake = _lib.View(4096, 4, 4, 128, 32, 8, 0, 1, 0)  # (never dereferenced: every call below fails its checks)
    rc = lib.stc_conv3_fwd(1, fake, 3, None, 8, fake, None, 1, _lib.NULL_VIEW, None)
    assert rc != 0 and b"Cin=3" in lib.stc_last_error()
    rc = lib.stc_conv3_fwd(1, null, 8, None, 8, fake, None, 1, _lib.NULL_VIEW, None)
    assert rc != 0 and b"input view is NULL" in lib.stc_last_error()
    rc = lib.stc_conv3_fwd(1, fake, 8, None, 8, fake, None, 1, _lib.NULL_VIEW, None)
    assert rc != 0 and b"packed weight is NULL" in lib.stc_last_error()
    rc = lib.stc_conv3_fwd(1 << 20, fake, 8, None, 8, fake, None, 1, _lib.NULL_VIEW, None)
    assert rc != 0 and b"2^24" in lib.stc_last_error()
    out = (_lib.ctypes.c_int32 * 8)()
    assert lib.stc_conv3_plan(1, 4, 4, 12, 8, out) != 0 and b"Cin=12" in lib.stc_last_error()
    assert lib.stc_conv3_plan(2, 20, 33, 64, 72, out) == 0
    path, th, tw, bn, kc, split, mt, nt = out
    assert mt == 2 * -(-20 // th) * -(-33 // tw) and nt == -(-72 // bn) and split >= 1 and kc % 8 == 0
    # a missing workspace
    rc = lib.stc_feat_mse_fwd(4096, 4096, 64, None, 4096, None)
    assert rc != 0 and b"workspace" in lib.stc_last_error()
    rc = lib.stc_feat_mse_fwd(4096, 4096, 12, 4096, 4096, None)
    assert rc != 0 and b"multiple of 8" in lib.stc_last_error()
    assert lib.stc_feat_mse_parts(8) == 1 and lib.stc_feat_mse_parts(4096 + 8) == 2
    rc = lib.stc_maxpool2_fwd(1, _lib.View(4096, 3, 4, 128, 32, 8, 0, 1, 0), 8, fake, None)
    assert rc != 0 and b"even" in lib.stc_last_error()
    rc = lib.stc_vgg_norm_fwd(1, 4, 4, None, 0, 0, 0, 0, fake, None)
    assert rc != 0 and b"source is NULL" in lib.stc_last_error()
    rc = lib.stc_vgg_norm_bwd(1, 4, 4, null, 4096, None)
    assert rc != 0 and b"gradient view is NULL" in lib.stc_last_error()
    rc = lib.stc_conv3_pack(0, None, None)
    assert rc != 0 and b"stc_conv3_pack" in lib.stc_last_error()
    with pytest.raises(RuntimeError, match="Cin=12"):
        _lib.check(lib.stc_conv3_plan(1, 4, 4, 12, 8, out), "stc_conv3_plan")


def test_trainer_configuration():
    """lambda4 = lambda5 = 0 (the default) builds no VisualLoss; a positive lambda needs the weights; negative
    lambdas are refused; args.visual_loss takes precedence over args.vgg_weights."""
    from stcgan_amd.loss import VisualLoss
    from stcgan_amd.stcgan import visual_loss_config
    ns = types.SimpleNamespace
    assert visual_loss_config(ns()) == (0.0, 0.0, None)
    assert visual_loss_config(ns(lambda4=0, lambda5=0.0, vgg_weights="/nonexistent"))[2] is None
    with pytest.raises(ValueError, match="vgg_weights"):
        visual_loss_config(ns(lambda5=0.5))
    for bad in (dict(lambda4=-1.0), dict(lambda5=-0.1), dict(lambda4=float("nan"))):
        with pytest.raises(ValueError, match="must be >= 0"):
            visual_loss_config(ns(**bad))
    mod = VisualLoss(nn.Sequential(nn.Conv2d(3, 8, 3, padding=1), nn.ReLU()))
    assert visual_loss_config(ns(lambda4=0.25, visual_loss=mod, vgg_weights="/nonexistent")) == (0.25, 0.0, mod)
    with pytest.raises(ValueError, match="VisualLoss"):
        visual_loss_config(ns(lambda4=0.25, visual_loss=nn.ReLU()))


def test_trainer_loads_weights_from_a_path(tmp_path):
    from stcgan_amd.loss import VisualLoss, vgg19_bn_features
    from stcgan_amd.stcgan import visual_loss_config
    src = seed_features(vgg19_bn_features(upto=53), 4)
    sd = {"features." + k: v for k, v in src.state_dict().items()}
    sd["classifier.0.weight"] = torch.zeros(2, 2)
    path = tmp_path / "vgg19_bn.pth"
    torch.save(sd, path)
    l4, l5, mod = visual_loss_config(types.SimpleNamespace(lambda5=1.0, vgg_weights=str(path)))
    assert (l4, l5) == (0.0, 1.0) and isinstance(mod, VisualLoss) and mod.num_pools == 4
    want = fold64(src[:40])
    assert bool(((mod.folded()[11][0].double() - want[11][0]).abs() <= 4 * EPS32 * want[11][0].abs()).all())
