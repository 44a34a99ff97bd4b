"""Resize-convolution up path (UnetGenerator(no_conv_t=True), args.NN_upconv) without a GPU: the module tree against
the torch.nn restatement (tests/upconv_ref.py), the refusals, the numpy restatement of the weight identity against fp64
and against torch's own Upsample + Conv2d autograd, and the C-ABI's argument validation (nothing is launched)."""
import functools

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import upconv_ref as U

AFFINE = functools.partial(nn.InstanceNorm2d, affine=True)


@pytest.mark.parametrize("norm", [nn.BatchNorm2d, nn.InstanceNorm2d, AFFINE], ids=["batch", "instance", "affine"])
@pytest.mark.parametrize("ngf", [8, 64])
@pytest.mark.parametrize("in_c,out_c", [(3, 1), (4, 3)])
def test_state_dict_matches_restatement(in_c, out_c, ngf, norm):
    from stcgan_amd import networks
    net = networks.get_generator(in_c, out_c, ngf=ngf, norm_layer=norm, no_conv_t=True)
    ref = U.UpRefG(in_c, out_c, ngf, 8, norm)
    sd, rd = net.state_dict(), ref.state_dict()
    assert list(sd) == list(rd)
    assert all(tuple(sd[k].shape) == tuple(rd[k].shape) for k in sd)
    # the keys the issue names: N.1.weight [cout, cin, 3, 3], and the outermost layer's bias
    assert tuple(sd["model.model.3.1.weight"].shape) == (out_c, 2 * ngf, 3, 3)
    assert tuple(sd["model.model.3.1.bias"].shape) == (out_c,)
    assert tuple(sd["model.model.1.model.5.1.weight"].shape) == (ngf, 4 * ngf, 3, 3)
    assert "model.model.1.model.5.1.bias" not in sd
    assert not any(isinstance(m, nn.ConvTranspose2d) for m in net.modules())
    ups = [m for m in net.modules() if isinstance(m, nn.Upsample)]
    assert len(ups) == 8 and all(u.scale_factor == 2 and u.mode == "nearest" for u in ups)
    assert all(m.padding_mode == "zeros" for m in net.modules() if isinstance(m, nn.Conv2d))
    ref.load_state_dict(sd)  # strict


def test_state_dict_with_dropout_and_depth():
    from stcgan_amd import networks
    net = networks.get_generator(3, 1, ngf=8, use_dropout=True, drop_rate=0.25, no_conv_t=True)
    ref = U.UpRefG(3, 1, 8, 8, nn.BatchNorm2d, use_dropout=True)
    assert list(net.state_dict()) == list(ref.state_dict())
    assert [m.p for m in net.modules() if isinstance(m, nn.Dropout)] == [0.25] * 3
    net = networks.get_generator(3, 1, ngf=8, num_downs=6, no_conv_t=True)
    ref = U.UpRefG(3, 1, 8, 6)
    assert list(net.state_dict()) == list(ref.state_dict())


def test_default_tree_unchanged():
    from oracle import stcgan_ref as ref
    from stcgan_amd import engine, networks
    for kw in ({}, {"no_conv_t": False}):
        net = networks.get_generator(4, 3, ngf=8, **kw)
        tmpl = ref.generator_state_template(4, 3, 8)
        sd = net.state_dict()
        assert list(sd) == list(tmpl) and all(tuple(sd[k].shape) == tuple(tmpl[k].shape) for k in sd)
        assert sum(isinstance(m, nn.ConvTranspose2d) for m in net.modules()) == 8
        assert not any(isinstance(m, nn.Upsample) for m in net.modules())
        plan = engine.GenPlan(net)
        assert plan.upconv is False
        assert (plan.pack_t_fwd, plan.pack_t_dgrad) == (3, 4)
    # the two constructions draw the same initial weights (same modules made in the same order)
    torch.manual_seed(5)
    a = networks.get_generator(3, 1, ngf=8).state_dict()
    torch.manual_seed(5)
    b = networks.get_generator(3, 1, ngf=8, no_conv_t=False).state_dict()
    assert all(torch.equal(a[k], b[k]) for k in a)


def test_plan_of_upconv_tree():
    from stcgan_amd import engine, networks
    net = networks.get_generator(4, 3, ngf=8, no_conv_t=True)
    plan = engine.GenPlan(net)
    assert plan.upconv is True and plan.out_c == 3 and plan.L == 8
    assert (plan.pack_t_fwd, plan.pack_t_dgrad) == (5, 6)
    assert all(isinstance(plan.convT[k], nn.Conv2d) and plan.convT[k].kernel_size == (3, 3) for k in range(8))
    assert plan.convT[0].bias is not None and all(plan.convT[k].bias is None for k in range(1, 8))
    assert len(plan.params) == len(list(net.parameters()))


def test_weights_init_touches_the_new_convs():
    from stcgan_amd import networks
    net = networks.get_generator(3, 1, ngf=8, no_conv_t=True)
    ups = [m[1] for m in net.modules() if isinstance(m, nn.Sequential) and len(m) == 2 and isinstance(m[0], nn.Upsample)]
    assert len(ups) == 8
    with torch.no_grad():
        for c in ups:
            c.weight.fill_(7.0)
            if c.bias is not None:
                c.bias.fill_(7.0)
    torch.manual_seed(3)
    net.apply(networks.weights_init)
    for c in ups:
        w = c.weight.detach()
        assert float(w.abs().max()) < 0.2 and float(w.std()) > 0.005  # N(0, 0.02)
        assert c.bias is None or float(c.bias.detach().abs().max()) == 0.0


def _up_layers(net):
    return [(n, m) for n, m in net.named_modules()
            if isinstance(m, nn.Sequential) and len(m) == 2 and isinstance(m[0], nn.Upsample)]


def test_reflect_up_layer_is_refused():
    from stcgan_amd import engine, networks
    net = networks.get_generator(3, 1, ngf=8, no_conv_t=True)
    name, pair = _up_layers(net)[2]
    c = pair[1]
    pair[1] = nn.Conv2d(c.in_channels, c.out_channels, 3, 1, 1, bias=False, padding_mode="reflect")
    with pytest.raises(NotImplementedError, match=name.replace(".", r"\.") + r".*reflect"):
        engine.GenPlan(net)


@pytest.mark.parametrize("what", ["kernel", "scale", "mode"])
def test_other_up_layer_forms_are_refused(what):
    from stcgan_amd import engine, networks
    net = networks.get_generator(3, 1, ngf=8, no_conv_t=True)
    name, pair = _up_layers(net)[1]
    c = pair[1]
    if what == "kernel":
        pair[1] = nn.Conv2d(c.in_channels, c.out_channels, 5, 1, 2, bias=False)
    elif what == "scale":
        pair[0] = nn.Upsample(scale_factor=4, mode="nearest")
    else:
        pair[0] = nn.Upsample(scale_factor=2, mode="bilinear")
    with pytest.raises(NotImplementedError, match=name.replace(".", r"\.")):
        engine.GenPlan(net)


def test_mixed_tree_is_refused():
    from stcgan_amd import engine, networks
    net = networks.get_generator(3, 1, ngf=8, no_conv_t=True)
    other = networks.get_generator(3, 1, ngf=8)
    net.model.model[3] = other.model.model[3]  # the outermost up layer back to a ConvTranspose2d
    with pytest.raises(NotImplementedError, match="mixing ConvTranspose2d and Upsample"):
        engine.GenPlan(net)
    other.model.model[1].model[5] = U.up_pair(32, 8, False)
    with pytest.raises(NotImplementedError, match=r"mixing.*model\.model\.1\.model\.5"):
        engine.GenPlan(other)


@pytest.mark.parametrize("bad", ["yes", 2, None, 1.0])
def test_non_bool_flag_is_refused(bad):
    from stcgan_amd import networks
    from stcgan_amd.stcgan import check_nn_upconv
    with pytest.raises(ValueError, match="args.NN_upconv must be a bool"):
        check_nn_upconv(bad)
    assert check_nn_upconv(True) is True and check_nn_upconv(0) is False
    with pytest.raises(ValueError, match="no_conv_t must be a bool"):
        networks.get_generator(3, 1, ngf=8, no_conv_t=bad)


def test_trainer_reads_the_flag_through_that_checker():
    """STCGAN.__init__ calls check_nn_upconv on args.NN_upconv (read from the source: the constructor needs a GPU)."""
    import inspect
    from stcgan_amd import stcgan
    src = inspect.getsource(stcgan.STCGAN.__init__)
    assert 'check_nn_upconv(getattr(args, "NN_upconv", False))' in src


# ---------------------------------------------------------------- the identity
def _w3(Ci, Co, seed):
    return torch.randn(Co, Ci, 3, 3, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


@pytest.mark.parametrize("B,Ci,Co,H,W", U.SHAPES)
def test_numpy_expand_collapse_against_fp64(B, Ci, Co, H, W):
    w3 = _w3(Ci, Co, 1).float()
    want = np.einsum("ka,oiab,lb->iokl", U.M, w3.double().numpy(), U.M)
    got = U.expand(w3.numpy())
    assert got.dtype == np.float32 and got.shape == (Ci, Co, 4, 4)
    # at most 3 fp32 additions of 4 terms: 3 roundings of partial sums bounded by sum |terms|
    bound = 3 * 2.0 ** -24 * np.einsum("ka,oiab,lb->iokl", U.M, w3.double().abs().numpy(), U.M) + 1e-300
    assert float((np.abs(got - want) / bound).max()) <= 1.0
    g4 = torch.randn(Ci, Co, 4, 4, generator=torch.Generator().manual_seed(2)).float()
    wantc = np.einsum("ka,iokl,lb->oiab", U.M, g4.double().numpy(), U.M)
    gotc = U.collapse(g4.numpy())
    assert gotc.dtype == np.float32 and gotc.shape == (Co, Ci, 3, 3)
    boundc = 3 * 2.0 ** -24 * np.einsum("ka,iokl,lb->oiab", U.M, g4.double().abs().numpy(), U.M)
    assert float((np.abs(gotc - wantc) / boundc).max()) <= 1.0
    # adjointness, exactly, on small integers (every sum exact)
    wi = torch.randint(-8, 9, (Co, Ci, 3, 3)).float().numpy()
    gi = torch.randint(-8, 9, (Ci, Co, 4, 4)).float().numpy()
    assert float((U.expand(wi).astype(np.float64) * gi).sum()) == float((wi.astype(np.float64) * U.collapse(gi)).sum())


def test_numpy_order_is_the_documented_one():
    """Terms chosen so that another association of the 4-term sums changes the fp32 result."""
    w = np.zeros((1, 1, 3, 3), dtype=np.float32)
    w[0, 0, 1, 1], w[0, 0, 1, 2], w[0, 0, 2, 1], w[0, 0, 2, 2] = 2.0 ** 24, 1.0, 1.0, -2.0 ** 24
    f = np.float32
    assert U.expand(w)[0, 0, 1, 1] == f(f(f(w[0, 0, 1, 1] + w[0, 0, 1, 2]) + w[0, 0, 2, 1]) + w[0, 0, 2, 2]) == 0.0
    g = np.zeros((1, 1, 4, 4), dtype=np.float32)
    g[0, 0, 1, 1], g[0, 0, 1, 2], g[0, 0, 2, 1], g[0, 0, 2, 2] = 2.0 ** 24, 1.0, 1.0, -2.0 ** 24
    assert U.collapse(g)[0, 0, 1, 1] == 0.0 and U.collapse(g)[0, 0, 0, 0] == -2.0 ** 24


@pytest.mark.parametrize("B,Ci,Co,H,W", U.SHAPES)
def test_identity_against_torch_autograd(B, Ci, Co, H, W):
    """F.interpolate + F.conv2d and their autograd (fp64) against conv_transpose2d with the expanded weight and the
    collapsed weight gradient; the zero border included (H = W = 1)."""
    g = torch.Generator().manual_seed(10 + Ci)
    x = torch.randn(B, Ci, H, W, generator=g, dtype=torch.float64, requires_grad=True)
    w3 = _w3(Ci, Co, 3).requires_grad_(True)
    y = F.conv2d(F.interpolate(x, scale_factor=2, mode="nearest"), w3, None, 1, 1)
    r = torch.randn(y.shape, generator=g, dtype=torch.float64)
    (y * r).sum().backward()
    W4 = torch.from_numpy(np.einsum("ka,oiab,lb->iokl", U.M, w3.detach().numpy(), U.M)).requires_grad_(True)
    x2 = x.detach().clone().requires_grad_(True)
    y2 = F.conv_transpose2d(x2, W4, None, 2, 1)
    (y2 * r).sum().backward()
    dw3 = torch.from_numpy(np.einsum("ka,iokl,lb->oiab", U.M, W4.grad.numpy(), U.M))
    assert float((y - y2).detach().abs().max()) <= 1e-12
    assert float((x.grad - x2.grad).abs().max()) <= 1e-12
    assert float((w3.grad - dw3).abs().max()) <= 1e-12
    # and the fp32 numpy restatement of the same maps, to fp32 rounding
    e = U.expand(w3.detach().float().numpy()).astype(np.float64) - W4.detach().numpy()
    assert float(np.abs(e).max()) <= 4 * 2.0 ** -23 * float(w3.detach().abs().max()) * 4


def test_reflect_equals_replicate_of_the_low_resolution_input():
    """Why "reflect" is out of scope, not equivalent: it is the same ConvT on the input replicate-padded by one pixel
    (then cropped), which a zero-filling halo cannot express."""
    g = torch.Generator().manual_seed(4)
    x = torch.randn(2, 3, 5, 4, generator=g, dtype=torch.float64)
    w3 = _w3(3, 2, 5)
    up = F.interpolate(x, scale_factor=2, mode="nearest")
    want = F.conv2d(F.pad(up, (1, 1, 1, 1), mode="reflect"), w3)
    W4 = torch.from_numpy(np.einsum("ka,oiab,lb->iokl", U.M, w3.numpy(), U.M))
    got = F.conv_transpose2d(F.pad(x, (1, 1, 1, 1), mode="replicate"), W4, None, 2, 1)[:, :, 2:-2, 2:-2]
    assert float((want - got).abs().max()) <= 1e-12


# ---------------------------------------------------------------- C-ABI validation (no launch)
def test_capi_validation():
    from stcgan_amd import _lib
    lib = _lib.lib()
    one = 16  # a non-null address that is never dereferenced: every call below fails before its launch
    cases = [
        (lambda: lib.stc_upconv_expand(one, 0, 4, one, None), b"stc_upconv_expand: channels"),
        (lambda: lib.stc_upconv_expand(one, 4, -1, one, None), b"stc_upconv_expand: channels"),
        (lambda: lib.stc_upconv_expand(None, 4, 4, one, None), b"stc_upconv_expand: null pointer"),
        (lambda: lib.stc_upconv_expand(one, 4, 4, None, None), b"stc_upconv_expand: null pointer"),
        (lambda: lib.stc_upconv_wgrad_collapse(one, 0, 4, one, None), b"stc_upconv_wgrad_collapse: channels"),
        (lambda: lib.stc_upconv_wgrad_collapse(one, 4, 0, one, None), b"stc_upconv_wgrad_collapse: channels"),
        (lambda: lib.stc_upconv_wgrad_collapse(None, 4, 4, one, None), b"stc_upconv_wgrad_collapse: null pointer"),
        (lambda: lib.stc_upconv_wgrad_collapse(one, 4, 4, None, None), b"stc_upconv_wgrad_collapse: null pointer"),
        (lambda: lib.stc_pack_weight(0, 7, one, 4, 4, one, 16, 8, None), b"stc_pack_weight: bad mode"),
        (lambda: lib.stc_pack_weight(0, -1, one, 4, 4, one, 16, 8, None), b"stc_pack_weight: bad mode"),
        (lambda: lib.stc_pack_weight(0, 5, one, 0, 4, one, 16, 8, None), b"stc_pack_weight: channels"),
        (lambda: lib.stc_pack_weight(1, 6, one, 4, -3, one, 16, 8, None), b"stc_pack_weight: channels"),
        (lambda: lib.stc_pack_weight(0, 5, None, 4, 4, one, 16, 8, None), b"stc_pack_weight: null pointer"),
        (lambda: lib.stc_pack_weight(0, 6, one, 4, 4, None, 16, 8, None), b"stc_pack_weight: null pointer"),
        (lambda: lib.stc_pack_weight(0, 5, one, 40, 4, one, 16, 8, None), b"stc_pack_weight: padded extent"),
    ]
    for call, msg in cases:
        assert call() != 0
        assert msg in lib.stc_last_error(), (msg, lib.stc_last_error())
    for mode, P, Q, W, out, msg in [(7, 4, 4, one, one, b"bad desc 1"), (5, 0, 4, one, one, b"bad desc 1 (channels)"),
                                    (6, 4, 4, None, one, b"bad desc 1"), (5, 4, 4, one, None, b"bad desc 1"),
                                    (6, 40, 4, one, one, b"bad desc 1 (padding)")]:
        descs = (_lib.PackDesc * 2)(_lib.PackDesc(3, 4, 4, 16, 8, 0, one, one),
                                    _lib.PackDesc(mode, P, Q, 16, 8, 0, W, out))
        assert lib.stc_pack_weights(0, 2, descs, None) != 0
        assert msg in lib.stc_last_error(), (msg, lib.stc_last_error())
    with pytest.raises(RuntimeError, match="null pointer"):
        _lib.check(lib.stc_upconv_expand(None, 1, 1, None, None), "stc_upconv_expand")


def test_export_helper_refuses_other_shapes():
    from stcgan_amd import networks
    with pytest.raises(ValueError, match="3, 3"):
        networks.upconv_to_conv_t(torch.zeros(4, 4, 4, 4))
    with pytest.raises(RuntimeError, match="GPU only"):
        networks.upconv_to_conv_t(torch.zeros(4, 4, 3, 3))
