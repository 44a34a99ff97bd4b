"""Instance norm without a GPU: module trees, refusals, the host queries and the argument validation of stc_in_*."""
import ctypes
import functools

import pytest
import torch
import torch.nn as nn

from inorm_ref import PLANES, RefD, RefG

AFFINE = functools.partial(nn.InstanceNorm2d, affine=True)
NORMS = [pytest.param(nn.InstanceNorm2d, id="plain"), pytest.param(AFFINE, id="affine")]


def _same_tree(net, ref):
    sd, rd = net.state_dict(), ref.state_dict()
    assert list(sd) == list(rd)
    assert all(tuple(sd[k].shape) == tuple(rd[k].shape) for k in sd)
    return sd


@pytest.mark.parametrize("norm", NORMS)
@pytest.mark.parametrize("in_c,out_c", [(3, 1), (4, 3)])
@pytest.mark.parametrize("ngf", [8, 64])
def test_generator_tree(norm, in_c, out_c, ngf):
    from stcgan_amd import networks
    sd = _same_tree(networks.get_generator(in_c, out_c, ngf=ngf, norm_layer=norm), RefG(in_c, out_c, ngf, 8, norm))
    assert not [k for k in sd if "running_" in k or "num_batches_tracked" in k]
    if norm is nn.InstanceNorm2d:
        assert len(sd) == 17  # the conv weights and the outermost ConvT bias
    else:
        assert len(sd) == 17 + 2 * 13 and "model.model.1.model.2.weight" in sd and "model.model.1.model.6.bias" in sd


@pytest.mark.parametrize("norm", NORMS)
@pytest.mark.parametrize("in_c", [4, 7])
def test_discriminator_tree(norm, in_c):
    from stcgan_amd import networks
    sd = _same_tree(networks.get_discriminator(in_c, ndf=8, norm_layer=norm), RefD(in_c, 8, 3, norm))
    assert not [k for k in sd if "running_" in k or "num_batches_tracked" in k]
    assert len(sd) == (7 if norm is nn.InstanceNorm2d else 13)


def test_eps_partial_and_use_bias():
    from stcgan_amd import engine, networks
    net = networks.get_generator(3, 1, ngf=8, norm_layer=functools.partial(nn.InstanceNorm2d, eps=1e-3, affine=True))
    plan = engine.GenPlan(net)
    assert plan.inorm and plan.affine and all(m.eps == 1e-3 for m in plan.bnu.values())
    assert all(m.bias is None for m in plan.conv) and plan.convT[1].bias is None  # use_bias stays False
    d = engine.DiscPlan(networks.get_discriminator(4, ndf=8, norm_layer=nn.InstanceNorm2d))
    assert d.inorm and not d.affine and len(d.bns) == 3


def test_refusals():
    from stcgan_amd import networks
    with pytest.raises(NotImplementedError, match="track_running_stats"):
        networks.get_generator(3, 1, ngf=8, norm_layer=functools.partial(nn.InstanceNorm2d, track_running_stats=True))
    with pytest.raises(NotImplementedError, match="track_running_stats"):
        networks.get_discriminator(4, ndf=8, norm_layer=functools.partial(nn.InstanceNorm2d, track_running_stats=True))
    with pytest.raises(NotImplementedError, match="GroupNorm"):
        networks.get_generator(3, 1, ngf=8, norm_layer=functools.partial(nn.GroupNorm, 2))
    with pytest.raises(NotImplementedError, match="LayerNorm"):
        networks.get_discriminator(4, ndf=8, norm_layer=nn.LayerNorm)
    with pytest.raises(NotImplementedError, match="use_dropout"):
        networks.get_generator(3, 1, ngf=8, norm_layer=nn.InstanceNorm2d, use_dropout=True)
    with pytest.raises(NotImplementedError, match="use_sigmoid"):
        networks.get_discriminator(4, ndf=8, norm_layer=nn.InstanceNorm2d, use_sigmoid=True)


def test_batchnorm_tree_unchanged():
    from oracle import stcgan_ref as ref
    from stcgan_amd import engine, networks
    g = networks.get_generator(4, 3, ngf=8, norm_layer=nn.BatchNorm2d)
    assert list(g.state_dict()) == list(ref.generator_state_template(4, 3, 8))
    _same_tree(g, RefG(4, 3, 8, 8, nn.BatchNorm2d))
    d = networks.get_discriminator(7, ndf=8, norm_layer=nn.BatchNorm2d)
    assert list(d.state_dict()) == list(ref.discriminator_state_template(7, 8))
    assert not engine.GenPlan(g).inorm and not engine.DiscPlan(d).inorm


def _plan(lib, dt, B, H, W, C):
    out = (ctypes.c_int32 * 4)()
    assert lib.stc_in_plan(dt, B, H, W, C, out) == 0, lib.stc_last_error()
    return tuple(out)


@pytest.mark.parametrize("dt,vec", [(0, 4), (1, 8)])
def test_plan_and_workspace(dt, vec):
    from stcgan_amd import _lib
    lib = _lib.lib()
    seen = {}
    for H, W in PLANES:
        for cv in (1, 3, 64):
            for B in (1, 3):
                regime, slab, chunks, m = _plan(lib, dt, B, H, W, cv * vec)
                assert regime in (0, 1, 2) and slab % vec == 0 and vec <= slab and chunks >= 1 and m >= 1
                assert (chunks > 1) == (regime == 2)
                ws = lib.stc_in_workspace(dt, B, H, W, cv * vec)
                assert ws >= 0 and (regime != 2 or ws >= B * chunks * cv * vec * 8)
                seen.setdefault(regime, (H, W))
    assert sorted(seen) == [0, 1, 2], seen
    assert _plan(lib, dt, 3, 2, 2, 64 * vec)[0] == 0 and _plan(lib, dt, 3, 127, 129, 64 * vec)[0] == 2
    assert lib.stc_in_workspace(dt, 3, 127, 129, 64 * vec) > 0


def test_invalid_arguments_fail_without_gpu():
    from stcgan_amd import _lib
    lib = _lib.lib()
    N = _lib.NULL_VIEW

    def view(H, W, C):
        return _lib.View(None, H, W, H * W * C, W * C, C, 0, 1, 0)

    out = (ctypes.c_int32 * 4)()
    assert lib.stc_in_plan(0, 2, 4, 4, 3, out) != 0 and b"C=3" in lib.stc_last_error()
    v = view(4, 4, 3)
    rc = lib.stc_in_fwd(0, 2, v, 3, None, None, 1e-5, None, None, v, v, 0.0, N, 0.0, None, 0, None)
    assert rc != 0 and b"C=3" in lib.stc_last_error()
    with pytest.raises(RuntimeError, match="C=3"):
        _lib.check(rc, "stc_in_fwd")
    rc = lib.stc_in_bwd(1, 2, v, 12, None, None, None, None, v, 0.0, N, 0.0, v, None, None, None, 0, None)
    assert rc != 0 and b"C=12" in lib.stc_last_error()
    v = view(1, 1, 64)
    for call in (lambda: lib.stc_in_fwd(0, 2, v, 64, None, None, 1e-5, None, None, v, v, 0.0, N, 0.0, None, 0, None),
                 lambda: lib.stc_in_bwd(0, 2, v, 64, None, None, None, None, v, 0.0, N, 0.0, v, None, None, None, 0,
                                        None),
                 lambda: lib.stc_in_plan(1, 2, 1, 1, 64, out)):
        lib.stc_in_plan(0, 2, 4, 4, 3, out)  # another message in between
        assert call() != 0
        assert b"more than 1 spatial element" in lib.stc_last_error()
        assert b"[2, 64, 1, 1]" in lib.stc_last_error()
    assert lib.stc_in_workspace(0, 2, 1, 1, 64) < 0
    # a streamed shape without its workspace: refused before any launch (the views are checked first, so give
    # 16-byte aligned dummies that are never dereferenced)
    buf = torch.zeros(4)
    v = view(127, 129, 8)
    v.p = (buf.data_ptr() + 15) // 16 * 16
    rc = lib.stc_in_fwd(0, 1, v, 8, None, None, 1e-5, ctypes.c_void_p(buf.data_ptr()),
                        ctypes.c_void_p(buf.data_ptr()), v, v, 0.0, N, 0.0, None, 0, None)
    assert rc != 0 and b"workspace" in lib.stc_last_error()
