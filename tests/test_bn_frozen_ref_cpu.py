"""The frozen-statistics BatchNorm reference (tests/bn_frozen_ref.py) against torch.autograd, and the host-side
pieces of the feature that need no GPU: freeze_norm(), the mixed-mode refusal, args.freeze_norm."""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import bn_frozen_ref as R

EPS = 1e-5


def _case(shape, seed):
    B, H, W, C = shape
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(shape, generator=g) * 2 + 0.5).double()
    gam = (torch.rand(C, generator=g) + 0.5).double()
    gam[1::3] *= -1.0
    bet = (torch.randn(C, generator=g) * 0.3).double()
    rm = (torch.randn(C, generator=g) * 0.5).double()
    rv = (torch.rand(C, generator=g) * 2 + 0.1).double()
    g1 = torch.randn(shape, generator=g).double()
    g2 = torch.randn(shape, generator=g).double()
    return x, gam, bet, rm, rv, g1, g2


@pytest.mark.parametrize("two,s1,s2", [(False, 0.0, 0.0), (True, 0.0, 0.2), (False, 0.2, 0.0), (True, 0.2, 0.0)])
@pytest.mark.parametrize("shape", [(2, 3, 5, 4), (3, 9, 8, 12), (1, 1, 1, 8)])
def test_reference_matches_autograd(shape, two, s1, s2):
    """dx, dgamma, dbeta and the forward of the restated formulas equal fp64 autograd through
    F.batch_norm(training=False) + relu / leaky_relu to 1e-12 relative; the buffers handed to torch do not move."""
    x, gam, bet, rm, rv, g1, g2 = _case(shape, 7 + shape[3])
    xr = x.permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    gr, br = gam.clone().requires_grad_(True), bet.clone().requires_grad_(True)
    rm0, rv0 = rm.clone(), rv.clone()
    n = F.batch_norm(xr, rm, rv, gr, br, False, 0.1, EPS)
    assert torch.equal(rm, rm0) and torch.equal(rv, rv0)

    def act(v, s):
        return F.relu(v) if s == 0.0 else F.leaky_relu(v, R.slope32(s))

    out = (act(n, s1) * g1.permute(0, 3, 1, 2)).sum()
    if two:
        out = out + (act(n, s2) * g2.permute(0, 3, 1, 2)).sum()
    gx, gg, gb = torch.autograd.grad(out, (xr, gr, br))
    scale, shift, rstd = R.tables(gam, bet, rm, rv, EPS)
    ref = R.backward(x, scale, shift, rm, rstd, g1, s1, g2 if two else None, s2)

    def close(a, b, what):
        err = float((a - b).abs().max())
        lim = 1e-12 * max(1.0, float(b.abs().max()))
        assert err <= lim, (what, err, lim)

    close(ref["n"], n.detach().permute(0, 2, 3, 1), "n")
    close(ref["dx"], gx.permute(0, 2, 3, 1), "dx")
    close(ref["dgamma"], gg, "dgamma")
    close(ref["dbeta"], gb, "dbeta")
    # the chunked sums add up to the whole ones
    val, _ = R.chunk_sums(ref, 3)
    close(val[..., 0].sum(0), gb, "chunks dbeta")
    close(val[..., 1].sum(0), gg, "chunks dgamma")


def test_reference_dropout_factor_is_a_scaled_gradient():
    """The dropout factor multiplies g1 only: the reference with a factor equals the reference fed g1 * factor."""
    shape = (2, 3, 5, 8)
    x, gam, bet, rm, rv, g1, g2 = _case(shape, 3)
    scale, shift, rstd = R.tables(gam, bet, rm, rv, EPS)
    f = R.drop_factor(0x1234ABCD5678, 7, 5, (2, 4, 6, 8), (3, 5), 0.2)
    assert tuple(f.shape) == shape and set(f.unique().tolist()) == {0.0, float(R.scale32(0.2))}
    a = R.backward(x, scale, shift, rm, rstd, g1, 0.0, g2, 0.2, factor=f)
    b = R.backward(x, scale, shift, rm, rstd, g1 * f, 0.0, g2, 0.2)
    for k in ("dx", "dgamma", "dbeta"):
        assert torch.equal(a[k], b[k]), k


def _nets():
    from stcgan_amd import networks
    return [networks.get_generator(3, 1, ngf=8, num_downs=6, use_dropout=True),
            networks.get_discriminator(4, ndf=8),
            networks.get_generator(3, 1, ngf=8, num_downs=6, norm_layer=nn.InstanceNorm2d)]


def _modes(net):
    return {n: m.training for n, m in net.named_modules()}


def test_freeze_norm_flips_exactly_the_norm_children():
    for net in _nets():
        net.train()
        before = _modes(net)
        assert net.freeze_norm() is net
        after = _modes(net)
        norms = {n for n, m in net.named_modules() if isinstance(m, (nn.BatchNorm2d, nn.InstanceNorm2d))}
        assert norms and {n for n in before if before[n] != after[n]} == norms
        assert not any(after[n] for n in norms) and net.training
        assert any(isinstance(m, nn.Dropout) and m.training for m in net.modules()) or net.kind == "D" \
            or net.norm_kind == "instance"
        net.freeze_norm()  # idempotent
        assert _modes(net) == after
        net.freeze_norm(False)  # back to the net's own mode
        assert _modes(net) == before
        net.eval()
        ev = _modes(net)
        net.freeze_norm(False)
        assert _modes(net) == ev
        net.freeze_norm()
        assert _modes(net) == ev
        net.train()  # torch's rule: .train() resets every child
        assert _modes(net) == before


def test_flags_follow_the_modules():
    g, d, gi = _nets()
    for net in (g, d):
        assert net.train()._batch_stats() is True
        assert net.freeze_norm()._batch_stats() is False and net.training
        assert net.freeze_norm(False)._batch_stats() is True
        assert net.eval()._batch_stats() is False
    # instance norm: one mode, the flag follows the net and nothing reads it
    assert gi.train().freeze_norm()._batch_stats() is True and gi.eval()._batch_stats() is False


def test_mixed_modes_raise_and_name_the_layers():
    g, d, _ = _nets()
    for net, x in ((g, torch.zeros(1, 3, 64, 64)), (d, torch.zeros(1, 4, 64, 64))):
        net.train()
        bns = [(n, m) for n, m in net.named_modules() if isinstance(m, nn.BatchNorm2d)]
        bns[0][1].eval()
        with pytest.raises(NotImplementedError) as ei:
            net(x)
        msg = str(ei.value)
        assert all(n in msg for n, _ in bns) and "mixed" in msg


def test_args_freeze_norm_values():
    from stcgan_amd.stcgan import check_freeze_norm
    assert check_freeze_norm(False) is False and check_freeze_norm(True) is True
    assert check_freeze_norm(0) is False and check_freeze_norm(1) is True
    for bad in ("yes", 2, None, 0.5, [True]):
        with pytest.raises(ValueError, match="freeze_norm"):
            check_freeze_norm(bad)
