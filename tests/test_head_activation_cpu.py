"""The generator's output head (get_generator(activation=...), args.activation) without a GPU: the module tree and the
state_dict keys for the four values, the refusals at construction and at plan time, the trainer's validation, the
composition with no_conv_t, the new C-ABI symbol and its argument validation (nothing is launched), and the exact
operand generators of tests/head_ref.py."""
import ctypes

import pytest
import torch
import torch.nn as nn

import head_ref as R

HEAD_TYPES = {"tanh": nn.Tanh, "sigmoid": nn.Sigmoid, "htanh": nn.Hardtanh}


@pytest.mark.parametrize("no_conv_t", [False, True], ids=["conv_t", "upconv"])
@pytest.mark.parametrize("act", R.HEADS)
def test_tree_and_keys(act, no_conv_t, monkeypatch):
    from stcgan_amd import engine, networks
    import upconv_ref as U
    # (the weight expansion is a HIP kernel; its numpy restatement stands in for it here: only the keys are looked at)
    monkeypatch.setattr(networks, "upconv_to_conv_t", U.expand_t)
    base = networks.get_generator(4, 3, ngf=8, no_conv_t=no_conv_t)
    net = networks.get_generator(4, 3, ngf=8, no_conv_t=no_conv_t, activation=act)
    assert net.activation == act and base.activation == "tanh"
    sd, bd = net.state_dict(), base.state_dict()
    assert list(sd) == list(bd) and all(tuple(sd[k].shape) == tuple(bd[k].shape) for k in sd)
    base.load_state_dict(sd)  # strict: checkpoints load across heads
    outer = net.model.model
    assert len(outer) == (4 if act == "none" else 5)
    assert isinstance(outer[0], nn.Conv2d) and isinstance(outer[2], nn.ReLU)
    assert isinstance(outer[3], nn.Sequential if no_conv_t else nn.ConvTranspose2d)
    if act != "none":
        assert type(outer[4]) is HEAD_TYPES[act] and type(outer[4]) is type(R.head_module(act))
        assert not list(outer[4].parameters()) and not list(outer[4].buffers())
    if act == "htanh":
        assert (outer[4].min_val, outer[4].max_val, outer[4].inplace) == (-1.0, 1.0, True)
    # no other block changes
    inner = [m for m in net.modules() if isinstance(m, networks.UnetSkipConnectionBlock) and not m.outermost]
    assert not any(isinstance(q, (nn.Tanh, nn.Sigmoid, nn.Hardtanh)) for m in inner for q in m.model.children())
    plan = engine.GenPlan(net)
    assert plan.head == act and plan.upconv == no_conv_t and engine.GenPlan(base).head == "tanh"
    # conv_t_state_dict() is unaffected by the head
    if no_conv_t:
        assert list(net.conv_t_state_dict()) == list(base.conv_t_state_dict())
        plain = networks.get_generator(4, 3, ngf=8, activation=act)
        assert list(net.conv_t_state_dict()) == list(plain.state_dict())


def test_none_is_the_string_none():
    from stcgan_amd import engine, networks
    a = networks.get_generator(3, 1, ngf=8, activation=None)
    b = networks.UnetGenerator(3, 1, ngf=8, activation="none")
    assert a.activation == b.activation == "none"
    assert len(a.model.model) == len(b.model.model) == 4
    assert [type(m) for m in a.modules()] == [type(m) for m in b.modules()]
    assert engine.GenPlan(a).head == engine.GenPlan(b).head == "none"


@pytest.mark.parametrize("bad", ["relu", "Tanh", "", 1, True, b"tanh"])
def test_unknown_activation_is_a_value_error(bad):
    from stcgan_amd import networks
    with pytest.raises(ValueError, match="'none', 'sigmoid', 'tanh', 'htanh'"):
        networks.get_generator(3, 1, ngf=8, activation=bad)


@pytest.mark.parametrize("swap", [nn.ReLU(), nn.Hardtanh(-2.0, 2.0), nn.Hardtanh(0.0, 1.0), nn.Softsign()],
                         ids=["relu", "htanh2", "htanh01", "softsign"])
def test_swapped_head_is_refused_at_plan_time(swap):
    from stcgan_amd import engine, networks
    net = networks.get_generator(3, 1, ngf=8)
    net.model.model[4] = swap
    with pytest.raises(NotImplementedError, match=r"model\.model\.4") as e:
        engine.GenPlan(net)
    assert type(swap).__name__ in str(e.value)
    # a second module behind the head is no head either
    net = networks.get_generator(3, 1, ngf=8)
    net.model.model.append(nn.Tanh())
    with pytest.raises(NotImplementedError, match=r"model\.model"):
        engine.GenPlan(net)
    # the supported modules, swapped in by hand, are read as what they are
    net = networks.get_generator(3, 1, ngf=8)
    net.model.model[4] = nn.Sigmoid()
    assert engine.GenPlan(net).head == "sigmoid"
    net.model.model[4] = nn.Hardtanh()
    assert engine.GenPlan(net).head == "htanh"
    del net.model.model[4]
    assert engine.GenPlan(net).head == "none"


def test_check_activation():
    from stcgan_amd import networks
    from stcgan_amd.stcgan import check_activation
    for v in R.HEADS:
        assert check_activation(v) == v and networks.check_activation(v) == v
    assert networks.check_activation(None) == "none"
    for bad in ("relu", None, 0, False, "TANH"):
        with pytest.raises(ValueError, match="'none', 'sigmoid', 'tanh'"):
            check_activation(bad)


def test_trainer_reads_the_option_through_that_checker():
    """STCGAN.__init__ validates args.activation (default "tanh") and hands it to both generators (read from the source:
    the constructor needs a GPU)."""
    import inspect
    from stcgan_amd import stcgan
    src = inspect.getsource(stcgan.STCGAN.__init__)
    assert 'check_activation(getattr(args, "activation", "tanh"))' in src
    assert src.count("**up)") == 2 and 'up["activation"] = self.activation' in src


def test_symbol_bound_and_arguments_validated():
    from stcgan_amd import _lib
    assert "stc_head_bwd" in _lib.EXPORTED and "stc_tanh_bias_bwd" in _lib.EXPORTED
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "stc_head_bwd")
    assert (_lib.HEAD_NONE, _lib.HEAD_TANH, _lib.HEAD_SIGMOID, _lib.HEAD_HTANH) == (0, 1, 2, 3)
    assert _lib.HEADS == R.CODES
    lib = _lib.lib()
    v = _lib.View(None, 4, 4, 0, 0, 4, 0, 1, 0)
    for act in (-1, 4, 7):
        rc = lib.stc_head_bwd(0, act, 1, 3, 4, 4, None, None, v, None, None, 1, None)
        assert rc != 0 and b"stc_head_bwd: act=" in lib.stc_last_error()
    rc = lib.stc_head_bwd(0, 2, 1, 5, 4, 4, None, None, v, None, None, 1, None)
    assert rc != 0 and b"C=5" in lib.stc_last_error()
    # the conv epilogue code: validated before anything else of the call
    x = _lib.View(None, 4, 4, 0, 0, 4, 0, 1, 0)
    for code in (-1, 4):
        rc = lib.stc_conv_fwd(0, 2, 1, x, 4, None, None, 0, 0.0, None, 3, x, None, code, 1, None, 0, None)
        assert rc != 0 and b"epilogue code" in lib.stc_last_error()
        rc = lib.stc_conv_fwd_ex(0, 2, 1, x, 4, None, 3, x, None, code, 1, None, 0, None, None, 0, None)
        assert rc != 0 and b"epilogue code" in lib.stc_last_error()


def test_head_code():
    from stcgan_amd import _lib
    assert [_lib.head_code(a) for a in R.HEADS] == [0, 1, 2, 3] and _lib.head_code(None) == 0
    with pytest.raises(ValueError, match="activation must be"):
        _lib.head_code("relu")


# ---------------------------------------------------------------- the reference's own properties
@pytest.mark.parametrize("act", R.HEADS)
def test_operands_are_exact(act):
    y, gy = R.operands(act, 3, 4, 10, 12, 5)
    dq, db = R.head_bwd_ref(act, y, gy)
    assert torch.equal(dq.to(torch.float32).double(), dq)
    R.require_exact(dq, 3 * 10 * 12)
    if act != "tanh":  # the torch fp32 form in the documented order gives the exact values
        assert torch.equal(R.dq_torch(act, y.float(), gy.float()).double(), dq)
    if act == "htanh":
        at = (y.abs() == 1)
        assert bool(at.any()) and bool((dq[at] == 0).all()) and torch.equal(dq[~at], gy[~at])
    if act == "none":
        assert torch.equal(dq, gy)
    assert torch.equal(db, dq.sum(dim=(0, 2, 3)))


@pytest.mark.parametrize("act", R.HEADS)
def test_derivative_matches_autograd(act):
    q = (torch.randn(4000, generator=torch.Generator().manual_seed(3), dtype=torch.float64) * 2).requires_grad_(True)
    y = R.head(act, q)
    y.sum().backward()
    assert float((q.grad - R.dhead(act, y.detach())).abs().max()) <= 1e-12
    mod = R.head_module(act)
    want = q.detach().clone() if mod is None else mod(q.detach().clone())
    assert float((y.detach() - want).abs().max()) <= 1e-15
