"""optim.Adam / optim.AdamW take torch's weight_decay, decoupled_weight_decay and amsgrad: constructor, param_groups,
argument checks, state dicts exchanged with torch.optim in both directions, and the C-ABI's option validation
(all before any launch: no GPU)."""
import copy
import ctypes

import pytest
import torch

from stcgan_amd import _lib as L
from stcgan_amd.optim import Adam, AdamW


def _param(n=5, seed=0):
    return torch.nn.Parameter(torch.randn(n, generator=torch.Generator().manual_seed(seed)))


def _groups(opt):
    return [{k: v for k, v in g.items() if k != "params"} for g in opt.param_groups]


@pytest.mark.parametrize("ours,theirs,kw", [
    (Adam, torch.optim.Adam, dict(weight_decay=0.1)),
    (Adam, torch.optim.Adam, dict(amsgrad=True)),
    (Adam, torch.optim.Adam, dict(weight_decay=0.3, decoupled_weight_decay=True)),
    (Adam, torch.optim.Adam, dict()),
    (AdamW, torch.optim.AdamW, dict()),
    (AdamW, torch.optim.AdamW, dict(lr=2e-3, betas=(0.5, 0.99), weight_decay=0.25, amsgrad=True)),
])
def test_constructs_with_torchs_param_groups(ours, theirs, kw):
    a, b = ours([_param()], **kw), theirs([_param()], **kw)
    assert _groups(a) == _groups(b)
    assert issubclass(AdamW, Adam)


def test_adamw_defaults():
    g = AdamW([_param()]).param_groups[0]
    assert g["weight_decay"] == 1e-2 and g["decoupled_weight_decay"] is True and g["amsgrad"] is False


def test_ignored_and_refused_arguments():
    g = Adam([_param()], foreach=True, fused=False, capturable=True).param_groups[0]
    assert g["foreach"] is True and g["fused"] is False and g["capturable"] is True
    for cls in (Adam, AdamW):
        with pytest.raises(ValueError, match="weight_decay"):
            cls([_param()], weight_decay=-1e-3)
        with pytest.raises(NotImplementedError):
            cls([_param()], maximize=True)
        with pytest.raises(NotImplementedError):
            cls([_param()], differentiable=True)
    with pytest.raises(ValueError):
        Adam([_param()], lr=-1.0)
    with pytest.raises(ValueError):
        Adam([_param()], betas=(1.0, 0.999))
    with pytest.raises(ValueError):
        Adam([_param()], eps=-1e-8)


def test_per_group_options():
    opt = Adam([dict(params=[_param()], weight_decay=0.2), dict(params=[_param(3, 1)], amsgrad=True, lr=1e-4)],
               lr=5e-5, betas=(0.5, 0.999))
    g0, g1 = opt.param_groups
    assert (g0["weight_decay"], g0["amsgrad"], g0["lr"]) == (0.2, False, 5e-5)
    assert (g1["weight_decay"], g1["amsgrad"], g1["lr"]) == (0, True, 1e-4)
    o0, a0 = Adam._options(g0)
    assert (o0.weight_decay, o0.decoupled, o0.amsgrad, a0) == (0.2, 0, 0, False)
    o1, a1 = Adam._options(g1)
    assert (o1.weight_decay, o1.decoupled, o1.amsgrad, a1) == (0.0, 0, 1, True)
    # no decay to apply and no amsgrad: the calls without options, AdamW included
    assert Adam._options(Adam([_param()]).param_groups[0]) == (None, False)
    assert Adam._options(AdamW([_param()], weight_decay=0).param_groups[0]) == (None, False)
    g0["weight_decay"] = -0.5  # (set after construction: refused when the group steps)
    with pytest.raises(ValueError):
        Adam._options(g0)


def _torch_adamw_after_one_step():
    p = _param(7, 3)
    ref = torch.optim.AdamW([p], lr=2e-3, betas=(0.5, 0.99), weight_decay=0.05, amsgrad=True)
    p.grad = torch.randn(7, generator=torch.Generator().manual_seed(4))
    ref.step()
    return p, ref


def test_state_dict_from_torch_adamw_amsgrad_loads():
    p, ref = _torch_adamw_after_one_step()
    sd = ref.state_dict()
    q = torch.nn.Parameter(p.detach().clone())
    opt = AdamW([q])
    opt.load_state_dict(sd)
    g = opt.param_groups[0]
    assert g["amsgrad"] is True and g["decoupled_weight_decay"] is True and g["weight_decay"] == 0.05
    assert g["lr"] == 2e-3 and tuple(g["betas"]) == (0.5, 0.99)
    st, rst = opt.state[q], ref.state[p]
    assert set(st) == {"step", "exp_avg", "exp_avg_sq", "max_exp_avg_sq"}
    assert float(st["step"]) == 1.0
    for k in ("exp_avg", "exp_avg_sq", "max_exp_avg_sq"):
        assert torch.equal(st[k], rst[k])
    # a plain Adam of ours takes the same state: the options travel with the groups
    opt2 = Adam([torch.nn.Parameter(p.detach().clone())])
    opt2.load_state_dict(sd)
    assert Adam._options(opt2.param_groups[0])[0].decoupled == 1


def test_state_dict_loads_into_torch_and_steps():
    p, ref = _torch_adamw_after_one_step()
    q = torch.nn.Parameter(p.detach().clone())
    opt = AdamW([q], lr=2e-3, betas=(0.5, 0.99), weight_decay=0.05, amsgrad=True)
    opt.load_state_dict(copy.deepcopy(ref.state_dict()))
    sd = copy.deepcopy(opt.state_dict())  # ours, under torch's keys (a copy: torch's load aliases the tensors)
    assert set(sd["state"][0]) == {"step", "exp_avg", "exp_avg_sq", "max_exp_avg_sq"}
    assert set(sd["param_groups"][0]) == set(ref.state_dict()["param_groups"][0])
    r = torch.nn.Parameter(p.detach().clone())
    back = torch.optim.AdamW([r])
    back.load_state_dict(sd)
    g = torch.randn(7, generator=torch.Generator().manual_seed(5))
    p.grad, r.grad = g.clone(), g.clone()
    ref.step()
    back.step()  # torch runs on with our state dict exactly as with its own
    assert torch.equal(p.detach(), r.detach())
    assert torch.equal(ref.state[p]["max_exp_avg_sq"], back.state[r]["max_exp_avg_sq"])
    # and into torch.optim.Adam (decoupled_weight_decay travels in the group)
    back2 = torch.optim.Adam([torch.nn.Parameter(p.detach().clone())])
    back2.load_state_dict(sd)
    assert back2.param_groups[0]["decoupled_weight_decay"] is True


def test_load_keeps_the_moment_buffers():
    """load_state_dict copies into the buffers the state already holds (a captured graph and the pointer tables keep
    their addresses): max_exp_avg_sq as exp_avg / exp_avg_sq, and zeros where the loaded state has none."""
    p, ref = _torch_adamw_after_one_step()
    q = torch.nn.Parameter(p.detach().clone())
    opt = AdamW([q], amsgrad=True)
    opt.load_state_dict(ref.state_dict())
    held = {k: opt.state[q][k] for k in ("exp_avg", "exp_avg_sq", "max_exp_avg_sq")}
    sd = ref.state_dict()
    sd["state"][0] = {k: (v + 1 if k != "step" else v) for k, v in sd["state"][0].items()}
    opt.load_state_dict(sd)
    for k, t in held.items():
        assert opt.state[q][k] is t
        assert torch.equal(t, sd["state"][0][k])
    del sd["state"][0]["max_exp_avg_sq"]  # a state saved without it
    opt.load_state_dict(sd)
    assert opt.state[q]["max_exp_avg_sq"] is held["max_exp_avg_sq"]
    assert not opt.state[q]["max_exp_avg_sq"].any()


EX_CALLS = {
    # name: (arguments before opts, arguments after) -- valid enough to pass the other checks; nothing may launch
    "stc_adam_pack_step_ex": ((None, 1, 1, 1e-3, 0.9, 0.999, 1e-8, 1), (None,)),
    "stc_adam_pack_step_dev_ex": ((None, 1, 1, 8, 8, 8, 8, 4, 8, 0.9, 0.999, 1e-8), (None,)),
    "stc_adam_coef_dev_ex": ((8, 8, 8, 8, 4, 8), (None,)),
    "stc_adam_pack_apply_ex": ((None, 1, 1, 1e-3, 1, None, 0.9, 0.999, 1e-8), (None,)),
}


@pytest.mark.parametrize("name", sorted(EX_CALLS))
@pytest.mark.parametrize("bad,msg", [
    ((-0.5, 0, 0), b"weight_decay"),
    ((float("nan"), 0, 0), b"weight_decay"),
    ((0.1, 2, 0), b"decoupled"),
    ((0.1, -1, 0), b"decoupled"),
    ((0.0, 0, 3), b"amsgrad"),
])
def test_ex_calls_refuse_bad_options_before_any_launch(name, bad, msg):
    lib = L.lib()
    pre, post = EX_CALLS[name]
    opts = L.AdamOpts(*bad)
    rc = getattr(lib, name)(*pre, ctypes.byref(opts), *post)
    assert rc != 0
    err = lib.stc_last_error()
    assert msg in err and name.encode() in err, err
    with pytest.raises(RuntimeError, match=msg.decode()):
        L.check(rc, name)


def test_ex_symbols_are_bound():
    assert {"stc_adam_pack_step_ex", "stc_adam_pack_step_dev_ex", "stc_adam_coef_dev_ex",
            "stc_adam_pack_apply_ex"} <= set(L.EXPORTED)
    assert ctypes.sizeof(L.AdamOpts) == 16
