"""Both networks with padding_mode="reflect" on the GPU against the fp64 torch.nn restatement of the same module tree
(tests/reflect_ref.py) on the CPU: ngf = ndf = 8, batch 2, 256 x 256, G (4 -> 3 channels) and D (7 channels).

fp32 with the project's model tolerances (tests/test_gpu_model.py; taken from there, not chosen here): output atol
1e-4; input gradient atol 2e-5, rtol 2e-3; parameter gradients atol 2e-4 * max|g| + 1e-6, rtol 2e-3; buffers atol 1e-5,
rtol 1e-4.  bf16 outputs within the stated 2e-2 max-abs of the same reference.

Seeds.  The project's rule: the first weight seed whose fp64 reference keeps every activation input at least 8 of its
own fp32 errors from zero (inorm_ref.sign_margin: a property of the reference alone, searched on the CPU by
scripts/pick_reflect_test_seeds.py and asserted again here).  SEEDS records each configuration's seed and margin.

The combined case (use_dropout, no_conv_t, activation="sigmoid") draws its train-mode masks from the generator's own
counter-based function, restated in numpy by tests/test_dropout_cpu.py: the reference multiplies by the same masks.

Odd levels.  A generator input with an odd level raises NotImplementedError at call time, naming the level (the
behaviour this project chose; networks.py docstring); an extent-1 plane raises RuntimeError as torch does."""
import functools

import pytest
import torch
import torch.nn as nn

import reflect_ref as P
from fixture_init import normal, uniform
from inorm_ref import randomise_affine, sign_margin
from test_dropout_cpu import dropout_mask as np_mask

DEV = "cuda"
MARGIN = 8.0
AFFINE = functools.partial(nn.InstanceNorm2d, affine=True)
NORMS = {"batch": nn.BatchNorm2d, "affine": AFFINE}
DROP_SEED, DROP_OFFSET = 0x5EED, 3
# (network, norm, combined options): the configurations of this file
CONFIGS = [("G", "batch", False), ("G", "affine", False), ("D", "batch", False), ("D", "affine", False),
           ("G", "batch", True)]
COMBINED = dict(use_dropout=True, no_conv_t=True, activation="sigmoid")
# configuration -> (seed, its sign_margin), from scripts/pick_reflect_test_seeds.py
SEEDS = {("G", "batch", False): (12, 8.32), ("G", "affine", False): (35, 9.28), ("D", "batch", False): (5, 13.45),
         ("D", "affine", False): (3, 8.91), ("G", "batch", True): (46, 8.21)}
SHAPE = {"G": (2, 4, 256, 256), "D": (2, 7, 256, 256)}


def masks_for(B, H, W, ngf=8, nd=8):
    """{level: NCHW fp64 keep / (1 - p)} of the generator call at {DROP_SEED, DROP_OFFSET}: levels 4 .. 6, p = 0.5."""
    out = {}
    for k in range(4, nd - 1):
        fh, fw = H >> k, W >> k
        m = np_mask(DROP_SEED, DROP_OFFSET, k, (B, fh, fw, ngf * 8), 0.5)
        out[k] = torch.from_numpy(m.astype("float64")).permute(0, 3, 1, 2) / 0.5
    return out


def make(cfg, seed):
    """(the project's network on the CPU, a maker of fresh fp32 restatements loaded with its state, the input)."""
    from stcgan_amd import networks
    kind, norm, combined = cfg
    kw = COMBINED if combined else {}
    if kind == "G":
        net = networks.get_generator(4, 3, ngf=8, norm_layer=NORMS[norm], padding_mode="reflect", **kw)
    else:
        net = networks.get_discriminator(7, ndf=8, norm_layer=NORMS[norm], padding_mode="reflect")
    torch.manual_seed(seed)
    net.apply(networks.weights_init)
    randomise_affine(net, seed + 100)
    sd = {k: v.clone() for k, v in net.state_dict().items()}
    x = uniform(SHAPE[kind], 44)

    def fresh():
        if kind == "G":
            m = P.ReflectG(4, 3, 8, 8, norm_layer=NORMS[norm], **kw)
            if combined:
                m.set_masks(masks_for(x.shape[0], x.shape[2], x.shape[3]))
        else:
            m = P.ReflectD(7, 8, 3, norm_layer=NORMS[norm])
        m.load_state_dict(sd)
        return m

    return net, fresh, x


@functools.lru_cache(maxsize=None)
def reference(cfg):
    """Once per configuration: (net, x, r, fresh, fp64 train output, input gradient, parameter gradients, buffers after
    the train forward, fp64 eval output of the untouched state, frozen output / input gradient / parameter gradients)."""
    seed, recorded = SEEDS[cfg]
    net, fresh, x = make(cfg, seed)
    margin = sign_margin(fresh, x)
    assert margin >= MARGIN, f"seed of {cfg}: an activation decision within fp32 rounding ({margin:.2f})"
    assert abs(margin - recorded) <= 0.05 * recorded, (cfg, margin, recorded)
    out = {}
    for mode in ("train", "eval", "frozen"):
        ref = fresh().double()
        ref.train(mode == "train")
        if mode != "train" and cfg[0] == "G" and cfg[2]:
            ref.set_masks(None)  # (dropout is off outside train mode; "frozen" keeps it on: below)
        if mode == "frozen":  # the network in train mode (dropout active), its norm layers on running statistics
            ref.train()
            for m in ref.modules():
                if isinstance(m, (nn.BatchNorm2d, nn.InstanceNorm2d)):
                    m.eval()
            if cfg[0] == "G" and cfg[2]:
                ref.set_masks(masks_for(x.shape[0], x.shape[2], x.shape[3]))
        x64 = x.double().requires_grad_(True)
        y = ref(x64)
        r = normal(tuple(y.shape), 45)
        (y * r.double()).sum().backward()
        out[mode] = (y.detach(), x64.grad.clone(), {k: p.grad.clone() for k, p in ref.named_parameters()},
                     {k: b.detach().clone() for k, b in ref.named_buffers()})
    return net, x, r, out


def run(net, x, r, mode, combined):
    for p in net.parameters():
        p.grad = None
    net.train(mode != "eval")
    if mode == "frozen":
        net.freeze_norm()
    if combined:
        net.set_dropout_seed(DROP_SEED, DROP_OFFSET)
    xg = x.clone().requires_grad_(True)
    out = net(xg)
    (out * r).sum().backward()
    torch.cuda.synchronize()
    return out.detach(), xg.grad


def close(what, got, want, atol, rtol, fails):
    err = (got.detach().cpu().double() - want).abs()
    ratio = float((err / (atol + rtol * want.abs())).max())
    print(f"[reflect_model] {what}: max err {float(err.max()):.3e}, error/bound {ratio:.3f}")
    if not ratio <= 1.0:
        fails.append(f"{what}: max err {float(err.max()):.3e}, error/bound {ratio:.3f}")


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["train", "eval", "frozen"])
@pytest.mark.parametrize("cfg", CONFIGS, ids=lambda c: f"{c[0]}-{c[1]}" + ("-combined" if c[2] else ""))
def test_parity_fp32(cfg, mode):
    net, x, r, ref = reference(cfg)
    sd0 = {k: v.clone() for k, v in net.state_dict().items()}
    try:
        net.to(DEV).set_compute_dtype("fp32")
        out, gx = run(net, x.to(DEV), r.to(DEV), mode, cfg[2])
        y_ref, gx_ref, grads, bufs = ref[mode]
        tag = f"{cfg} {mode}"
        fails = []
        close(f"{tag} output", out, y_ref, 1e-4, 0.0, fails)
        close(f"{tag} input grad", gx, gx_ref, 2e-5, 2e-3, fails)
        params = dict(net.named_parameters())
        assert set(params) == set(grads)
        for k, g in grads.items():
            close(f"{tag} grad {k}", params[k].grad, g, 2e-4 * float(g.abs().max()) + 1e-6, 2e-3, fails)
        for k, b in net.named_buffers():
            close(f"{tag} buffer {k}", b, bufs[k].double(), 1e-5, 1e-4, fails)
        assert not fails, fails
    finally:
        net.cpu().load_state_dict(sd0)  # (the shared network: its running statistics back where they were)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["train", "eval", "frozen"])
@pytest.mark.parametrize("cfg", CONFIGS, ids=lambda c: f"{c[0]}-{c[1]}" + ("-combined" if c[2] else ""))
def test_bf16_output(cfg, mode):
    net, x, r, ref = reference(cfg)
    sd0 = {k: v.clone() for k, v in net.state_dict().items()}
    try:
        net.to(DEV).set_compute_dtype("bf16")
        out, gx = run(net, x.to(DEV), r.to(DEV), mode, cfg[2])
        err = float((out.cpu().double() - ref[mode][0]).abs().max())
        print(f"[reflect_model] {cfg} {mode} bf16 output max-abs {err:.3e}")
        assert err <= 2e-2 and bool(torch.isfinite(gx).all())
    finally:
        net.cpu().load_state_dict(sd0)
        net.set_compute_dtype("fp32")


def fwd_bwd(net, x, r):
    for p in net.parameters():
        p.grad = None
    xg = x.clone().requires_grad_(True)
    out = net(xg)
    (out * r).sum().backward()
    torch.cuda.synchronize()
    return out.detach(), xg.grad, {k: p.grad.clone() for k, p in net.named_parameters()}, \
        {k: b.clone() for k, b in net.named_buffers()}


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("kind", ["G", "D"])
def test_zeros_keyword_is_the_default_network(kind, dtype):
    """padding_mode="zeros" and no keyword at all: bit-identical outputs, gradients and buffers."""
    from stcgan_amd import networks
    nets = []
    for kw in ({}, dict(padding_mode="zeros")):
        n = networks.get_generator(4, 3, ngf=8, **kw) if kind == "G" else networks.get_discriminator(7, ndf=8, **kw)
        torch.manual_seed(11)
        n.apply(networks.weights_init)
        nets.append(n.to(DEV).set_compute_dtype(dtype).train())
    x = uniform(SHAPE[kind], 46).to(DEV)
    r = normal((2, 3, 256, 256) if kind == "G" else (2, 1, 30, 30), 47).to(DEV)
    a, b = fwd_bwd(nets[0], x, r), fwd_bwd(nets[1], x, r)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    for i in (2, 3):
        assert set(a[i]) == set(b[i]) and all(torch.equal(a[i][k], b[i][k]) for k in a[i]), i


@pytest.mark.gpu
def test_extent_one_plane_raises():
    """8 levels over 128 x 128: the innermost conv would reflect a 1 x 1 plane -- torch's refusal, before any launch
    of that call leaves garbage behind; the discriminator's last conv over a 1-high plane likewise."""
    from stcgan_amd import networks
    g = networks.get_generator(4, 3, ngf=8, padding_mode="reflect").to(DEV)
    with pytest.raises(RuntimeError, match="Padding size should be less than the corresponding input dimension"):
        g(torch.zeros(1, 4, 128, 128, device=DEV))
    d = networks.get_discriminator(7, ndf=8, padding_mode="reflect").to(DEV)
    with pytest.raises(RuntimeError, match="Padding size should be less than the corresponding input dimension"):
        d(torch.zeros(1, 7, 16, 64, device=DEV))  # 16 -> 8 -> 4 -> 2 -> 1 rows: the logits conv reads a 1-high plane
    with pytest.raises(RuntimeError, match="Padding size should be less than the corresponding input dimension"):
        P.ReflectD(7, 8)(torch.zeros(1, 7, 16, 64))  # (and so does torch on the same tree)


@pytest.mark.gpu
def test_odd_level_raises_not_implemented():
    """The behaviour chosen for a generator input with an odd level: NotImplementedError at call time naming the
    level; the zeros network takes the same input."""
    from stcgan_amd import networks
    g = networks.get_generator(4, 3, ngf=8, num_downs=6, padding_mode="reflect").to(DEV)
    x = torch.zeros(1, 4, 72, 64, device=DEV)  # 72 -> 36 -> 18 -> 9: level 3 reads an odd plane
    with pytest.raises(NotImplementedError, match=r"level 3 .*odd 9 x 8"):
        g(x)
    assert g(torch.zeros(1, 4, 64, 64, device=DEV)).shape == (1, 3, 64, 64)
    z = networks.get_generator(4, 3, ngf=8, num_downs=6).to(DEV)
    assert z(x).shape == (1, 3, 72, 64)


ODD_SHAPE = (2, 7, 62, 70)  # stride-2 planes 62 x 70, 31 x 35 (odd), 15 x 17 (odd); stride-1 planes 7 x 8 and 6 x 7
ODD_SEED = (1, 15.19)  # (seed, sign_margin) by the rule of SEEDS, for the BatchNorm discriminator on ODD_SHAPE


def make_odd(seed):
    from stcgan_amd import networks
    net = networks.get_discriminator(7, ndf=8, padding_mode="reflect")
    torch.manual_seed(seed)
    net.apply(networks.weights_init)
    randomise_affine(net, seed + 100)
    sd = {k: v.clone() for k, v in net.state_dict().items()}

    def fresh():
        m = P.ReflectD(7, 8, 3)
        m.load_state_dict(sd)
        return m

    return net, fresh, uniform(ODD_SHAPE, 48)


@pytest.mark.gpu
def test_discriminator_odd_extents_follow_torch():
    """The discriminator follows torch for every extent >= 2: a 62 x 70 input, whose second and third stride-2 convs
    read odd planes (31 x 35, 15 x 17), against the fp64 restatement -- output, input gradient, parameter gradients and
    buffers of a train-mode step with the tolerances of test_parity_fp32; bf16 output within 2e-2.  (The zero-padded
    discriminator keeps refusing odd stride-2 planes.)"""
    from stcgan_amd import networks
    seed, recorded = ODD_SEED
    net, fresh, x = make_odd(seed)
    margin = sign_margin(fresh, x)
    assert margin >= MARGIN and abs(margin - recorded) <= 0.05 * recorded, (margin, recorded)
    ref = fresh().double().train()
    x64 = x.double().requires_grad_(True)
    y = ref(x64)
    assert tuple(y.shape) == (2, 1, 5, 6)
    r = normal(tuple(y.shape), 49)
    (y * r.double()).sum().backward()
    net.to(DEV).set_compute_dtype("fp32")
    out, gx = run(net, x.to(DEV), r.to(DEV), "train", False)
    fails = []
    close("D odd output", out, y.detach(), 1e-4, 0.0, fails)
    close("D odd input grad", gx, x64.grad, 2e-5, 2e-3, fails)
    params = dict(net.named_parameters())
    for k, p in ref.named_parameters():
        close(f"D odd grad {k}", params[k].grad, p.grad, 2e-4 * float(p.grad.abs().max()) + 1e-6, 2e-3, fails)
    for k, b in ref.named_buffers():
        close(f"D odd buffer {k}", dict(net.named_buffers())[k], b.double(), 1e-5, 1e-4, fails)
    assert not fails, fails
    net.load_state_dict(fresh().state_dict())
    net.set_compute_dtype("bf16")
    out16, gx16 = run(net, x.to(DEV), r.to(DEV), "train", False)
    assert float((out16.cpu().double() - y.detach()).abs().max()) <= 2e-2 and bool(torch.isfinite(gx16).all())
    z = networks.get_discriminator(7, ndf=8).to(DEV)
    with pytest.raises(AssertionError, match="even sizes"):
        z(x.to(DEV))
