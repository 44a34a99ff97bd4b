"""Plain torch.nn restatement of the two ST-CGAN networks with a free ``norm_layer`` (helper of the
instance-norm tests; not a test module).  Same Sequential layout as the pix2pix-family constructors, so the
``state_dict`` keys are what those give; the generator's forward pads a copy at odd sizes and crops the
up-path output, with the norm of the up path running over the full ConvT extent before the crop."""
import torch
import torch.nn as nn
import torch.nn.functional as F

PLANES = [(1, 2), (2, 2), (3, 3), (8, 8), (5, 13), (31, 31), (64, 64), (17, 241), (127, 129)]


class RefBlock(nn.Module):
    def __init__(self, outer_nc, inner_nc, input_nc=None, submodule=None, outermost=False, innermost=False,
                 norm_layer=nn.BatchNorm2d):
        super().__init__()
        self.outermost, self.innermost = outermost, innermost
        input_nc = outer_nc if input_nc is None else input_nc
        down = nn.Conv2d(input_nc, inner_nc, 4, 2, 1, bias=False)
        if outermost:
            layers = [down, submodule, nn.ReLU(), nn.ConvTranspose2d(inner_nc * 2, outer_nc, 4, 2, 1), nn.Tanh()]
        elif innermost:
            layers = [nn.LeakyReLU(0.2), down, nn.ReLU(), nn.ConvTranspose2d(inner_nc, outer_nc, 4, 2, 1, bias=False),
                      norm_layer(outer_nc)]
        else:
            layers = [nn.LeakyReLU(0.2), down, norm_layer(inner_nc), submodule, nn.ReLU(),
                      nn.ConvTranspose2d(inner_nc * 2, outer_nc, 4, 2, 1, bias=False), norm_layer(outer_nc)]
        self.model = nn.Sequential(*layers)

    def forward(self, x):
        m = self.model
        if self.outermost:
            return torch.tanh(m[3](F.relu(m[1](m[0](x)))))
        h, w = x.shape[2], x.shape[3]
        odd = (h % 2) or (w % 2)
        a = F.leaky_relu(F.pad(x, (0, w % 2, 0, h % 2)) if odd else x, 0.2)
        d = m[1](a)
        if self.innermost:
            u = m[4](m[3](F.relu(d)))
        else:
            u = m[6](m[5](F.relu(m[3](m[2](d)))))
        if odd:
            u = u[:, :, :h, :w]
        return torch.cat([x if odd else a, u], 1)


class RefG(nn.Module):
    def __init__(self, in_c, out_c, ngf=64, num_downs=8, norm_layer=nn.BatchNorm2d):
        super().__init__()
        blk = RefBlock(ngf * 8, ngf * 8, innermost=True, norm_layer=norm_layer)
        for _ in range(num_downs - 5):
            blk = RefBlock(ngf * 8, ngf * 8, submodule=blk, norm_layer=norm_layer)
        for mult in (4, 2, 1):
            blk = RefBlock(ngf * mult, ngf * mult * 2, submodule=blk, norm_layer=norm_layer)
        self.model = RefBlock(out_c, ngf, input_nc=in_c, submodule=blk, outermost=True, norm_layer=norm_layer)

    def forward(self, x):
        return self.model(x)


class RefD(nn.Module):
    def __init__(self, in_c, ndf=64, n_layers=3, norm_layer=nn.BatchNorm2d):
        super().__init__()
        seq = [nn.Conv2d(in_c, ndf, 4, 2, 1), nn.LeakyReLU(0.2)]
        mult = 1
        for n in range(1, n_layers + 1):
            prev, mult = mult, min(2 ** n, 8)
            seq += [nn.Conv2d(ndf * prev, ndf * mult, 4, 2 if n < n_layers else 1, 1, bias=False),
                    norm_layer(ndf * mult), nn.LeakyReLU(0.2)]
        seq += [nn.Conv2d(ndf * mult, 1, 4, 1, 1)]
        self.model = nn.Sequential(*seq)

    def forward(self, x):
        return self.model(x)


def randomise_affine(net, seed):
    """Affine norm parameters away from (1, 0), so that a missing multiply or add shows."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, (nn.InstanceNorm2d, nn.BatchNorm2d)) and m.weight is not None:
                m.weight.copy_(torch.rand(m.weight.shape, generator=g) + 0.5)
                m.bias.copy_(torch.rand(m.bias.shape, generator=g) - 0.5)


def activation_inputs(ref):
    """The modules of a RefG / RefD whose output feeds a ReLU / LeakyReLU: every norm, and the convs without one."""
    mods = []
    for m in ref.modules():
        if isinstance(m, RefBlock):
            if m.outermost:
                mods.append(m.model[0])
            elif m.innermost:
                mods += [m.model[1], m.model[4]]
            else:
                mods += [m.model[2], m.model[6]]
        elif isinstance(m, RefD):
            mods += [m.model[0]] + [q for q in m.model if isinstance(q, (nn.InstanceNorm2d, nn.BatchNorm2d))]
    return mods


def sign_margin(make_ref, x):
    """How far the reference's activation decisions are from fp32 rounding, from the reference alone: the smallest
    |n| / e over every activation input n of the fp64 forward, e the larger of that element's |fp32 - fp64|
    difference and the rms of that difference over its tensor (a torch.nn fp32 forward of the same network).
    A seed whose margin is small puts some ReLU decision inside fp32 rounding: the gradient of ANY fp32
    implementation then differs from fp64 by that element's whole contribution, which no tolerance covers."""
    rec = {}
    for dt in (torch.float64, torch.float32):
        ref = make_ref().to(dt)
        outs = []
        for mod in activation_inputs(ref):
            mod.register_forward_hook(lambda _m, _i, o, outs=outs: outs.append(o.detach().double()))
        with torch.no_grad():
            ref.train()(x.to(dt))
        rec[dt] = outs
    margin = float("inf")
    for a, b in zip(rec[torch.float64], rec[torch.float32]):
        d = (a - b).abs()
        e = torch.maximum(d, d.pow(2).mean().sqrt().expand_as(d)).clamp_min(1e-30)
        margin = min(margin, float((a.abs() / e).min()))
    return margin
