"""What stcgan_amd.engine asks of the library, as text -- and, with --gpu, what comes back, as digests.

Default (no GPU): every public function of stcgan_amd.ops is replaced by a recorder that returns a correctly shaped
stand-in, GradWriter.dest / done / flush and _WgradLane.run are wrapped, and gen_forward / gen_backward /
disc_forward / disc_backward are called directly on CPU tensors over a matrix of networks, norm modes, dtypes and
call options.  One line per call: the callee and every argument, bound to the callee's signature (so a positional
and a keyword spelling of the same call are the same line).  Views print as V(H,W,bs,rs,ps,co,cs,null?), tensors as
shape and dtype, modules / parameters / buffers by their state_dict name; views and tensors also carry the ordinal
of the buffer they refer to (#n, in order of first appearance within the case), never an address.  Two trees whose
engines enqueue the same work write the same bytes.

  python scripts/engine_call_log.py --out full.log --digest digests.txt [--tree OTHER_CHECKOUT]

--digest writes one line per case (name, lines, sha256 of the case's log) -- the full log is tens of MB.
--coverage prints how many cases reached each norm-backward callee (the arms of the engine's backward step).

--gpu: no stubs.  The networks of tests/test_gpu_eval_backward.py (its builders, fixture weights and input seeds; ngf 8,
batch 2; 480 x 640 at batch 1) run forward + backward on the device through the public modules, and one sha256 per
output, source gradient, parameter gradient and norm buffer is written.  One fresh process per tree; compare the files.
"""
import argparse
import functools
import hashlib
import inspect
import os
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                help="root of the checkout whose engine is run (default: this one)")
ap.add_argument("--out", default=None, help="the full log (CPU mode) or the digest list (--gpu)")
ap.add_argument("--digest", default=None, help="CPU mode: one sha256 per case")
ap.add_argument("--coverage", action="store_true")
ap.add_argument("--gpu", action="store_true")
args = ap.parse_args()
TREE = os.path.abspath(args.tree)
for p in ("tests", os.path.join("tests", "golden"), "shadow-removal-istd_amd", ""):
    sys.path.insert(0, os.path.join(TREE, p))

import torch  # noqa: E402
import torch.nn as nn  # noqa: E402

from stcgan_amd import _lib as L  # noqa: E402
from stcgan_amd import engine, networks, ops  # noqa: E402

IN_AFFINE = functools.partial(nn.InstanceNorm2d, affine=True)
# mode: (norm_layer, use_dropout, train, batch_stats)
MODES = {
    "bn-train": (nn.BatchNorm2d, False, True, True),
    "bn-frozen": (nn.BatchNorm2d, False, True, False),
    "bn-eval": (nn.BatchNorm2d, False, False, False),
    "drop-train": (nn.BatchNorm2d, True, True, True),
    "drop-frozen": (nn.BatchNorm2d, True, True, False),
    "in": (nn.InstanceNorm2d, False, True, True),
    "in-affine": (IN_AFFINE, False, True, True),
}
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16}
NETS = {"G3to1": ("G", (3,), 1), "G4to3": ("G", (3, 1), 3), "D4": ("D", (3, 1), 1), "D7": ("D", (3, 1, 3), 1)}


def make(net, mode):
    kind, src_c, cout = NETS[net]
    norm, drop = MODES[mode][:2]
    if kind == "G":
        return networks.get_generator(sum(src_c), cout, ngf=8, norm_layer=norm, use_dropout=drop)
    return networks.get_discriminator(sum(src_c), ndf=8, norm_layer=norm)


# ----------------------------------------------------------------------------- CPU: the call log
LOG = []
_labels, _alive = {}, []


def _key(t):
    if t.numel() == 0:
        return ("z", id(t))
    return (t.untyped_storage().data_ptr(), t.storage_offset(), tuple(t.shape), tuple(t.stride()), t.dtype)


def _label(t, name=None):
    """The name of tensor ``t``: as given here, else the ordinal of its first appearance in this case."""
    k = _key(t)
    if name is not None:
        _labels[k] = name
    elif k not in _labels:
        _labels[k] = f"#{sum(v.startswith('#') for v in _labels.values())}"
    _alive.append(t)  # (no address is reused within a case)
    return _labels[k]


def _new_case(net):
    LOG.clear()
    _labels.clear()
    _alive.clear()
    for n, p in net.named_parameters():
        _label(p, "P:" + n)
    for n, b in net.named_buffers():
        _label(b, "B:" + n)
    return {id(m): "M:" + n for n, m in net.named_modules()}


_modules = {}


def fmt(a):
    if a is None or isinstance(a, (bool, int, float, str)):
        return repr(a)
    if isinstance(a, L.View):
        keep = getattr(a, "_keep", None)
        return (f"V({a.H},{a.W},{a.bs},{a.rs},{a.ps},{a.co},{a.cs},{'null' if not a.p else 'set'})"
                + ("" if keep is None else _label(keep)))
    if isinstance(a, torch.Tensor):
        return f"T({list(a.shape)},{str(a.dtype)[6:]}){_label(a)}"
    if isinstance(a, nn.Module):
        return _modules.get(id(a), "M?" + type(a).__name__)
    if isinstance(a, (list, tuple)):
        o, c = "[]" if isinstance(a, list) else "()"
        return o + ",".join(fmt(x) for x in a) + c
    if isinstance(a, dict):
        return "dict"
    if isinstance(a, (torch.dtype, torch.device)):
        return str(a)
    if callable(a):
        return "fn"
    return type(a).__name__


def record(name, sig, a, k, skip=0):
    b = sig.bind(*a, **k)
    b.apply_defaults()
    LOG.append(name + " " + " ".join(f"{n}={fmt(v)}" for n, v in list(b.arguments.items())[skip:]))


ANSWER = {"conv_act": True, "conv_act_backward": True}


def _z(*shape, dtype=torch.float32):
    return torch.zeros(shape, dtype=dtype)


def _wgrad_ret(B, stride, Dv, R, Gv, Cg, Cg_out, dt, dpro=None, dslope=None, gpro=None, gslope=None, device=None,
               force=None, rows=None, rows_kernel=None, out=None):
    return out if out is not None else _z(rows or R, Cg_out, 4, 4)


STUBS = dict(
    gather=None, scatter=None, conv=None, bn_apply=None, bn_eval_table=None, refresh_packs=None, chan_sum=None,
    grad_accumulate=None, tanh_bias_bwd=None,
    packed=lambda cache, W, mode, n_pad, c_pad, dt: _z(1),
    conv_act=lambda *a, **k: ANSWER["conv_act"],
    conv_act_backward=lambda *a, **k: ANSWER["conv_act_backward"],
    conv_bn_act=lambda kind, B, xv, cin, w, cout, *a, **k: (_z(2, cout), (_z(cout), _z(cout))),
    conv_stats=lambda *a, **k: (_z(1), 1),
    bn_finalize_part=lambda part, nch, C, *a, **k: (_z(C), _z(C)),
    bn_running_rstd=lambda C, bn, out=None: _z(C),
    in_forward=lambda B, xv, C, *a, **k: (_z(B, C), _z(B, C)),
    dropout_next=lambda state: _z(2, dtype=torch.int64),
    wgrad=_wgrad_ret,
    conv_bn_backward=(None, None), bn_backward=(None, None), bn_backward_frozen=(None, None), in_backward=(None, None),
)
# no library call behind them: recorded, and answered by the function itself (the last two are reached through
# the generator's _dropout_tensor)
PURE = ("vec", "pad_channels", "dropout_rank_seed", "dropout_state_tensor")


def install_stubs():
    def recorder(name, orig, ret):
        sig = inspect.signature(orig)

        def g(*a, **k):
            record(name, sig, a, k)
            return ret(*a, **k) if callable(ret) else ret
        return g

    for name, f in list(vars(ops).items()):
        if not (inspect.isfunction(f) and not name.startswith("_") and f.__module__ == ops.__name__):
            continue
        if name in STUBS:
            setattr(ops, name, recorder(name, f, STUBS[name]))
        elif name in PURE:
            setattr(ops, name, recorder(name, f, f))
        else:  # not a function the engine has any business calling
            setattr(ops, name, functools.partial(_unexpected, name))

    def method(cls, name, after=None):
        orig = getattr(cls, name)
        sig = inspect.signature(orig)

        def g(self, *a, **k):
            record(cls.__name__ + "." + name, sig, (self,) + a, k, skip=1)
            r = orig(self, *a, **k)
            if after is not None:
                after(self, r, *a, **k)
            return r
        setattr(cls, name, g)

    def dest_done(self, r, p):
        fresh = r is p.grad
        LOG[-1] += " -> " + ("view" if fresh else "scratch")
        _label(r, ("G:" if fresh else "S:") + _labels[_key(p)][2:])

    method(engine.GradWriter, "dest", dest_done)
    method(engine.GradWriter, "done")
    method(engine.GradWriter, "flush")
    method(engine._WgradLane, "run")
    engine.WGRAD_OVERLAP = False

    class _NoStream:  # (_ones_plane synchronises the current stream after its one fill)
        def synchronize(self):
            pass
    torch.cuda.current_stream = lambda dev=None: _NoStream()


def _unexpected(name, *a, **k):
    raise AssertionError(f"the engine called ops.{name}, which this script has no stand-in for")


def run_cpu(tag, net_name, mode, dt, hw=(256, 256), need_w=True, src="all", trace=False, answer=True, save=True,
            stats_only=False, defer=False, inputs=False, twice=False):
    global _modules
    kind, src_c, _ = NETS[net_name]
    _, _, train, batch_stats = MODES[mode]
    net = make(net_name, mode)
    _modules = _new_case(net)
    plan = engine.GenPlan(net) if kind == "G" else engine.DiscPlan(net)
    sources = [torch.zeros(1, c, *hw) for c in src_c]
    need_src = {"all": [True] * len(src_c), "some": [i == 0 for i in range(len(src_c))], "none": None}[src]
    ANSWER["conv_act"] = ANSWER["conv_act_backward"] = answer
    engine.TRACE = {} if trace else None
    engine._ONES.clear()
    cache, cached_inputs = {}, ({} if inputs else None)
    try:
        for _ in range(2 if twice else 1):
            if kind == "G":
                y, saved = engine.gen_forward(plan, sources, train, dt, cache, save, batch_stats)
            else:
                y, saved = engine.disc_forward(plan, sources, train, dt, cache, save, cached_inputs, stats_only,
                                               [] if defer else None, batch_stats)
                if inputs:  # the second call of the trainer's pair: the gathered input is reused
                    engine.disc_forward(plan, sources, train, dt, cache, False, cached_inputs, stats_only, None,
                                        batch_stats)
            LOG.append("-- forward done; saved " + ("None" if saved is None else ",".join(sorted(saved))))
            if saved is None:
                continue
            W = engine.GradWriter(net) if need_w else None
            bwd = engine.gen_backward if kind == "G" else engine.disc_backward
            grads = bwd(plan, saved, torch.zeros_like(y), dt, cache, need_src, W)
            if W is not None:
                W.flush()
            LOG.append("-- backward done; source grads " + fmt(grads))
    finally:
        engine.TRACE = None
    return tag, list(LOG)


def cpu_cases():
    for net in NETS:
        kind = NETS[net][0]
        modes = [m for m in MODES if kind == "G" or not m.startswith("drop")]
        for dn, dt in DTYPES.items():
            for mode in modes:
                for need_w in (True, False):
                    base = f"{net}/{dn}/{mode}/{'w' if need_w else 'now'}"
                    yield base, dict(net_name=net, mode=mode, dt=dt, need_w=need_w)
                    if net in ("G3to1", "D7"):
                        continue
                    # one option at a time, on the second network of each kind
                    var = dict(net_name=net, mode=mode, dt=dt, need_w=need_w)
                    yield base + "/fallback", dict(var, answer=False)
                    yield base + "/trace", dict(var, trace=True)
                    yield base + "/src-some", dict(var, src="some")
                    if need_w:
                        yield base + "/src-none", dict(var, src="none")
                        yield base + "/nosave", dict(var, save=False)
                    if kind == "G":
                        yield base + "/480x640", dict(var, hw=(480, 640))
                        yield base + "/480x640/fallback/src-some", dict(var, hw=(480, 640), answer=False, src="some")
                        # S[1] odd: the level-0 activation backward cannot take the conv epilogue
                        yield base + "/250x254", dict(var, hw=(250, 254))
                    else:
                        yield base + "/stats-only", dict(var, stats_only=True, save=False)
                        yield base + "/stats-only-saved", dict(var, stats_only=True)
                        yield base + "/defer", dict(var, defer=True)
                        yield base + "/inputs", dict(var, inputs=True)
                        if need_w:
                            yield base + "/twice", dict(var, twice=True)
                            yield base + "/twice/fallback/trace", dict(var, twice=True, answer=False, trace=True)


ARMS = ("conv_act_backward", "bn_backward ", "in_backward", "bn_backward_frozen", "conv_bn_backward", "conv_bn_act",
        "in_forward", "bn_eval_table", "conv_act ")


def main_cpu():
    torch.manual_seed(0)  # (a use_dropout generator's first seed is torch.initial_seed())
    install_stubs()
    out = open(args.out, "w") if args.out else None
    dig = open(args.digest, "w") if args.digest else None
    reach = {a: 0 for a in ARMS}
    reach.update({"bn_backward drop": 0, "bn_backward no-norm": 0, "bn_backward_frozen drop": 0})
    n = 0
    for tag, kw in cpu_cases():
        _, lines = run_cpu(tag, **kw)
        text = "".join(f"{tag}: {ln}\n" for ln in lines)
        if out:
            out.write(text)
        if dig:
            dig.write(f"{tag} {len(lines)} {hashlib.sha256(text.encode()).hexdigest()}\n")
        for a in ARMS:
            reach[a] += any(ln.startswith(a) for ln in lines)
        reach["bn_backward drop"] += any(ln.startswith("bn_backward ") and "drop=(" in ln for ln in lines)
        reach["bn_backward no-norm"] += any(ln.startswith("bn_backward ") and "bn_state=None" in ln for ln in lines)
        reach["bn_backward_frozen drop"] += any(ln.startswith("bn_backward_frozen") and "drop=(" in ln for ln in lines)
        n += 1
    print(f"{n} cases")
    if args.coverage:
        for a, c in reach.items():
            print(f"{c:5d} cases reach {a.strip()}")


# ----------------------------------------------------------------------------- GPU: digests
def main_gpu():
    import test_gpu_eval_backward as T
    from fixture_init import fixture_state, normal, uniform
    dev = "cuda"
    out = open(args.out, "w") if args.out else sys.stdout
    n = [0]

    pending = []

    def emit(tag, name, t):
        pending.append((f"{tag} {name}", None if t is None else t.detach().reshape(-1).view(torch.uint8)))

    def flush():
        """One device-to-host copy for everything emitted since the last flush, then one sha256 each."""
        ts = [t for _, t in pending if t is not None]
        host = torch.cat(ts).cpu().numpy() if ts else None
        at = 0
        for label, t in pending:
            if t is None:
                out.write(f"{label} None\n")
            else:
                out.write(f"{label} {hashlib.sha256(host[at:at + t.numel()].tobytes()).hexdigest()[:20]}\n")
                at += t.numel()
        n[0] += len(pending)
        pending.clear()

    def build(case, mode):
        norm, drop = MODES[mode][:2]
        kw = dict(norm_layer=norm)
        if drop:
            kw["use_dropout"] = True
        if case == "G-4to3-480x640":
            net = networks.get_generator(4, 3, ngf=T.NGF, **kw)
            net.load_state_dict(fixture_state(net.state_dict(), 12, "one"))
            x = uniform((1, 4, 480, 640), 112)
        else:
            net, _ = T.make_net(case, **kw)
            x = T.case_input(case, T.X_SEED[case])
        if norm is IN_AFFINE:
            g = torch.Generator().manual_seed(5)
            with torch.no_grad():
                for m in net.modules():
                    if isinstance(m, nn.InstanceNorm2d):
                        m.weight.copy_(torch.rand(m.weight.shape, generator=g) + 0.5)
                        m.bias.copy_(torch.randn(m.bias.shape, generator=g) * 0.2)
        return net.to(dev), x.to(dev)

    def set_mode(net, mode):
        _, drop, train, batch_stats = MODES[mode]
        net.train() if train else net.eval()
        if train and not batch_stats:
            net.freeze_norm()
        if drop:
            net.set_dropout_seed(T.SEED, T.OFFSET)

    def split(case, x):
        c = x.shape[1]
        cuts = {3: (3,), 4: (3, 1), 7: (3, 1, 3)}[c]
        return [s.contiguous() for s in torch.split(x, cuts, 1)]

    def one(tag, net, srcs, need, r=None, zero=True, **attrs):
        if zero:
            net.zero_grad(set_to_none=True)
        xs = [s.detach().clone().requires_grad_(nd) for s, nd in zip(srcs, need)]
        for k, v in attrs.items():
            setattr(net, k, v)
        try:
            y = net(xs if len(xs) > 1 else xs[0])
        finally:
            for k in attrs:
                setattr(net, k, {"stats_only": False}.get(k))
        emit(tag, "out", y)
        if y.requires_grad:
            if r is None:
                r = normal(tuple(y.shape), 212).to(dev)
            (y * r).sum().backward()
        torch.cuda.synchronize()
        for i, s in enumerate(xs):
            emit(tag, f"src{i}.grad", s.grad)
        for k, p in net.named_parameters():
            emit(tag, k + ".grad", p.grad)
        for k, b in net.named_buffers():
            emit(tag, k, b)
        flush()

    small =["G-3to1-64", "G-4to3-64", "G-4to3-60x44", "D-4-64", "D-7-64"]
    big = ["G-4to3-256-full", "G-4to3-480x640"]
    for case in small + big:
        kind = case[0]
        for mode in MODES:
            if kind == "D" and mode.startswith("drop"):
                continue
            net, x = build(case, mode)
            srcs = split(case, x)
            for dn in DTYPES:
                net.set_compute_dtype(dn)
                tag = f"{case}/{dn}/{mode}"
                set_mode(net, mode)
                one(tag + "/w/src-all", net, srcs, [True] * len(srcs))
                if case in big:
                    continue
                for trace in (False, True):
                    engine.TRACE = {} if trace else None
                    try:
                        t2 = tag + ("/trace" if trace else "")
                        set_mode(net, mode)
                        one(t2 + "/w/src-some", net, srcs, [i == 0 for i in range(len(srcs))])
                        one(t2 + "/w/src-none", net, srcs, [False] * len(srcs))
                        net.requires_grad_(False)
                        one(t2 + "/now/src-all", net, srcs, [True] * len(srcs))
                        one(t2 + "/now/src-none", net, srcs, [False] * len(srcs))  # (nothing saved)
                        net.requires_grad_(True)
                    finally:
                        engine.TRACE = None
                if kind == "D":
                    set_mode(net, mode)
                    one(tag + "/stats-only", net, srcs, [False] * len(srcs), stats_only=True)
                    with torch.no_grad():
                        one(tag + "/stats-only-nograd", net, srcs, [False] * len(srcs), stats_only=True)
                    one(tag + "/inputs-1", net, srcs, [True] * len(srcs), input_cache={})
                    cache = {}
                    one(tag + "/twice-1", net, srcs, [True] * len(srcs), input_cache=cache)
                    one(tag + "/twice-2", net, srcs, [True] * len(srcs), zero=False, input_cache=cache)
                    if MODES[mode][3] and not mode.startswith("in"):
                        later = []
                        one(tag + "/defer", net, srcs, [True] * len(srcs), defer_running=later)
                        for ent in later:
                            ops.bn_running_update(*ent)
                        torch.cuda.synchronize()
                        for k, b in net.named_buffers():
                            emit(tag + "/defer-applied", k, b)
                        flush()
    print(f"{n[0]} digests")


if __name__ == "__main__":
    main_gpu() if args.gpu else main_cpu()
