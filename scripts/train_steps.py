"""K bf16 bs=32 256^2 train steps (the bench workload) and nothing else: the command profiled by
scripts/gpu_steps.sh, so per-step kernel totals are the rocprof totals / (K + W)."""
import argparse
import json
import os
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "shadow-removal-istd_amd"))
import torch  # noqa: E402

from stcgan_amd import engine  # noqa: E402
from stcgan_amd.stcgan import STCGAN  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=4)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--dtype", default="bf16")
ap.add_argument("--streams", type=int, default=1)
ap.add_argument("--fused", type=int, default=1)
ap.add_argument("--host-sleep-us", type=int, default=0, help="extra host time per step (host-boundness probe)")
ap.add_argument("--repeat", type=int, default=1)
ap.add_argument("--wgrad-overlap", type=int, default=1)
ap.add_argument("--ab", default="", help="comma list of wgrad-overlap settings cycled per repeat (same process)")
ap.add_argument("--ab-attr", default="", help="name=v1,v2: trainer attribute (int) cycled per repeat (same process)")
ap.add_argument("--ab-plans", default="", help="JSON list of {name, conv: [[key..., cfg, ks]], wgrad: [[key..., cfg, "
                "splits]]} plan-override settings cycled per repeat (same process)")
ap.add_argument("--use-dropout", type=int, default=0, help="1: generators with use_dropout=True (p = --droprate)")
ap.add_argument("--droprate", type=float, default=0.5)
ap.add_argument("--ab-dropout", action="store_true", help="a second trainer with use_dropout=True; the two are "
                "timed alternately, one per repeat (same process)")
ap.add_argument("--nn-upconv", type=int, default=0, help="1: generators with Upsample + Conv2d(3) up layers "
                "(args.NN_upconv)")
ap.add_argument("--ab-upconv", action="store_true", help="a second trainer with NN_upconv=True; the two are timed "
                "alternately, one per repeat (same process)")
ap.add_argument("--activation", default="tanh", help="the generators' output head: none, sigmoid, tanh, htanh "
                "(args.activation)")
ap.add_argument("--ab-activation", default="", help="a second trainer with this output head; the two are timed "
                "alternately, one per repeat (same process)")
ap.add_argument("--padding-mode", default="zeros", help="the padding mode of every 4x4 conv of all four networks: "
                "zeros, reflect (args.padding_mode)")
args = ap.parse_args()
engine.WGRAD_OVERLAP = args.wgrad_overlap > 0
if args.wgrad_overlap > 1:
    engine.WGRAD_OVERLAP_MAX_PIX = args.wgrad_overlap
a = types.SimpleNamespace(devices=["cuda:0"], tasks=["train"], lr_G=5e-5, lr_D=2e-5, beta1=0.5, beta2=0.999,
                          D_loss_fn="standard", D_loss_type="normal", ngf=64, dtype=args.dtype, load_weights_g1=None,
                          load_weights_g2=None, load_weights_d1=None, load_weights_d2=None,
                          streams=bool(args.streams), fused_objectives=bool(args.fused),
                          use_dropout=bool(args.use_dropout), droprate=args.droprate, NN_upconv=bool(args.nn_upconv),
                          activation=args.activation, padding_mode=args.padding_mode)
torch.manual_seed(1234)
tr = STCGAN(a)
drop_trs = None
if args.ab_dropout:
    a_d = types.SimpleNamespace(**{**vars(a), "use_dropout": True})
    drop_trs = [tr, STCGAN(a_d)]
elif args.ab_upconv:
    drop_trs = [tr, STCGAN(types.SimpleNamespace(**{**vars(a), "NN_upconv": True}))]
elif args.ab_activation:
    drop_trs = [tr, STCGAN(types.SimpleNamespace(**{**vars(a), "activation": args.ab_activation}))]
import stcgan_amd.stcgan as _st  # noqa: E402


def _slowed(step):
    def _slow(*aa, **kk):
        t_end = time.perf_counter() + args.host_sleep_us * 1e-6
        while time.perf_counter() < t_end:
            pass
        return step(*aa, **kk)
    return _slow


for t_ in drop_trs or [tr]:  # (every trainer: --ab-dropout / --ab-upconv switch between two)
    t_.set_early = lambda v: setattr(_st, "EARLY_D_BACKWARD", int(v))  # (--ab-attr early=0,1,2)
    t_.set_late = lambda v: setattr(_st, "LATE_STATS_CALLS", bool(v))  # (--ab-attr late=0,1)
    if args.host_sleep_us:
        t_.train_step = _slowed(t_.train_step)
dev = torch.device("cuda", 0)
B = 32
x = torch.rand((B, 3, 256, 256), device=dev) * 2 - 1
m = (torch.rand((B, 1, 256, 256), device=dev) < 0.5).float() * 2 - 1
y = torch.rand((B, 3, 256, 256), device=dev) * 2 - 1
for _ in range(args.warmup):
    tr.train_step(x, m, y)
torch.cuda.synchronize()
ab = [int(v) for v in args.ab.split(",")] if args.ab else None
plans = json.loads(args.ab_plans) if args.ab_plans else None
res = {}
drop_label = (f"use_dropout={args.use_dropout}" + (f", NN_upconv={args.nn_upconv}" if args.nn_upconv else "")
              + (f", padding_mode={args.padding_mode}" if args.padding_mode != "zeros" else ""))
attr = None
if args.ab_attr:
    an, av = args.ab_attr.split("=")
    attr = (an, [int(v) for v in av.split(",")])
for rep in range(args.repeat):
    if drop_trs:
        tr = drop_trs[rep % 2]
        drop_label = (f"NN_upconv={rep % 2}" if args.ab_upconv else
                      f"activation={(args.activation, args.ab_activation)[rep % 2]}" if args.ab_activation else
                      f"use_dropout={rep % 2}")
        for _ in range(2):
            tr.train_step(x, m, y)
        torch.cuda.synchronize()
    if attr:
        v = attr[1][rep % len(attr[1])]
        setter = getattr(tr, "set_" + attr[0], None)
        if setter is not None:
            setter(v)
        else:
            setattr(tr, attr[0], type(getattr(tr, attr[0]))(v))
        args.wgrad_overlap = f"{attr[0]}={v}"
        for _ in range(2):
            tr.train_step(x, m, y)
        torch.cuda.synchronize()
    if plans:
        from stcgan_amd import ops
        pl = plans[rep % len(plans)]
        ops.FORCE_CONV.clear()
        ops.FORCE_WGRAD.clear()
        for e in pl.get("conv", []):
            ops.FORCE_CONV[tuple(e[:6])] = tuple(e[6:8])
        for e in pl.get("wgrad", []):
            ops.FORCE_WGRAD[tuple(e[:5])] = tuple(e[5:7])
        args.wgrad_overlap = pl["name"]
        for _ in range(2):
            tr.train_step(x, m, y)
        torch.cuda.synchronize()
    if ab:
        o = ab[rep % len(ab)]
        engine.WGRAD_OVERLAP = o > 0
        engine.WGRAD_OVERLAP_MAX_PIX = o if o > 1 else 1 << 30
        args.wgrad_overlap = o
        for _ in range(2):
            tr.train_step(x, m, y)
        torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        tr.train_step(x, m, y)
    torch.cuda.synchronize()
    print(f"{(time.perf_counter() - t0) / args.steps * 1e3:.3f} ms/step  mem {torch.cuda.memory_allocated() / 2**30:.2f} GiB "
          f"reserved {torch.cuda.memory_reserved() / 2**30:.2f} GiB ({args.steps} steps, streams={args.streams}, "
          f"fused={args.fused}, wgrad_overlap={args.wgrad_overlap}, {drop_label})", flush=True)
    res.setdefault((args.wgrad_overlap, drop_label), []).append((time.perf_counter() - t0) / args.steps * 1e3)
if ab or plans or attr or drop_trs:
    for (k, dl), v in res.items():
        print(f"wgrad_overlap={k}, {dl}: median {sorted(v)[len(v) // 2]:.3f} ms/step over {len(v)}", flush=True)
