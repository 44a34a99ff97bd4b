"""The bench workload (bf16, bs=32, 256^2, ngf 64) with the optimiser options switched in one process: the default
update, coupled decay, decoupled decay and amsgrad in interleaved windows of --steps train steps, --repeat rounds.
Per option set: ms/step (host clock around the window) and the time of optim_G.step() / optim_D.step() on the GPU
(events around the call on its stream: the update launch -- one kernel per optimiser -- and nothing else).  The
options are group entries the optimiser reads at every eager step, so one trainer serves all four."""
import argparse
import os
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "shadow-removal-istd_amd"))
import torch  # noqa: E402

from stcgan_amd.stcgan import STCGAN  # noqa: E402

SETS = [("default", dict(weight_decay=0.0, decoupled_weight_decay=False, amsgrad=False)),
        ("coupled wd=1e-2", dict(weight_decay=1e-2, decoupled_weight_decay=False, amsgrad=False)),
        ("decoupled wd=1e-2", dict(weight_decay=1e-2, decoupled_weight_decay=True, amsgrad=False)),
        ("amsgrad", dict(weight_decay=0.0, decoupled_weight_decay=False, amsgrad=True))]

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--repeat", type=int, default=3)
args = ap.parse_args()
a = types.SimpleNamespace(devices=["cuda:0"], tasks=["train"], lr_G=5e-5, lr_D=2e-5, beta1=0.5, beta2=0.999,
                          D_loss_fn="standard", D_loss_type="normal", ngf=64, dtype="bf16", load_weights_g1=None,
                          load_weights_g2=None, load_weights_d1=None, load_weights_d2=None)
torch.manual_seed(1234)
tr = STCGAN(a)
dev = torch.device("cuda", 0)
B = 32
x = torch.rand((B, 3, 256, 256), device=dev) * 2 - 1
m = (torch.rand((B, 1, 256, 256), device=dev) < 0.5).float() * 2 - 1
y = torch.rand((B, 3, 256, 256), device=dev) * 2 - 1

events = {"G": [], "D": []}
for name, opt in (("G", tr.optim_G), ("D", tr.optim_D)):
    def timed(step=opt.step, log=events[name]):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = step()
        e1.record()
        log.append((e0, e1))
        return out
    opt.step = timed

for _ in range(args.warmup):
    tr.train_step(x, m, y)
torch.cuda.synchronize()
res = {n: dict(ms=[], G=[], D=[]) for n, _ in SETS}
for rep in range(args.repeat):
    for name, opts in SETS:
        for o in (tr.optim_G, tr.optim_D):
            o.param_groups[0].update(opts)
        for _ in range(2):  # (a switched amsgrad takes the general path once)
            tr.train_step(x, m, y)
        torch.cuda.synchronize()
        events["G"].clear()
        events["D"].clear()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            tr.train_step(x, m, y)
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) / args.steps * 1e3
        us = {k: sorted(e0.elapsed_time(e1) * 1e3 for e0, e1 in events[k]) for k in ("G", "D")}
        med = {k: v[len(v) // 2] for k, v in us.items()}
        res[name]["ms"].append(ms)
        res[name]["G"].append(med["G"])
        res[name]["D"].append(med["D"])
        print(f"round {rep} {name}: {ms:.3f} ms/step, update G {med['G']:.0f} us, D {med['D']:.0f} us "
              f"(medians of {args.steps})", flush=True)
for name, _ in SETS:
    r = {k: sorted(v)[len(v) // 2] for k, v in res[name].items()}
    print(f"{name}: median over {args.repeat} rounds {r['ms']:.3f} ms/step, update G {r['G']:.0f} us, "
          f"D {r['D']:.0f} us", flush=True)
