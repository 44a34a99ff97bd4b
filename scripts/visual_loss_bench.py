"""VisualLoss timings on the MI355X (HIP events, warm-up, interleaved repeats; not bench.py).

  --kernels   every conv layer of vgg19_bn.features[:40] at the real widths with random weights, bf16, bs 32,
              256 x 256: stc_conv3_fwd as VisualLoss runs it -- the forward on the pred | target batch of 2 x 32, the
              input gradient on the 32 pred images -- us per call and TFLOP/s (2 * M * 9 * Cin * Cout over the call
              time; the 3-channel first layer is counted with its 3 real channels), beside the k4 s1 halo kernel's
              rate of profiles/r06_final/summary.txt as context; then the pools, the normalise and the MSE (us).
              A window is REPS back-to-back calls between two events.
  --loss      VisualLoss forward + backward of one term (ms), bs 32, 256 x 256, full widths.
  --step      ms/step of STCGAN.train_step at C3 (ngf 64, bs 32, bf16) with lambda5 on, with lambda4 and lambda5 on,
              and off, alternating in one process."""
import argparse
import json
import os
import statistics
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "shadow-removal-istd_amd"))
import torch  # noqa: E402

from stcgan_amd import ops  # noqa: E402
from stcgan_amd.loss import VisualLoss, vgg19_bn_features  # noqa: E402

DEV = "cuda"
DT = torch.bfloat16
B = 32
SIZE = 256
HALO_K4_S1_PFLOPS = 1.13  # profiles/r06_final/summary.txt: the existing k4 s1 halo kernel (context, not a bar)
# (Cin, Cout, H) of the 12 convs of features[:40]; a pool follows convs 1, 3, 7, 11
LAYERS = [(3, 64, 256), (64, 64, 256), (64, 128, 128), (128, 128, 128), (128, 256, 64), (256, 256, 64), (256, 256, 64),
          (256, 256, 64), (256, 512, 32), (512, 512, 32), (512, 512, 32), (512, 512, 32)]


def window(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3  # us per call


def interleaved(fns, reps, repeats, warm=3):
    for fn in fns.values():
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():
            out[k].append(window(fn, reps))
    return out


def stat(v, unit="us"):
    return {f"median_{unit}": statistics.median(v), f"min_{unit}": min(v), f"max_{unit}": max(v)}


def random_vgg():
    seq = vgg19_bn_features()
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():
        for mod in seq:
            if isinstance(mod, torch.nn.Conv2d):
                mod.weight.copy_(torch.randn(mod.weight.shape, generator=g) * (2.0 / (9 * mod.in_channels)) ** 0.5)
            elif isinstance(mod, torch.nn.BatchNorm2d):
                mod.running_var.copy_(torch.rand(mod.running_var.shape, generator=g) + 0.5)
    return seq


def kernels(args):
    rows = []
    for k, (ci, co, H) in enumerate(LAYERS):
        cip = max(8, ci)
        w = torch.randn(co, ci, 3, 3, device=DEV) * (2.0 / (9 * ci)) ** 0.5
        (wf, wd), = ops.pack_conv3([w])
        bias = torch.randn(co, device=DEV) * 0.1
        x = torch.relu(torch.randn(2 * B, H, H, cip, device=DEV)).to(DT)
        y = torch.empty(2 * B, H, H, co, device=DEV, dtype=DT)
        g = torch.randn(B, H, H, co, device=DEV).to(DT)
        gx = torch.empty(B, H, H, cip, device=DEV, dtype=DT)
        mask = x[:B] if k > 0 else None

        def fwd():
            ops.conv3(x, wf, y, bias=bias, relu=True)

        def dgrad():
            ops.conv3(g, wd, gx, bias=None, relu=False, mask=mask)

        t = interleaved(dict(fwd=fwd, dgrad=dgrad), args.reps, args.repeats)
        flop_f = 2.0 * (2 * B) * H * H * 9 * ci * co
        flop_d = flop_f / 2
        row = dict(layer=k, cin=ci, cout=co, hw=H, plan=list(ops.conv3_plan(2 * B, H, H, cip, co)),
                   fwd=stat(t["fwd"]), dgrad=stat(t["dgrad"]))
        row["fwd_TFLOPs"] = flop_f / row["fwd"]["median_us"] / 1e6
        row["dgrad_TFLOPs"] = flop_d / row["dgrad"]["median_us"] / 1e6
        rows.append(row)
        print(f"conv{k:<2} {ci:3d}->{co:3d} {H:3d}x{H:<3d} fwd (2x{B}) {row['fwd']['median_us']:8.1f} us "
              f"[{row['fwd']['min_us']:.1f}, {row['fwd']['max_us']:.1f}] {row['fwd_TFLOPs']:6.1f} TF/s | dgrad ({B}) "
              f"{row['dgrad']['median_us']:8.1f} us [{row['dgrad']['min_us']:.1f}, {row['dgrad']['max_us']:.1f}] "
              f"{row['dgrad_TFLOPs']:6.1f} TF/s | k4 s1 halo kernel: {HALO_K4_S1_PFLOPS * 1e3:.0f} TF/s", flush=True)
        del x, y, g, gx, mask
    tot_f = sum(r["fwd"]["median_us"] for r in rows)
    tot_d = sum(r["dgrad"]["median_us"] for r in rows)
    print(f"all 12 convs: forward (2x{B}) {tot_f / 1e3:.2f} ms, input gradient ({B}) {tot_d / 1e3:.2f} ms")
    small = []
    for H, C in ((256, 64), (128, 128), (64, 256), (32, 512)):
        x = torch.relu(torch.randn(2 * B, H, H, C, device=DEV)).to(DT)
        y = torch.empty(2 * B, H // 2, H // 2, C, device=DEV, dtype=DT)
        g = torch.randn(B, H // 2, H // 2, C, device=DEV).to(DT)
        gx = torch.empty(B, H, H, C, device=DEV, dtype=DT)
        t = interleaved(dict(pool_fwd=lambda: ops.maxpool2(x, y), pool_bwd=lambda: ops.maxpool2_backward(x[:B], g, gx)),
                        args.reps, args.repeats)
        small.append(dict(op="maxpool2", hw=H, c=C, fwd=stat(t["pool_fwd"]), bwd=stat(t["pool_bwd"])))
        print(f"pool {H:3d}x{H:<3d}x{C:3d}: fwd (2x{B}) {small[-1]['fwd']['median_us']:7.1f} us, bwd ({B}) "
              f"{small[-1]['bwd']['median_us']:7.1f} us", flush=True)
        del x, y, g, gx
    src = torch.rand(B, 3, SIZE, SIZE, device=DEV) * 2 - 1
    xin = torch.empty(2 * B, SIZE, SIZE, 8, device=DEV, dtype=DT)
    gin = torch.randn(B, SIZE, SIZE, 8, device=DEV).to(DT)
    f = torch.relu(torch.randn(2 * B, 16, 16, 512, device=DEV)).to(DT)
    one = torch.ones((), device=DEV)
    t = interleaved(dict(norm_fwd=lambda: ops.vgg_normalise(src, xin[:B]),
                         norm_bwd=lambda: ops.vgg_normalise_backward(gin),
                         mse_fwd=lambda: ops.feature_mse(f[:B], f[B:]),
                         mse_bwd=lambda: ops.feature_mse_backward(f[:B], f[B:], one, True)), args.reps, args.repeats)
    for k, v in t.items():
        small.append(dict(op=k, **stat(v)))
        print(f"{k}: {statistics.median(v):7.1f} us [{min(v):.1f}, {max(v):.1f}]", flush=True)
    print(json.dumps(dict(kind="visual_kernels", reps=args.reps, repeats=args.repeats, convs=rows, others=small)))


def loss(args):
    vl = VisualLoss(random_vgg())
    vl.prepare(torch.device(DEV))
    yp = (torch.rand(B, 3, SIZE, SIZE, device=DEV) * 2 - 1).requires_grad_(True)
    yt = torch.rand(B, 3, SIZE, SIZE, device=DEV) * 2 - 1

    def fb():
        yp.grad = None
        vl(yp, yt).backward()

    def fo():
        with torch.no_grad():
            vl(yp, yt)

    t = interleaved(dict(fwd_bwd=fb, fwd_only=fo), args.steps, args.repeats, warm=2)
    res = {k: stat([u / 1e3 for u in v], "ms") for k, v in t.items()}
    for k, r in res.items():
        print(f"VisualLoss {k} (one term, bs {B}, {SIZE}x{SIZE}, full widths): {r['median_ms']:.2f} ms "
              f"[{r['min_ms']:.2f}, {r['max_ms']:.2f}]")
    print(json.dumps(dict(kind="visual_loss", **res)))


def step(args):
    from stcgan_amd.stcgan import STCGAN
    vl = VisualLoss(random_vgg())

    def trainer(l4, l5):
        torch.manual_seed(7)
        a = types.SimpleNamespace(devices=["cuda:0"], tasks=["train"], lr_G=5e-5, lr_D=2e-5, beta1=0.5, beta2=0.999,
                                  D_loss_fn="standard", D_loss_type="normal", ngf=64, dtype="bf16",
                                  load_weights_g1=None, load_weights_g2=None, load_weights_d1=None,
                                  load_weights_d2=None, lambda4=l4, lambda5=l5, visual_loss=vl)
        return STCGAN(a)

    g = torch.Generator(device=DEV)
    g.manual_seed(3)
    x = torch.rand((B, 3, SIZE, SIZE), generator=g, device=DEV) * 2 - 1
    m = (torch.rand((B, 1, SIZE, SIZE), generator=g, device=DEV) < 0.5).float() * 2 - 1
    y = torch.rand((B, 3, SIZE, SIZE), generator=g, device=DEV) * 2 - 1
    tr = {"off": trainer(0.0, 0.0), "lambda5": trainer(0.0, 0.5), "lambda4+lambda5": trainer(0.25, 0.5)}
    for t in tr.values():
        for _ in range(args.warmup):
            t.train_step(x, m, y)
    torch.cuda.synchronize()
    ms = {n: [] for n in tr}
    for _ in range(args.repeats):
        for n, t in tr.items():
            ms[n].append(window(lambda: t.train_step(x, m, y), args.steps) / 1e3)
    res = {n: stat(v, "ms") for n, v in ms.items()}
    for n in tr:
        print(f"train_step C3 {n:16}: {res[n]['median_ms']:.3f} ms/step [{res[n]['min_ms']:.3f}, {res[n]['max_ms']:.3f}] "
              f"over {args.repeats} windows of {args.steps} steps")
    print(json.dumps(dict(kind="visual_step", **res)))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--loss", action="store_true")
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("visual_loss_bench: needs a ROCm GPU")
    if a.kernels:
        kernels(a)
    if a.loss:
        loss(a)
    if a.step:
        step(a)
