"""Frozen-statistics BatchNorm timings on the MI355X (HIP events, warm-up, interleaved repeats; not bench.py).

  --kernels   stc_bn_bwd_frozen with sums (one pass + the chunk merge) and without (one streaming pass) beside the
              train-mode pair stc_bn_bwd_reduce + stc_bn_bwd_apply on the same tensors in the same run, at the C3
              shapes (bs 32, bf16, every normed tensor of G and D at 256x256; the table of scripts/inorm_bench.py),
              one incoming gradient.  A window is REPS back-to-back calls between two events, so a call shorter than
              its enqueue (~10-20 us of host time per library call) is timed at the enqueue rate.
  --step      ms/step of STCGAN.train_step at C3 (ngf 64, bs 32, bf16) with args.freeze_norm on beside off,
              interleaved windows."""
import argparse
import json
import os
import statistics
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "shadow-removal-istd_amd"))
import torch  # noqa: E402

from stcgan_amd import _lib as L, ops  # noqa: E402

DEV = "cuda"
DT = torch.bfloat16
B = 32
SHAPES = [(128, 128, 64, "G up1"), (64, 64, 128, "G down1/up2, D1"), (32, 32, 256, "G down2/up3, D2"),
          (31, 31, 512, "D3"), (16, 16, 512, "G down3/up4"), (8, 8, 512, "G down4/up5"), (4, 4, 512, "G down5/up6"),
          (2, 2, 512, "G down6/up7")]


def window(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3  # us per call


def interleaved(fns, reps, repeats):
    for fn in fns.values():
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():
            out[k].append(window(fn, reps))
    return out


def kernels(args):
    rows = []
    for H, W, C, where in SHAPES:
        x = torch.randn(B, H, W, C, device=DEV).to(DT)
        g = torch.randn(B, H, W, C, device=DEV).to(DT)
        dx = torch.empty_like(x)
        xv, gv, dxv = L.nhwc_view(x), L.nhwc_view(g), L.nhwc_view(dx)
        gamma = torch.rand(C, device=DEV) + 0.5
        mean, rstd = torch.randn(C, device=DEV) * 0.1, torch.rand(C, device=DEV) + 0.5
        scale, shift = gamma * rstd, torch.randn(C, device=DEV) * 0.1
        state = (scale, shift, mean, rstd)

        def pair():
            ops.bn_backward(B, xv, C, DT, dxv, g1=gv, s1=0.2, bn_state=state + (gamma,))

        def frozen_sums():
            ops.bn_backward_frozen(B, xv, C, DT, dxv, gv, 0.2, state=state)

        def frozen_dx():
            ops.bn_backward_frozen(B, xv, C, DT, dxv, gv, 0.2, state=state, want_params=False)

        t = interleaved(dict(pair=pair, frozen_sums=frozen_sums, frozen_dx=frozen_dx), args.reps, args.repeats)
        row = dict(shape=f"{B}x{H}x{W}x{C}", where=where, MB=x.numel() * 2 / 1e6)
        for k, v in t.items():
            row[k] = dict(median_us=statistics.median(v), min_us=min(v), max_us=max(v))
        row["frozen_dx_GBps"] = 3 * x.numel() * 2 / row["frozen_dx"]["median_us"] / 1e3  # x, g read, dx written
        rows.append(row)
        print(f"{row['shape']:>16} {where:>18} | " + " | ".join(
            f"{k} {row[k]['median_us']:7.1f} us [{row[k]['min_us']:.1f}, {row[k]['max_us']:.1f}]" for k in t)
            + f" | dx pass {row['frozen_dx_GBps']:6.0f} GB/s", flush=True)
    print(json.dumps(dict(kind="frozen_norm_kernels", reps=args.reps, repeats=args.repeats, rows=rows)))


def step(args):
    from stcgan_amd.stcgan import STCGAN

    def trainer(freeze):
        torch.manual_seed(7)
        a = types.SimpleNamespace(devices=["cuda:0"], tasks=["train"], lr_G=5e-5, lr_D=2e-5, beta1=0.5, beta2=0.999,
                                  D_loss_fn="standard", D_loss_type="normal", ngf=64, dtype="bf16",
                                  load_weights_g1=None, load_weights_g2=None, load_weights_d1=None,
                                  load_weights_d2=None, freeze_norm=freeze)
        return STCGAN(a)

    g = torch.Generator(device=DEV)
    g.manual_seed(3)
    x = torch.rand((B, 3, 256, 256), generator=g, device=DEV) * 2 - 1
    m = (torch.rand((B, 1, 256, 256), generator=g, device=DEV) < 0.5).float() * 2 - 1
    y = torch.rand((B, 3, 256, 256), generator=g, device=DEV) * 2 - 1
    tr = {n: trainer(n == "frozen") for n in ("batch", "frozen")}
    for t in tr.values():
        for _ in range(args.warmup):
            t.train_step(x, m, y)
    torch.cuda.synchronize()
    ms = {n: [] for n in tr}
    for _ in range(args.repeats):
        for n, t in tr.items():
            ms[n].append(window(lambda: t.train_step(x, m, y), args.steps) / 1e3)
    res = {n: dict(median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v)) for n, v in ms.items()}
    res["ratio"] = res["frozen"]["median_ms"] / res["batch"]["median_ms"]
    for n in tr:
        print(f"train_step C3 freeze_norm={n == 'frozen'!s:5}: {res[n]['median_ms']:.3f} ms/step [{res[n]['min_ms']:.3f}, "
              f"{res[n]['max_ms']:.3f}] over {args.repeats} windows of {args.steps} steps")
    print(f"frozen / batch = {res['ratio']:.3f}")
    print(json.dumps(dict(kind="frozen_norm_step", **res)))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("frozen_norm_bench: needs a ROCm GPU")
    if a.kernels:
        kernels(a)
    if a.step:
        step(a)
