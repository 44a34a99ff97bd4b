"""Instance-norm timings on the MI355X (HIP events, warm-up, interleaved repeats; not bench.py).

  --kernels   stc_in_fwd / stc_in_bwd at the C3 shapes (bs 32, bf16, every normed tensor of G and D at 256x256)
              beside the unfused BatchNorm sequence on the same tensor in the same run
              (stc_chan_stats + stc_bn_finalize + stc_bn_apply, resp. stc_bn_bwd_reduce + stc_bn_bwd_apply; those
              kernels are the parent commit's).  Both with affine parameters, one output / one incoming gradient.
              A window is REPS back-to-back calls between two events, so a call shorter than its enqueue (~10-20 us of
              host time per library call) is timed at the enqueue rate: one launch against three still shows.
              Bytes/s of the streamed shapes count two reads and one write of the tensor (backward: x and g twice,
              dx once); the second read of a 2 MB-per-sample plane is cache-resident, so this is not an HBM figure.
  --step      ms/step of STCGAN.train_step at C3 (ngf 64, bs 32, bf16) with norm="instance" beside norm="batch",
              interleaved.
STC_LIB_PATH selects another build of the library (e.g. -DSTC_IN_SLAB_VECS=1 for a 16-byte slab): the A/B of the
slab width is this script run once per build."""
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
# (H, W, C, where): every normed tensor of the C3 step
SHAPES = [(128, 128, 64, "G up1"), (64, 64, 128, "G down1/up2, D1"), (32, 32, 256, "G down2/up3, D2"),
          (31, 31, 512, "D3"), (16, 16, 512, "G down3/up4"), (8, 8, 512, "G down4/up5"), (4, 4, 512, "G down5/up6"),
          (2, 2, 512, "G down6/up7")]
REGIME = ["tiny", "resident", "streamed"]


class Norm:
    def __init__(self, C):
        self.weight = torch.rand(C, device=DEV) + 0.5
        self.bias = torch.randn(C, device=DEV) * 0.1
        self.running_mean = torch.zeros(C, device=DEV)
        self.running_var = torch.ones(C, device=DEV)
        self.num_batches_tracked = torch.zeros((), dtype=torch.long, device=DEV)
        self.momentum, self.eps = 0.1, 1e-5


def window(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3  # us per call


def interleaved(fns, reps, repeats):
    """{name: [us per call, one per repeat]}, the candidates alternating inside every repeat."""
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
        y = torch.empty_like(x)
        dx = torch.empty_like(x)
        nrm = Norm(C)
        xv, gv, yv, dxv = L.nhwc_view(x), L.nhwc_view(g), L.nhwc_view(y), L.nhwc_view(dx)
        tab = torch.empty((2, C), device=DEV)
        stats = ops.in_forward(B, xv, C, DT, nrm, xv, yv, 0.2)
        bn_stats = ops.bn_train_table(B, xv, C, DT, nrm, tab[0], tab[1])

        def in_f():
            ops.in_forward(B, xv, C, DT, nrm, xv, yv, 0.2)

        def bn_f():
            ops.bn_train_table(B, xv, C, DT, nrm, tab[0], tab[1])
            ops.bn_apply(B, xv, C, DT, (tab[0], tab[1]), yv, 0.2)

        def in_b():
            ops.in_backward(B, xv, C, DT, dxv, nrm, stats, g1=gv, s1=0.2)

        def bn_b():
            ops.bn_backward(B, xv, C, DT, dxv, g1=gv, s1=0.2,
                            bn_state=(tab[0], tab[1], bn_stats[0], bn_stats[1], nrm.weight))

        t = interleaved(dict(in_fwd=in_f, bn_fwd=bn_f, in_bwd=in_b, bn_bwd=bn_b), args.reps, args.repeats)
        regime, slab, chunks, m = ops.in_plan(B, H, W, C, DT)
        nbytes = x.numel() * 2
        row = dict(shape=f"{B}x{H}x{W}x{C}", where=where, regime=REGIME[regime], slab_channels=slab, chunks=chunks)
        for k, v in t.items():
            row[k] = dict(median_us=statistics.median(v), min_us=min(v), max_us=max(v))
        row["in_fwd_GBps"] = 3 * nbytes / row["in_fwd"]["median_us"] / 1e3
        row["in_bwd_GBps"] = 5 * nbytes / row["in_bwd"]["median_us"] / 1e3
        rows.append(row)
        f, bf, b, bb = row["in_fwd"], row["bn_fwd"], row["in_bwd"], row["bn_bwd"]
        print(f"{row['shape']:>16} {row['regime']:>8} slab {slab:3d} chunks {chunks:2d} | fwd IN {f['median_us']:7.1f} us "
              f"[{f['min_us']:.1f}, {f['max_us']:.1f}]  BN x3 {bf['median_us']:7.1f} us [{bf['min_us']:.1f}, "
              f"{bf['max_us']:.1f}] | bwd IN {b['median_us']:7.1f} us [{b['min_us']:.1f}, {b['max_us']:.1f}]  BN x2 "
              f"{bb['median_us']:7.1f} us [{bb['min_us']:.1f}, {bb['max_us']:.1f}] | IN {row['in_fwd_GBps']:6.0f} / "
              f"{row['in_bwd_GBps']:6.0f} GB/s", flush=True)
    print(json.dumps(dict(kind="inorm_kernels", lib=os.path.basename(L.LIB_PATH), reps=args.reps, repeats=args.repeats,
                          rows=rows)))


def step(args):
    from stcgan_amd.stcgan import STCGAN

    def trainer(norm):
        torch.manual_seed(7)
        a = types.SimpleNamespace(devices=["cuda:0"], tasks=["train"], lr_G=5e-5, lr_D=2e-5, beta1=0.5, beta2=0.999,
                                  D_loss_fn="standard", D_loss_type="normal", ngf=64, dtype="bf16",
                                  load_weights_g1=None, load_weights_g2=None, load_weights_d1=None,
                                  load_weights_d2=None, norm=norm)
        return STCGAN(a)

    g = torch.Generator(device=DEV)
    g.manual_seed(3)
    x = torch.rand((B, 3, 256, 256), generator=g, device=DEV) * 2 - 1
    m = (torch.rand((B, 1, 256, 256), generator=g, device=DEV) < 0.5).float() * 2 - 1
    y = torch.rand((B, 3, 256, 256), generator=g, device=DEV) * 2 - 1
    tr = {n: trainer(n) for n in ("batch", "instance")}
    for t in tr.values():
        for _ in range(args.warmup):
            t.train_step(x, m, y)
    torch.cuda.synchronize()
    ms = {n: [] for n in tr}
    for _ in range(args.repeats):
        for n, t in tr.items():
            ms[n].append(window(lambda: t.train_step(x, m, y), args.steps) / 1e3)
    res = {n: dict(median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v)) for n, v in ms.items()}
    res["ratio"] = res["instance"]["median_ms"] / res["batch"]["median_ms"]
    for n in tr:
        print(f"train_step C3 norm={n:8}: {res[n]['median_ms']:.3f} ms/step [{res[n]['min_ms']:.3f}, "
              f"{res[n]['max_ms']:.3f}] over {args.repeats} windows of {args.steps} steps")
    print(f"instance / batch = {res['ratio']:.3f}")
    print(json.dumps(dict(kind="inorm_step", **res)))


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
        sys.exit("inorm_bench: needs a ROCm GPU")
    if a.kernels:
        kernels(a)
    if a.step:
        step(a)
