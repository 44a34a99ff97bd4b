"""Library calls and collectives of one train step, args.norm = "batch" against "sync_batch", at world 2.

Two processes share GPU 0 over gloo (as tests/test_gpu_syncbn_dist.py), ngf 8, 256 x 256, local batch 2, fp32.  Every
C-ABI entry point of the library and every torch.distributed collective is counted over the third train step (the
first two warm the caches), on rank 0:

  python scripts/sync_bn_counts.py > profiles/sync_bn/launch_counts.txt

A library call is one or more kernel launches (include/stcgan_hip.h says which); the sync forms replace the fused
stc_conv_bn_fwd (conv, finalize, apply) by stc_conv_fwd_ex + stc_bn_stats_pack + stc_bn_finalize + stc_bn_apply and
stc_conv_bwd_bn_apply (conv, finalize, apply) by stc_conv_bwd_bn + stc_bn_bwd_sums + stc_bn_bwd_apply_sync: one launch
more per normed layer forward, none backward, and one collective each way."""
import collections
import os
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("tests", os.path.join("tests", "golden"), "shadow-removal-istd_amd", ""):
    sys.path.insert(0, os.path.join(ROOT, p))

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

import syncbn_ref as S  # noqa: E402

COLLECTIVES = ("all_reduce", "all_gather_into_tensor", "broadcast", "all_gather_object", "barrier")


def worker(rank, world, port, out):
    S.init_world(rank, world, port)
    try:
        from fixture_init import pm_one, uniform
        from stcgan_amd import _lib as L
        from stcgan_amd.stcgan import STCGAN
        torch.cuda.set_device(0)
        counts = collections.Counter()
        on = [False]
        h = L.lib()
        for name in L.EXPORTED:  # count every entry point (the ctypes functions keep their prototypes)
            fn = getattr(h, name)

            def wrapped(*a, _fn=fn, _name=name):
                if on[0]:
                    counts["lib:" + _name] += 1
                return _fn(*a)
            setattr(h, name, wrapped)
        for name in COLLECTIVES:
            fn = getattr(dist, name)

            def wrapped(*a, _fn=fn, _name=name, **kw):
                if on[0]:
                    counts["dist:" + _name] += 1
                return _fn(*a, **kw)
            setattr(dist, name, wrapped)
        res = {}
        for norm in ("batch", "sync_batch"):
            torch.manual_seed(5)
            a = types.SimpleNamespace(devices=["cuda:0"], tasks=["train"], lr_G=5e-5, lr_D=2e-5, beta1=0.5,
                                      beta2=0.999, D_loss_fn="standard", D_loss_type="normal", ngf=8, dtype="fp32",
                                      norm=norm, load_weights_g1=None, load_weights_g2=None, load_weights_d1=None,
                                      load_weights_d2=None)
            tr = STCGAN(a)
            x, m, y = (uniform((2, 3, 256, 256), 1 + rank).cuda(), pm_one((2, 1, 256, 256), 3 + rank).cuda(),
                       uniform((2, 3, 256, 256), 5 + rank).cuda())
            for step in range(3):
                counts.clear()
                on[0] = step == 2
                tr.train_step(x, m, y)
                torch.cuda.synchronize()
            on[0] = False
            res[norm] = dict(counts)
        S.put_result(out, rank, res)
        dist.barrier()
    finally:
        dist.destroy_process_group()


if __name__ == "__main__":
    got = S.run_world(worker, 2)[0]
    names = sorted(set(got["batch"]) | set(got["sync_batch"]))
    print("calls in one train step on rank 0 (world 2, gloo, ngf 8, 256 x 256, local batch 2, fp32, loss type normal)")
    print(f"{'call':44s} {'batch':>8s} {'sync_batch':>11s}")
    for n in names:
        a, b = got["batch"].get(n, 0), got["sync_batch"].get(n, 0)
        print(f"{n:44s} {a:8d} {b:11d}" + ("" if a == b else "   *"))
    for kind in ("lib:", "dist:"):
        a = sum(v for k, v in got["batch"].items() if k.startswith(kind))
        b = sum(v for k, v in got["sync_batch"].items() if k.startswith(kind))
        print(f"{'total ' + kind:44s} {a:8d} {b:11d}")
