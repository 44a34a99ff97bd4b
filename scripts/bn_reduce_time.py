"""Per-launch time (HIP events, 50 launches after a warm-up) of the per-chunk channel reductions of csrc/bn.hip --
stc_chan_stats, stc_chan_sum, stc_bn_bwd_reduce -- on the train step's shapes (B = 32), fp32 and bf16, with whichever
library STC_LIB_PATH names.  The bf16 step runs the first and the last inside conv epilogues, so a kernel trace of the
step does not show them."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "shadow-removal-istd_amd"))
import torch  # noqa: E402

from stcgan_amd import _lib as L  # noqa: E402

dev, B, REPS = "cuda", 32, 50
lib = L.lib()


def timed(fn):
    for _ in range(3):
        assert fn() == 0, lib.stc_last_error().decode()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(REPS):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / REPS * 1e3


for dt in (torch.float32, torch.bfloat16):
    code = L.dtype_code(dt)
    for H, C in ((128, 64), (64, 128), (16, 512)):
        x, g1, g2 = (torch.randn(B, H, H, C, device=dev).to(dt) for _ in range(3))
        xv, g1v, g2v = L.nhwc_view(x), L.nhwc_view(g1), L.nhwc_view(g2)
        tab = [torch.rand(C, device=dev) + 0.5 for _ in range(4)]
        nch = lib.stc_chan_stats_chunks(B, H, H)
        part = torch.empty(nch * C * 4, device=dev)
        out = torch.empty(C, device=dev)
        st = L.stream()
        t = [timed(lambda: lib.stc_chan_stats(code, B, xv, C, L.ptr(part), nch, st)),
             timed(lambda: lib.stc_chan_sum(code, B, xv, C, C, L.ptr(part), nch, L.ptr(out), st)),
             timed(lambda: lib.stc_bn_bwd_reduce(code, B, xv, C, *(L.ptr(v) for v in tab), g1v, 0.0, g2v, 0.2, L.ptr(part),
                                                 nch, st))]
        print(f"{'f32' if dt == torch.float32 else 'bf16'} {B}x{H}x{H}x{C}: chan_stats {t[0]:7.1f} us  "
              f"chan_sum (+final) {t[1]:7.1f} us  bn_bwd_reduce {t[2]:7.1f} us")
