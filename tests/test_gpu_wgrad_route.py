"""ops.wgrad runs what the library's route names: for one smallest shape per route kernel its result is bit-identical
to calling the entry point the route names directly with the route's workspace, and the label it puts into the timer
is the route's kernel name (csrc/wgrad_route.cpp).

Operands are small integers (tests/conv_exact_ref.py): every sum is exact, so nothing here needs a tolerance.
"""
import ctypes

import pytest
import torch

from conv_exact_ref import acts
from stcgan_amd import _lib as L
from stcgan_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, BF = torch.float32, torch.bfloat16

# id: (kernel, dtype, stride, D extent, G extent, R, Cg, rows, force, dslope, pad, plan config or None)
CASES = {
    "rows_mfma": (L.WG_ROWS_MFMA, BF, 1, (4, 4), (5, 5), 8, 64, 1, None, None, L.PAD_ZEROS, None),
    "rows_f32": (L.WG_ROWS, F32, 1, (4, 4), (5, 5), 8, 64, 1, None, None, L.PAD_ZEROS, None),
    "rows_wide": (L.WG_ROWS, BF, 1, (1, 32), (2, 33), 8, 64, 1, None, None, L.PAD_ZEROS, None),  # past 32 MFMA slots
    "tile_cfg2": (L.WG_BF16_TILE, BF, 2, (4, 4), (8, 8), 8, 8, None, None, None, L.PAD_ZEROS, 2),
    "tile_cfg1": (L.WG_BF16_TILE, BF, 2, (4, 4), (8, 8), 64, 8, None, None, None, L.PAD_ZEROS, 1),
    "ld": (L.WG_BF16_LD, BF, 2, (4, 4), (8, 8), 128, 8, None, None, None, L.PAD_ZEROS, 7),
    # the tile configs the automatic plan of so small a shape does not pick, forced: the label of each instantiation
    "cfg0": (L.WG_BF16_TILE, BF, 2, (4, 4), (8, 8), 128, 8, None, (0, 0), None, L.PAD_ZEROS, 0),
    "cfg3": (L.WG_BF16_TILE, BF, 2, (4, 4), (8, 8), 128, 8, None, (3, 0), None, L.PAD_ZEROS, 3),
    "cfg4": (L.WG_BF16_TILE, BF, 2, (4, 4), (8, 8), 128, 8, None, (4, 0), None, L.PAD_ZEROS, 4),
    "cfg5": (L.WG_BF16_TILE, BF, 2, (4, 4), (8, 8), 128, 8, None, (5, 0), None, L.PAD_ZEROS, 5),
    "cfg6": (L.WG_BF16_LD, BF, 2, (4, 4), (8, 8), 128, 8, None, (6, 0), None, L.PAD_ZEROS, 6),
    "halo_s2": (L.WG_HALO, BF, 2, (8, 8), (16, 16), 128, 16, None, (8, 0), None, L.PAD_ZEROS, 8),
    "halo_s1": (L.WG_HALO, BF, 1, (31, 31), (32, 32), 128, 16, None, (8, 0), None, L.PAD_ZEROS, 8),
    "fp_f32": (L.WG_FP_TILE, F32, 2, (4, 4), (8, 8), 8, 8, None, None, None, L.PAD_ZEROS, -1),
    "fp_prologue": (L.WG_FP_TILE, BF, 2, (4, 4), (8, 8), 8, 8, None, None, 0.5, L.PAD_ZEROS, -1),
    "reflect_bf16": (L.WG_FP_TILE, BF, 2, (2, 2), (4, 4), 8, 8, None, None, None, L.PAD_REFLECT, -1),
    "reflect_f32": (L.WG_FP_TILE, F32, 2, (2, 2), (4, 4), 8, 8, None, None, None, L.PAD_REFLECT, -1),
}
NAMES = {"rows_mfma": "wgrad_rows_mfma_kernel", "rows_f32": "wgrad_rows_kernel", "rows_wide": "wgrad_rows_kernel",
         "tile_cfg2": "wgrad_bf16_kernel<128, 16, 4, 1, true, true>",
         "tile_cfg1": "wgrad_bf16_kernel<64, 128, 1, 4, false, true>",
         "ld": "wgrad_bf16_ld_kernel<128, 128, 2, 2, false, true, 4, 3>",
         "cfg0": "wgrad_bf16_kernel<128, 128, 2, 2, false, true>",
         "cfg3": "wgrad_bf16_kernel<256, 256, 2, 4, false, false>",
         "cfg4": "wgrad_bf16_kernel<256, 128, 4, 2, false, true>",
         "cfg5": "wgrad_bf16_kernel<128, 256, 2, 4, false, true>",
         "cfg6": "wgrad_bf16_ld_kernel<128, 128, 2, 2, false, true, 4, 4>",
         "halo_s2": "wgrad_halo_kernel<8, false>", "halo_s1": "wgrad_halo_kernel<32, true>",
         "fp_f32": "wgrad_kernel", "fp_prologue": "wgrad_kernel",
         "reflect_bf16": "wgrad_reflect_kernel", "reflect_f32": "wgrad_reflect_kernel"}


def nhwc(B, H, W, C, seed, dt):
    return acts((B, H, W, C), seed).to(DEV, dt).contiguous()


@pytest.mark.parametrize("case", list(CASES))
def test_wgrad_runs_the_route(case):
    kernel, dt, stride, (dh, dw), (gh, gw), R, Cg, rows, force, dslope, pad, cfg = CASES[case]
    B = 1
    d, g = nhwc(B, dh, dw, R, 11, dt), nhwc(B, gh, gw, Cg, 12, dt)
    if rows:
        d[..., rows:] = 0  # (the padded channels)
    Dv, Gv = L.nhwc_view(d), L.nhwc_view(g)
    ws_bytes, plan, k, _, name = ops._wgrad_route(B, stride, Dv, R, Gv, Cg, Cg, dt, rows or 0, dslope is not None, pad,
                                                  force)
    assert k == kernel and name == NAMES[case], (k, name, plan)
    assert cfg is None or plan[0] == cfg, plan

    ops._timer = []
    try:
        got = ops.wgrad(B, stride, Dv, R, Gv, Cg, Cg, dt, dslope=dslope, device=DEV, force=force, rows=rows,
                        rows_kernel=True if rows else None, pad=pad)
        torch.cuda.synchronize()
        labels = [e[0] for e in ops._timer]
    finally:
        ops._timer = None
    assert labels == [name]

    # the entry point the route names, called directly with the route's workspace
    l, code = L.lib(), L.dtype_code(dt)
    ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=DEV)
    want = torch.full((R, Cg, 4, 4), float("nan"), dtype=F32, device=DEV)
    fp = (ctypes.c_int32 * 2)(*force) if force else None
    if kernel in (L.WG_ROWS, L.WG_ROWS_MFMA):
        rc = l.stc_conv_wgrad_rows(code, B, Dv, R, rows, Gv, Cg, Cg, L.ptr(want), L.ptr(ws), ws_bytes, L.stream())
    elif pad == L.PAD_REFLECT:
        rc = l.stc_conv_pad_wgrad(code, L.CONV_S2 if stride == 2 else L.CONV_S1, pad, B, Dv, R, Gv, Cg, Cg, L.ptr(want),
                                  fp, L.ptr(ws), ws_bytes, L.stream())
    else:
        rc = l.stc_conv_wgrad_ex(code, B, stride, Dv, R, None, None, 0 if dslope is None else 1,
                                 0.0 if dslope is None else dslope, Gv, Cg, Cg, None, None, 0, 0.0, L.ptr(want), fp,
                                 L.ptr(ws), ws_bytes, L.stream())
    L.check(rc, "the route's entry point")
    torch.cuda.synchronize()
    assert torch.equal(got, want)
    assert bool(got.abs().sum() > 0)
