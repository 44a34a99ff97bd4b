#!/usr/bin/env python3
"""Every host-only answer of the conv dispatch, as text: one line per question and answer.

    python scripts/conv_route_table.py LIBRARY [--out FILE] [--reduced]

No GPU: the questions are stc_conv_fwd_workspace, stc_conv_fwd_plan, stc_conv_fwd_query, stc_conv_bwd_bn_chunks,
stc_conv_bwd_bn_chunks_ex, stc_conv_fwd_act_ok and stc_conv_bwd_act_ok, which only compute.  Two builds of the
library decide every call alike exactly when their tables are byte-identical (profiles/conv_route/README.md).  The
table goes to FILE (default: nowhere); the line count, the sha256 of the whole and one sha256 per section are printed.
Views are named by their layout, never by an address.
"""
import argparse
import ctypes
import hashlib
import itertools
import sys

F32, BF16 = 0, 1
KINDS = {0: "conv_s2", 1: "conv_s1", 2: "convt_s2", 3: "conv_s1_dgrad"}
BASE = 1 << 20  # a 16-byte aligned stand-in address (nothing is dereferenced)


class View(ctypes.Structure):
    _fields_ = [("p", ctypes.c_void_p), ("H", ctypes.c_int32), ("W", ctypes.c_int32), ("bs", ctypes.c_int64),
                ("rs", ctypes.c_int64), ("ps", ctypes.c_int32), ("co", ctypes.c_int32), ("cs", ctypes.c_int32),
                ("pad_", ctypes.c_int32)]


class BnbFuse(ctypes.Structure):
    _fields_ = [("x", View), ("g_other", View), ("scale", ctypes.c_void_p), ("shift", ctypes.c_void_p),
                ("mean", ctypes.c_void_p), ("rstd", ctypes.c_void_p), ("slope_self", ctypes.c_float),
                ("slope_other", ctypes.c_float), ("C", ctypes.c_int32), ("ch_off", ctypes.c_int32)]


def load(path):
    lib = ctypes.CDLL(path)
    i, i64, vp = ctypes.c_int, ctypes.c_int64, ctypes.c_void_p
    lib.stc_conv_fwd_workspace.restype = i64
    lib.stc_conv_fwd_workspace.argtypes = [i] * 7
    lib.stc_conv_fwd_plan.argtypes = [i] * 7 + [vp]
    lib.stc_conv_fwd_query.argtypes = [i] * 8 + [vp] * 4
    lib.stc_conv_bwd_bn_chunks.argtypes = [i] * 9
    lib.stc_conv_bwd_bn_chunks_ex.argtypes = [i, i, i, View, i, i, View, vp]
    lib.stc_conv_fwd_act_ok.argtypes = [i, i, i, View, i, i, View, View]
    lib.stc_conv_bwd_act_ok.argtypes = [i, i, i, View, i, i, View, View, View]
    lib.stc_set_splitk_inlaunch.argtypes = [i]
    return lib


# ---- the matrix
# GEMM grids: the generator's levels for 256 x 256 (128 ... 1), 480 x 640 (with its padded 15 x 20 -> 16 x 20 and
# 4 x 5 -> 4 x 6 levels) and 250 x 254 inputs; the PatchGAN's 128, 64, 32, 31, 30
GRIDS = [(g, g) for g in (1, 2, 4, 8, 16, 30, 31, 32, 64, 128)] + [
    (240, 320), (120, 160), (60, 80), (30, 40), (15, 20), (16, 20), (8, 10), (4, 5), (4, 6), (2, 3), (1, 2),
    (125, 127), (62, 63), (63, 64), (31, 32), (16, 16), (15, 16), (8, 8), (7, 8)]
GRIDS = list(dict.fromkeys(GRIDS))
BATCHES = (1, 2, 32)
CINS = (8, 16, 32, 64, 128, 256, 512, 1024)   # ngf / ndf 8 and 64, padded to the kernels' 8-channel units
COUTS = (1, 8, 16, 32, 64, 128, 256, 512, 1024)
FORCES = [None, (-1, 0), (-2, 0)] + [(100, s) for s in range(7)] + [(0, 1), (5, 2), (5, 4), (12, 8)]
LAYOUTS = ("dense", "concat", "co4", "rowpad", "crop", "off8", "nchw_out", "in2g")

REDUCED = dict(grids=[(1, 1), (2, 2), (8, 8), (16, 16), (31, 31), (32, 32), (128, 128), (15, 20), (4, 6)],
               cins=(8, 64, 512, 1024), couts=(1, 8, 64, 128, 512))


def extents(kind, Hg, Wg):
    """(input H, W), (output H, W) of a conv kind for the GEMM grid Hg x Wg."""
    if kind == 0:
        return (2 * Hg, 2 * Wg), (Hg, Wg)
    if kind == 1:
        return (Hg + 1, Wg + 1), (Hg, Wg)
    if kind == 2:
        return (Hg, Wg), (2 * Hg, 2 * Wg)
    return (Hg - 1, Wg - 1), (Hg, Wg)


def view(layout, H, W, C, B, role):
    """A view of H x W x C in the named layout; role: 'in', 'out' or 'side' (BN input, second gradient / output)."""
    v = View(BASE, H, W, H * W * C, W * C, C, 0, 1, 0)
    if layout == "concat":      # the second half of a 2C-channel concat buffer
        v.ps, v.co, v.rs, v.bs = 2 * C, C, W * 2 * C, H * W * 2 * C
    elif layout == "co4":       # channel offset 4 in a buffer of C + 8 channels
        v.ps, v.co, v.rs, v.bs = C + 8, 4, W * (C + 8), H * W * (C + 8)
    elif layout == "rowpad":    # one pixel of padding at the end of each row
        v.rs, v.bs = (W + 1) * C, H * (W + 1) * C
    elif layout == "crop":      # the top-left H x W of an (H + 2) x (W + 2) allocation
        v.rs, v.bs = (W + 2) * C, (H + 2) * (W + 2) * C
    elif layout == "off8":      # 8 bytes off 16-byte alignment
        v.p = BASE + 8
    elif layout == "nchw_out" and role == "out":   # an NCHW (fp32) output
        v.ps, v.rs, v.cs, v.bs = 1, W, H * W, C * H * W
    elif layout == "in2g" and role == "in":        # an input view of >= 2^31 bytes
        need = -(-(1 << 30) // B)
        v.bs = max(v.bs, (need + 7) // 8 * 8)
    return v


def run(lib, out, reduced):
    grids, cins, couts = (REDUCED["grids"], REDUCED["cins"], REDUCED["couts"]) if reduced else (GRIDS, CINS, COUTS)
    digests = {}
    total = hashlib.sha256()
    count = [0]

    def emit(section, line):
        data = (section + " " + line + "\n").encode()
        total.update(data)
        digests.setdefault(section, hashlib.sha256()).update(data)
        count[0] += 1
        if out:
            out.write(data)

    plan4 = (ctypes.c_int32 * 4)()
    plan5 = (ctypes.c_int32 * 5)()
    ws = ctypes.c_int64()
    nch = ctypes.c_int32()
    null_view = View()
    old = lib.stc_set_splitk_inlaunch(-1)
    try:
        for inl in (1, 0):
            lib.stc_set_splitk_inlaunch(inl)
            for dtype, kind, B, (Hg, Wg), Cin, Cout in itertools.product((F32, BF16), KINDS, BATCHES, grids, cins, couts):
                (iH, iW), (oH, oW) = extents(kind, Hg, Wg)
                key = "inl=%d %s %s B=%d grid=%dx%d Cin=%d Cout=%d" % (inl, "bf16" if dtype else "f32", KINDS[kind], B, Hg,
                                                                      Wg, Cin, Cout)
                shape = (dtype, kind, B, Hg, Wg, Cin, Cout)
                emit("workspace", "%s -> %d" % (key, lib.stc_conv_fwd_workspace(*shape)))
                rc = lib.stc_conv_fwd_plan(*shape, plan4)
                emit("plan", "%s -> rc=%d %s" % (key, rc, list(plan4)))
                emit("bwd_bn_chunks", "%s x=%dx%d -> %d" % (key, oH, oW, lib.stc_conv_bwd_bn_chunks(*shape, oH, oW)))
                for force in FORCES:
                    fp = (ctypes.c_int32 * 2)(*force) if force else None
                    for out_f32 in (0, 1):
                        rc = lib.stc_conv_fwd_query(*shape, out_f32, fp, ctypes.byref(ws), ctypes.byref(nch), plan5)
                        emit("query", "%s out_f32=%d force=%s -> rc=%d ws=%d chunks=%d plan=%s" % (
                            key, out_f32, force, rc, ws.value, nch.value, list(plan5)))
                # the forms that take views (an input-gradient grid of one row or column has no input to view)
                if iH < 1 or iW < 1:
                    continue
                for layout in LAYOUTS:
                    x = view(layout, iH, iW, Cin, B, "in")
                    y = view(layout, oH, oW, Cout, B, "out")
                    side = view(layout, oH, oW, Cout, B, "side")
                    for second in (0, 1):
                        f = BnbFuse(x=side, g_other=side if second else null_view, C=Cout, ch_off=0)
                        vkey = "%s views=%s second=%d" % (key, layout, second)
                        emit("bwd_bn_chunks_ex", "%s -> %d" % (
                            vkey, lib.stc_conv_bwd_bn_chunks_ex(dtype, kind, B, x, Cin, Cout, y, ctypes.byref(f))))
                        emit("fwd_act_ok", "%s -> %d" % (
                            vkey, lib.stc_conv_fwd_act_ok(dtype, kind, B, x, Cin, Cout, y, side if second else null_view)))
                        emit("bwd_act_ok", "%s -> %d" % (
                            vkey, lib.stc_conv_bwd_act_ok(dtype, kind, B, x, Cin, Cout, y, side,
                                                          side if second else null_view)))
    finally:
        lib.stc_set_splitk_inlaunch(old)
    return count[0], total.hexdigest(), {k: v.hexdigest() for k, v in digests.items()}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("library")
    ap.add_argument("--out", help="write the table here")
    ap.add_argument("--reduced", action="store_true", help="a small matrix (seconds)")
    args = ap.parse_args()
    lib = load(args.library)
    out = open(args.out, "wb") if args.out else None
    n, whole, sections = run(lib, out, args.reduced)
    if out:
        out.close()
    print("lines %d" % n)
    print("sha256 %s" % whole)
    for name in sorted(sections):
        print("section %-17s %s" % (name, sections[name]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
