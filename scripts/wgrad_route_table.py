#!/usr/bin/env python3
"""Every host-only answer of the weight-gradient dispatch, as text: one line per question and answer.

    python scripts/wgrad_route_table.py LIBRARY [--out FILE] [--reduced] [--old-only]

No GPU.  Section "old": stc_conv_wgrad_query, stc_conv_wgrad_workspace, stc_conv_pad_wgrad_query and
stc_conv_wgrad_rows_workspace, which every build of the library has: two builds answer alike exactly when these
sections are byte-identical (profiles/wgrad_route/README.md).  Section "route": stc_conv_wgrad_route, the route of
actual views and stride (skipped with --old-only, or where the library has no such symbol).  The table goes to FILE
(default: nowhere); the line count, one sha256 per section and the kernel x reduce pairs that occur are printed.
Over the whole cross it also checks that the stride-less query's workspace covers the route's (every GEMM ask with
zero padding): misses are printed and the exit status is 1.
Views are named by their layout, never by an address.
"""
import argparse
import collections
import ctypes
import hashlib
import itertools
import sys

F32, BF16 = 0, 1
ZEROS, REFLECT = 0, 1
CONV_S2, CONV_S1 = 0, 1
BASE = 1 << 20  # a 16-byte aligned stand-in address (nothing is dereferenced)
KERNELS = ("WG_NONE", "WG_FP_TILE", "WG_BF16_TILE", "WG_BF16_LD", "WG_HALO", "WG_ROWS", "WG_ROWS_MFMA")
REDUCES = ("WR_NONE", "WR_PLAIN", "WR_V4", "WR_MANY")


class View(ctypes.Structure):
    _fields_ = [("p", ctypes.c_void_p), ("H", ctypes.c_int32), ("W", ctypes.c_int32), ("bs", ctypes.c_int64),
                ("rs", ctypes.c_int64), ("ps", ctypes.c_int32), ("co", ctypes.c_int32), ("cs", ctypes.c_int32),
                ("pad_", ctypes.c_int32)]


def load(path):
    lib = ctypes.CDLL(path)
    i, i64, vp = ctypes.c_int, ctypes.c_int64, ctypes.c_void_p
    lib.stc_conv_wgrad_query.argtypes = [i] * 6 + [vp] * 3
    lib.stc_conv_wgrad_workspace.restype = i64
    lib.stc_conv_wgrad_workspace.argtypes = [i] * 6
    lib.stc_conv_pad_wgrad_query.argtypes = [i] * 8 + [vp] * 3
    lib.stc_conv_wgrad_rows_workspace.restype = i64
    lib.stc_conv_wgrad_rows_workspace.argtypes = [i] * 4
    if hasattr(lib, "stc_conv_wgrad_route"):
        lib.stc_conv_wgrad_route.argtypes = [i, i, i, View, i, i, View, i, i, i, i, vp, vp, vp, vp, vp, i]
    return lib


# ---- the matrix
DTYPES = (F32, BF16)
BATCHES = (1, 2, 5, 32)
GRIDS = [(g, g) for g in (1, 2, 4, 8, 15, 16, 30, 31, 32, 62, 64, 128)] + [(4, 5), (31, 32)]
RS = (8, 16, 64, 96, 128, 256, 512)
CGS = (8, 16, 64, 128, 256, 512)
FORCES = [None, (-1, 0), (-1, -1)] + [(c, 0) for c in range(9)] + [(7, 4), (8, 2)]
LAYOUTS = ("dense", "concat", "co8", "rowpad", "off8", "nchw")
G_GRIDS = ("2x", "+1", "neither")

REDUCED = dict(batches=(1, 32), grids=[(1, 1), (4, 4), (8, 8), (31, 31), (32, 32), (4, 5)], rs=(8, 64, 128, 512),
               cgs=(8, 64, 256))


def view(layout, H, W, C):
    v = View(BASE, H, W, H * W * C, W * C, C, 0, 1, 0)
    if layout == "concat":      # the second half of a 2C-channel concat buffer
        v.ps, v.co, v.rs, v.bs = 2 * C, C, W * 2 * C, H * W * 2 * C
    elif layout == "co8":       # channel offset 8 in a buffer of C + 16 channels
        v.ps, v.co, v.rs, v.bs = C + 16, 8, W * (C + 16), H * W * (C + 16)
    elif layout == "rowpad":    # one pixel of padding at the end of each row
        v.rs, v.bs = (W + 1) * C, H * (W + 1) * C
    elif layout == "off8":      # 8 bytes off 16-byte alignment
        v.p = BASE + 8
    elif layout == "nchw":
        v.ps, v.rs, v.cs, v.bs = 1, W, H * W, C * H * W
    return v


def g_extent(which, Hd, Wd):
    return {"2x": (2 * Hd, 2 * Wd), "+1": (Hd + 1, Wd + 1), "neither": (2 * Hd + 1, 2 * Wd + 1)}[which]


def shapes(reduced):
    m = REDUCED if reduced else {}
    return itertools.product(DTYPES, m.get("batches", BATCHES), m.get("grids", GRIDS), m.get("rs", RS), m.get("cgs", CGS))


def route(lib, dtype, B, stride, D, R, rows, G, Cg, prologue, pad, force):
    """(rc, workspace bytes, plan, kernel, reduce, name) of stc_conv_wgrad_route."""
    ws, plan, kr, name = ctypes.c_int64(), (ctypes.c_int32 * 5)(), (ctypes.c_int32 * 2)(), ctypes.create_string_buffer(96)
    fp = (ctypes.c_int32 * 2)(*force) if force else None
    rc = lib.stc_conv_wgrad_route(dtype, B, stride, D, R, rows, G, Cg, Cg, prologue, pad, fp, ctypes.byref(ws), plan, kr,
                                  name, 96)
    return rc, ws.value, list(plan), kr[0], kr[1], name.value.decode()


def run(lib, out, reduced, old_only):
    digests = {}
    count = [0]
    pairs = collections.Counter()
    bound, misses = {}, []

    def emit(section, line):
        data = (section + " " + line + "\n").encode()
        digests.setdefault(section, hashlib.sha256()).update(data)
        count[0] += 1
        if out:
            out.write(data)

    plan = (ctypes.c_int32 * 5)()
    ws = ctypes.c_int64()
    for dtype, B, (Hd, Wd), R, Cg in shapes(reduced):
        key = "%s B=%d D=%dx%d R=%d Cg=%d" % ("bf16" if dtype else "f32", B, Hd, Wd, R, Cg)
        emit("workspace", "%s -> %d" % (key, lib.stc_conv_wgrad_workspace(dtype, B, Hd, Wd, R, Cg)))
        for rows in (1, 2):
            emit("rows_workspace", "%s rows=%d -> %d" % (key, rows, lib.stc_conv_wgrad_rows_workspace(B, Hd + 1, rows, Cg)))
        for force in FORCES:
            fp = (ctypes.c_int32 * 2)(*force) if force else None
            rc = lib.stc_conv_wgrad_query(dtype, B, Hd, Wd, R, Cg, fp, ctypes.byref(ws), plan)
            emit("query", "%s force=%s -> rc=%d ws=%d plan=%s" % (key, force, rc, ws.value, list(plan)))
            bound[key, force] = ws.value
            for kind, pad in itertools.product((CONV_S2, CONV_S1), (ZEROS, REFLECT)):
                if pad == REFLECT and force:
                    continue  # (refused: no plan can be forced under reflect)
                rc = lib.stc_conv_pad_wgrad_query(dtype, kind, pad, B, Hd, Wd, R, Cg, fp, ctypes.byref(ws), plan)
                emit("pad_query", "%s s%d pad=%d force=%s -> rc=%d ws=%d plan=%s" % (
                    key, 2 - kind, pad, force, rc, ws.value, list(plan)))
    if old_only or not hasattr(lib, "stc_conv_wgrad_route"):
        return count[0], digests, pairs, misses
    # the route of actual views: every layout and G grid; rows, prologue and reflect with the automatic plan
    for dtype, B, (Hd, Wd), R, Cg in shapes(reduced):
        key = "%s B=%d D=%dx%d R=%d Cg=%d" % ("bf16" if dtype else "f32", B, Hd, Wd, R, Cg)
        for layout, gg, stride in itertools.product(LAYOUTS, G_GRIDS, (2, 1)):
            D, G = view(layout, Hd, Wd, R), view(layout, *g_extent(gg, Hd, Wd), Cg)
            for force in FORCES:
                asks = [(0, 0, ZEROS)] if force else [(r, p, ZEROS) for r in (0, 1, 2) for p in (0, 1)] + [(0, 0, REFLECT)]
                for rows, pro, pad in asks:
                    rc, w, pl, k, rd, name = route(lib, dtype, B, stride, D, R, rows, G, Cg, pro, pad, force)
                    pairs[(KERNELS[k], REDUCES[rd])] += 1
                    if pad == ZEROS and KERNELS[k] not in ("WG_ROWS", "WG_ROWS_MFMA") and w > bound[key, force]:
                        misses.append("%s s%d views=%s G=%s rows=%d pro=%d force=%s: route %d > query %d" % (
                            key, stride, layout, gg, rows, pro, force, w, bound[key, force]))
                    emit("route", "%s s%d views=%s G=%s rows=%d pro=%d pad=%d force=%s -> rc=%d ws=%d plan=%s %s %s %s" % (
                        key, stride, layout, gg, rows, pro, pad, force, rc, w, pl, KERNELS[k], REDUCES[rd], name))
    return count[0], digests, pairs, misses


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("library")
    ap.add_argument("--out", help="write the table here")
    ap.add_argument("--reduced", action="store_true", help="a small matrix (seconds)")
    ap.add_argument("--old-only", action="store_true", help="only the queries every build has")
    args = ap.parse_args()
    lib = load(args.library)
    out = open(args.out, "wb") if args.out else None
    n, sections, pairs, misses = run(lib, out, args.reduced, args.old_only)
    if out:
        out.close()
    print("lines %d" % n)
    for name in sorted(sections):
        print("section %-14s %s" % (name, sections[name].hexdigest()))
    for (k, r), c in sorted(pairs.items()):
        print("pair %-13s %-9s %d" % (k, r, c))
    if not args.old_only:
        print("route workspace above the stride-less query's: %d asks" % len(misses))
        for m in misses[:20]:
            print("  " + m)
    return 1 if misses else 0


if __name__ == "__main__":
    sys.exit(main())
