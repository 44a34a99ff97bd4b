"""The weight-gradient dispatch's host-only entry points agree with each other (no GPU: they only compute).

One route function answers all of them (csrc/wgrad_route.cpp): stc_conv_wgrad_route for a call's
actual views and stride, the stride-less queries for a D grid.  These are the agreements ops.wgrad and the scripts
rely on.  The full table of answers is scripts/wgrad_route_table.py.
"""
import ctypes
import functools
import itertools

import pytest

F32, BF16 = 0, 1
ZEROS, REFLECT = 0, 1
CONV_S2, CONV_S1 = 0, 1
WG_NONE, WG_FP_TILE, WG_BF16_TILE, WG_BF16_LD, WG_HALO, WG_ROWS, WG_ROWS_MFMA = range(7)
GRIDS = [(g, g) for g in (1, 2, 4, 8, 15, 16, 30, 31, 32, 62, 64, 128)] + [(4, 5), (31, 32)]
SHAPES = list(itertools.product((F32, BF16), (1, 2, 5, 32), GRIDS, (8, 16, 64, 96, 128, 256, 512),
                                (8, 16, 64, 128, 256, 512)))  # dtype, B, D grid, R, Cg
FORCES = [None, (-1, 0), (-1, -1)] + [(c, 0) for c in range(9)] + [(7, 4), (8, 2)]
LAYOUTS = ("dense", "concat", "co8", "rowpad", "off8", "nchw")
G_GRIDS = ("2x", "+1", "neither")


@pytest.fixture(scope="module")
def lib():
    from stcgan_amd import _lib
    h = ctypes.CDLL(_lib.LIB_PATH)
    i, vp = ctypes.c_int, ctypes.c_void_p
    h.stc_conv_wgrad_query.argtypes = [i] * 6 + [vp] * 3
    h.stc_conv_wgrad_workspace.restype = ctypes.c_int64
    h.stc_conv_wgrad_workspace.argtypes = [i] * 6
    h.stc_conv_pad_wgrad_query.argtypes = [i] * 8 + [vp] * 3
    h.stc_conv_wgrad_rows_workspace.restype = ctypes.c_int64
    h.stc_conv_wgrad_rows_workspace.argtypes = [i] * 4
    h.stc_conv_wgrad_route.argtypes = [i, i, i, _lib.View, i, i, _lib.View, i, i, i, i, vp, vp, vp, vp, vp, i]
    return h


_ws, _plan, _kr, _name = ctypes.c_int64(), (ctypes.c_int32 * 5)(), (ctypes.c_int32 * 2)(), ctypes.create_string_buffer(96)
_wsp = ctypes.byref(_ws)


@functools.lru_cache(maxsize=None)
def _force(f):
    return (ctypes.c_int32 * 2)(*f) if f else None


def query(lib, dtype, B, Hd, Wd, R, Cg, force=None):
    assert lib.stc_conv_wgrad_query(dtype, B, Hd, Wd, R, Cg, _force(force), _wsp, _plan) == 0
    return _ws.value, list(_plan)


def route(lib, dtype, B, stride, D, R, G, Cg, rows=0, pro=0, pad=ZEROS, force=None, Cg_out=None):
    """(workspace bytes, plan, kernel, reduce, name) of stc_conv_wgrad_route"""
    assert lib.stc_conv_wgrad_route(dtype, B, stride, D, R, rows, G, Cg, Cg if Cg_out is None else Cg_out, pro, pad,
                                    _force(force), _wsp, _plan, _kr, _name, 96) == 0
    return _ws.value, list(_plan), _kr[0], _kr[1], _name.value.decode()


@functools.lru_cache(maxsize=None)
def view(layout, H, W, C):
    from stcgan_amd import _lib
    v = _lib.View(1 << 20, H, W, H * W * C, W * C, C, 0, 1, 0)  # (a 16-byte aligned stand-in: never dereferenced)
    if layout == "concat":
        v.ps, v.co, v.rs, v.bs = 2 * C, C, W * 2 * C, H * W * 2 * C
    elif layout == "co8":
        v.ps, v.co, v.rs, v.bs = C + 16, 8, W * (C + 16), H * W * (C + 16)
    elif layout == "rowpad":
        v.rs, v.bs = (W + 1) * C, H * (W + 1) * C
    elif layout == "off8":
        v.p = (1 << 20) + 8
    elif layout == "nchw":
        v.ps, v.rs, v.cs, v.bs = 1, W, H * W, C * H * W
    return v


def g_extent(which, Hd, Wd):
    return {"2x": (2 * Hd, 2 * Wd), "+1": (Hd + 1, Wd + 1), "neither": (2 * Hd + 1, 2 * Wd + 1)}[which]


def in_2g(B, *views):
    """The bf16 LDS-DMA kernels address a view with 32 bits: below 2 GiB, which the stride-less queries (a shape has no
    allocation) count as met"""
    return all(B * v.bs * 2 < 1 << 31 for v in views)


def test_workspace_is_the_query_workspace(lib):
    """(a)"""
    for dtype, B, (Hd, Wd), R, Cg in SHAPES:
        assert lib.stc_conv_wgrad_workspace(dtype, B, Hd, Wd, R, Cg) == query(lib, dtype, B, Hd, Wd, R, Cg)[0]


def test_query_workspace_covers_every_route(lib):
    """(b) What the stride-less query reports is enough for the call that then runs, whatever its stride, G grid,
    layout, prologue or forced plan.  Every stride and G grid on dense views for every shape; the prologue, the other
    layouts and the forced plans with G on the stride's grid, for a part of the shapes (the whole cross is
    scripts/wgrad_route_table.py)."""
    on_grid = ((2, "2x"), (1, "+1"))
    for dtype, B, (Hd, Wd), R, Cg in SHAPES:
        have = query(lib, dtype, B, Hd, Wd, R, Cg)[0]
        D = view("dense", Hd, Wd, R)
        asks = [("dense", s, gg, p, None) for s, gg in itertools.product((2, 1), G_GRIDS) for p in (0, 1)
                if not p or (s, gg) in on_grid]
        if B in (1, 32) and R in (8, 128, 512):
            asks += [(lay, s, gg, 0, None) for lay in LAYOUTS[1:] for s, gg in on_grid]
        if B in (1, 32) and Cg in (8, 64, 256):
            asks += [("dense", s, gg, 0, f) for s, gg in on_grid for f in FORCES[1:]]
        for layout, stride, gg, pro, f in asks:
            D, G = view(layout, Hd, Wd, R), view(layout, *g_extent(gg, Hd, Wd), Cg)
            limit = have if f is None else query(lib, dtype, B, Hd, Wd, R, Cg, f)[0]
            need = route(lib, dtype, B, stride, D, R, G, Cg, 0, pro, ZEROS, f)[0]
            assert need <= limit, (dtype, B, Hd, Wd, R, Cg, layout, gg, stride, f, pro, need, limit)


def test_pad_query(lib):
    """(c) With STC_PAD_ZEROS the pad query is the plain query; a reflect call runs the register-staged kernel
    whatever the dtype, and its query answers for it."""
    for dtype, B, (Hd, Wd), R, Cg in SHAPES:
        plain = query(lib, dtype, B, Hd, Wd, R, Cg)
        for kind in (CONV_S2, CONV_S1):
            assert lib.stc_conv_pad_wgrad_query(dtype, kind, ZEROS, B, Hd, Wd, R, Cg, None, _wsp, _plan) == 0
            assert (_ws.value, list(_plan)) == plain
            assert lib.stc_conv_pad_wgrad_query(dtype, kind, REFLECT, B, Hd, Wd, R, Cg, None, _wsp, _plan) == 0
            refl = (_ws.value, list(_plan))
            stride = 2 if kind == CONV_S2 else 1
            D, G = view("dense", Hd, Wd, R), view("dense", *g_extent("2x" if stride == 2 else "+1", Hd, Wd), Cg)
            ws, plan, kernel, _, name = route(lib, dtype, B, stride, D, R, G, Cg, pad=REFLECT)
            assert kernel == WG_FP_TILE and name == "wgrad_reflect_kernel" and (ws, plan) == refl
    # a forced plan under reflect is refused, as by stc_conv_pad_wgrad and its query
    D, G = view("dense", 4, 4, 8), view("dense", 8, 8, 8)
    assert lib.stc_conv_wgrad_route(BF16, 2, 2, D, 8, 0, G, 8, 8, 0, REFLECT, _force((0, 0)), _wsp, _plan, _kr, _name, 96) != 0


def test_query_plan_is_the_route_plan(lib):
    """(d) The stride-less query reports the plan of the stride-2 call with G on the doubled grid.  The one exception is
    as old as the stride-1 halo tile: a 31-wide D grid of odd height, which no stride-2 conv of an even extent
    produces, reports the stride-1 plan (the PatchGAN's layer 4; tests/test_gpu_igemm_bf16.py pins it)."""
    for (dtype, B, (Hd, Wd), R, Cg), f in itertools.product(SHAPES, FORCES):
        if B not in (1, 32) and f is not None:
            continue
        plan = query(lib, dtype, B, Hd, Wd, R, Cg, f)[1]
        D, G2 = view("dense", Hd, Wd, R), view("dense", 2 * Hd, 2 * Wd, Cg)
        s2 = route(lib, dtype, B, 2, D, R, G2, Cg, force=f)
        if dtype == BF16 and not in_2g(B, D, G2):  # (the query's plan, the register-staged kernel's workspace)
            assert s2[2] == WG_FP_TILE and plan[0] >= 0
            continue
        if Wd != 31:
            assert plan == s2[1], (dtype, B, Hd, Wd, R, Cg, f)
            continue
        s1 = route(lib, dtype, B, 1, D, R, view("dense", Hd + 1, Wd + 1, Cg), Cg, force=f)
        assert plan in (s1[1], s2[1])
        if s1[2] == WG_HALO:
            assert plan == s1[1] and plan[0] == 8
        if not (dtype == BF16 and Hd % 2 == 1 and R >= 96 and Cg % 16 == 0):
            assert plan == s2[1]


def rows_today(dtype, B, stride, D, R, G, Cg, rows, pro, force):
    """Where ops.wgrad went to the rows kernels before the route decided it (its condition, literal constants
    included, rows_kernel on), and where stc_conv_wgrad_rows then took the call (its own checks)."""
    python = (rows is not None and rows <= 2 and stride == 1 and not pro and force is None and Cg % 64 == 0
              and ((D.H + 4) * (D.W + 4) + 16384) * rows <= 40000)
    entry = (dtype in (F32, BF16) and 1 <= rows <= 2 and rows <= R and Cg % 64 == 0 and G.cs == 1 and G.co % 4 == 0
             and G.ps % 4 == 0 and D.cs == 1 and D.H == G.H - 1 and D.W == G.W - 1)
    lds = ((rows * (D.H + 4) * (D.W + 4) + 3) // 4 * 4 + 16 * rows * 16 * 64) * 4
    parts = (G.H + 15) // 16
    mfma = (dtype == BF16 and G.ps % 8 == 0 and G.co % 8 == 0 and G.W <= 32 and G.H <= 32 and parts <= 4
            and rows * D.H * D.W <= 2048 and 16 * 32 * 128 + rows * 4 * (D.H + 5) * 40 * 2 <= 96 * 1024
            and B * G.bs * 2 < 1 << 31)
    if not (python and entry and (mfma or lds <= 160 * 1024)):
        return WG_NONE
    return WG_ROWS_MFMA if mfma else WG_ROWS


def test_rows_route(lib):
    """(e) The rows kernels are chosen exactly where the Python condition of old and stc_conv_wgrad_rows's own checks
    both hold; their workspace is stc_conv_wgrad_rows_workspace."""
    seen = set()
    for dtype, B, (Hd, Wd), R, Cg in SHAPES:
        if R not in (8, 512) or B == 5:  # (R matters only through rows <= R)
            continue
        for layout, gg in itertools.product(LAYOUTS, G_GRIDS):
            D, G = view(layout, Hd, Wd, R), view(layout, *g_extent(gg, Hd, Wd), Cg)
            asks = [(1, 1, 0, None), (1, 2, 0, None)]
            if layout == "dense" and gg == "+1":  # what turns the rows kernels off: stride 2, a prologue, a forced plan
                asks += [(2, 1, 0, None), (1, 1, 1, None), (1, 2, 0, (-1, 0))]
            for stride, rows, pro, f in asks:
                ws, _, kernel, _, name = route(lib, dtype, B, stride, D, R, G, Cg, rows, pro, ZEROS, f)
                want = rows_today(dtype, B, stride, D, R, G, Cg, rows, pro, f)
                got = kernel if kernel in (WG_ROWS, WG_ROWS_MFMA) else WG_NONE
                assert got == want, (dtype, B, Hd, Wd, R, Cg, layout, gg, stride, rows, pro, f, kernel)
                if want:
                    seen.add(want)
                    assert ws == lib.stc_conv_wgrad_rows_workspace(B, G.H, rows, Cg)
                    assert name == ("wgrad_rows_mfma_kernel" if want == WG_ROWS_MFMA else "wgrad_rows_kernel")
    assert seen == {WG_ROWS, WG_ROWS_MFMA}
    # rows = 0 (not asked, or the rows kernels off): never
    D, G = view("dense", 4, 4, 8), view("dense", 5, 5, 64)
    assert route(lib, BF16, 1, 1, D, 8, G, 64, rows=1)[2] == WG_ROWS_MFMA
    assert route(lib, BF16, 1, 1, D, 8, G, 64, rows=0)[2] == WG_BF16_TILE
    assert route(lib, BF16, 1, 1, D, 8, G, 64, rows=3)[2] == WG_BF16_TILE


# the timer label ops.py built from the query's plan before the route carried the name (a copy: the package has none)
_WB_TILES = [(128, 128, 2, 2, "false"), (64, 128, 1, 4, "false"), (128, 16, 4, 1, "true"), (256, 256, 2, 4, "false"),
             (256, 128, 4, 2, "false"), (128, 256, 2, 4, "false"), (128, 128, 2, 2, "false", 4, 4),
             (128, 128, 2, 2, "false", 4, 3),
             (128, 256, 2, 2, "false", -2, 4)]  # (BM, BN, WM, WN, swapped[, loader waves (-2: halo), stages])


def _wgrad_kernel_name(plan, Hd, Wd):
    cfg = plan[0]
    if cfg < 0:
        return "wgrad_kernel"
    bm, bn, wm, wn, sw = _WB_TILES[cfg][:5]
    ld, nst = _WB_TILES[cfg][5:] if len(_WB_TILES[cfg]) > 5 else (0, 2)
    ghw = Hd * Wd
    pow2 = lambda v: v > 0 and (v & (v - 1)) == 0  # noqa: E731
    fast = Wd % 64 == 0 or (pow2(Wd) and ghw % 64 == 0) or (pow2(ghw) and pow2(Wd) and 64 % ghw == 0)
    fast = fast and cfg != 3  # the 256x256 tile keeps the general addressing (register budget)
    if ld == -2:  # (the stride-1 halo tile: a 31-wide grid run as 32 x 32)
        return "wgrad_halo_kernel<32, true>" if Wd == 31 else f"wgrad_halo_kernel<{min(Wd, 64)}, false>"
    if ld:
        return f"wgrad_bf16_ld_kernel<{bm}, {bn}, {wm}, {wn}, {sw}, {str(fast).lower()}, {ld}, {nst}>"
    return f"wgrad_bf16_kernel<{bm}, {bn}, {wm}, {wn}, {sw}, {str(fast).lower()}>"


def test_route_name_is_the_label_of_its_own_plan(lib):
    """(f) For every GEMM route (not the rows kernels, not reflect) the name is what the label function of old gives
    for the route's own plan and D grid; and the kernel code agrees with the name."""
    family = {"wgrad_kernel": WG_FP_TILE, "wgrad_bf16_kernel": WG_BF16_TILE, "wgrad_bf16_ld_kernel": WG_BF16_LD,
              "wgrad_halo_kernel": WG_HALO}
    for (dtype, B, (Hd, Wd), R, Cg), f in itertools.product(SHAPES, FORCES):
        if B not in (1, 32) and f is not None:
            continue
        D = view("dense", Hd, Wd, R)
        for stride, gg, pro in ((2, "2x", 0), (1, "+1", 0), (2, "neither", 0), (1, "+1", 1)):
            if f is not None and pro:
                continue
            _, plan, kernel, _, name = route(lib, dtype, B, stride, D, R, view("dense", *g_extent(gg, Hd, Wd), Cg), Cg,
                                             pro=pro, force=f)
            assert name == _wgrad_kernel_name(plan, Hd, Wd), (dtype, B, Hd, Wd, R, Cg, f, stride, gg, pro)
            assert family[name.split("<")[0]] == kernel


def test_forced_config_the_geometry_does_not_allow(lib):
    """(g) A forced halo config falls back to the automatic plan where the geometry does not allow the halo tile
    (a G off the stride's grid included), splits and all; an unknown config is the automatic plan too, {-1, -1} without
    the channel-group-major direct store."""
    took = fell = 0
    for dtype, B, (Hd, Wd), R, Cg in SHAPES:
        if dtype != BF16:
            continue
        D = view("dense", Hd, Wd, R)
        for stride, gg in ((2, "2x"), (1, "+1"), (2, "neither"), (2, "+1"), (1, "2x")):
            G = view("dense", *g_extent(gg, Hd, Wd), Cg)
            auto = route(lib, BF16, B, stride, D, R, G, Cg)
            assert route(lib, BF16, B, stride, D, R, G, Cg, force=(-1, 0)) == auto
            assert route(lib, BF16, B, stride, D, R, G, Cg, force=(9, 3)) == auto
            on_grid = (stride, gg) in ((2, "2x"), (1, "+1"))
            ok = on_grid and in_2g(B, D, G) and Cg % 16 == 0 and R >= 96 and (
                (stride == 1 and Wd == 31 and Hd % 2 == 1) or
                (stride == 2 and Wd in (8, 16, 32, 64, 128) and Hd % (64 // min(Wd, 64)) == 0))
            for f in ((8, 0), (8, 2)):
                forced = route(lib, BF16, B, stride, D, R, G, Cg, force=f)
                if ok:
                    took += 1
                    assert forced[2] == WG_HALO and forced[1][0] == 8
                else:
                    fell += 1
                    assert forced == auto, (B, Hd, Wd, R, Cg, stride, gg, f)
            nocm = route(lib, BF16, B, stride, D, R, G, Cg, force=(-1, -1))
            assert nocm[1][:4] == auto[1][:4] and nocm[2] == auto[2]  # (the same tile and splits; slab may differ)
    assert took and fell
