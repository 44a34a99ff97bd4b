"""The conv dispatch's host-only entry points agree with each other (no GPU: they only compute).

One route function answers all of them (csrc/conv_route.cpp); these are the agreements a caller
relies on -- a query that drifted from the launch is a hard error in the middle of a train step.  The full table of
answers is scripts/conv_route_table.py.
"""
import ctypes
import itertools

import pytest

F32, BF16 = 0, 1
CONV_S2, CONV_S1, CONVT_S2, CONV_S1_DGRAD = 0, 1, 2, 3
SHAPES = list(itertools.product((F32, BF16), (CONV_S2, CONV_S1, CONVT_S2, CONV_S1_DGRAD), (1, 2, 32),
                                (1, 2, 4, 8, 16, 31, 32, 64, 128), (8, 64, 128, 512, 1024), (1, 8, 16, 64, 128, 512)))


@pytest.fixture(scope="module")
def lib():
    from stcgan_amd import _lib
    h = ctypes.CDLL(_lib.LIB_PATH)
    i, vp = ctypes.c_int, ctypes.c_void_p
    h.stc_conv_fwd_workspace.restype = ctypes.c_int64
    h.stc_conv_fwd_workspace.argtypes = [i] * 7
    h.stc_conv_fwd_plan.argtypes = [i] * 7 + [vp]
    h.stc_conv_fwd_query.argtypes = [i] * 8 + [vp] * 4
    h.stc_conv_bwd_bn_chunks.argtypes = [i] * 9
    h.stc_conv_bwd_bn_chunks_ex.argtypes = [i, i, i, _lib.View, i, i, _lib.View, vp]
    h.stc_set_splitk_inlaunch.argtypes = [i]
    return h


def query(lib, shape, out_f32=0):
    dtype, kind, B, g, Cin, Cout = shape
    ws, nch, plan = ctypes.c_int64(), ctypes.c_int32(), (ctypes.c_int32 * 5)()
    assert lib.stc_conv_fwd_query(dtype, kind, B, g, g, Cin, Cout, out_f32, None, ctypes.byref(ws), ctypes.byref(nch),
                                  plan) == 0
    return ws.value, nch.value, list(plan)


def extents(kind, g):
    """input and output extent of a conv kind for the GEMM grid g x g"""
    return {CONV_S2: (2 * g, g), CONV_S1: (g + 1, g), CONVT_S2: (g, 2 * g), CONV_S1_DGRAD: (g - 1, g)}[kind]


def dense(n, C):
    from stcgan_amd import _lib
    return _lib.View(1 << 20, n, n, n * n * C, n * C, C, 0, 1, 0)  # (a 16-byte aligned stand-in: never dereferenced)


def test_plan_is_the_head_of_the_query_plan(lib):
    out = (ctypes.c_int32 * 4)()
    for shape in SHAPES:
        dtype, kind, B, g, Cin, Cout = shape
        assert lib.stc_conv_fwd_plan(dtype, kind, B, g, g, Cin, Cout, out) == 0
        assert list(out) == query(lib, shape)[2][:4], shape


def test_workspace_covers_the_query_workspace(lib):
    for shape in SHAPES:
        dtype, kind, B, g, Cin, Cout = shape
        assert lib.stc_conv_fwd_workspace(dtype, kind, B, g, g, Cin, Cout) >= query(lib, shape)[0], shape


def test_shape_chunks_equal_view_chunks_on_dense_views(lib):
    """stc_conv_bwd_bn_chunks (shape only) is stc_conv_bwd_bn_chunks_ex on dense, offset-0, aligned views with no second
    gradient -- except where the dense input view is 2 GiB or more, which a shape cannot know: there the shape form
    keeps the fused kernel's count and the view form answers for the unfused path that then runs."""
    from stcgan_amd import _lib
    excluded, differ = [], []
    for shape in SHAPES:
        dtype, kind, B, g, Cin, Cout = shape
        xin, xout = extents(kind, g)
        if xin < 1:
            continue
        x, y = dense(xin, Cin), dense(xout, Cout)
        f = _lib.BnbFuse(x=dense(xout, Cout), C=Cout, ch_off=0)
        by_shape = lib.stc_conv_bwd_bn_chunks(dtype, kind, B, g, g, Cin, Cout, xout, xout)
        by_view = lib.stc_conv_bwd_bn_chunks_ex(dtype, kind, B, x, Cin, Cout, y, ctypes.byref(f))
        if B * x.bs * 2 < 2 ** 31:
            assert by_shape == by_view, shape
        else:
            excluded.append(shape)
            if by_shape != by_view:
                differ.append(shape)
    # the excluded cases: Conv2d s2 of a 256 x 256 input at batch 32 with 512 or 1024 input channels
    assert excluded == [s for s in SHAPES if s[1:4] == (CONV_S2, 32, 128) and s[4] >= 512]
    assert len(excluded) == 24
    # ... of which the bf16 ones with a fused kernel (Cout >= 16) answer differently
    assert differ == [s for s in excluded if s[0] == BF16 and s[5] >= 16]
    assert len(differ) == 8


def test_inlaunch_switch_moves_split_layers_only(lib):
    old = lib.stc_set_splitk_inlaunch(-1)
    moved = 0
    try:
        answers = []
        for on in (0, 1):
            lib.stc_set_splitk_inlaunch(on)
            answers.append([(query(lib, s), lib.stc_conv_bwd_bn_chunks(*s[:3], s[3], s[3], s[4], s[5], extents(s[1], s[3])[1],
                                                                       extents(s[1], s[3])[1])) for s in SHAPES])
        for shape, off, on in zip(SHAPES, *answers):
            assert off[0][2] == on[0][2], shape   # the plan does not depend on the switch
            if off != on:
                moved += 1
                assert shape[0] == BF16 and on[0][2][2] > 1, shape   # a split-K layer of the bf16 tile
    finally:
        lib.stc_set_splitk_inlaunch(old)
    assert moved > 0
    assert lib.stc_set_splitk_inlaunch(-1) == old
