"""stc_bn_bwd_frozen / stc_bn_running_rstd (csrc/bn.hip) against tests/bn_frozen_ref.py, by the method of
tests/test_gpu_bn_family.py: the reference is evaluated in fp64 from exactly the values uploaded (fp32, or
bf16-rounded activations; fp32 tables), every view has a NaN surround that must survive, and note() prints each worst
error / bound.

Bounds (EPS32 = 2^-23), from the accumulation lengths and the number formats as that file's docstring derives them:
element-wise dx within one fp32 ulp of the exact value (2^-23 |ref|: dn is formed with one rounding -- the slope-0
term is exact and the second term enters through an fma; a dropout factor on a single gradient adds one -- and the
product with scale rounds once more, two half-ulp roundings), bf16 the round-to-nearest-even of such a value; a
chunk's partial sums within m * EPS32 * sum|terms| with m = ceil(per / RL) + RL + 8; dgamma / dbeta within
4 * EPS32 * sum|partials| of the fp64 sum of the device's own partials, and within m * EPS32 * sum|terms| of the
exact sums.

Measured worst error / bound on an MI355X: see profiles/frozen_norm/test_ratios.txt.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import bn_frozen_ref as R
import dropout_ref as DR
import test_gpu_bn_family as Fam
from stcgan_amd import _lib as L
from stcgan_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, BF16 = torch.float32, torch.bfloat16
NAN = float("nan")
EPS32 = Fam.EPS32
note, place, new_buf, read_back, view_of = Fam.note, Fam.place, Fam.new_buf, Fam.read_back, Fam._view
dtname = Fam.dtname

# thread layouts CG = C / N of 1, 3 (fp32) and 24, 256 (bf16); P = 30 (one chunk), 216 (4 chunks), and 65537 pixels
# (1024 chunks of 65 with empty tail chunks) at the narrowest C
CHANNELS = {F32: (4, 12), BF16: (192, 2048)}
PIXELS = [(2, 3, 5), (3, 9, 8)]
SHAPES = [(dt, bhw + (C,)) for dt in (F32, BF16) for C in CHANNELS[dt] for bhw in PIXELS] + [(F32, (1, 1, 65537, 4))]
# view mixes (x, g1, g2, dx): all dense; the up path's (g1 in channels [C, 2C) of a concat gradient, dx likewise into
# a wider buffer); cropped x / g2 / dx with a dense g1
MIXES = {"dense": ("dense", "dense", "dense", "dense"), "hi": ("dense", "hi", "dense", "hi"),
         "crop": ("crop", "dense", "crop", "crop")}
# (g2 present, slope1, slope2): one gradient at slope 0; two at slopes 0 and 0.2
GRADS = [(False, 0.0, 0.0), (True, 0.0, 0.2)]


def _sid(shape):
    return "x".join(str(v) for v in shape)


def _shape_params(shapes=SHAPES):
    return [pytest.param(dt, shape, id=f"{dtname(dt)}-{_sid(shape)}") for dt, shape in shapes]


@functools.lru_cache(maxsize=None)
def case(shape, dt):
    """Stored x, hand-made fp32 tables (scale with negative entries, shift, a 'running mean' and 'rstd' unrelated to
    the data: the kernel takes them as given), two stored gradients.  No activation input lies within 0.09 of zero
    (Fam.apply_case asserts it), so no ReLU / LeakyReLU decision is rounding-sensitive."""
    C = shape[3]
    x, sc, sh, _ = Fam.apply_case(shape, dt, True)
    g = torch.Generator().manual_seed(190 + C)
    mean = (1.0 + 0.5 * torch.randn(C, generator=g)).float()
    rstd = (0.3 + 0.9 * torch.rand(C, generator=g)).float()
    g1, g2 = Fam.grads_for(shape, dt, 191 + C)
    return x, (sc, sh, mean, rstd), g1, g2


def frozen(B, xv, C, dt, dxv, g1v, s1, g2v, s2, state, sums=True, drop=None, nch=None):
    """stc_bn_bwd_frozen with buffers of the test's own: (partials or None, dgamma, dbeta).  sums=False hands the
    entry point no running mean / rstd, no partials buffer and nchunks = 0."""
    scale, shift, mean, rstd = state
    P = B * xv.H * xv.W
    part = dg = db = None
    if sums:
        nch = Fam.stat_chunks(P) if nch is None else nch
        part = torch.full((nch, C, 2), NAN, device=DEV)
        dg, db = torch.full((C,), NAN, device=DEV), torch.full((C,), NAN, device=DEV)
    else:
        mean = rstd = None
        nch = 0
    d = ops._drop(drop) if drop is not None else None
    ops.check(L.lib().stc_bn_bwd_frozen(L.dtype_code(dt), B, xv, C, L.ptr(scale), L.ptr(shift), L.ptr(mean),
                                        L.ptr(rstd), g1v if g1v is not None else L.NULL_VIEW, float(s1),
                                        g2v if g2v is not None else L.NULL_VIEW, float(s2),
                                        ctypes.byref(d) if d is not None else None, L.ptr(part), nch, dxv, L.ptr(dg),
                                        L.ptr(db), L.stream()), "stc_bn_bwd_frozen")
    return part, dg, db


def check_sums(tag, ref, part, dg, db, P, C, dt):
    nch = part.shape[0]
    m = Fam.acc_len(P, C, dt)
    val, absv = R.chunk_sums(ref, nch)
    pd = part.cpu().double()
    per = -(-P // nch)
    live = torch.tensor([k * per < P for k in range(nch)])
    assert bool((pd[~live] == 0).all()), "an empty tail chunk holds a sum"
    note(f"{tag}.partials", (pd - val).abs(), m * EPS32 * absv)
    merged = pd.sum(0)
    bound = 4 * EPS32 * pd.abs().sum(0)
    note(f"{tag}.merge.dbeta", (db.cpu().double() - merged[:, 0]).abs(), bound[:, 0])
    note(f"{tag}.merge.dgamma", (dg.cpu().double() - merged[:, 1]).abs(), bound[:, 1])
    note(f"{tag}.dbeta", (db.cpu().double() - ref["dbeta"]).abs(), m * EPS32 * ref["mag_beta"])
    note(f"{tag}.dgamma", (dg.cpu().double() - ref["dgamma"]).abs(), m * EPS32 * ref["mag_gamma"])


@pytest.mark.parametrize("mix", list(MIXES))
@pytest.mark.parametrize("dt,shape", _shape_params())
def test_frozen_backward(dt, shape, mix):
    """bn_bwd_frozen_sums_kernel<T, NoMask> (every thread layout, one / several chunks, empty tail chunks; both merge
    kernels) and bn_bwd_frozen_kernel<T, DENSE, NoMask> (streaming where every view is pixel-dense and 256 % CG == 0,
    general addressing otherwise): dx, the chunk partials, dgamma / dbeta; dx of the no-sums form equal to the sums
    form's bit for bit; a repeated call bit-identical; NaN surrounds intact."""
    x, state, g1, g2 = case(shape, dt)
    B, H, W, C = shape
    P = B * H * W
    mx, mg1, mg2, mdx = MIXES[mix]
    dev_state = tuple(t.to(DEV) for t in state)
    xb, xv = place(x, dt, mx)
    g1b, g1v = place(g1, dt, mg1)
    g2b, g2v = place(g2, dt, mg2)
    for two, s1, s2 in GRADS:
        ref = R.backward(x, *state, g1, s1, g2 if two else None, s2)
        dxb = new_buf(shape, dt, mdx)
        part, dg, db = frozen(B, xv, C, dt, view_of(dxb, shape, mdx), g1v, s1, g2v if two else None, s2, dev_state)
        tag = f"frozen.{dtname(dt)}"
        Fam.check_elementwise(f"{tag}.dx", read_back(dxb, shape, mdx), ref["dx"], dt)
        check_sums(tag, ref, part, dg, db, P, C, dt)
        # no parameter gradient wanted: the streaming pass, with no tables but scale / shift and no partials
        dxn = new_buf(shape, dt, mdx)
        assert frozen(B, xv, C, dt, view_of(dxn, shape, mdx), g1v, s1, g2v if two else None, s2, dev_state,
                      sums=False) == (None, None, None)
        Fam.check_elementwise(f"{tag}.dx.nosums", read_back(dxn, shape, mdx), ref["dx"], dt)
        assert torch.equal(Fam._region(dxn, shape, mdx), Fam._region(dxb, shape, mdx))
        # the public wrapper, again: the same bits
        dx2 = new_buf(shape, dt, mdx)
        dg2, db2 = ops.bn_backward_frozen(B, xv, C, dt, view_of(dx2, shape, mdx), g1v, s1, g2v if two else None, s2,
                                          state=dev_state)
        assert torch.equal(dg2, dg) and torch.equal(db2, db)
        assert torch.equal(Fam._region(dx2, shape, mdx), Fam._region(dxb, shape, mdx))
        dx3 = new_buf(shape, dt, mdx)
        assert ops.bn_backward_frozen(B, xv, C, dt, view_of(dx3, shape, mdx), g1v, s1, g2v if two else None, s2,
                                      state=dev_state, want_params=False) == (None, None)
        assert torch.equal(Fam._region(dx3, shape, mdx), Fam._region(dxb, shape, mdx))
    for buf, md in ((xb, mx), (g1b, mg1), (g2b, mg2)):  # (the inputs' surrounds untouched)
        read_back(buf, shape, md)


@pytest.mark.parametrize("dt,shape", _shape_params([(F32, (3, 9, 8, 12)), (BF16, (3, 9, 8, 192)),
                                                    (F32, (1, 1, 65537, 4))]))
def test_sums_equal_the_train_mode_reduce(dt, shape):
    """dgamma / dbeta of stc_bn_bwd_frozen are torch.equal to those of the existing reduce + finalize
    (ops.bn_backward) handed the same four tables: the same partition, the same terms in the same order."""
    x, state, g1, g2 = case(shape, dt)
    B, H, W, C = shape
    dev_state = tuple(t.to(DEV) for t in state)
    gamma = torch.ones(C, device=DEV)
    _, xv = place(x, dt, "dense")
    _, g1v = place(g1, dt, "hi")
    _, g2v = place(g2, dt, "dense")
    for two, s1, s2 in GRADS:
        dxa, dxb = new_buf(shape, dt, "dense"), new_buf(shape, dt, "dense")
        dg, db = ops.bn_backward_frozen(B, xv, C, dt, L.nhwc_view(dxa), g1v, s1, g2v if two else None, s2,
                                        state=dev_state)
        dg0, db0 = ops.bn_backward(B, xv, C, dt, L.nhwc_view(dxb), g1=g1v, s1=s1, g2=g2v if two else None, s2=s2,
                                   bn_state=dev_state + (gamma,))
        assert torch.equal(dg, dg0) and torch.equal(db, db0)
        assert not torch.equal(dxa, dxb)  # (the train-mode dx carries the batch terms)


# a level / extent pair of tests/test_gpu_dropout_family.py: level 7, the 3 x 4 x 6 extent cropped to 3 x 5
LEVEL, EXTENT, HW = 7, (3, 4, 6), (3, 5)


@pytest.mark.parametrize("sums", [True, False], ids=["sums", "nosums"])
@pytest.mark.parametrize("p,two", [(0.5, False), (0.5, True), (0.2, False)], ids=["p0.5", "p0.5-two", "p0.2"])
@pytest.mark.parametrize("dt,C", [(F32, 4), (F32, 12), (BF16, 192), (BF16, 2048)],
                         ids=["f32-cg1", "f32-cg3", "bf16-cg24", "bf16-cg256"])
def test_frozen_backward_dropout(dt, C, p, two, sums):
    """The PhiloxMask instantiations: g1 (the upper half of a concat gradient, as in the generator) times
    keep / (1 - p), the mask recomputed from the call's {seed, offset} over the full extent while x and dx are its
    cropped view.  p = 0.5: the factor 2 is exact, one or two gradients; p = 0.2: the factor 1.25 rounds g1 once,
    one gradient (what the generator's dropout levels have)."""
    B, (H, W) = EXTENT[0], HW
    shape = (B, H, W, C)
    x, state, g1, g2 = case(shape, dt)
    dev_state = tuple(t.to(DEV) for t in state)
    st = ops.dropout_state_tensor(DR.SEED, DR.OFFSET, DEV)
    drop = (st, LEVEL, p, EXTENT[1], EXTENT[2])
    f = R.drop_factor(DR.SEED, DR.OFFSET, LEVEL, EXTENT + (C,), HW, p)
    assert 0.0 < float((f == 0).double().mean()) < 1.0
    ref = R.backward(x, *state, g1, 0.0, g2 if two else None, 0.2, factor=f)
    _, xv = place(x, dt, "crop")
    _, g1v = place(g1, dt, "hi")
    _, g2v = place(g2, dt, "dense")
    dxb = new_buf(shape, dt, "crop")
    part, dg, db = frozen(B, xv, C, dt, view_of(dxb, shape, "crop"), g1v, 0.0, g2v if two else None, 0.2, dev_state,
                          sums=sums, drop=drop)
    tag = f"frozen.drop.{dtname(dt)}"
    Fam.check_elementwise(f"{tag}.dx", read_back(dxb, shape, "crop"), ref["dx"], dt)
    if sums:
        check_sums(tag, ref, part, dg, db, B * H * W, C, dt)
    # without the mask the result is another one
    plain = new_buf(shape, dt, "crop")
    frozen(B, xv, C, dt, view_of(plain, shape, "crop"), g1v, 0.0, g2v if two else None, 0.2, dev_state, sums=False)
    assert not torch.equal(Fam._region(plain, shape, "crop"), Fam._region(dxb, shape, "crop"))
    assert st.tolist() == [DR.SEED, DR.OFFSET]  # (the backward reads the call's counter; it advances nothing)


@pytest.mark.parametrize("C", [1, 5, 256, 257])
def test_running_rstd(C):
    """bn_running_rstd_kernel: 1 / sqrt(running_var + eps) within 2 fp32 ulp (add, sqrt, divide: the bound of
    test_eval_table in tests/test_gpu_bn_family.py, same inputs), and the eval table's scale is gamma times it,
    bit for bit."""
    g = torch.Generator().manual_seed(40 + C)
    bn = Fam._BN(C, 41 + C)
    rv = (10.0 ** (torch.rand(C, generator=g) * 9.0 - 6.0)).float()
    rv[0], rv[-1] = 1e-6, 1e3
    bn.running_var = rv.to(DEV)
    out = torch.full((C + 1,), NAN, device=DEV)
    rstd = ops.bn_running_rstd(C, bn, out=out[:C])
    assert bool(torch.isnan(out[C:]).all())
    ref = 1.0 / torch.sqrt(rv.double() + Fam.BN_EPS)
    note("frozen.rstd_run", (rstd.cpu().double() - ref).abs(), 2 * Fam.ulp32(ref))
    tab = torch.full((2, C), NAN, device=DEV)
    ops.bn_eval_table(C, bn, tab[0], tab[1])
    assert torch.equal(tab[0], bn.weight * rstd)


def test_bad_arguments_name_the_entry_point():
    """Refused calls raise with the entry point's name and write nothing."""
    B, H, W = 1, 3, 5
    x6, x8 = torch.randn(B, H, W, 6, device=DEV), torch.randn(B, H, W, 8, device=DEV)
    t8 = torch.ones(8, device=DEV)
    state8 = (t8, t8, t8, t8)
    st = ops.dropout_state_tensor(1, 2, DEV)

    def refused(fn, *outs):
        with pytest.raises(RuntimeError, match="stc_bn_bwd_frozen"):
            fn()
        torch.cuda.synchronize()
        for o in outs:
            assert bool(torch.isnan(o).all())

    y6 = torch.full((B, H, W, 6), NAN, device=DEV)  # C not a multiple of the 16-byte vector
    refused(lambda: ops.bn_backward_frozen(B, L.nhwc_view(x6), 6, F32, L.nhwc_view(y6), L.nhwc_view(x6), 0.0,
                                           state=state8), y6)
    y8 = torch.full((B, H, W, 8), NAN, device=DEV)
    xv, yv = L.nhwc_view(x8), L.nhwc_view(y8)
    # a dropout block without g1
    refused(lambda: ops.bn_backward_frozen(B, xv, 8, F32, yv, None, 0.0, g2=xv, s2=0.2, state=state8,
                                           drop=(st, 3, 0.5, H, W)), y8)
    refused(lambda: ops.bn_backward_frozen(B, xv, 8, F32, yv, None, 0.0, g2=xv, s2=0.2, state=state8,
                                           want_params=False, drop=(st, 3, 0.5, H, W)), y8)
    # sums wanted with a chunk count other than stat_chunks(P)
    for nch in (2, 0):
        refused(lambda: frozen(B, xv, 8, F32, yv, xv, 0.0, None, 0.0, state8, nch=nch), y8)
    # sums wanted without the running tables; a view outside the dropout extent; dx missing
    refused(lambda: ops.bn_backward_frozen(B, xv, 8, F32, yv, xv, 0.0, state=(t8, t8, None, t8)), y8)
    refused(lambda: ops.bn_backward_frozen(B, xv, 8, F32, yv, xv, 0.0, state=state8, drop=(st, 3, 0.5, H - 1, W)), y8)
    refused(lambda: ops.bn_backward_frozen(B, xv, 8, F32, L.NULL_VIEW, xv, 0.0, state=state8))
