"""The use_dropout=True kernels of csrc/bn.hip (bn_apply_drop_kernel, bn_bwd_reduce_kernel<T, PhiloxMask>,
bn_bwd_apply_drop_kernel, dropout_mask_kernel, dropout_next_kernel) and the mask function of csrc/philox.hpp against
the independent references of tests/dropout_ref.py: the numpy Philox for every keep bit, fp64 arithmetic on operands
chosen so that a correct kernel must EQUAL the reference (apply, the reduce's partials, dgamma, dbeta), and derived
bounds where rounding is unavoidable (real-valued sums, dx).  See that module's docstring for the constructions and
the bounds; none of them was chosen after looking at a kernel's output.

No expected value here comes from a kernel of the dropout family, with two stated exceptions: "p = 0 equals the plain
kernels bit for bit" and "the fused stc_conv_bn_fwd_drop equals its three separate calls bit for bit".  The BatchNorm
tables of the real-valued backward cases come from ops.bn_train_table (pinned by tests/test_gpu_bn_family.py) and
are read back: the reference uses the fp32 values the kernels receive.

Every output is a view of a larger NaN-filled buffer (everything inside written, nothing outside), channel-offset
inputs have NaN in the other channels, and the cases run in fp32 and bf16.  The pixel-index division beyond 2^24
pixels is the shared pix_bxy, which tests/test_gpu_bn_family.py pins on both sides (test_pixel_index_boundary); it is
deliberately not repeated here.

Measured on an MI355X: see DESIGN.md section 5 and profiles/dropout_family/.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from stcgan_amd import _lib as L
from stcgan_amd import ops

import dropout_ref as R
from dropout_ref import BF16, F32, assert_same, dtname, note

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")
DTS = [F32, BF16]


# ---------------------------------------------------------------- layouts
# dense: the tensor itself; lo / hi: channels [0, C) / [C, 2C) of a 2C-wide buffer; crop: the top-left H x W of the
# full extent [B, FH, FW, C].  Everything outside the view is NaN.
def new_buf(shape, dt, mode, full=None):
    B, H, W, C = shape
    dims = {"dense": (B, H, W, C), "lo": (B, H, W, 2 * C), "hi": (B, H, W, 2 * C)}.get(mode)
    if mode == "crop":
        dims = (B, full[0], full[1], C)
    return torch.full(dims, NAN, device=DEV, dtype=dt)


def region(buf, shape, mode):
    B, H, W, C = shape
    if mode == "dense":
        return buf
    if mode in ("lo", "hi"):
        c0 = 0 if mode == "lo" else C
        return buf[..., c0:c0 + C]
    return buf[:, :H, :W, :]


def view(buf, shape, mode):
    B, H, W, C = shape
    if mode == "dense":
        return L.nhwc_view(buf)
    if mode in ("lo", "hi"):
        return L.nhwc_view(buf, 0 if mode == "lo" else C)
    return L.nhwc_view(buf, 0, H, W)


def place(vals, dt, mode, full=None):
    """Upload the CPU values [B, H, W, C] in the layout ``mode``: (buffer, view)."""
    shape = tuple(vals.shape)
    buf = new_buf(shape, dt, mode, full)
    region(buf, shape, mode).copy_(vals.to(dt))
    return buf, view(buf, shape, mode)


def read_back(buf, shape, mode):
    """The view's elements on the CPU in the storage type, after asserting that everything outside is still NaN."""
    got = region(buf, shape, mode).detach().clone()
    rest = buf.detach().clone()
    region(rest, shape, mode).fill_(NAN)
    assert bool(torch.isnan(rest).all()), f"{mode}: an element outside the view was written"
    return got.cpu()


def state(seed=R.SEED, offset=R.OFFSET):
    return ops.dropout_state_tensor(seed, offset, DEV)


def case_params(cases):
    return [pytest.param(c, dt, id=f"{dtname(dt)}-{c.id}") for dt in DTS for c in cases]


# ================================================================ a. the mask export
def export_mask(st, level, shape, p):
    """stc_dropout_mask into the middle of a 0xAB-filled byte buffer: the mask, after asserting the guard bytes."""
    B, H, W, C = shape
    n = B * H * W * C
    buf = torch.full((n + 128,), 0xAB, dtype=torch.uint8, device=DEV)
    d = L.Dropout(st.data_ptr(), float(p), int(level), int(H), int(W), 0)
    ops.check(L.lib().stc_dropout_mask(ctypes.byref(d), B, C, ctypes.c_void_p(buf.data_ptr() + 64), L.stream()),
              "stc_dropout_mask")
    torch.cuda.synchronize()
    assert bool((buf[:64] == 0xAB).all()) and bool((buf[64 + n:] == 0xAB).all()), "a byte outside the mask was written"
    return buf[64:64 + n].reshape(shape).cpu().numpy()


BIG_MASK = (1, 1, 1, 4 * (2 * R.GRID_CAP + 257))  # the grid-stride loop runs three times, with a ragged end
MASK_CASES = [(s, lv) for s in ((1, 1, 1, 4), (3, 4, 6, 64)) for lv in (0, 7, 2 ** 31 - 1)] + [(BIG_MASK, 2 ** 31 - 1)]


@pytest.mark.parametrize("shape,level", MASK_CASES,
                         ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_mask_export_vs_numpy(shape, level):
    """dropout_mask_kernel against the numpy Philox at levels 0, 7 and 2^31 - 1, the seed 0xFFFFFFFFFFFFFFFD (a
    negative int64 in the device state), an offset with its high word set, every p of the family (0 and 1e-12 keep
    everything), one quad, a small extent, and 2 * 8192 * 256 + 257 quads (three trips of the grid-stride loop; this
    shape at the largest level only: the level is one counter word and does not meet the loop)."""
    st = state(R.SEED_TOP, R.OFFSET)
    assert int(st[0]) < 0 and int(st[1]) >> 32 == 1
    words = R.words_view(R.SEED_TOP, R.OFFSET, level, shape)
    index_set = R.words_at(R.SEED_TOP, R.OFFSET, level, shape, 0, 0, 0, np.arange(min(shape[3], 64)))
    assert np.array_equal(index_set, words[0, 0, 0, :64])
    for p in R.P_ALL:
        got = export_mask(st, level, shape, p)
        want = (words >= np.uint64(R.thresh(p))).astype(np.uint8)
        assert got.dtype == np.uint8
        bad = np.flatnonzero(got.reshape(-1) != want.reshape(-1))
        assert bad.size == 0, (f"p={p}: {bad.size} of {got.size} elements differ, first linear indices "
                               f"{bad[:8].tolist()}")
        if p in (0.0, 1e-12):
            assert bool(got.all())
    assert st.tolist() == [R.SEED_TOP - (1 << 64), R.OFFSET]  # the export reads the state, it does not advance it


# ================================================================ b / c. the apply
def run_apply(case, dt, drop):
    """bn_apply of the case into NaN-surrounded outputs: (y1, y2 or None) on the CPU."""
    x, sc, sh = R.apply_inputs(case, dt)
    shape, full = case.shape(dt), (case.FH, case.FW)
    xbuf, xv = place(x, dt, "crop", full)
    m1, m2 = R.OUTS[case.outs]
    y1 = new_buf(shape, dt, m1, full)
    y2 = new_buf(shape, dt, m2, full) if m2 else None
    tab = (sc.to(DEV), sh.to(DEV)) if case.table else None
    ops.bn_apply(case.B, xv, case.C(dt), dt, tab, view(y1, shape, m1), case.slopes[0],
                 view(y2, shape, m2) if m2 else None, case.slopes[1], drop=drop)
    assert_same(read_back(xbuf, shape, "crop"), x.to(dt), "the input")
    return read_back(y1, shape, m1), read_back(y2, shape, m2) if m2 else None


@pytest.mark.parametrize("case,dt", case_params(R.APPLY_CASES))
def test_apply_exact(case, dt):
    """bn_apply_drop_kernel on every thread layout (CG = 1, 3, 24, 64, 256), crop (none, one axis, both, one pixel),
    output arrangement (y1 / y2 in the upper half of a concat buffer or dense, y2 absent), slope pair, with and
    without a table, at p = 0.3 and on CG = 3 / 64 at p in {0.5, 0.2, 0.3, 0.9, 1 - 2^-24}: EQUAL to
    act(keep ? fl32(n * scale32) : 0) (bf16: its round-to-nearest-even) with the numpy mask at full-extent indices.
    The same call at p = 0 equals the plain kernel bit for bit, and the reference with everything kept."""
    x, sc, sh = R.apply_inputs(case, dt)
    keep = R.case_keep(case, dt)
    st = state(case.seed, R.case_offset(case, dt))
    got = run_apply(case, dt, (st, case.level, case.p, case.FH, case.FW))
    for y, s, name in zip(got, case.slopes, ("y1", "y2")):
        if y is not None:
            assert_same(y, R.apply_ref(x, sc, sh, keep, case.p, s, dt), f"{case.id} {name}")
    plain = run_apply(case, dt, None)
    zero = run_apply(case, dt, (st, case.level, 0.0, case.FH, case.FW))
    ones = torch.ones_like(keep)
    for a, b, s, name in zip(zero, plain, case.slopes, ("y1", "y2")):
        if a is not None:
            assert_same(a, b, f"{case.id} p=0 {name} vs the plain kernel")
            assert_same(a, R.apply_ref(x, sc, sh, ones, 0.0, s, dt), f"{case.id} p=0 {name}")


# ================================================================ d. the backward
def bwd_drop(B, xv, C, dt, dxv, g1v, s1, g2v, s2, st5, drop, part=None, nch=None):
    """stc_bn_bwd_reduce_drop + stc_bn_bwd_apply_drop through the C entry points, so that the reduce's partials are
    seen (part given: only the apply, on those partials).  Returns (part2 [nch, C, 2], dgamma, dbeta)."""
    l = L.lib()
    sc, sh, mean, rstd, gam = st5
    st, level, p, FH, FW = drop
    d = L.Dropout(st.data_ptr(), float(p), int(level), int(FH), int(FW), 0)
    g2v = g2v if g2v is not None else L.NULL_VIEW
    if part is None:
        nch = ops.stats_chunks(B, xv.H, xv.W)
        part = torch.full((nch, C, 2), NAN, device=DEV)
        ops.check(l.stc_bn_bwd_reduce_drop(L.dtype_code(dt), B, xv, C, L.ptr(sc), L.ptr(sh), L.ptr(mean), L.ptr(rstd),
                                           g1v, float(s1), g2v, float(s2), ctypes.byref(d), L.ptr(part), nch,
                                           L.stream()), "stc_bn_bwd_reduce_drop")
    dgamma = torch.full((C,), NAN, device=DEV)
    dbeta = torch.full((C,), NAN, device=DEV)
    ops.check(l.stc_bn_bwd_apply_drop(L.dtype_code(dt), B, xv, C, L.ptr(sc), L.ptr(sh), L.ptr(mean), L.ptr(rstd),
                                      L.ptr(gam), g1v, float(s1), g2v, float(s2), ctypes.byref(d), L.ptr(part), nch,
                                      dxv, L.ptr(dgamma), L.ptr(dbeta), L.stream()), "stc_bn_bwd_apply_drop")
    torch.cuda.synchronize()
    return part, dgamma, dbeta


class _BN:
    def __init__(self, C, seed):
        g = torch.Generator().manual_seed(seed)
        w = torch.rand(C, generator=g) + 0.5
        w[1::3] *= -1.0
        self.weight, self.bias = w.to(DEV), (torch.randn(C, generator=g) * 0.3).to(DEV)
        self.running_mean = (torch.randn(C, generator=g) * 0.1).to(DEV)
        self.running_var = (torch.rand(C, generator=g) + 0.5).to(DEV)
        self.num_batches_tracked = torch.zeros((), dtype=torch.long, device=DEV)
        self.momentum, self.eps = 0.1, 1e-5

    def clone(self):
        other = _BN.__new__(_BN)
        for k in ("weight", "bias", "running_mean", "running_var", "num_batches_tracked"):
            setattr(other, k, getattr(self, k).clone())
        other.momentum, other.eps = self.momentum, self.eps
        return other


def gpu_tables(case, dt):
    """(scale, shift, mean, rstd, gamma) of ops.bn_train_table on the case's unconditioned x, read back."""
    C, full = case.C(dt), (case.FH, case.FW)
    _, xv = place(R.real_x(case, dt), dt, "crop", full)
    bn = _BN(C, 300 + C)
    tab = torch.empty((2, C), device=DEV)
    mean, rstd = ops.bn_train_table(case.B, xv, C, dt, bn, tab[0], tab[1])
    return tuple(t.cpu() for t in (tab[0], tab[1], mean, rstd, bn.weight))


@pytest.mark.parametrize("case,dt", case_params(R.BWD_CASES))
def test_backward(case, dt):
    """bn_bwd_reduce_kernel<T, PhiloxMask> and bn_bwd_apply_drop_kernel (with the backward finalize between them) through
    the C entry points, on every thread layout (the idle lanes pl >= RL at CG = 3 and 24), cropped x and dx, g1 dense or
    the upper half of a 2C-wide NaN-surrounded buffer, g2 absent / dense / a lower half.
    exact cases (p = 0.5, 0.75, 0.2, 0.6): the partials, dgamma and dbeta EQUAL the fp64 sums; with slope 0.2 the
      term g2 * fl32(0.2) cannot be summed exactly and the sums take the derived bound (dropout_ref's docstring).
    real-valued cases (p = 0.3; tables from ops.bn_train_table): within m * EPS32 * sum|terms|; P = 65537 gives 1024
      chunks (asserted), so bn_bwd_finalize_kernel<BlockMerge> runs behind the drop reduce, with empty tail chunks.
    dx within 16 * EPS32 * (|k1 dn| + |k2 x| + |k0|) + |k1| * EPS32 * (2 |t1| + |t2|) of the fp64 value (bf16: inside
    the rounding interval of such a value).  The second part was added after the P = 65537 fp32 case missed the first
    alone by 7.9 x: a derivation error, not a kernel error -- a correctly rounded fp32 evaluation on the CPU misses
    it by 8.4 x where g1 * m and g2 cancel (dropout_ref's docstring; test_dx_bound_counts_the_terms_roundings).
    The same call at p = 0 equals the plain kernels bit for bit.
    Measured worst error / bound (MI355X): exact operands with slope 0.2: part2 0.075, dbeta 0.055, dgamma 0.075;
    real-valued: part2 0.027, dbeta 0.023, dgamma 0.027; dx fp32 0.32; dx bf16 every element inside its interval."""
    C, shape, full = case.C(dt), case.shape(dt), (case.FH, case.FW)
    x, st5, g1, g2 = R.bwd_inputs(case, dt, gpu_tables(case, dt) if case.kind == "real" else None)
    keep = R.keep_view(case.seed, case.offset, case.level, case.extent(dt), (case.H, case.W), case.p)
    ref = R.bwd_ref(x, st5, keep, case.p, g1, case.s1, g2, case.s2)
    xbuf, xv = place(x, dt, "crop", full)
    _, g1v = place(g1, dt, case.g1)
    g2v = place(g2, dt, case.g2)[1] if case.g2 else None
    dev5 = tuple(t.to(DEV) for t in st5)
    st = state(case.seed, case.offset)
    dxb = new_buf(shape, dt, "crop", full)
    nch = ops.stats_chunks(case.B, case.H, case.W)
    assert nch == R.stat_chunks(case.P) and (nch > 256) == (case.P > 256 * 64)
    part, dgamma, dbeta = bwd_drop(case.B, xv, C, dt, view(dxb, shape, "crop"), g1v, case.s1, g2v, case.s2, dev5,
                                   (st, case.level, case.p, case.FH, case.FW))
    tag = f"d.{case.kind}" + ("" if case.sums_exact else ".bounded")
    R.compare_sums(tag, case, dt, ref, part, nch, dgamma, dbeta)
    R.compare_dx(tag, dt, read_back(dxb, shape, "crop"), x, st5, ref, dgamma, dbeta, case.P)
    assert_same(read_back(xbuf, shape, "crop"), x.to(dt), "the input")
    # p = 0 through the drop kernels: the plain kernels' result
    outs = []
    for drop in (None, (st, case.level, 0.0, case.FH, case.FW)):
        dx0 = new_buf(shape, dt, "crop", full)
        dg0, db0 = ops.bn_backward(case.B, xv, C, dt, view(dx0, shape, "crop"), g1=g1v, s1=case.s1, g2=g2v, s2=case.s2,
                                   bn_state=dev5, drop=drop)
        outs.append((read_back(dx0, shape, "crop"), dg0.cpu(), db0.cpu()))
    for a, b, name in zip(outs[1], outs[0], ("dx", "dgamma", "dbeta")):
        assert_same(a, b, f"{case.id} p=0 {name} vs the plain kernels")


# ================================================================ e. the grid caps
@functools.lru_cache(maxsize=None)
def grid_words(name, C):
    B, FH, FW, H, W = R.GRID_CASES[name]
    return R.words_view(R.SEED, R.OFFSET, 6, (B, FH, FW, C), (H, W))


@pytest.mark.parametrize("dt", DTS, ids=dtname)
@pytest.mark.parametrize("name", list(R.GRID_CASES))
def test_grid_caps(name, dt):
    """One vector per pixel (C = 4 fp32 / 8 bf16) past the 8192-block cap of grid_for: P = 8192 * 256 + 1024 (1024
    threads run the two-in-flight body of bn_apply_drop_kernel once, the others only its tail) and P = 2.5 * 8192 *
    256 + 77 (body, then tail, with a ragged end); bn_bwd_apply_drop_kernel's grid-stride loop makes two and three
    trips.  The apply EQUALS the reference; dx (on hand-made partials of one chunk, so that only this kernel is
    measured) is within the bound of dropout_ref.  Cropped x / y1 / dx: the NaN surround survives.  (The pixel-index
    division beyond 2^24 pixels is the shared pix_bxy, pinned on both sides by tests/test_gpu_bn_family.py: not
    repeated here.)  Measured worst error / bound (MI355X): dx fp32 0.052, bf16 every element inside its interval;
    0.9 - 5.1 s per case, nearly all of it the numpy mask and the fp64 reference of 8 - 42 M elements."""
    B, FH, FW, H, W = R.GRID_CASES[name]
    C, P, p = R.vec(dt), B * H * W, 0.3
    assert P > R.GRID_CAP and (name == "above_cap") == (P < 2 * R.GRID_CAP)
    shape, full = (B, H, W, C), (FH, FW)
    keep = torch.from_numpy((grid_words(name, C) >= np.uint64(R.thresh(p))).astype(np.uint8))
    x = R.exact_values(shape, 11)
    sc, sh = R.exact_table(C, 12)
    st = state()
    drop = (st, 6, p, FH, FW)
    _, xv = place(x, dt, "crop", full)
    y1 = new_buf(shape, dt, "crop", full)
    ops.bn_apply(B, xv, C, dt, (sc.to(DEV), sh.to(DEV)), view(y1, shape, "crop"), 0.5, None, 1.0, drop=drop)
    assert_same(read_back(y1, shape, "crop"), R.apply_ref(x, sc, sh, keep, p, 0.5, dt), f"{name} apply")
    del y1
    g = torch.Generator().manual_seed(13)
    sc, sh = R.exact_table(C, 12, wide=False)
    st5 = (sc, sh, torch.randint(-4, 5, (C,), generator=g).float() / 4, torch.tensor([0.5, 1.0, 2.0, 1.0] * (C // 4)),
           torch.tensor([1.0, -2.0, 0.5, 2.0] * (C // 4)))
    g1 = R.exact_values(shape, 14, lim=16)
    part = (torch.randint(-64, 65, (1, C, 2), generator=g).float() * 1024).to(DEV)
    _, g1v = place(g1, dt, "dense")
    dxb = new_buf(shape, dt, "crop", full)
    _, dgamma, dbeta = bwd_drop(B, xv, C, dt, view(dxb, shape, "crop"), g1v, 0.0, None, 0.0,
                                tuple(t.to(DEV) for t in st5), drop, part=part, nch=1)
    assert_same(dbeta.cpu(), part[0, :, 0].cpu(), "dbeta of one chunk")
    assert_same(dgamma.cpu(), part[0, :, 1].cpu(), "dgamma of one chunk")
    ref = R.bwd_ref(x, st5, keep, p, g1, 0.0, None, 0.0, sums=False)
    R.compare_dx(f"e.{name}", dt, read_back(dxb, shape, "crop"), x, st5, ref, dgamma, dbeta, P)


# ================================================================ f. stc_conv_bn_fwd_drop
BF = BF16
# (B, Cin, Cout, GH, GW) of a ConvT: the smallest grid whose automatic plan is the halo kernel (it must fill the
# chip: 64 M-tiles of 256 grid points at N <= 64, one 64-channel chunk; N = 64 as in tests/test_gpu_halo.py) and
# the smallest shape that takes an im2col tile (tests/test_gpu_igemm_bf16.py; below N = 16 the narrow-N kernel runs)
FUSED = {"halo": (4, 64, 64, 64, 64), "im2col": (2, 64, 16, 2, 3)}


def fused_inputs(name):
    B, Cin, Cout, GH, GW = FUSED[name]
    g = torch.Generator().manual_seed(31 + Cout)
    x = torch.randn((B, GH, GW, Cin), generator=g).to(DEV, BF)
    w = (torch.randn((Cin, Cout, 4, 4), generator=g) * 0.05).to(DEV)
    return x, ops.pack(L.PACK_CONVT_FWD, w, Cout, Cin, BF)


@pytest.mark.parametrize("name", list(FUSED))
def test_fused_conv_bn_drop_equals_separate_calls(name):
    """ops.conv_bn_act(drop=) -- stc_conv_bn_fwd_drop, one call, three launches -- against conv_stats,
    bn_finalize_part and bn_apply(drop=) on the same inputs: the raw ConvT output, both activations (cropped by one
    row, y1 in the upper half of a NaN concat buffer), the table, mean / rstd, the running buffers and
    num_batches_tracked bit for bit.  (An equality of two paths of the library: what either computes is pinned by the
    other tests of this file and by the conv tests.)"""
    B, Cin, Cout, GH, GW = FUSED[name]
    plan = ops.conv_query(L.CONVT_S2, B, GH, GW, Cin, Cout, BF)[2]
    assert (plan[4] == ops.HALO_CFG) == (name == "halo") and (name == "halo" or plan[4] >= 0), plan
    x, wp = fused_inputs(name)
    FH, FW = 2 * GH, 2 * GW
    H, W = FH - 1, FW
    shape = (B, H, W, Cout)
    st = state()
    drop = (st, 4, 0.3, FH, FW)
    bn_a = _BN(Cout, 77)
    bn_b = bn_a.clone()

    def outputs():
        return (torch.full((B, FH, FW, Cout), NAN, device=DEV, dtype=BF), new_buf(shape, BF, "hi"),
                new_buf(shape, BF, "dense"))

    ya, y1a, y2a = outputs()
    tab_a, (mean_a, rstd_a) = ops.conv_bn_act(L.CONVT_S2, B, L.nhwc_view(x), Cin, wp, Cout, L.nhwc_view(ya), BF, bn_a,
                                              L.nhwc_view(ya, 0, H, W), view(y1a, shape, "hi"), 0.0,
                                              view(y2a, shape, "dense"), 0.2, drop=drop)
    yb, y1b, y2b = outputs()
    part, nch = ops.conv_stats(L.CONVT_S2, B, L.nhwc_view(x), Cin, wp, Cout, L.nhwc_view(yb), BF)
    tab_b = torch.full((2, Cout), NAN, device=DEV)
    mean_b, rstd_b = ops.bn_finalize_part(part, nch, Cout, bn_b, tab_b[0], tab_b[1])
    ops.bn_apply(B, L.nhwc_view(yb, 0, H, W), Cout, BF, (tab_b[0], tab_b[1]), view(y1b, shape, "hi"), 0.0,
                 view(y2b, shape, "dense"), 0.2, drop=drop)
    torch.cuda.synchronize()
    assert not bool(torch.isnan(ya).any()) and bool((y1a[..., Cout:] == 0).any()) and bool((y2a < 0).any())
    for a, b, what in ((ya, yb, "raw"), (y1a, y1b, "y1"), (y2a, y2b, "y2"), (tab_a, tab_b, "table"),
                       (mean_a, mean_b, "mean"), (rstd_a, rstd_b, "rstd"),
                       (bn_a.running_mean, bn_b.running_mean, "running_mean"),
                       (bn_a.running_var, bn_b.running_var, "running_var"),
                       (bn_a.num_batches_tracked, bn_b.num_batches_tracked, "num_batches_tracked")):
        assert_same(a, b, f"{name} {what}")
    assert int(bn_a.num_batches_tracked) == 1
    read_back(y1a, shape, "hi")  # (the lower half of the concat buffer still NaN)


def test_refusals_launch_nothing():
    """p = 1, a view larger than the dropout extent and C % 4 != 0 raise from every entry that takes a dropout block,
    and launch nothing: NaN-filled outputs stay NaN -- for stc_conv_bn_fwd_drop also the raw conv output, and the
    running buffers keep their values."""
    B, FH, FW, H, W, C = 2, 4, 6, 3, 5, 8
    st = state()
    x = torch.randn((B, FH, FW, C), device=DEV)
    xv = L.nhwc_view(x, 0, H, W)
    tab = (torch.ones(C, device=DEV), torch.zeros(C, device=DEV))
    st5 = tab + (torch.zeros(C, device=DEV), torch.ones(C, device=DEV), torch.ones(C, device=DEV))

    def refused(fn, *outs):
        with pytest.raises(RuntimeError, match="stc_"):
            fn()
        torch.cuda.synchronize()
        for o in outs:
            assert bool(torch.isnan(o).all()), "a refused call wrote an output"

    for drop in ((st, 5, 1.0, FH, FW), (st, 5, 0.5, H - 1, W), (st, 5, 0.5, H, W - 1)):
        y = torch.full((B, H, W, C), NAN, device=DEV)
        refused(lambda: ops.bn_apply(B, xv, C, F32, tab, L.nhwc_view(y), 0.0, drop=drop), y)
        dg, db = torch.full((C,), NAN, device=DEV), torch.full((C,), NAN, device=DEV)
        refused(lambda: ops.bn_backward(B, xv, C, F32, L.nhwc_view(y), g1=xv, bn_state=st5, dgamma=dg, dbeta=db,
                                        drop=drop), y, dg, db)
    x6 = torch.randn((B, FH, FW, 6), device=DEV)
    y6 = torch.full((B, H, W, 6), NAN, device=DEV)
    refused(lambda: ops.bn_apply(B, L.nhwc_view(x6, 0, H, W), 6, F32, None, L.nhwc_view(y6), 0.0,
                                 drop=(st, 5, 0.5, FH, FW)), y6)
    with pytest.raises(RuntimeError, match="stc_dropout_mask"):
        ops.dropout_mask(st, 5, (B, FH, FW, 6))
    with pytest.raises(RuntimeError, match="stc_dropout_mask"):
        ops.dropout_mask(st, 5, (B, FH, FW, C), p=1.0)
    # the fused call: nothing of its three launches may run
    Bc, Cin, Cout, GH, GW = FUSED["im2col"]
    xc, wp = fused_inputs("im2col")
    for drop in ((st, 4, 1.0, 2 * GH, 2 * GW), (st, 4, 0.5, 2 * GH - 1, 2 * GW), (st, 4, 0.5, 2 * GH, 2 * GW - 1)):
        bn = _BN(Cout, 78)
        before = bn.clone()
        raw = torch.full((Bc, 2 * GH, 2 * GW, Cout), NAN, device=DEV, dtype=BF)
        y1 = torch.full((Bc, 2 * GH, 2 * GW, Cout), NAN, device=DEV, dtype=BF)
        refused(lambda: ops.conv_bn_act(L.CONVT_S2, Bc, L.nhwc_view(xc), Cin, wp, Cout, L.nhwc_view(raw), BF, bn,
                                        L.nhwc_view(raw), L.nhwc_view(y1), 0.0, drop=drop), raw, y1)
        for k in ("running_mean", "running_var", "num_batches_tracked"):
            assert_same(getattr(bn, k), getattr(before, k), f"{k} after a refused call")


# ================================================================ g. dropout_next
def test_dropout_next_two_generators_and_a_side_stream():
    """Two generators' states advance independently when their calls interleave, and a call made on a side stream
    (joined through stc_stream_wait, as the engine's lanes are) continues the same {seed, offset} sequence."""
    a, b = state(R.SEED_TOP, R.OFFSET), state(5, (1 << 32) - 2)
    calls = [ops.dropout_next(s) for s in (a, b, b, a, b)]
    assert [c.tolist() for c in calls] == [[R.SEED_TOP - (1 << 64), R.OFFSET], [5, (1 << 32) - 2], [5, (1 << 32) - 1],
                                           [R.SEED_TOP - (1 << 64), R.OFFSET + 1], [5, 1 << 32]]
    assert a.tolist() == [R.SEED_TOP - (1 << 64), R.OFFSET + 2] and b.tolist() == [5, (1 << 32) + 1]
    cur, side = torch.cuda.current_stream(), torch.cuda.Stream()
    cur_h, side_h = ctypes.c_void_p(cur.cuda_stream), ctypes.c_void_p(side.cuda_stream)
    st = state(9, 100)
    seq = []
    for i in range(6):
        if i % 2:
            ops.check(L.lib().stc_stream_wait(side_h, cur_h), "stc_stream_wait")
            with torch.cuda.stream(side):
                seq.append(ops.dropout_next(st))
            ops.check(L.lib().stc_stream_wait(cur_h, side_h), "stc_stream_wait")
        else:
            seq.append(ops.dropout_next(st))
    torch.cuda.synchronize()
    assert [c.tolist() for c in seq] == [[9, 100 + i] for i in range(6)] and st.tolist() == [9, 106]


@pytest.mark.parametrize("dt", DTS, ids=dtname)
def test_forward_and_backward_of_one_call_share_the_mask(dt):
    """With the device copy dropout_next returns for a call: the zeros of the applied output (identity table, slope
    1, no zero input) and the zeros of dx (gamma = rstd = 1, g2 absent, zero partials, no zero gradient) are the
    dropped elements of the numpy mask at that call's offset -- for two consecutive calls."""
    B, FH, FW, H, W, C, level, p = 2, 4, 6, 3, 5, 64, 6, 0.3
    shape, full = (B, H, W, C), (FH, FW)
    x = R.exact_values(shape, 21)
    x[x == 0] = 0.125
    g1 = R.exact_values(shape, 22)
    g1[g1 == 0] = -0.25
    st = state(R.SEED, 41)
    one, zero = torch.ones(C, device=DEV), torch.zeros(C, device=DEV)
    _, xv = place(x, dt, "crop", full)
    _, g1v = place(g1, dt, "hi")
    for call_no in range(2):
        call = ops.dropout_next(st)
        drop = (call, level, p, FH, FW)
        y = new_buf(shape, dt, "dense")
        ops.bn_apply(B, xv, C, dt, None, view(y, shape, "dense"), 1.0, drop=drop)
        dxb = new_buf(shape, dt, "crop", full)
        bwd_drop(B, xv, C, dt, view(dxb, shape, "crop"), g1v, 1.0, None, 0.0, (one, zero, zero, one, one), drop,
                 part=torch.zeros((1, C, 2), device=DEV), nch=1)
        keep = R.keep_view(R.SEED, 41 + call_no, level, (B, FH, FW, C), (H, W), p).bool()
        assert 0.5 < float(keep.float().mean()) < 0.9
        assert_same(read_back(y, shape, "dense") != 0, keep, f"call {call_no}: the kept elements of the forward")
        assert_same(read_back(dxb, shape, "crop") != 0, keep, f"call {call_no}: the kept elements of the backward")
    assert st.tolist() == [R.SEED, 43]


# ================================================================ h. coverage
def test_cases_meet_every_path():
    """From the case lists alone: every thread layout, both sides of each grid cap, <= 256 and > 256 chunks, g2 on and
    off, a has2 = 0 apply, a NULL table and every p.  This map restates the dispatch of csrc/bn.hip (N = 4 / 8
    elements per vector, RL = 256 / CG with idle lanes where CG does not divide 256, grid_for's cap of 8192 blocks of
    256 threads, STAT_PIX = 64 pixels per chunk up to 1024 chunks, the backward finalize's switch at 256 chunks); if
    that dispatch changes, this map has to be revised with it."""
    cov = R.coverage()
    assert cov["apply_cg"] == {1, 3, 24, 64, 256} and cov["bwd_cg"] == {1, 3, 24, 64, 256}
    assert cov["grid"] == {(True, False), (True, True)}  # (the sizes below the cap: every other case)
    assert all(c.P * c.CG <= R.GRID_CAP for c in R.APPLY_CASES + R.BWD_CASES)
    assert cov["chunks"] == {False, True} and cov["g2"] == {False, True} and cov["g1_hi"]
    assert cov["idle_lanes"] == {False, True}
    assert cov["has2_0"] and cov["null_table"]
    assert cov["apply_p"] >= {0.5, 0.2, 0.3, 0.9, 0.1, R.P_MAX} and cov["bwd_p"] >= {0.5, 0.75, 0.2, 0.6, 0.3}
    assert set(R.P_ALL) >= cov["apply_p"] | cov["bwd_p"] | {0.0, 1e-12}  # (the mask export runs all of P_ALL)
    assert cov["crops"] >= {"none", "one", "both", "pixel"} and cov["outs"] == set(R.OUTS)
    assert cov["slopes"] == {(0.0, 0.2), (0.0, 1.0), (0.5, 0.0)}
    for layout in ("cg3", "cg64"):
        assert {c.p for c in R.APPLY_CASES if c.layout == layout} >= set(R.P_SWEEP)
    for layout in R.LAYOUTS:  # the exact backward configurations on every layout
        cfg = {(bool(c.g2), c.s2 if c.g2 else None, c.g1) for c in R.BWD_CASES
               if c.layout == layout and c.kind == "exact"}
        assert {(False, None, "hi"), (True, 0.2, "dense"), (True, 1.0, "hi")} <= cfg, (layout, cfg)
    assert R.LAYOUTS["cg256"][1:] == (1, 2, 3) and R.CROPS["row"] == (1, 3)
    assert any(c.kind == "real" and c.P == 65537 and c.CG == 1 for c in R.BWD_CASES)
    assert {c.layout for c in R.BWD_CASES if c.kind == "real"} >= {"cg3", "cg64"}
