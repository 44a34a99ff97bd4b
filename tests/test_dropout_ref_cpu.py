"""tests/dropout_ref.py without a GPU: the index-set mask against the full-extent numpy mask, the drop parameters at
the family's probabilities, every case's preconditions from the numpy mask alone, and -- on the very inputs of the
GPU cases -- that each comparison REJECTS a result that is wrong in one of the ways a dropout kernel can be subtly
wrong: the neighbouring word's keep bit in ONE element, the scale applied after the bf16 rounding in one element,
g2 sent through the mask, the crop width in the logical index, one pixel left out of one channel's sums."""
import numpy as np
import pytest
import torch

import dropout_ref as R
from dropout_ref import BF16, F32, dtname
from test_dropout_cpu import dropout_mask

DTS = [F32, BF16]


def case_params(cases):
    return [pytest.param(c, dt, id=f"{dtname(dt)}-{c.id}") for dt in DTS for c in cases]


# ---------------------------------------------------------------- the mask and its parameters
@pytest.mark.parametrize("level", [0, 7, 2 ** 31 - 1])
@pytest.mark.parametrize("extent,hw", [((3, 4, 6, 64), (4, 6)), ((3, 4, 6, 64), (3, 5)), ((2, 5, 3, 12), (1, 1)),
                                       ((1, 1, 1, 4), (1, 1)), ((1, 2, 3, 2048), (1, 3))])
def test_index_set_mask_equals_the_full_extent_mask(extent, hw, level):
    B, FH, FW, C = extent
    H, W = hw
    for seed, offset, p in ((R.SEED, R.OFFSET, 0.3), (R.SEED_TOP, 3, 0.5), (R.SEED_TOP, R.OFFSET, 0.9)):
        full = dropout_mask(seed, offset, level, extent, p)
        got = R.keep_view(seed, offset, level, extent, hw, p).numpy()
        assert np.array_equal(got, full[:, :H, :W, :])
        # an arbitrary index set: a shuffled list of (b, y, x, c)
        rs = np.random.RandomState(level % 1000 + C)
        n = 200
        b, y, x, c = rs.randint(0, B, n), rs.randint(0, FH, n), rs.randint(0, FW, n), rs.randint(0, C, n)
        assert np.array_equal(R.keep_at(seed, offset, level, extent, p, b, y, x, c), full[b, y, x, c])


def test_scale32_and_thresh():
    f = np.float32
    want = {0.0: (0, f(1.0)), 1e-12: (0, f(1.0)), 0.1: (429496729, f(1.0 / 0.9)), 0.2: (858993459, f(1.25)),
            0.3: (1288490188, f(1.0 / 0.7)), 0.5: (1 << 31, f(2.0)), 0.6: (2576980377, f(2.5)),
            0.75: (3 << 30, f(4.0)), 0.9: (3865470566, f(10.0)), R.P_MAX: ((1 << 32) - 256, f(2.0 ** 24))}
    assert set(want) == set(R.P_ALL)
    for p, (t, s) in want.items():
        assert R.thresh(p) == t and 0 <= t < 1 << 32, (p, R.thresh(p))
        assert R.scale32(p) == s and R.scale32(p).dtype == np.float32, (p, R.scale32(p))
    # inexact scales: what pins "scale in fp32 before the rounding to the storage type"
    for p in (0.3, 0.1):
        assert float(R.scale32(p)) != 1.0 / (1.0 - p)


def test_p_max_offsets_are_the_first_that_keep_an_element():
    for case in R.APPLY_CASES:
        if case.p == R.P_MAX:
            for dt in DTS:
                off = R.case_offset(case, dt)
                assert int(R.case_keep(case, dt).sum()) >= 1, (case.id, dtname(dt))
                # (the search itself, over the last few candidates only)
                assert R.first_offset_with_kept(case.seed, case.level, case.extent(dt), (case.H, case.W), case.p,
                                                off - 50) == off


# ---------------------------------------------------------------- helpers
def rejects(fn):
    with pytest.raises(AssertionError):
        fn()


def crop_width_keep(case, dt):
    """The mask a kernel would use with the view's W in drop_index."""
    return R.case_keep(case, dt, extent=(case.B, case.FH, case.W, case.C(dt)))


def neighbour_keep(case, dt, keep):
    """keep of the neighbouring word of the same quad (channel c ^ 1), for every element of the view."""
    B, H, W, C = case.shape(dt)
    b, y, x, c = np.meshgrid(np.arange(B), np.arange(H), np.arange(W), np.arange(C) ^ 1, indexing="ij")
    nb = R.keep_at(case.seed, R.case_offset(case, dt), case.level, case.extent(dt), case.p, b, y, x, c)
    assert np.array_equal(nb.reshape(B, H, W, C // 2, 2)[..., ::-1].reshape(B, H, W, C), keep.numpy())
    return torch.from_numpy(nb)


def with_one(a, b, where):
    """``a`` with the first element at which ``where`` holds taken from ``b``."""
    idx = tuple(where.nonzero()[0].tolist())
    out = a.clone()
    out[idx] = b[idx]
    return out


# ---------------------------------------------------------------- the apply cases
def late_scale_counts(case, dt, refs=None, check=False):
    """(kept elements, elements that change when the scale follows the rounding to the storage type) over the case's
    outputs; check: ONE such element is rejected."""
    x, sc, sh = R.apply_inputs(case, dt)
    keep = R.case_keep(case, dt)
    kept = differ = 0
    for s in case.slopes:
        ref = R.apply_ref(x, sc, sh, keep, case.p, s, dt)
        late = R.apply_late_scale(x, sc, sh, keep, case.p, s, dt)
        d = late != ref
        kept, differ = kept + int(keep.sum()), differ + int(d.sum())
        if check and bool(d.any()):
            rejects(lambda: R.assert_same(with_one(ref, late, d), ref, "late scale"))
    return kept, differ


@pytest.mark.parametrize("case,dt", case_params(R.APPLY_CASES))
def test_apply_case_preconditions_and_rejections(case, dt):
    x, sc, sh = R.apply_inputs(case, dt)
    assert torch.equal(R.stored(x, dt), x)  # the operands are exact in the storage type
    keep = R.case_keep(case, dt)
    R.affine(x, sc, sh)  # (asserts that n is exact in fp32)
    assert bool(keep.any()) and not bool(keep.all()), "both kept and dropped elements"
    refs = [R.apply_ref(x, sc, sh, keep, case.p, s, dt) for s in case.slopes]
    for ref in refs:
        R.assert_same(ref.clone(), ref, "the reference against itself")
    # ONE element with the neighbouring word's keep bit
    nb = neighbour_keep(case, dt, keep)
    hit = False
    for s, ref in zip(case.slopes, refs):
        wrong = R.apply_ref(x, sc, sh, nb, case.p, s, dt)
        if bool((wrong != ref).any()):
            rejects(lambda: R.assert_same(with_one(ref, wrong, wrong != ref), ref, "neighbouring word"))
            hit = True
    assert hit, "no element tells the neighbouring word apart"
    # the crop width in the logical index
    if case.W != case.FW:
        kw = crop_width_keep(case, dt)
        if case.P > 3:  # (a one-pixel view has too few elements to promise a difference)
            assert not torch.equal(kw, keep)
            wrong = [R.apply_ref(x, sc, sh, kw, case.p, s, dt) for s in case.slopes]
            assert any(bool((w != r).any()) for w, r in zip(wrong, refs))
            for w, r in zip(wrong, refs):
                if bool((w != r).any()):
                    rejects(lambda: R.assert_same(w, r, "crop width"))
    # one element scaled after the rounding to the storage type
    if dt == BF16:
        kept, differ = late_scale_counts(case, dt, check=True)
        if case.p == 0.3 and case.table and kept >= 256:
            assert differ >= 0.05 * kept, (differ, kept)
        if float(R.scale32(case.p)) in (2.0, 4.0, 2.0 ** 24):
            assert differ == 0  # a power of two commutes with the rounding: those p cannot show the order


def test_late_scale_differs_often_enough():
    """Over the p = 0.3 bf16 apply cases with a table: at least 5 % of the kept elements change when the scale is
    applied after the rounding (so a kernel doing that cannot pass)."""
    counts = [late_scale_counts(c, BF16) for c in R.APPLY_CASES if c.p == 0.3 and c.table]
    kept, differ = sum(k for k, _ in counts), sum(d for _, d in counts)
    print(f"late scale: {differ} of {kept} kept elements differ")
    assert len(counts) >= 5 and differ >= 0.05 * kept > 0


# ---------------------------------------------------------------- the backward cases
def result_of(ref, nch, x, st5, P, dt, dgamma=None, dbeta=None):
    """What a kernel computing ``ref`` would return: fp32 partials, dgamma, dbeta and dx in the storage type."""
    val, _ = R.chunk_sums(ref, nch)
    dg = ref["dgamma"].float() if dgamma is None else dgamma
    db = ref["dbeta"].float() if dbeta is None else dbeta
    return val.float(), dg, db, R.dx_ref(x, st5, ref, dg, db, P)[0].float().to(dt)


@pytest.mark.parametrize("case,dt", case_params(R.BWD_CASES))
def test_backward_case_preconditions_and_rejections(case, dt):
    x, st5, g1, g2 = R.bwd_inputs(case, dt)
    assert torch.equal(R.stored(x, dt), x) and torch.equal(R.stored(g1, dt), g1)
    keep = R.keep_view(case.seed, case.offset, case.level, case.extent(dt), (case.H, case.W), case.p)
    assert bool(keep.any()) and not bool(keep.all())
    ref = R.bwd_ref(x, st5, keep, case.p, g1, case.s1, g2, case.s2)
    if case.kind == "exact":
        R.affine(x, st5[0], st5[1])
        assert float(R.scale32(case.p)) in (2.0, 4.0, 1.25, 2.5)
    else:
        assert float(ref["n"].abs().min()) >= 1e-3
    if case.sums_exact:
        R.require_exact_sums(ref)
    nch = R.stat_chunks(case.P)
    tag = "cpu"
    part, dg, db, dx = result_of(ref, nch, x, st5, case.P, dt)
    R.compare_sums(tag, case, dt, ref, part, nch, dg, db)  # the reference passes its own comparison
    R.compare_dx(tag, dt, dx, x, st5, ref, dg, db, case.P)

    def wrong_result(bad, what, sums=True, elementwise=True):
        bp, bdg, bdb, _ = result_of(bad, nch, x, st5, case.P, dt)
        if sums:
            rejects(lambda: R.compare_sums(tag, case, dt, ref, bp, nch, bdg, bdb))
        if elementwise:  # (dx with the right dgamma / dbeta: only the element's own dn is wrong)
            bdx = result_of(bad, nch, x, st5, case.P, dt, dg, db)[3]
            rejects(lambda: R.compare_dx(tag, dt, bdx, x, st5, ref, dg, db, case.P))

    # g2 through the mask
    if case.g2:
        bad = R.bwd_ref(x, st5, keep, case.p, g1, case.s1, g2, case.s2, mask_g2=True)
        assert not torch.equal(bad["dn"], ref["dn"])
        wrong_result(bad, "g2 masked")
    # ONE element with the neighbouring word's keep bit
    nb = neighbour_keep(case, dt, keep)
    bad_all = R.bwd_ref(x, st5, nb, case.p, g1, case.s1, g2, case.s2)
    d = bad_all["dn"] != ref["dn"]
    assert bool(d.any())
    one = R.bwd_ref(x, st5, with_one(keep, nb, d), case.p, g1, case.s1, g2, case.s2)
    assert int((one["dn"] != ref["dn"]).sum()) == 1
    wrong_result(one, "neighbouring word")
    # the crop width in the logical index
    if case.W != case.FW and case.B * case.H > 1:  # (one row of one image: the width never enters the index)
        kw = R.keep_view(case.seed, case.offset, case.level, (case.B, case.FH, case.W, case.C(dt)), (case.H, case.W),
                         case.p)
        assert not torch.equal(kw, keep)
        wrong_result(R.bwd_ref(x, st5, kw, case.p, g1, case.s1, g2, case.s2), "crop width")
    # one pixel left out of one channel's sums
    idx = tuple(ref["dn"].nonzero()[0].tolist())
    less = dict(ref)
    less["dn"] = ref["dn"].clone()
    less["dn"][idx] = 0.0
    less["dbeta"] = less["dn"].sum(dim=(0, 1, 2))
    less["dgamma"] = (less["dn"] * ref["xh"]).sum(dim=(0, 1, 2))
    wrong_result(less, "a pixel left out", elementwise=False)
    bp, bdg, bdb, _ = result_of(less, nch, x, st5, case.P, dt)
    if case.P < 1000:  # (above, one term is within the bound of a whole channel's sum: the partials catch it)
        rejects(lambda: R.compare_sums(tag, case, dt, ref, part, nch, dg, bdb))  # (dbeta alone)
    rejects(lambda: R.compare_sums(tag, case, dt, ref, bp, nch, dg, db))     # (the partials alone)


def test_dx_bound_counts_the_terms_roundings():
    """The documented dx formula evaluated in correctly rounded fp32 (numpy float32, each fma as one rounding of the
    fp64 value) on the P = 65537 case: it does NOT meet 16 * EPS32 * (|k1 dn| + |k2 x| + |k0|) alone -- where g1 * m
    and g2 cancel, the rounding of g1 * m is larger than that of everything that is left -- and it meets the bound
    of dropout_ref with room to spare.  So the second part of that bound is owed to the number format, not to a
    kernel."""
    f32 = np.float32
    case = next(c for c in R.BWD_CASES if c.P == R.BIG_P)
    x, st5, g1, g2 = R.bwd_inputs(case, F32)
    keep = R.keep_view(case.seed, case.offset, case.level, case.extent(F32), (case.H, case.W), case.p)
    ref = R.bwd_ref(x, st5, keep, case.p, g1, case.s1, g2, case.s2)
    dg, db = ref["dgamma"].float(), ref["dbeta"].float()
    sc, sh, mu, rs, gm = (t.numpy().astype(f32) for t in st5)
    X, G1, G2 = (t.numpy().astype(f32) for t in (x, g1, g2))
    inv_p = f32(1.0) / f32(case.P)
    k1 = gm * rs
    k2 = k1 * rs * dg.numpy() * inv_p
    k0 = k1 * (db.numpy() * inv_p - mu * rs * dg.numpy() * inv_p)
    n = (X.astype(np.float64) * sc + sh).astype(f32)
    m = keep.numpy().astype(f32) * R.scale32(case.p)
    dn = (G1 * m) * np.where(n > 0, f32(1), f32(case.s1))
    dn = dn + G2 * np.where(n > 0, f32(1), f32(case.s2))
    inner = (k2.astype(np.float64) * X + k0).astype(f32)
    dx = torch.from_numpy((k1.astype(np.float64) * dn - inner).astype(f32))
    assert dx.dtype == torch.float32 and k0.dtype == f32 and dn.dtype == f32
    val, family = R.dx_ref(x, st5, ref, dg, db, case.P, family_only=True)
    _, full = R.dx_ref(x, st5, ref, dg, db, case.P)
    err = (dx.double() - val).abs()
    worst_family, worst_full = float((err / family).max()), float((err / full).max())
    print(f"fp32 emulation: error / family bound {worst_family:.3f}, error / bound {worst_full:.3f}")
    assert worst_family > 2.0 and worst_full < 0.5
    cancel = ref["dn"].abs() < 1e-3 * ref["mag"]
    assert bool(cancel.any()) and bool(((err > family) <= (ref["dn"].abs() < 0.05 * ref["mag"])).all())


# ---------------------------------------------------------------- the grid-cap cases
def test_grid_case_preconditions_and_rejection():
    """The sizes sit where the docstring of the GPU test says, and on the smaller one (fp32) the operands are exact,
    both kept and dropped elements occur, the crop-width mask differs and one wrong keep bit is rejected."""
    (B, FH, FW, H, W) = R.GRID_CASES["above_cap"]
    assert 0 < B * H * W - R.GRID_CAP <= 4096 and FW > W
    (B2, FH2, FW2, H2, W2) = R.GRID_CASES["2.5_caps"]
    assert B2 * H2 * W2 == 5 * R.GRID_CAP // 2 + 77 and FW2 > W2
    C, p = 4, 0.3
    shape = (B, H, W, C)
    keep = R.keep_view(R.SEED, R.OFFSET, 6, (B, FH, FW, C), (H, W), p)
    assert abs(float(keep.float().mean()) - 0.7) < 1e-3
    assert not torch.equal(R.keep_view(R.SEED, R.OFFSET, 6, (B, FH, W, C), (H, W), p), keep)
    x = R.exact_values(shape, 11)
    sc, sh = R.exact_table(C, 12)
    ref = R.apply_ref(x, sc, sh, keep, p, 0.5, F32)
    n = R.affine(x, sc, sh)
    idx = tuple((n != 0).nonzero()[-1].tolist())  # the last element whose value shows its keep bit
    flip = keep.clone()
    flip[idx] = 1 - flip[idx]
    rejects(lambda: R.assert_same(R.apply_ref(x, sc, sh, flip, p, 0.5, F32), ref, "one keep bit"))


def test_case_lists_meet_every_path():
    """The coverage map of the GPU file holds without a GPU as well (the same assertions run there)."""
    cov = R.coverage()
    assert cov["apply_cg"] == cov["bwd_cg"] == {1, 3, 24, 64, 256}
    assert cov["chunks"] == {False, True} and cov["g2"] == {False, True} and cov["idle_lanes"] == {False, True}
    for cases in (R.APPLY_CASES, R.BWD_CASES):
        assert len({c.id for c in cases}) == len(cases)
