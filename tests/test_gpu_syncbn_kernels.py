"""The sync-statistics BatchNorm kernels (stc_bn_stats_pack, stc_bn_bwd_sums, stc_bn_bwd_apply_sync) in one process: the
ranks are emulated by sharding one batch, every shard a tensor of its own with its own partials and record, the
"gather" a torch.stack in rank order.  References, operands, cases and the derivation of every bound:
tests/syncbn_ref.py.

Measured worst error / bound on an MI355X: profiles/sync_bn/test_ratios.txt (the lines this file prints with -s)."""
import ctypes

import pytest
import torch

import dropout_ref as R
import syncbn_ref as S
from dropout_ref import BF16, EPS32, F32, assert_same, dtname, note
from stcgan_amd import _lib as L
from stcgan_amd import ops
from test_gpu_bn_family import _BN
from test_gpu_bn_family import finalize_ref as partials_ref
from test_gpu_bn_family import make_partials
from test_gpu_dropout_family import new_buf, place, read_back, view

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")
DTS = [F32, BF16]


def _ids(v):
    return dtname(v) if isinstance(v, torch.dtype) else "+".join(map(str, v)) if isinstance(v, tuple) else str(v)


def shard_record(xs, dt, mode):
    """chan_stats partials of one shard [b, H, W, C] in layout ``mode`` and its packed record [C, 4]."""
    b, H, W, C = xs.shape
    _, xv = place(xs, dt, mode)
    nch = ops.stats_chunks(b, H, W)
    part = torch.full((nch, C, 4), NAN, device=DEV)
    ops.check(L.lib().stc_chan_stats(L.dtype_code(dt), b, xv, C, L.ptr(part), nch, L.stream()), "stc_chan_stats")
    rec = ops.bn_stats_pack(part, nch, C)
    assert tuple(rec.shape) == (C, 4)
    return part, nch, rec


def finalize_records(recs, C, seed):
    """stc_bn_finalize over records [world, C, 4]: ({name: device result}, the module stand-in)."""
    bn = _BN(C, seed)
    tab = torch.full((2, C), NAN, device=DEV)
    mean, rstd = ops.bn_finalize_part(recs, recs.shape[0], C, bn, tab[0], tab[1])
    torch.cuda.synchronize()
    return {"mean": mean, "rstd": rstd, "scale": tab[0], "shift": tab[1], "running_mean": bn.running_mean,
            "running_var": bn.running_var}, bn


# ================================================================ a. statistics: pack per shard, finalize over records
@pytest.mark.parametrize("mode", S.LAYOUTS)
@pytest.mark.parametrize("shards", S.SHARDS, ids=_ids)
@pytest.mark.parametrize("cg", S.CGS)
@pytest.mark.parametrize("dt", DTS, ids=_ids)
def test_stats_exact_operands(dt, cg, shards, mode):
    """Exact operands: every record EQUALS {n, 0, sum (x - a)^2, a}; the finalize over the ranks' records gives
    mean == a, rstd and scale equal to the fp64 values rounded to fp32 whatever the sharding, the table's shift and the
    running buffers within 4 EPS32 sum|terms|, and num_batches_tracked advances by one."""
    C = cg * R.vec(dt)
    x, a = S.exact_batch(sum(shards), *S.HW, C, 1)
    recs = []
    for xs in S.split(x, shards):
        _, _, rec = shard_record(xs, dt, mode)
        st = S.whole_stats(xs)
        want = torch.stack([torch.full((C,), float(st["N"]), dtype=torch.float64), torch.zeros(C, dtype=torch.float64),
                            ((xs.double() - a.double()) ** 2).sum(dim=(0, 1, 2)), a.double()], dim=-1)
        assert_same(rec.cpu().double(), want, f"record of a shard of {xs.shape[0]}")
        recs.append(rec)
    got, bn = finalize_records(torch.stack(recs), C, 300 + C)
    whole = S.whole_stats(x)
    host = [bn.host[k] for k in ("weight", "bias", "running_mean", "running_var")]
    ref = S.finalize_ref(float(whole["N"]), a.double(), whole["M2"], *host)
    for k in ("mean", "rstd"):
        assert_same(got[k].cpu(), ref[k][0].float(), f"{k} {shards}")
    # (the kernel multiplies gamma by the rounded rstd: one exact 24 x 24-bit product, rounded once)
    assert_same(got["scale"].cpu(), (bn.host["weight"].double() * ref["rstd"][0].float().double()).float(),
                f"scale {shards}")
    for k in ("shift", "running_mean", "running_var"):
        note(f"a.exact.{k}", (got[k].cpu().double() - ref[k][0]).abs(), 4 * EPS32 * ref[k][1])
    assert int(bn.num_batches_tracked) == 1


@pytest.mark.parametrize("mode", S.LAYOUTS)
@pytest.mark.parametrize("shards", S.SHARDS, ids=_ids)
@pytest.mark.parametrize("cg", S.CGS)
@pytest.mark.parametrize("dt", DTS, ids=_ids)
def test_stats_real_operands(dt, cg, shards, mode):
    """Real-valued operands against the fp64 statistics of the WHOLE batch: mean, variance (from rstd), the table from
    the device's own mean / rstd, running mean / var with the unbiased variance of the global count."""
    C = cg * R.vec(dt)
    x = S.real_batch((sum(shards), *S.HW, C), dt, 2)
    recs = torch.stack([shard_record(xs, dt, mode)[2] for xs in S.split(x, shards)])
    check_stats("a.real", x, recs, C, cg, [b * S.HW[0] * S.HW[1] for b in shards])


def check_stats(tag, x, recs, C, cg, pixels):
    got, bn = finalize_records(recs, C, 300 + C)
    ref = S.whole_stats(x)
    assert float(recs[:, 0, 0].sum()) == ref["N"]
    m = max(S.acc_len_stats(P, cg) for P in pixels)
    mean_b, var_b = S.stats_bounds(ref, m)
    mean, rstd = got["mean"].cpu().double(), got["rstd"].cpu().double()
    note(f"{tag}.mean", (mean - ref["mean"]).abs(), mean_b)
    note(f"{tag}.var", (1.0 / (rstd * rstd) - S.BN_EPS - ref["var"]).abs(), var_b)
    rm0, rv0 = bn.host["running_mean"].double(), bn.host["running_var"].double()
    note(f"{tag}.running_mean", (got["running_mean"].cpu().double() - ((1 - S.MOM) * rm0 + S.MOM * ref["mean"])).abs(),
         4 * EPS32 * (((1 - S.MOM) * rm0).abs() + (S.MOM * ref["mean"]).abs()) + S.MOM * mean_b)
    note(f"{tag}.running_var", (got["running_var"].cpu().double() - ((1 - S.MOM) * rv0 + S.MOM * ref["unb"])).abs(),
         4 * EPS32 * (((1 - S.MOM) * rv0).abs() + S.MOM * ref["unb"]) + S.MOM * var_b * ref["N"] / (ref["N"] - 1.0))
    gam, bet = bn.host["weight"].double(), bn.host["bias"].double()
    sc = got["scale"].cpu().double()
    note(f"{tag}.scale", (sc - gam * rstd).abs(), 4 * EPS32 * (gam * rstd).abs())
    note(f"{tag}.shift", (got["shift"].cpu().double() - (bet - mean * sc)).abs(),
         4 * EPS32 * (bet.abs() + (mean * sc).abs()))
    assert int(bn.num_batches_tracked) == 1


@pytest.mark.parametrize("dt", DTS, ids=_ids)
def test_stats_many_chunks_unequal_counts(dt):
    """One vector per pixel, shards of 65537 (1024 chunks, empty tail chunks) and 130 pixels (3 chunks)."""
    C = R.vec(dt)
    x = S.real_batch((1, 1, sum(S.MANY), C), dt, 3)
    recs = []
    for xs, nch_want in zip(S.split(x, S.MANY, dim=2), (1024, 3)):
        _, nch, rec = shard_record(xs.contiguous(), dt, "dense")
        assert nch == nch_want
        recs.append(rec)
    check_stats("a.many", x, torch.stack(recs), C, 1, S.MANY)


@pytest.mark.parametrize("C", [3, 4])
@pytest.mark.parametrize("nch", S.PACK_NCH)
def test_pack_synthetic_partials(nch, C):
    """bn_stats_pack_kernel<WaveMerge> (<= 1024 chunks: 1, 2 and 4 load groups per lane) and <BlockMerge> (above, up
    to the looping form) on the hand-made partials of tests/test_gpu_bn_family.py (empty chunks, a constant channel,
    slightly negative chunk M2): pack, then finalize the ONE record, against the long-double merge of the partials."""
    part = make_partials(nch, C)
    pd = torch.from_numpy(part).to(DEV)
    rec = ops.bn_stats_pack(pd, nch, C)
    got, bn = finalize_records(rec.unsqueeze(0), C, 500 + C)
    for k, (val, mag) in partials_ref(part, bn).items():
        note(f"a.synthetic.{k}", (got[k].cpu().double() - val).abs(), 5 * EPS32 * mag)
    # the record's shift is the fp32 mean, its count the partials' total
    assert_same(rec[:, 3].cpu(), got["mean"].cpu(), "record shift == fl32(mean)")
    assert_same(rec[:, 0].cpu().double(), torch.from_numpy(part[..., 0].astype("float64").sum(0)), "record count")


# ================================================================ b. the backward
def shard_backward(case, dt, xs, g1s, g2s, dev5, drop, xmode="dense"):
    """One shard's reduce + stc_bn_bwd_sums, and stc_bn_bwd_apply[_drop] on the same partials for comparison.
    Returns dict(views, part, nch, rec, dgamma, dbeta, local dx readback)."""
    b, H, W, C = xs.shape
    shape = tuple(xs.shape)
    _, xv = place(xs, dt, xmode)
    _, g1v = place(g1s, dt, case.g1)
    g2v = place(g2s, dt, case.g2)[1] if case.g2 else None
    sc, sh, mean, rstd, gam = dev5
    l = L.lib()
    nch = ops.stats_chunks(b, H, W)
    part = torch.full((nch, C, 2), NAN, device=DEV)
    g2n = g2v if g2v is not None else L.NULL_VIEW
    d = ops._drop(drop) if drop is not None else None
    if d is not None:
        ops.check(l.stc_bn_bwd_reduce_drop(L.dtype_code(dt), b, xv, C, L.ptr(sc), L.ptr(sh), L.ptr(mean), L.ptr(rstd),
                                           g1v, float(case.s1), g2n, float(case.s2), ctypes.byref(d), L.ptr(part), nch,
                                           L.stream()), "stc_bn_bwd_reduce_drop")
    else:
        ops.check(l.stc_bn_bwd_reduce(L.dtype_code(dt), b, xv, C, L.ptr(sc), L.ptr(sh), L.ptr(mean), L.ptr(rstd), g1v,
                                      float(case.s1), g2n, float(case.s2), L.ptr(part), nch, L.stream()),
                  "stc_bn_bwd_reduce")
    dgamma, dbeta = torch.full((C,), NAN, device=DEV), torch.full((C,), NAN, device=DEV)
    rec = ops.bn_bwd_sums(part, nch, C, dgamma, dbeta)
    # the local apply on the same partials: its dgamma / dbeta are the bits bwd_sums must give
    dg0, db0 = torch.full((C,), NAN, device=DEV), torch.full((C,), NAN, device=DEV)
    dx0 = new_buf(shape, dt, "hi")
    if d is not None:
        ops.check(l.stc_bn_bwd_apply_drop(L.dtype_code(dt), b, xv, C, L.ptr(sc), L.ptr(sh), L.ptr(mean), L.ptr(rstd),
                                          L.ptr(gam), g1v, float(case.s1), g2n, float(case.s2), ctypes.byref(d),
                                          L.ptr(part), nch, view(dx0, shape, "hi"), L.ptr(dg0), L.ptr(db0), L.stream()),
                  "stc_bn_bwd_apply_drop")
    else:
        ops.check(l.stc_bn_bwd_apply(L.dtype_code(dt), b, xv, C, L.ptr(sc), L.ptr(sh), L.ptr(mean), L.ptr(rstd),
                                     L.ptr(gam), g1v, float(case.s1), g2n, float(case.s2), L.ptr(part), nch,
                                     view(dx0, shape, "hi"), L.ptr(dg0), L.ptr(db0), L.stream()), "stc_bn_bwd_apply")
    torch.cuda.synchronize()
    assert_same(dgamma.cpu(), dg0.cpu(), "bwd_sums dgamma vs stc_bn_bwd_apply's")
    assert_same(dbeta.cpu(), db0.cpu(), "bwd_sums dbeta vs stc_bn_bwd_apply's")
    assert_same(rec.cpu(), torch.stack([db0, dg0], dim=-1).cpu(), "record == {dbeta, dgamma}")
    # no parameter gradient wanted: the same record, nothing else written
    assert_same(ops.bn_bwd_sums(part, nch, C).cpu(), rec.cpu(), "record without dgamma / dbeta")
    # world = 1, count = this shard's pixels: the local apply, bit for bit
    dx1 = new_buf(shape, dt, "hi")
    ops.bn_bwd_apply_sync(b, xv, C, dt, view(dx1, shape, "hi"), g1v, case.s1, g2v, case.s2, dev5, rec.unsqueeze(0),
                          b * H * W, drop)
    torch.cuda.synchronize()
    assert_same(read_back(dx1, shape, "hi"), read_back(dx0, shape, "hi"), "world = 1 dx vs stc_bn_bwd_apply's")
    return dict(xv=xv, g1v=g1v, g2v=g2v, rec=rec, dgamma=dgamma, dbeta=dbeta, shape=shape)


def run_backward(tag, case, dt, shards, dim=0, gpu_tables=None, xmode="dense"):
    x, st5, g1, g2 = R.bwd_inputs(case, dt, gpu_tables)
    refs, whole = S.shard_refs(case, dt, x, st5, g1, g2, shards, dim)
    dev5 = tuple(t.to(DEV) for t in st5)
    C = case.C(dt)
    xs_l, g1_l = S.split(x, shards, dim), S.split(g1, shards, dim)
    g2_l = S.split(g2, shards, dim) if g2 is not None else [None] * len(shards)
    outs = []
    for r, (xs, a, b) in enumerate(zip(xs_l, g1_l, g2_l)):
        drop = None
        if case.p > 0.0:
            drop = (ops.dropout_state_tensor(S.rank_seed(r), case.offset, DEV), case.level, case.p, case.FH, case.FW)
        o = shard_backward(case, dt, xs.contiguous(), a.contiguous(), b.contiguous() if b is not None else None, dev5,
                           drop, xmode)
        o["drop"] = drop
        outs.append(o)
    # the shards' local sums add up to the whole batch's
    pixels = [int(xs.numel() // C) for xs in xs_l]
    dbeta = sum(o["dbeta"].cpu().double() for o in outs)
    dgamma = sum(o["dgamma"].cpu().double() for o in outs)
    if case.sums_exact:
        R.require_exact_sums(whole)
        assert_same(dbeta, whole["dbeta"], f"{tag} sum of the shards' dbeta")
        assert_same(dgamma, whole["dgamma"], f"{tag} sum of the shards' dgamma")
    else:
        m = S.sums_bound(case, pixels)
        note(f"{tag}.dbeta", (dbeta - whole["dbeta"]).abs(), m * EPS32 * whole["abs_dbeta"])
        note(f"{tag}.dgamma", (dgamma - whole["dgamma"]).abs(), m * EPS32 * whole["abs_dgamma"])
    # every rank applies the global sums: the records in rank order, the global count
    recs = torch.stack([o["rec"] for o in outs])
    gb, gg = S.global_sums(recs.cpu())
    count = sum(pixels)
    for o, xs, ref in zip(outs, xs_l, refs):
        dxb = new_buf(o["shape"], dt, "hi")
        ops.bn_bwd_apply_sync(o["shape"][0], o["xv"], C, dt, view(dxb, o["shape"], "hi"), o["g1v"], case.s1, o["g2v"],
                              case.s2, dev5, recs, count, o["drop"])
        torch.cuda.synchronize()
        val, tol = S.dx_ref(xs, st5, ref, gg, gb, count)
        R.check_elementwise(f"{tag}.dx.{dtname(dt)}", read_back(dxb, o["shape"], "hi").double(), val, dt, tol)


@pytest.mark.parametrize("xmode", S.LAYOUTS)
@pytest.mark.parametrize("shards", S.SHARDS, ids=_ids)
@pytest.mark.parametrize("case", S.BWD_CASES, ids=lambda c: c.id)
@pytest.mark.parametrize("dt", DTS, ids=_ids)
def test_backward(dt, case, shards, xmode):
    """x dense or the upper half of a 2C-wide NaN-surrounded buffer (g1 per case, dx always an upper half).
    Per shard: bwd_sums' dgamma / dbeta / record are the bits of stc_bn_bwd_apply from the same partials, with and
    without gradient outputs; world = 1 is stc_bn_bwd_apply bit for bit.  Over the shards: the local sums add up to the
    whole batch's (exact operands: equal to the fp64 sums); dx of every shard from the gathered records and the global
    count against fp64."""
    run_backward(f"b.{case.kind}", S.with_batch(case, sum(shards)), dt, shards, xmode=xmode)


@pytest.mark.parametrize("dt", DTS, ids=_ids)
def test_backward_masked(dt):
    """A dropout level: every rank masks g1 with its own seed over its own extent (dropout_ref.bwd_ref per shard);
    world = 1 is stc_bn_bwd_apply_drop bit for bit."""
    run_backward("b.masked", S.MASKED, dt, (2, 1))


@pytest.mark.parametrize("dt", DTS, ids=_ids)
def test_backward_many_chunks_unequal_counts(dt):
    """Shards of 65537 and 130 pixels: bn_bwd_sums_kernel<BlockMerge> (1024 chunks) beside <WaveMerge> (3)."""
    run_backward("b.many", S.MANY_CASE, dt, S.MANY, dim=2)


# ================================================================ c. refusals
def test_bad_arguments_fail_with_messages():
    C = 8
    part = torch.zeros((2, C, 4), device=DEV)
    rec = torch.full((C, 4), NAN, device=DEV)
    l = L.lib()

    def refused(rc, needle):
        assert rc != 0
        msg = l.stc_last_error().decode()
        assert msg.startswith("stc_") and needle in msg, msg

    refused(l.stc_bn_stats_pack(L.ptr(part), 0, C, L.ptr(rec), L.stream()), "stc_bn_stats_pack")
    refused(l.stc_bn_stats_pack(None, 2, C, L.ptr(rec), L.stream()), "stc_bn_stats_pack")
    refused(l.stc_bn_bwd_sums(L.ptr(part), 2, C, L.ptr(rec), None, L.ptr(rec), L.stream()), "come together")
    refused(l.stc_bn_bwd_sums(L.ptr(part), 0, C, None, None, L.ptr(rec), L.stream()), "stc_bn_bwd_sums")
    x = torch.zeros((1, 2, 2, C), device=DEV)
    xv, dxv = L.nhwc_view(x), L.nhwc_view(torch.full_like(x, NAN))
    t = torch.ones(C, device=DEV)
    recs = torch.zeros((1, C, 2), device=DEV)

    def apply(world=1, count=4, recs_=recs, drop=None, g1=xv, C_=C):
        return l.stc_bn_bwd_apply_sync(L.F32, 1, xv, C_, L.ptr(t), L.ptr(t), L.ptr(t), L.ptr(t), L.ptr(t), g1, 0.0,
                                       L.NULL_VIEW, 0.0, drop, L.ptr(recs_), world, count, dxv, L.stream())

    refused(apply(world=0), "world=0")
    refused(apply(count=3), "count=3")
    refused(apply(recs_=None), "missing")
    refused(apply(C_=6), "bad C=6")
    d = ops._drop((ops.dropout_state_tensor(1, 0, DEV), 1, 0.5, 2, 2))
    refused(apply(drop=ctypes.byref(d), g1=L.NULL_VIEW), "needs g1")
    torch.cuda.synchronize()
    assert bool(torch.isnan(rec).all()) and bool(torch.isnan(dxv._keep).all()), "a refused call wrote something"
    assert apply() == 0


def test_ratios_summary():
    """(last: prints the worst error / bound of every quantity of this file's run.)"""
    for k in sorted(R.WORST):
        if k.startswith(("a.", "b.")):
            print(f"[syncbn_kernels] worst {k}: {R.WORST[k]:.4f}")
