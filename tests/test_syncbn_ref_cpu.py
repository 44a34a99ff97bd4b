"""No GPU: the references, operands and bounds of tests/syncbn_ref.py checked against themselves and against torch;
parallel.gather_records on a gloo world of 3 CPU processes; and the public surface of nn.SyncBatchNorm networks
(state_dict keys, process_group refusal, args.norm values, conversion before the first forward plans as sync)."""
import functools

import pytest
import torch
import torch.distributed as dist
import torch.nn as nn
import torch.nn.functional as F

import dropout_ref as R
import syncbn_ref as S
from dropout_ref import BF16, F32, F64

DTS = [F32, BF16]


# ================================================================ operands and references
@pytest.mark.parametrize("dt", DTS, ids=R.dtname)
@pytest.mark.parametrize("cg", S.CGS)
def test_exact_batch_meets_its_preconditions(cg, dt):
    """Every sample's mean is a_c exactly, the values are exact in the storage type, and every sum a chunk or a merge
    forms -- shifted by the chunk's first pixel, as chan_stats_kernel does -- is an integer below 2^24 in units of
    1/64."""
    C = cg * R.vec(dt)
    for shards in S.SHARDS:
        x, a = S.exact_batch(sum(shards), *S.HW, C, 1)
        assert torch.equal(R.stored(x, dt), x)
        xd = x.double()
        assert torch.equal(xd.mean(dim=(1, 2)), a.double().expand(sum(shards), C))
        for xs in S.split(xd, shards):
            flat = xs.reshape(-1, C)
            nch = R.stat_chunks(flat.shape[0])
            per = -(-flat.shape[0] // nch)
            for k in range(nch):
                ch = flat[k * per:(k + 1) * per]
                d = ch - ch[0]
                for s in (d.abs().sum(0), (d * d).sum(0)):
                    u = s * 64
                    assert torch.equal(u, u.round()) and float(u.max()) < R.LIMIT
            st = S.whole_stats(xs)
            assert torch.equal(st["mean"], a.double())
            rec = S.record_ref(st)
            assert torch.equal(rec[:, 1], torch.zeros(C, dtype=F64)) and torch.equal(rec[:, 3], a.double())
            assert torch.equal(rec[:, 2], st["M2"])  # (fp32 holds it)


@pytest.mark.parametrize("shards", S.SHARDS, ids=str)
def test_records_merge_to_the_whole_batch(shards):
    """record_ref of every shard's fp64 statistics, merged: the whole batch's mean within 2^-46 of its magnitude and
    variance within 2^-23 relative (the record's documented loss).  The same records with shift = 0 lose the mean's
    fp32 rounding of N * mean, 2^15 times more: what the choice of shift is for."""
    x = S.real_batch((sum(shards), *S.HW, 12), F32, 2) + 100.0
    ref = S.whole_stats(x)
    sts = [S.whole_stats(xs) for xs in S.split(x, shards)]
    N, mean, M2 = S.merge_records(torch.stack([S.record_ref(st) for st in sts]))
    assert float(N[0]) == ref["N"]
    err = (mean - ref["mean"]).abs()
    assert bool((err <= 2.0 ** -46 * ref["mean"].abs()).all()), float((err / ref["mean"].abs()).max())
    live = ref["var"] > 0
    assert bool(((M2 / N - ref["var"]).abs()[live] <= 2.0 ** -23 * ref["var"][live]).all())
    zero = []
    for st in sts:  # shift = 0: S1 = N * mean, S2 = M2 + N * mean^2
        n = float(st["N"])
        zero.append(torch.stack([torch.full_like(st["mean"], n), (n * st["mean"]).float().double(),
                                 (st["M2"] + n * st["mean"] ** 2).float().double(), torch.zeros_like(st["mean"])], -1))
    _, mean0, _ = S.merge_records(torch.stack(zero))
    assert float((mean0 - ref["mean"]).abs().max()) > 2.0 ** 15 * float(err.max())


def test_finalize_ref_is_torch_batch_norm():
    """finalize_ref of the whole batch's statistics: F.batch_norm's output table and running buffers (fp64)."""
    x = S.real_batch((3, *S.HW, 12), F32, 2).double()
    g = torch.Generator().manual_seed(5)
    gam, bet, rm, rv = (torch.rand(12, generator=g, dtype=F64) + 0.5 for _ in range(4))
    st = S.whole_stats(x)
    ref = S.finalize_ref(float(st["N"]), st["mean"], st["M2"], gam, bet, rm, rv)
    rm_t, rv_t = rm.clone(), rv.clone()
    y = F.batch_norm(x.permute(0, 3, 1, 2), rm_t, rv_t, gam, bet, True, S.MOM, S.BN_EPS).permute(0, 2, 3, 1)
    assert torch.allclose(x * ref["scale"][0] + ref["shift"][0], y, rtol=0, atol=1e-12)
    assert torch.allclose(ref["running_mean"][0], rm_t, rtol=0, atol=1e-12)
    assert torch.allclose(ref["running_var"][0], rv_t, rtol=0, atol=1e-12)


@pytest.mark.parametrize("case", S.BWD_CASES + [S.MASKED], ids=lambda c: c.id)
def test_sharded_backward_is_autograd_of_the_whole_batch(case):
    """The sync backward of the references -- per-shard dn (each shard's own mask), sums over all shards, dx with the
    global sums and count -- is torch autograd through F.batch_norm of the WHOLE batch and the masked activations
    (fp64); per-rank statistics instead miss it.  Exact cases meet dropout_ref's exact-sum preconditions."""
    dt, shards = F32, (2, 1)
    x, st5, g1, g2 = R.bwd_inputs(case, dt)
    C = case.C(dt)
    # the statistics must be the data's own for autograd to agree: tables of x itself, in fp64
    xd = x.double().requires_grad_(True)
    gam = st5[4].double()
    mean = xd.detach().mean(dim=(0, 1, 2))
    rstd = 1.0 / torch.sqrt(((xd.detach() - mean) ** 2).mean(dim=(0, 1, 2)) + S.BN_EPS)
    bet = torch.linspace(-0.5, 0.5, C, dtype=F64)
    state = (gam * rstd, bet - mean * gam * rstd, mean, rstd, gam)
    refs, whole = S.shard_refs(case, dt, x, state, g1, g2, shards)
    n = F.batch_norm(xd.permute(0, 3, 1, 2), None, None, gam, bet, True, 0.0, S.BN_EPS).permute(0, 2, 3, 1)
    keep = torch.cat(S.shard_keeps(case, dt, shards)).double() * float(R.scale32(case.p))
    loss = (g1.double() * F.leaky_relu(n * keep, R.slope32(case.s1))).sum()
    if g2 is not None:
        loss = loss + (g2.double() * F.leaky_relu(n, R.slope32(case.s2))).sum()
    loss.backward()
    P = x.numel() // C
    dx, _ = R.dx_ref(x, state, whole, whole["dgamma"], whole["dbeta"], P)
    assert float((dx - xd.grad).abs().max()) <= 1e-9 * float(xd.grad.abs().max() + 1.0)
    # per-rank sums and counts (what a network without sync statistics computes) do not give that
    local = torch.cat([R.dx_ref(xs, state, r, r["dgamma"], r["dbeta"], xs.numel() // C)[0]
                       for xs, r in zip(S.split(x, shards), refs)])
    assert float((local - xd.grad).abs().max()) > 1e-3 * float(xd.grad.abs().max())
    if case.sums_exact:
        ex, st_ex, a, b = R.bwd_inputs(case, dt)
        _, w = S.shard_refs(case, dt, ex, st_ex, a, b, shards)
        R.require_exact_sums(w)


def test_dx_bound_counts_the_products_of_k0():
    """A plain fp32 evaluation of dx = k1 dn - (k2 x + k0) with the exact global sums: inside S.dx_ref's bound in every
    case and sharding, while dropout_ref's bound alone is missed where k0's two products cancel."""
    worst_old = worst_new = 0.0
    for case0 in S.BWD_CASES:
        for shards in S.SHARDS:
            case = S.with_batch(case0, sum(shards))
            x, st5, g1, g2 = R.bwd_inputs(case, F32)
            _, whole = S.shard_refs(case, F32, x, st5, g1, g2, shards)
            C = case.C(F32)
            P = x.numel() // C
            db, dg = whole["dbeta"].float(), whole["dgamma"].float()
            _, _, mean, rstd, gam = (t.float() for t in st5)
            invP = torch.tensor(1.0, dtype=F32) / torch.tensor(float(P), dtype=F32)
            k1 = gam * rstd
            k2 = k1 * rstd * dg * invP
            k0 = k1 * (db * invP - mean * rstd * dg * invP)
            d = k1 * whole["dn"].float() - (k2 * x.float() + k0)
            val, old = R.dx_ref(x, st5, whole, dg, db, P)
            _, new = S.dx_ref(x, st5, whole, dg, db, P)
            err = (d.double() - val).abs()
            worst_old = max(worst_old, float((err / old.clamp_min(1e-300)).max()))
            worst_new = max(worst_new, float((err / new.clamp_min(1e-300)).max()))
    assert worst_old > 1.0 and worst_new <= 0.5, (worst_old, worst_new)


def test_global_sums_are_rank_ordered_fp64_sums_rounded_once():
    recs = torch.tensor([[[1.0, 2.0 ** -30]], [[2.0 ** -25, 1.0]], [[2.0 ** -25, -1.0]]])
    db, dg = S.global_sums(recs)
    assert float(db) == float(torch.tensor(1.0 + 2.0 ** -24).float()) and float(dg) == 2.0 ** -30


def test_case_lists_cover_the_issue():
    assert S.SHARDS == ((3,), (1, 2), (2, 1, 1)) and S.CGS == (1, 3, 24, 64) and S.HW == (4, 6)
    assert set(S.LAYOUTS) == {"dense", "hi"}
    assert [R.stat_chunks(p) for p in S.MANY] == [1024, 3]
    assert {c.kind for c in S.BWD_CASES} == {"exact", "real"} and {c.CG for c in S.BWD_CASES} == set(S.CGS)
    assert any(c.g1 == "hi" for c in S.BWD_CASES) and {bool(c.g2) for c in S.BWD_CASES} == {True, False}
    assert any(c.sums_exact for c in S.BWD_CASES) and S.MASKED.p > 0
    assert min(S.PACK_NCH) == 1 and any(1024 < n <= 4096 for n in S.PACK_NCH) and max(S.PACK_NCH) > 4096


# ================================================================ parallel.gather_records, gloo, world 3
def _rank_record(rank):
    g = torch.Generator().manual_seed(40 + rank)
    rec = torch.randn((5, 4), generator=g)
    rec[0, 0] = float(rank + 1)
    rec[1, 1] = -0.0
    rec[2, 2] = float("inf")
    return rec


def _gather_worker(rank, world, port, out):
    S.init_world(rank, world, port)
    try:
        from stcgan_amd import parallel
        got = parallel.gather_records(_rank_record(rank))
        two = parallel.gather_records(_rank_record(rank)[:, :2])  # (a non-contiguous record)
        nb = parallel.global_batch(rank + 1, torch.device("cpu"))
        S.put_result(out, rank, (got, two, nb))
        dist.barrier()
    finally:
        dist.destroy_process_group()


def test_gather_records_gloo_world3():
    """Every rank gets [world, *shape] in rank order, the same bits on every rank and the senders' own bits (a -0
    arrives as +0: the zero-slot sum); a non-contiguous record; global_batch sums unequal local batches."""
    got = S.run_world(_gather_worker, 3)
    want = torch.stack([_rank_record(r) for r in range(3)])
    for r in range(3):
        full, two, nb = got[r]
        assert tuple(full.shape) == (3, 5, 4) and tuple(two.shape) == (3, 5, 2)
        assert torch.equal(full.view(torch.int32), got[0][0].view(torch.int32)), "ranks differ"
        assert torch.equal(full, want) and torch.equal(two, want[:, :, :2])
        assert nb == 1 + 2 + 3
    neg = got[0][0][:, 1, 1]
    assert bool((neg == 0).all()) and not bool(torch.signbit(neg).any())


def test_gather_records_without_a_group():
    from stcgan_amd import parallel
    rec = _rank_record(0)
    out = parallel.gather_records(rec)
    assert tuple(out.shape) == (1, 5, 4) and out.data_ptr() == rec.data_ptr()
    assert parallel.global_batch(5, torch.device("cpu")) == 5


# ================================================================ the public surface
def _nets(norm_layer):
    from stcgan_amd import networks
    return (networks.get_generator(3, 1, ngf=8, norm_layer=norm_layer),
            networks.get_discriminator(4, ndf=8, norm_layer=norm_layer))


def test_state_dict_keys_are_the_batchnorm_networks():
    for a, b in zip(_nets(nn.BatchNorm2d), _nets(nn.SyncBatchNorm)):
        sa, sb = a.state_dict(), b.state_dict()
        assert list(sa) == list(sb)
        assert all(sa[k].shape == sb[k].shape and sa[k].dtype == sb[k].dtype for k in sa)
        b.load_state_dict(sa)
        assert b.norm_kind == "sync_batch" and a.norm_kind == "batch"
        assert sum(isinstance(m, nn.SyncBatchNorm) for m in b.modules()) == \
            sum(isinstance(m, nn.BatchNorm2d) for m in a.modules()) > 0


def test_modes_and_freeze_norm_see_sync_layers():
    g, d = _nets(nn.SyncBatchNorm)
    for net in (g, d):
        assert net.train()._batch_stats() is True and net.eval()._batch_stats() is False
        assert net.train().freeze_norm()._batch_stats() is False
        assert all(not m.training for m in net.modules() if isinstance(m, nn.SyncBatchNorm))
        assert net.freeze_norm(False)._batch_stats() is True
        first = next(m for m in net.modules() if isinstance(m, nn.SyncBatchNorm))
        first.eval()
        with pytest.raises(NotImplementedError, match="mixed"):
            net._batch_stats()


def test_process_group_is_refused():
    from stcgan_amd import engine, networks
    group = object()
    with pytest.raises(NotImplementedError, match="process_group"):
        networks.get_generator(3, 1, ngf=8, norm_layer=functools.partial(nn.SyncBatchNorm, process_group=group))
    with pytest.raises(NotImplementedError, match="process_group"):
        networks.get_discriminator(4, ndf=8, norm_layer=functools.partial(nn.SyncBatchNorm, process_group=group))
    for net, plan in zip(_nets(nn.BatchNorm2d), (engine.GenPlan, engine.DiscPlan)):
        conv = nn.SyncBatchNorm.convert_sync_batchnorm(net, process_group=group)
        with pytest.raises(NotImplementedError, match="process_group"):
            plan(conv)
    with pytest.raises(NotImplementedError):
        networks.get_generator(3, 1, ngf=8, norm_layer=nn.GroupNorm)


def test_conversion_before_the_first_forward_plans_as_sync():
    from stcgan_amd import engine
    for net, plan in zip(_nets(nn.BatchNorm2d), (engine.GenPlan, engine.DiscPlan)):
        before = list(net.state_dict())
        assert plan(net).sync is False
        conv = nn.SyncBatchNorm.convert_sync_batchnorm(net)
        assert conv is net and list(net.state_dict()) == before
        p = plan(net)
        assert p.sync is True and not p.inorm
        assert set(p.norm_names.values()) == {n for n, m in net.named_modules() if isinstance(m, nn.SyncBatchNorm)}
        # without a process group there is one rank: the BatchNorm2d mode, the same launches
        assert engine._norm_mode(p, True) == engine._BATCH and engine._norm_mode(p, False) == engine._RUNNING
    gi, _ = _nets(nn.InstanceNorm2d)
    assert engine.GenPlan(gi).sync is False


def test_args_norm_values():
    from stcgan_amd.stcgan import check_norm
    assert check_norm("batch") is nn.BatchNorm2d and check_norm("instance") is nn.InstanceNorm2d
    assert check_norm("sync_batch") is nn.SyncBatchNorm
    for bad in ("sync", "syncbatch", "group", None, 1, nn.SyncBatchNorm):
        with pytest.raises(ValueError, match="norm"):
            check_norm(bad)
