"""nn.SyncBatchNorm networks and args.norm = "sync_batch": two processes sharing the one GPU (gloo over the device
tensors), ngf 8 at 256 x 256 (the smallest input the 8-level U-Net admits), fp32.

* world 1 (this process, no process group): SyncBatchNorm networks are the BatchNorm2d networks bit for bit.
* network level, UNEQUAL shards 3 + 1 of a batch of 4: each rank runs G (4 -> 3, without and with use_dropout) and
  D (in_c 7) in train mode with loss sum(out * r_shard); the concatenated outputs, input gradients, the parameter
  gradients summed over the ranks and the buffers against a plain torch network on the WHOLE batch -- inorm_ref.RefG /
  RefD with nn.BatchNorm2d in fp64; with dropout the torch U-Net of tests/test_gpu_dropout.py with every rank's exported
  masks.  Tolerances of tests/test_gpu_model.py: output 1e-4; input gradient 2e-5 + 2e-3 |g|; parameter gradients
  2e-4 max|g| + 1e-6 + 2e-3 |g|; buffers 1e-5 + 1e-4 |w|.  Buffers are bit-identical between the ranks.
  Seeds: a ReLU decision inside fp32 rounding moves a whole gradient term in any fp32 implementation, so the weight and
  input seeds are chosen so that the fp64 reference keeps every activation input MARGIN of its own fp32 errors from zero
  (inorm_ref.sign_margin, a property of the torch reference alone; asserted again here), for the masked U-Net
  tests/test_gpu_dropout.py's 1e-5 absolute margin.
* trainer: args.norm = "sync_batch", two train_steps on shards 2 + 2 of global batches of 4, loss types normal and
  rel_avg.  All parameters and buffers bit-identical between the ranks; rank 0 against OracleSTCGAN(shards=1) on the
  global batch at 5e-5 + 1e-4 |w|.  The inputs make the shards differ (0.5 * uniform + a per-sample offset), and the test
  asserts on the CPU that the shards=2 oracle -- per-rank statistics -- misses the shards=1 BatchNorm buffers by at
  least 20 x that tolerance, so a silently per-rank implementation cannot pass.  The per-call collective lists are
  equal on both ranks.  STCGAN.capture refuses."""
import functools
import types

import pytest
import torch
import torch.distributed as dist
import torch.nn as nn

import syncbn_ref as S
from fixture_init import fixture_state, normal, pm_one, uniform
from inorm_ref import RefD, RefG, randomise_affine, sign_margin

pytestmark = pytest.mark.gpu
DEV = "cuda"
NETS = ("G1", "G2", "D1", "D2")
NET_SEED = {"G1": 11, "G2": 12, "D1": 13, "D2": 14}
# At a batch of 4 no weight / input seed pair of the 288 tried (weight seeds 2-13, input seeds 501-524) reaches the
# margin of 8 that the batch-of-2 tests use (best 5.15: ~2e7 activation inputs per forward compete for the minimum).
# e is at least the rms fp32 error of the element's tensor, so 4 asks an independent fp32 implementation to err by more
# than 4 rms errors on one of the few elements at the minimum before a decision can flip.
MARGIN = 4.0
DROP_SEED, DROP_OFFSET = 0x1234ABCD5678, (1 << 32) + 7
SHARDS = (3, 1)
# (kind, use_dropout) -> (in_c, out_c, weight seed, input seed): G the best of the pairs tried (5.15), D and the masked
# U-Net the first input seed that meets the margin (9.59; 1.6e-5)
CONFIGS = {("G", False): (4, 3, 11, 504), ("G", True): (4, 3, 1, 604), ("D", False): (7, 1, 1, 506)}


def bn_state(kind, drop):
    """The state_dict of the configuration's BatchNorm2d network: weights_init, then affine parameters off (1, 0)."""
    from stcgan_amd import networks
    in_c, out_c, wseed, _ = CONFIGS[(kind, drop)]
    net = (networks.get_generator(in_c, out_c, ngf=8, use_dropout=drop) if kind == "G" else
           networks.get_discriminator(in_c, ndf=8))
    torch.manual_seed(wseed)
    net.apply(networks.weights_init)
    randomise_affine(net, wseed + 100)
    return {k: v.detach().clone() for k, v in net.state_dict().items()}


def make_net(kind, drop, norm_layer):
    from stcgan_amd import networks
    in_c, out_c, _, _ = CONFIGS[(kind, drop)]
    net = (networks.get_generator(in_c, out_c, ngf=8, norm_layer=norm_layer, use_dropout=drop) if kind == "G" else
           networks.get_discriminator(in_c, ndf=8, norm_layer=norm_layer))
    net.load_state_dict(bn_state(kind, drop))
    return net.to(DEV).train()


def inputs(kind, drop):
    in_c, out_c, _, xseed = CONFIGS[(kind, drop)]
    x = uniform((sum(SHARDS), in_c, 256, 256), xseed)
    oshape = (sum(SHARDS), out_c, 256, 256) if kind == "G" else (sum(SHARDS), 1, 30, 30)
    return x, normal(oshape, xseed + 1)


def run_net(net, x, r):
    """One train-mode forward / backward with loss sum(out * r): CPU copies of everything a caller compares."""
    xg = x.to(DEV).requires_grad_(True)
    out = net(xg)
    assert tuple(out.shape) == tuple(r.shape), (out.shape, r.shape)
    (out * r.to(DEV)).sum().backward()
    torch.cuda.synchronize()
    return dict(out=out.detach().cpu(), gx=xg.grad.cpu(), grads={k: p.grad.cpu() for k, p in net.named_parameters()},
                bufs={k: b.detach().cpu().clone() for k, b in net.named_buffers()})


# ================================================================ world 1
@pytest.mark.parametrize("kind,drop", list(CONFIGS), ids=lambda v: str(v))
def test_world1_is_batchnorm2d_bit_for_bit(kind, drop):
    assert not dist.is_initialized()
    x, r = inputs(kind, drop)
    res = []
    for nl in (nn.BatchNorm2d, nn.SyncBatchNorm):
        net = make_net(kind, drop, nl)
        if drop:
            net.set_dropout_seed(DROP_SEED, DROP_OFFSET)
        net.sync_log = []
        res.append(run_net(net, x, r))
        assert net.sync_log == []  # (no call on sync statistics: one rank)
    a, b = res
    assert torch.equal(a["out"], b["out"]) and torch.equal(a["gx"], b["gx"])
    for key in ("grads", "bufs"):
        assert list(a[key]) == list(b[key])
        for k in a[key]:
            assert torch.equal(a[key][k], b[key][k]), (key, k)


# ================================================================ network level, shards 3 + 1
def _net_worker(rank, world, port, out):
    S.init_world(rank, world, port)
    try:
        from stcgan_amd import engine, ops
        torch.cuda.set_device(0)
        lo = sum(SHARDS[:rank])
        res = {}
        for (kind, drop) in CONFIGS:
            x, r = inputs(kind, drop)
            net = make_net(kind, drop, nn.SyncBatchNorm)
            net.sync_log = []
            if drop:
                net.set_dropout_seed(DROP_SEED + rank, DROP_OFFSET)
            one = run_net(net, x[lo:lo + SHARDS[rank]], r[lo:lo + SHARDS[rank]])
            one["log"] = [[tuple(c) for c in call] for call in net.sync_log]
            if drop:  # this rank's masks, from the library's export: {level: NCHW keep / (1 - p)}
                sizes = engine._sizes(256, 256, 8)
                one["masks"] = {}
                for k in (4, 5, 6):
                    fh, fw = engine._pad2(sizes, k)
                    m = ops.dropout_mask(ops.dropout_state_tensor(DROP_SEED + rank, DROP_OFFSET, DEV), k,
                                         (SHARDS[rank], fh, fw, 64), p=0.5)
                    one["masks"][k] = m.permute(0, 3, 1, 2).float().cpu() / 0.5
            res[f"{kind}{int(drop)}"] = one
        S.put_result(out, rank, res)
        dist.barrier()
    finally:
        dist.destroy_process_group()


@functools.lru_cache(maxsize=None)
def net_world():
    return S.run_world(_net_worker, len(SHARDS))


def close(what, got, want, atol, rtol, fails):
    err = (got.double() - want.double()).abs()
    lim = atol + rtol * want.double().abs()
    ratio = float((err / lim).max())
    print(f"[syncbn_dist] {what}: max err {float(err.max()):.3e}, error/bound {ratio:.3f}")
    if not ratio <= 1.0:
        fails.append(f"{what}: max err {float(err.max()):.3e}, error/bound {ratio:.3f}")


def compare_with_whole_batch(tag, ranks, ref):
    """ranks: the per-rank results; ref: dict(out, gx, grads, bufs) of the torch network on the whole batch."""
    fails = []
    close(f"{tag} output", torch.cat([r["out"] for r in ranks]), ref["out"], 1e-4, 0.0, fails)
    close(f"{tag} input grad", torch.cat([r["gx"] for r in ranks]), ref["gx"], 2e-5, 2e-3, fails)
    assert set(ranks[0]["grads"]) == set(ref["grads"])
    for k, g in ref["grads"].items():
        close(f"{tag} grad {k}", sum(r["grads"][k].double() for r in ranks), g, 2e-4 * float(g.abs().max()) + 1e-6,
              2e-3, fails)
    assert set(ranks[0]["bufs"]) == set(ref["bufs"]) and ref["bufs"]
    for k, b in ref["bufs"].items():
        for i, r in enumerate(ranks):  # every rank holds the global statistics, the same bits
            assert torch.equal(r["bufs"][k], ranks[0]["bufs"][k]), f"{tag} buffer {k}: rank {i} differs from rank 0"
        if b.is_floating_point():
            close(f"{tag} buffer {k}", ranks[0]["bufs"][k], b, 1e-5, 1e-4, fails)
        else:
            assert torch.equal(ranks[0]["bufs"][k], b), (tag, k)
    assert not fails, fails


def check_logs(ranks, n_norm):
    """One collective per normed layer and direction, in the same host order on every rank."""
    logs = [r["log"] for r in ranks]
    assert all(lg == logs[0] for lg in logs), logs
    (call,) = logs[0]
    assert len(call) == 2 * n_norm and [d for _, d in call] == ["forward"] * n_norm + ["backward"] * n_norm
    assert len({n for n, _ in call}) == n_norm


@pytest.mark.parametrize("kind", ["G", "D"])
def test_unequal_shards_match_the_whole_batch(kind):
    in_c, out_c, _, _ = CONFIGS[(kind, False)]
    x, r = inputs(kind, False)
    sd = bn_state(kind, False)

    def fresh():
        m = RefG(in_c, out_c, 8, 8, nn.BatchNorm2d) if kind == "G" else RefD(in_c, 8, 3, nn.BatchNorm2d)
        m.load_state_dict(sd)
        return m

    margin = sign_margin(fresh, x)
    assert margin >= MARGIN, f"{kind}: an activation decision within fp32 rounding (margin {margin:.2f})"
    ref = fresh().double().train()
    x64 = x.double().requires_grad_(True)
    out = ref(x64)
    (out * r.double()).sum().backward()
    want = dict(out=out.detach(), gx=x64.grad, grads={k: p.grad for k, p in ref.named_parameters()},
                bufs={k: b.detach() for k, b in ref.named_buffers()})
    got = net_world()
    ranks = [got[i][f"{kind}0"] for i in range(len(SHARDS))]
    compare_with_whole_batch(f"{kind} shards {SHARDS}", ranks, want)
    check_logs(ranks, 13 if kind == "G" else 3)
    # per-rank statistics would be far away: rank 1's lone sample normalised alone
    alone = fresh().double().train()
    with torch.no_grad():
        far = float((alone(x[3:].double()) - out.detach()[3:]).abs().max())
    assert far > 100 * 1e-4, far


def test_unequal_shards_with_dropout_match_the_whole_batch():
    from test_gpu_dropout import _params, unet
    x, r = inputs("G", True)
    got = net_world()
    ranks = [got[i]["G1"] for i in range(len(SHARDS))]
    masks = {k: torch.cat([rk["masks"][k] for rk in ranks]) for k in (4, 5, 6)}
    assert all(not torch.equal(ranks[0]["masks"][k][:1], ranks[1]["masks"][k]) for k in masks)  # per-rank masks
    ps = _params(bn_state("G", True))
    xr = x.clone().requires_grad_(True)
    margins = []
    yr = unet(ps, xr, True, masks, margins)
    assert min(m for _, m in margins) >= 1e-5, sorted(margins, key=lambda t: t[1])[:3]
    (yr * r).sum().backward()
    names = [k for k in ps if ps[k].requires_grad]
    want = dict(out=yr.detach(), gx=xr.grad, grads={k: ps[k].grad for k in names},
                bufs={k: v.detach() for k, v in ps.items() if k not in names})
    compare_with_whole_batch(f"G dropout shards {SHARDS}", ranks, want)
    check_logs(ranks, 13)


# ================================================================ the trainer, shards 2 + 2
OFFS = (-0.5, -0.4, 0.4, 0.5)


def global_batches(n=2, bs=4, seed=2100):
    """tests/test_gpu_dist.py's seeds; x and y scaled and offset per sample so that the two shards differ."""
    off = torch.tensor(OFFS).reshape(bs, 1, 1, 1)
    return [(0.5 * uniform((bs, 3, 256, 256), seed + 10 * i) + off, pm_one((bs, 1, 256, 256), seed + 10 * i + 1),
             0.5 * uniform((bs, 3, 256, 256), seed + 10 * i + 2) + off) for i in range(n)]


def _trainer(loss_type):
    from stcgan_amd.stcgan import STCGAN
    torch.manual_seed(5)
    a = types.SimpleNamespace(devices=["cuda:0"], tasks=["train"], lr_G=5e-5, lr_D=2e-5, beta1=0.5, beta2=0.999,
                              D_loss_fn="standard", D_loss_type=loss_type, ngf=8, dtype="fp32", norm="sync_batch",
                              load_weights_g1=None, load_weights_g2=None, load_weights_d1=None, load_weights_d2=None)
    tr = STCGAN(a)
    for name in NETS:
        net = getattr(tr, name)
        net.load_state_dict(fixture_state(net.state_dict(), NET_SEED[name], "ref"))
    return tr


def _train_worker(rank, world, port, loss_type, out):
    S.init_world(rank, world, port)
    try:
        torch.cuda.set_device(0)
        tr = _trainer(loss_type)
        assert all(isinstance(m, nn.SyncBatchNorm) for n in NETS for m in getattr(tr, n).modules()
                   if isinstance(m, torch.nn.modules.batchnorm._BatchNorm))
        logs = {n: [] for n in NETS}
        for n in NETS:
            getattr(tr, n).sync_log = logs[n]
        for x, m, y in global_batches():
            b = x.shape[0] // world
            x, m, y = (t[rank * b:(rank + 1) * b].contiguous().cuda() for t in (x, m, y))
            tr.train_step(x, m, y)
            for n in NETS:
                getattr(tr, n).grad_exchange.check_order()
        torch.cuda.synchronize()
        refused = False
        try:
            tr.capture(x, m, y)
        except NotImplementedError as e:
            refused = "sync_batch" in str(e)
        state = {n: {k: v.detach().cpu().clone() for k, v in getattr(tr, n).state_dict().items()} for n in NETS}
        S.put_result(out, rank, dict(state=state, refused=refused,
                                     logs={n: [[tuple(c) for c in call] for call in logs[n]] for n in NETS}))
        dist.barrier()
    finally:
        dist.destroy_process_group()


@functools.lru_cache(maxsize=None)
def oracle_state(loss_type, shards):
    from oracle import stcgan_ref as ref
    templ = {"G1": ref.generator_state_template(3, 1, 8), "G2": ref.generator_state_template(4, 3, 8),
             "D1": ref.discriminator_state_template(4, 8), "D2": ref.discriminator_state_template(7, 8)}
    orc = ref.OracleSTCGAN({n: fixture_state(templ[n], NET_SEED[n], "ref") for n in NETS}, loss_type=loss_type,
                           shards=shards)
    orc.run_epoch([([], x, m, y) for x, m, y in global_batches()], training=True)
    return {n: {k: v.detach().clone() for k, v in orc.st[n].items()} for n in NETS}


def _tol(w):
    return 5e-5 + 1e-4 * w.double().abs()


@pytest.mark.parametrize("loss_type", ["normal", "rel_avg"])
def test_trainer_sync_batch_matches_the_global_batch_oracle(loss_type):
    from oracle.stcgan_ref import _is_buffer
    whole, per_rank = oracle_state(loss_type, 1), oracle_state(loss_type, 2)
    # the inputs discriminate: per-rank statistics leave every network's BatchNorm buffers >= 20 tolerances away
    for n in NETS:
        worst = max(float(((per_rank[n][k].double() - w.double()).abs() / _tol(w)).max())
                    for k, w in whole[n].items() if _is_buffer(k) and w.is_floating_point())
        print(f"[syncbn_dist] {loss_type} {n}: shards=2 oracle buffers miss shards=1 by {worst:.1f} tolerances")
        assert worst >= 20.0, (n, worst)
    got = S.run_world(_train_worker, 2, (loss_type,))
    assert got[0]["refused"] and got[1]["refused"], "STCGAN.capture did not refuse sync statistics at world 2"
    for n in NETS:  # parameters AND buffers: every rank finalizes from the same records
        for k, v in got[0]["state"][n].items():
            assert torch.equal(v, got[1]["state"][n][k]), (n, k)
        assert got[0]["logs"][n] == got[1]["logs"][n] and got[0]["logs"][n], n
        assert all(call for call in got[0]["logs"][n])
    worst, fails = 0.0, []
    for n in NETS:
        for k, v in got[0]["state"][n].items():
            w = whole[n][k].detach()
            if not v.is_floating_point():
                assert torch.equal(v, w), (n, k)
                continue
            ratio = float(((v.double() - w.double()).abs() / _tol(w)).max())
            worst = max(worst, ratio)
            if not ratio <= 1.0:
                fails.append((n, k, ratio))
    print(f"[syncbn_dist] trainer sync_batch vs shards=1 oracle [{loss_type}]: worst error / tolerance {worst:.3f}")
    assert not fails, fails
