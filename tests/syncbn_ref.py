"""fp64 references, operands, derived bounds and the case lists of the sync-statistics BatchNorm kernels of csrc/bn.hip
(stc_bn_stats_pack, stc_bn_bwd_sums, stc_bn_bwd_apply_sync; tests/test_gpu_syncbn_kernels.py; checked without a GPU by
tests/test_syncbn_ref_cpu.py).  Plain torch / numpy on the CPU; nothing here calls the HIP library, and nothing comes
from a kernel.  (Also the process runner of the multi-process tests, run_world.)  The backward's references are those
of tests/dropout_ref.py (bwd_ref with every element kept at scale 1 is the plain backward), evaluated per shard and on
the whole batch.

Ranks are emulated by sharding one batch [B, H, W, C] along B (SHARDS); the many-chunk case shards one row of 65667
pixels into 65537 + 130 (MANY).  Every shard is a tensor of its own, with its own chunk partials.

The record.  A rank's chunk partials {n_b, S1_b, S2_b, shift_b} merge (fp64, Chan) into (N, mean, M2).  The record is
    {N, S1 = N d, S2 = M2 + N d^2, shift = fl32(mean)},   d = mean - shift,  |d| <= ulp32(mean) / 2,
which the merge of stc_bn_finalize reads back as mean_b = shift + S1 / N = mean and M2_b = S2 - S1^2 / N = M2.  Any
shift would do in exact arithmetic; this one makes |S1| <= N ulp32(mean) / 2, so the fp32 rounding of S1 moves the
mean by at most 2^-24 * ulp32(mean) / 2 (2^-48 relative), and S1^2 / N <= N ulp32(mean)^2 / 4 is far below one fp32
step of S2 unless the channel is constant to fp32 precision; the fp32 rounding of S2 moves M2, and so the variance,
by at most 2^-24 relative.  N is an integer below 2^24 and exact.  (shift = a chunk's own shift, or 0, would put the whole
N * mean into S1 and lose 2^-24 of the MEAN, which is what the shifted sums exist to avoid.)

Exact operands (exact_batch).  x multiples of 1/8 in [-4, 4] with every sample's second half of pixels mirrored about a
per-channel a_c (a multiple of 1/8): every sample, so every shard and the batch, has mean a_c exactly, and every
(x - shift)^2 and (x - a)^2 is a multiple of 1/64 with sums far below 2^24: the chunk partials are exact in fp32, the
record must EQUAL {N, 0, sum (x - a)^2, a} (M2's fp64 merge is within 1e-15 of a value fp32 holds: it rounds to it),
and the finalize over the records must give mean == a, rstd == fl32(1 / sqrt(M2 / N + eps)) and scale ==
fl32(gamma * that rstd).  (shift, the running updates: a multiply-add the compiler may or may not fuse -- bounded,
below.)

Real-valued operands.  tests/test_gpu_bn_family.py's bounds for one tensor, with the accumulation length of the
LONGEST shard, m = max_r acc_len(P_r): |mean - ref| <= ulp32(ref) + m EPS32 max|x - mean| (the pack's 2^-48 sits inside
the half ulp that bound leaves); variance within 1e-5 relative + 3 EPS32 (var + eps): that file's 2 EPS32 for rstd's
own rounding, and one more for the record's S2.  Downstream of the merge: 4 EPS32 * sum|terms|, as there.
Synthetic partials (the > 1024-chunk pack): pack + finalize of the one record against that file's long-double merge,
at 5 EPS32 * sum|terms| (its 4, and the record's S2).

Backward.  Local sums: stc_bn_bwd_sums must give the bits stc_bn_bwd_apply gives from the same partials (equality, no
bound).  The shards' dbeta / dgamma add up to the whole batch's: exact operands (dropout_ref's, sums_exact) EQUAL the
fp64 sums; otherwise within max_r m_r EPS32 sum|terms|, m_r = dropout_ref.acc_len of shard r.  dx: dropout_ref.dx_ref
with the global sums the kernel forms -- fl32 of the fp64 sum of the ranks' fp32 records, in rank order -- and the
global count in the coefficients, at that module's bound with k0's two products counted (dx_ref below).  world = 1,
count = P: bit-identical to stc_bn_bwd_apply[_drop].
"""
import io
import os
import queue
import socket
import sys
import time
from datetime import timedelta

import numpy as np
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import dropout_ref as R
from dropout_ref import EPS32, F64

MOM = float(np.float32(0.1))
BN_EPS = float(np.float32(1e-5))

SHARDS = ((3,), (1, 2), (2, 1, 1))       # samples per emulated rank; B = 3, 3 and 4
CGS = (1, 3, 24, 64)                     # 16-byte vectors per pixel (C = CG * 4 fp32 / 8 bf16)
HW = (4, 6)
LAYOUTS = ("dense", "hi")                # x itself / the upper half of a 2C-wide concat buffer
MANY = (65537, 130)                      # pixels per shard of the one-vector many-chunk case (1024 and 3 chunks)
PACK_NCH = (1, 257, 1024, 1025, 2049, 4097)  # synthetic partials: both lane policies and every load-group count


def ulp32(t):
    a = np.abs(t.detach().double().numpy().astype(np.float32))
    return torch.from_numpy(np.spacing(a).astype(np.float64))


def split(t, shards, dim=0):
    """The shards of a batch tensor (views)."""
    assert sum(shards) == t.shape[dim]
    return list(torch.split(t, list(shards), dim=dim))


def acc_len_stats(P, CG):
    """m of tests/test_gpu_bn_family.py for a per-channel fp32 reduction over P pixels at CG vectors per pixel."""
    rl = 256 // CG
    per = -(-P // R.stat_chunks(P))
    return -(-per // rl) + rl + 8


# ---------------------------------------------------------------- forward operands
def exact_batch(B, H, W, C, seed):
    """(x [B, H, W, C], a [C]): module docstring.  H * W must be even."""
    assert (H * W) % 2 == 0
    g = torch.Generator().manual_seed(7000 + seed + 13 * C)
    a = torch.randint(-8, 9, (C,), generator=g).float() / 8
    half = torch.randint(-16, 17, (B, H * W // 2, C), generator=g).float() / 8
    x = torch.cat([a + half, a - half], dim=1).reshape(B, H, W, C)
    assert float(x.abs().max()) <= 4.0
    return x, a


def real_batch(shape, dt, seed):
    g = torch.Generator().manual_seed(7100 + seed + shape[-1])
    x = torch.randn(shape, generator=g) * 2.0 + 1.25
    x[..., 1] = 2.5  # a constant channel
    return R.stored(x, dt)


def whole_stats(x):
    """fp64 statistics of the whole batch x [..., C]: dict of N, mean, M2, var (biased), unb, dev = max|x - mean|."""
    xd = x.double().reshape(-1, x.shape[-1])
    N = xd.shape[0]
    mean = xd.mean(0)
    M2 = ((xd - mean) ** 2).sum(0)
    return {"N": N, "mean": mean, "M2": M2, "var": M2 / N, "unb": M2 / (N - 1) if N > 1 else M2 / N,
            "dev": (xd - mean).abs().amax(0)}


def record_ref(stats):
    """The record [C, 4] (fp64 values of its fp32 fields) of a rank whose merged statistics are ``stats``."""
    mean = stats["mean"]
    shift = mean.float().double()
    d = mean - shift
    N = float(stats["N"])
    return torch.stack([torch.full_like(mean, N), (N * d).float().double(), (stats["M2"] + N * d * d).float().double(),
                        shift], dim=-1)


def merge_records(recs):
    """(N, mean, M2) per channel of records [world, C, 4], by the merge of csrc/bn.hip's header comment, fp64."""
    r = recs.double()
    n, S1, S2, sh = r[..., 0], r[..., 1], r[..., 2], r[..., 3]
    N = n.sum(0)
    mean = (n * sh + S1).sum(0) / N
    q = (S2 - S1 * S1 / n).clamp_min(0.0)
    d = sh + S1 / n - mean
    return N, mean, (q + n * d * d).sum(0)


def finalize_ref(N, mean, M2, gamma, beta, rm, rv):
    """fp64 {name: (value, sum|terms|)} of what stc_bn_finalize makes of merged statistics."""
    var = M2 / N
    rstd = 1.0 / torch.sqrt(var + BN_EPS)
    if torch.is_tensor(N):
        unb = torch.where(N > 1, M2 / (N - 1).clamp_min(1.0), var)
    else:
        unb = M2 / (N - 1) if N > 1 else var
    g, b, rm, rv = (t.double() for t in (gamma, beta, rm, rv))
    scale = g * rstd
    return {"mean": (mean, mean.abs()), "rstd": (rstd, rstd.abs()), "scale": (scale, scale.abs()),
            "shift": (b - mean * scale, b.abs() + (mean * scale).abs()),
            "running_mean": ((1 - MOM) * rm + MOM * mean, ((1 - MOM) * rm).abs() + (MOM * mean).abs()),
            "running_var": ((1 - MOM) * rv + MOM * unb, ((1 - MOM) * rv).abs() + (MOM * unb).abs())}


def stats_bounds(ref, m):
    """(mean bound, variance bound) of real-valued operands: module docstring."""
    return ulp32(ref["mean"]) + m * EPS32 * ref["dev"], 1e-5 * ref["var"] + 3 * EPS32 * (ref["var"] + BN_EPS)


# ---------------------------------------------------------------- backward cases (dropout_ref.BwdCase on B x 4 x 6)
def bwd_case(cg, kind, s1, g2, s2, g1="dense", p=0.0, B=3):
    return R.BwdCase(f"cg{cg}", "none", p, s1, g2, s2, g1=g1, kind=kind, shape=(cg, B, HW[0], HW[1], HW[0], HW[1]))


def with_batch(case, B):
    """The case on a batch of B samples (SHARDS differ in their total)."""
    return bwd_case(case.CG, case.kind, case.s1, case.g2, case.s2, g1=case.g1, p=case.p, B=B)


BWD_CASES = []
for _cg in CGS:
    BWD_CASES += [bwd_case(_cg, "exact", 0.0, None, 0.0, g1="hi"),      # the generator's up path: the concat gradient
                  bwd_case(_cg, "exact", 0.5, "dense", 0.0),            # two consumers, exact sums
                  bwd_case(_cg, "real", 0.0, "dense", 0.2, g1="hi"),    # the generator's down path
                  bwd_case(_cg, "real", 0.2, None, 0.0)]                # the discriminator
MASKED = bwd_case(3, "real", 0.0, None, 0.0, g1="hi", p=0.5)            # a dropout level (per-rank masks)
MANY_CASE = R.BwdCase("cg1many", "none", 0.0, 0.0, "dense", 0.2, kind="real",
                      shape=(1, 1, 1, sum(MANY), 1, sum(MANY)))


def rank_seed(r):
    """The dropout seed of emulated rank r (distinct per rank, as ops.dropout_rank_seed gives)."""
    return R.SEED + r


def shard_keeps(case, dt, shards):
    """The keep masks of the shards: every rank draws over its OWN local extent with its own seed (or all ones)."""
    C = case.C(dt)
    if case.p == 0.0:
        return [torch.ones((b, case.H, case.W, C), dtype=torch.uint8) for b in shards]
    return [R.keep_view(rank_seed(r), case.offset, case.level, (b, case.FH, case.FW, C), (case.H, case.W), case.p)
            for r, b in enumerate(shards)]


def shard_refs(case, dt, x, state, g1, g2, shards, dim=0):
    """dropout_ref.bwd_ref of every shard (its own mask), and the whole batch's dn, mag1, mag2, xh by concatenation."""
    keeps = shard_keeps(case, dt, shards) if dim == 0 else [torch.ones_like(t, dtype=torch.uint8)
                                                            for t in split(x, shards, dim)]
    g2s = split(g2, shards, dim) if g2 is not None else [None] * len(shards)
    refs = [R.bwd_ref(xs, state, k, case.p, a, case.s1, b, case.s2)
            for xs, k, a, b in zip(split(x, shards, dim), keeps, split(g1, shards, dim), g2s)]
    whole = {k: torch.cat([r[k] if r[k].dim() else r[k].expand_as(r["dn"]) for r in refs], dim=dim)
             for k in ("dn", "mag", "mag1", "mag2", "xh")}
    for k in ("dbeta", "dgamma", "abs_dbeta", "abs_dgamma"):
        whole[k] = sum(r[k] for r in refs)
    return refs, whole


def global_sums(recs):
    """(dbeta, dgamma) as stc_bn_bwd_apply_sync forms them from records [world, C, 2]: fp64 sums in rank order,
    rounded to fp32."""
    s = torch.zeros(recs.shape[1:], dtype=F64)
    for r in range(recs.shape[0]):
        s = s + recs[r].double()
    s = s.float()
    return s[:, 0], s[:, 1]


def dx_ref(x, state, ref, dgamma, dbeta, count):
    """(dx, bound) of dx = k1 dn - (k2 x + k0) with the global dgamma / dbeta and the global count in the
    coefficients: dropout_ref.dx_ref's value and bound, plus 16 EPS32 |k1| (|dbeta| + |mean rstd dgamma|) / count.
    k0 = k1 (dbeta / count - mean rstd dgamma / count) is a difference of two rounded products, whose roundings scale
    with the products, not with what is left after they cancel; dropout_ref's 16 EPS32 |k0| counts only the latter.
    Its own cases never cancel that far; the exact-operand case at 64 vectors, shards 2 + 1 + 1, does: the kernels
    missed the uncorrected bound by 2.08 x there, and a plain fp32 evaluation of the formula on the CPU by 3.76 x
    (tests/test_syncbn_ref_cpu.py, test_dx_bound_counts_the_products_of_k0), while world = 1 equals stc_bn_bwd_apply
    bit for bit: a derivation error of the bound, not of the kernel."""
    val, tol = R.dx_ref(x, state, ref, dgamma, dbeta, count)
    _, _, mean, rstd, gam = (t.double() for t in state)
    k0_terms = (dbeta.double().abs() + (mean * rstd * dgamma.double()).abs()) / count
    return val, tol + 16 * EPS32 * (gam * rstd).abs() * k0_terms


def sums_bound(case, pixels):
    """max_r m_r over the shards' pixel counts: every shard's sum is within m_r EPS32 sum|its terms| (dropout_ref), so
    their total is within max_r m_r EPS32 of the whole batch's sum|terms|."""
    return max(R.acc_len(P, case.CG, R.stat_chunks(P)) for P in pixels)


# ---------------------------------------------------------------- multi-process runs that cannot hang
def init_world(rank, world, port):
    """The worker's side: the repository on sys.path, a gloo group with a 120 s timeout on every collective."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for p in (root, os.path.join(root, "shadow-removal-istd_amd"), os.path.join(root, "tests", "golden")):
        if p not in sys.path:
            sys.path.insert(0, p)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=timedelta(seconds=120))


def put_result(out, rank, obj):
    """A worker's result as bytes (not shared-memory tensors: the worker may exit first)."""
    buf = io.BytesIO()
    torch.save(obj, buf)
    out.put((rank, buf.getvalue()))


def run_world(target, world, args=()):
    """Spawn ``world`` processes target(rank, world, port, *args, queue); wait for one result each while polling the
    exit codes (a dead worker fails the test at once), join with timeouts, kill whatever is left.  No retries."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    procs = [ctx.Process(target=target, args=(r, world, port) + tuple(args) + (q,)) for r in range(world)]
    for p in procs:
        p.start()
    got, t0 = {}, time.time()
    try:
        while len(got) < world and time.time() - t0 < 240:
            try:
                r, val = q.get(timeout=1)
                got[r] = val
            except queue.Empty:
                assert all(p.exitcode in (None, 0) for p in procs), [p.exitcode for p in procs]
        assert len(got) == world, "a worker did not answer in time"
        for p in procs:
            p.join(timeout=60)
            assert p.exitcode == 0, [x.exitcode for x in procs]
    finally:
        for p in procs:
            if p.is_alive():
                p.kill()
    return {r: torch.load(io.BytesIO(v), weights_only=True) for r, v in got.items()}
