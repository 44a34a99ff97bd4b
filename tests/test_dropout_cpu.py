"""The generator's dropout mask function restated in numpy (include/stcgan_hip.h) and the host-side
pieces of use_dropout=True: seed derivation and the module tree.  No GPU."""
import math

import numpy as np
import pytest

M32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(ctr, key):
    """Philox4x32-10 (Random123): ctr = 4 arrays / ints (uint32 values), key = 2; returns 4 uint64 arrays < 2^32."""
    c = [np.asarray(v, dtype=np.uint64) & M32 for v in ctr]
    k = [np.uint64(int(v) & 0xFFFFFFFF) for v in key]
    m0, m1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
    w0, w1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
    for _ in range(10):
        p0, p1 = m0 * c[0], m1 * c[2]  # 32 x 32 -> 64 bit products
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k[0], p1 & M32, (p0 >> np.uint64(32)) ^ c[3] ^ k[1], p0 & M32]
        k = [(k[0] + w0) & M32, (k[1] + w1) & M32]
    return c


def dropout_mask(seed, offset, level, shape, p):
    """keep (1) / drop (0), uint8 NHWC ``shape`` = the full ConvT extent (B, H, W, C): key = seed (lo, hi), counter =
    (idx >> 2, level, offset lo, offset hi) with idx the NHWC linear index, word idx & 3, keep <=> word >=
    floor(p * 2^32)."""
    n = int(np.prod(shape))
    assert n < 1 << 34 and n % 4 == 0
    q = np.arange(n // 4, dtype=np.uint64)
    words = philox4x32_10((q, level, offset & 0xFFFFFFFF, (offset >> 32) & 0xFFFFFFFF),
                          (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))
    w = np.stack(words, axis=1).reshape(-1)  # element idx: call idx >> 2, word idx & 3
    thr = np.uint64(math.floor(p * 4294967296.0))
    return (w >= thr).astype(np.uint8).reshape(shape)


def test_philox_known_answers():
    """The two Random123 known-answer vectors of philox4x32-10."""
    z = philox4x32_10((0, 0, 0, 0), (0, 0))
    assert [int(v) for v in z] == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    f = 0xFFFFFFFF
    o = philox4x32_10((f, f, f, f), (f, f))
    assert [int(v) for v in o] == [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]


CASES = [((2, 16, 16, 512), 4), ((2, 8, 8, 512), 5), ((2, 4, 4, 512), 6)]


@pytest.mark.parametrize("p", [0.5, 0.2])
@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("shape,level", CASES)
def test_keep_share(shape, level, offset, p):
    m = dropout_mask(1234, offset, level, shape, p)
    n = m.size
    share = float(m.sum()) / n
    sigma = math.sqrt(p * (1 - p) / n)
    print(f"keep share {share:.5f} vs {1 - p} ({abs(share - (1 - p)) / sigma:.2f} sigma)")
    assert abs(share - (1 - p)) <= 4 * sigma


def test_masks_are_independent():
    """Another offset, or another level, is another mask: they agree on about half of the elements at p = 0.5."""
    shape = (2, 16, 16, 512)
    a = dropout_mask(1234, 0, 4, shape, 0.5)
    for other in (dropout_mask(1234, 1, 4, shape, 0.5), dropout_mask(1234, 0, 5, shape, 0.5)):
        agree = float((a == other).mean())
        print(f"agreement {agree:.4f}")
        assert 0.49 <= agree <= 0.51


def test_mask_edges():
    shape = (1, 2, 2, 8)
    assert dropout_mask(5, 0, 4, shape, 0.0).all()  # threshold 0: everything kept
    # the offset's and the seed's high words are part of the function
    assert not np.array_equal(dropout_mask(5, 1 << 32, 4, (2, 8, 8, 64), 0.5), dropout_mask(5, 0, 4, (2, 8, 8, 64), 0.5))
    assert not np.array_equal(dropout_mask(5 + (1 << 32), 0, 4, (2, 8, 8, 64), 0.5),
                              dropout_mask(5, 0, 4, (2, 8, 8, 64), 0.5))


def test_rank_seed_derivation():
    from stcgan_amd import ops
    assert ops.dropout_rank_seed(100) == 100
    assert ops.dropout_rank_seed(100, rank=3) == 103
    # distinct over every (generator, rank) of a run
    seeds = {ops.dropout_rank_seed(7, r, 4, n) for r in range(4) for n in range(2)}
    assert len(seeds) == 8
    assert ops.dropout_rank_seed((1 << 64) - 1, rank=2) == 1  # modulo 2^64
    assert 0 <= ops.dropout_rank_seed(-5) < 1 << 64


@pytest.mark.parametrize("base", [4242, (1 << 64) - 2])
def test_checkpoint_seeds_are_rederived_per_rank(base):
    """A checkpoint is written by rank 0 and read by every rank: it keeps the base seed, and each rank derives its own
    seeds from it -- the ones it was constructed with, distinct over every (generator, rank)."""
    from stcgan_amd import ops
    from stcgan_amd.stcgan import dropout_checkpoint_entry, dropout_from_checkpoint, dropout_trainer_seeds
    world = 4
    built = {r: dropout_trainer_seeds(base, r, world) for r in range(world)}  # what STCGAN.__init__ sets
    assert built[0] == [ops.dropout_rank_seed(base, 0, world, 0), ops.dropout_rank_seed(base, 0, world, 1)]
    entry = dropout_checkpoint_entry(base, [17, 18])  # (rank 0's view: the offsets are the same on every rank)
    seen = set()
    for r in range(world):
        got_base, states = dropout_from_checkpoint(entry, r, world)
        assert got_base == base
        assert [s for s, _ in states] == built[r] and [o for _, o in states] == [17, 18]
        seen.update(s for s, _ in states)
    assert len(seen) == 2 * world
    # another world size at the resume: still distinct per (generator, rank)
    other = {s for r in range(2) for s, _ in dropout_from_checkpoint(entry, r, 2)[1]}
    assert len(other) == 4


def test_set_drop_rate_remakes_the_plan():
    from stcgan_amd import engine, networks
    net = networks.get_generator(3, 1, ngf=8, use_dropout=True)
    net._plan = engine.GenPlan(net)
    assert set(net._plan.drop.values()) == {0.5}
    net.set_drop_rate(0.25)
    assert net._plan is None and set(engine.GenPlan(net).drop.values()) == {0.25}
    with pytest.raises(ValueError):
        net.set_drop_rate(1.0)


def test_state_tensor_round_trip():
    """The unsigned 64-bit seed survives its int64 storage."""
    import torch
    from stcgan_amd import networks, ops
    t = ops.dropout_state_tensor((1 << 64) - 3, 9, "cpu")
    assert t.dtype == torch.int64 and t.tolist() == [-3, 9]
    net = networks.get_generator(3, 1, ngf=8, use_dropout=True)
    assert net.set_dropout_seed((1 << 63) + 5, 2).dropout_state() == ((1 << 63) + 5, 2)
    assert "_drop_state" not in dict(net.named_buffers()) and not any("drop" in k for k in net.state_dict())


@pytest.mark.parametrize("num_downs", [6, 8])
def test_module_tree(num_downs):
    import torch.nn as nn
    from stcgan_amd import engine, networks
    plain = networks.get_generator(4, 3, ngf=8, num_downs=num_downs)
    net = networks.get_generator(4, 3, ngf=8, num_downs=num_downs, use_dropout=True)
    assert list(net.state_dict()) == list(plain.state_dict())
    blocks = [m for m in net.modules() if isinstance(m, networks.UnetSkipConnectionBlock)]
    with_drop = [b for b in blocks if any(isinstance(m, nn.Dropout) for m in b.model)]
    assert len(with_drop) == num_downs - 5
    for b in with_drop:
        assert isinstance(b.model[-1], nn.Dropout) and b.model[-1].p == 0.5 and len(b.model) == 8
        assert sum(isinstance(m, nn.Dropout) for m in b.model) == 1
    assert not any(isinstance(m, nn.Dropout) for m in plain.modules())
    # the plan: the num_downs - 5 blocks directly above the innermost one (levels counted from the outermost, 0)
    plan = engine.GenPlan(net)
    assert plan.drop == {k: 0.5 for k in range(num_downs - 1 - (num_downs - 5), num_downs - 1)}
    assert engine.GenPlan(plain).drop == {}
    net2 = networks.get_generator(4, 3, ngf=8, num_downs=num_downs, use_dropout=True, drop_rate=0.2)
    assert set(engine.GenPlan(net2).drop.values()) <= {0.2} and all(b.model[-1].p == 0.2 for b in [
        m for m in net2.modules() if isinstance(m, networks.UnetSkipConnectionBlock) and len(m.model) == 8])


@pytest.mark.parametrize("bad", [1.0, -0.1, 1.5, "0.5", True, float("nan")])
def test_bad_drop_rate(bad):
    from stcgan_amd import networks
    with pytest.raises(ValueError):
        networks.get_generator(3, 1, ngf=8, use_dropout=True, drop_rate=bad)


def test_bad_module_probability():
    """p is read from the nn.Dropout modules: one set to 1 afterwards is refused when the plan is made."""
    from stcgan_amd import engine, networks
    net = networks.get_generator(3, 1, ngf=8, use_dropout=True)
    next(m for m in net.modules() if m.__class__.__name__ == "Dropout").p = 1.0
    with pytest.raises(ValueError):
        engine.GenPlan(net)
