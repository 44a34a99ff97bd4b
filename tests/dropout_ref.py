"""References, exactly-reproducible operands, derived bounds and the case list for the use_dropout=True kernels of
csrc/bn.hip and csrc/philox.hpp (tests/test_gpu_dropout_family.py; checked without a GPU by
tests/test_dropout_ref_cpu.py).

Plain torch / numpy on the CPU; nothing here calls the HIP library, and nothing comes from a kernel.

Mask.  The numpy Philox4x32-10 of tests/test_dropout_cpu.py, evaluated for an arbitrary index set (b, y, x, c) of a
full extent (B, FH, FW, C): counter (idx >> 2, level, offset lo, offset hi), key = seed (lo, hi), word idx & 3,
keep <=> word >= thresh(p) = floor(p * 2^32); kept values are multiplied by scale32(p) = fl32(1 / (1 - p)).

Forward.  n = x * sc + sh, v = keep ? fl32(n * scale32) : 0, y = act(v, slope), in fp64 from the stored values.  The
operands are x multiples of 1/8 in [-4, 4], sc in {+-1, +-2, 0.5}, sh multiples of 1/4: n is then exact in fp32
(asserted), so fl32(n * scale32) is the correctly rounded fp64 product (24 + 24 bits fit in 53) whatever the scale,
and with slope 0.2 one more fp32 product follows, reproduced the same way.  An fp32 output must EQUAL the reference and
a bf16 output its round-to-nearest-even rounding: this pins "scale in fp32, before the rounding to the storage type".
(sh reaches +-250 in half of the channels, so that n needs more than the 8 bits of a bf16 significand: with a
bf16-exact n the order of scaling and rounding could not be seen.)

Backward.  dn = g1 * keep * scale32 * act1'(n) + g2 * act2'(n); dbeta = sum dn, dgamma = sum dn * xhat with
xhat = (x - mean) * rstd; dx = k1 * dn - (k2 * x + k0).  mean, rstd, scale, shift, gamma are hand-made arrays.
  exact cases: g multiples of 1/8, mean multiples of 1/4, rstd and gamma powers of two, p in {0.5, 0.75, 0.2, 0.6}
    (scales 2, 4, 1.25, 2.5) and slopes in {0, 0.5, 1}: every term is a multiple of a common power of two u and
    sum|terms| / u < 2^24 (asserted), so every partial sum of every order is exact and the partials, dbeta and dgamma
    must EQUAL the fp64 sums.  With slope 0.2 a term g2 * fl32(0.2) is a 24-bit number, no two of which add exactly:
    those cases keep the exact operands and every per-element check, and their sums take the derived bound below.
  bounded cases (EPS32 = 2^-23): a chunk holds per = ceil(P / nchunks) pixels, each thread adds ceil(per / RL) of
    them (RL = 256 // CG lanes), RL lane totals follow, and a term carries two roundings more than the plain kernel's
    (g1 * m, then * act'): a per-channel sum is within m * EPS32 * sum|terms|, m = ceil(per / RL) + RL + 10.  dx is
    within 16 * EPS32 * (|k1 dn| + |k2 x| + |k0|) (the bound tests/test_gpu_bn_family.py derives for bn_bwd_apply, with
    the device's own dgamma / dbeta in the coefficients) + |k1| * EPS32 * (2 |t1| + |t2|), t1 = g1 * m * act1'(n),
    t2 = g2 * act2'(n); bf16: inside the rounding interval of such a value.  The second part is the term's roundings
    counted where they act: fl(fl(g1 * m) * act1') is off by up to 2 roundings of |t1| and fl(g2 * act2') by one of
    |t2|, whatever is left of dn = t1 + t2 after the two cancel, so 16 * EPS32 * |k1 dn| alone does not cover them.
    (A correctly rounded fp32 evaluation of the formula exceeds the first part alone by a factor of 8 at 168 of the
    262148 elements of the P = 65537 case, where |dn| < 1e-3 * (|t1| + |t2|) occurs: tests/test_dropout_ref_cpu.py,
    test_dx_bound_counts_the_terms_roundings.  Without g2, or with t1 and t2 of one sign, the part is at most 1/8 of
    the first.)
"""
import functools
import math

import numpy as np
import torch

from test_dropout_cpu import philox4x32_10

F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16
EPS32 = 2.0 ** -23
LIMIT = float(2 ** 24)
P_MAX = 1.0 - 2.0 ** -24  # thresh 2^32 - 256, scale 2^24
P_ALL = (0.0, 1e-12, 0.1, 0.2, 0.3, 0.5, 0.6, 0.75, 0.9, P_MAX)
SEED, OFFSET = 0x1234ABCD5678, (1 << 32) + 7
SEED_TOP = 0xFFFFFFFFFFFFFFFD  # top bit set: a negative int64 on the device
GRID_CAP = 8192 * 256          # vectors one launch of the element-wise dropout kernels covers without striding

WORST = {}


# ---------------------------------------------------------------- comparison helpers
def note(key, err, bound):
    """Largest error / bound of one quantity (printed: a run with -s records the measured ratios); asserts
    err <= bound element-wise and that the error is finite."""
    err, bound = torch.as_tensor(err, dtype=F64).cpu(), torch.as_tensor(bound, dtype=F64).cpu()
    assert bool(torch.isfinite(err).all()), f"{key}: not finite"
    ratio = float((err / bound.clamp_min(1e-300)).max())
    WORST[key] = max(WORST.get(key, 0.0), ratio)
    print(f"[dropout_family] {key}: error/bound {ratio:.4f}")
    assert bool((err <= bound).all()), f"{key}: error/bound {ratio:.4f} (max err {float(err.max()):.3e}); first at " \
                                       f"{tuple((err > bound).nonzero()[0].tolist()) if err.dim() else ()}"


def assert_same(got, exp, what):
    """torch.equal with a report of where the wrong elements are (dims named d0..); a NaN matches only a NaN."""
    got, exp = got.detach().cpu(), exp.detach().cpu()
    assert got.shape == exp.shape and got.dtype == exp.dtype, (what, got.shape, exp.shape, got.dtype, exp.dtype)
    if torch.equal(got, exp):
        return
    g, e = got.double(), exp.double()
    bad = ~((g == e) | (torch.isnan(g) & torch.isnan(e)))
    if not bool(bad.any()):
        return
    if bad.dim() == 0:
        raise AssertionError(f"{what}: got {float(g)!r} expected {float(e)!r}")
    idx = bad.nonzero()
    dims = ", ".join(f"d{d}: {sorted(set(idx[:, d].tolist()))[:12]}" for d in range(idx.shape[1]))
    first = tuple(idx[0].tolist())
    raise AssertionError(f"{what}: {len(idx)} of {bad.numel()} elements differ (shape {tuple(got.shape)}); indices by "
                         f"dim -- {dims}; first {first}: got {float(g[first])!r} expected {float(e[first])!r}; "
                         f"NaN (unwritten / poisoned): {int(torch.isnan(g).sum())}")


def check_elementwise(key, got, ref, dt, tol):
    """fp32: |got - ref| <= tol.  bf16: got lies between the bf16 roundings of ref -/+ tol, i.e. it is the
    round-to-nearest-even of an fp32 value that close to ref; ratio reported in units of the allowed interval."""
    got, ref, tol = got.double(), ref.double(), tol.double()
    if dt == F32:
        note(key, (got - ref).abs(), tol)
        return
    lo, hi = (ref - tol).float().to(BF16).double(), (ref + tol).float().to(BF16).double()
    mid, half = 0.5 * (lo + hi), 0.5 * (hi - lo)
    err = (got - mid).abs()
    assert bool(torch.isfinite(got).all()), f"{key}: not finite"
    # (an exact hit of a degenerate interval is ratio 0; any miss of it is > 1)
    note(key, torch.where(err <= half, err / half.clamp_min(1e-300), torch.full_like(err, 2.0)).nan_to_num(0.0),
         torch.ones_like(err))


def dtname(dt):
    return "f32" if dt == F32 else "bf16"


def vec(dt):
    return 4 if dt == F32 else 8


def stored(t, dt):
    """fp32 CPU values as the storage type holds them."""
    return t.float() if dt == F32 else t.float().to(BF16).float()


def slope32(s):
    return float(np.float32(s))


# ---------------------------------------------------------------- the mask
def scale32(p):
    """keep / (1 - p) as the kernels hold it: (float)(1.0 / (1.0 - p))."""
    return np.float32(1.0 / (1.0 - p))


def thresh(p):
    """floor(p * 2^32): an element is kept when its Philox word is >= this."""
    return int(math.floor(p * 4294967296.0))


def _key_ctr(seed, offset, level):
    m = 0xFFFFFFFF
    return (seed & m, (seed >> 32) & m), (int(level), offset & m, (offset >> 32) & m)


def words_at(seed, offset, level, extent, b, y, x, c):
    """The 32-bit Philox word (uint64 array) of every element of the index set (b, y, x, c) -- broadcastable integer
    arrays -- over the full extent (B, FH, FW, C)."""
    B, FH, FW, C = extent
    b, y, x, c = (np.asarray(v).astype(np.uint64) for v in (b, y, x, c))
    idx = ((b * np.uint64(FH) + y) * np.uint64(FW) + x) * np.uint64(C) + c
    assert int(idx.max()) < 1 << 34
    key, (lv, o0, o1) = _key_ctr(seed, offset, level)
    w = philox4x32_10((idx >> np.uint64(2), lv, o0, o1), key)
    return np.choose((idx & np.uint64(3)).astype(np.int64), w)


def keep_at(seed, offset, level, extent, p, b, y, x, c):
    """keep (1) / drop (0), uint8, of the index set (b, y, x, c) over the full extent (B, FH, FW, C)."""
    return (words_at(seed, offset, level, extent, b, y, x, c) >= np.uint64(thresh(p))).astype(np.uint8)


def words_view(seed, offset, level, extent, hw=None):
    """words_at of the top-left H x W view of the full extent, [B, H, W, C], with one Philox call per 4 channels."""
    B, FH, FW, C = extent
    H, W = (FH, FW) if hw is None else hw
    assert C % 4 == 0 and H <= FH and W <= FW
    b = np.arange(B, dtype=np.uint64).reshape(B, 1, 1, 1)
    y = np.arange(H, dtype=np.uint64).reshape(1, H, 1, 1)
    x = np.arange(W, dtype=np.uint64).reshape(1, 1, W, 1)
    c = np.arange(0, C, 4, dtype=np.uint64).reshape(1, 1, 1, C // 4)
    idx = ((b * np.uint64(FH) + y) * np.uint64(FW) + x) * np.uint64(C) + c
    assert int(idx.max()) < 1 << 34
    key, (lv, o0, o1) = _key_ctr(seed, offset, level)
    q = (idx >> np.uint64(2)).reshape(-1)
    out = np.empty((q.size, 4), dtype=np.uint64)
    for a in range(0, q.size, 1 << 15):  # (cache-sized pieces: the ten rounds are memory-bound on a whole array)
        out[a:a + (1 << 15)] = np.stack(philox4x32_10((q[a:a + (1 << 15)], lv, o0, o1), key), axis=-1)
    return out.reshape(B, H, W, C)


def keep_view(seed, offset, level, extent, hw, p):
    return torch.from_numpy((words_view(seed, offset, level, extent, hw) >= np.uint64(thresh(p))).astype(np.uint8))


def first_offset_with_kept(seed, level, extent, hw, p, start, count=1 << 16):
    """The first offset >= start at which the view keeps at least one element (p close to 1): how the P_MAX cases'
    offsets below were found; tests/test_dropout_ref_cpu.py asserts that they still do."""
    for off in range(start, start + count):
        if bool((words_view(seed, off, level, extent, hw) >= np.uint64(thresh(p))).any()):
            return off
    raise AssertionError("no offset keeps an element")


# ---------------------------------------------------------------- layouts and cases
# thread layouts CG = C / N (N = 4 fp32, 8 bf16 elements per 16-byte vector): name -> (CG, B, FH, FW)
LAYOUTS = {"cg1": (1, 3, 4, 6), "cg3": (3, 3, 4, 6), "cg24": (24, 3, 4, 6), "cg64": (64, 3, 4, 6),
           "cg256": (256, 1, 2, 3)}
# crops of the 4 x 6 extent: none, one axis, both, a single pixel (cg256: 2 x 3 -> 1 x 3)
CROPS = {"none": (4, 6), "one": (4, 5), "both": (3, 5), "pixel": (1, 1), "row": (1, 3)}
# outputs: (y1 mode, y2 mode or None); hi = the upper channel half of a 2C-wide concat buffer
OUTS = {"cat_dense": ("hi", "dense"), "dense_cat": ("dense", "hi"), "single": ("hi", None)}


class ApplyCase:
    def __init__(self, layout, crop, outs, slopes, table, p, offset=OFFSET, seed=SEED, level=5):
        self.layout, self.crop, self.outs, self.slopes, self.table, self.p = layout, crop, outs, slopes, table, p
        self.offset, self.seed, self.level = offset, seed, level
        self.CG, self.B, self.FH, self.FW = LAYOUTS[layout]
        self.H, self.W = CROPS[crop]
        self.P = self.B * self.H * self.W

    @property
    def id(self):
        return f"{self.layout}-{self.crop}-{self.outs}-s{self.slopes[0]}_{self.slopes[1]}-" \
               f"{'tab' if self.table else 'null'}-p{self.p:.8g}"

    def C(self, dt):
        return self.CG * vec(dt)

    def extent(self, dt):
        return (self.B, self.FH, self.FW, self.C(dt))

    def shape(self, dt):
        return (self.B, self.H, self.W, self.C(dt))


# offsets at which the P_MAX cases keep at least one element of the view (first_offset_with_kept from OFFSET;
# {(layout, dtype name): offset})
P_MAX_OFFSETS = {("cg3", "f32"): OFFSET + 35059, ("cg3", "bf16"): OFFSET + 14460,
                 ("cg64", "f32"): OFFSET + 492, ("cg64", "bf16"): OFFSET + 492}

P_SWEEP = (0.5, 0.2, 0.3, 0.9, P_MAX)
APPLY_CASES = (
    [ApplyCase("cg1", "none", "cat_dense", (0.0, 0.2), True, 0.3),
     ApplyCase("cg1", "pixel", "dense_cat", (0.5, 0.0), True, 0.3),
     ApplyCase("cg3", "one", "single", (0.0, 1.0), False, 0.3),       # has2 = 0, scale = shift = NULL
     ApplyCase("cg3", "none", "dense_cat", (0.0, 1.0), True, 0.1),
     ApplyCase("cg24", "one", "dense_cat", (0.0, 1.0), True, 0.3),
     ApplyCase("cg64", "none", "single", (0.5, 0.0), True, 0.3),
     ApplyCase("cg256", "row", "cat_dense", (0.0, 0.2), True, 0.3)]
    + [ApplyCase("cg3", "both", "cat_dense", (0.0, 0.2), True, p) for p in P_SWEEP]
    + [ApplyCase("cg64", "both", "cat_dense", (0.0, 0.2), True, p, seed=SEED_TOP) for p in P_SWEEP])


def case_offset(case, dt):
    """The case's offset: its own, or for p = P_MAX the recorded one at which the view keeps an element."""
    if case.p == P_MAX:
        return P_MAX_OFFSETS[(case.layout, dtname(dt))]  # (apply cases only)
    return case.offset


def case_keep(case, dt, hw=None, extent=None, p=None):
    return keep_view(case.seed, case_offset(case, dt), case.level, extent or case.extent(dt), hw or (case.H, case.W),
                     case.p if p is None else p)


def _gen(*key):
    seed = 0
    for k in key:
        seed = (seed * 1000003 + int(k)) % ((1 << 31) - 1)
    return torch.Generator().manual_seed(seed)


def exact_table(C, seed, wide=True):
    """sc in {+-1, +-2, 0.5}, sh multiples of 1/4: |sh| <= 2 in the even channels, <= 250 in the odd ones."""
    g = _gen(101, C, seed)
    sc = torch.tensor([1.0, -1.0, 2.0, -2.0, 0.5])[torch.randint(0, 5, (C,), generator=g)]
    sh = torch.randint(-8, 9, (C,), generator=g).float() / 4
    if wide:
        sh[1::2] = torch.randint(-1000, 1001, (C // 2,), generator=g).float() / 4
    return sc, sh


def exact_values(shape, seed, lim=32):
    """Multiples of 1/8 in [-lim/8, lim/8]."""
    return torch.randint(-lim, lim + 1, shape, generator=_gen(103, seed, *shape)).float() / 8


@functools.lru_cache(maxsize=None)
def apply_inputs(case, dt):
    """(x [B, H, W, C] stored values, sc, sh -- both None for the identity table) of an apply case."""
    C = case.C(dt)
    x = exact_values(case.shape(dt), 1)
    sc, sh = exact_table(C, 2) if case.table else (None, None)
    return x, sc, sh


def affine(x, sc, sh):
    """n = x * sc + sh in fp64, asserted exact in fp32 (what fmaf returns, and what the reference may then scale)."""
    n = x.double() if sc is None else x.double() * sc.double() + sh.double()
    assert torch.equal(n.float().double(), n), "n = x * sc + sh is not exact in fp32: a mistake of the test's operands"
    return n


def act_scaled(n, keep, p, slope):
    """y = act(keep ? fl32(n * scale32) : 0, slope) as fp32: every step the correctly rounded fp32 operation."""
    v = torch.where(keep.bool(), (n * float(scale32(p))).float(), torch.zeros((), dtype=F32))
    return torch.where(v > 0, v, (v.double() * slope32(slope)).float())


def apply_ref(x, sc, sh, keep, p, slope, dt):
    """The expected output tensor of the storage type (fp32: the value; bf16: its round-to-nearest-even)."""
    return act_scaled(affine(x, sc, sh), keep, p, slope).to(dt)


def apply_late_scale(x, sc, sh, keep, p, slope, dt):
    """The wrong order: the activation rounded to the storage type first, the scale applied to that."""
    n = affine(x, sc, sh)
    a = torch.where(n > 0, n.float(), (n * slope32(slope)).float()).to(dt).double()
    return torch.where(keep.bool(), (a * float(scale32(p))).float(), torch.zeros((), dtype=F32)).to(dt)


# ---------------------------------------------------------------- backward
class BwdCase:
    """kind 'exact' / 'real'; g1 'dense' or 'hi' (the upper half of a 2C-wide buffer); g2 None or a mode."""

    def __init__(self, layout, crop, p, s1, g2, s2, g1="dense", kind="exact", shape=None, level=5, seed=SEED):
        self.layout, self.crop, self.p, self.s1, self.g2, self.s2, self.g1, self.kind = \
            layout, crop, p, s1, g2, s2, g1, kind
        self.level, self.seed, self.offset = level, seed, OFFSET
        if shape is None:
            self.CG, self.B, self.FH, self.FW = LAYOUTS[layout]
            self.H, self.W = CROPS[crop]
        else:
            self.CG, self.B, self.FH, self.FW, self.H, self.W = shape
        self.P = self.B * self.H * self.W

    @property
    def id(self):
        return f"{self.kind}-{self.layout}-{self.crop}-p{self.p:g}-s{self.s1}-g1{self.g1}-" \
               f"{'g2' + self.g2 + '_s' + str(self.s2) if self.g2 else 'nog2'}"

    C, extent, shape = ApplyCase.C, ApplyCase.extent, ApplyCase.shape

    @property
    def sums_exact(self):
        return self.kind == "exact" and not (self.g2 and self.s2 == 0.2) and self.s1 != 0.2


_LAYOUT_CROP = {"cg1": "none", "cg3": "both", "cg24": "one", "cg64": "both", "cg256": "row"}
BWD_CASES = []
for _l, _c in _LAYOUT_CROP.items():
    BWD_CASES += [BwdCase(_l, _c, 0.5, 0.0, None, 0.0, g1="hi"),          # g2 absent; the concat gradient
                  BwdCase(_l, _c, 0.2, 0.0, "dense", 0.2),
                  BwdCase(_l, _c, 0.75, 0.0, "lo", 1.0, g1="hi"),
                  BwdCase(_l, _c, 0.6, 0.5, "dense", 0.0)]
BWD_CASES += [BwdCase("cg1", "pixel", 0.5, 0.0, "dense", 1.0)]
BIG_P = 65537  # more than 256 chunks: bn_bwd_finalize_kernel<BlockMerge> behind the drop reduce
BWD_CASES += [BwdCase("cg3", "both", 0.3, 0.0, "dense", 0.2, g1="hi", kind="real"),
              BwdCase("cg64", "both", 0.3, 0.2, None, 0.0, kind="real"),
              BwdCase("cg1big", "one", 0.3, 0.0, "dense", 0.2, kind="real", shape=(1, 1, 1, BIG_P + 3, 1, BIG_P))]


def stat_chunks(P):
    return max(1, min(1024, (P + 63) // 64))


def acc_len(P, CG, nch):
    """m of the module docstring."""
    rl = 256 // CG
    per = -(-P // nch)
    return -(-per // rl) + rl + 10


def cpu_tables(x, C, seed):
    """Train-mode BatchNorm tables of x [B, H, W, C] in fp64, rounded to fp32: (scale, shift, mean, rstd, gamma) --
    the stand-in for ops.bn_train_table where there is no GPU."""
    g = _gen(107, C, seed)
    gam = (0.5 + torch.rand(C, generator=g)).float()
    gam[2::3] *= -1.0
    bet = (torch.randn(C, generator=g) * 0.3).float()
    xd = x.double()
    mean = xd.mean(dim=(0, 1, 2))
    rstd = 1.0 / torch.sqrt(((xd - mean) ** 2).mean(dim=(0, 1, 2)) + 1e-5)
    scale = gam.double() * rstd
    return scale.float(), (bet.double() - mean * scale).float(), mean.float(), rstd.float(), gam


def real_x(case, dt):
    """The Gaussian activations of a real-valued case before conditioning (what the tables are taken from)."""
    return stored(torch.randn(case.shape(dt), generator=_gen(109, *case.shape(dt))) * 1.5 + 0.3, dt)


def bwd_inputs(case, dt, tables=None):
    """(x, (scale, shift, mean, rstd, gamma), g1, g2 or None) as stored values.  exact: hand-made exact operands.
    real: Gaussian x and g with ``tables`` (from ops.bn_train_table on real_x; None: cpu_tables), x then moved
    where |n| < 1e-3 so that no activation decision depends on the rounding of n (asserted)."""
    shape, C = case.shape(dt), case.C(dt)
    if case.kind == "exact":
        x = exact_values(shape, 3)
        sc, sh = exact_table(C, 4, wide=False)
        g = _gen(113, C)
        mean = torch.randint(-4, 5, (C,), generator=g).float() / 4
        rstd = torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (C,), generator=g)]
        gam = torch.tensor([0.5, -1.0, 2.0, 1.0])[torch.randint(0, 4, (C,), generator=g)]
        g1 = exact_values(shape, 5, lim=16)
        g2 = exact_values(shape, 6, lim=16) if case.g2 else None
        return x, (sc, sh, mean, rstd, gam), g1, g2
    x = real_x(case, dt)
    tab = tables if tables is not None else cpu_tables(x, C, 7)
    sc, sh = tab[0].double(), tab[1].double()
    for _ in range(8):
        n = x.double() * sc + sh
        near = n.abs() < 1e-3
        if not bool(near.any()):
            break
        x = stored(torch.where(near, x.double() + 0.0625 / sc.abs().clamp_min(1e-3), x.double()), dt)
    assert float((x.double() * sc + sh).abs().min()) >= 1e-3, "conditioning did not converge"
    g = _gen(127, *shape)
    g1 = stored(torch.randn(shape, generator=g), dt)
    g2 = stored(torch.randn(shape, generator=g), dt) if case.g2 else None
    return x, tab, g1, g2


def dact_ref(n, slope):
    return torch.where(n > 0, 1.0, slope32(slope)).double()


def bwd_ref(x, state, keep, p, g1, s1, g2, s2, mask_g2=False, sums=True):
    """fp64 reference of the masked backward: dict of n, dn, the terms' magnitudes (mag = mag1 + mag2), and -- with
    ``sums`` -- xhat and the per-channel sums.  In the exact cases no operation rounds at all, except g2 * fl32(0.2).
    mask_g2: the wrong rule, g2 through the mask too."""
    sc, sh, mean, rstd, _ = (t.double() for t in state)
    n = x.double() * sc + sh
    m = keep.double() * float(scale32(p))
    t1 = g1.double() * m * dact_ref(n, s1)
    if g2 is None:
        dn, mag1, mag2 = t1, t1.abs(), torch.zeros((), dtype=F64)
    else:
        t2 = g2.double() * (m if mask_g2 else 1.0) * dact_ref(n, s2)
        dn, mag1, mag2 = t1 + t2, t1.abs(), t2.abs()
    mag = mag1 + mag2
    out = {"n": n, "dn": dn, "mag": mag, "mag1": mag1, "mag2": mag2}
    if sums:
        xh = (x.double() - mean) * rstd
        out.update({"xh": xh, "dbeta": dn.sum(dim=(0, 1, 2)), "dgamma": (dn * xh).sum(dim=(0, 1, 2)),
                    "abs_dbeta": mag.sum(dim=(0, 1, 2)), "abs_dgamma": (mag * xh.abs()).sum(dim=(0, 1, 2))})
    return out


def chunk_sums(ref, nch):
    """part2[chunk][c] = {sum dn, sum dn * xhat} over the chunk's pixels (per = ceil(P / nch) consecutive pixels of
    the view), and the same of the absolute terms: ([nch, C, 2], [nch, C, 2]) fp64."""
    C = ref["dn"].shape[-1]
    dn, mag, xh = (ref[k].reshape(-1, C) for k in ("dn", "mag", "xh"))
    P = dn.shape[0]
    per = -(-P // nch)
    val = torch.zeros((nch, C, 2), dtype=F64)
    mg = torch.zeros((nch, C, 2), dtype=F64)
    for k in range(nch):
        a, b = k * per, min(P, (k + 1) * per)
        if a < b:
            val[k, :, 0], val[k, :, 1] = dn[a:b].sum(0), (dn[a:b] * xh[a:b]).sum(0)
            mg[k, :, 0], mg[k, :, 1] = mag[a:b].sum(0), (mag[a:b] * xh[a:b].abs()).sum(0)
    return val, mg


def common_unit_total(terms):
    """sum|terms| per channel in units of the largest power of two u that divides every term (<= 2^-0, >= 2^-40)."""
    t = terms.double()
    for k in range(0, 41):
        s = t * 2.0 ** k
        if torch.equal(s, s.round()):
            return s.abs().reshape(-1, t.shape[-1]).sum(0)
    raise AssertionError("the terms have no common power-of-two unit down to 2^-40")


def require_exact_sums(ref):
    """The precondition of exact sums: in their common unit, sum|terms| < 2^24 for dbeta's and dgamma's terms."""
    for name, terms in (("dbeta", ref["dn"]), ("dgamma", ref["dn"] * ref["xh"])):
        tot = common_unit_total(terms)
        # (dn itself may cancel between g1's and g2's term; the bound is on the magnitudes that were added)
        mag = common_unit_total(ref["mag"] if name == "dbeta" else ref["mag"] * ref["xh"].abs())
        assert float(mag.max()) < LIMIT and float(tot.max()) < LIMIT, (name, float(mag.max()))


def compare_sums(tag, case, dt, ref, part, nch, dgamma, dbeta):
    """The reduce's partials and what the finalize makes of them: equal to the fp64 sums (exact cases) or within
    m * EPS32 * sum|terms| (bounded; printed)."""
    val, mg = chunk_sums(ref, nch)
    part, dgamma, dbeta = part.double().cpu(), dgamma.double().cpu(), dbeta.double().cpu()
    if case.sums_exact:
        require_exact_sums(ref)
        assert_same(part, val, f"{tag} part2")
        assert_same(dbeta, ref["dbeta"], f"{tag} dbeta")
        assert_same(dgamma, ref["dgamma"], f"{tag} dgamma")
        return
    m = acc_len(case.P, case.CG, nch)
    note(f"{tag}.part2", (part - val).abs(), m * EPS32 * mg)
    note(f"{tag}.dbeta", (dbeta - ref["dbeta"]).abs(), m * EPS32 * ref["abs_dbeta"])
    note(f"{tag}.dgamma", (dgamma - ref["dgamma"]).abs(), m * EPS32 * ref["abs_dgamma"])


def dx_ref(x, state, ref, dgamma, dbeta, P, family_only=False):
    """(dx, bound) of dx = k1 * dn - (k2 * x + k0) with the given dgamma / dbeta in the coefficients.  bound =
    16 * EPS32 * (|k1 dn| + |k2 x| + |k0|) + |k1| * EPS32 * (2 |t1| + |t2|) (the module docstring); family_only: the
    first part alone, which a correctly rounded fp32 evaluation does not meet where t1 and t2 cancel."""
    _, _, mean, rstd, gam = (t.double() for t in state)
    dgamma, dbeta = dgamma.double().cpu(), dbeta.double().cpu()
    k1 = gam * rstd
    k2 = k1 * rstd * dgamma / P
    k0 = k1 * (dbeta / P - mean * rstd * dgamma / P)
    xd, dn = x.double(), ref["dn"]
    bound = 16 * EPS32 * ((k1 * dn).abs() + (k2 * xd).abs() + k0.abs())
    if not family_only:
        bound = bound + k1.abs() * EPS32 * (2 * ref["mag1"] + ref["mag2"])
    return k1 * dn - k0 - k2 * xd, bound


def compare_dx(tag, dt, got, x, state, ref, dgamma, dbeta, P):
    val, tol = dx_ref(x, state, ref, dgamma, dbeta, P)
    check_elementwise(f"{tag}.dx.{dtname(dt)}", got.double().cpu(), val, dt, tol)


# ---------------------------------------------------------------- grid caps
# one vector per pixel (C = 4 fp32 / 8 bf16): name -> (B, FH, FW, H, W); P just above the cap (some threads run the
# two-in-flight body once, the rest only the tail) and 2.5 caps + 77 (body, then tail, with a ragged end)
GRID_CASES = {"above_cap": (1, 3, 699393, 3, 699392), "2.5_caps": (1, 1, 5242960, 1, 5 * GRID_CAP // 2 + 77)}


# ---------------------------------------------------------------- coverage map
def coverage():
    """What the case lists reach, from the lists alone (see test_cases_meet_every_path)."""
    cov = {"apply_cg": {c.CG for c in APPLY_CASES}, "bwd_cg": {c.CG for c in BWD_CASES},
           "apply_p": {c.p for c in APPLY_CASES}, "bwd_p": {c.p for c in BWD_CASES},
           "has2_0": any(OUTS[c.outs][1] is None for c in APPLY_CASES),
           "null_table": any(not c.table for c in APPLY_CASES),
           "g2": {bool(c.g2) for c in BWD_CASES}, "g1_hi": any(c.g1 == "hi" for c in BWD_CASES),
           "chunks": {stat_chunks(c.P) > 256 for c in BWD_CASES},
           "idle_lanes": {256 % c.CG != 0 for c in BWD_CASES},
           "grid": {(B * H * W > GRID_CAP, B * H * W > 2 * GRID_CAP) for B, _, _, H, W in GRID_CASES.values()},
           "crops": {c.crop for c in APPLY_CASES}, "outs": {c.outs for c in APPLY_CASES},
           "slopes": {c.slopes for c in APPLY_CASES}}
    return cov
