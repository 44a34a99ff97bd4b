"""tests/edge_loss_ref.py checked without a GPU: the references against torch (torch.cat, F.l1_loss, F.mse_loss,
F.binary_cross_entropy_with_logits, autograd, F.conv2d / F.conv_transpose2d) in fp64, the constant U re-measured,
and the sensitivity of every comparison tests/test_gpu_edge_loss_family.py makes: a missing, a doubled, a
sign-flipped and a misplaced element planted in a copy of the expected output must be rejected by that file's own
comparison functions (``assert_same`` for the exact cases, ``note`` with the derived bound for the others)."""
import pytest
import torch
import torch.nn.functional as F

import edge_loss_ref as R
import test_gpu_edge_loss_family as G

F64, F32, BF = torch.float64, torch.float32, torch.bfloat16


def rejected(fn, *a):
    with pytest.raises(AssertionError):
        fn(*a)


# ---------------------------------------------------------------- references against torch
def test_layout_references():
    g = torch.Generator().manual_seed(1)
    srcs = [torch.randn((2, c, 5, 7), generator=g, dtype=F64) for c in (3, 1, 3)]
    ref = R.gather_ref(srcs, 8)
    cat = torch.cat(srcs, 1)
    assert torch.equal(ref[..., :7], cat.permute(0, 2, 3, 1)) and float(ref[..., 7].abs().max()) == 0
    back = R.scatter_ref(ref, [3, 1, 3], 5, 7)
    assert all(torch.equal(b, s) for b, s in zip(back, srcs))
    crop = R.scatter_ref(ref, [3, 1, 3], 4, 6)
    assert all(torch.equal(b, s[:, :, :4, :6]) for b, s in zip(crop, srcs))
    # the tanh + bias backward against autograd
    q = torch.randn((2, 3, 4, 5), generator=g, dtype=F64).requires_grad_(True)
    b = torch.zeros(3, dtype=F64, requires_grad=True)
    y = torch.tanh(q + b[None, :, None, None])
    gy = torch.randn(y.shape, generator=g, dtype=F64)
    gq, gb = torch.autograd.grad(y, (q, b), gy)
    dq, db = R.tanh_bwd_ref(y.detach(), gy)
    assert float((dq - gq).abs().max()) <= 1e-14 and float((db - gb).abs().max()) <= 1e-13


@pytest.mark.parametrize("kind", [R.L1, R.MSE, R.BCE])
@pytest.mark.parametrize("tensor_target", [False, True])
def test_loss_references(kind, tensor_target):
    g = torch.Generator().manual_seed(2 + kind)
    n = 1000
    p = torch.cat((torch.randn(n - 6, generator=g, dtype=F64) * 3, torch.tensor([0.0, 20.0, -20.0, 89.0, -104.0, 1e4], dtype=F64)))
    if tensor_target:
        t = torch.randn(n, generator=g, dtype=F64) if kind != R.BCE else torch.rand(n, generator=g, dtype=F64) * 2 - 1
    else:
        t = 0.9 if kind == R.BCE else -1.0
    tt = t if torch.is_tensor(t) else torch.full((n,), t, dtype=F64)
    fn = {R.L1: F.l1_loss, R.MSE: F.mse_loss, R.BCE: F.binary_cross_entropy_with_logits}[kind]
    pr = p.clone().requires_grad_(True)
    v = fn(pr, tt)
    (gr,) = torch.autograd.grad(v * 3.0, pr)
    assert abs(float(R.loss_value(kind, p, t) - v.detach())) <= 1e-13 * abs(float(v.detach()))
    ref = R.loss_grad_ref(kind, p, t, 3.0 / n)
    assert float((ref - gr).abs().max()) <= 1e-13 * float(gr.abs().max())


def test_objective_references():
    """combine_d / combine_g are the torch evaluation of the reference's scalar arithmetic on fp32 tensors, and
    grad_scale is the factor autograd applies to a term."""
    v = [torch.tensor(x, dtype=F32) for x in (0.7312, 1.9, 0.333, 21.25)]
    l1, l2, l3 = (torch.tensor(x, dtype=F32) for x in G.LAMBDAS)
    D1 = (v[0] + v[1]) * 0.5
    D2 = (v[2] + v[3]) * 0.5
    D = l2 * D1 + l3 * D2
    for got, exp in zip(R.combine_d(v, G.LAMBDAS[1], G.LAMBDAS[2]), (D, D1, D2)):
        assert torch.equal(got, exp)
    assert torch.equal(R.combine_g(v, *G.LAMBDAS), v[0] + l1 * v[1] + l2 * v[2] + l3 * v[3])
    # autograd through the D objective in fp64 with the fp32 lambdas
    ps = [torch.randn(n, dtype=F64, generator=torch.Generator().manual_seed(n)).requires_grad_(True) for n in (5, 9)]
    w2, w3 = R.f32(0.1), R.f32(0.3)
    obj = w2 * ((F.mse_loss(ps[0], torch.zeros(5, dtype=F64)) + F.mse_loss(ps[0] * 0, torch.zeros(5, dtype=F64))) * 0.5) \
        + w3 * ((F.mse_loss(ps[1], torch.ones(9, dtype=F64)) + 0.0) * 0.5)
    gs = torch.autograd.grad(obj * R.f32(1 / 3), ps)
    for g, p, c, w in zip(gs, ps, (0.0, 1.0), (0.1, 0.3)):
        ref = R.loss_grad_ref(R.MSE, p.detach(), c, R.grad_scale(1 / 3, w, 0.5, p.numel()))
        assert float((ref - g).abs().max()) <= 1e-14
    assert float(R.grad_scale_f32(1 / 3, 0.1, 0.5, 7)) == pytest.approx(R.grad_scale(1 / 3, 0.1, 0.5, 7), rel=4 * R.EPS)


def _pad2(x):
    return F.pad(x, (2, 2, 2, 2))


def taps16(packed, x, stride, Ho, Wo):
    """y[n, oy, ox] = sum_{kh, kw, c} x[c, stride*oy - 1 + kh, stride*ox - 1 + kw] * packed[0][n][kh*4 + kw][c]."""
    xp = _pad2(x)
    y = torch.zeros((packed.shape[1], Ho, Wo), dtype=F64)
    for kh in range(4):
        for kw in range(4):
            win = xp[:, 1 + kh:1 + kh + stride * Ho:stride, 1 + kw:1 + kw + stride * Wo:stride]
            y += torch.einsum("nc,chw->nhw", packed[0, :, kh * 4 + kw, :x.shape[0]], win)
    return y


def taps16_dgrad(packed, dy, Ho, Wo):
    """dx[n, iy, ix] = sum_{kh, kw, c} dy[c, iy + 1 - kh, ix + 1 - kw] * packed[0][n][kh*4 + kw][c]."""
    xp = _pad2(dy)
    y = torch.zeros((packed.shape[1], Ho, Wo), dtype=F64)
    for kh in range(4):
        for kw in range(4):
            win = xp[:, 3 - kh:3 - kh + Ho, 3 - kw:3 - kw + Wo]
            y += torch.einsum("nc,chw->nhw", packed[0, :, kh * 4 + kw, :dy.shape[0]], win)
    return y


def taps_phased(packed, x):
    """y[n, 2i + ph, 2j + pw] = sum_{a, b, c} x[c, i + ph - a, j + pw - b] * packed[ph*2 + pw][n][a*2 + b][c]."""
    C, H, W = x.shape
    xp = _pad2(x)
    y = torch.zeros((packed.shape[1], 2 * H, 2 * W), dtype=F64)
    for ph in range(2):
        for pw in range(2):
            for a in range(2):
                for b in range(2):
                    win = xp[:, 2 + ph - a:2 + ph - a + H, 2 + pw - b:2 + pw - b + W]
                    y[:, ph::2, pw::2] += torch.einsum("nc,chw->nhw", packed[ph * 2 + pw, :, a * 2 + b, :C], win)
    return y


@pytest.mark.parametrize("mode", R.PACK_MODES)
def test_pack_reference_reproduces_torch_convolutions(mode):
    """The layout reference as the operand of explicit tap sums equals torch's convolution of the same weight, for
    the geometry each mode serves: independent of any kernel."""
    P, Q = 3, 5
    W = R.pack_weights(P, Q, 5)
    n_pad, c_pad = G.pack_pads(mode, P, Q, False)
    pk = R.pack_ref(mode, W, n_pad, c_pad)
    cin = Q if mode in R.N_IS_P else P
    nout = P if mode in R.N_IS_P else Q
    x = torch.randint(-8, 9, (cin, 6, 6), generator=torch.Generator().manual_seed(6)).to(F64)
    if mode == R.PACK_CONV_FWD:  # W[co][ci]: Conv2d stride 2 and stride 1
        pairs = [(taps16(pk, x, 2, 3, 3), F.conv2d(x[None], W, None, 2, 1)[0]),
                 (taps16(pk, x, 1, 5, 5), F.conv2d(x[None], W, None, 1, 1)[0])]
    elif mode == R.PACK_CONVT_DGRAD:  # W[ci][co] of a ConvTranspose2d: its input gradient is a stride-2 conv
        z = torch.zeros((1, P, 3, 3), dtype=F64, requires_grad=True)
        (gz,) = torch.autograd.grad(F.conv_transpose2d(z, W, None, 2, 1), z, x[None])
        pairs = [(taps16(pk, x, 2, 3, 3), gz[0])]
    elif mode == R.PACK_CONV_S1_DGRAD:  # W[co][ci] of a stride-1 Conv2d: its input gradient
        z = torch.zeros((1, Q, 7, 7), dtype=F64, requires_grad=True)
        (gz,) = torch.autograd.grad(F.conv2d(z, W, None, 1, 1), z, x[None])
        pairs = [(taps16_dgrad(pk, x, 7, 7), gz[0])]
    elif mode == R.PACK_CONVT_FWD:  # W[ci][co]: ConvTranspose2d stride 2
        pairs = [(taps_phased(pk, x), F.conv_transpose2d(x[None], W, None, 2, 1)[0])]
    else:  # PACK_CONV_DGRAD, W[co][ci] of a stride-2 Conv2d: its input gradient (ConvT geometry)
        z = torch.zeros((1, Q, 12, 12), dtype=F64, requires_grad=True)
        (gz,) = torch.autograd.grad(F.conv2d(z, W, None, 2, 1), z, x[None])
        pairs = [(taps_phased(pk, x), gz[0])]
    for got, exp in pairs:
        assert got.shape[0] == n_pad and torch.equal(got[:nout], exp) and float(got[nout:].abs().max()) == 0
    assert float(pk[:, nout:].abs().max()) == 0 and float(pk[..., cin:].abs().max()) == 0


def test_pack_weights_are_distinct_and_exact():
    for P, Q in G.PACK_SHAPES:
        W = R.pack_weights(P, Q, 1)
        assert W.unique().numel() == P * Q * 16 and (P * Q * 16 > 510 or float(W.abs().max()) < 256)
    W = R.pack_weights(64, 64, 1, unique=False)  # (asserted inside: bf16-exact integers, no zero)
    assert bool((W[..., :-1] != W[..., 1:]).all()) and bool((W[:, :-1] != W[:, 1:]).all())


# ---------------------------------------------------------------- U and the preconditions
def all_bce_inputs():
    xs = [R.bce_inputs(n, n + 1) for n in G.BCE_NS] + [R.bce_inputs(n, n) for n in (257, 4097)]
    xs += G.d_case(True)[1] + G.g_case(True)[0][2:]
    xs += [p for p, k in zip(G.multi8_case()[2], G.MULTI8_KIND) if k == R.BCE]
    return xs


def test_u_covers_four_times_the_cpu_libm():
    worst = max(R.measure_u(x) for x in all_bce_inputs())
    print(f"fp32 CPU expf -> log1pf / reciprocal: worst error {worst:.3f} EPS; U = {R.U}")
    assert 4.0 * worst <= R.U and worst >= 0.5


def test_preconditions_reject_inexact_operands():
    rejected(R.require_loss_exact, torch.tensor([0.3], dtype=F64))
    rejected(R.require_loss_exact, torch.tensor([64.25], dtype=F64))
    R.require_loss_exact(torch.tensor([64.0, 0.0625], dtype=F64))
    rejected(R.require_tanh_exact, torch.tensor([4.0], dtype=F64), 2 ** 14)
    R.require_tanh_exact(torch.tensor([4.0], dtype=F64), 2 ** 14 - 1)
    p, t = R.loss_operands(R.L1, 8193, 3)
    assert bool((p[:3] == t[:3]).all() and (p[4093:4099] == t[4093:4099]).all() and (p[-3:-1] == t[-3:-1]).all())
    y, gy = R.tanh_operands(2, 3, 4, 8, 1)
    dq = R.tanh_bwd_ref(y, gy)[0]
    assert not torch.equal(dq.to(BF).to(F64), dq)  # the bf16 output really rounds


# ---------------------------------------------------------------- sensitivity: layout kernels
def plant_layout(exp):
    """Copies of an expected tensor with one element unwritten (NaN), zero, written also to its neighbour, and with
    the wrong sign."""
    flat = exp.reshape(-1)
    nz = (flat != 0).nonzero().flatten()
    i = int(nz[len(nz) // 2])
    j = i + 1 if i + 1 < flat.numel() and flat[i + 1] != flat[i] else i - 1
    out = []
    for what in ("nan", "zero", "dup", "sign"):
        c = flat.clone()
        if what == "nan":
            c[i] = float("nan")
        elif what == "zero":
            c[i] = 0
        elif what == "dup":
            c[j] = c[i]
        else:
            c[i] = -c[i]
        out.append(c.reshape(exp.shape))
    return out


def layout_expectations():
    for dt in (F32, BF):
        for chans, dims, cpad in (((3, 1, 3), (3, 6, 8), None), ((3, 1, 3, 1), (3, 6, 7), None), ((20,), (2, 5, 7), 24),
                                  ((3,), (3, 6, 8), 4)):
            yield f"gather {chans} {dt}", G.gather_case(chans, *dims, dt, cpad or G.cpad_for(chans, dt))[1]
        for chans, cpad, _ in G.SCATTER_SPLITS[:1] + G.SCATTER_SPLITS[-1:]:
            for dims in G.SCATTER_DIMS:
                for k, e in enumerate(G.scatter_case(chans, cpad, dims, dt)[1]):
                    yield f"scatter {chans} {dims} {dt} [{k}]", e
        for _, B, H, W in G.TANH_SHAPES:
            for C in (1, 3, 4):
                yield f"tanh dq {B}x{C}x{H}x{W} {dt}", G.tanh_case(B, C, H, W, dt, seed=C)[2]


def test_layout_comparisons_see_one_element():
    count = 0
    for key, exp in layout_expectations():
        G.assert_same(exp.clone(), exp, key)
        for bad in plant_layout(exp):
            rejected(G.assert_same, bad, exp, key)
        count += 1
    assert count >= 40
    # an element written outside the view lands in the NaN guard: a NaN expectation matches only a NaN
    e = torch.tensor([float("nan"), 1.0])
    G.assert_same(e.clone(), e, "poison kept")
    rejected(G.assert_same, torch.tensor([0.0, 1.0]), e, "poison overwritten")


def test_tanh_dbias_sees_one_pixel():
    for dt in (F32, BF):
        for _, B, H, W in G.TANH_SHAPES:
            for C in (1, 3, 4):
                _, _, _, exp_db, dq = G.tanh_case(B, C, H, W, dt, seed=C)
                R.require_tanh_exact(dq, B * H * W)  # (one chunk holding every pixel: the loosest case)
                c = C - 1
                px = dq[:, c].reshape(-1)
                v = px[(px != 0).nonzero().flatten()[0]]
                for delta in (-v, v, -2 * v):  # left out, counted twice, wrong sign
                    bad = dq.sum(dim=(0, 2, 3))
                    bad[c] += delta
                    rejected(G.assert_same, bad.to(F32), exp_db, "dbias")


def test_pack_comparison_sees_a_moved_tap():
    for dt in (F32, BF):
        for mode in R.PACK_MODES:
            for P, Q in G.PACK_SHAPES:
                for wide in (False, True):
                    _, exp, n_pad, c_pad = G.pack_case(mode, P, Q, wide, dt)
                    taps = exp.shape[2]
                    for z, n, t, c in ((0, 0, 0, 0), (exp.shape[0] - 1, (P if mode in R.N_IS_P else Q) - 1, taps - 1,
                                                      (Q if mode in R.N_IS_P else P) - 1)):
                        assert float(exp[z, n, t, c]) != 0
                        bad = exp.clone()
                        t2 = t + 1 if t + 1 < taps else t - 1
                        bad[z, n, t2, c], bad[z, n, t, c] = exp[z, n, t, c], exp[z, n, t2, c]
                        rejected(G.assert_same, bad, exp, "pack")
                        bad = exp.clone()
                        bad[z, n, t, c] = 0  # left out
                        rejected(G.assert_same, bad, exp, "pack")
                        bad = exp.clone()
                        bad[z, n_pad - 1, t, c_pad - 1] = exp[z, n, t, c]  # written twice: also into the padding
                        if (n_pad - 1, c_pad - 1) != (n, c):
                            rejected(G.assert_same, bad, exp, "pack")
    # the strided case: magnitudes repeat, neighbouring taps still differ
    _, exp, _, _ = G.pack_case(R.PACK_CONVT_FWD, 64, 40, False, BF, unique=False)
    bad = exp.clone()
    bad[1, 5, 2, 7], bad[1, 5, 3, 7] = exp[1, 5, 3, 7], exp[1, 5, 2, 7]
    rejected(G.assert_same, bad, exp, "pack")


# ---------------------------------------------------------------- sensitivity: loss values and gradients
def value_cases():
    """Every (key, kind, p, t) whose mean the GPU file compares."""
    for name, kind, const in G.FORMS:
        for n in G.NS:
            yield (f"{name} n={n}", kind, *R.loss_operands(kind, n, seed=n, const=const))
    for name, kind, const in (G.FORMS[0], G.FORMS[2]):
        yield (f"{name} stride", kind, *R.loss_operands(kind, G.STRIDE_N, seed=11, const=const))
    for k, (n, c) in enumerate(zip((256 * 4096 + 1, 1, 4097, 255), (0.0, 1.0, 0.0, 1.0))):  # test_multi_fwd_many_partials
        yield (f"many partials [{k}]", R.MSE, *R.loss_operands(R.MSE, n, 90 + k, const=c))
    for n in (257, 4097):
        yield (f"mse tensor n={n}", R.MSE, *R.loss_operands(R.MSE, n, seed=3 * n))
        lab = torch.tensor([R.f32(c) for c in (1.0, -1.0, 0.0, 0.9)], dtype=F64)[torch.arange(n) % 4]
        yield f"bce tensor n={n}", R.BCE, R.bce_inputs(n, seed=n), lab
    for label in G.BCE_LABELS:
        for n in G.BCE_NS:
            yield f"bce {label} n={n}", R.BCE, R.bce_inputs(n, seed=n + 1), torch.tensor(R.f32(label), dtype=F64)
    for ls in (False, True):
        kind, ps, consts = G.d_case(ls)
        for k in range(4):
            yield f"D ls={ls} [{k}]", kind, ps[k].reshape(-1), torch.tensor(consts[k], dtype=F64)
        preds, targets, kinds = G.g_case(ls)
        for k in range(4):
            t = targets[k].reshape(-1) if torch.is_tensor(targets[k]) else torch.tensor(targets[k], dtype=F64)
            yield f"G ls={ls} [{k}]", kinds[k], preds[k].reshape(-1), t


def grad_cases():
    """Every gradient comparison of the GPU file: the value cases (r = 2; r = 4 inside an objective) and the
    multi-term backward cases."""
    for key, kind, p, t in value_cases():
        yield key, kind, p, t, (4 if key[0] in "DG" else 2)
    kinds, consts, preds, targets = G.multi8_case()
    for k in range(8):
        t = targets[k] if targets[k] is not None else torch.tensor(consts[k], dtype=F64)
        yield f"multi8 [{k}]", kinds[k], preds[k], t, 4
    for n in (900, 2048 * 256 + 1):
        yield f"d_term_grad n={n}", R.MSE, R.loss_operands(R.MSE, n, seed=60 + n % 7, const=1.0)[0], torch.tensor(1.0, dtype=F64), 4


def typical(v, mask=None):
    """Index of an element of median magnitude among the nonzero (and unmasked) ones."""
    a = v.abs().clone()
    if mask is not None:
        a[~mask] = 0
    nz = (a > 0).nonzero().flatten()
    assert len(nz) > 0, "a case without a nonzero element cannot show a missing one"
    order = a[nz].argsort()
    return int(nz[order[len(nz) // 2]])


def bulk_mask(kind, p):
    """For BCE the plant is a Gaussian-bulk element (|x| < 10), not one of the fixed extremes."""
    return (p.abs() < 10) & (p.abs() > 1e-6) if kind == R.BCE else None


def test_value_comparisons_see_one_element():
    n_cases = 0
    for key, kind, p, t in value_cases():
        elem = R.loss_elem(kind, p, t)
        n = p.numel()
        i = typical(elem, bulk_mask(kind, p))
        ref = elem.sum() / n
        tail = elem[(n - 1) // R.LOSS_PER_BLOCK * R.LOSS_PER_BLOCK:].sum()  # the last (partly filled) block
        plants = [("left out", (elem.sum() - elem[i]) / n), ("twice", (elem.sum() + elem[i]) / n)]
        if kind != R.BCE:  # (the last of the fixed BCE inputs, -1e4, has an exactly zero loss against label 0)
            plants += [("last element left out", (elem.sum() - elem[-1]) / n), ("last block left out", (elem.sum() - tail) / n)]
        for what, planted in plants:
            if kind == R.BCE:
                bound = R.bce_mean_bound(p, t)
                G.note(key, torch.zeros(()), bound)
                rejected(G.note, key, (planted - ref).abs(), bound)
            else:
                G.assert_same(ref.to(F32), R.value_f32(kind, p, t), key)
                rejected(G.assert_same, planted.to(F32), R.value_f32(kind, p, t), f"{key} {what}")
        n_cases += 1
    assert n_cases >= 60


def test_objective_combinations_see_a_changed_term():
    for ls in (False,):
        kind, ps, consts = G.d_case(ls)
        v = [R.value_f32(kind, p, c) for p, c in zip(ps, consts)]
        exp = R.combine_d(v, *G.LAMBDAS[1:])
        for k in range(4):
            elem = R.loss_elem(kind, ps[k].reshape(-1), consts[k])
            w = list(v)
            w[k] = ((elem.sum() - elem[typical(elem)]) / elem.numel()).to(F32)
            bad = R.combine_d(w, *G.LAMBDAS[1:])
            rejected(G.assert_same, bad[0], exp[0], "D")
            rejected(G.assert_same, bad[1 + k // 2], exp[1 + k // 2], "D1/D2")
        preds, targets, kinds = G.g_case(ls)
        v = [R.value_f32(k_, p, t) for k_, p, t in zip(kinds, preds, targets)]
        exp = R.combine_g(v, *G.LAMBDAS)
        for k in range(4):
            elem = R.loss_elem(kinds[k], preds[k], targets[k]).reshape(-1)
            w = list(v)
            w[k] = ((elem.sum() - elem[typical(elem)]) / elem.numel()).to(F32)
            rejected(G.assert_same, R.combine_g(w, *G.LAMBDAS), exp, "G")


def test_gradient_comparisons_see_one_wrong_sign():
    n_cases = 0
    for key, kind, p, t, r in grad_cases():
        n = p.numel()
        for gout in G.GOUTS:
            wa, wb = (0.1, 0.5) if r == 4 else (1.0, 1.0)
            scale = R.grad_scale(gout, wa, wb, n)
            ref = R.loss_grad_ref(kind, p, t, scale)
            bound = R.grad_bound(kind, p, t, scale, r)
            G.note(key, torch.zeros_like(ref), bound)
            i = typical(ref, bulk_mask(kind, p))
            for what in ("sign", "left out", "twice"):
                bad = ref.clone()
                bad[i] = {"sign": -ref[i], "left out": 0.0, "twice": 2 * ref[i]}[what]
                rejected(G.note, f"{key} {what}", (bad - ref).abs(), bound)
            if kind != R.BCE:  # the bit-equal form
                g32 = R.grad_scale_f32(gout, wa if r == 4 else None, wb if r == 4 else None, n)
                e32 = g32 * R.loss_dgrad(kind, p, t).to(F32)
                G.note(key + " fp32 formula within the bound", (e32.to(F64) - ref).abs(), bound)
                bad = e32.clone()
                bad[i] = -bad[i]
                rejected(G.assert_same, bad, e32, key)
        n_cases += 1
    assert n_cases >= 70


def test_bce_extreme_gradients_are_exact_in_the_formula():
    """At x = +-1e4 the fp32 formula gives s = 1 / 0 exactly, so the expectation of check_bce_extremes is the
    formula's own value; it stays inside the derived bound of the fp64 reference."""
    n = 1000
    x = R.bce_inputs(n, n + 1)
    for label in G.BCE_LABELS:
        x32 = x.to(F32)
        s = 1.0 / (1.0 + torch.exp(-x32))
        assert bool((s[x == 1e4] == 1).all() and (s[x == -1e4] == 0).all())
        g32 = R.grad_scale_f32(G.GOUTS[1], n=n)
        got = g32 * (s - torch.tensor(label, dtype=F32))
        scale = R.grad_scale(G.GOUTS[1], 1.0, 1.0, n)
        G.note("cpu fp32 bce gradient", (got.to(F64) - R.loss_grad_ref(R.BCE, x, R.f32(label), scale)).abs(),
               R.grad_bound(R.BCE, x, R.f32(label), scale, 2))
        v32 = (x32.clamp_min(0) - x32 * torch.tensor(label, dtype=F32) + torch.log1p(torch.exp(-x32.abs())))
        assert bool(((v32.to(F64) - R.loss_elem(R.BCE, x, R.f32(label))).abs() <= R.bce_elem_bound(x, R.f32(label))).all())
