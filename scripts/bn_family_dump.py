"""Run every entry point of csrc/bn.hip and csrc/inorm.hip, and the csrc/vgg.hip ones that read bf16 vectors, on
seeded inputs with whichever library STC_LIB_PATH names, and save every output buffer whole (the NaN surround of
offset and cropped views included):

  STC_LIB_PATH=old.so python scripts/bn_family_dump.py dump old.npz
  STC_LIB_PATH=new.so python scripts/bn_family_dump.py dump new.npz
  python scripts/bn_family_dump.py --compare old.npz new.npz      # raw bytes; exit 1 on any difference

A refactor of these files has to leave every byte alone.  The shapes are those of tests/test_gpu_bn_family.py,
tests/test_gpu_dropout_family.py, tests/test_gpu_instance_norm.py and tests/test_gpu_vgg_ops.py."""
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "shadow-removal-istd_amd"))

NAN = float("nan")
OUT = {}


def dump(path):
    import torch
    from stcgan_amd import _lib as L
    dev = torch.device("cuda", 0)
    lib = L.lib()
    F32, BF16 = torch.float32, torch.bfloat16
    st = L.stream

    def ok(rc):
        assert rc == 0, lib.stc_last_error().decode()

    def save(name, *tensors):
        torch.cuda.synchronize()
        for i, t in enumerate(tensors):
            assert name + f".{i}" not in OUT, name
            OUT[f"{name}.{i}"] = t.detach().contiguous().view(torch.uint8).cpu().numpy().copy()

    def rnd(shape, seed, scale=1.0, shift=0.0):
        g = torch.Generator().manual_seed(seed)
        return torch.randn(shape, generator=g) * scale + shift

    def dev32(t):
        return t.float().to(dev)

    # layouts: the tensor itself; channels [C, 2C) of a 2C-wide buffer; the top-left H x W of [B, H+1, W+3, C]
    def new_buf(shape, dt, mode):
        B, H, W, C = shape
        full = {"dense": (B, H, W, C), "hi": (B, H, W, 2 * C), "crop": (B, H + 1, W + 3, C)}[mode]
        return torch.full(full, NAN, device=dev, dtype=dt)

    def region(buf, shape, mode):
        B, H, W, C = shape
        return buf if mode == "dense" else buf[..., C:] if mode == "hi" else buf[:, :H, :W, :]

    def view(buf, shape, mode):
        B, H, W, C = shape
        return L.nhwc_view(buf) if mode == "dense" else L.nhwc_view(buf, C) if mode == "hi" else L.nhwc_view(buf, 0, H, W)

    def place(vals, dt, mode):
        buf = new_buf(tuple(vals.shape), dt, mode)
        region(buf, tuple(vals.shape), mode).copy_(vals.to(dt))
        return buf, view(buf, tuple(vals.shape), mode)

    def tables(C, seed):
        g = torch.Generator().manual_seed(seed)
        sc = 0.5 + 0.75 * torch.rand(C, generator=g)
        sc[::3] *= -1.0
        return [dev32(t) for t in (sc, torch.rand(C, generator=g) - 0.5, torch.randn(C, generator=g) * 0.3,
                                   0.5 + torch.rand(C, generator=g), 0.5 + torch.rand(C, generator=g))]

    def tag(dt, shape, *rest):
        return "-".join([("f32" if dt == F32 else "bf16"), "x".join(map(str, shape))] + [str(r) for r in rest])

    # ---- finalize and eval table on synthetic partials {n, S1, S2, shift}
    def partials(nch, C, empty):
        rs = np.random.RandomState(977 * nch + C)
        n = rs.randint(1, 4097, size=(nch, C)).astype(np.float64)
        if empty:
            n[rs.rand(nch, C) < 0.3] = 0.0
            n[0] = np.maximum(n[0], 1.0)
        m, sig = 1.5 + 3.0 * rs.randn(nch, C), 0.5 + 3.0 * rs.rand(nch, C)
        sh = m + sig * rs.uniform(-1.0, 1.0, size=(nch, C))
        S1 = n * (m - sh)
        S2 = np.maximum(n - 1.0, 0.0) * sig ** 2 + S1 * S1 / np.maximum(n, 1.0)
        return (np.stack([n, S1, S2, sh], axis=-1) * (n > 0)[..., None]).astype(np.float32)

    C = 5
    for nch, empty in [(k, False) for k in (1, 65, 256, 257, 512, 513, 1024, 1025, 2049, 4097, 9001)] + [(513, True), (2049, True)]:
        part = torch.from_numpy(partials(nch, C, empty)).to(dev)
        gam, bet, rm, rv = (dev32(rnd((C,), 5 + i, 0.3, 1.0)) for i in range(4))
        rv = rv.abs()
        nbt = torch.zeros(1, dtype=torch.long, device=dev)
        o = torch.full((4, C), NAN, device=dev)
        ok(lib.stc_bn_finalize(L.ptr(part), nch, C, L.ptr(gam), L.ptr(bet), L.ptr(rm), L.ptr(rv), L.ptr(nbt), 0.1, 1e-5,
                               L.ptr(o[0]), L.ptr(o[1]), L.ptr(o[2]), L.ptr(o[3]), st()))
        save(f"finalize-nch{nch}-{'empty' if empty else 'full'}", o, rm, rv, nbt)
    for C in (1, 5, 257):
        gam, bet, rm, rv = (dev32(rnd((C,), 15 + i, 0.3, 1.0)) for i in range(4))
        o = torch.full((2, C), NAN, device=dev)
        ok(lib.stc_bn_finalize(None, 0, C, L.ptr(gam), L.ptr(bet), L.ptr(rm), L.ptr(rv.abs()), None, 0.1, 1e-5, None, None,
                               L.ptr(o[0]), L.ptr(o[1]), st()))
        save(f"eval_table-C{C}", o)

    # ---- backward finalize through stc_bn_bwd_apply, synthetic part2
    for nch in (1, 256, 257, 1025):
        shape, C = (1, 5, 13, 20), 20
        x = rnd(shape, 31)
        g1 = rnd(shape, 32)
        _, xv = place(x, F32, "dense")
        _, gv = place(g1, F32, "dense")
        sc, sh, mu, rs, gm = tables(C, 33)
        part2 = dev32(rnd((nch, C, 2), 34 + nch))
        dx = new_buf(shape, F32, "dense")
        dgb = torch.full((2, C), NAN, device=dev)
        ok(lib.stc_bn_bwd_apply(L.F32, 1, xv, C, L.ptr(sc), L.ptr(sh), L.ptr(mu), L.ptr(rs), L.ptr(gm), gv, 0.2, L.NULL_VIEW,
                                0.0, L.ptr(part2), nch, L.nhwc_view(dx), L.ptr(dgb[0]), L.ptr(dgb[1]), st()))
        save(f"bwd_finalize-nch{nch}", dgb, dx)

    # ---- chan_stats, chan_sum, bn_bwd_reduce: CG = 1, 2, 3, 24, 256, an empty tail chunk
    RED = [(F32, (1, 5, 13, 8)), (F32, (1, 8, 8, 96)), (F32, (1, 5, 13, 1024)), (F32, (1, 1, 65537, 4)),
           (BF16, (1, 5, 13, 24)), (BF16, (1, 5, 13, 2048)), (BF16, (3, 15, 20, 128))]
    for dt, shape in RED:
        B, H, W, C = shape
        code = L.dtype_code(dt)
        nch = lib.stc_chan_stats_chunks(B, H, W)
        x, g1, g2 = rnd(shape, 41, 3.0, 1.5), rnd(shape, 42), rnd(shape, 43)
        sc, sh, mu, rs, gm = tables(C, 44)
        for mode in ("dense", "hi", "crop"):
            _, xv = place(x, dt, mode)
            part = torch.full((nch, C, 4), NAN, device=dev)
            ok(lib.stc_chan_stats(code, B, xv, C, L.ptr(part), nch, st()))
            save("chan_stats-" + tag(dt, shape, mode), part)
            part1 = torch.full((nch, C), NAN, device=dev)
            out = torch.full((C,), NAN, device=dev)
            ok(lib.stc_chan_sum(code, B, xv, C, C - 1, L.ptr(part1), nch, L.ptr(out), st()))
            save("chan_sum-" + tag(dt, shape, mode), part1, out)
            _, g1v = place(g1, dt, "hi" if mode == "dense" else "dense")
            _, g2v = place(g2, dt, mode)
            for has1, has2 in ((True, True), (True, False), (False, True)):
                part2 = torch.full((nch, C, 2), NAN, device=dev)
                ok(lib.stc_bn_bwd_reduce(code, B, xv, C, L.ptr(sc), L.ptr(sh), L.ptr(mu), L.ptr(rs),
                                         g1v if has1 else L.NULL_VIEW, 0.0, g2v if has2 else L.NULL_VIEW, 0.2,
                                         L.ptr(part2), nch, st()))
                save("bwd_reduce-" + tag(dt, shape, mode, int(has1), int(has2)), part2)

    # ---- bn_apply / bn_bwd_apply: DENSE and general form, one and two outputs / gradients, with and without tables
    APPLY = [(F32, (2, 1, 1, 4)), (F32, (1, 5, 13, 8)), (F32, (1, 1, 63, 96)), (F32, (1, 8, 8, 96)), (F32, (1, 5, 13, 1024)),
             (F32, (3, 15, 20, 128)), (F32, (1, 257, 255, 4)), (F32, (1, 1, 65537, 4)), (F32, (1, 1, 70000, 128)),
             (BF16, (2, 1, 1, 8)), (BF16, (1, 5, 13, 24)), (BF16, (1, 1, 65, 64)), (BF16, (1, 5, 13, 2048)),
             (BF16, (3, 15, 20, 128)), (BF16, (1, 257, 255, 8)), (BF16, (1, 1, 65537, 8))]
    MIXES = {"dense": ("dense", "dense", "dense"), "cat": ("dense", "hi", "dense"), "crop": ("crop", "crop", "dense")}
    for dt, shape in APPLY:
        B, H, W, C = shape
        code = L.dtype_code(dt)
        x, g1, g2 = rnd(shape, 51, 2.0), rnd(shape, 52), rnd(shape, 53)
        sc, sh, mu, rs, gm = tables(C, 54)
        nch = lib.stc_chan_stats_chunks(B, H, W)
        part2 = dev32(rnd((nch, C, 2), 55))
        big = shape == (1, 1, 70000, 128)  # past both grid caps: one configuration per form
        for mix, (mx, m1, m2) in MIXES.items():
            if big and mix == "cat":
                continue
            _, xv = place(x, dt, mx)
            for table in ((True,) if big else (True, False)):
                for s1, s2 in (((0.2, 0.0),) if big else ((0.2, 0.0), (0.0, None), (1.0, None))):
                    y1 = new_buf(shape, dt, m1)
                    y2 = new_buf(shape, dt, m2)
                    ok(lib.stc_bn_apply(code, B, xv, C, L.ptr(sc) if table else None, L.ptr(sh) if table else None,
                                        view(y1, shape, m1), s1, view(y2, shape, m2) if s2 is not None else L.NULL_VIEW,
                                        s2 if s2 is not None else 1.0, st()))
                    save("apply-" + tag(dt, shape, mix, int(table), s1, s2), y1, y2)
            _, g1v = place(g1, dt, m1)
            _, g2v = place(g2, dt, m2)
            for has1, has2, s1, s2 in ((True, True, 0.0, 0.2), (True, False, 0.2, 0.0), (False, True, 1.0, 0.2))[:1 if big else 3]:
                a, b = (g1v if has1 else L.NULL_VIEW), (g2v if has2 else L.NULL_VIEW)
                dx = new_buf(shape, dt, m1)
                dgb = torch.full((2, C), NAN, device=dev)
                ok(lib.stc_bn_bwd_apply(code, B, xv, C, L.ptr(sc), L.ptr(sh), L.ptr(mu), L.ptr(rs), L.ptr(gm), a, s1, b, s2,
                                        L.ptr(part2), nch, view(dx, shape, m1), L.ptr(dgb[0]), L.ptr(dgb[1]), st()))
                save("bwd_apply-" + tag(dt, shape, mix, int(has1), int(has2)), dx, dgb)
                for table in (True, False):  # activation only (mean == nullptr), with and without the affine
                    dx = new_buf(shape, dt, m1)
                    ok(lib.stc_bn_bwd_apply(code, B, xv, C, L.ptr(sc) if table else None, L.ptr(sh) if table else None, None,
                                            None, None, a, s1, b, s2, None, 0, view(dx, shape, m1), None, None, st()))
                    save("act_bwd-" + tag(dt, shape, mix, int(has1), int(has2), int(table)), dx)

    # ---- dropout: the mask and the three _drop entry points (full extent B x H x W, views cropped or not)
    state = torch.tensor([0x1234567887654321, 7], dtype=torch.long, device=dev)  # {seed, offset}
    for shape, level in (((1, 1, 1, 4), 0), ((3, 4, 6, 64), 7), ((3, 4, 6, 64), 2 ** 31 - 1)):
        B, H, W, C = shape
        for p in (0.0, 0.5):
            d = L.Dropout(state.data_ptr(), p, level, H, W, 0)
            m = torch.full(shape, 255, dtype=torch.uint8, device=dev)
            ok(lib.stc_dropout_mask(ctypes.byref(d), B, C, L.ptr(m), st()))
            save(f"mask-{'x'.join(map(str, shape))}-{level}-{p}", m)
    for dt in (F32, BF16):
        code, N = L.dtype_code(dt), (4 if dt == F32 else 8)
        for cv, crop in ((1, (0, 0)), (3, (1, 2)), (24, (0, 3)), (64, (1, 0)), (256, (1, 2))):
            B, Hf, Wf, C = 3, 5, 7, cv * N
            H, W = Hf - crop[0], Wf - crop[1]
            shape, full = (B, H, W, C), (B, Hf, Wf, C)
            x, g1, g2 = rnd(full, 61, 2.0), rnd(full, 62), rnd(full, 63)
            sc, sh, mu, rs, gm = tables(C, 64)
            nch = lib.stc_chan_stats_chunks(B, H, W)

            def fullview(t):
                buf = t.to(dt).to(dev)
                return buf, L.nhwc_view(buf, 0, H, W)

            _, xv = fullview(x)
            _, g1v = fullview(g1)
            _, g2v = fullview(g2)
            for p in (0.0, 0.5):
                d = L.Dropout(state.data_ptr(), p, 3, Hf, Wf, 0)
                for table in (True, False):
                    y1 = torch.full((B, Hf, Wf, 2 * C), NAN, device=dev, dtype=dt)
                    y2 = torch.full(full, NAN, device=dev, dtype=dt)
                    ok(lib.stc_bn_apply_drop(code, B, xv, C, L.ptr(sc) if table else None, L.ptr(sh) if table else None,
                                             L.nhwc_view(y1, C, H, W), 0.2, L.nhwc_view(y2, 0, H, W), 0.0,
                                             ctypes.byref(d), st()))
                    save("apply_drop-" + tag(dt, shape, p, int(table)), y1, y2)
                for has2 in (True, False):
                    b = g2v if has2 else L.NULL_VIEW
                    part2 = torch.full((nch, C, 2), NAN, device=dev)
                    ok(lib.stc_bn_bwd_reduce_drop(code, B, xv, C, L.ptr(sc), L.ptr(sh), L.ptr(mu), L.ptr(rs), g1v, 0.0, b, 0.2,
                                                  ctypes.byref(d), L.ptr(part2), nch, st()))
                    dx = torch.full(full, NAN, device=dev, dtype=dt)
                    dgb = torch.full((2, C), NAN, device=dev)
                    ok(lib.stc_bn_bwd_apply_drop(code, B, xv, C, L.ptr(sc), L.ptr(sh), L.ptr(mu), L.ptr(rs), L.ptr(gm), g1v,
                                                 0.0, b, 0.2, ctypes.byref(d), L.ptr(part2), nch, L.nhwc_view(dx, 0, H, W),
                                                 L.ptr(dgb[0]), L.ptr(dgb[1]), st()))
                    save("bwd_drop-" + tag(dt, shape, p, int(has2)), part2, dx, dgb)

    # ---- InstanceNorm: one shape per regime (tiny, one launch, two launches), affine and plain
    for dt in (F32, BF16):
        code, N = L.dtype_code(dt), (4 if dt == F32 else 8)
        for B, H, W, cv in ((3, 2, 2, 64), (3, 31, 31, 3), (3, 8, 8, 64), (1, 64, 64, 3), (1, 64, 64, 64)):
            C = cv * N
            shape = (B, H, W, C)
            plan = (ctypes.c_int32 * 4)()
            ok(lib.stc_in_plan(code, B, H, W, C, plan))
            nbytes = int(lib.stc_in_workspace(code, B, H, W, C))
            x, g1, g2 = rnd(shape, 71, 2.0, 0.5), rnd(shape, 72), rnd(shape, 73)
            gam, bet = dev32(rnd((C,), 74, 0.3, 1.0)), dev32(rnd((C,), 75, 0.3))
            for mode in ("dense", "crop"):
                _, xv = place(x, dt, mode)
                _, g1v = place(g1, dt, mode)
                _, g2v = place(g2, dt, "dense")
                for affine in (True, False):
                    ws = torch.full((max(nbytes, 16),), 0xAB, dtype=torch.uint8, device=dev)
                    ms = torch.full((2, B, C), NAN, device=dev)
                    y1, y2 = new_buf(shape, dt, mode), new_buf(shape, dt, "hi")
                    ok(lib.stc_in_fwd(code, B, xv, C, L.ptr(gam) if affine else None, L.ptr(bet) if affine else None, 1e-5,
                                      L.ptr(ms[0]), L.ptr(ms[1]), xv, view(y1, shape, mode), 0.2,
                                      view(y2, shape, "hi") if affine else L.NULL_VIEW, 0.0, L.ptr(ws), nbytes, st()))
                    save("in_fwd-" + tag(dt, shape, mode, int(affine), f"regime{plan[0]}"), ms, y1, y2)
                    dx = new_buf(shape, dt, mode)
                    dgb = torch.full((2, C), NAN, device=dev)
                    ok(lib.stc_in_bwd(code, B, xv, C, L.ptr(gam) if affine else None, L.ptr(bet) if affine else None,
                                      L.ptr(ms[0]), L.ptr(ms[1]), g1v, 0.0, g2v if affine else L.NULL_VIEW, 0.2,
                                      view(dx, shape, mode), L.ptr(dgb[0]) if affine else None,
                                      L.ptr(dgb[1]) if affine else None, L.ptr(ws), nbytes, st()))
                    save("in_bwd-" + tag(dt, shape, mode, int(affine), f"regime{plan[0]}"), dx, dgb)

    # ---- vgg.hip: the kernels that unpack bf16 vectors
    B, H, W, C = 2, 6, 10, 24
    x = rnd((B, H, W, C), 81).to(BF16).to(dev)
    y = torch.full((B, H // 2, W // 2, C), NAN, dtype=BF16, device=dev)
    ok(lib.stc_maxpool2_fwd(B, L.nhwc_view(x), C, L.nhwc_view(y), st()))
    gy = rnd((B, H // 2, W // 2, C), 82).to(BF16).to(dev)
    gx = torch.full((B, H, W, C), NAN, dtype=BF16, device=dev)
    ok(lib.stc_maxpool2_bwd(B, L.nhwc_view(x), C, L.nhwc_view(gy), L.nhwc_view(gx), st()))
    save("maxpool2", y, gx)
    g8 = rnd((B, H, W, 8), 83).to(BF16).to(dev)
    dst = torch.full((B, 3, H, W), NAN, device=dev)
    ok(lib.stc_vgg_norm_bwd(B, H, W, L.nhwc_view(g8), L.ptr(dst), st()))
    save("vgg_norm_bwd", dst)
    n = 2 * 13 * 17 * 64
    fp, ft = rnd((n,), 84).to(BF16).to(dev), rnd((n,), 85).to(BF16).to(dev)
    part = torch.full((lib.stc_feat_mse_parts(n),), NAN, device=dev)
    out = torch.full((1,), NAN, device=dev)
    ok(lib.stc_feat_mse_fwd(L.ptr(fp), L.ptr(ft), n, L.ptr(part), L.ptr(out), st()))
    gout = torch.tensor([0.37], device=dev)
    for relu in (0, 1):
        g = torch.full((n,), NAN, dtype=BF16, device=dev)
        ok(lib.stc_feat_mse_bwd(L.ptr(fp), L.ptr(ft), n, L.ptr(gout), relu, L.ptr(g), st()))
        save(f"feat_mse_bwd-{relu}", g)
    save("feat_mse_fwd", part, out)

    np.savez(path, **OUT)
    print(f"{len(OUT)} buffers, {sum(v.nbytes for v in OUT.values())} bytes, library {L.LIB_PATH}")


def compare(a, b):
    A, Bz = np.load(a), np.load(b)
    assert sorted(A.files) == sorted(Bz.files), "the two dumps hold different buffers"
    bad = nbytes = 0
    for k in A.files:
        same = A[k].shape == Bz[k].shape and A[k].tobytes() == Bz[k].tobytes()
        nbytes += A[k].nbytes
        if not same:
            bad += 1
            ndiff = int((A[k] != Bz[k]).sum()) if A[k].shape == Bz[k].shape else -1
            print(f"{k}: DIFFERENT ({ndiff} of {A[k].nbytes} bytes)")
    print(f"{len(A.files)} buffers, {nbytes} bytes compared: {bad} buffers differ")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    if sys.argv[1] == "--compare":
        compare(sys.argv[2], sys.argv[3])
    else:
        dump(sys.argv[2] if sys.argv[1] == "dump" else sys.argv[1])
