"""The resize-convolution weight kernels of csrc/eltwise.hip against exact references: stc_upconv_expand and
stc_upconv_wgrad_collapse bit for bit against the numpy restatement of the documented summation order
(tests/upconv_ref.py), and the pack modes STC_PACK_UPCONV_FWD / _DGRAD byte for byte against edge_loss_ref's pack of
the expanded weight in the modes STC_PACK_CONVT_FWD / _DGRAD (pad rows and columns zero, the memory around the output
untouched), through stc_pack_weight and through stc_pack_weights alone and mixed with the 4x4 modes.

Gaussian weights, so every sum and every bf16 cast really rounds.  Shapes (Ci, Co): ragged 16 x 16 tiles on either
side, several tiles, one output channel, and the outermost layers' 1 and 3."""
import pytest
import torch

import edge_loss_ref as R
import upconv_ref as U
from stcgan_amd import _lib as L
from stcgan_amd import ops
from test_gpu_edge_loss_family import arena, assert_same, guards_intact, pack_case, pack_pads

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF, F32 = torch.bfloat16, torch.float32
SHAPES = [(3, 5), (8, 8), (17, 33), (64, 4), (16, 1), (16, 3)]  # (Ci, Co)
CONVT_OF = {L.PACK_UPCONV_FWD: R.PACK_CONVT_FWD, L.PACK_UPCONV_DGRAD: R.PACK_CONVT_DGRAD}


def dn(dt):
    return "f32" if dt == F32 else "bf16"


def w3_of(Ci, Co, seed=0):
    return torch.randn(Co, Ci, 3, 3, generator=torch.Generator().manual_seed(700 + seed), dtype=F32)


def offset_by_one(t):
    flat = torch.full((t.numel() + 2,), float("nan"), dtype=t.dtype, device=DEV)
    v = flat[1:1 + t.numel()].view(t.shape)
    assert v.data_ptr() % 16 == 4
    return flat, v


@pytest.mark.parametrize("Ci,Co", SHAPES, ids=lambda v: str(v))
def test_expand(Ci, Co):
    w3 = w3_of(Ci, Co)
    exp = torch.from_numpy(U.expand(w3.numpy()))
    buf, out = arena(exp.shape, F32)
    wd = w3.to(DEV)
    L.check(L.lib().stc_upconv_expand(L.ptr(wd), Ci, Co, L.ptr(out), L.stream()), "stc_upconv_expand")
    torch.cuda.synchronize()
    assert_same(out, exp, f"expand {Ci}x{Co}")
    guards_intact(buf, f"expand {Ci}x{Co}")
    assert_same(ops.upconv_expand(wd), exp, f"ops.upconv_expand {Ci}x{Co}")
    # an output that is only 4-byte aligned (the scalar-store path)
    flat, v = offset_by_one(exp)
    L.check(L.lib().stc_upconv_expand(L.ptr(wd), Ci, Co, L.ptr(v), L.stream()), "stc_upconv_expand")
    torch.cuda.synchronize()
    assert_same(v, exp, f"expand {Ci}x{Co} at +4 bytes")
    assert bool(torch.isnan(flat[0])) and bool(torch.isnan(flat[-1]))


@pytest.mark.parametrize("Ci,Co", SHAPES, ids=lambda v: str(v))
def test_wgrad_collapse(Ci, Co):
    g4 = torch.randn(Ci, Co, 4, 4, generator=torch.Generator().manual_seed(800 + Ci), dtype=F32)
    exp = torch.from_numpy(U.collapse(g4.numpy()))
    gd = g4.to(DEV)
    buf, out = arena(exp.shape, F32)
    L.check(L.lib().stc_upconv_wgrad_collapse(L.ptr(gd), Ci, Co, L.ptr(out), L.stream()), "stc_upconv_wgrad_collapse")
    torch.cuda.synchronize()
    assert_same(out, exp, f"collapse {Ci}x{Co}")
    guards_intact(buf, f"collapse {Ci}x{Co}")
    # a slice of a flat buffer at a 4-byte aligned offset, and a 4-byte aligned source
    flat, v = offset_by_one(exp)
    sflat, sv = offset_by_one(g4)
    sv.copy_(gd)
    assert_same(ops.upconv_wgrad_collapse(sv, v), exp, f"collapse {Ci}x{Co} at +4 bytes")
    torch.cuda.synchronize()
    assert bool(torch.isnan(flat[0])) and bool(torch.isnan(flat[-1]))


def upconv_case(mode, Ci, Co, wide, dt, seed=0):
    """(w3 fp32, the expected operand: edge_loss_ref's pack of the expanded weight in the ConvT mode, N_pad, C_pad)."""
    w3 = w3_of(Ci, Co, seed)
    W4 = torch.from_numpy(U.expand(w3.numpy()))
    n_pad, c_pad = pack_pads(CONVT_OF[mode], Ci, Co, wide)
    return w3, R.pack_ref(CONVT_OF[mode], W4, n_pad, c_pad).to(dt), n_pad, c_pad


@pytest.mark.parametrize("dt", [F32, BF], ids=dn)
@pytest.mark.parametrize("wide", [False, True], ids=["pad16x8", "pad64x32"])
@pytest.mark.parametrize("Ci,Co", SHAPES, ids=lambda v: str(v))
@pytest.mark.parametrize("mode", [L.PACK_UPCONV_FWD, L.PACK_UPCONV_DGRAD])
def test_pack_weight(mode, Ci, Co, wide, dt):
    w3, exp, n_pad, c_pad = upconv_case(mode, Ci, Co, wide, dt)
    buf, out = arena(exp.shape, dt)
    wd = w3.to(DEV)
    L.check(L.lib().stc_pack_weight(L.dtype_code(dt), mode, L.ptr(wd), Ci, Co, L.ptr(out), n_pad, c_pad, L.stream()),
            "stc_pack_weight")
    torch.cuda.synchronize()
    what = f"pack mode {mode} {Ci}x{Co} -> {n_pad}x{c_pad} {dn(dt)}"
    assert_same(out, exp, what)  # (pad rows and columns of exp are zeros)
    guards_intact(buf, what)
    if not wide:  # the wrapper the engine uses; and the same bytes as the ConvT mode gives from the HIP expansion
        assert_same(ops.pack(mode, wd, n_pad, c_pad, dt), exp, what + " (ops.pack)")
        assert_same(ops.pack(CONVT_OF[mode], ops.upconv_expand(wd), n_pad, c_pad, dt), exp, what + " (ConvT mode)")


def run_multi(jobs, dt, what):
    """jobs: [(mode, P, Q, wide)] as one stc_pack_weights call; modes 0-4 take edge_loss_ref's integer weights."""
    cases = []
    for i, (m, P, Q, wide) in enumerate(jobs):
        cases.append(upconv_case(m, P, Q, wide, dt, seed=i) if m in CONVT_OF else pack_case(m, P, Q, wide, dt, seed=i))
    Ws = [c[0].to(DEV) for c in cases]
    outs = [arena(c[1].shape, dt) for c in cases]
    descs = (L.PackDesc * len(jobs))(*[L.PackDesc(j[0], j[1], j[2], c[2], c[3], 0, w.data_ptr(), o[1].data_ptr())
                                       for j, c, w, o in zip(jobs, cases, Ws, outs)])
    L.check(L.lib().stc_pack_weights(L.dtype_code(dt), len(jobs), descs, L.stream()), "stc_pack_weights")
    torch.cuda.synchronize()
    for i, (c, (buf, out)) in enumerate(zip(cases, outs)):
        assert_same(out, c[1], f"{what} descriptor {i} {jobs[i]}")
        guards_intact(buf, f"{what} descriptor {i}")


@pytest.mark.parametrize("dt", [F32, BF], ids=dn)
def test_pack_weights_upconv_only(dt):
    """Every shape in both modes, alternating paddings: the launch the generator's refresh makes."""
    jobs = [(5 + (i % 2), *SHAPES[i // 2], bool(i % 3 == 1)) for i in range(2 * len(SHAPES))]
    run_multi(jobs, dt, f"pack_weights upconv {dn(dt)}")
    run_multi(jobs[3:4], dt, f"pack_weights upconv n=1 {dn(dt)}")


@pytest.mark.parametrize("dt", [F32, BF], ids=dn)
def test_pack_weights_mixed_modes(dt):
    """Old and new modes interleaved in one call, up to STC_PACK_MAX descriptors."""
    jobs = [(i % 7, *SHAPES[(i // 7 + i) % len(SHAPES)], bool(i % 3 == 1)) for i in range(L.PACK_MAX)]
    assert {j[0] for j in jobs} == set(range(7))
    run_multi(jobs, dt, f"pack_weights mixed {dn(dt)}")


@pytest.mark.parametrize("dt", [F32, BF], ids=dn)
def test_pack_weights_strided(dt):
    """A descriptor with more tiles (33 x 32 = 1056) than its 1024-block share between two small ones: the first
    blocks stride over the tiles."""
    jobs = [(5, 3, 5, False), (6, 528, 512, False), (5, 17, 33, False)]
    assert -(-pack_pads(4, 528, 512, False)[0] // 16) * -(-pack_pads(4, 528, 512, False)[1] // 16) > 1024
    run_multi(jobs, dt, f"pack_weights strided {dn(dt)}")
