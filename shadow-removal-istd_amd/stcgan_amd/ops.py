"""Thin tensor-level wrappers over the C-ABI (include/stcgan_hip.h).

Every function here enqueues HIP kernels of libstcgan_hip.so on torch's current
stream; torch is used only for device memory (caching allocator) and streams.
"""
import ctypes

import torch

from . import _lib as L
from ._lib import check, lib, ptr, stream

LRELU = 0.2
BN_EPS = 1e-5
BN_MOMENTUM = 0.1


def vec(dt):
    """Elements per 16-byte chunk for the activation dtype."""
    return 4 if dt == torch.float32 else 8


def pad_channels(c, dt):
    """Smallest power of two >= max(c, vec(dt))."""
    p = vec(dt)
    while p < c:
        p *= 2
    return p


def _ws(nbytes, device):
    if nbytes <= 0:
        return None, 0
    return torch.empty(int(nbytes), dtype=torch.uint8, device=device), int(nbytes)


def _pro(pro):
    if pro is None:
        return None, None
    sc, sh = pro
    return ptr(sc), ptr(sh)


# Instrumentation (bench.py / scripts): when a list, conv()/conv_stats()/conv_bn_backward()/wgrad() append
# (kernel, single-kernel call, flops, start event, end event, description); the events bracket the call's
# MAIN kernel only (stc_time_next_main_kernel), not a split-K / split-pixel reduction it enqueues after it.
_timer = None
# when a list: wgrad() also appends (kernel, start, end) events around the WHOLE call (main kernel + its
# split-pixel reduction), so that the roofline can charge the reduction to the kernel
_call_timer = None


def _main_events():
    """A pair of timing events armed to bracket the next main kernel this thread launches."""
    e0 = torch.cuda.Event(enable_timing=True)
    e1 = torch.cuda.Event(enable_timing=True)
    e0.record()  # creates the events; the library records them again around the kernel
    e1.record()
    check(lib().stc_time_next_main_kernel(ctypes.c_void_p(e0.cuda_event), ctypes.c_void_p(e1.cuda_event)),
          "stc_time_next_main_kernel")
    return e0, e1


def _disarm():
    lib().stc_time_next_main_kernel(None, None)


# Plan / workspace answers of the library are pure functions of their arguments (no environment, no device
# state), and the step asks the same few dozen questions every iteration: memoised, ~5 us of host time per call.
_MEMO = {}


def _conv_ws_bytes(kind, B, gh, gw, cin, cout, dt):
    key = ("cws", kind, B, gh, gw, cin, cout, dt)
    v = _MEMO.get(key)
    if v is None:
        v = _MEMO[key] = lib().stc_conv_fwd_workspace(L.dtype_code(dt), kind, B, gh, gw, cin, cout)
    return v


def set_splitk_inlaunch(on):
    """Split-K combined inside the GEMM launch (True, the default) or by a separate reduction launch (False; A/B):
    stc_set_splitk_inlaunch.  The workspace sizes and statistics chunk counts follow it, so the memoised queries
    are dropped.  Returns the previous setting."""
    old = bool(lib().stc_set_splitk_inlaunch(1 if on else 0))
    _MEMO.clear()
    return old


def plan_of(kind, B, gh, gw, cin, cout, dt):
    out = (ctypes.c_int32 * 4)()
    check(lib().stc_conv_fwd_plan(L.dtype_code(dt), kind, B, gh, gw, cin, cout, out), "stc_conv_fwd_plan")
    return tuple(out)


_DGRAD_OF = {L.CONVT_S2: L.CONV_S2, L.CONV_S1_DGRAD: L.CONV_S1}  # the Conv2d kind an input-gradient kind belongs to


def conv_pad_query(kind, B, H, W, cin, cout, dt, pad, out_f32=False, force=None):
    """(workspace bytes, stats chunks, plan) of stc_conv_pad_fwd for a Conv2d kind over an H x W input."""
    key = ("cpq", kind, B, H, W, cin, cout, dt, pad, bool(out_f32), None if force is None else tuple(force))
    r = _MEMO.get(key)
    if r is None:
        ws, nch, po = ctypes.c_int64(), ctypes.c_int32(), (ctypes.c_int32 * 5)()
        fp = (ctypes.c_int32 * 2)(*force) if force is not None else None
        check(lib().stc_conv_pad_fwd_query(L.dtype_code(dt), kind, pad, B, H, W, cin, cout, int(out_f32), fp,
                                           ctypes.byref(ws), ctypes.byref(nch), po), "stc_conv_pad_fwd_query")
        r = _MEMO[key] = (ws.value, nch.value, tuple(po))
    return r


def conv_pad_dgrad_query(kind, B, H, W, cout, cin, dt, pad, out_f32=False):
    """(workspace bytes, plan) of stc_conv_pad_dgrad: the input gradient (cin channels, H x W) of a Conv2d kind; under
    reflect the plan is the frame conv's and the workspace holds the fp32 frame and its split-K slabs."""
    key = ("cpdq", kind, B, H, W, cout, cin, dt, pad, bool(out_f32))
    r = _MEMO.get(key)
    if r is None:
        ws, po = ctypes.c_int64(), (ctypes.c_int32 * 5)()
        check(lib().stc_conv_pad_dgrad_query(L.dtype_code(dt), kind, pad, B, H, W, cout, cin, int(out_f32),
                                             ctypes.byref(ws), po), "stc_conv_pad_dgrad_query")
        r = _MEMO[key] = (ws.value, tuple(po))
    return r


def conv_pad(kind, B, xv, cin, w_packed, cout, yv, dt, pad, bias=None, act=None, out_f32=False, stats=False):
    """A Conv2d k4 p1 with a padding mode, ``kind`` as conv() takes it: a Conv2d kind is the forward
    (stc_conv_pad_fwd), STC_CONVT_S2 / STC_CONV_S1_DGRAD the input gradient of the stride-2 / stride-1 conv
    (stc_conv_pad_dgrad: xv the output gradient, yv the input gradient).  stats (forward): returns the BatchNorm
    partials (part, chunks) of the stored output.  DESIGN.md section 8i."""
    dev = w_packed.device
    code = L.dtype_code(dt)
    if kind in _DGRAD_OF:
        assert bias is None and act is None and not stats
        nbytes, _ = conv_pad_dgrad_query(_DGRAD_OF[kind], B, yv.H, yv.W, cin, cout, dt, pad, out_f32)
        ws, nb = _ws(nbytes, dev)
        check(lib().stc_conv_pad_dgrad(code, _DGRAD_OF[kind], pad, B, xv, cin, ptr(w_packed), cout, yv, int(out_f32),
                                       ptr(ws), nb, stream()), "stc_conv_pad_dgrad")
        return None
    nbytes, nch, _ = conv_pad_query(kind, B, xv.H, xv.W, cin, cout, dt, pad, out_f32)
    ws, nb = _ws(nbytes, dev)
    part = torch.empty((nch, cout, 4), dtype=torch.float32, device=dev) if stats else None
    check(lib().stc_conv_pad_fwd(code, kind, pad, B, xv, cin, ptr(w_packed), cout, yv, ptr(bias), L.head_code(act),
                                 int(out_f32), ptr(part), nch if stats else 0, None, ptr(ws), nb, stream()),
          "stc_conv_pad_fwd")
    return (part, nch) if stats else None


def conv(kind, B, xv, cin, w_packed, cout, yv, dt, pro=None, slope=None, bias=None, tanh=False, out_f32=False,
         force=None, act=None, pad=L.PAD_ZEROS):
    """Implicit-GEMM conv family (stc_conv_fwd; force: a forced narrow-N tile through stc_conv_fwd_ex, tests).
    act: the output head of the epilogue (_lib.head_code); tanh=True means act="tanh".
    pad: L.PAD_REFLECT runs conv_pad (no prologue, no forced plan); L.PAD_ZEROS is this function as ever."""
    if act is not None and tanh and L.head_code(act) != L.HEAD_TANH:
        raise ValueError(f"stcgan_amd: conv(tanh=True) together with act={act!r}")
    if pad != L.PAD_ZEROS:
        if pro is not None or slope is not None or force is not None:
            raise ValueError("stcgan_amd: a reflect conv takes no prologue and no forced plan")
        return conv_pad(kind, B, xv, cin, w_packed, cout, yv, dt, pad, bias=bias,
                        act=act if act is not None else ("tanh" if tanh else None), out_f32=out_f32)
    tanh = L.head_code(act) if act is not None else int(bool(tanh))
    dev = w_packed.device
    if kind == L.CONVT_S2:
        gh, gw = xv.H, xv.W
    else:
        gh, gw = yv.H, yv.W
    l = lib()
    nbytes = _conv_ws_bytes(kind, B, gh, gw, cin, cout, dt)
    ws, nb = _ws(nbytes, dev)
    sc, sh = _pro(pro)
    timer = _timer
    if timer is not None:
        e0, e1 = _main_events()
    if force is not None:
        assert pro is None and slope is None
        rc = l.stc_conv_fwd_ex(L.dtype_code(dt), kind, B, xv, cin, ptr(w_packed), cout, yv, ptr(bias), tanh,
                               int(out_f32), None, 0, (ctypes.c_int32 * 2)(*force), ptr(ws), nb, stream())
    else:
        rc = l.stc_conv_fwd(L.dtype_code(dt), kind, B, xv, cin, sc, sh, 0 if slope is None else 1,
                            0.0 if slope is None else float(slope), ptr(w_packed), cout, yv, ptr(bias), tanh,
                            int(out_f32), ptr(ws), nb, stream())
    if timer is not None:
        _disarm()
    check(rc, "stc_conv_fwd")
    if timer is not None:
        _time_entry(timer, kind, B, gh, gw, cin, cout, dt, e0, e1)


def conv_query(kind, B, gh, gw, cin, cout, dt, out_f32=False, force=None):
    """(workspace bytes, stats chunks, plan (BM, BN, ksplit, narrow, cfg)) of stc_conv_fwd_ex."""
    key = ("cq", kind, B, gh, gw, cin, cout, dt, bool(out_f32), None if force is None else tuple(force))
    r = _MEMO.get(key)
    if r is not None:
        return r
    ws = ctypes.c_int64()
    nch = ctypes.c_int32()
    po = (ctypes.c_int32 * 5)()
    fp = (ctypes.c_int32 * 2)(*force) if force is not None else None
    check(lib().stc_conv_fwd_query(L.dtype_code(dt), kind, B, gh, gw, cin, cout, int(out_f32), fp, ctypes.byref(ws),
                                   ctypes.byref(nch), po), "stc_conv_fwd_query")
    r = _MEMO[key] = (ws.value, nch.value, tuple(po))
    return r


# Tuning hooks (scripts/train_steps.py --ab-plans): per-shape plan overrides of the forward convs with
# fused statistics, keyed (kind, B, gh, gw, cin, cout), and of the weight gradients, keyed
# (B, Hd, Wd, R, Cg); values {tile config, splits}.  Empty in production.
FORCE_CONV = {}
FORCE_WGRAD = {}


# conv + activation epilogue for the layers without BatchNorm (stc_conv_fwd_act); False (A/B scripts): conv +
# bn_apply
FUSE_ACT = True
# input-gradient conv + activation backward for the same layers (stc_conv_bwd_act); False (A/B, tests): conv +
# bn_backward(no table)
FUSE_ACT_BWD = True


def conv_act(kind, B, xv, cin, w_packed, cout, y1v, s1, dt, y2v=None, s2=0.0, bias=None):
    """Conv whose output goes straight through LeakyReLU/ReLU (no BatchNorm): y1 = act(out, s1) [and
    y2 = act(out, s2)] from the conv epilogue, bit-identical to conv + bn_apply(table None) without the raw
    tensor.  Returns False (nothing launched) when the shape has no such epilogue: the caller then runs the
    two-call form."""
    l = lib()
    y2 = y2v if y2v is not None else L.NULL_VIEW
    if not FUSE_ACT or dt != torch.bfloat16 or not l.stc_conv_fwd_act_ok(L.dtype_code(dt), kind, B, xv, cin, cout,
                                                                           y1v, y2):
        return False
    gh, gw = (xv.H, xv.W) if kind == L.CONVT_S2 else (y1v.H, y1v.W)
    dev = w_packed.device
    nbytes = _conv_ws_bytes(kind, B, gh, gw, cin, cout, dt)
    ws, nb = _ws(nbytes, dev)
    timer = _timer
    if timer is not None:
        e0, e1 = _main_events()
    rc = l.stc_conv_fwd_act(L.dtype_code(dt), kind, B, xv, cin, ptr(w_packed), cout, y1v, float(s1), y2, float(s2),
                            ptr(bias), ptr(ws), nb, stream())
    if timer is not None:
        _disarm()
    check(rc, "stc_conv_fwd_act")
    if timer is not None:
        # the 8-channel first layers run the streaming stem kernel (csrc/stem_bf16.hip, stem_eligible)
        stem = (kind == L.CONV_S2 and cin == 8 and cout == 64 and xv.W in (256, 512) and xv.co == 0 and xv.ps == 8
                and xv.H == 2 * gh and gh % 8 == 0)
        _time_entry(timer, kind, B, gh, gw, cin, cout, dt, e0, e1,
                    name=f"stem_conv_kernel<{xv.W}, {2 if y2v is not None else 1}>" if stem else None)
    return True


def conv_act_backward(kind, B, xv, cin, w_packed, cout, yv, dt, act_x, s_self, g_other=None, s_other=0.0):
    """Input-gradient conv (output yv) whose output reaches an activation with no BatchNorm: yv receives
    g_other*act'(x, s_other) + out*act'(x, s_self) (x = ``act_x``, the activation's input) from the conv epilogue,
    bit-identical to conv + bn_backward(no table) without the intermediate gradient tensor.  Returns False (nothing
    launched) when the layer has no such epilogue: the caller then runs the two-call form."""
    if not FUSE_ACT_BWD or dt != torch.bfloat16:
        return False
    l = lib()
    g2 = g_other if g_other is not None else L.NULL_VIEW
    key = ("actb", kind, B, cin, cout, L.layout_key(xv), L.layout_key(yv), L.layout_key(act_x),
           L.layout_key(g2) if g_other is not None else None)
    ok = _MEMO.get(key)
    if ok is None:
        ok = _MEMO[key] = bool(l.stc_conv_bwd_act_ok(L.dtype_code(dt), kind, B, xv, cin, cout, yv, act_x, g2))
    if not ok:
        return False
    timer = _timer
    if timer is not None:
        e0, e1 = _main_events()
    rc = l.stc_conv_bwd_act(L.dtype_code(dt), kind, B, xv, cin, ptr(w_packed), cout, yv, act_x, float(s_self), g2,
                            float(s_other), stream())
    if timer is not None:
        _disarm()
    check(rc, "stc_conv_bwd_act")
    if timer is not None:
        gh, gw = (xv.H, xv.W) if kind == L.CONVT_S2 else (yv.H, yv.W)
        _time_entry(timer, kind, B, gh, gw, cin, cout, dt, e0, e1, bnb=True)
    return True


def conv_stats(kind, B, xv, cin, w_packed, cout, yv, dt, bias=None, force=None, pad=L.PAD_ZEROS):
    """Conv forward + fused BatchNorm partial statistics of its output (stc_conv_fwd_ex).
    Returns (part [chunks, cout, 4] fp32, chunks) for bn_finalize.  pad=L.PAD_REFLECT: the reflect conv, the
    partials from a pass over its stored output (conv_pad)."""
    if pad != L.PAD_ZEROS:
        return conv_pad(kind, B, xv, cin, w_packed, cout, yv, dt, pad, bias=bias, stats=True)
    dev = w_packed.device
    gh, gw = (xv.H, xv.W) if kind == L.CONVT_S2 else (yv.H, yv.W)
    if force is None and FORCE_CONV:
        force = FORCE_CONV.get((kind, B, gh, gw, cin, cout))
    nbytes, nch, plan = conv_query(kind, B, gh, gw, cin, cout, dt, force=force)
    ws, nb = _ws(nbytes, dev)
    part = torch.empty((nch, cout, 4), dtype=torch.float32, device=dev)
    fp = (ctypes.c_int32 * 2)(*force) if force is not None else None
    timer = _timer
    if timer is not None:
        e0, e1 = _main_events()
    rc = lib().stc_conv_fwd_ex(L.dtype_code(dt), kind, B, xv, cin, ptr(w_packed), cout, yv, ptr(bias), 0, 0,
                               ptr(part), nch, fp, ptr(ws), nb, stream())
    if timer is not None:
        _disarm()
    check(rc, "stc_conv_fwd_ex")
    if timer is not None:
        _time_entry(timer, kind, B, gh, gw, cin, cout, dt, e0, e1)
    return part, nch


def conv_bn_act(kind, B, xv, cin, w_packed, cout, yv, dt, bn, apply_x, y1, s1, y2=None, s2=0.0, defer=None,
                drop=None, pad=L.PAD_ZEROS):
    """A BatchNorm layer's train-mode forward: conv into ``yv`` with the batch statistics, the BN finalize (running
    statistics updated) and the activation pass of ``apply_x`` into y1 [and y2] (y1 None: no pass) -- one library call
    (stc_conv_bn_fwd; the instrumented / forced-plan runs take the three separate calls).  Returns ((2, cout) scale /
    shift table, (mean, rstd)), views of one fp32 buffer.  defer (a list): the running statistics are left alone and
    (partials, chunks, cout, bn) is appended for bn_running_update.  drop (a dropout level, see dropout_next): the
    activation pass applies the dropout mask (stc_conv_bn_fwd_drop, the same launches).  pad=L.PAD_REFLECT: the
    three separate calls, around the reflect conv."""
    dev = w_packed.device
    gh, gw = (xv.H, xv.W) if kind == L.CONVT_S2 else (yv.H, yv.W)
    upd = defer is None
    if pad != L.PAD_ZEROS or _timer is not None or (FORCE_CONV and (kind, B, gh, gw, cin, cout) in FORCE_CONV):
        t = torch.empty((2, cout), dtype=torch.float32, device=dev)
        part, nch = conv_stats(kind, B, xv, cin, w_packed, cout, yv, dt, pad=pad)
        st = bn_finalize_part(part, nch, cout, bn, t[0], t[1], update_running=upd)
        if not upd:
            defer.append((part, nch, cout, bn))
        if y1 is not None:
            bn_apply(B, apply_x, cout, dt, (t[0], t[1]), y1, s1, y2, s2, drop=drop)
        return t, st
    nbytes, nch, _ = conv_query(kind, B, gh, gw, cin, cout, dt)
    ws, nb = _ws(nbytes, dev)
    P = nch * cout * 4
    fws = torch.empty(P + 4 * cout, dtype=torch.float32, device=dev)
    mom = bn.momentum if bn.momentum is not None else BN_MOMENTUM
    if drop is not None:
        d = _drop(drop)
        check(lib().stc_conv_bn_fwd_drop(L.dtype_code(dt), kind, B, xv, cin, ptr(w_packed), cout, yv, ptr(fws), nch,
                                         ptr(bn.weight), ptr(bn.bias), ptr(bn.running_mean) if upd else None,
                                         ptr(bn.running_var) if upd else None,
                                         ptr(bn.num_batches_tracked) if upd else None, float(mom), float(bn.eps),
                                         apply_x, y1, float(s1), y2 if y2 is not None else L.NULL_VIEW, float(s2),
                                         ctypes.byref(d), ptr(ws), nb, stream()), "stc_conv_bn_fwd_drop")
        if not upd:
            defer.append((fws, nch, cout, bn))
        tab = fws[P:]
        return tab[2 * cout:].view(2, cout), (tab[:cout], tab[cout:2 * cout])
    check(lib().stc_conv_bn_fwd(L.dtype_code(dt), kind, B, xv, cin, ptr(w_packed), cout, yv, ptr(fws), nch,
                                ptr(bn.weight), ptr(bn.bias), ptr(bn.running_mean) if upd else None,
                                ptr(bn.running_var) if upd else None, ptr(bn.num_batches_tracked) if upd else None,
                                float(mom), float(bn.eps),
                                apply_x if y1 is not None else L.NULL_VIEW, y1 if y1 is not None else L.NULL_VIEW,
                                float(s1), y2 if y2 is not None else L.NULL_VIEW, float(s2), ptr(ws), nb, stream()),
          "stc_conv_bn_fwd")
    if not upd:
        defer.append((fws, nch, cout, bn))
    tab = fws[P:]
    return tab[2 * cout:].view(2, cout), (tab[:cout], tab[cout:2 * cout])


# ----------------------------------------------------------------------------- dropout (use_dropout=True generators)
# A dropout level of one generator call is the tuple ``(call_state, level, p, H, W)``: the call's device int64
# {seed, offset} (dropout_next), the U-Net block, the drop probability and the full ConvT extent the mask's logical
# index runs over (include/stcgan_hip.h, stc_dropout; csrc/philox.hpp holds the mask function).


def dropout_rank_seed(base, rank=0, world=1, net=0):
    """The 64-bit dropout seed of generator number ``net`` on data-parallel rank ``rank``: distinct for every
    (net, rank) of one run -- base + net * world + rank, modulo 2^64."""
    return (int(base) + int(net) * int(world) + int(rank)) & 0xFFFFFFFFFFFFFFFF


def dropout_state_tensor(seed, offset, device):
    """The device int64 {seed, offset} of a generator (the unsigned 64-bit seed stored in two's complement)."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    return torch.tensor([seed - (1 << 64) if seed >= (1 << 63) else seed, int(offset)], dtype=torch.int64,
                        device=device)


def dropout_next(state):
    """One call's counter (stc_dropout_next, one tiny launch): returns a new device {seed, offset} copy for every
    dropout kernel of this call, forward and backward, and advances ``state``'s offset by one."""
    assert state.dtype == torch.int64 and state.numel() == 2 and state.is_contiguous()
    call = torch.empty(2, dtype=torch.int64, device=state.device)
    check(lib().stc_dropout_next(ptr(state), ptr(call), stream()), "stc_dropout_next")
    return call


def _drop(drop):
    state, level, p, H, W = drop
    d = L.Dropout(state.data_ptr(), float(p), int(level), int(H), int(W), 0)
    d._keep = state
    return d


def dropout_mask(state, level, shape, p=0.5):
    """keep (1) / drop (0) of every element of the NHWC full extent ``shape`` = (B, H, W, C) at ``level`` for the
    {seed, offset} in ``state`` (device int64[2]) -- the device function the dropout kernels use (stc_dropout_mask).
    Returns a uint8 NHWC tensor."""
    B, H, W, C = shape
    out = torch.empty((B, H, W, C), dtype=torch.uint8, device=state.device)
    d = _drop((state, level, p, H, W))
    check(lib().stc_dropout_mask(ctypes.byref(d), B, C, ptr(out), stream()), "stc_dropout_mask")
    return out


def bn_running_update(part, nch, C, bn):
    """The running-statistics update a train-mode BatchNorm call left for later (conv_bn_act(defer=...)): the same
    finalize launch on the same partials (so the same mean / variance, bit for bit) with the running buffers this
    time, its table output discarded."""
    dev = part.device
    scratch = torch.empty(2 * C, dtype=torch.float32, device=dev)
    mom = bn.momentum if bn.momentum is not None else BN_MOMENTUM
    check(lib().stc_bn_finalize(ptr(part), nch, C, ptr(bn.weight), ptr(bn.bias), ptr(bn.running_mean),
                                ptr(bn.running_var), ptr(bn.num_batches_tracked), float(mom), float(bn.eps), None, None,
                                ptr(scratch), ptr(scratch[C:]), stream()), "stc_bn_finalize")


# bf16 LDS-DMA tile configurations (csrc/igemm_bf16.hip kTiles): cfg -> (BM, BN, WM, WN, stages, BK[, loader waves])
_BF16_TILES = [(128, 128, 2, 2, 2, 64), (256, 128, 2, 2, 2, 64), (128, 64, 2, 2, 2, 64), (256, 64, 4, 1, 2, 64),
               (64, 128, 1, 4, 2, 64), (64, 64, 2, 2, 2, 64), (256, 256, 2, 4, 2, 64), (128, 256, 2, 4, 2, 64),
               (128, 128, 2, 2, 3, 64), (128, 256, 2, 4, 3, 64), (64, 128, 1, 4, 3, 64), (128, 64, 2, 2, 3, 64),
               (64, 64, 2, 2, 3, 64), (256, 128, 4, 2, 3, 64), (256, 256, 2, 4, 4, 32), (256, 128, 4, 2, 4, 32),
               (128, 256, 2, 4, 4, 32), (128, 128, 2, 2, 4, 32), (128, 64, 2, 2, 4, 32), (64, 64, 2, 2, 4, 32),
               (128, 128, 2, 2, 3, 32), (128, 128, 2, 2, 2, 32), (256, 128, 4, 2, 3, 32), (128, 64, 2, 2, 3, 32),
               (128, 128, 2, 4, 2, 64), (128, 128, 4, 2, 2, 64), (128, 64, 4, 2, 2, 64), (256, 128, 4, 4, 2, 64),
               (128, 256, 4, 4, 2, 64), (128, 128, 2, 2, 4, 64, 4), (128, 128, 2, 2, 3, 64, 4),
               (256, 128, 4, 2, 3, 64, 4), (128, 64, 2, 2, 4, 64, 4), (128, 128, 2, 2, 2, 64, 2),
               (128, 64, 2, 2, 2, 64, 2), (128, 256, 2, 4, 2, 64, 2)]


# plan config of the conv-s2 halo kernel (stc_conv_fwd_query plan[4]; force_plan (HALO_CFG, 1) forces it)
HALO_CFG = 100


def kernel_name(kind, B, gh, gw, cin, cout, dt, bnb=False):
    """(kernel symbol as rocprof shows it, launches-a-single-kernel) of one conv call
    (bnb: the input-gradient form with the BatchNorm-backward reduction fused in)."""
    ws, _, plan = conv_query(kind, B, gh, gw, cin, cout, dt)
    bm, bn, ks, narrow, cfg = plan
    if narrow:
        if dt == torch.bfloat16 and cin % 64 == 0:
            geom = 0 if kind == L.CONVT_S2 else 1
            npc = 4 * cout if geom == 0 else cout
            nb = 2 if npc > 16 else 1
            # csrc/narrow_bf16.hip narrow_plan: the streaming ConvT kernel where it applies, else the 4x16 K-split tile
            if geom == 0 and gh % 16 == 0 and gw % 64 == 0 and ((cin == 128 and npc <= 16) or
                                                               (cin == 64 and 16 < npc <= 32)):
                return f"narrow_stream_kernel<{cin}, {nb}, {3 if cin == 128 else 4}>", True
            if geom == 1 and cout == 1 and cin in (256, 512):  # the two-pass logits form (taps GEMM + gather)
                return f"logits_taps_kernel<{cin}>", False
            return f"narrow_wk_kernel<{geom}, {nb}, 4, 1>", ws == 0
        return "narrow_tiled_kernel", True
    if cfg == HALO_CFG:  # the LDS-resident input halo kernels (csrc/halo_bf16.hip): template as rocprof names it
        convt = kind == L.CONVT_S2
        geom = {L.CONV_S2: 0, L.CONVT_S2: 1, L.CONV_S1: 2, L.CONV_S1_DGRAD: 3}[kind]
        vh, vw = (gh + 1, gw + 1) if kind == L.CONV_S1 else (gh, gw)  # (the s1 forward: its input grid)
        blocks = B * vh * vw // 256 * ((cout + bn - 1) // bn) * (4 if convt else 1)
        if bn == 64:  # (csrc/halo_bf16.hip halo_launch: conv-s2 grids <= 32 wide take the 8-wave 256 x 64 block)
            rb, wm, wn = (128, 8, 1) if (kind == L.CONV_S2 and vw <= 32) else (64, 4, 1)
            if convt and blocks // 2 >= 256:  # (the ConvT phase pair, GEOM 4: two phases per block)
                geom = 4
        else:
            rb, wm, wn = (64, 2, 2) if blocks >= 512 else (128, 4, 2)
        return (f"halo_conv_kernel<{geom}, {vw}, {bn}, {str(bnb).lower()}, {rb}, {wm}, {wn}>", True)
    if cfg >= 0:
        t = _BF16_TILES[cfg]
        if len(t) > 6:  # loader-wave blocks
            return (f"igemm_bf16_ld_kernel<{t[0]}, {t[1]}, {t[2]}, {t[3]}, {t[4]}, {t[5]}, {str(bnb).lower()}, {t[6]}>",
                    ks == 1)
        return f"igemm_bf16_kernel<{t[0]}, {t[1]}, {t[2]}, {t[3]}, {t[4]}, {t[5]}, {str(bnb).lower()}>", ks == 1
    tname = {torch.float32: "float", torch.bfloat16: "__hip_bfloat16"}[dt]
    return f"igemm_kernel<{tname}, {bm}, {bn}>", ks == 1


def _time_entry(timer, kind, B, gh, gw, cin, cout, dt, e0, e1, bnb=False, name=None):
    name, single = (name, True) if name else kernel_name(kind, B, gh, gw, cin, cout, dt, bnb)
    outs = B * gh * gw * (4 if kind == L.CONVT_S2 else 1)
    taps = 4 if kind == L.CONVT_S2 else 16
    timer.append((name, single, 2.0 * outs * cout * taps * cin, e0, e1,
                  f"{['conv_s2', 'conv_s1', 'convT', 's1_dgrad'][kind]} B{B} grid{gh}x{gw} cin{cin} cout{cout}"))


def conv_bn_backward(kind, B, xv, cin, w_packed, cout, yv, dt, bn_x, C, bn_state, gamma, s_self, ch_off=0,
                     g_other=None, s_other=0.0, dxv=None, dgamma=None, dbeta=None):
    """Input-gradient conv (output yv) whose output feeds a BatchNorm backward, with the BN
    reduction fused into the conv (stc_conv_bwd_bn), then the BN apply (stc_bn_bwd_apply):
    dx = BN-backward of dn = out*act'(n, s_self) [+ g_other*act'(n, s_other)].
    bn_state = (scale, shift, mean, rstd); returns (dgamma, dbeta) (written into ``dgamma``/``dbeta`` when given)."""
    dev = w_packed.device
    l = lib()
    gh, gw = (xv.H, xv.W) if kind == L.CONVT_S2 else (yv.H, yv.W)
    nbytes = _conv_ws_bytes(kind, B, gh, gw, cin, cout, dt)
    ws, nb = _ws(nbytes, dev)
    scale, shift, mean, rstd = bn_state
    fuse = L.BnbFuse(bn_x, g_other if g_other is not None else L.NULL_VIEW, scale.data_ptr(), shift.data_ptr(),
                     mean.data_ptr(), rstd.data_ptr(), float(s_self), float(s_other), C, ch_off)
    # the chunk count depends on which kernel takes the call, which depends on the views' layout (not only shapes)
    key = ("bnbch", kind, B, cin, cout, dt, L.layout_key(xv), L.layout_key(yv), bn_x.H, bn_x.W, g_other is None)
    nch = _MEMO.get(key)
    if nch is None:
        nch = _MEMO[key] = l.stc_conv_bwd_bn_chunks_ex(L.dtype_code(dt), kind, B, xv, cin, cout, yv,
                                                       ctypes.byref(fuse))
        check(0 if nch > 0 else -1, "stc_conv_bwd_bn_chunks_ex")
    part = torch.empty((nch, C, 2), dtype=torch.float32, device=dev)
    timer = _timer
    dgamma = _out1(dgamma, C, dev)
    dbeta = _out1(dbeta, C, dev)
    if timer is None:  # (both launches from one call)
        check(l.stc_conv_bwd_bn_apply(L.dtype_code(dt), kind, B, xv, cin, ptr(w_packed), cout, yv, ctypes.byref(fuse),
                                      ptr(part), nch, ptr(gamma), dxv, ptr(dgamma), ptr(dbeta), ptr(ws), nb, stream()),
              "stc_conv_bwd_bn_apply")
        return dgamma, dbeta
    e0, e1 = _main_events()
    rc = l.stc_conv_bwd_bn(L.dtype_code(dt), kind, B, xv, cin, ptr(w_packed), cout, yv, ctypes.byref(fuse),
                           ptr(part), nch, ptr(ws), nb, stream())
    _disarm()
    check(rc, "stc_conv_bwd_bn")
    _time_entry(timer, kind, B, gh, gw, cin, cout, dt, e0, e1, bnb=yv.cs == 1)
    # apply: g1 = the conv output at the BN channels over the BN extent
    g1 = L.View(yv.p, bn_x.H, bn_x.W, yv.bs, yv.rs, yv.ps, yv.co + ch_off, yv.cs, 0)
    g1._keep = yv
    check(l.stc_bn_bwd_apply(L.dtype_code(dt), B, bn_x, C, ptr(scale), ptr(shift), ptr(mean), ptr(rstd), ptr(gamma),
                             g1, float(s_self), g_other if g_other is not None else L.NULL_VIEW, float(s_other),
                             ptr(part), nch, dxv, ptr(dgamma),
                             ptr(dbeta), stream()), "stc_bn_bwd_apply")
    return dgamma, dbeta


def bn_finalize_part(part, nch, C, bn, scale_out, shift_out, update_running=True):
    """mean/rstd + (scale, shift) table from conv_stats partials; updates running stats."""
    dev = scale_out.device
    mean = torch.empty(C, dtype=torch.float32, device=dev)
    rstd = torch.empty(C, dtype=torch.float32, device=dev)
    rm = bn.running_mean if update_running else None
    rv = bn.running_var if update_running else None
    nbt = bn.num_batches_tracked if update_running else None
    mom = bn.momentum if bn.momentum is not None else BN_MOMENTUM
    check(lib().stc_bn_finalize(ptr(part), nch, C, ptr(bn.weight), ptr(bn.bias), ptr(rm), ptr(rv), ptr(nbt),
                                float(mom), float(bn.eps), ptr(mean), ptr(rstd), ptr(scale_out), ptr(shift_out),
                                stream()), "stc_bn_finalize")
    return mean, rstd


def wgrad_query(B, Hd, Wd, R, Cg, dt, force=None):
    """(workspace bytes, plan (cfg, BM, BN, splits, slab)) of stc_conv_wgrad_ex for these arguments."""
    key = ("wq", B, Hd, Wd, R, Cg, dt, None if force is None else tuple(force))
    r = _MEMO.get(key)
    if r is not None:
        return r
    ws = ctypes.c_int64()
    po = (ctypes.c_int32 * 5)()
    fp = (ctypes.c_int32 * 2)(*force) if force is not None else None
    check(lib().stc_conv_wgrad_query(L.dtype_code(dt), B, Hd, Wd, R, Cg, fp, ctypes.byref(ws), po),
          "stc_conv_wgrad_query")
    r = _MEMO[key] = (ws.value, tuple(po))
    return r


# The narrow-R weight gradient (stc_conv_wgrad_rows) for the PatchGAN logits layer: bf16 on the MFMA rows kernel
# (11 + 5 us with its ordered reduce, bs=32), fp32 on the VALU rows kernel (non-packed v_fma_f32: compiled to
# v_pk_fma_f32 with op_sel it returned sporadically different low-half sums with two processes on one GPU,
# tests/test_gpu_dist.py); ~75 us for the padded GEMM.  rows_kernel=False per call takes the GEMM path.
_ROWS_DEFAULT = True


def _out1(t, n, device):
    """A caller-provided fp32 output of n elements (e.g. a view of a flat gradient buffer), or a new one."""
    if t is None:
        return torch.empty(n, dtype=torch.float32, device=device)
    assert t.dtype == torch.float32 and t.is_contiguous() and t.numel() == n, "output: fp32, contiguous, n elements"
    return t


def _out_w(t, R, Cg_out, device):
    if t is None:
        return torch.empty((R, Cg_out, 4, 4), dtype=torch.float32, device=device)
    assert t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == (R, Cg_out, 4, 4), \
        f"wgrad output: fp32 contiguous [{R}, {Cg_out}, 4, 4], got {tuple(t.shape)}"
    return t


def wgrad_pad_query(stride, B, Hd, Wd, R, Cg, dt, pad, force=None):
    """(workspace bytes, plan (cfg, BM, BN, splits, slab)) of stc_conv_pad_wgrad over the output grid Hd x Wd."""
    key = ("wpq", stride, B, Hd, Wd, R, Cg, dt, pad, None if force is None else tuple(force))
    r = _MEMO.get(key)
    if r is None:
        ws, po = ctypes.c_int64(), (ctypes.c_int32 * 5)()
        fp = (ctypes.c_int32 * 2)(*force) if force is not None else None
        check(lib().stc_conv_pad_wgrad_query(L.dtype_code(dt), L.CONV_S2 if stride == 2 else L.CONV_S1, pad, B, Hd, Wd,
                                             R, Cg, fp, ctypes.byref(ws), po), "stc_conv_pad_wgrad_query")
        r = _MEMO[key] = (ws.value, tuple(po))
    return r


def _wgrad_route(B, stride, Dv, R, Gv, Cg, Cg_out, dt, rows=0, prologue=False, pad=L.PAD_ZEROS, force=None):
    """(workspace bytes, plan (cfg, BM, BN, slabs, slab), kernel (L.WG_*), reduce, kernel name) of one weight-gradient
    call, for its views and stride: stc_conv_wgrad_route (csrc/wgrad_route.cpp decides, nothing here does)."""
    key = ("wr", B, R, Cg, Cg_out, dt, L.layout_key(Dv), L.layout_key(Gv), stride, rows, prologue, pad,
           None if force is None else tuple(force))
    r = _MEMO.get(key)
    if r is None:
        ws, po, ko = ctypes.c_int64(), (ctypes.c_int32 * 5)(), (ctypes.c_int32 * 2)()
        name = ctypes.create_string_buffer(96)
        fp = (ctypes.c_int32 * 2)(*force) if force is not None else None
        check(lib().stc_conv_wgrad_route(L.dtype_code(dt), B, stride, Dv, R, rows, Gv, Cg, Cg_out, int(prologue), pad, fp,
                                         ctypes.byref(ws), po, ko, name, 96), "stc_conv_wgrad_route")
        r = _MEMO[key] = (ws.value, tuple(po), ko[0], ko[1], name.value.decode())
    return r


def wgrad(B, stride, Dv, R, Gv, Cg, Cg_out, dt, dpro=None, dslope=None, gpro=None, gslope=None, device=None,
          force=None, rows=None, rows_kernel=None, out=None, pad=L.PAD_ZEROS):
    """Weight gradient [R][Cg_out][4][4] fp32 (force = optional {tile config, splits}), written into ``out`` when
    given (e.g. a view of a flat gradient buffer).  The library's route (_wgrad_route) names the kernel, and with it
    the entry point: stc_conv_wgrad_rows, stc_conv_pad_wgrad (reflect) or stc_conv_wgrad_ex.
    rows: the number of nonzero (real) channels of D when the rest is padding -- a stride-1 layer with
    1-2 of them goes to the rows kernels (which then write only R = ``rows`` rows when R == rows).
    pad=L.PAD_REFLECT (a Conv2d's weight gradient: Dv its output gradient, Gv its input): the register-staged kernel
    with the reflect gather; no prologue, no rows kernel."""
    l = lib()
    reflect = pad != L.PAD_ZEROS
    pro = dpro is not None or gpro is not None or dslope is not None or gslope is not None
    if reflect and pro:
        raise ValueError("stcgan_amd: a reflect weight gradient takes no prologue")
    if not rows or not (_ROWS_DEFAULT if rows_kernel is None else rows_kernel):
        rows = 0
    route = _wgrad_route(B, stride, Dv, R, Gv, Cg, Cg_out, dt, rows, pro, pad, force)
    is_rows = route[2] in (L.WG_ROWS, L.WG_ROWS_MFMA)
    if is_rows and out is not None and out.shape[0] == rows:  # only the real rows (e.g. straight into a gradient view)
        R = rows
    if out is not None and out.shape[0] != R:  # real rows of a padded R: through a scratch
        full = wgrad(B, stride, Dv, R, Gv, Cg, Cg_out, dt, dpro, dslope, gpro, gslope, device, force, pad=pad)
        out.copy_(full[:out.shape[0]])
        return out
    if force is None and FORCE_WGRAD and not is_rows and not reflect:
        force = FORCE_WGRAD.get((B, Dv.H, Dv.W, R, Cg))
        if force is not None:
            route = _wgrad_route(B, stride, Dv, R, Gv, Cg, Cg_out, dt, rows, pro, pad, force)
    nbytes, plan, _, _, name = route
    if not is_rows and not reflect:  # the D grid's bound, whatever the stride: the cached workspace grows once per grid
        nbytes = wgrad_query(B, Dv.H, Dv.W, R, Cg, dt, force)[0]
    ws, nb = _ws(nbytes, device)
    dW = _out_w(out, R, Cg_out, device)
    fp = (ctypes.c_int32 * 2)(*force) if force is not None else None
    timer, ctimer = _timer, _call_timer
    if timer is not None:
        e0, e1 = _main_events()
    if ctimer is not None:
        c0, c1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        c0.record()
    if is_rows:
        what = "stc_conv_wgrad_rows"
        rc = l.stc_conv_wgrad_rows(L.dtype_code(dt), B, Dv, R, rows, Gv, Cg, Cg_out, ptr(dW), ptr(ws), nb, stream())
    elif reflect:
        what = "stc_conv_pad_wgrad"
        rc = l.stc_conv_pad_wgrad(L.dtype_code(dt), L.CONV_S2 if stride == 2 else L.CONV_S1, pad, B, Dv, R, Gv, Cg,
                                  Cg_out, ptr(dW), fp, ptr(ws), nb, stream())
    else:
        what = "stc_conv_wgrad_ex"
        dsc, dsh = _pro(dpro)
        gsc, gsh = _pro(gpro)
        rc = l.stc_conv_wgrad_ex(L.dtype_code(dt), B, stride, Dv, R, dsc, dsh, 0 if dslope is None else 1,
                                 0.0 if dslope is None else float(dslope), Gv, Cg, Cg_out, gsc, gsh,
                                 0 if gslope is None else 1, 0.0 if gslope is None else float(gslope), ptr(dW), fp,
                                 ptr(ws), nb, stream())
    if ctimer is not None:
        c1.record()
    if timer is not None:
        _disarm()
    check(rc, what)
    if ctimer is not None:
        ctimer.append((name, c0, c1))
    if timer is not None:
        timer.append((name, is_rows or not plan[4], 2.0 * B * Dv.H * Dv.W * R * 16 * Cg, e0, e1,
                      f"wgrad s{stride} P={B * Dv.H * Dv.W} R{R}" + (f" (real {rows})" if is_rows else "") + f" Cg{Cg}"))
    return dW


_PHASED = {L.PACK_CONV_DGRAD, L.PACK_CONVT_FWD, L.PACK_UPCONV_FWD}
# the ConvT operands of a resize-convolution up layer, made from its conv weight [Co][Ci][3][3]
_UPCONV = {L.PACK_UPCONV_FWD, L.PACK_UPCONV_DGRAD}


def _pack_pq(mode, W):
    """(P, Q) of stc_pack_weight for weight W: its two leading extents; (Ci, Co) of a [Co][Ci][3][3] conv weight
    for the UPCONV modes (the extents of the ConvT weight it stands for)."""
    if mode in _UPCONV:
        assert tuple(W.shape[2:]) == (3, 3), "UPCONV pack modes take a [Co][Ci][3][3] weight"
        return W.shape[1], W.shape[0]
    return W.shape[0], W.shape[1]


# bumped whenever a packed-operand buffer is created or dropped: the optimiser's cached pointer tables
# (optim.Adam._fast_step) hold the addresses of these buffers
PACK_EPOCH = 0


def invalidate_packs():
    global PACK_EPOCH
    PACK_EPOCH += 1


def pack(mode, W, n_pad, c_pad, dt):
    """Pack a torch weight [P][Q][4][4] (UPCONV modes: [Co][Ci][3][3]) into the GEMM operand layout
    [phases][n_pad][taps][c_pad]."""
    invalidate_packs()
    P, Q = _pack_pq(mode, W)
    nph, taps = (4, 4) if mode in _PHASED else (1, 16)
    out = torch.empty((nph, n_pad, taps, c_pad), dtype=dt, device=W.device)
    Wc = W.detach()
    if not Wc.is_contiguous():
        Wc = Wc.contiguous()
    check(lib().stc_pack_weight(L.dtype_code(dt), mode, ptr(Wc), P, Q, ptr(out), n_pad, c_pad, stream()),
          "stc_pack_weight")
    return out


# generation counter bumped by our optimizer (it updates parameters in place behind autograd's back)
_GEN = {}
# id(weight) -> {cache key: cache} of every packed operand made from it (the optimizer rewrites
# them in the same pass as the update: stc_adam_pack_step)
_PACK_OWNERS = {}


def pack_version(W):
    return (W._version, _GEN.get(id(W), 0), W.data_ptr())


def pack_targets(W):
    """[(key, cache, mode, out, n_pad, c_pad, dtype)] of the packed operands of weight W."""
    out = []
    for key, cache in _PACK_OWNERS.get(id(W), {}).items():
        hit = cache.get(key)
        if hit is None:
            continue
        _, mode, n_pad, c_pad, dt = cache["__keys__"][key]
        out.append((key, cache, mode, hit[1], n_pad, c_pad, dt))
    return out


def bump(params):
    for p in params:
        _GEN[id(p)] = _GEN.get(id(p), 0) + 1


def packed(cache, W, mode, n_pad, c_pad, dt):
    """Cached packed weight; repacked when the parameter changed (version or optimizer step).
    Every key is remembered so that refresh_packs() can repack all stale ones in one launch."""
    key = (id(W), mode, n_pad, c_pad, dt)
    ver = (W._version, _GEN.get(id(W), 0), W.data_ptr())
    hit = cache.get(key)
    if hit is not None and hit[0] == ver:
        return hit[1]
    cache.setdefault("__keys__", {})[key] = (W, mode, n_pad, c_pad, dt)
    _PACK_OWNERS.setdefault(id(W), {})[key] = cache
    t = pack(mode, W, n_pad, c_pad, dt)
    cache[key] = (ver, t)
    return t


def refresh_packs(cache):
    """Repack every stale cached operand of a network (after an optimiser step) with one
    multi-tensor launch per dtype (stc_pack_weights), reusing the packed buffers in place."""
    keys = cache.get("__keys__")
    if not keys:
        return
    jobs = {}
    for key, (W, mode, n_pad, c_pad, dt) in keys.items():
        ver = (W._version, _GEN.get(id(W), 0), W.data_ptr())
        hit = cache.get(key)
        if hit is not None and hit[0] == ver:
            continue
        if hit is None:
            nph, taps = (4, 4) if mode in _PHASED else (1, 16)
            out = torch.empty((nph, n_pad, taps, c_pad), dtype=dt, device=W.device)
            invalidate_packs()
        else:
            out = hit[1]
        Wc = W.detach()
        assert Wc.is_contiguous()
        jobs.setdefault(dt, []).append((L.PackDesc(mode, *_pack_pq(mode, W), n_pad, c_pad, 0, Wc.data_ptr(),
                                                   out.data_ptr()), key, ver, out))
    for dt, lst in jobs.items():
        for i in range(0, len(lst), L.PACK_MAX):
            chunk = lst[i:i + L.PACK_MAX]
            arr = (L.PackDesc * len(chunk))(*[c[0] for c in chunk])
            check(lib().stc_pack_weights(L.dtype_code(dt), len(chunk), arr, stream()), "stc_pack_weights")
            for _, key, ver, out in chunk:
                cache[key] = (ver, out)


def upconv_expand(w3):
    """The ConvTranspose2d(4, 2, 1) weight [Ci][Co][4][4] equivalent to the resize-convolution weight w3
    [Co][Ci][3][3] (nearest 2x upsampling + zero-padded 3x3 conv): stc_upconv_expand, fp32, fixed summation order."""
    assert w3.dim() == 4 and tuple(w3.shape[2:]) == (3, 3) and w3.dtype == torch.float32
    w3 = w3.detach().contiguous()
    Co, Ci = w3.shape[0], w3.shape[1]
    W4 = torch.empty((Ci, Co, 4, 4), dtype=torch.float32, device=w3.device)
    check(lib().stc_upconv_expand(ptr(w3), Ci, Co, ptr(W4), stream()), "stc_upconv_expand")
    return W4


def upconv_wgrad_collapse(dW4, out):
    """out [Co][Ci][3][3] (contiguous fp32, any 4-byte aligned slice) = the adjoint of upconv_expand applied to
    the ConvT-layout gradient dW4 [Ci][Co][4][4]."""
    Ci, Co = dW4.shape[0], dW4.shape[1]
    assert tuple(out.shape) == (Co, Ci, 3, 3) and out.is_contiguous() and dW4.is_contiguous()
    check(lib().stc_upconv_wgrad_collapse(ptr(dW4), Ci, Co, ptr(out), stream()), "stc_upconv_wgrad_collapse")
    return out


def stats_chunks(B, H, W):
    return lib().stc_chan_stats_chunks(B, H, W)


def bn_train_table(B, xv, C, dt, bn, scale_out, shift_out, update_running=True):
    """Batch statistics of x (view, C channels) -> (mean, rstd); writes the prologue table
    scale_out/shift_out (views of C floats) and updates bn's running statistics."""
    dev = scale_out.device
    nch = stats_chunks(B, xv.H, xv.W)
    part = torch.empty((nch, C, 4), dtype=torch.float32, device=dev)
    check(lib().stc_chan_stats(L.dtype_code(dt), B, xv, C, ptr(part), nch, stream()), "stc_chan_stats")
    mean = torch.empty(C, dtype=torch.float32, device=dev)
    rstd = torch.empty(C, dtype=torch.float32, device=dev)
    rm = bn.running_mean if update_running else None
    rv = bn.running_var if update_running else None
    nbt = bn.num_batches_tracked if update_running else None
    mom = bn.momentum if bn.momentum is not None else BN_MOMENTUM
    check(lib().stc_bn_finalize(ptr(part), nch, C, ptr(bn.weight), ptr(bn.bias), ptr(rm), ptr(rv), ptr(nbt),
                                float(mom), float(bn.eps), ptr(mean), ptr(rstd), ptr(scale_out), ptr(shift_out),
                                stream()), "stc_bn_finalize")
    return mean, rstd


def bn_eval_table(C, bn, scale_out, shift_out):
    check(lib().stc_bn_finalize(None, 0, C, ptr(bn.weight), ptr(bn.bias), ptr(bn.running_mean),
                                ptr(bn.running_var), None, 0.0, float(bn.eps), None, None, ptr(scale_out),
                                ptr(shift_out), stream()), "stc_bn_finalize(eval)")


def bn_apply(B, xv, C, dt, table, y1, s1, y2=None, s2=1.0, drop=None):
    """y1 = act(x*scale+shift, s1) [, y2 = act(.., s2)]; table = (scale, shift) or None (identity).
    drop (a dropout level, see dropout_next): y = act((x*scale+shift) * keep/(1-p), s) (stc_bn_apply_drop)."""
    sc, sh = _pro(table)
    if drop is not None:
        d = _drop(drop)
        check(lib().stc_bn_apply_drop(L.dtype_code(dt), B, xv, C, sc, sh, y1, float(s1),
                                      y2 if y2 is not None else L.NULL_VIEW, float(s2), ctypes.byref(d), stream()),
              "stc_bn_apply_drop")
        return
    check(lib().stc_bn_apply(L.dtype_code(dt), B, xv, C, sc, sh, y1, float(s1),
                             y2 if y2 is not None else L.NULL_VIEW, float(s2), stream()), "stc_bn_apply")


def bn_backward(B, xv, C, dt, dxv, g1=None, s1=0.0, g2=None, s2=0.0, bn_state=None, dgamma=None, dbeta=None,
                drop=None):
    """Fused activation + BatchNorm backward.  bn_state = (scale, shift, mean, rstd, gamma) or None
    (no BN: dx = g1*act1'(x) + g2*act2'(x)).  Returns (dgamma, dbeta) or (None, None).
    drop (a dropout level, see dropout_next; needs bn_state and g1): g1 reaches the BN output through the dropout,
    g1 * keep/(1-p) with the mask recomputed from the call's counter (stc_bn_bwd_reduce_drop / _apply_drop)."""
    l = lib()
    g1v = g1 if g1 is not None else L.NULL_VIEW
    g2v = g2 if g2 is not None else L.NULL_VIEW
    dev_t = None
    if bn_state is None:
        if drop is not None:
            raise ValueError("bn_backward: the dropout form needs the BatchNorm state")
        check(l.stc_bn_bwd_apply(L.dtype_code(dt), B, xv, C, None, None, None, None, None, g1v, float(s1), g2v,
                                 float(s2), None, 0, dxv, None, None, stream()), "stc_bn_bwd_apply")
        return None, None
    scale, shift, mean, rstd, gamma = bn_state
    dev_t = scale.device
    nch = stats_chunks(B, xv.H, xv.W)
    part = torch.empty((nch, C, 2), dtype=torch.float32, device=dev_t)
    if drop is not None:
        d = _drop(drop)
        check(l.stc_bn_bwd_reduce_drop(L.dtype_code(dt), B, xv, C, ptr(scale), ptr(shift), ptr(mean), ptr(rstd), g1v,
                                       float(s1), g2v, float(s2), ctypes.byref(d), ptr(part), nch, stream()),
              "stc_bn_bwd_reduce_drop")
        dgamma = _out1(dgamma, C, dev_t)
        dbeta = _out1(dbeta, C, dev_t)
        check(l.stc_bn_bwd_apply_drop(L.dtype_code(dt), B, xv, C, ptr(scale), ptr(shift), ptr(mean), ptr(rstd),
                                      ptr(gamma), g1v, float(s1), g2v, float(s2), ctypes.byref(d), ptr(part), nch, dxv,
                                      ptr(dgamma), ptr(dbeta), stream()), "stc_bn_bwd_apply_drop")
        return dgamma, dbeta
    check(l.stc_bn_bwd_reduce(L.dtype_code(dt), B, xv, C, ptr(scale), ptr(shift), ptr(mean), ptr(rstd), g1v,
                              float(s1), g2v, float(s2), ptr(part), nch, stream()), "stc_bn_bwd_reduce")
    dgamma = _out1(dgamma, C, dev_t)
    dbeta = _out1(dbeta, C, dev_t)
    check(l.stc_bn_bwd_apply(L.dtype_code(dt), B, xv, C, ptr(scale), ptr(shift), ptr(mean), ptr(rstd), ptr(gamma),
                             g1v, float(s1), g2v, float(s2), ptr(part), nch, dxv, ptr(dgamma), ptr(dbeta), stream()),
          "stc_bn_bwd_apply")
    return dgamma, dbeta


# ----------------------------------------------------------------------------- sync statistics (nn.SyncBatchNorm)
# The split forms of conv_bn_act / conv_bn_backward / bn_backward with one exchange between "partials" and "table / dx"
# (DESIGN.md section 8g): every rank packs its partials into one record per channel, the records of all ranks are
# gathered in rank order (parallel.gather_records, one collective on the current stream) and every rank finishes
# from the same records -- the same bits everywhere.


def bn_stats_pack(part, nch, C):
    """One record {n, S1, S2, shift} per channel from this rank's ``nch`` chunk partials (stc_bn_stats_pack)."""
    rec = torch.empty((C, 4), dtype=torch.float32, device=part.device)
    check(lib().stc_bn_stats_pack(ptr(part), nch, C, ptr(rec), stream()), "stc_bn_stats_pack")
    return rec


def bn_bwd_sums(part2, nch, C, dgamma=None, dbeta=None):
    """This rank's dbeta / dgamma (into ``dgamma`` / ``dbeta`` when given, else not written) and the record
    [C, 2] = {sum dn, sum dn * xhat} of the backward reduce's partials (stc_bn_bwd_sums)."""
    rec = torch.empty((C, 2), dtype=torch.float32, device=part2.device)
    check(lib().stc_bn_bwd_sums(ptr(part2), nch, C, ptr(dgamma), ptr(dbeta), ptr(rec), stream()), "stc_bn_bwd_sums")
    return rec


def bn_bwd_apply_sync(B, xv, C, dt, dxv, g1, s1, g2, s2, bn_state, recs, count, drop=None):
    """dx of a BatchNorm on the statistics of ``count`` pixels spread over the ranks whose records
    ``recs`` [world, C, 2] holds (stc_bn_bwd_apply_sync); bn_state = (scale, shift, mean, rstd, gamma)."""
    scale, shift, mean, rstd, gamma = bn_state
    d = _drop(drop) if drop is not None else None
    assert recs.dim() == 3 and tuple(recs.shape[1:]) == (C, 2) and recs.is_contiguous()
    check(lib().stc_bn_bwd_apply_sync(L.dtype_code(dt), B, xv, C, ptr(scale), ptr(shift), ptr(mean), ptr(rstd),
                                      ptr(gamma), g1 if g1 is not None else L.NULL_VIEW, float(s1),
                                      g2 if g2 is not None else L.NULL_VIEW, float(s2),
                                      ctypes.byref(d) if d is not None else None, ptr(recs), recs.shape[0], int(count),
                                      dxv, stream()), "stc_bn_bwd_apply_sync")


def conv_bn_act_sync(kind, B, xv, cin, w_packed, cout, yv, dt, bn, apply_x, y1, s1, y2=None, s2=0.0, defer=None,
                     drop=None, gather=None, pad=L.PAD_ZEROS):
    """conv_bn_act on the statistics of all ranks: conv with its partials, pack, gather, the finalize over the ranks'
    records (every rank updates its running statistics with the global, unbiased-by-the-global-count values) and the
    activation pass.  defer (a list): (gathered records, world, cout, bn) is appended for bn_running_update."""
    upd = defer is None
    t = torch.empty((2, cout), dtype=torch.float32, device=w_packed.device)
    part, nch = conv_stats(kind, B, xv, cin, w_packed, cout, yv, dt, pad=pad)
    recs = gather(bn_stats_pack(part, nch, cout))
    st = bn_finalize_part(recs, recs.shape[0], cout, bn, t[0], t[1], update_running=upd)
    if not upd:
        defer.append((recs, recs.shape[0], cout, bn))
    if y1 is not None:
        bn_apply(B, apply_x, cout, dt, (t[0], t[1]), y1, s1, y2, s2, drop=drop)
    return t, st


def conv_bn_backward_sync(kind, B, xv, cin, w_packed, cout, yv, dt, bn_x, C, bn_state, gamma, s_self, ch_off, g_other,
                          s_other, dxv, dgamma, dbeta, count, gather):
    """conv_bn_backward on the statistics of all ranks: the input-gradient conv with the BatchNorm reduction fused in
    (stc_conv_bwd_bn), this rank's sums, the gather, the apply on the global sums."""
    dev = w_packed.device
    l = lib()
    gh, gw = (xv.H, xv.W) if kind == L.CONVT_S2 else (yv.H, yv.W)
    ws, nb = _ws(_conv_ws_bytes(kind, B, gh, gw, cin, cout, dt), dev)
    scale, shift, mean, rstd = bn_state
    fuse = L.BnbFuse(bn_x, g_other if g_other is not None else L.NULL_VIEW, scale.data_ptr(), shift.data_ptr(),
                     mean.data_ptr(), rstd.data_ptr(), float(s_self), float(s_other), C, ch_off)
    key = ("bnbch", kind, B, cin, cout, dt, L.layout_key(xv), L.layout_key(yv), bn_x.H, bn_x.W, g_other is None)
    nch = _MEMO.get(key)
    if nch is None:
        nch = _MEMO[key] = l.stc_conv_bwd_bn_chunks_ex(L.dtype_code(dt), kind, B, xv, cin, cout, yv,
                                                       ctypes.byref(fuse))
        check(0 if nch > 0 else -1, "stc_conv_bwd_bn_chunks_ex")
    part = torch.empty((nch, C, 2), dtype=torch.float32, device=dev)
    check(l.stc_conv_bwd_bn(L.dtype_code(dt), kind, B, xv, cin, ptr(w_packed), cout, yv, ctypes.byref(fuse),
                            ptr(part), nch, ptr(ws), nb, stream()), "stc_conv_bwd_bn")
    recs = gather(bn_bwd_sums(part, nch, C, dgamma, dbeta))
    # g1 = the conv output at the BN channels over the BN extent (as conv_bn_backward's split form)
    g1 = L.View(yv.p, bn_x.H, bn_x.W, yv.bs, yv.rs, yv.ps, yv.co + ch_off, yv.cs, 0)
    g1._keep = yv
    # the kernels form g1 * act1' + g2 * act2' in this order: another consumer's gradient first
    a1 = (g1, s_self, None, 0.0)
    if g_other is not None:
        a1 = (g_other, s_other, g1, s_self)
    bn_bwd_apply_sync(B, bn_x, C, dt, dxv, *a1, (scale, shift, mean, rstd, gamma), recs, count)


def bn_backward_sync(B, xv, C, dt, dxv, g1, s1, g2, s2, bn_state, dgamma, dbeta, drop, count, gather):
    """bn_backward on the statistics of all ranks: the reduce (through ``drop`` where there is one), this rank's sums,
    the gather, the apply on the global sums."""
    l = lib()
    scale, shift, mean, rstd, gamma = bn_state
    g1v = g1 if g1 is not None else L.NULL_VIEW
    g2v = g2 if g2 is not None else L.NULL_VIEW
    nch = stats_chunks(B, xv.H, xv.W)
    part = torch.empty((nch, C, 2), dtype=torch.float32, device=scale.device)
    if drop is not None:
        d = _drop(drop)
        check(l.stc_bn_bwd_reduce_drop(L.dtype_code(dt), B, xv, C, ptr(scale), ptr(shift), ptr(mean), ptr(rstd), g1v,
                                       float(s1), g2v, float(s2), ctypes.byref(d), ptr(part), nch, stream()),
              "stc_bn_bwd_reduce_drop")
    else:
        check(l.stc_bn_bwd_reduce(L.dtype_code(dt), B, xv, C, ptr(scale), ptr(shift), ptr(mean), ptr(rstd), g1v,
                                  float(s1), g2v, float(s2), ptr(part), nch, stream()), "stc_bn_bwd_reduce")
    recs = gather(bn_bwd_sums(part, nch, C, dgamma, dbeta))
    bn_bwd_apply_sync(B, xv, C, dt, dxv, g1, s1, g2, s2, bn_state, recs, count, drop)


def bn_running_rstd(C, bn, out=None):
    """rstd_run[c] = 1 / sqrt(running_var[c] + eps) of a BatchNorm2d (stc_bn_running_rstd): the factor inside
    bn_eval_table's scale, which the frozen-statistics backward needs on its own for dgamma."""
    out = _out1(out, C, bn.running_var.device)
    check(lib().stc_bn_running_rstd(C, ptr(bn.running_var), float(bn.eps), ptr(out), stream()), "stc_bn_running_rstd")
    return out


def bn_backward_frozen(B, xv, C, dt, dxv, g1, s1, g2=None, s2=0.0, state=None, dgamma=None, dbeta=None,
                       want_params=True, drop=None):
    """Fused activation + BatchNorm backward of a layer that normalised with its running statistics
    (stc_bn_bwd_frozen; one pass): dx = scale * dn into dxv, with dn as in bn_backward.  state = (scale, shift,
    running_mean, rstd_run) -- bn_eval_table's table, the buffer itself and bn_running_rstd.  want_params: also
    dbeta = sum dn and dgamma = sum dn * xhat (written into ``dgamma`` / ``dbeta`` when given); returns them, or
    (None, None) -- then no sums are formed and no partials buffer exists.  drop (a dropout level, see dropout_next;
    needs g1): g1 reaches the BatchNorm output through the dropout, as in bn_backward."""
    scale, shift, mean, rstd = state
    dev = scale.device
    d = _drop(drop) if drop is not None else None
    part, nch = None, 0
    if want_params:
        nch = stats_chunks(B, xv.H, xv.W)
        part = torch.empty((nch, C, 2), dtype=torch.float32, device=dev)
        dgamma = _out1(dgamma, C, dev)
        dbeta = _out1(dbeta, C, dev)
    else:
        dgamma = dbeta = None
    check(lib().stc_bn_bwd_frozen(L.dtype_code(dt), B, xv, C, ptr(scale), ptr(shift), ptr(mean), ptr(rstd),
                                  g1 if g1 is not None else L.NULL_VIEW, float(s1),
                                  g2 if g2 is not None else L.NULL_VIEW, float(s2),
                                  ctypes.byref(d) if d is not None else None, ptr(part), nch, dxv, ptr(dgamma),
                                  ptr(dbeta), stream()), "stc_bn_bwd_frozen")
    return dgamma, dbeta


def in_plan(B, H, W, C, dt):
    """(regime 0 tiny / 1 resident / 2 streamed, channels per slab, pixel chunks per sample, m) of stc_in_plan."""
    key = ("inp", B, H, W, C, dt)
    r = _MEMO.get(key)
    if r is None:
        out = (ctypes.c_int32 * 4)()
        check(lib().stc_in_plan(L.dtype_code(dt), B, H, W, C, out), "stc_in_plan")
        r = _MEMO[key] = tuple(out)
    return r


def _in_ws(B, xv, C, dt, dev):
    key = ("inw", B, xv.H, xv.W, C, dt)
    nbytes = _MEMO.get(key)
    if nbytes is None:
        nbytes = lib().stc_in_workspace(L.dtype_code(dt), B, xv.H, xv.W, C)
        check(0 if nbytes >= 0 else -1, "stc_in_workspace")
        _MEMO[key] = nbytes
    return _ws(nbytes, dev)


def in_forward(B, xv, C, dt, norm, apply_x, y1, s1, y2=None, s2=0.0):
    """Instance norm of x (statistics per sample and channel over xv's extent) + activation pass of ``apply_x``
    (xv or its top-left crop) into y1 [and y2]; ``norm``: the nn.InstanceNorm2d (eps; weight / bias when affine).
    Returns (mean, rstd), fp32 [B, C]."""
    dev = xv._keep.device
    mean = torch.empty((B, C), dtype=torch.float32, device=dev)
    rstd = torch.empty((B, C), dtype=torch.float32, device=dev)
    ws, nb = _in_ws(B, xv, C, dt, dev)
    check(lib().stc_in_fwd(L.dtype_code(dt), B, xv, C, ptr(norm.weight), ptr(norm.bias), float(norm.eps), ptr(mean),
                           ptr(rstd), apply_x, y1, float(s1), y2 if y2 is not None else L.NULL_VIEW, float(s2),
                           ptr(ws), nb, stream()), "stc_in_fwd")
    return mean, rstd


def in_backward(B, xv, C, dt, dxv, norm, stats, g1=None, s1=0.0, g2=None, s2=0.0, dgamma=None, dbeta=None):
    """Fused activation + instance-norm backward into dxv; ``stats`` = in_forward's (mean, rstd).  Returns
    (dgamma, dbeta), (None, None) for a norm without affine parameters."""
    dev = xv._keep.device
    mean, rstd = stats
    ws, nb = _in_ws(B, xv, C, dt, dev)
    if norm.weight is not None:
        dgamma = _out1(dgamma, C, dev)
        dbeta = _out1(dbeta, C, dev)
    else:
        dgamma = dbeta = None
    check(lib().stc_in_bwd(L.dtype_code(dt), B, xv, C, ptr(norm.weight), ptr(norm.bias), ptr(mean), ptr(rstd),
                           g1 if g1 is not None else L.NULL_VIEW, float(s1), g2 if g2 is not None else L.NULL_VIEW,
                           float(s2), dxv, ptr(dgamma), ptr(dbeta), ptr(ws), nb, stream()), "stc_in_bwd")
    return dgamma, dbeta


def chan_sum(B, xv, C, Cout, dt, device, out=None):
    nch = stats_chunks(B, xv.H, xv.W)
    part = torch.empty((nch, C), dtype=torch.float32, device=device)
    out = _out1(out, Cout, device)
    check(lib().stc_chan_sum(L.dtype_code(dt), B, xv, C, Cout, ptr(part), nch, ptr(out), stream()), "stc_chan_sum")
    return out


def tanh_bias_bwd(y, gy, dqv, dt, dbias=None):
    """dq = gy*(1-y^2) into the NHWC view dqv (padded channels zero); returns dbias [C] (into ``dbias``
    when given)."""
    B, C, H, W = y.shape
    nch = stats_chunks(B, H, W)
    part = torch.empty((nch, C), dtype=torch.float32, device=y.device)
    dbias = _out1(dbias, C, y.device)
    check(lib().stc_tanh_bias_bwd(L.dtype_code(dt), B, C, H, W, ptr(y), ptr(gy), dqv, ptr(dbias), ptr(part), nch,
                                  stream()), "stc_tanh_bias_bwd")
    return dbias


def head_bwd(y, gy, dqv, dt, act, dbias=None):
    """tanh_bias_bwd for any output head ``act`` (_lib.head_code): dq = gy * act'(q) from the stored output y into the NHWC
    view dqv (padded channels zero); returns dbias [C] (into ``dbias`` when given).  stc_head_bwd."""
    B, C, H, W = y.shape
    nch = stats_chunks(B, H, W)
    part = torch.empty((nch, C), dtype=torch.float32, device=y.device)
    dbias = _out1(dbias, C, y.device)
    check(lib().stc_head_bwd(L.dtype_code(dt), L.head_code(act), B, C, H, W, ptr(y), ptr(gy), dqv, ptr(dbias),
                             ptr(part), nch, stream()), "stc_head_bwd")
    return dbias


def gather(sources, dst, dt):
    """NCHW fp32 sources (channel concat) -> NHWC dst [B, H, W, Cpad] (extra channels zero)."""
    B, H, W, cpad = dst.shape
    n = len(sources)
    arr = (ctypes.c_void_p * n)(*[s.data_ptr() for s in sources])
    cs = (ctypes.c_int * n)(*[s.shape[1] for s in sources])
    check(lib().stc_gather_nchw(L.dtype_code(dt), B, H, W, n, arr, cs, L.nhwc_view(dst), cpad, stream()),
          "stc_gather_nchw")


def scatter(src_nhwc, dsts, chans, dt, H=None, W=None):
    """NHWC -> NCHW fp32 per channel range; dsts entries may be None (skipped)."""
    B, Ha, Wa, _ = src_nhwc.shape
    H = Ha if H is None else H
    W = Wa if W is None else W
    n = len(dsts)
    arr = (ctypes.c_void_p * n)(*[None if d is None else d.data_ptr() for d in dsts])
    cs = (ctypes.c_int * n)(*chans)
    check(lib().stc_scatter_nchw(L.dtype_code(dt), B, H, W, L.nhwc_view(src_nhwc, 0, H, W), n, arr, cs, stream()),
          "stc_scatter_nchw")


def infer_output(net_out, oh=192, ow=256):
    """STCGAN.infer output stage on the GPU (stc_infer_output): generator output [B, C, H, W] fp32
    (tanh range) -> uint8 [B, oh, ow, C] = float2uint(cv.resize(x*0.5+0.5, (ow, oh), INTER_LINEAR)),
    the arrays the reference hands to cv.imwrite (STCGAN/stcgan.py:355-377, utils.py:63-65)."""
    if not net_out.is_cuda:
        raise RuntimeError("stcgan_amd.infer_output: CUDA (HIP) tensors only")
    x = net_out.detach().float().contiguous()
    B, C, H, W = x.shape
    out = torch.empty((B, oh, ow, C), dtype=torch.uint8, device=x.device)
    check(lib().stc_infer_output(ptr(x), B, C, H, W, oh, ow, ptr(out), stream()), "stc_infer_output")
    return out


def grad_accumulate(pairs):
    """dst += src (fp32, contiguous, same numel) for every (dst, src) in pairs: one launch per 16."""
    for k in range(0, len(pairs), 16):
        chunk = pairs[k:k + 16]
        for d, s in chunk:
            assert d.dtype == torch.float32 and s.dtype == torch.float32 and d.is_contiguous() \
                and s.is_contiguous() and d.numel() == s.numel(), "grad_accumulate: fp32 contiguous pairs"
        n = len(chunk)
        dst = (ctypes.c_void_p * n)(*[d.data_ptr() for d, _ in chunk])
        src = (ctypes.c_void_p * n)(*[s.data_ptr() for _, s in chunk])
        num = (ctypes.c_int64 * n)(*[d.numel() for d, _ in chunk])
        check(lib().stc_grad_accumulate(n, dst, src, num, stream()), "stc_grad_accumulate")


# ---- VisualLoss: vgg19_bn features in bf16 (stc_conv3_* / stc_maxpool2_* / stc_vgg_norm_* / stc_feat_mse_*) ----
def _view(t):
    """An NHWC bf16 tensor [B, H, W, C] or a ready View."""
    return t if isinstance(t, L.View) else L.nhwc_view(t)


def conv3_plan(B, H, W, cin, cout):
    """stc_conv3_plan: (path, TH, TW, BN, K chunk, K splits, M tiles, N tiles)."""
    key = ("c3plan", B, H, W, cin, cout)
    v = _MEMO.get(key)
    if v is None:
        out = (ctypes.c_int32 * 8)()
        check(lib().stc_conv3_plan(B, H, W, cin, cout, out), "stc_conv3_plan")
        v = _MEMO[key] = tuple(out)
    return v


def pack_conv3(weights, want_dgrad=True):
    """fp32 [Co, Ci, 3, 3] weights -> [(fwd bf16 [Co_pad, 9, Ci_pad], dgrad bf16 [Ci_pad, 9, Co_pad] or None)], channel
    counts padded to multiples of 8; one stc_conv3_pack launch per 16 layers."""
    out = []
    for k in range(0, len(weights), L.CONV3_PACK_MAX):
        chunk = [w.detach().float().contiguous() for w in weights[k:k + L.CONV3_PACK_MAX]]
        descs = (L.Conv3PackDesc * len(chunk))()
        for d, w in zip(descs, chunk):
            if w.dim() != 4 or tuple(w.shape[2:]) != (3, 3) or not w.is_cuda:
                raise ValueError(f"pack_conv3: a CUDA [Co, Ci, 3, 3] weight is required, got {tuple(w.shape)}")
            co, ci = w.shape[:2]
            cop, cip = -(-co // 8) * 8, -(-ci // 8) * 8
            f = torch.empty((cop, 9, cip), dtype=torch.bfloat16, device=w.device)
            g = torch.empty((cip, 9, cop), dtype=torch.bfloat16, device=w.device) if want_dgrad else None
            d.W, d.fwd, d.dgrad = w.data_ptr(), f.data_ptr(), g.data_ptr() if g is not None else None
            d.Co, d.Ci, d.Co_pad, d.Ci_pad = co, ci, cop, cip
            out.append((f, g))
        check(lib().stc_conv3_pack(len(chunk), descs, stream()), "stc_conv3_pack")
    return out


def conv3(x, w_packed, y, bias=None, relu=True, mask=None, B=None):
    """stc_conv3_fwd: y = act(conv3x3(x, w_packed) + bias) [* (mask > 0)]; x, y, mask: NHWC bf16 tensors or Views
    (then with B); w_packed: bf16 [Cout, 9, Cin]."""
    xv, yv = _view(x), _view(y)
    if B is None:
        B = x.shape[0]
    cout, _, cin = w_packed.shape
    check(lib().stc_conv3_fwd(B, xv, cin, ptr(w_packed), cout, yv, ptr(bias), 1 if relu else 0,
                              _view(mask) if mask is not None else L.NULL_VIEW, stream()), "stc_conv3_fwd")
    return y


def maxpool2(x, y=None):
    """MaxPool2d(2, 2) of an NHWC bf16 tensor."""
    B, H, W, C = x.shape
    if y is None:
        y = torch.empty((B, H // 2, W // 2, C), dtype=x.dtype, device=x.device)
    check(lib().stc_maxpool2_fwd(B, L.nhwc_view(x), C, L.nhwc_view(y), stream()), "stc_maxpool2_fwd")
    return y


def maxpool2_backward(x, gy, gx=None):
    """The gradient of maxpool2 at its input x (first maximal element of a window, torch's rule)."""
    B, H, W, C = x.shape
    if gx is None:
        gx = torch.empty_like(x)
    check(lib().stc_maxpool2_bwd(B, L.nhwc_view(x), C, L.nhwc_view(gy), L.nhwc_view(gx), stream()), "stc_maxpool2_bwd")
    return gx


def vgg_normalise(src, dst):
    """((src * 0.5 + 0.5) - mean) / std of an fp32 [B, 3, H, W] tensor of any strides into the NHWC bf16 [B, H, W, 8]
    tensor dst (channels 3..7 zero)."""
    B, C, H, W = src.shape
    if C != 3 or src.dtype != torch.float32:
        raise ValueError(f"vgg_normalise: an fp32 [B, 3, H, W] tensor is required, got {tuple(src.shape)} {src.dtype}")
    sb, sc, sh, sw = src.stride()
    check(lib().stc_vgg_norm_fwd(B, H, W, ptr(src), sb, sc, sh, sw, L.nhwc_view(dst), stream()), "stc_vgg_norm_fwd")
    return dst


def vgg_normalise_backward(g):
    """NHWC bf16 [B, H, W, 8] gradient of the normalised input -> contiguous fp32 [B, 3, H, W], times 0.5 / std."""
    B, H, W, _ = g.shape
    out = torch.empty((B, 3, H, W), dtype=torch.float32, device=g.device)
    check(lib().stc_vgg_norm_bwd(B, H, W, L.nhwc_view(g), ptr(out), stream()), "stc_vgg_norm_bwd")
    return out


def feature_mse(fp, ft):
    """mean((fp - ft)^2) of two dense bf16 tensors as a 0-dim fp32 tensor (deterministic two-level sum)."""
    assert fp.is_contiguous() and ft.is_contiguous() and fp.shape == ft.shape and fp.dtype == torch.bfloat16
    n = fp.numel()
    part = torch.empty(max(1, lib().stc_feat_mse_parts(n)), dtype=torch.float32, device=fp.device)
    out = torch.empty((), dtype=torch.float32, device=fp.device)
    check(lib().stc_feat_mse_fwd(ptr(fp), ptr(ft), n, ptr(part), ptr(out), stream()), "stc_feat_mse_fwd")
    return out


def feature_mse_backward(fp, ft, gout, relu_mask=False):
    """bf16(gout * 2 (fp - ft) / n) [* (fp > 0)]; gout: fp32 device scalar."""
    assert fp.is_contiguous() and ft.is_contiguous() and fp.shape == ft.shape and fp.dtype == torch.bfloat16
    g = torch.empty_like(fp)
    check(lib().stc_feat_mse_bwd(ptr(fp), ptr(ft), fp.numel(), ptr(gout), 1 if relu_mask else 0, ptr(g), stream()),
          "stc_feat_mse_bwd")
    return g
