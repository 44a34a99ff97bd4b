"""Whole-network forward/backward orchestration over the HIP kernels.

Each network call is ONE autograd node (NetFn): the forward enqueues the layer
kernels in order; the backward is written out by hand in reverse layer order,
with BatchNorm backward fused with the activation backward of every consumer.
Nothing here computes on the CPU.

Activations are materialised once per element by ``stc_bn_apply`` (BN-apply +
LeakyReLU / ReLU), so every GEMM and weight-gradient kernel stages plain operands:
in an implicit GEMM each input element is re-read by 4-16 taps per N tile, so a
fused load-time transform would be paid 4-16x over.

Generator layout (STCGAN/networks.py:79-143, pad/crop of
src/models/stcgan_g.py:120-132), L = num_downs levels, co[k] = conv_k output
channels, S[k] the block-k input resolution (S[1] = S[0]//2, S[k+1] = ceil(S[k]/2)):
  rd[k]  raw conv_k output r_k                    (res S[k+1])
  ad[k]  LeakyReLU(BN_d(r_k)) -> input of conv_{k+1}
         (the in-place LeakyReLU of networks.py:106 -- also the skip half)
  rq[k]  raw convT_k output q_k                   (res 2*S[k+1] = padded S[k])
  cr[k]  [ ReLU(BN_d(r_k)) | ReLU(BN_u(q_{k+1})) ] -> input of convT_k
         (networks.py:108,143: ReLU of the concat; ReLU(LeakyReLU(v)) = ReLU(v))
         use_dropout, train mode, the levels right above the innermost one: ReLU(BN_u(q_{k+1}) * keep/(1-p)), the
         mask a counter-based function of logical indices (GenPlan.drop, ops.dropout_next)
  y = head(convT_0(cr[0]) + bias), written NCHW fp32; head = tanh unless get_generator(activation=...) says otherwise.

norm_layer=nn.InstanceNorm2d (GenPlan.inorm / DiscPlan.inorm): the same buffers, with every
"BN" above an instance norm -- a normed layer is the plain conv, then one instance-norm forward (statistics per sample
over the stored raw output + the activation pass); its backward the input-gradient conv, then one instance-norm
backward.  The BatchNorm path takes none of these calls.

BatchNorm layers on their running statistics (eval mode, or norm children frozen under a train-mode network;
DESIGN.md section 8e): conv, the eval table (+ rstd_run when a backward follows) and the apply pass forward; backward
the input-gradient conv, then one frozen-statistics backward (one pass; the sums only where parameter gradients are
wanted).

nn.SyncBatchNorm layers with more than one data-parallel rank: the BatchNorm forms split where
the statistics are merged, with one small all-gather of per-channel records there -- per normed layer one in the
forward and one in the backward, issued in the same host order on every rank.

Every place where a conv meets a norm layer goes through two functions, whatever the norm and its mode (_IN, _BATCH,
_RUNNING, _SYNC): _conv_norm_act forward and _conv_act_norm_backward backward, which name the library calls of each form.
The latter is also the one place where a conv's weight is released to the optimiser (GradWriter.done) after its last
read.
"""
import typing

import torch

from . import _lib as L
from . import ops
from . import parallel
from .ops import LRELU

# ----------------------------------------------------------------------------- tracing (tests)
# TRACE: None, or a dict that collects, per network call, the forward's saved buffers and the backward's
# per-level gradient tensors (tests/test_gpu_c3_layers.py checks every layer against torch on those).
TRACE = None


def _trace(kind, key, t):
    if TRACE is not None:
        TRACE.setdefault(kind, [{}])[-1][key] = t


def _trace_new(kind):
    if TRACE is not None:
        TRACE.setdefault(kind, []).append({})


# ----------------------------------------------------------------------------- weight-gradient lane
# The weight gradients of a backward hang off its input-gradient chain (each needs that layer's incoming
# gradient and saved input; nothing on the chain needs them), so they run on a side stream per calling
# stream and overlap the rest of the chain -- most of the deep (1x1-8x8) layers' kernels are latency-bound
# small grids.  Joined before the backward returns its gradients.
WGRAD_OVERLAP = True
# interleaved A/B (scripts/train_steps.py --ab): round 2: none 13.74, <= 32x32 13.45, <= 64x64 13.64, all 13.75
# ms/step; round 6 (the D-step backward of each discriminator call right after its forward,
# profiles/r06/wgrad_lane/): <= 32x32 10.57, <= 64x64 10.47, all 10.52 ms/step
WGRAD_OVERLAP_MAX_PIX = 64 * 64
_WG_SIDE = {}
# streams (raw handles) whose backward keeps its weight gradients on the stream itself while a HIP graph
# is being captured: the discriminator lanes (STCGAN.capture).  A weight-gradient side stream forked from a
# lane, itself forked from the capturing stream, made the capture's end fault on this ROCm (round-3 probe:
# scripts/graph_capture_probe.py -- lanes alone and side streams of the main stream alone capture fine).
NO_SIDE_IN_CAPTURE = set()
# True: STCGAN.capture keeps the lanes' weight-gradient side streams too (probe switch only: hipStreamEndCapture
# segfaults on this ROCm with them, also when they first fork from the capturing stream and every fork has its own
# event -- profiles/r05/graph_ab/late/)
SIDE_IN_CAPTURE = False


_set_stream = torch._C._cuda_setStream


def _stream_wait(waiter_h, src_h):
    """Stream ``waiter_h`` waits for what is queued on ``src_h`` (raw handles), through one library call
    (stc_stream_wait: a pooled event that outlives an open capture)."""
    L.check(L.lib().stc_stream_wait(waiter_h, src_h), "stc_stream_wait")

# Events recorded or waited on while a HIP graph is being captured, kept alive until the capture has ended
# (STCGAN.capture sets a list here and drops it after capture_end).  torch's Stream.wait_stream and a fork's local
# event are otherwise destroyed inside the open capture, while capture edges still refer to them: the first suspect
# of the hipStreamEndCapture fault with the lanes' weight-gradient side streams (profiles/r05/graph_ab/late/).
CAPTURE_EVENTS = None


def hold(ev):
    """ev, kept alive until the open capture ends (no-op outside a capture)."""
    if CAPTURE_EVENTS is not None:
        CAPTURE_EVENTS.append(ev)
    return ev


def wait_stream(waiter, src):
    """waiter.wait_stream(src), as _stream_wait."""
    _stream_wait(waiter.cuda_stream, src.cuda_stream)


class _WgradLane:
    def __init__(self):
        self.cur = torch.cuda.current_stream() if WGRAD_OVERLAP else None
        self.side = None
        self.last_side = False
        if (self.cur is not None and self.cur.cuda_stream in NO_SIDE_IN_CAPTURE
                and torch.cuda.is_current_stream_capturing()):
            self.cur = None
        if self.cur is not None:
            ent = _WG_SIDE.get(self.cur.cuda_stream)
            if ent is None:
                side = torch.cuda.Stream(self.cur.device)
                ent = _WG_SIDE[self.cur.cuda_stream] = (side, side.cuda_stream, self.cur.cuda_stream)
            self.side, self._side_h, self._cur_h = ent

    def run(self, fn, *reads, pixels=0):
        """fn() on the side stream, after everything queued so far on the calling stream; ``reads``: the
        calling stream's tensors fn reads that may be freed before the backward ends.  Only layers of at
        most WGRAD_OVERLAP_MAX_PIX output pixels per image go to the side (the big ones fill the GPU alone;
        overlapping them measured slower).  (The fork is one library call on raw stream handles (stc_stream_wait, a
        pooled event) and a direct current-stream switch: ``Stream.wait_stream`` creates an event per call and
        ``torch.cuda.stream()`` queries the current stream twice -- together ~15 us of host time per call, 50 calls
        per step.)"""
        if self.side is None or pixels > WGRAD_OVERLAP_MAX_PIX:
            self.last_side = False
            return fn()
        self.last_side = True
        side, cur = self.side, self.cur
        _stream_wait(self._side_h, self._cur_h)
        for t in reads:
            t.record_stream(side)
        _set_stream(side.stream_id, side.device_index, side.device_type)
        try:
            return fn()
        finally:
            _set_stream(cur.stream_id, cur.device_index, cur.device_type)

    def join(self):
        if self.side is not None:
            _stream_wait(self._cur_h, self._side_h)


class GradWriter:
    """Where one backward writes its network's parameter gradients: the network's flat gradient buffer
    (parallel.FlatGrads; each ``p.grad`` is a view of it), so no gradient is allocated, copied into an
    exchange buffer or accumulated by autograd.  torch's accumulation semantics are kept: a parameter
    whose ``.grad`` is None (the optimiser's zero_grad) gets its view and the kernels write it in place; a
    parameter that already holds a gradient (the discriminator's real and fake calls inside one graph,
    STCGAN/stcgan.py:219-227) gets a scratch result that ``flush`` adds to it (one multi-tensor launch),
    old + new in that order.  With data parallelism the network's BucketExchange is told as each layer's
    gradients are enqueued (``done``), so its buckets are all-reduced while the backward continues."""

    def __init__(self, net):
        from .parallel import exchange_of, flat_grads
        self.flat = flat_grads(net)
        self.exchange = exchange_of(net)
        self.acc = []
        self._acc_ids = set()

    def dest(self, p):
        g = p.grad
        if g is None:
            p.grad = self.flat.view(p)
            return p.grad
        if not self.flat.owns(g, p):
            # a gradient that is not this network's flat-buffer view (assigned by the caller, or carried along by
            # a module move): moved into the view, so that the exchange averages what the optimiser reads
            v = self.flat.view(p)
            v.copy_(g)
            p.grad = g = v
        s = torch.empty(p.shape, dtype=torch.float32, device=p.device)
        self.acc.append((g, s, p))
        self._acc_ids.add(id(p))
        return s

    def done(self, params, lane=None):
        """Gradients of ``params`` enqueued (on the lane's side stream when its last job went there)."""
        if self.exchange is None:
            return
        fresh = [p for p in params if id(p) not in self._acc_ids]
        if fresh:
            side = lane.side if (lane is not None and lane.last_side) else None
            self.exchange.ready(fresh, side)

    def flush(self):
        if self.acc:
            ops.grad_accumulate([(g, s) for g, s, _ in self.acc])
            if self.exchange is not None:
                self.exchange.ready([p for _, _, p in self.acc])
            self.acc, self._acc_ids = [], set()


_ONES = {}


def _ones_plane(B, H, W, dev):
    """A persistent [B, 1, H, W] fp32 plane of ones (filled once, synchronously: streams share it)."""
    key = (B, H, W, str(dev))
    t = _ONES.get(key)
    if t is None:
        t = _ONES[key] = torch.ones((B, 1, H, W), dtype=torch.float32, device=dev)
        torch.cuda.current_stream(dev).synchronize()
    return t


def _nhwc(B, H, W, C, dt, dev, zero=False):
    f = torch.zeros if zero else torch.empty
    return f((B, H, W, C), dtype=dt, device=dev)


class GenPlan:
    """Static structure of a UnetGenerator module (parameters by role)."""

    def __init__(self, net):
        self.net = net
        outer = net.model  # outermost UnetSkipConnectionBlock
        self.in_c = outer.model[0].in_channels
        conv, bnd, convT, bnu, drop = [], {}, {}, {}, {}
        names = {id(m): n for n, m in net.named_modules()}
        kinds = {}  # {level: the up layer is a resize-convolution}

        def up(k, m):
            convT[k], kinds[k] = _up_layer(m, names.get(id(m), "?"))

        conv.append(outer.model[0])
        up(0, outer.model[3])
        self.out_c = convT[0].out_channels
        # the output head ("none", "tanh", "sigmoid", "htanh"): read from the module after the outermost up layer, as
        # dropout's p is read -- it selects the ConvT epilogue and the first backward kernel
        self.head = _head_of(outer.model, names.get(id(outer), "model"))
        blk = outer.model[1]
        k = 1
        while True:
            seq = blk.model
            conv.append(seq[1])
            if blk.innermost:
                up(k, seq[3])
                bnu[k] = seq[4]
                break
            bnd[k] = seq[2]
            up(k, seq[5])
            bnu[k] = seq[6]
            if isinstance(seq[-1], torch.nn.Dropout):  # use_dropout: after the up-norm (networks.py)
                p = seq[-1].p
                if not 0.0 <= p < 1.0:
                    raise ValueError(f"stcgan_amd: dropout probability must satisfy 0 <= p < 1, got {p!r}")
                if p > 0.0:  # (p = 0 keeps everything and, as torch's dropout, draws nothing: the plain path)
                    drop[k] = float(p)
            blk = seq[3]
            k += 1
        self.L = len(conv)
        # up layers: nn.ConvTranspose2d(4, 2, 1) (weight [Ci][Co][4][4]), or -- every one of them, no_conv_t -- the
        # nn.Conv2d(3, 1, 1) of an Upsample + Conv2d pair (weight [Co][Ci][3][3]), run as the ConvT it equals
        if len(set(kinds.values())) > 1:
            raise NotImplementedError(
                "stcgan_amd: a generator mixing ConvTranspose2d and Upsample + Conv2d up layers is not supported -- "
                "resize-convolution: " + ", ".join(names.get(id(convT[j]), "?") for j in sorted(kinds) if kinds[j])
                + "; ConvTranspose2d: " + ", ".join(names.get(id(convT[j]), "?") for j in sorted(kinds) if not kinds[j]))
        self.upconv = kinds[0]
        self.pack_t_fwd = L.PACK_UPCONV_FWD if self.upconv else L.PACK_CONVT_FWD
        self.pack_t_dgrad = L.PACK_UPCONV_DGRAD if self.upconv else L.PACK_CONVT_DGRAD
        self.conv, self.bnd, self.convT, self.bnu = conv, bnd, convT, bnu
        # {level k: p}: train-mode dropout on the output of BN_up[k] (the blocks right above the innermost one)
        self.drop = drop
        self.co = [c.out_channels for c in conv]
        # the padding mode of each down conv (L.PAD_ZEROS / L.PAD_REFLECT), read from the module as torch would run it:
        # a reflect layer takes the reflect kernels and the unfused step forms
        self.conv_names = [names.get(id(c), "?") for c in conv]
        self.pad = [_pad_of(c, n) for c, n in zip(conv, self.conv_names)]
        # which norm the network uses: BatchNorm2d, or InstanceNorm2d (affine or not)
        self.inorm, self.affine = _norm_kind(list(bnd.values()) + list(bnu.values()))
        self.sync, self.norm_names = _sync_kind(list(bnd.values()) + list(bnu.values()), names)
        self.params = list(net.parameters())


def _head_of(seq, name):
    """The output head of the outermost block's Sequential [downconv, submodule, uprelu, upconv, <activation>]: nothing
    after the up layer is "none"; nn.Tanh, nn.Sigmoid and nn.Hardtanh(-1, 1) are the other three.  Any other module
    there (swapped in by hand) raises NotImplementedError naming its path."""
    nn = torch.nn
    if len(seq) == 4:
        return "none"
    m = seq[4] if len(seq) == 5 else None
    if type(m) is nn.Tanh:
        return "tanh"
    if type(m) is nn.Sigmoid:
        return "sigmoid"
    if type(m) is nn.Hardtanh and m.min_val == -1.0 and m.max_val == 1.0:
        return "htanh"
    where = f"{name}.model.4" if m is not None else f"{name}.model ({len(seq)} modules)"
    what = repr(m) if m is not None else "more than one module after the up layer"
    raise NotImplementedError(f"stcgan_amd: output activation {where}: {what} is not supported -- nothing (none), "
                              "nn.Tanh, nn.Sigmoid or nn.Hardtanh(-1.0, 1.0)")


def _pad_of(conv, name):
    """L.PAD_ZEROS / L.PAD_REFLECT of a 4x4 nn.Conv2d; "replicate" and "circular" have no kernel."""
    if conv.padding_mode not in L.PADS:
        raise NotImplementedError(f"stcgan_amd: conv layer {name}: padding_mode={conv.padding_mode!r} is not supported "
                                  "('zeros' or 'reflect')")
    return L.PADS[conv.padding_mode]


def _check_reflect_plane(name, B, C, h, w):
    """torch's refusal of a reflect pad as wide as the plane (ReflectionPad2d), before any launch."""
    if h < 2 or w < 2:
        raise RuntimeError(f"stcgan_amd: conv layer {name} (padding_mode='reflect'): Padding size should be less than "
                           f"the corresponding input dimension, but got: padding (1, 1) of input [{B}, {C}, {h}, {w}]")


def _up_layer(m, name):
    """(the module that holds an up layer's weight and bias, is it a resize-convolution): m is the reference's
    nn.ConvTranspose2d, or nn.Sequential(nn.Upsample(2, "nearest"), nn.Conv2d(3, 1, 1, padding_mode="zeros")), which
    the ConvT kernels run; any other form of the pair raises NotImplementedError."""
    nn = torch.nn
    if isinstance(m, nn.ConvTranspose2d):
        return m, False
    if not (isinstance(m, nn.Sequential) and len(m) == 2 and isinstance(m[0], nn.Upsample)
            and isinstance(m[1], nn.Conv2d)):
        raise NotImplementedError(f"stcgan_amd: up layer {name} ({type(m).__name__}) is neither a ConvTranspose2d nor "
                                  "nn.Sequential(nn.Upsample, nn.Conv2d)")
    u, c = m
    sf = u.scale_factor
    sf = tuple(sf) if isinstance(sf, (tuple, list)) else (sf, sf)
    if u.mode != "nearest" or u.size is not None or sf != (2, 2):
        raise NotImplementedError(f"stcgan_amd: up layer {name}: nn.Upsample(scale_factor=2, mode='nearest') only, got "
                                  f"scale_factor={u.scale_factor!r}, size={u.size!r}, mode={u.mode!r}")
    if c.padding_mode != "zeros":
        raise NotImplementedError(f"stcgan_amd: up layer {name}: padding_mode={c.padding_mode!r} is not supported "
                                  "(the conv kernels' halo is zero-filled: padding_mode='zeros' only)")
    if (tuple(c.kernel_size), tuple(c.stride), c.padding, tuple(c.dilation), c.groups) != \
            ((3, 3), (1, 1), (1, 1), (1, 1), 1):
        raise NotImplementedError(f"stcgan_amd: up layer {name}: nn.Conv2d(kernel_size=3, stride=1, padding=1) only, "
                                  f"got {c}")
    return c, True


def _sizes(H, W, Lv):
    S = [(H, W), (H // 2, W // 2)]
    for _ in range(2, Lv + 1):
        h, w = S[-1]
        S.append(((h + 1) // 2, (w + 1) // 2))
    return S


def _pad2(S, k):
    """Padded size of resolution level k: 2 * S[k+1] (the extent a ConvT from level k+1 produces)."""
    return (2 * S[k + 1][0], 2 * S[k + 1][1])


def _norm_kind(norms):
    """(instance norm?, affine?) of a network's norm modules (networks.py admits one kind per network)."""
    inorm = any(isinstance(m, torch.nn.InstanceNorm2d) for m in norms)
    assert not inorm or all(type(m) is torch.nn.InstanceNorm2d for m in norms)
    return inorm, inorm and any(m.weight is not None for m in norms)


def _sync_kind(norms, names):
    """(nn.SyncBatchNorm layers?, {id(norm): its module name}) of a network's norm modules; a SyncBatchNorm bound
    to a process group of its own is refused (the records travel over the default group)."""
    sync = [m for m in norms if isinstance(m, torch.nn.SyncBatchNorm)]
    assert not sync or len(sync) == len(norms)
    for m in sync:
        if m.process_group is not None:
            raise NotImplementedError(f"stcgan_amd: nn.SyncBatchNorm layer {names.get(id(m), '?')} has a process_group "
                                      "of its own: only the default process group is supported")
    return bool(sync), {id(m): names.get(id(m), "?") for m in norms}


def _check_plane(B, C, h, w):
    """torch's refusal of an instance norm over one spatial element (train and eval alike), before any launch."""
    if h * w <= 1:
        raise ValueError(f"Expected more than 1 spatial element when training, got input size "
                         f"torch.Size([{B}, {C}, {h}, {w}])")


# ----------------------------------------------------------------------------- the normed-layer step
# How the norm layers of one network call normalise: instance norm (one mode); BatchNorm on batch statistics;
# BatchNorm on its running statistics (eval mode, or frozen under a train-mode network); nn.SyncBatchNorm layers on
# the batch statistics of all data-parallel ranks (only with a process group of more than one rank: else _BATCH, the
# very same launches as nn.BatchNorm2d's).
_IN, _BATCH, _RUNNING, _SYNC = 0, 1, 2, 3


def _norm_mode(plan, batch_stats):
    if plan.inorm:
        return _IN
    if not batch_stats:
        return _RUNNING
    return _SYNC if (plan.sync and parallel.world() > 1) else _BATCH


class _Sync:
    """What the _SYNC layers of one network call share: the global batch size (the ranks' local batches may differ)
    and the call's list of collectives, [(norm layer, "forward" / "backward")] in host order, appended to
    ``net.sync_log`` when that is a list -- every rank must issue the same sequence (tests compare the lists)."""

    def __init__(self, plan, B, dev):
        self.Bg = parallel.global_batch(B, dev)
        self.names = plan.norm_names
        self.calls = []
        log = getattr(plan.net, "sync_log", None)
        if log is not None:
            log.append(self.calls)

    def count(self, xv):
        """Pixels per channel of the global batch over xv's extent (the same on every rank)."""
        return self.Bg * xv.H * xv.W

    def gather(self, norm, direction):
        def run(rec):
            self.calls.append((self.names[id(norm)], direction))
            return parallel.gather_records(rec)
        return run


def _conv_norm_act(kind, B, xv, cin, w, cout, yv, dt, norm, mode, apply_x, y1, s1, y2, s2, drop, defer, keep,
                   sync=None, pad=L.PAD_ZEROS):
    """Conv into ``yv`` -> norm layer ``norm`` -> activation pass of ``apply_x`` (yv or its top-left crop) into y1 [and
    y2] (y1 None: no pass).  Returns ((2, cout) scale / shift table or None, (mean, rstd) or None).
    _BATCH: one library call, the statistics out of the conv itself; ``defer`` (a list): the running statistics are not
    updated, the update's inputs are appended (bn_running_update).  _RUNNING: conv, the table from the running
    statistics, the apply pass; ``keep`` (a backward will follow): (running_mean, rstd_run) beside the table.  _IN:
    conv, then the statistics of the stored raw output with the pass; no table.  ``drop``: a dropout level between a
    BatchNorm and the activation (dropout_next).  _SYNC (``sync``: the call's _Sync): the split form of _BATCH with
    one gather of the ranks' records between the partials and the table; ``defer`` gets the gathered records.
    pad=L.PAD_REFLECT: the same forms around the reflect conv; _BATCH then takes its three separate calls (the
    statistics from a pass over the stored output)."""
    if mode == _SYNC:
        return ops.conv_bn_act_sync(kind, B, xv, cin, w, cout, yv, dt, norm, apply_x, y1, s1, y2, s2, defer, drop,
                                    sync.gather(norm, "forward"), pad)
    if mode == _BATCH:
        return ops.conv_bn_act(kind, B, xv, cin, w, cout, yv, dt, norm, apply_x, y1, s1, y2, s2, defer, drop, pad)
    ops.conv(kind, B, xv, cin, w, cout, yv, dt, pad=pad)
    if mode == _IN:
        return None, ops.in_forward(B, yv, cout, dt, norm, apply_x, y1, s1, y2, s2)
    t = torch.empty((2, cout), dtype=torch.float32, device=w.device)
    ops.bn_eval_table(cout, norm, t[0], t[1])
    st = (norm.running_mean, ops.bn_running_rstd(cout, norm)) if keep else None
    if y1 is not None:
        ops.bn_apply(B, apply_x, cout, dt, (t[0], t[1]), y1, s1, y2, s2, drop)
    return t, st


def _conv_act_norm_backward(kind, B, gv, cg, wd, cin, gt, yv, dt, norm, mode, tab, st, xv, C, s_self, g_other, s_other,
                            ch_off, dxv, drop, own, W, lane, sync=None, pad=L.PAD_ZEROS):
    """The backward of one layer boundary: the input-gradient conv (kind, gv with cg channels, packed weight wd, cin
    output channels) into the view ``yv`` of tensor ``gt``, then the backward of the activation(s) and of the norm
    layer ``norm`` (None: none) that produced the conv's input, into ``dxv``.  xv: the norm's input (C channels),
    (tab, st) what _conv_norm_act returned for it.  The norm's output fed this conv through an activation of slope
    s_self and, where ``g_other`` is given, another consumer through one of slope s_other.  The conv's own gradient as
    the norm sees it is ``gt`` at channel ch_off over xv's extent.

    ``own``: the conv's parameters; W.done(own, lane) right after the last read of the weight: from there the
    optimiser may update it and, under data parallelism, the exchange may start on its gradient.  Then the norm's own.

    norm None              the activation backward in the conv epilogue where there is one, else conv + bn_backward
    _IN                    conv, in_backward
    _RUNNING               conv, bn_backward_frozen (through ``drop`` where there is one)
    _BATCH with ``drop``   conv, bn_backward (the GEMM epilogues know nothing of the mask)
    _BATCH                 the BatchNorm reduction fused into the conv (conv_bn_backward)
    _SYNC                  as _BATCH, in the split forms with one gather of the ranks' sums before the apply
    pad=L.PAD_REFLECT (the conv whose input gradient this is pads by reflection): the reflect input gradient -- frame
    and fold -- and always the unfused forms: a fused epilogue would form its sums before the fold."""
    if norm is None:
        # (no epilogue form under TRACE, which wants the conv's own output, or where the conv writes a larger extent
        # than the activation's: an odd generator level)
        if (TRACE is None and pad == L.PAD_ZEROS and yv.H == xv.H and yv.W == xv.W
                and ops.conv_act_backward(kind, B, gv, cg, wd, cin, dxv, dt, xv, s_self, g_other, s_other)):
            if W is not None:
                W.done(own, lane)
            return
        fused = False
    else:
        fused = mode in (_BATCH, _SYNC) and drop is None and pad == L.PAD_ZEROS
    if not fused:
        ops.conv(kind, B, gv, cg, wd, cin, yv, dt, pad=pad)
        if W is not None and norm is not None:
            W.done(own, lane)
        # the kernels form g1 * act1' + g2 * act2' in this order: another consumer's gradient first
        g1, s1, g2, s2 = L.nhwc_view(gt, ch_off, xv.H, xv.W), s_self, None, 0.0
        if g_other is not None:
            g1, s1, g2, s2 = g_other, s_other, g1, s1
        if norm is None:
            ops.bn_backward(B, xv, C, dt, dxv, g1, s1, g2, s2)
            if W is not None:
                W.done(own, lane)
            return
    # where the affine parameters' gradients go: nowhere when they are not wanted or the norm has none
    dgamma = dbeta = None
    if W is not None and norm.weight is not None:
        dgamma, dbeta = W.dest(norm.weight), W.dest(norm.bias)
    if fused and mode == _SYNC:
        ops.conv_bn_backward_sync(kind, B, gv, cg, wd, cin, yv, dt, xv, C, (tab[0], tab[1], st[0], st[1]), norm.weight,
                                  s_self, ch_off, g_other, s_other, dxv, dgamma, dbeta, sync.count(xv),
                                  sync.gather(norm, "backward"))
        if W is not None:
            W.done(own, lane)
    elif fused:
        ops.conv_bn_backward(kind, B, gv, cg, wd, cin, yv, dt, xv, C, (tab[0], tab[1], st[0], st[1]), norm.weight,
                             s_self, ch_off, g_other, s_other, dxv, dgamma, dbeta)
        if W is not None:
            W.done(own, lane)
    elif mode == _IN:
        ops.in_backward(B, xv, C, dt, dxv, norm, st, g1, s1, g2, s2, dgamma, dbeta)
    elif mode == _RUNNING:
        ops.bn_backward_frozen(B, xv, C, dt, dxv, g1, s1, g2, s2, (tab[0], tab[1], st[0], st[1]), dgamma, dbeta,
                               W is not None, drop)
    elif mode == _SYNC:
        ops.bn_backward_sync(B, xv, C, dt, dxv, g1, s1, g2, s2, (tab[0], tab[1], st[0], st[1], norm.weight), dgamma,
                             dbeta, drop, sync.count(xv), sync.gather(norm, "backward"))
    else:
        ops.bn_backward(B, xv, C, dt, dxv, g1, s1, g2, s2, (tab[0], tab[1], st[0], st[1], norm.weight), dgamma, dbeta,
                        drop)
    if dgamma is not None:
        W.done([norm.weight, norm.bias])


def _input_grads(B, gv, cg, weight, saved, hw, need_src, dt, cache, dev, pad=L.PAD_ZEROS):
    """The tail of a backward: the first layer's input-gradient conv (gradient view gv, cg channels) into a padded
    NHWC tensor, scattered into one NCHW fp32 gradient per source that needs one (None for the others)."""
    cin_pad = saved["cin_pad"]
    wd = ops.packed(cache, weight, L.PACK_CONV_DGRAD, cin_pad, cg, dt)
    # (zeros: the ConvT geometry writes 2 * gv.H rows; reflect: the fold writes the input's own extent, odd or even)
    gx = _nhwc(B, *(hw if pad != L.PAD_ZEROS else (2 * gv.H, 2 * gv.W)), cin_pad, dt, dev)
    ops.conv(L.CONVT_S2, B, gv, cg, wd, cin_pad, L.nhwc_view(gx), dt, pad=pad)
    H, W_ = hw
    # only the sources that need a gradient; the scatter writes every element of those
    src_grads = [torch.empty((B, c, H, W_), dtype=torch.float32, device=dev) if nd else None
                 for c, nd in zip(saved["src_c"], need_src)]
    ops.scatter(gx, src_grads, saved["src_c"], dt, H, W_)
    return src_grads


# ----------------------------------------------------------------------------- generator


def gen_forward(plan, sources, train, dt, cache, save, batch_stats=None):
    """train: dropout levels active (the network's own mode).  batch_stats (None: as train): the BatchNorm layers
    use batch statistics and update their running ones; False: running statistics, buffers untouched (frozen)."""
    if batch_stats is None:
        batch_stats = train
    dev = sources[0].device
    B, _, H, W = sources[0].shape
    Lv, co = plan.L, plan.co
    S = _sizes(H, W, Lv)
    assert S[Lv][0] >= 1 and S[Lv][1] >= 1, "input too small for the generator depth"
    cin = sum(s.shape[1] for s in sources)
    assert cin == plan.in_c, f"generator expects {plan.in_c} input channels, got {cin}"
    if plan.inorm:
        for k in range(1, Lv - 1):
            _check_plane(B, co[k], *S[k + 1])
    for k in range(Lv):  # conv_k reads the S[k] plane
        if plan.pad[k] != L.PAD_REFLECT:
            continue
        name = plan.conv_names[k]
        _check_reflect_plane(name, B, cin if k == 0 else co[k - 1], *S[k])
        if S[k][0] % 2 or S[k][1] % 2:
            # (the reference tree zero-pads an odd level to even and reflects about the padded extent: not built)
            raise NotImplementedError(
                f"stcgan_amd: generator level {k} ({name}, padding_mode='reflect') reads an odd {S[k][0]} x {S[k][1]} "
                f"plane for a {H} x {W} input: reflect padding needs every level even (H and W multiples of "
                f"{2 ** (Lv - 1)} here)")
    cin_pad = ops.pad_channels(cin, dt)
    xin = _nhwc(B, H, W, cin_pad, dt, dev)
    ops.gather(sources, xin, dt)

    def cin_t(k):
        return co[k] if k == Lv - 1 else 2 * co[k]

    rd = [None] + [_nhwc(B, *S[k + 1], co[k], dt, dev) for k in range(1, Lv)]  # (rd[0]: below)
    ad = [_nhwc(B, *S[k + 1], co[k], dt, dev) if k < Lv - 1 else None for k in range(Lv)]
    cr = [_nhwc(B, *S[k + 1], cin_t(k), dt, dev) for k in range(Lv)]
    rq = [None] + [_nhwc(B, *_pad2(S, k), co[k - 1], dt, dev) for k in range(1, Lv)]
    tab_d, tab_u, st_d, st_u = {}, {}, {}, {}
    mode = _norm_mode(plan, batch_stats)
    sync = _Sync(plan, B, dev) if mode == _SYNC else None

    # use_dropout, train mode: this call's {seed, offset} copy (one tiny launch; the generator's offset advances),
    # read from device memory by every dropout kernel of the call, forward and backward
    drop_state = ops.dropout_next(plan.net._dropout_tensor(dev)) if (train and plan.drop) else None

    def drop_of(k):
        """The dropout level on BN_up[k]'s output, over the full ConvT extent (before the crop), or None."""
        if drop_state is None or k not in plan.drop:
            return None
        return (drop_state, k, plan.drop[k]) + _pad2(S, k)

    # ---- down path
    w0 = ops.packed(cache, plan.conv[0].weight, L.PACK_CONV_FWD, co[0], cin_pad, dt)
    xv, av, sv = L.nhwc_view(xin), L.nhwc_view(ad[0]), L.nhwc_view(cr[0], 0)  # conv input, its activation, the skip
    if plan.pad[0] == L.PAD_ZEROS and ops.conv_act(L.CONV_S2, B, xv, cin_pad, w0, co[0], av, LRELU, dt, sv, 0.0):
        # no raw r_0: its only reader, the backward's ReLU/LeakyReLU test, sees the same signs in ad[0]
        rd[0] = ad[0]
    else:
        rd[0] = _nhwc(B, *S[1], co[0], dt, dev)
        rv = L.nhwc_view(rd[0])
        ops.conv(L.CONV_S2, B, xv, cin_pad, w0, co[0], rv, dt, pad=plan.pad[0])
        ops.bn_apply(B, rv, co[0], dt, None, av, LRELU, sv, 0.0)
    for k in range(1, Lv):
        wk = ops.packed(cache, plan.conv[k].weight, L.PACK_CONV_FWD, co[k], co[k - 1], dt)
        xv, rv = av, L.nhwc_view(rd[k])  # (conv_k reads the activation the level above wrote)
        if k <= Lv - 2:
            av = L.nhwc_view(ad[k])
            t, st_d[k] = _conv_norm_act(L.CONV_S2, B, xv, co[k - 1], wk, co[k], rv, dt, plan.bnd[k], mode, rv, av,
                                        LRELU, L.nhwc_view(cr[k], 0), 0.0, None, None, save, sync, plan.pad[k])
            if t is not None:
                tab_d[k] = t
        else:  # innermost: no down-norm (STCGAN/networks.py:118-124)
            ops.conv(L.CONV_S2, B, xv, co[k - 1], wk, co[k], rv, dt, pad=plan.pad[k])
            ops.bn_apply(B, rv, co[k], dt, None, L.nhwc_view(cr[k]), 0.0)
    # ---- up path
    for k in range(Lv - 1, 0, -1):
        wt = ops.packed(cache, plan.convT[k].weight, plan.pack_t_fwd, co[k - 1], cin_t(k), dt)
        # statistics over the full ConvT extent (before the crop of an odd level)
        t, st_u[k] = _conv_norm_act(L.CONVT_S2, B, L.nhwc_view(cr[k]), cin_t(k), wt, co[k - 1], L.nhwc_view(rq[k]), dt,
                                    plan.bnu[k], mode, L.nhwc_view(rq[k], 0, *S[k]),
                                    L.nhwc_view(cr[k - 1], co[k - 1]), 0.0, None, 0.0, drop_of(k), None, save, sync)
        if t is not None:
            tab_u[k] = t
    # ---- outermost: head(convT_0(cr[0]) + bias) -> NCHW fp32 (plan.head; tanh by default)
    Ho, Wo = 2 * S[1][0], 2 * S[1][1]
    y = torch.empty((B, plan.out_c, Ho, Wo), dtype=torch.float32, device=dev)
    wt0 = ops.packed(cache, plan.convT[0].weight, plan.pack_t_fwd, plan.out_c, 2 * co[0], dt)
    ops.conv(L.CONVT_S2, B, L.nhwc_view(cr[0]), 2 * co[0], wt0, plan.out_c, L.nchw_view(y), dt,
             bias=plan.convT[0].bias, act=plan.head, out_f32=True)
    saved = None
    if save:
        saved = dict(S=S, xin=xin, rd=rd, ad=ad, cr=cr, rq=rq, tab_d=tab_d, tab_u=tab_u, st_d=st_d, st_u=st_u,
                     y=y, cin=cin, cin_pad=cin_pad, src_c=[s.shape[1] for s in sources],
                     frozen=not (plan.inorm or batch_stats), sync=sync)
        if drop_state is not None:
            saved["drop"] = {k: drop_of(k) for k in plan.drop}
        if TRACE is not None:
            _trace_new("G")
            _trace("G", "saved", saved)
    return y, saved


def gen_backward(plan, saved, gy, dt, cache, need_src, W):
    """Returns the list of source grads (NCHW fp32 or None); the parameter gradients go to the
    GradWriter ``W`` (None: not needed)."""
    S, xin, rd, ad, cr, rq = saved["S"], saved["xin"], saved["rd"], saved["ad"], saved["cr"], saved["rq"]
    tab_d, tab_u, st_d, st_u, y = saved["tab_d"], saved["tab_u"], saved["st_d"], saved["st_u"], saved["y"]
    Lv, co = plan.L, plan.co
    dev = y.device
    B = y.shape[0]
    gy = gy.contiguous()
    need_w = W is not None
    lane = _WgradLane() if need_w else None
    drops = saved.get("drop") or {}  # {level: dropout level of the forward call} (use_dropout, train mode)
    mode, sync = _norm_mode(plan, not saved["frozen"]), saved["sync"]
    assert (mode == _SYNC) == (sync is not None), "the process group changed between a forward and its backward"
    # ---- output head + bias (the default head keeps its own entry: the same call as ever)
    cp = ops.vec(dt)
    Ho, Wo = y.shape[2], y.shape[3]
    dq = _nhwc(B, Ho, Wo, cp, dt, dev)
    dbias = W.dest(plan.convT[0].bias) if need_w else None
    if plan.head == "tanh":
        ops.tanh_bias_bwd(y, gy, L.nhwc_view(dq), dt, dbias=dbias)
    else:
        ops.head_bwd(y, gy, L.nhwc_view(dq), dt, plan.head, dbias=dbias)
    if need_w:
        W.done([plan.convT[0].bias])
    _trace("G", ("dq", 0), dq)
    # ---- up path backward: convT_k, then BN_up[k+1]
    gcat = [None] * Lv
    for k in range(Lv):
        cin_t = co[k] if k == Lv - 1 else 2 * co[k]
        cout_t = plan.out_c if k == 0 else co[k - 1]
        cg = cp if k == 0 else cout_t
        dqv = L.nhwc_view(dq)
        wT = plan.convT[k].weight
        if need_w:  # D = convT input (grid S[k+1]), G = dq gathered at stride 2
            out = W.dest(wT)
            if plan.upconv:
                def wg():  # (run at once, by lane.run: the scratch, the GEMM and the collapse on its stream)
                    dW4 = torch.empty((cin_t, cout_t, 4, 4), dtype=torch.float32, device=dev)
                    ops.wgrad(B, 2, L.nhwc_view(cr[k]), cin_t, dqv, cg, cout_t, dt, device=dev, out=dW4)
                    ops.upconv_wgrad_collapse(dW4, out)
                lane.run(wg, dq, pixels=S[k + 1][0] * S[k + 1][1])
            else:
                lane.run(lambda: ops.wgrad(B, 2, L.nhwc_view(cr[k]), cin_t, dqv, cg, cout_t, dt, device=dev, out=out),
                         dq, pixels=S[k + 1][0] * S[k + 1][1])
        wd = ops.packed(cache, wT, plan.pack_t_dgrad, cin_t, cg, dt)
        if k == Lv - 1:
            gcat[k] = _nhwc(B, *S[Lv], cin_t, dt, dev)
            _trace("G", ("gcat", k), gcat[k])
            ops.conv(L.CONV_S2, B, dqv, cg, wd, cin_t, L.nhwc_view(gcat[k], 0, *S[k + 1]), dt)
            if need_w:  # (after the last read of the weight: the optimiser may update it from here on)
                W.done([wT], lane)
            break
        # BN_up[k+1] over q_{k+1}: full (padded) extent; the cropped rows carry zero gradient.
        # Its gradient is the second half of gcat[k] (ReLU of the concat: channels C..2C -> BN channels 0..C)
        ah, aw = _pad2(S, k + 1)
        gcat[k] = _nhwc(B, ah, aw, cin_t, dt, dev, zero=(ah, aw) != S[k + 1])
        _trace("G", ("gcat", k), gcat[k])
        C = co[k]
        dq = _nhwc(B, ah, aw, C, dt, dev)
        _conv_act_norm_backward(L.CONV_S2, B, dqv, cg, wd, cin_t, gcat[k], L.nhwc_view(gcat[k], 0, *S[k + 1]), dt,
                                plan.bnu[k + 1], mode, tab_u.get(k + 1), st_u[k + 1], L.nhwc_view(rq[k + 1]), C, 0.0,
                                None, 0.0, C, L.nhwc_view(dq), drops.get(k + 1), [wT], W, lane, sync)
        _trace("G", ("dq", k + 1), dq)
    # ---- innermost r_{L-1}: ReLU backward (no BN)
    dr = _nhwc(B, *S[Lv], co[Lv - 1], dt, dev)
    ops.bn_backward(B, L.nhwc_view(rd[Lv - 1]), co[Lv - 1], dt, L.nhwc_view(dr), g1=L.nhwc_view(gcat[Lv - 1]),
                    s1=0.0)
    # ---- down path backward: conv_k, then BN_down[k-1]
    src_grads = None
    for k in range(Lv - 1, -1, -1):
        drv = L.nhwc_view(dr)
        _trace("G", ("dr", k), dr)
        wk = plan.conv[k].weight
        if k == 0:
            if need_w:
                out = W.dest(wk)
                lane.run(lambda: ops.wgrad(B, 2, drv, co[0], L.nhwc_view(xin), saved["cin_pad"], saved["cin"], dt,
                                           device=dev, out=out, pad=plan.pad[0]), dr, pixels=S[1][0] * S[1][1])
            if need_src:
                src_grads = _input_grads(B, drv, co[0], wk, saved, S[0], need_src, dt, cache, dev, plan.pad[0])
            if need_w:
                W.done([wk], lane)
            break
        j, cprev = k - 1, co[k - 1]
        if need_w:  # D = dr_k (grid S[k+1]), G = conv_k input = ad[k-1]
            out = W.dest(wk)
            lane.run(lambda: ops.wgrad(B, 2, drv, co[k], L.nhwc_view(ad[j]), cprev, cprev, dt, device=dev, out=out,
                                       pad=plan.pad[k]), dr, pixels=S[k + 1][0] * S[k + 1][1])
        wd = ops.packed(cache, wk, L.PACK_CONV_DGRAD, cprev, co[k], dt)
        ga = _nhwc(B, 2 * S[k + 1][0], 2 * S[k + 1][1], cprev, dt, dev)
        _trace("G", ("ga", k), ga)
        # r_{k-1} feeds the skip (ReLU; its gradient the first half of gcat[k-1]) and conv_k (LeakyReLU; ga, cropped
        # to S[k]); then BN_down[k-1] (absent for k-1 == 0)
        dr = _nhwc(B, *S[k], cprev, dt, dev)
        _conv_act_norm_backward(L.CONVT_S2, B, drv, co[k], wd, cprev, ga, L.nhwc_view(ga), dt, plan.bnd.get(j), mode,
                                tab_d.get(j), st_d.get(j), L.nhwc_view(rd[j]), cprev, LRELU,
                                L.nhwc_view(gcat[j], 0, *S[k]), 0.0, 0, L.nhwc_view(dr), None, [wk], W, lane, sync,
                                plan.pad[k])
    if lane is not None:
        lane.join()
    return src_grads


# ----------------------------------------------------------------------------- discriminator


class DiscPlan:
    """NLayerDiscriminator (STCGAN/networks.py:147-192): conv+bias, LReLU, [conv, BN, LReLU] x n, conv+bias."""

    def __init__(self, net):
        self.net = net
        seq = net.model
        convs = [m for m in seq if isinstance(m, torch.nn.Conv2d)]
        bns = [m for m in seq if isinstance(m, (torch.nn.BatchNorm2d, torch.nn.SyncBatchNorm,
                                                torch.nn.InstanceNorm2d))]
        assert len(convs) == len(bns) + 2
        self.convs, self.bns = convs, bns
        self.inorm, self.affine = _norm_kind(bns)
        self.sync, self.norm_names = _sync_kind(bns, {id(m): n for n, m in net.named_modules()})
        self.n = len(convs)
        self.strides = [c.stride[0] for c in convs]
        names = {id(m): n for n, m in net.named_modules()}
        self.conv_names = [names.get(id(c), "?") for c in convs]
        self.pad = [_pad_of(c, n) for c, n in zip(convs, self.conv_names)]  # per conv: L.PAD_ZEROS / L.PAD_REFLECT
        self.in_c = convs[0].in_channels
        self.params = list(net.parameters())


def _conv_out(h, s):
    return (h + 2 - 4) // s + 1


def disc_forward(plan, sources, train, dt, cache, save, inputs=None, stats_only=False, defer=None,
                 batch_stats=None):
    """train / batch_stats: as gen_forward's (a discriminator has no dropout: only batch_stats matters).
    raw[i] = conv_{i-1} raw output (raw[0] = padded input); act[i] = input of conv_i.
    inputs: optional dict reusing the gathered NHWC input across calls on the same source tensors
    (the trainer's real/fake pairs are fed to each discriminator twice per step, STCGAN/stcgan.py:215-280;
    valid while those tensors are alive and unmodified -- one train step)."""
    dev = sources[0].device
    B, _, H, W = sources[0].shape
    cin = sum(s.shape[1] for s in sources)
    assert cin == plan.in_c, f"discriminator expects {plan.in_c} input channels, got {cin}"
    n = plan.n
    if batch_stats is None:
        batch_stats = train
    if stats_only and (plan.inorm or not batch_stats):
        # no running statistics to advance: nothing to do (the zero-element placeholder, as below)
        return torch.empty((B, plan.convs[-1].out_channels, 0, 0), dtype=torch.float32, device=dev), None
    if plan.inorm:
        hw = (H, W)
        for i, cv in enumerate(plan.convs[:-1]):
            hw = (_conv_out(hw[0], plan.strides[i]), _conv_out(hw[1], plan.strides[i]))
            if i >= 1:
                _check_plane(B, cv.out_channels, *hw)
    cin_pad = ops.pad_channels(cin, dt)
    # first-layer bias gradient for free: a constant-1 plane in the first padding channel (its packed weights
    # are zero) makes the weight gradient's tap (1,1) of that channel sum the output gradient over every pixel
    # (k4 s2 p1: input row 2*o + kh - 1 = 2*o is always inside), replacing a full pass over that gradient
    bias_ch = cin if (plan.convs[0].bias is not None and cin < cin_pad and len(sources) < 4
                      and plan.strides[0] == 2) else None
    key = None
    if inputs is not None:
        key = tuple((s.data_ptr(), s._version, tuple(s.shape)) for s in sources) + (dt, cin_pad)
    xin = inputs.get(key) if key is not None else None
    if xin is None:
        xin = _nhwc(B, H, W, cin_pad, dt, dev)
        ops.gather(list(sources) + ([_ones_plane(B, H, W, dev)] if bias_ch is not None else []), xin, dt)
        if key is not None:
            inputs[key] = xin
    raw, act, dims, chans, tabs, stats = [xin], [xin], [(H, W)], [cin_pad], [None], [None]
    out = None
    mode = _norm_mode(plan, batch_stats)
    sync = _Sync(plan, B, dev) if mode == _SYNC else None
    xv = L.nhwc_view(xin)  # (of act[i], the input of conv_i)
    for i, cv in enumerate(plan.convs):
        s = plan.strides[i]
        if s == 2 and plan.pad[i] == L.PAD_ZEROS:  # (a reflect layer takes every extent >= 2, as torch: section 8i)
            assert dims[i][0] % 2 == 0 and dims[i][1] % 2 == 0, "stride-2 discriminator layers need even sizes"
        h, w = _conv_out(dims[i][0], s), _conv_out(dims[i][1], s)
        cout = cv.out_channels
        pad = plan.pad[i]
        if pad == L.PAD_REFLECT:
            _check_reflect_plane(plan.conv_names[i], B, cv.in_channels, *dims[i])
        wp = ops.packed(cache, cv.weight, L.PACK_CONV_FWD, cout, chans[i], dt)
        kind = L.CONV_S2 if s == 2 else L.CONV_S1
        if i == n - 1:
            if stats_only:  # logits not computed: a zero-element placeholder, so that no caller can read garbage
                out = torch.empty((B, cout, 0, 0), dtype=torch.float32, device=dev)
                break
            out = torch.empty((B, cout, h, w), dtype=torch.float32, device=dev)
            ops.conv(kind, B, xv, chans[i], wp, cout, L.nchw_view(out), dt, bias=cv.bias, out_f32=True, pad=pad)
            break
        tab, st = None, None
        a = _nhwc(B, h, w, cout, dt, dev)
        av = L.nhwc_view(a)
        if i >= 1:  # conv -> norm -> LeakyReLU (networks.py:167-180); no conv bias there
            assert cv.bias is None
            o = _nhwc(B, h, w, cout, dt, dev)
            ov = L.nhwc_view(o)
            # (stats_only: only the logits layer reads the last activation -- no pass)
            t, st = _conv_norm_act(kind, B, xv, chans[i], wp, cout, ov, dt, plan.bns[i - 1], mode, ov,
                                   None if (stats_only and i == n - 2) else av, LRELU, None, 0.0, None, defer, save, sync,
                                   pad)
            if t is not None:
                tab = (t[0], t[1])
        elif pad == L.PAD_ZEROS and ops.conv_act(kind, B, xv, chans[i], wp, cout, av, LRELU, dt, bias=cv.bias):
            o = a  # no raw output: the backward's LeakyReLU test sees the same signs in the activation
        else:
            o = _nhwc(B, h, w, cout, dt, dev)
            ov = L.nhwc_view(o)
            ops.conv(kind, B, xv, chans[i], wp, cout, ov, dt, bias=cv.bias, pad=pad)
            ops.bn_apply(B, ov, cout, dt, None, av, LRELU)
        xv = av
        raw.append(o)
        act.append(a)
        dims.append((h, w))
        chans.append(cout)
        tabs.append(tab)
        stats.append(st)
    saved = None
    if save:
        saved = dict(raw=raw, act=act, dims=dims, chans=chans, tabs=tabs, stats=stats, cin=cin, cin_pad=cin_pad,
                     bias_ch=bias_ch, frozen=not (plan.inorm or batch_stats), sync=sync,
                     src_c=[s.shape[1] for s in sources])
        if TRACE is not None:
            _trace_new("D")
            _trace("D", "saved", saved)
    return out, saved


def disc_backward(plan, saved, gout, dt, cache, need_src, W):
    """Returns the list of source grads (NCHW fp32 or None); parameter gradients go to the GradWriter ``W``."""
    raw, act, dims, chans, tabs, stats = (saved["raw"], saved["act"], saved["dims"], saved["chans"], saved["tabs"],
                                          saved["stats"])
    dev = gout.device
    B = gout.shape[0]
    n = plan.n
    need_w = W is not None
    cp = ops.vec(dt)
    h, w = gout.shape[2], gout.shape[3]
    # gradient of the logits [B,1,h,w] -> NHWC with cp channels (channel counts are vector multiples)
    g = _nhwc(B, h, w, cp, dt, dev)
    ops.gather([gout.contiguous()], g, dt)
    gch = cp
    src_grads = None
    lane = _WgradLane() if need_w else None
    mode, sync = _norm_mode(plan, not saved["frozen"]), saved["sync"]
    assert (mode == _SYNC) == (sync is not None), "the process group changed between a forward and its backward"
    for i in range(n - 1, -1, -1):
        cv = plan.convs[i]
        s = plan.strides[i]
        cout = cv.out_channels
        pad = plan.pad[i]
        gv = L.nhwc_view(g, 0, h, w)  # gradient wrt conv_i output (pre-activation / pre-BN), gch channels
        _trace("D", ("g", i), g)
        if need_w:
            bc = saved["bias_ch"] if i == 0 else None
            if bc is None:
                dw_out = W.dest(cv.weight)
                db_out = W.dest(cv.bias) if cv.bias is not None else None
            else:  # the weight gradient of the padded input (+ the constant-1 channel) goes through a scratch
                dw_out, db_out = W.dest(cv.weight), W.dest(cv.bias)

            def wg():  # (run at once, by lane.run)
                if bc is not None:  # the constant-1 channel's tap (1,1) is the bias gradient (disc_forward)
                    dW = ops.wgrad(B, s, gv, gch, L.nhwc_view(act[i]), chans[i], bc + 1, dt, device=dev, rows=cout,
                                   pad=pad)
                    dw_out.copy_(dW[:cout, :saved["cin"]])
                    db_out.copy_(dW[:cout, bc, 1, 1])
                    return
                ops.wgrad(B, s, gv, gch, L.nhwc_view(act[i]), chans[i], saved["cin"] if i == 0 else chans[i], dt,
                          device=dev, rows=cout, out=dw_out, pad=pad)
                if cv.bias is not None:
                    ops.chan_sum(B, gv, gch, cout, dt, dev, out=db_out)
            lane.run(wg, g, pixels=h * w)
        own = [cv.weight] + ([cv.bias] if cv.bias is not None else [])
        if i == 0:
            if need_src:
                src_grads = _input_grads(B, gv, gch, cv.weight, saved, dims[0], need_src, dt, cache, dev, pad)
            if need_w:
                W.done(own, lane)
            break
        # input gradient of conv_i (grad wrt act[i])
        ph, pw = dims[i]
        cin = chans[i]
        ga = _nhwc(B, ph, pw, cin, dt, dev)
        if s == 2:
            wd = ops.packed(cache, cv.weight, L.PACK_CONV_DGRAD, cin, gch, dt)
            dkind = L.CONVT_S2
        else:
            wd = ops.packed(cache, cv.weight, L.PACK_CONV_S1_DGRAD, cin, gch, dt)
            dkind = L.CONV_S1_DGRAD
        # through LeakyReLU and the norm of layer i-1's output (none after layer 0)
        gn = _nhwc(B, ph, pw, cin, dt, dev)
        _trace("D", ("ga", i), ga)
        _conv_act_norm_backward(dkind, B, gv, gch, wd, cin, ga, L.nhwc_view(ga), dt,
                                plan.bns[i - 2] if i >= 2 else None, mode, tabs[i], stats[i], L.nhwc_view(raw[i]), cin,
                                LRELU, None, 0.0, 0, L.nhwc_view(gn), None, own, W, lane, sync, pad)
        g, gch, h, w = gn, cin, ph, pw
    if lane is not None:
        lane.join()
    return src_grads


# ----------------------------------------------------------------------------- autograd


class Ctrl(typing.NamedTuple):
    """What one network call needs beside its tensors (NetFn's first input; networks._HipNet._run)."""
    plan: object         # GenPlan / DiscPlan
    kind: str            # "G" / "D"
    train: bool          # the network's own training flag (dropout levels)
    dt: torch.dtype      # compute dtype
    cache: dict          # packed weights
    nsrc: int            # number of sources among the tensor inputs
    inputs: object       # dict reusing gathered discriminator inputs, or None
    consumer: object     # stream that reads the source gradients, or None
    stats_only: bool     # discriminator: only the running statistics are wanted
    defer: object        # list collecting the running-statistics updates, or None
    batch_stats: bool    # the BatchNorm modules' mode (networks._HipNet._batch_stats)


class NetFn(torch.autograd.Function):
    """One autograd node per network call.  inputs: (ctrl, *sources, *params), ctrl a Ctrl.

    The backward returns gradients for the sources only: the parameters' gradients are written by the
    kernels straight into the network's flat gradient buffer (GradWriter), so autograd never allocates,
    accumulates or hooks them (``p.grad`` is set by the backward itself)."""

    @staticmethod
    def forward(ctx, ctrl, *tensors):
        sources = [t.contiguous().float() for t in tensors[:ctrl.nsrc]]
        save = any(ctx.needs_input_grad[1:])  # (every mode: nothing under torch.no_grad())
        ops.refresh_packs(ctrl.cache)  # all operands packed since the last optimiser step, one launch
        if ctrl.kind == "G":
            out, saved = gen_forward(ctrl.plan, sources, ctrl.train, ctrl.dt, ctrl.cache, save, ctrl.batch_stats)
        else:
            out, saved = disc_forward(ctrl.plan, sources, ctrl.train, ctrl.dt, ctrl.cache, save, ctrl.inputs,
                                      ctrl.stats_only and not save, ctrl.defer, ctrl.batch_stats)
        ctx.ctrl = ctrl
        ctx.saved_net = saved
        return out

    @staticmethod
    def backward(ctx, gout):
        ctrl = ctx.ctrl
        plan, nsrc, consumer = ctrl.plan, ctrl.nsrc, ctrl.consumer
        saved = ctx.saved_net
        if saved is None:
            raise RuntimeError("stcgan_amd: this network call saved nothing for a backward (a second backward "
                               "through the same call?)")
        need = ctx.needs_input_grad[1:]
        need_src = list(need[:nsrc]) if any(need[:nsrc]) else None  # per source, or None
        W = GradWriter(plan.net) if any(need[nsrc:]) else None
        if gout.is_cuda:
            # a side-stream network's incoming gradient is allocated on the main stream (the loss
            # backward): autograd orders this stream after it, but does not keep the caching allocator
            # from handing the block back to the main stream once this Python call returns, while the
            # kernels enqueued here may still read it
            gout.record_stream(torch.cuda.current_stream(gout.device))
        bwd = gen_backward if ctrl.kind == "G" else disc_backward
        src_grads = bwd(plan, saved, gout, ctrl.dt, ctrl.cache, need_src, W)
        if W is not None:
            W.flush()
        ctx.saved_net = None
        out = [None]
        for i in range(nsrc):
            out.append(src_grads[i] if (src_grads is not None and need[i]) else None)
            if consumer is not None and out[-1] is not None:
                # a side-stream network's input gradient is read (and freed) on the consumer's stream: keep
                # its block from being reused on this stream before the consumer is done with it
                out[-1].record_stream(consumer)
        out.extend([None] * len(plan.params))
        return tuple(out)
