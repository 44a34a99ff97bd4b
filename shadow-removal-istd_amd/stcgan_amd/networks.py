"""Drop-in replacement for STCGAN/networks.py on MI355X.

Same factories (``get_generator``, ``get_discriminator``, ``weights_init``),
same module tree and therefore identical ``state_dict`` keys/shapes, so
reference checkpoints (``G1-latest.pt`` ...) load unchanged.  The torch.nn
layers inside the tree only hold parameters and buffers; ``forward`` of the
network runs the whole network as hand-written HIP kernels
(``engine.gen_forward`` / ``engine.disc_forward``) behind one autograd node.

``norm_layer``: nn.BatchNorm2d (default), nn.SyncBatchNorm (the BatchNorm2d tree and keys; with torch.distributed
initialised and more than one rank its train-mode statistics run over the batches of all ranks, one small collective per
normed layer and direction, default process group only; otherwise exactly BatchNorm2d -- also a BatchNorm2d network
converted by ``nn.SyncBatchNorm.convert_sync_batchnorm`` before its first forward), nn.InstanceNorm2d, or a functools.partial of nn.InstanceNorm2d with
``affine`` and/or ``eps`` (instance statistics in train and eval mode; no buffers); anything else raises.

Differences from the reference that a caller can observe: none in values
(parity-tested; ``use_dropout=True`` draws its train-mode masks from a counter-based
generator of its own, ``set_dropout_seed`` / ``dropout_state``, not torch's); odd spatial sizes follow the pad/crop generator of
src/models/stcgan_g.py:120-132 (the STCGAN/networks.py version raises there);
forward also accepts a list/tuple of NCHW tensors, treated as their channel
concatenation without materialising it (what ``torch.cat(..., 1)`` would give).

``no_conv_t=True`` (the ``--NN-upconv`` option of the reference's src/ line, src/models/opt_layers.py:39-56): every
``ConvTranspose2d(4, 2, 1)`` of the up path becomes ``nn.Upsample(scale_factor=2, mode="nearest")`` +
``nn.Conv2d(3, 1, 1)`` (resize-convolution, no checkerboard artifacts).  The same HIP kernels run it: with zero
padding the pair is exactly a ConvTranspose2d whose 4x4 weight is a fixed sum of the 3x3 taps.
The up convs' ``padding_mode`` is ``"zeros"``; the reference's helper uses ``"reflect"`` there (equal to replicate
padding of the low-resolution input by one pixel), which the ConvT kernels that run the pair cannot express: out of
scope on the up path, refused.

``padding_mode`` (``"zeros"``, the default, or ``"reflect"``; both factories): with ``"reflect"`` every
``nn.Conv2d(kernel_size=4)`` of the tree -- the generator's down convs, all convs of the discriminator -- is built with
``padding_mode="reflect"``, as the convs of the reference's src/models (mnet.py, patchgan.py, unet.py) are.  No
state_dict key or shape changes; the network computes what torch computes for that tree.  ConvTranspose2d has no padding
mode and keeps zeros, as do the 3x3 up convs of ``no_conv_t``.  The reflect layers run the reflect instantiations of
the gather kernels and the unfused step forms.  A reflect conv over a plane one pixel high or
wide raises RuntimeError as torch does; a generator input with an odd level (H or W no multiple of 2^(num_downs-1))
raises NotImplementedError at call time, naming the level (the reference zero-pads such a level to even and reflects
about the padded extent: not built).  The reflect discriminator follows torch for every extent >= 2, odd stride-2
planes included.
``conv_t_state_dict()`` exports such a generator as the plain ST-CGAN one.

``activation`` (the ``--activation`` option of the same line, src/models/opt_layers.py:7-18): the generator's output head,
``"tanh"`` (default), ``"sigmoid"``, ``"htanh"`` (``nn.Hardtanh(-1, 1)``) or ``"none"`` / ``None``; fused into the output
ConvT's epilogue and the first backward kernel.

Modes are torch's, read from the modules at every call: the network's own ``training`` flag governs the dropout
levels, its BatchNorm2d children's flags govern batch statistics + running update (train) against running statistics
with untouched buffers (eval) -- ``net.eval()``, or ``net.train()`` with the norm children in eval (``freeze_norm``).
Every mode has a backward.  BatchNorm children in mixed modes raise NotImplementedError.
"""
import torch
import torch.nn as nn

from . import engine
from . import ops

# the norm modules with batch / running statistics (nn.SyncBatchNorm is no subclass of nn.BatchNorm2d)
_BATCH_NORMS = (nn.BatchNorm2d, nn.SyncBatchNorm)
_DTYPES = {"fp32": torch.float32, "float32": torch.float32, "bf16": torch.bfloat16, "bfloat16": torch.bfloat16}


@torch.no_grad()
def weights_init(m):
    """custom weights initialization called on network model (STCGAN/networks.py:9-20)"""
    classname = m.__class__.__name__
    if classname.find('Conv') != -1 or classname.find('BatchNorm') != -1:
        nn.init.normal_(m.weight.data, 0.0, 0.02)
        if m.bias is not None:
            nn.init.constant_(m.bias.data, 0)
    elif classname.find('Linear') != -1:
        nn.init.normal_(m.weight.data, 1.0, 0.02)
        if m.bias is not None:
            nn.init.constant_(m.bias.data, 0)


def get_generator(*args, **kwargs):
    return UnetGenerator(*args, **kwargs)


def get_discriminator(*args, **kwargs):
    return NLayerDiscriminator(*args, **kwargs)


def check_drop_rate(p):
    """A dropout probability as a float, 0 <= p < 1 (ValueError otherwise)."""
    if isinstance(p, bool) or not isinstance(p, (int, float)) or not 0.0 <= float(p) < 1.0:
        raise ValueError(f"stcgan_amd: dropout probability must be a number with 0 <= p < 1, got {p!r}")
    return float(p)


def check_norm_layer(norm_layer, use_dropout=False):
    """'batch' for nn.BatchNorm2d, 'sync_batch' for nn.SyncBatchNorm (default process group), 'instance' for nn.InstanceNorm2d or a functools.partial of it (affine and/or eps);
    NotImplementedError for anything else.  Decided from the constructed module, as the layers will be."""
    if norm_layer is nn.BatchNorm2d:
        return "batch"
    if norm_layer is nn.SyncBatchNorm:
        return "sync_batch"
    name = getattr(getattr(norm_layer, "func", norm_layer), "__name__", repr(norm_layer))
    try:
        m = norm_layer(8)
    except Exception:
        m = None
    if type(m) is nn.SyncBatchNorm:  # (a functools.partial of it)
        if m.process_group is not None:
            raise NotImplementedError("stcgan_amd: nn.SyncBatchNorm with a process_group of its own is not supported "
                                      "(the statistics travel over the default process group)")
        if not (m.affine and m.track_running_stats):
            raise NotImplementedError("stcgan_amd: nn.SyncBatchNorm with affine=False or track_running_stats=False "
                                      "is not supported")
        return "sync_batch"
    if type(m) is not nn.InstanceNorm2d:
        raise NotImplementedError(f"stcgan_amd: norm_layer {name if m is None else type(m).__name__} is not on the "
                                  "ST-CGAN path (nn.BatchNorm2d, nn.SyncBatchNorm, nn.InstanceNorm2d or a functools.partial of "
                                  "nn.InstanceNorm2d with affine / eps)")
    if m.track_running_stats:
        raise NotImplementedError("stcgan_amd: nn.InstanceNorm2d with track_running_stats=True is not supported "
                                  "(instance statistics only, in train and eval mode)")
    if use_dropout:
        raise NotImplementedError("stcgan_amd: use_dropout=True together with nn.InstanceNorm2d is not supported "
                                  "(the dropout kernels are written against the BatchNorm per-channel tables)")
    return "instance"


ACTIVATIONS = ("none", "sigmoid", "tanh", "htanh")


def check_activation(v):
    """A generator output activation as one of ACTIVATIONS (None means "none"; ValueError otherwise)."""
    if v is None:
        return "none"
    if not isinstance(v, str) or v not in ACTIVATIONS:
        raise ValueError("stcgan_amd: activation must be one of 'none', 'sigmoid', 'tanh', 'htanh' (or None for "
                         f"'none'), got {v!r}")
    return v


def get_activation(key):
    """The module of an output activation, as the reference maps it (src/models/opt_layers.py:7-18); None for
    "none"."""
    key = check_activation(key)
    if key == "tanh":
        return nn.Tanh()
    if key == "sigmoid":
        return nn.Sigmoid()
    if key == "htanh":
        return nn.Hardtanh(min_val=-1.0, max_val=1.0, inplace=True)
    return None


PADDING_MODES = ("zeros", "reflect")


def check_padding_mode(v):
    """A padding mode of the 4x4 convs as one of PADDING_MODES (ValueError otherwise)."""
    if not isinstance(v, str) or v not in PADDING_MODES:
        raise ValueError(f"stcgan_amd: padding_mode must be one of 'zeros', 'reflect', got {v!r}")
    return v


def check_flag(name, v):
    """A boolean option as a bool (True / False / 0 / 1; ValueError otherwise)."""
    if not isinstance(v, (bool, int)) or v not in (0, 1):
        raise ValueError(f"stcgan_amd: {name} must be a bool, got {v!r}")
    return bool(v)


def upconv_to_conv_t(weight):
    """The ``ConvTranspose2d(4, 2, 1)`` weight [cin, cout, 4, 4] that computes what ``nn.Upsample(2, "nearest")`` +
    ``nn.Conv2d(cin, cout, 3, 1, 1)`` with this weight [cout, cin, 3, 3] computes (zero padding; fp32, on the weight's
    ROCm device: stc_upconv_expand).  W4[ci][co][k][l] = sum of w[co][ci][a][b] over a in rows(k), b in rows(l), with
    rows(0) = {2}, rows(1) = {1, 2}, rows(2) = {0, 1}, rows(3) = {0}."""
    if weight.dim() != 4 or tuple(weight.shape[2:]) != (3, 3):
        raise ValueError(f"stcgan_amd: a [cout, cin, 3, 3] conv weight is expected, got {tuple(weight.shape)}")
    if not weight.is_cuda:
        raise RuntimeError("stcgan_amd: upconv_to_conv_t runs on the GPU only (HIP kernel); move the weight to a "
                           "ROCm device")
    return ops.upconv_expand(weight.detach().float())


class _HipNet(nn.Module):
    """Common runner: compute dtype, packed-weight cache, one autograd node per call."""

    kind = None

    def __init__(self):
        super().__init__()
        self.compute_dtype = torch.float32
        self._pack_cache = {}
        self._plan = None
        self._bn_named = None  # [(name, BatchNorm2d child)], made at the first call (_batch_stats)
        # parallel.BucketExchange averaging this network's gradients over the ranks while its backward runs
        # (set by the trainer when world > 1), or None
        self.grad_exchange = None
        self._exchange_spec = None
        # dict reusing gathered inputs across this network's calls on the same tensors (set by the trainer
        # for one train step), or None
        self.input_cache = None
        # stream that consumes this network's input gradients when it runs on a side stream (set by the
        # trainer), or None
        self.grad_consumer = None
        # a call whose output is not used but whose BatchNorm running statistics must advance (the trainer's
        # G-step real-input discriminator calls with loss type "normal"): the layers after the last
        # BatchNorm are skipped and the output is left unwritten
        self.stats_only = False
        # a list (set by the trainer for one call): the call's BatchNorm layers leave their running statistics
        # alone and append what ops.bn_running_update needs to apply the update later (the trainer orders it after
        # another call's, as the reference's call order has it)
        self.defer_running = None
        # a list (tests, diagnostics): every call on sync statistics appends its list of collectives,
        # [(norm layer name, "forward" / "backward")] in host order (engine._Sync)
        self.sync_log = None

    def set_compute_dtype(self, dtype):
        """'fp32' (default, parity path) or 'bf16' (bf16 operands, fp32 accumulation/BN/master weights)."""
        self.compute_dtype = _DTYPES[dtype] if isinstance(dtype, str) else dtype
        self._pack_cache.clear()
        ops.invalidate_packs()
        return self

    def _run(self, inp):
        sources = list(inp) if isinstance(inp, (list, tuple)) else [inp]
        batch_stats = self._batch_stats()  # (first: mixed BatchNorm modes are refused whatever the inputs)
        for s in sources:
            if not s.is_cuda:
                raise RuntimeError("stcgan_amd networks run on the GPU only (HIP kernels); move the model and "
                                   "inputs to a ROCm device")
        if self._plan is None:
            self._plan = self._make_plan()
        params = self._plan.params
        ctrl = engine.Ctrl(plan=self._plan, kind=self.kind, train=self.training, dt=self.compute_dtype,
                           cache=self._pack_cache, nsrc=len(sources), inputs=self.input_cache,
                           consumer=self.grad_consumer, stats_only=self.stats_only, defer=self.defer_running,
                           batch_stats=batch_stats)
        return engine.NetFn.apply(ctrl, *sources, *params)

    def _batch_stats(self):
        """Whether this call's BatchNorm layers use batch statistics (and update their running ones): their own
        ``training`` flags, all alike.  Instance norm has one mode: the network's flag, which nothing reads."""
        named = self._bn_named
        if named is None:  # (the module tree is fixed at construction)
            named = self._bn_named = [(n, m) for n, m in self.named_modules() if isinstance(m, _BATCH_NORMS)]
        on = sum(m.training for _, m in named)
        if on == len(named):
            return bool(named) or self.training
        if on == 0:
            return False
        raise NotImplementedError(
            "stcgan_amd: BatchNorm2d layers of one network in mixed modes are not supported -- in train mode: "
            + ", ".join(n for n, m in named if m.training) + "; in eval mode: "
            + ", ".join(n for n, m in named if not m.training) + " (freeze_norm() switches all of them)")

    def freeze_norm(self, on=True):
        """Put exactly the norm children in eval mode (BatchNorm2d: running statistics, buffers untouched; the
        usual fine-tuning idiom), or with ``on=False`` back into the network's own mode.  Dropout keeps following
        the network's mode.  ``net.train()`` / ``net.eval()`` reset every child, as in torch: call this after
        them.  No effect on the computation of instance-norm networks.  Returns self."""
        for m in self.modules():
            if isinstance(m, _BATCH_NORMS + (nn.InstanceNorm2d,)):
                m.training = self.training and not on
        return self

    def _apply(self, fn, *args, **kwargs):
        self._pack_cache.clear()
        ops.invalidate_packs()
        self._plan = None
        # the flat gradient buffer (parallel.flat_grads) lives on the parameters' device: a new one is made
        # on the next backward; an exchange bound to the old buffer is dropped with it
        self._flat_grads = None
        ex = self.grad_exchange
        if ex is not None:  # re-made on the new buffer by the next backward (engine.GradWriter)
            self._exchange_spec = (ex.bucket_elems * 4 / (1 << 20), ex.active, ex.on_complete, ex.expected)
        self.grad_exchange = None
        return super()._apply(fn, *args, **kwargs)


class UnetGenerator(_HipNet):
    """Create a Unet-based generator (STCGAN/networks.py:31-76)"""

    kind = "G"

    def __init__(self, in_channels, out_channels, ngf=64, num_downs=8, norm_layer=nn.BatchNorm2d,
                 use_dropout=False, drop_rate=None, no_conv_t=False, activation="tanh", padding_mode="zeros"):
        """padding_mode: "zeros" (default) or "reflect" -- the padding mode of the num_downs 4x4 down convs (module
        docstring); the up layers keep zeros.  Read from the conv modules when the launch plan is
        made.  Composes with every other option.
        activation (the reference's keyword, src/main.py:295-297, src/models/opt_layers.py:7-18): the module after the
        outermost up layer -- "tanh" (default) nn.Tanh, "sigmoid" nn.Sigmoid, "htanh" nn.Hardtanh(-1, 1), "none" / None
        nothing (the outermost Sequential then has 4 modules).  None of them has parameters: every state_dict key is the
        default generator's and checkpoints load across heads.  The head runs in the output ConvT's epilogue and in the
        first backward kernel; it is read from that module when the launch plan is made (a module outside this table,
        swapped in by hand, raises NotImplementedError there).  Composes with every other option.
        no_conv_t (the reference's keyword, src/models/opt_layers.py:39-56): each up layer is
        nn.Sequential(nn.Upsample(scale_factor=2, mode="nearest"), nn.Conv2d(cin, cout, 3, 1, 1)) at the ConvTranspose2d's
        index, its keys ``...model.N.1.weight`` [cout, cin, 3, 3] (and ``model.3.1.bias`` on the outermost layer).
        Their padding_mode is "zeros" whatever ``padding_mode`` says: the reference helper's "reflect" (a replicate
        halo of the low-resolution input) is out of scope.  Composes with every other option.
        use_dropout: nn.Dropout after the up-norm of the num_downs - 5 blocks above the innermost one, as the
        reference (p = 0.5; ``drop_rate`` overrides it, 0 <= drop_rate < 1).  Train mode only; the masks are a
        counter-based function of this generator's {seed, offset} (set_dropout_seed / dropout_state).  p is read
        from the nn.Dropout modules when the launch plan is made (the first forward, and again after a module move):
        set_drop_rate changes it later; writing ``Dropout.p`` by hand does not reach an existing plan."""
        super().__init__()
        self.norm_kind = check_norm_layer(norm_layer, use_dropout)
        p = check_drop_rate(0.5 if drop_rate is None else drop_rate)
        self._drop_state = None  # device int64 {seed, offset}: a plain attribute, the state_dict keys stay the reference's
        self.no_conv_t = nct = check_flag("no_conv_t", no_conv_t)
        self.activation = check_activation(activation)
        self.padding_mode = pm = check_padding_mode(padding_mode)
        unet_block = UnetSkipConnectionBlock(ngf * 8, ngf * 8, input_nc=None, submodule=None,
                                             norm_layer=norm_layer, innermost=True, no_conv_t=nct, padding_mode=pm)
        for _ in range(num_downs - 5):
            unet_block = UnetSkipConnectionBlock(ngf * 8, ngf * 8, input_nc=None, submodule=unet_block,
                                                 norm_layer=norm_layer, use_dropout=bool(use_dropout), drop_rate=p,
                                                 no_conv_t=nct, padding_mode=pm)
        unet_block = UnetSkipConnectionBlock(ngf * 4, ngf * 8, input_nc=None, submodule=unet_block,
                                             norm_layer=norm_layer, no_conv_t=nct, padding_mode=pm)
        unet_block = UnetSkipConnectionBlock(ngf * 2, ngf * 4, input_nc=None, submodule=unet_block,
                                             norm_layer=norm_layer, no_conv_t=nct, padding_mode=pm)
        unet_block = UnetSkipConnectionBlock(ngf, ngf * 2, input_nc=None, submodule=unet_block,
                                             norm_layer=norm_layer, no_conv_t=nct, padding_mode=pm)
        self.model = UnetSkipConnectionBlock(out_channels, ngf, input_nc=in_channels, submodule=unet_block,
                                             outermost=True, norm_layer=norm_layer, no_conv_t=nct,
                                             activation=self.activation, padding_mode=pm)

    def conv_t_state_dict(self):
        """The state_dict of the equivalent plain ST-CGAN generator (ConvTranspose2d up layers): each up layer's
        ``N.1.weight`` [cout, cin, 3, 3] becomes ``N.weight`` [cin, cout, 4, 4] (upconv_to_conv_t), ``N.1.bias``
        becomes ``N.bias``, everything else is copied.  Loads into the reference's STCGAN/networks.py generator and
        into this module's default one, which then computes what this generator computes.  A generator that already
        has ConvTranspose2d up layers returns a copy of its state_dict."""
        sd = self.state_dict()
        up = {}  # key prefix of each Upsample + Conv2d up layer -> its Conv2d
        for name, m in self.named_modules():
            if isinstance(m, nn.Sequential) and len(m) == 2 and isinstance(m[0], nn.Upsample):
                up[name + ".1."] = name + "."
        out = type(sd)()
        for key, v in sd.items():
            pre = next((p for p in up if key.startswith(p)), None)
            if pre is None:
                out[key] = v.detach().clone()
            elif key == pre + "weight":
                out[up[pre] + "weight"] = upconv_to_conv_t(v)
            else:
                out[up[pre] + key[len(pre):]] = v.detach().clone()
        return out

    def _make_plan(self):
        return engine.GenPlan(self)

    def _apply(self, fn, *args, **kwargs):
        if self._drop_state is not None:  # the counter moves with the module (a plain attribute: not in _buffers)
            self._drop_state = fn(self._drop_state)
        return super()._apply(fn, *args, **kwargs)

    def _dropout_tensor(self, device):
        """The device int64 {seed, offset}; made at first use with the seed torch.initial_seed() + rank."""
        st = self._drop_state
        if st is None or st.device != device:
            from . import parallel
            seed, off = ((int(v) for v in st.tolist()) if st is not None else
                         (ops.dropout_rank_seed(torch.initial_seed(), parallel.rank()), 0))
            st = self._drop_state = ops.dropout_state_tensor(seed, off, device)
        return st

    def set_dropout_seed(self, seed, offset=0):
        """Set the dropout {seed, offset} (64-bit seed; offset = the number of train-mode forwards drawn so far).
        Written in place once the state exists, so a captured graph keeps reading it."""
        dev = next(self.parameters()).device
        new = ops.dropout_state_tensor(seed, offset, dev)
        if self._drop_state is not None and self._drop_state.device == dev:
            self._drop_state.copy_(new)
        else:
            self._drop_state = new
        return self

    def set_drop_rate(self, p):
        """Set the drop probability (0 <= p < 1) of every nn.Dropout of this generator; the launch plan, which
        caches it, is made again at the next forward."""
        p = check_drop_rate(p)
        for m in self.modules():
            if isinstance(m, nn.Dropout):
                m.p = p
        self._plan = None
        return self

    def dropout_state(self):
        """(seed, offset) as Python ints (a host sync); the seed unsigned.  Not a pure read on a generator whose state
        does not exist yet: like the first train-mode forward it creates it, fixing the default seed
        torch.initial_seed() + rank as of this call.  That default is the same for every generator of a process, so
        two stand-alone generators that are never given seeds draw the same masks at equal level and shape: give
        them distinct seeds (set_dropout_seed), as the trainer does."""
        dev = next(self.parameters()).device
        seed, off = (int(v) for v in self._dropout_tensor(dev).tolist())
        return seed & 0xFFFFFFFFFFFFFFFF, off

    def forward(self, input):
        """Standard forward: input NCHW fp32 (or a list of NCHW tensors to concatenate)."""
        return self._run(input)


class UnetSkipConnectionBlock(nn.Module):
    """Parameter container with the reference block's layer layout (STCGAN/networks.py:79-143).
    Executed only as part of UnetGenerator (the whole U-Net is one fused HIP schedule)."""

    def __init__(self, outer_nc, inner_nc, input_nc=None, submodule=None, outermost=False, innermost=False,
                 norm_layer=nn.BatchNorm2d, use_dropout=False, drop_rate=0.5, no_conv_t=False, activation="tanh",
                 padding_mode="zeros"):
        super().__init__()
        self.outermost = outermost
        self.innermost = innermost
        use_bias = isinstance(norm_layer, nn.InstanceNorm2d)  # always False, as in the reference
        if input_nc is None:
            input_nc = outer_nc
        downconv = nn.Conv2d(input_nc, inner_nc, kernel_size=4, stride=2, padding=1, bias=use_bias,
                             padding_mode=check_padding_mode(padding_mode))
        downrelu = nn.LeakyReLU(0.2, True)
        downnorm = norm_layer(inner_nc)
        uprelu = nn.ReLU(True)
        upnorm = norm_layer(outer_nc)

        def up(cin, cout, bias=True):
            if no_conv_t:  # resize-convolution (src/models/opt_layers.py:39-56, with zero padding)
                return nn.Sequential(nn.Upsample(scale_factor=2, mode="nearest"),
                                     nn.Conv2d(cin, cout, kernel_size=3, stride=1, padding=1, bias=bias))
            return nn.ConvTranspose2d(cin, cout, kernel_size=4, stride=2, padding=1, bias=bias)

        if outermost:
            upconv = up(inner_nc * 2, outer_nc)
            head = get_activation(activation)  # ("none": nothing appended, src/models/unet.py:57-58)
            model = [downconv, submodule, uprelu, upconv] + ([head] if head is not None else [])
        elif innermost:
            upconv = up(inner_nc, outer_nc, bias=use_bias)
            model = [downrelu, downconv, uprelu, upconv, upnorm]
        else:
            upconv = up(inner_nc * 2, outer_nc, bias=use_bias)
            model = [downrelu, downconv, downnorm, submodule, uprelu, upconv, upnorm]
            if use_dropout:  # last, as the reference: indices 0-6 and every state_dict key unchanged
                model.append(nn.Dropout(check_drop_rate(drop_rate)))
        self.model = nn.Sequential(*model)

    def forward(self, x):
        raise RuntimeError("stcgan_amd: UnetSkipConnectionBlock runs only inside UnetGenerator.forward")


class NLayerDiscriminator(_HipNet):
    """PatchGAN discriminator (STCGAN/networks.py:147-192)."""

    kind = "D"

    def __init__(self, in_channels, ndf=64, n_layers=3, norm_layer=nn.BatchNorm2d, use_sigmoid=False,
                 padding_mode="zeros"):
        """padding_mode: "zeros" (default) or "reflect" -- the padding mode of all n_layers + 2 convs (module docstring;
        DESIGN.md section 8i)."""
        super().__init__()
        self.padding_mode = pm = check_padding_mode(padding_mode)
        self.norm_kind = check_norm_layer(norm_layer)
        if use_sigmoid:
            raise NotImplementedError("stcgan_amd: use_sigmoid=True is not on the ST-CGAN path "
                                      "(STCGAN/stcgan.py:39,41)")
        use_bias = isinstance(norm_layer, nn.InstanceNorm2d)
        kw, padw = 4, 1
        sequence = [nn.Conv2d(in_channels, ndf, kernel_size=kw, stride=2, padding=padw, padding_mode=pm),
                    nn.LeakyReLU(0.2, True)]
        nf_mult = 1
        for n in range(1, n_layers):
            nf_mult_prev = nf_mult
            nf_mult = min(2 ** n, 8)
            sequence += [nn.Conv2d(ndf * nf_mult_prev, ndf * nf_mult, kernel_size=kw, stride=2, padding=padw,
                                   bias=use_bias, padding_mode=pm),
                         norm_layer(ndf * nf_mult), nn.LeakyReLU(0.2, True)]
        nf_mult_prev = nf_mult
        nf_mult = min(2 ** n_layers, 8)
        sequence += [nn.Conv2d(ndf * nf_mult_prev, ndf * nf_mult, kernel_size=kw, stride=1, padding=padw,
                               bias=use_bias, padding_mode=pm),
                     norm_layer(ndf * nf_mult), nn.LeakyReLU(0.2, True)]
        sequence += [nn.Conv2d(ndf * nf_mult, 1, kernel_size=kw, stride=1, padding=padw, padding_mode=pm)]
        self.model = nn.Sequential(*sequence)

    def _make_plan(self):
        return engine.DiscPlan(self)

    def forward(self, input):
        return self._run(input)
