"""
    Host-side plumbing between the pytorchcv-style module tree and the HIP kernels: NHWC activation handles, weight
    pre-packing (BN folding, K-major MFMA-ordered weights) cached per module, and one function per C-ABI hot-path call.
    PyTorch is used for device memory and streams only.
"""

__all__ = ['NHWC', 'DTYPES', 'default_dtype', 'set_compute_dtype', 'compute_dtype_of', 'Fp16Guard', 'fp16_overflow_count', 'from_nchw', 'to_nchw', 'ConvRunner',
           'MixConvRunner', 'ghost_dw', 'BnActRunner', 'IBNConvRunner', 'InstNormRunner', 'maxpool2d', 'avgpool2d', 'avgpool2d_pad', 'global_avgpool', 'se_excite', 'se_scale', 'se_forward', 'splat_forward', 'cbam_channel_gate', 'cbam_spatial', 'cbam_forward', 'channel_slice', 'cat_shuffle2', 'act_code',
           'boundary', 'round8', 'source_key', 'channel_concat_into', 'interpolate', 'add', 'hr_fuse', 'hr_fuse_supported', 'classify']

import os
import ctypes
import torch
import torch.nn as nn
import torch.nn.functional as F
from . import _lib
from ._lib import ConvDesc

DTYPES = {"fp32": (0, torch.float32), "bf16": (1, torch.bfloat16), "fp16": (2, torch.float16)}
_CODE_OF_TORCH = {torch.float32: 0, torch.bfloat16: 1, torch.float16: 2}
_NAME_OF_TORCH = {torch.float32: "fp32", torch.bfloat16: "bf16", torch.float16: "fp16"}


def default_dtype() -> str:
    """Process-wide storage / MFMA type of the hot path (env PCV_AMD_DTYPE): "auto" (default), "bf16", "fp16" or "fp32"."""
    d = os.environ.get("PCV_AMD_DTYPE", "auto")
    if d not in DTYPES and d != "auto":
        raise ValueError("PCV_AMD_DTYPE must be one of {}".format(sorted(DTYPES) + ["auto"]))
    return d


def set_compute_dtype(net: nn.Module, dtype: str) -> nn.Module:
    """Select the storage/MFMA type of the hot path for `net`: "auto" (default: the family's 16-bit mode, see
    `compute_dtype_of`), "bf16", "fp16" or "fp32"."""
    if dtype not in DTYPES and dtype != "auto":
        raise ValueError("dtype must be one of {}".format(sorted(DTYPES) + ["auto"]))
    for m in net.modules():
        m._pcv_dtype = dtype
    return net


def stamp_family_dtype(net: nn.Module) -> nn.Module:
    """Give every sub-module of `net` the 16-bit mode its family declares (`pcv_16bit` on the net class), so that "auto" resolves to the
    SAME type whether the whole net or one of its parts (`net.features(x)`, a unit, a block) is called with an NCHW tensor. Called at
    the end of the family's constructor."""
    mode = getattr(net, "pcv_16bit", None)
    if mode is not None:
        for m in net.modules():
            if m is not net:
                m.pcv_16bit = mode
    return net


def compute_dtype_of(module: nn.Module) -> str:
    """The type `module` runs in. "auto" resolves to the module's own 16-bit mode: bf16, except for the net classes that declare
    `pcv_16bit = "fp16"` - the depthwise-separable families (MobileNetV2 / V3, EfficientNet), whose logits stay within the
    north-star 1e-2 of the reference's fp32 forward in fp16 (2e-3 .. 5e-3) but not in bf16 (1.3e-2 .. 2.2e-2: 8 mantissa bits on
    weights that multiply [0, 6]-bounded activations). Same MFMA rate, same bytes; fp16's narrower exponent
    range is covered by the range guard (`Fp16Guard`)."""
    d = getattr(module, "_pcv_dtype", None) or default_dtype()
    if d == "auto":
        d = getattr(module, "pcv_16bit", None) or "bf16"
    return d


class Fp16Guard(object):
    """fp16 range guard around one forward (include/pcv_amd.h, pcv_fp16_guard_begin / _end): every kernel counts the values it
    rounds beyond fp16's range; `finish(y)` - stream-ordered, no host synchronisation, capturable - overwrites the fp32 result `y`
    with NaN when the count moved during the forward. A no-op for bf16 / fp32."""
    __slots__ = ("slot", "device")

    def __init__(self, device, torch_dtype):
        self.slot = None
        self.device = device
        if torch_dtype == torch.float16:
            self.slot = torch.empty(1, dtype=torch.int32, device=device)
            _call(device, "fp16_guard_begin", _ptr(self.slot))

    def finish(self, y: torch.Tensor) -> torch.Tensor:
        if self.slot is not None:
            if y.dtype != torch.float32 or not y.is_contiguous():
                raise RuntimeError("the fp16 guard poisons a contiguous fp32 result")
            _call(self.device, "fp16_guard_end", _ptr(self.slot), _ptr(y), y.numel())
        return y


def fp16_overflow_count(device) -> int:
    """How many threads of this device's context have rounded a value beyond fp16's range so far (synchronises the stream)."""
    n = ctypes.c_uint(0)
    _call(device, "fp16_overflow_count", ctypes.byref(n))
    return int(n.value)


def round8(c: int) -> int:
    return (int(c) + 7) // 8 * 8


def _even(w: int) -> int:
    return (int(w) + 1) // 2 * 2


class NHWC(object):
    """
    An activation on the hot path: `t` is a contiguous device tensor [N, H, wpitch, cpitch]; (H, W, C) is the logical
    extent. The kernels move 16-byte channel chunks, so the physical channel count `cpitch` is C rounded up to a multiple
    of 8 (what the pad channels hold never reaches a logical channel: every weight that would read them is zero-padded).
    The network input is the exception: C <= 4 -> cpitch 4, W -> even (the stem kernel's layout).
    """
    __slots__ = ("t", "N", "H", "W", "C", "wpitch", "cpitch")

    def __init__(self, t, N, H, W, C, wpitch=None, cpitch=None):
        self.t, self.N, self.H, self.W, self.C = t, N, H, W, C
        self.wpitch = W if wpitch is None else wpitch
        self.cpitch = C if cpitch is None else cpitch

    @property
    def dtype(self):
        return self.t.dtype

    @property
    def device(self):
        return self.t.device

    @property
    def dense(self) -> bool:
        """Canonical internal layout: no row padding, channels padded to the next multiple of 8 only."""
        return self.wpitch == self.W and self.cpitch == round8(self.C)

    def size(self, dim=None):
        s = (self.N, self.C, self.H, self.W)        # reported NCHW-style, as callers of the reference expect
        return s if dim is None else s[dim]


class ShapeOnly(object):
    """A dense handle's shape, dtype and (optionally) device for a tensor that does not exist: what `ConvRunner.desc` and `prepare`
    read of their input. The intermediate maps of a fused unit; a model asks with one whether a unit WOULD be covered before its
    input exists (bottleneck_fused's probe)."""
    __slots__ = ("N", "H", "W", "C", "dtype", "wpitch", "cpitch", "device")
    dense = True

    def __init__(self, N, H, W, C, dtype, device=None):
        self.N, self.H, self.W, self.C, self.dtype, self.wpitch, self.cpitch, self.device = N, H, W, C, dtype, W, round8(C), device


def _device_index(device) -> int:
    if device.type != "cuda":
        raise RuntimeError("pytorchcv_amd runs on MI355X (gfx950) only: got a tensor on '{}'. Move the model and the input "
                           "to a CUDA/HIP device; there is no CPU path in this package.".format(device))
    return device.index if device.index is not None else torch.cuda.current_device()


# the current stream's handle without building a torch.cuda.Stream around it: a forward at batch 1 is bound by this host code, and
# every launch asks for the stream
_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None) or (lambda idx: torch.cuda.current_stream(idx).cuda_stream)


def _stream(device) -> ctypes.c_void_p:
    return ctypes.c_void_p(_raw_stream(_device_index(device)))


def _ctx(device):
    return _lib.ctx_for(_device_index(device))


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _call(device, name, *args, accept=()):
    """pcv_<name>(ctx, *args, stream) on `device`'s context and current stream. A non-zero code raises PcvError with the library's
    text, unless it is one of `accept`: those are returned for the caller to handle."""
    ctx = _ctx(device)
    rc = getattr(_lib.lib(), "pcv_" + name)(ctx, *args, _stream(device))
    if rc != 0 and rc not in accept:
        _lib.check(rc, ctx)
    return rc


def _ptrs(r):
    """(packed, scale, shift) pointers of a prepared runner; three Nones for no runner."""
    return (_ptr(r.packed), _ptr(r.scale), _ptr(r.shift)) if r is not None else (None, None, None)


def _check_residual(residual, shape, dtype, detail=False):
    """A skip tensor (None passes) is a dense handle of exactly the output's physical shape and type."""
    if residual is not None and (not residual.dense or residual.dtype != dtype or tuple(residual.t.shape) != shape):
        raise RuntimeError("residual shape/dtype mismatch" + (": {} vs {}".format(tuple(residual.t.shape), shape) if detail else ""))


def _split_batch(N: int, launch, n0: int = 0):
    """Images [n0, n0 + N) through `launch(n0, n1, accept) -> rc`, which hands `accept` to `_call`: one launch addresses less than
    2 GiB, so a range of more than one image may be refused as too large and is then halved, left half first. A single image is
    launched with nothing accepted: any refusal raises in `_call`."""
    n1 = n0 + N
    accept = (_lib.PCV_ERR_TOO_LARGE,) if N > 1 else ()
    if launch(n0, n1, accept) in accept:
        mid = (n0 + n1) // 2
        _split_batch(mid - n0, launch, n0)
        _split_batch(n1 - mid, launch, mid)


def source_key(tensors):
    """Cache key over source tensors (None entries allowed): storage and version, so load_state_dict, .to() and in-place edits change it."""
    return tuple([(t.data_ptr(), t._version) if t is not None else None for t in tensors])


def _bn_fold_sources(bn, C: int, bias=None, what="into the conv epilogue"):
    """The fp32 inputs of pcv_bn_fold over `C` physical channels, pure torch: (gamma, beta, mean, var, bias) of the eval-mode
    BatchNorm2d `bn` (gamma 1, beta 0 without affine parameters) and the convolution's `bias`, each padded to C - gamma, beta, mean
    and bias with 0, var with 1, so that a pad channel gets scale 0 and shift 0. `bn` None: four Nones (scale 1, shift bias)."""
    def padded(t, fill=0.0):
        t = t.detach().float()
        return (F.pad(t, (0, C - t.numel()), value=fill) if t.numel() != C else t).contiguous()
    bias = padded(bias) if bias is not None else None
    if bn is None:
        return None, None, None, None, bias
    if not isinstance(bn, nn.BatchNorm2d):
        raise NotImplementedError("only BatchNorm2d folds {}, got {}".format(what, type(bn).__name__))
    mean = bn.running_mean
    return (padded(bn.weight if bn.weight is not None else torch.ones_like(mean)),
            padded(bn.bias if bn.bias is not None else torch.zeros_like(mean)), padded(mean), padded(bn.running_var, 1.0), bias)


def _fold_bn(dev, bn, C: int, bias=None, what="into the conv epilogue"):
    """(scale, shift): fp32 [C] on `dev` with y = scale * conv + shift = bn(conv + bias) (pcv_bn_fold). The sources it reads are
    temporaries: the caller synchronises the stream once per prepare()."""
    scale = torch.empty(C, dtype=torch.float32, device=dev)
    shift = torch.empty(C, dtype=torch.float32, device=dev)
    g, b, m, v, bias = _bn_fold_sources(bn, C, bias, what)
    _call(dev, "bn_fold", C, _ptr(g), _ptr(b), _ptr(m), _ptr(v), ctypes.c_float(bn.eps if bn is not None else 0.0), _ptr(bias),
          _ptr(scale), _ptr(shift))
    return scale, shift


class _DerivedState(object):
    """What the runners that cache state folded from a module's parameters share: the key the state was built for, and whether the
    state was RECEIVED (parallel.broadcast_packed_state) - then the local fp32 sources are not what it was derived from and nothing
    may be re-derived from them. A subclass names its source tensors (`_sources`) and its refusal text (`_refusal`)."""
    _refusal = None

    def __init__(self):
        self._key = None
        self._foreign = False
        self.packed = self.scale = self.shift = None

    def _sources(self):
        raise NotImplementedError

    def _rebuilding(self):
        """What prepare() calls once its key differs from `_key` (the same key returns before, inline: it is the per-forward path).
        Received state is never rebuilt: a new key would re-derive it from THIS rank's fp32 tensors, which
        broadcast_packed_state never updated - wrong logits with no error - so that raises; the caller re-synchronises the fp32
        state first."""
        if self._foreign:
            raise RuntimeError(self._refusal)

    def adopt_foreign_state(self):
        """Called after the state was overwritten with another rank's (parallel.broadcast_packed_state): the cache key stays valid
        for exactly the configuration it was built for, anything else raises in prepare()."""
        self._foreign = True

    def local_state_restored(self):
        """The fp32 sources are authoritative again (parallel.broadcast_module_state, load_state_dict): re-derive on next use."""
        self._foreign = False
        self._key = None


def _conv_out(d: ConvDesc, H: int, W: int):
    """(Ho, Wo) of the convolution `d` on an H x W map."""
    return ((H + d.pad_t + d.pad_b - d.dil_h * (d.kh - 1) - 1) // d.stride_h + 1,
            (W + d.pad_l + d.pad_r - d.dil_w * (d.kw - 1) - 1) // d.stride_w + 1)


def _require_eval(*runners):
    """BatchNorm is folded into the packed state: a runner (None entries are skipped) whose BatchNorm is in training mode is refused."""
    for r in runners:
        if r is not None and r.bn is not None and r.bn.training:
            raise RuntimeError("pytorchcv_amd is an inference path: call net.eval() first (BatchNorm is folded)")


class LazyNCHW(NHWC):
    """The network input as the caller gave it - fp32 NCHW - seen through the handle interface of its padded NHWC4 view. The stem
    kernel reads the fp32 planes itself (`ConvRunner._stem_from_nchw`, pcv_conv2d_nchw_stem_fused); anything else that asks for
    `.t` gets the converted tensor (pcv_nchw_to_nhwc, once)."""
    __slots__ = ("src", "_conv", "_dtype_name")

    def __init__(self, x: torch.Tensor, dtype: str):
        N, C, H, W = x.shape
        self.src, self._conv, self._dtype_name = x, None, dtype
        self.N, self.H, self.W, self.C = N, H, W, C
        self.wpitch, self.cpitch = _even(W), 4

    @property
    def t(self):
        if self._conv is None:
            self._conv = from_nchw(self.src, self._dtype_name, stem=True).t
        return self._conv

    @property
    def materialized(self) -> bool:
        return self._conv is not None

    @property
    def dtype(self):
        return DTYPES[self._dtype_name][1]

    @property
    def device(self):
        return self.src.device


def network_input(x: torch.Tensor, dtype: str) -> NHWC:
    """Handle of a net's fp32 NCHW input: lazy (the stem kernel reads the planes directly) when the stem layout applies."""
    if x.dim() == 4 and x.shape[1] <= 3 and x.shape[3] % 4 == 0 and STEM_FROM_NCHW:
        return LazyNCHW(x.contiguous().float(), dtype)
    return from_nchw(x, dtype, stem=True)       # (which refuses anything but 4-D)


def from_nchw(x: torch.Tensor, dtype: str, stem: bool = True) -> NHWC:
    """fp32 NCHW -> NHWC handle (pcv_nchw_to_nhwc). With `stem`, C <= 4 is padded to 4 channels and W to even."""
    if x.dim() != 4:
        raise ValueError("expected a 4-D NCHW tensor")
    x = x.contiguous().float()
    N, C, H, W = x.shape
    code, tdt = DTYPES[dtype]
    cp, wp = (4, _even(W)) if C <= 4 and stem else (round8(C), W)
    y = torch.empty((N, H, wp, cp), dtype=tdt, device=x.device)
    _call(x.device, "nchw_to_nhwc", _ptr(x), _ptr(y), N, C, H, W, cp, wp, code)
    return NHWC(y, N, H, W, C, wpitch=wp, cpitch=cp)


def to_nchw(a: NHWC) -> torch.Tensor:
    """NHWC handle -> fp32 NCHW tensor (pcv_nhwc_to_nchw)."""
    if a.wpitch != a.W:
        raise RuntimeError("cannot convert a row-padded input handle back to NCHW")
    y = torch.empty((a.N, a.C, a.H, a.W), dtype=torch.float32, device=a.device)
    _call(a.device, "nhwc_to_nchw", _ptr(a.t), _ptr(y), a.N, a.C, a.H, a.W, a.cpitch, _CODE_OF_TORCH[a.dtype])
    return y


def boundary(module: nn.Module, x, fn, stem: bool = False):
    """Run `fn` on the hot path. An `NHWC` handle passes straight through; an NCHW fp32 tensor (how the reference's
    blocks are called) is converted in and the result converted back, so a block is a drop-in on its own."""
    if isinstance(x, NHWC):
        return fn(x)
    if not torch.is_tensor(x):
        raise TypeError("expected a torch.Tensor or an NHWC handle")
    dtype = compute_dtype_of(module)
    guard = Fp16Guard(x.device, DTYPES[dtype][1])
    y = fn(from_nchw(x, dtype, stem=stem))
    if isinstance(y, tuple):                          # (output, pre-activated input) of the pre-activation blocks: the guard poisons both
        return tuple(guard.finish(to_nchw(v)) if isinstance(v, NHWC) else v for v in y)
    y = to_nchw(y) if isinstance(y, NHWC) else y
    return guard.finish(y) if torch.is_tensor(y) and y.dtype == torch.float32 else y


def act_code(activ) -> int:
    """pcv_act code of an activation module of common/activ.py (None -> 0)."""
    from .models.common.activ import Swish, HSigmoid, HSwish
    if activ is None:
        return 0
    if isinstance(activ, nn.ReLU):
        return 1
    if isinstance(activ, nn.ReLU6):
        return 2
    if isinstance(activ, nn.Sigmoid):
        return 3
    if isinstance(activ, Swish):
        return 4
    if isinstance(activ, HSigmoid):
        return 5
    if isinstance(activ, HSwish):
        return 6
    from .models.ghostnet import GhostHSigmoid
    if isinstance(activ, GhostHSigmoid):                 # clamp(x, 0, 1): PCV_ACT_CLAMP01 (pcv_se_excite / pcv_fc_f32 / pcv_ghost_dw_fused)
        return 7
    raise NotImplementedError("activation {} has no fused MI355X epilogue yet".format(type(activ).__name__))


def _pair(v):
    return (int(v[0]), int(v[1])) if isinstance(v, (tuple, list)) else (int(v), int(v))


class ConvRunner(_DerivedState):
    """
    Packed state of one Conv2d (+ optional BatchNorm2d) for one (device, dtype, input channel pitch): weights in the
    kernel's layout and the folded fp32 scale/shift. Rebuilt whenever a source parameter changes (load_state_dict, .to()).
    """
    _refusal = ("this convolution's packed weights were received by parallel.broadcast_packed_state and would have to be re-packed "
                "(the input's dtype / channel pitch / padding parity or a parameter changed), but this rank's fp32 parameters are "
                "not the source's. Call parallel.broadcast_module_state(net) (or load_state_dict on every rank) before running "
                "another configuration.")

    def __init__(self, conv: nn.Conv2d, bn, pad4=None):
        super(ConvRunner, self).__init__()
        self.conv, self.bn, self.pad4 = conv, bn, pad4
        self._sq_key = None                                                 # squeezed_excite's folded SE layers and their key
        self._sq_w1 = self._sq_b1 = self._sq_w2 = self._sq_b2 = None
        self._bnu_refused = set()                                           # bottleneck_fused: shapes the library refused (on conv1's runner)
        self.depthwise = (conv.groups > 1 and conv.groups == conv.in_channels == conv.out_channels)
        if 1 < conv.groups and not self.depthwise and (conv.in_channels % 8 or conv.out_channels % 8):
            raise NotImplementedError("grouped convolution with channel counts that are not multiples of 8")

    def _phys(self, x_cpitch: int, out_fp32: bool):
        """Physical (Cin, Cout, groups) the kernels run with: logical counts rounded up to multiples of 8, weights and BN
        constants zero-padded accordingly in prepare(). Exceptions: the padded network input of the stem (cpitch 4) keeps the
        logical Cin, and the fp32 classifier output keeps its logical width (ragged epilogue)."""
        c = self.conv
        cin = c.in_channels if x_cpitch == 4 and c.in_channels <= 4 else round8(c.in_channels)
        cout = c.out_channels if out_fp32 else round8(c.out_channels)
        groups = cin if self.depthwise else c.groups
        return cin, cout, groups

    def _sources(self):
        ts = [self.conv.weight, self.conv.bias]
        if self.bn is not None:
            ts += [self.bn.weight, self.bn.bias, self.bn.running_mean, self.bn.running_var]
        return ts

    def _state_key(self, dtype, cpitch, d: ConvDesc):
        # everything the packed blob and the scale/shift arrays depend on besides the source tensors: physical channel counts
        # (the fp32 classifier output keeps its logical width), output type, and the parity of the left padding (the stem
        # packing depends on it; TF-"same" mode changes it per call)
        return (dtype, cpitch, d.Cin, d.Cout, d.groups, d.out_dtype, d.pad_l & 1) + source_key(self._sources())

    def desc(self, x: NHWC, act, post_act, has_res, out_code=None, logits=False, pad4=None) -> ConvDesc:
        """`pad4`: per-call (left, right, top, bottom) padding overriding the block's own (never stored on the runner)."""
        c = self.conv
        kh, kw = _pair(c.kernel_size)
        sh, sw = _pair(c.stride)
        dh, dw = _pair(c.dilation)
        pad4 = pad4 if pad4 is not None else self.pad4
        if pad4 is not None:                    # ConvBlock's 4-tuple padding: (left, right, top, bottom)
            pl, pr, pt, pb = [int(v) for v in pad4]
        else:
            ph, pw = _pair(c.padding)
            pt = pb = ph
            pl = pr = pw
        code = _CODE_OF_TORCH[x.dtype]
        cin, cout, groups = self._phys(x.cpitch, logits)          # `logits`: the fp32 classifier output keeps its logical width
        if x.cpitch != cin and not (x.cpitch == 4 and cin <= 4):
            raise RuntimeError("input handle has {} physical channels, this convolution expects {}".format(x.cpitch, cin))
        d = ConvDesc(N=x.N, H=x.H, W=x.W, Cin=cin, Cout=cout, kh=kh, kw=kw, stride_h=sh, stride_w=sw,
                     pad_t=pt, pad_l=pl, pad_b=pb, pad_r=pr, dil_h=dh, dil_w=dw, groups=groups, act=act, post_act=post_act,
                     has_residual=1 if has_res else 0, dtype=code, out_dtype=code if out_code is None else out_code,
                     x_cpitch=x.cpitch, x_wpitch=x.wpitch)
        return d

    def prepare(self, x: NHWC, d: ConvDesc):
        if isinstance(c_mode := self.conv.padding_mode, str) and c_mode != "zeros":
            raise NotImplementedError("padding_mode {}".format(c_mode))
        key = self._state_key(x.dtype, x.cpitch, d)
        if key == self._key:
            return
        self._rebuilding()
        dev = x.device
        w = self.conv.weight
        if w.device != dev:
            raise RuntimeError("model parameters are on {} but the input is on {}".format(w.device, dev))
        L = _lib.lib()
        nbytes = ctypes.c_size_t(0)
        fn_bytes = L.pcv_dwconv_packed_bytes if self.depthwise else L.pcv_conv_packed_bytes
        if fn_bytes(ctypes.byref(d), ctypes.byref(nbytes)) != 0:
            raise _lib.PcvError(-1, "unsupported convolution configuration: {}".format(
                {f[0]: getattr(d, f[0]) for f in d._fields_}))
        packed = torch.empty((nbytes.value + 15) // 16 * 16, dtype=torch.uint8, device=dev)
        w32 = w.detach().float()
        if w32.dim() == 2:                                          # nn.Linear viewed as a 1x1 convolution
            w32 = w32[:, :, None, None]
        C = d.Cout                                                  # physical output channels
        cin_g = d.Cin // d.groups                                   # physical input channels per group
        if w32.shape[0] != C or w32.shape[1] != cin_g:              # zero rows / columns for the pad channels
            w32 = F.pad(w32, (0, 0, 0, 0, 0, cin_g - w32.shape[1], 0, C - w32.shape[0]))
        w32 = w32.contiguous()
        _call(dev, "dwconv_pack" if self.depthwise else "conv_pack", ctypes.byref(d), _ptr(w32), _ptr(packed))
        scale, shift = _fold_bn(dev, self.bn, C, self.conv.bias)
        torch.cuda.current_stream(dev).synchronize()      # w32 & friends are temporaries; load-time only
        self.packed, self.scale, self.shift, self._key = packed, scale, shift, key

    def adopt_foreign_state(self):
        super(ConvRunner, self).adopt_foreign_state()
        self._sq_key = None

    def run(self, x: NHWC, act=0, residual: NHWC | None = None, post_act=0, out_fp32=False, pad4=None, out=None, gate=None) -> NHWC:
        """`pad4`: explicit (left, right, top, bottom) zero padding for this call (the `F.pad` a unit applies in front of
        a padding-0 convolution, efficientnet.py:108-109,189-190,236-237); it stays inside the kernel's bounds checks."""
        _require_eval(self)
        if isinstance(x, LazyNCHW) and not x.materialized and residual is None and out is None and gate is None and not out_fp32 \
                and post_act == 0 and pad4 is None:
            y = self._stem_from_nchw(x, act, pool=False)
            if y is not None:
                return y
        d = self.desc(x, act, post_act, residual is not None, out_code=0 if out_fp32 else None, logits=out_fp32, pad4=pad4)
        self.prepare(x, d)
        return self._launch(x, d, residual, out, gate)

    def _stem_from_nchw(self, x: "LazyNCHW", act: int, pool: bool):
        """The stem convolution (+ the init block's MaxPool2d(3, 2, 1) with `pool`) straight from the fp32 NCHW image
        (pcv_conv2d_nchw_stem_fused); None when this convolution is not the covered stem shape."""
        if self.depthwise or self.pad4 is not None or x.src.numel() * 4 >= (1 << 31):      # (one launch addresses < 2 GiB: the
            return None                                                                      # converted path splits the batch)
        d = self.desc(x, act, 0, False)
        if not _lib.lib().pcv_conv2d_nchw_stem_supported(ctypes.byref(d), 1 if pool else 0):
            return None
        self.prepare(x, d)
        Ho, Wo = _conv_out(d, x.H, x.W)
        if pool:
            Ho, Wo = (Ho + 2 - 3) // 2 + 1, (Wo + 2 - 3) // 2 + 1
        if Ho <= 0 or Wo <= 0:
            return None
        y = torch.empty((x.N, Ho, Wo, d.Cout), dtype=x.dtype, device=x.device)
        _call(x.device, "conv2d_nchw_stem_fused", ctypes.byref(d), _ptr(x.src), *_ptrs(self), _ptr(y), 1 if pool else 0)
        return NHWC(y, x.N, Ho, Wo, self.conv.out_channels, cpitch=d.Cout)

    def run_maxpool(self, x: NHWC, act: int, k: int, s: int, p: int, ceil_mode: bool = False):
        """This convolution + BN + activation and the MaxPool2d(k, s, p) behind it as ONE launch when covered
        (pcv_conv2d_maxpool_fused: the stem convolution with MaxPool2d(3, 2, 1)); returns the pooled handle or None."""
        if not FUSE_UNITS or self.depthwise or self.pad4 is not None:
            return None
        _require_eval(self)
        if isinstance(x, LazyNCHW) and not x.materialized and (k, s, p) == (3, 2, 1) and not ceil_mode:
            y = self._stem_from_nchw(x, act, pool=True)
            if y is not None:
                return y
        d = self.desc(x, act, 0, False)
        if not _lib.lib().pcv_conv2d_maxpool_supported(ctypes.byref(d), k, s, p, 1 if ceil_mode else 0):
            return None
        self.prepare(x, d)
        Ho, Wo = _conv_out(d, x.H, x.W)
        Hq, Wq = (Ho + 2 * p - k) // s + 1, (Wo + 2 * p - k) // s + 1
        if Hq <= 0 or Wq <= 0:
            return None
        y = torch.empty((x.N, Hq, Wq, d.Cout), dtype=x.dtype, device=x.device)
        _call(x.device, "conv2d_maxpool_fused", ctypes.byref(d), _ptr(x.t), *_ptrs(self), _ptr(y), k, s, p, 1 if ceil_mode else 0)
        return NHWC(y, x.N, Hq, Wq, self.conv.out_channels, cpitch=d.Cout)

    def run_pair(self, x: NHWC, residual: NHWC, act: int, post_act: int, nxt: "ConvRunner", nxt_act: int, gate=None):
        """This convolution (+ residual, + post_act) and the 1x1 convolution `nxt` that consumes its output, as ONE launch
        (pcv_conv1x1_pair_fused): returns (y1, y2), or None when the pair of shapes is not covered by the fused kernel."""
        if not FUSE_UNITS or residual is None or self.depthwise or nxt.depthwise or self.pad4 is not None or nxt.pad4 is not None:
            return None
        _require_eval(self, nxt)
        c = self.conv
        L = _lib.lib()
        d1 = self.desc(x, act, post_act, True)
        d2 = nxt.desc(ShapeOnly(x.N, x.H, x.W, c.out_channels, x.dtype), nxt_act, 0, False)
        supported = L.pcv_conv1x1_pair_gated_supported if gate is not None else L.pcv_conv1x1_pair_supported
        if not supported(ctypes.byref(d1), ctypes.byref(d2)):
            return None
        _check_residual(residual, (x.N, x.H, x.W, d1.Cout), x.dtype)
        if gate is not None and (gate.dtype != torch.float32 or tuple(gate.shape) != (x.N, d1.Cout) or not gate.is_contiguous()):
            raise RuntimeError("gate must be a contiguous fp32 [N, {}] tensor".format(d1.Cout))
        t1 = torch.empty((x.N, x.H, x.W, d1.Cout), dtype=x.dtype, device=x.device)
        t2 = torch.empty((x.N, x.H, x.W, d2.Cout), dtype=x.dtype, device=x.device)
        y1 = NHWC(t1, x.N, x.H, x.W, c.out_channels, cpitch=d1.Cout)
        self.prepare(x, d1)
        nxt.prepare(y1, d2)
        first = (ctypes.byref(d1), ctypes.byref(d2), _ptr(x.t), *_ptrs(self))
        second = (_ptr(residual.t), _ptr(t1), *_ptrs(nxt), _ptr(t2))
        if gate is not None:
            _call(x.device, "conv1x1_pair_gated_fused", *first, _ptr(gate), *second)
        else:
            _call(x.device, "conv1x1_pair_fused", *first, *second)
        return y1, NHWC(t2, x.N, x.H, x.W, nxt.conv.out_channels, cpitch=d2.Cout)

    def run_pair_idconv(self, x: NHWC, x0: NHWC, idr: "ConvRunner", act: int, post_act: int, nxt: "ConvRunner", nxt_act: int):
        """`run_pair` for the first unit of a stage: the skip tensor is `idr` (1x1 convolution + BN, no activation) applied to
        the unit's input `x0`, recomputed inside the fused kernel instead of being written and read back
        (pcv_conv1x1_pair_idconv_fused). Returns (y1, y2), or None when the shapes are not covered."""
        if not FUSE_UNITS or any(r.depthwise or r.pad4 is not None for r in (self, idr, nxt)):
            return None
        _require_eval(self, idr, nxt)
        if not x0.dense or x0.dtype != x.dtype or (x0.N, x0.H, x0.W) != (x.N, x.H, x.W):
            return None
        c = self.conv
        di = idr.desc(x0, 0, 0, False)
        d1 = self.desc(x, act, post_act, True)
        d2 = nxt.desc(ShapeOnly(x.N, x.H, x.W, c.out_channels, x.dtype), nxt_act, 0, False)
        if not _lib.lib().pcv_conv1x1_pair_idconv_supported(ctypes.byref(di), ctypes.byref(d1), ctypes.byref(d2)):
            return None
        t1 = torch.empty((x.N, x.H, x.W, d1.Cout), dtype=x.dtype, device=x.device)
        t2 = torch.empty((x.N, x.H, x.W, d2.Cout), dtype=x.dtype, device=x.device)
        y1 = NHWC(t1, x.N, x.H, x.W, c.out_channels, cpitch=d1.Cout)
        idr.prepare(x0, di)
        self.prepare(x, d1)
        nxt.prepare(y1, d2)
        _call(x.device, "conv1x1_pair_idconv_fused", ctypes.byref(di), ctypes.byref(d1), ctypes.byref(d2), _ptr(x0.t), *_ptrs(idr),
              _ptr(x.t), *_ptrs(self), _ptr(t1), *_ptrs(nxt), _ptr(t2))
        return y1, NHWC(t2, x.N, x.H, x.W, nxt.conv.out_channels, cpitch=d2.Cout)

    def _launch(self, x: NHWC, d: ConvDesc, residual, out=None, gate=None):
        """`out` = (tensor [N, Ho, Wo, Ctot], channel offset): write the result into that channel slice of a wider
        (concatenation) buffer instead of a fresh tensor - `torch.cat((identity, x), dim=1)` without the copy."""
        c = self.conv
        Ho, Wo = _conv_out(d, x.H, x.W)
        if Ho <= 0 or Wo <= 0:
            raise RuntimeError("convolution output would be empty")
        out_dt = torch.float32 if d.out_dtype == 0 else x.dtype
        if out is not None:
            buf, coff = out
            if self.depthwise or tuple(buf.shape[:3]) != (x.N, Ho, Wo) or buf.dtype != out_dt or not buf.is_contiguous() or \
                    coff % 8 != 0 or c.out_channels % 8 != 0 or coff + c.out_channels > buf.shape[3] or buf.device != x.device:
                raise RuntimeError("bad concatenation slice for a convolution output (channel counts must be multiples of 8)")
            d.y_cpitch = int(buf.shape[3])
            y = buf[:, :, :, coff:]                 # a view: its data_ptr is the first element of the slice
        else:
            y = torch.empty((x.N, Ho, Wo, d.Cout), dtype=out_dt, device=x.device)          # d.Cout: physical channels
        _check_residual(residual, (x.N, Ho, Wo, d.Cout), x.dtype, detail=True)
        if gate is not None:
            if self.depthwise or gate.dtype != torch.float32 or tuple(gate.shape) != (x.N, d.Cout) or not gate.is_contiguous():
                raise RuntimeError("gate must be a contiguous fp32 [N, {}] tensor of a dense convolution".format(d.Cout))

        def launch(n0, n1, accept):
            d.N = n1 - n0
            args = (ctypes.byref(d), _ptr(x.t[n0:n1]), *_ptrs(self))
            rest = (_ptr(residual.t[n0:n1]) if residual is not None else None, _ptr(y[n0:n1]))
            if gate is not None:
                return _call(x.device, "conv2d_gated_fused", *args, _ptr(gate[n0:n1]), *rest, accept=accept)
            return _call(x.device, "dwconv2d_fused" if self.depthwise else "conv2d_fused", *args, *rest, accept=accept)
        _split_batch(x.N, launch)
        return None if out is not None else NHWC(y, x.N, Ho, Wo, c.out_channels, cpitch=d.Cout)

    def squeezed_excite(self, z: NHWC, w1, b1, w2, b2, mid_act: int, out_act: int) -> torch.Tensor:
        """SE gate of `SEBlock(BN(conv(z)))` for a 1x1 stride-1 convolution WITHOUT activation, computed before the convolution
        runs: mean_hw(BN(conv(z))) = BN(conv(mean_hw(z))) (both affine), and the first excitation layer absorbs that map:
        mid = mid_act(W1 . (S W mean + shift) + b1) = mid_act((W1 S W) . mean + (W1 shift + b1)) with the [M, Cin] product
        folded once at load time. Two small fp32 layers on the squeezed INPUT: gate fp32 [N, Cout_physical]."""
        c = self.conv
        if self.depthwise or c.groups != 1 or tuple(_pair(c.kernel_size)) != (1, 1) or tuple(_pair(c.stride)) != (1, 1) or \
                self.pad4 is not None or tuple(_pair(c.padding)) != (0, 0):
            raise RuntimeError("squeezed_excite needs a plain 1x1 stride-1 convolution")
        d = self.desc(z, 0, 0, False)
        self.prepare(z, d)                                   # scale / shift of the folded BatchNorm (+ bias)
        key = ("sq", self._key) + source_key((w1, w2, b1, b2))
        if self._sq_key != key:
            Cl, CP = c.out_channels, d.Cout
            w = c.weight.detach().float().reshape(Cl, -1)
            w = F.pad(w, (0, d.Cin - w.shape[1], 0, CP - Cl)) * self.scale[:, None]       # [CP, Cin]: BN scale folded into the rows
            w1p = F.pad(w1.float(), (0, CP - Cl))                                          # [M, CP]
            self._sq_w1 = (w1p @ w).contiguous()                                           # [M, Cin]
            self._sq_b1 = (w1p @ self.shift + b1.float()).contiguous()
            self._sq_w2 = F.pad(w2.float(), (0, 0, 0, CP - Cl)).contiguous()               # [CP, M]
            self._sq_b2 = F.pad(b2.float(), (0, CP - Cl)).contiguous()
            self._sq_key = key
        M = self._sq_w1.shape[0]
        mean = torch.empty((z.N, d.Cin), dtype=torch.float32, device=z.device)
        _call(z.device, "se_squeeze", _ptr(z.t), _ptr(mean), z.N, z.H * z.W, d.Cin, _CODE_OF_TORCH[z.dtype])
        mid = torch.empty((z.N, M), dtype=torch.float32, device=z.device)
        gate = torch.empty((z.N, d.Cout), dtype=torch.float32, device=z.device)
        _call(z.device, "fc_f32", _ptr(mean), _ptr(self._sq_w1), _ptr(self._sq_b1), _ptr(mid), z.N, d.Cin, M, mid_act)
        _call(z.device, "fc_f32", _ptr(mid), _ptr(self._sq_w2), _ptr(self._sq_b2), _ptr(gate), z.N, M, d.Cout, out_act)
        return gate


class MixConvRunner(ConvRunner):
    """
    Packed state of one depthwise MixConv (+ BatchNorm2d): the G depthwise Conv2d modules of a reference MixConv (mixnet.py:59-73,
    windows 3, 5, ..., 3 + 2 (G - 1), padding k // 2) as ONE blob (pcv_mixconv_pack) and the folded fp32 scale / shift of the block's
    BatchNorm over all channels. One launch per block (pcv_mixconv2d_fused): every group reads and writes its channel slice in place.
    A ConvRunner as far as the packed-state plumbing goes (cache key, parallel.broadcast_packed_state).
    """
    _refusal = ("this MixConv's packed weights were received by parallel.broadcast_packed_state and would have to be "
                "re-packed: call parallel.broadcast_module_state(net) first")

    def __init__(self, convs, bn):
        self.convs = list(convs)
        G = len(self.convs)
        for g, c in enumerate(self.convs):
            k = 3 + 2 * g
            if _pair(c.kernel_size) != (k, k) or _pair(c.padding) != (k // 2, k // 2) or _pair(c.dilation) != (1, 1) or \
                    c.groups != c.in_channels or c.in_channels != c.out_channels or _pair(c.stride) != _pair(self.convs[0].stride) or \
                    c.padding_mode != "zeros":
                raise NotImplementedError("MixConv on the MI355X path: depthwise groups with windows 3, 5, ... and padding k // 2, "
                                          "got group {} = {}".format(g, c))
        super(MixConvRunner, self).__init__(self.convs[0], bn)      # `conv`: group 0, whose stride is every group's
        self.depthwise = True                                       # (also where group 0 is a single channel: groups == 1)
        if not 2 <= G <= 5:
            raise NotImplementedError("MixConv with {} kernels: the MI355X path takes 2 to 5".format(G))
        self.channels = sum(c.out_channels for c in self.convs)
        self.kernels = (ctypes.c_int * G)(*[3 + 2 * g for g in range(G)])

    def _sources(self):
        ts = []
        for c in self.convs:
            ts += [c.weight, c.bias]
        if self.bn is not None:
            ts += [self.bn.weight, self.bn.bias, self.bn.running_mean, self.bn.running_var]
        return ts

    def _state_key(self, dtype, cpitch, d: ConvDesc):
        return (dtype, d.Cin) + source_key(self._sources())

    def desc(self, x: NHWC, act: int) -> ConvDesc:
        C, G = self.channels, len(self.convs)
        if not x.dense or x.C != C or x.cpitch != C:
            raise RuntimeError("MixConv expects a dense handle of {} channels (a multiple of 8), got {} / pitch {}".format(C, x.C, x.cpitch))
        k = 3 + 2 * (G - 1)
        s = _pair(self.conv.stride)
        code = _CODE_OF_TORCH[x.dtype]
        return ConvDesc(N=x.N, H=x.H, W=x.W, Cin=C, Cout=C, kh=k, kw=k, stride_h=s[0], stride_w=s[1], pad_t=k // 2, pad_l=k // 2,
                        pad_b=k // 2, pad_r=k // 2, dil_h=1, dil_w=1, groups=C, act=act, post_act=0, has_residual=0, dtype=code,
                        out_dtype=code, x_cpitch=C, x_wpitch=x.W)

    def prepare(self, x: NHWC, d: ConvDesc):
        key = self._state_key(x.dtype, x.cpitch, d)
        if key == self._key:
            return
        self._rebuilding()
        dev, C, G = x.device, d.Cin, len(self.convs)
        if self.conv.weight.device != dev:
            raise RuntimeError("model parameters are on {} but the input is on {}".format(self.conv.weight.device, dev))
        L = _lib.lib()
        nbytes = ctypes.c_size_t(0)
        if L.pcv_mixconv_packed_bytes(ctypes.byref(d), self.kernels, G, ctypes.byref(nbytes)) != 0:
            raise _lib.PcvError(-1, "unsupported MixConv configuration: {}".format((L.pcv_last_error(None) or b"").decode()))
        packed = torch.empty((nbytes.value + 15) // 16 * 16, dtype=torch.uint8, device=dev)
        ws = [c.weight.detach().float().contiguous() for c in self.convs]
        _call(dev, "mixconv_pack", ctypes.byref(d), self.kernels, G, (ctypes.c_void_p * G)(*[w.data_ptr() for w in ws]), _ptr(packed))
        bias = None
        if any(c.bias is not None for c in self.convs):
            bias = torch.cat([c.bias.detach().float() if c.bias is not None else torch.zeros(c.out_channels, device=dev)
                              for c in self.convs])
        scale, shift = _fold_bn(dev, self.bn, C, bias)
        torch.cuda.current_stream(dev).synchronize()      # the fp32 copies are temporaries; load-time only
        self.packed, self.scale, self.shift, self._key = packed, scale, shift, key

    def run(self, x: NHWC, act: int = 0) -> NHWC:
        _require_eval(self)
        d = self.desc(x, act)
        self.prepare(x, d)
        Ho, Wo = _conv_out(d, x.H, x.W)
        y = torch.empty((x.N, Ho, Wo, d.Cout), dtype=x.dtype, device=x.device)

        def launch(n0, n1, accept):
            d.N = n1 - n0
            return _call(x.device, "mixconv2d_fused", ctypes.byref(d), self.kernels, len(self.convs), _ptr(x.t[n0:n1]), *_ptrs(self),
                         _ptr(y[n0:n1]), accept=accept)
        _split_batch(x.N, launch)
        return NHWC(y, x.N, Ho, Wo, self.channels, cpitch=d.Cout)


def ghost_dw(runner: ConvRunner, m: NHWC, act: int, residual: NHWC | None = None) -> NHWC:
    """The second half of a ghost module as ONE launch (pcv_ghost_dw_fused; reference ghostnet.py:57-60 and, with `residual`, the
    `x + identity` of ghostnet.py:167-174): y = cat((m, act(bn(dw3x3(m)))), channels) + residual, dense [N, H, W, 2 Cm].
    `runner` is the plain depthwise ConvRunner of `cheap_conv` (its packed taps and folded BatchNorm are used as they are, at the
    pitch round8(Cm)); `m` the main convolution's output with Cm logical channels. Shapes the kernel does not take raise
    NotImplementedError with the library's text."""
    _require_eval(runner)
    c = runner.conv
    Cm = c.out_channels
    if not runner.depthwise or c.in_channels != Cm:
        raise NotImplementedError("ghost module: the cheap convolution must be depthwise with as many outputs as inputs, got {}".format(c))
    if not m.dense or m.C != Cm:
        raise RuntimeError("ghost module: expected a dense handle of {} channels, got {} / pitch {} / row pitch {}".format(
            Cm, m.C, m.cpitch, m.wpitch))
    dp = runner.desc(m, act, 0, False)                  # the physical (round8) descriptor the taps and scale / shift are packed for
    d = runner.desc(m, act, 0, residual is not None)
    d.Cin = d.Cout = d.groups = Cm                      # the launch's: logical width, pitch round8(Cm)
    d.y_cpitch = 2 * Cm
    L = _lib.lib()
    if not L.pcv_ghost_supported(ctypes.byref(d)):
        raise NotImplementedError("ghost module ({} + {} channels on a {}x{} map) is not covered by the MI355X path: {}".format(
            Cm, Cm, m.H, m.W, (L.pcv_last_error(None) or b"").decode()))
    runner.prepare(m, dp)
    _check_residual(residual, (m.N, m.H, m.W, 2 * Cm), m.dtype, detail=True)
    y = torch.empty((m.N, m.H, m.W, 2 * Cm), dtype=m.dtype, device=m.device)

    def launch(n0, n1, accept):
        d.N = n1 - n0
        return _call(m.device, "ghost_dw_fused", ctypes.byref(d), _ptr(m.t[n0:n1]), *_ptrs(runner),
                     _ptr(residual.t[n0:n1]) if residual is not None else None, _ptr(y[n0:n1]), accept=accept)
    _split_batch(m.N, launch)
    return NHWC(y, m.N, m.H, m.W, 2 * Cm, cpitch=2 * Cm)


def _pool_out(n: int, k: int, s: int, p: int, ceil_mode: bool) -> int:
    o = (n + 2 * p - k + (s - 1 if ceil_mode else 0)) // s + 1
    if ceil_mode and (o - 1) * s >= n + p:
        o -= 1
    return o


def channel_slice(x: NHWC, offset: int, count: int) -> NHWC:
    """x[:, offset:offset+count] (channel dimension) as a canonical handle of its own (torch.chunk / split)."""
    if x.wpitch != x.W or offset < 0 or offset + count > x.C:
        raise RuntimeError("bad channel slice")
    cp = round8(count)
    y = torch.empty((x.N, x.H, x.W, cp), dtype=x.dtype, device=x.device)
    _call(x.device, "channel_slice", _ptr(x.t), _ptr(y), x.N * x.H * x.W, count, offset, x.cpitch, cp, _CODE_OF_TORCH[x.dtype])
    return NHWC(y, x.N, x.H, x.W, count, cpitch=cp)


def channel_concat_into(x: NHWC, buf: torch.Tensor, coff: int):
    """buf[:, :, :, coff:coff + x.C] = x (the copy form of torch.cat along channels; a convolution writes its slice itself
    through `ConvRunner.run(out=(buf, coff))`). x.C and coff must be multiples of 8."""
    if x.wpitch != x.W or x.C % 8 or coff % 8 or tuple(buf.shape[:3]) != (x.N, x.H, x.W) or buf.dtype != x.dtype or \
            coff + x.C > buf.shape[3] or not buf.is_contiguous():
        raise RuntimeError("channel concatenation needs channel counts / offsets that are multiples of 8 and equal maps")
    _call(x.device, "channel_concat", _ptr(x.t), _ptr(buf), x.N * x.H * x.W, x.C, x.cpitch, int(buf.shape[3]), coff,
          _CODE_OF_TORCH[x.dtype])


def interpolate(x: NHWC, out_size, bilinear: bool, align_corners: bool) -> NHWC:
    """F.interpolate(size=out_size, mode="bilinear" | "nearest", align_corners) on an NHWC handle (pcv_interpolate)."""
    if not x.dense:
        raise RuntimeError("interpolation on a padded handle")
    Ho, Wo = int(out_size[0]), int(out_size[1])
    y = torch.empty((x.N, Ho, Wo, x.cpitch), dtype=x.dtype, device=x.device)
    _call(x.device, "interpolate", _ptr(x.t), _ptr(y), x.N, x.H, x.W, x.cpitch, Ho, Wo, 1 if bilinear else 0,
          1 if align_corners else 0, _CODE_OF_TORCH[x.dtype])
    return NHWC(y, x.N, Ho, Wo, x.C, cpitch=x.cpitch)


def add(a: NHWC, b: NHWC, post_act: int = 0) -> NHWC:
    """post_act(a + b) as one pass (pcv_se_scale with a unit gate): the fallback of a summing `Concurrent` whose branch does not
    end in a convolution (a convolution takes the running sum as its epilogue residual instead)."""
    if a.t.shape != b.t.shape or a.dtype != b.dtype or not a.dense:
        raise RuntimeError("add: operands do not match")
    return se_scale(a, torch.ones((a.N, a.cpitch), dtype=torch.float32, device=a.device), b, post_act)


def hr_fuse_supported(shifts, N: int, H: int, W: int, cpitch: int, act: int, dtype) -> bool:
    """Whether `hr_fuse` takes this shape (pcv_hr_fuse_supported: host arithmetic, no context); the reason for a refusal is
    the library's pcv_last_error(None)."""
    sh = (ctypes.c_int * len(shifts))(*[int(s) for s in shifts])
    return bool(_lib.lib().pcv_hr_fuse_supported(len(shifts), sh, N, H, W, cpitch, act, _CODE_OF_TORCH[dtype]))


def hr_fuse(sources, shifts, act: int = 0) -> NHWC:
    """HRNet's exchange for one output branch as ONE launch (pcv_hr_fuse; reference hrnet.py:40-47,126-134):
    y[n, h, w] = act(sum_t sources[t][n, h >> shifts[t], w >> shifts[t]]), fp32 sum in list order, rounded once. A source with shift
    s is the dense handle of the map H >> s x W >> s (an UpSamplingBlock's 1x1 output, never upsampled); the output size is that of
    the shift-0 sources, or source 0 scaled up when there is none. Handles that do not fit together and shapes the kernel refuses
    raise RuntimeError."""
    sources, shifts = list(sources), [int(s) for s in shifts]
    if not sources or len(sources) != len(shifts) or not all(isinstance(s, NHWC) for s in sources):
        raise RuntimeError("hr_fuse: expected as many NHWC handles as shifts, got {} / {}".format(len(sources), len(shifts)))
    if any(s < 0 or s > 8 for s in shifts):
        raise RuntimeError("hr_fuse: shifts out of range: {}".format(shifts))
    a = sources[0]
    N, C, H, W = a.N, a.C, a.H << shifts[0], a.W << shifts[0]
    for s, k in zip(sources, shifts):
        if not s.dense or s.dtype != a.dtype or s.device != a.device or (s.N, s.C) != (N, C) or \
                (s.H << k, s.W << k) != (H, W) or tuple(s.t.shape) != (N, s.H, s.W, s.cpitch):
            raise RuntimeError("hr_fuse: source [{}, {}, {}, {}] (pitch {} / row pitch {}, {}) at shift {} does not fit the output "
                               "[{}, {}, {}, {}] ({})".format(s.N, s.H, s.W, s.C, s.cpitch, s.wpitch, s.dtype, k, N, H, W, C, a.dtype))
    y = torch.empty((N, H, W, a.cpitch), dtype=a.dtype, device=a.device)
    src = (ctypes.c_void_p * len(sources))(*[s.t.data_ptr() for s in sources])
    sh = (ctypes.c_int * len(shifts))(*shifts)
    try:
        _call(a.device, "hr_fuse", src, sh, len(sources), _ptr(y), N, H, W, a.cpitch, int(act), _CODE_OF_TORCH[a.dtype])
    except _lib.PcvError as e:
        raise RuntimeError("hr_fuse: the kernel refuses {} source(s) with shifts {} on [{}, {}, {}, {}]: {}".format(
            len(sources), shifts, N, H, W, C, e))
    return NHWC(y, N, H, W, C, cpitch=a.cpitch)


def cat_shuffle2(a: NHWC, b: NHWC, half: int) -> NHWC:
    """channel_shuffle(torch.cat((a[:, :half], b[:, :half]), dim=1), groups=2) in one pass."""
    if (a.N, a.H, a.W) != (b.N, b.H, b.W) or a.dtype != b.dtype or a.wpitch != a.W or b.wpitch != b.W or half > a.C or half > b.C:
        raise RuntimeError("cat/shuffle operands do not match")
    cp = round8(2 * half)
    y = torch.empty((a.N, a.H, a.W, cp), dtype=a.dtype, device=a.device)
    _call(a.device, "channel_interleave2", _ptr(a.t), _ptr(b.t), _ptr(y), a.N * a.H * a.W, half, a.cpitch, b.cpitch, cp,
          _CODE_OF_TORCH[a.dtype])
    return NHWC(y, a.N, a.H, a.W, 2 * half, cpitch=cp)


def maxpool2d(x: NHWC, k: int, s: int, p: int, ceil_mode: bool = False) -> NHWC:
    if not x.dense:
        raise RuntimeError("max-pool on a padded handle")
    Ho, Wo = _pool_out(x.H, k, s, p, ceil_mode), _pool_out(x.W, k, s, p, ceil_mode)
    if Ho <= 0 or Wo <= 0:
        raise RuntimeError("MaxPool2d({}, {}, {}) output of a {}x{} map would be empty".format(k, s, p, x.H, x.W))
    y = torch.empty((x.N, Ho, Wo, x.cpitch), dtype=x.dtype, device=x.device)
    _call(x.device, "maxpool2d", _ptr(x.t), _ptr(y), x.N, x.H, x.W, x.cpitch, k, s, p, 1 if ceil_mode else 0, _CODE_OF_TORCH[x.dtype])
    return NHWC(y, x.N, Ho, Wo, x.C, cpitch=x.cpitch)


def avgpool2d(x: NHWC, k: int, s: int, out_fp32: bool = False) -> NHWC:
    """`out_fp32`: write the pooled map in fp32 (the classifier input: see FP32_HEAD)."""
    if not x.dense:
        raise RuntimeError("avg-pool on a padded handle")
    if k > x.H or k > x.W:
        raise RuntimeError("AvgPool2d kernel {} larger than the {}x{} map".format(k, x.H, x.W))
    Ho, Wo = (x.H - k) // s + 1, (x.W - k) // s + 1
    y = torch.empty((x.N, Ho, Wo, x.cpitch), dtype=torch.float32 if out_fp32 else x.dtype, device=x.device)
    code = _CODE_OF_TORCH[x.dtype]
    _call(x.device, "avgpool2d", _ptr(x.t), _ptr(y), x.N, x.H, x.W, x.cpitch, k, s, code, 0 if out_fp32 else code)
    return NHWC(y, x.N, Ho, Wo, x.C, cpitch=x.cpitch)


def avgpool2d_pad(x: NHWC, k: int, s: int, p: int = 0, ceil_mode: bool = False, count_include_pad: bool = True) -> NHWC:
    """nn.AvgPool2d(k, s, p, ceil_mode, count_include_pad) on an NHWC handle (pcv_avgpool2d_pad): ResNeSt's padded 3x3 pool and
    its ceil-mode identity pool (reference resnesta.py:45-48,138-142)."""
    if not x.dense:
        raise RuntimeError("avg-pool on a padded handle")
    Ho, Wo = _pool_out(x.H, k, s, p, ceil_mode), _pool_out(x.W, k, s, p, ceil_mode)
    if Ho <= 0 or Wo <= 0:
        raise RuntimeError("AvgPool2d({}, {}, {}) output of a {}x{} map would be empty".format(k, s, p, x.H, x.W))
    y = torch.empty((x.N, Ho, Wo, x.cpitch), dtype=x.dtype, device=x.device)
    code = _CODE_OF_TORCH[x.dtype]
    _call(x.device, "avgpool2d_pad", _ptr(x.t), _ptr(y), x.N, x.H, x.W, x.cpitch, k, s, p, 1 if ceil_mode else 0,
          1 if count_include_pad else 0, code, code)
    return NHWC(y, x.N, Ho, Wo, x.C, cpitch=x.cpitch)


# The classifier head runs in fp32: the `final_pool` of a net writes fp32 pooled features and the classifier behind it (Linear /
# 1x1 convolutions on the 1 x 1 map: 2-3 MMAC per image, nothing) runs on the exact-f32 MFMA path with fp32 weights. Measured on the
# golden fixtures (tests/tools/bf16_drift.py): everything in front of the global pool is averaged over the 49 positions of the last
# map, the rounding of the pooled vector and of the classifier weights is not - those two roundings alone were 43 % of the
# noise power of ResNet-50's bf16 logits (max |d| vs the fp32 reference 1.1e-2 -> 8.1e-3, ResNeXt-101 1.3e-2 -> 8.9e-3).
FP32_HEAD = os.environ.get("PCV_AMD_FP32_HEAD", "1") != "0"
STEM_FROM_NCHW = os.environ.get("PCV_AMD_STEM_NCHW", "1") != "0"     # the stem reads the fp32 NCHW input itself (0: layout kernel first)


# Unit-level fusions (pcv_mbconv_fused, pcv_conv1x1_pair_fused) can be switched off to time the per-layer kernels on their own
# (bench.py's roofline pass over the depthwise kernel class does that); the results are the same either way.
FUSE_UNITS = os.environ.get("PCV_AMD_FUSE_UNITS", "1") != "0"


def mbconv_fused(exp, exp_act: int, dw, dw_act: int, proj, proj_act: int, x: NHWC, residual, post_act: int):
    """[expand 1x1 ->] depthwise 3x3 -> project 1x1 (+ residual) as ONE launch (pcv_mbconv_fused); `exp`, `dw`, `proj` are
    the ConvRunners of the three blocks (`exp` may be None). Returns the unit output, or None when the triple of shapes is
    not covered by the fused kernel (the caller then issues the separate launches)."""
    if not FUSE_UNITS or not x.dense or not dw.depthwise or proj.depthwise or (exp is not None and exp.depthwise):
        return None
    if any(r is not None and r.pad4 is not None for r in (exp, dw, proj)):
        return None
    _require_eval(exp, dw, proj)
    cur = x
    d_exp = None
    if exp is not None:
        d_exp = exp.desc(x, exp_act, 0, False)
        cur = ShapeOnly(x.N, x.H, x.W, exp.conv.out_channels, x.dtype, x.device)
    d_dw = dw.desc(cur, dw_act, 0, False)
    Ho, Wo = _conv_out(d_dw, cur.H, cur.W)
    mid = ShapeOnly(x.N, Ho, Wo, dw.conv.out_channels, x.dtype, x.device)
    d_proj = proj.desc(mid, proj_act, post_act, residual is not None)
    if not _lib.lib().pcv_mbconv_supported(ctypes.byref(d_exp) if d_exp is not None else None, ctypes.byref(d_dw), ctypes.byref(d_proj)):
        return None
    Cout = d_proj.Cout                                           # physical
    _check_residual(residual, (x.N, Ho, Wo, Cout), x.dtype)
    # weights / BN constants are packed through the runners' own caches (dense handles of the right shape and dtype)
    if exp is not None:
        exp.prepare(x, d_exp)
    dw.prepare(cur, d_dw)
    proj.prepare(mid, d_proj)
    y = torch.empty((x.N, Ho, Wo, Cout), dtype=x.dtype, device=x.device)
    _call(x.device, "mbconv_fused", ctypes.byref(d_exp) if d_exp is not None else None, ctypes.byref(d_dw), ctypes.byref(d_proj),
          _ptr(x.t), *_ptrs(exp), *_ptrs(dw), *_ptrs(proj), _ptr(residual.t) if residual is not None else None, _ptr(y))
    return NHWC(y, x.N, Ho, Wo, proj.conv.out_channels, cpitch=Cout)


def bottleneck_fused(c1, act1: int, c2, act2: int, c3, act3: int, x: NHWC, post_act: int, idr=None, probe=False):
    """A whole bottleneck unit - 1x1 -> 3x3 -> 1x1, + skip, + post_act - as ONE launch (pcv_bottleneck_fused): `c1`, `c2`, `c3` are
    the ConvRunners of the body's blocks; the skip is `x` itself or, with `idr` (the runner of the unit's `identity_conv`), that
    convolution of `x`, computed inside the launch. Returns the unit output, or None when the unit is not covered (the caller then
    issues the separate launches). `probe`: `x` is a ShapeOnly; returns whether a dense input of that shape would be covered."""
    runners = (c1, c2, c3) + ((idr,) if idr is not None else ())
    if not FUSE_UNITS or not x.dense or any(r.depthwise or r.pad4 is not None for r in runners):
        return None
    _require_eval(*runners)
    # every bottleneck unit of every stage asks on every forward, and an eager forward at batch 1 is bound by this host code: what the
    # library refused once for a shape is not asked again (three descriptors and a call per unit; a refusal only ever means the
    # separate launches, so a remembered one is safe even if pcv_set_tuning("bnu", ...) changes later)
    key = (x.N, x.H, x.W, x.dtype, x.cpitch, act1, act2, act3, post_act, idr is not None)
    refused = c1._bnu_refused
    if key in refused:
        return None
    d1 = c1.desc(x, act1, 0, False)
    t1 = ShapeOnly(x.N, x.H, x.W, c1.conv.out_channels, x.dtype, x.device)
    d2 = c2.desc(t1, act2, 0, False)
    if _conv_out(d2, x.H, x.W) != (x.H, x.W):
        refused.add(key)
        return None
    t2 = ShapeOnly(x.N, x.H, x.W, c2.conv.out_channels, x.dtype, x.device)
    d3 = c3.desc(t2, act3, post_act, True)
    di = idr.desc(x, 0, 0, False) if idr is not None else None
    if not _lib.lib().pcv_bottleneck_supported(ctypes.byref(d1), ctypes.byref(d2), ctypes.byref(d3),
                                               ctypes.byref(di) if di is not None else None):
        refused.add(key)
        return None
    if probe:
        return True
    c1.prepare(x, d1)
    c2.prepare(t1, d2)
    c3.prepare(t2, d3)
    if idr is not None:
        idr.prepare(x, di)
    y = torch.empty((x.N, x.H, x.W, d3.Cout), dtype=x.dtype, device=x.device)
    _call(x.device, "bottleneck_fused", ctypes.byref(d1), ctypes.byref(d2), ctypes.byref(d3), ctypes.byref(di) if di is not None else None,
          _ptr(x.t), *_ptrs(c1), *_ptrs(c2), *_ptrs(c3), *_ptrs(idr), _ptr(y))
    return NHWC(y, x.N, x.H, x.W, c3.conv.out_channels, cpitch=d3.Cout)


class BnActRunner(_DerivedState):
    """Eval-mode BatchNorm2d + activation as one elementwise launch (pcv_bn_act); scale/shift are folded once and refolded
    when the parameters change (same cache rule as ConvRunner; `packed` stays None)."""
    _refusal = ("this BatchNorm's folded constants were received by parallel.broadcast_packed_state and its local "
                "parameters changed: call parallel.broadcast_module_state(net) first")

    _sq_key = None      # (no SE squeeze map folds through a BatchNorm: see ConvRunner.squeezed_excite; parallel asks every runner)

    def __init__(self, bn):
        super(BnActRunner, self).__init__()
        self.bn = bn

    def _sources(self):
        return [self.bn.weight, self.bn.bias, self.bn.running_mean, self.bn.running_var]

    def _state_key(self):
        return source_key(self._sources())

    def prepare(self, x: NHWC):
        key = self._state_key()
        if key == self._key:
            return
        self._rebuilding()
        bn, dev = self.bn, x.device
        if isinstance(bn, nn.BatchNorm2d) and bn.running_mean.device != dev:
            raise RuntimeError("model parameters are on {} but the input is on {}".format(bn.running_mean.device, dev))
        scale, shift = _fold_bn(dev, bn, round8(bn.num_features), what="to scale/shift")
        torch.cuda.current_stream(dev).synchronize()
        self.scale, self.shift, self._key = scale, shift, key

    def run(self, x: NHWC, act: int) -> NHWC:
        _require_eval(self)
        if x.wpitch != x.W:
            raise RuntimeError("BatchNorm + activation on a row-padded handle")
        if x.C != self.bn.num_features:
            raise RuntimeError("BatchNorm2d expects {} channels, got {}".format(self.bn.num_features, x.C))
        self.prepare(x)
        CP = round8(x.C)                        # physical channels processed (x may also be the prefix of a wider concat buffer)
        y = torch.empty((x.N, x.H, x.W, CP), dtype=x.dtype, device=x.device)
        _call(x.device, "bn_act", _ptr(x.t), _ptr(self.scale), _ptr(self.shift), _ptr(y), x.N * x.H * x.W, CP, x.cpitch, act,
              _CODE_OF_TORCH[x.dtype])
        return NHWC(y, x.N, x.H, x.W, x.C, cpitch=CP)


class IBNConvRunner(ConvRunner):
    """A convolution whose output goes through IBN (common/norm.py `IBN`): the BatchNorm2d of the second channel section folds into
    the epilogue as usual, the InstanceNorm2d section leaves the convolution untouched - scale 1, shift 0 (+ the convolution's
    bias) - for `InstNormRunner` to normalise with the statistics of the image in flight."""
    def __init__(self, conv: nn.Conv2d, ibn, pad4=None):
        super(IBNConvRunner, self).__init__(conv, None, pad4=pad4)
        self.ibn = ibn

    def _sources(self):
        bn = self.ibn.batch_norm
        return [self.conv.weight, self.conv.bias, bn.weight, bn.bias, bn.running_mean, bn.running_var]

    def prepare(self, x: NHWC, d: ConvDesc):
        before = self._key
        super(IBNConvRunner, self).prepare(x, d)
        if self._key == before:
            return
        bn, dev = self.ibn.batch_norm, x.device
        h1, h2 = self.ibn.split_sections
        if d.Cout != h1 + h2 or bn.num_features != h2:
            raise RuntimeError("IBN sections {} do not cover the convolution's {} output channels".format((h1, h2), d.Cout))
        scale, shift = _fold_bn(dev, bn, h2, self.conv.bias[h1:] if self.conv.bias is not None else None)
        self.scale[h1:].copy_(scale)
        self.shift[h1:].copy_(shift)
        torch.cuda.current_stream(dev).synchronize()

    def run(self, x: NHWC, *args, **kwargs) -> NHWC:
        if self.ibn.batch_norm.training:
            raise RuntimeError("pytorchcv_amd is an inference path: call net.eval() first (BatchNorm is folded)")
        return super(IBNConvRunner, self).run(x, *args, **kwargs)


class InstNormRunner(object):
    """nn.InstanceNorm2d(affine=True) at inference + activation on the leading `norm.num_features` channels of a handle, the rest
    only activated (pcv_instnorm_act: two launches, statistics then apply). Nothing folds at load time - the statistics are those
    of the image in flight - so the runner keeps no derived state: gamma / beta are read where the module holds them (fp32)."""
    def __init__(self, norm):
        if not isinstance(norm, nn.InstanceNorm2d):
            raise NotImplementedError("InstNormRunner runs nn.InstanceNorm2d, got {}".format(type(norm).__name__))
        if not norm.affine or norm.track_running_stats:
            raise NotImplementedError("only InstanceNorm2d(affine=True, track_running_stats=False) is on the MI355X path")
        if norm.num_features % 8:
            raise NotImplementedError("InstanceNorm2d over {} channels: the MI355X path needs a multiple of 8".format(norm.num_features))
        self.norm = norm

    def run(self, x: NHWC, act: int) -> NHWC:
        norm = self.norm
        if x.wpitch != x.W:
            raise RuntimeError("InstanceNorm on a row-padded handle")
        Cn, CP = norm.num_features, round8(x.C)
        if Cn > x.C or x.C % 8:
            raise RuntimeError("InstanceNorm2d over the first {} channels of a handle with {}".format(Cn, x.C))
        if norm.weight.device != x.device:
            raise RuntimeError("model parameters are on {} but the input is on {}".format(norm.weight.device, x.device))
        gamma = norm.weight.detach().float().contiguous()        # (no copy for fp32 parameters)
        beta = norm.bias.detach().float().contiguous()
        nbytes = ctypes.c_size_t(0)
        if _lib.lib().pcv_instnorm_workspace_bytes(x.N, Cn, ctypes.byref(nbytes)) != 0:
            raise _lib.PcvError(-1, "pcv_instnorm_workspace_bytes({}, {})".format(x.N, Cn))
        ws = torch.empty(max(nbytes.value, 16), dtype=torch.uint8, device=x.device)
        y = torch.empty((x.N, x.H, x.W, CP), dtype=x.dtype, device=x.device)
        _call(x.device, "instnorm_act", _ptr(x.t), _ptr(gamma), _ptr(beta), _ptr(y), _ptr(ws), x.N, x.H * x.W, CP, Cn, x.cpitch,
              ctypes.c_float(norm.eps), act, _CODE_OF_TORCH[x.dtype])
        return NHWC(y, x.N, x.H, x.W, x.C, cpitch=CP)


def global_avgpool(x: NHWC, out_fp32: bool = False) -> NHWC:
    """nn.AdaptiveAvgPool2d(1) -> [N,1,1,C]. `out_fp32`: see avgpool2d."""
    if not x.dense:
        raise RuntimeError("avg-pool on a padded handle")
    y = torch.empty((x.N, 1, 1, x.cpitch), dtype=torch.float32 if out_fp32 else x.dtype, device=x.device)
    code = _CODE_OF_TORCH[x.dtype]
    _call(x.device, "global_avgpool", _ptr(x.t), _ptr(y), x.N, x.H * x.W, x.cpitch, code, 0 if out_fp32 else code)
    return NHWC(y, x.N, 1, 1, x.C, cpitch=x.cpitch)


def se_excite(v: torch.Tensor, w1, b1, w2, b2, mid_act: int, out_act: int) -> torch.Tensor:
    """The two fp32 layers of an excitation on a contiguous fp32 [N, C] tensor (pcv_se_excite): out_act(w2 . mid_act(w1 . v + b1) + b2)
    with w1 [M, C], b1 [M], w2 [C, M], b2 [C] -> fp32 [N, C]."""
    N, C, M = v.shape[0], v.shape[1], w1.shape[0]
    mid = torch.empty((N, M), dtype=torch.float32, device=v.device)
    gate = torch.empty((N, C), dtype=torch.float32, device=v.device)
    _call(v.device, "se_excite", _ptr(v), _ptr(w1), _ptr(b1), _ptr(w2), _ptr(b2), _ptr(mid), _ptr(gate), N, C, M, mid_act, out_act)
    return gate


def se_scale(x: NHWC, gate: torch.Tensor, residual: NHWC | None = None, post_act: int = 0) -> NHWC:
    """post_act(x * gate + residual) with a per-image, per-channel fp32 gate [N, x.cpitch] (pcv_se_scale). The callers have checked that
    `x` is dense and that `gate` is a contiguous fp32 tensor of that shape on x's device; only the residual is checked here."""
    if residual is not None and (residual.t.shape != x.t.shape or residual.dtype != x.dtype):
        raise RuntimeError("SE residual shape/dtype mismatch")
    y = torch.empty_like(x.t)
    _call(x.device, "se_scale", _ptr(x.t), _ptr(gate), _ptr(residual.t) if residual is not None else None, _ptr(y), x.N, x.H * x.W,
          x.cpitch, post_act, _CODE_OF_TORCH[x.dtype])
    return NHWC(y, x.N, x.H, x.W, x.C, cpitch=x.cpitch)


def se_forward(x: NHWC, w1, b1, w2, b2, mid_act: int, out_act: int, residual: NHWC | None, post_act: int) -> NHWC:
    """SEBlock on the hot path: squeeze -> excite (fp32) -> scale (+ residual, + activation)."""
    if not x.dense:
        raise RuntimeError("SE on a padded handle")
    CP = x.cpitch                                              # physical channels; the FC weights get zero columns / rows for the pads
    if CP != x.C:
        w1 = F.pad(w1, (0, CP - x.C)).contiguous()
        w2 = F.pad(w2, (0, 0, 0, CP - x.C)).contiguous()
        b2 = F.pad(b2, (0, CP - x.C)).contiguous()
    mean = torch.empty((x.N, CP), dtype=torch.float32, device=x.device)
    _call(x.device, "se_squeeze", _ptr(x.t), _ptr(mean), x.N, x.H * x.W, CP, _CODE_OF_TORCH[x.dtype])
    return se_scale(x, se_excite(mean, w1, b1, w2, b2, mid_act, out_act), residual, post_act)


def splat_forward(x: NHWC, radix: int, groups: int, w1, b1, w2, b2, residual: NHWC | None = None, post_act: int = 0) -> NHWC:
    """Split attention on the hot path (SABlock, reference att.py:172-189; SKConvBlock, sknet.py:68-83): squeeze the sum of the
    `radix` splits of x [N, H, W, radix * C] -> fp32 MLP (w1 [M, C], b1 [M] with the MLP's BatchNorm folded in; w2 [radix C, M],
    b2 [radix C]) -> softmax across the splits -> per-channel weighted sum of the splits (+ residual, + activation): three
    launches, the result is [N, H, W, C]."""
    if not x.dense or x.C % radix:
        raise RuntimeError("split attention needs a dense handle whose channels split into {} parts".format(radix))
    C = x.C // radix
    if C % 8:
        raise NotImplementedError("split attention with {} channels per split: the MI355X path needs multiples of 8".format(C))
    code = _CODE_OF_TORCH[x.dtype]
    N, HW, M = x.N, x.H * x.W, int(w1.shape[0])
    s = torch.empty((N, C), dtype=torch.float32, device=x.device)
    _call(x.device, "splat_squeeze", _ptr(x.t), _ptr(s), N, HW, C, radix, code)
    mid = torch.empty((N, M), dtype=torch.float32, device=x.device)
    logits = torch.empty((N, radix * C), dtype=torch.float32, device=x.device)
    att = torch.empty((N, radix * C), dtype=torch.float32, device=x.device)
    _call(x.device, "splat_excite", _ptr(s), _ptr(w1), _ptr(b1), _ptr(w2), _ptr(b2), _ptr(mid), _ptr(logits), _ptr(att), N, C, M,
          radix, groups)
    y = torch.empty((N, x.H, x.W, C), dtype=x.dtype, device=x.device)
    if residual is not None and (tuple(residual.t.shape) != tuple(y.shape) or residual.dtype != x.dtype):
        raise RuntimeError("split-attention residual shape/dtype mismatch: {} vs {}".format(tuple(residual.t.shape), tuple(y.shape)))
    _call(x.device, "splat_combine", _ptr(x.t), _ptr(att), _ptr(residual.t) if residual is not None else None, _ptr(y), N, HW, C, radix,
          post_act, code)
    return NHWC(y, N, x.H, x.W, C)


def _cbam_handle(x: NHWC):
    """The CBAM launches take a dense handle with a multiple of 8 channels; anything else is refused before any of them."""
    if not x.dense or x.C % 8:
        raise NotImplementedError("CBAM on {} channels: the MI355X path needs a dense handle with a multiple of 8".format(x.C))


def cbam_channel_gate(x: NHWC, w1, b1, w2, b2) -> torch.Tensor:
    """CBAM's channel gate (ChannelGate, reference cbamresnet.py:48-80) as an fp32 [N, C] factor: mean and max over the map
    (pcv_cbam_pool) -> shared fp32 MLP (w1 [M, C], b1 [M], w2 [C, M], b2 [C]) on both, summed, sigmoid (pcv_cbam_excite)."""
    _cbam_handle(x)
    N, C, M = x.N, x.C, int(w1.shape[0])
    if tuple(w1.shape) != (M, C) or tuple(w2.shape) != (C, M):
        raise RuntimeError("CBAM weights do not fit {} channels".format(C))
    f32 = dict(dtype=torch.float32, device=x.device)
    s = torch.empty((N, 2, C), **f32)
    _call(x.device, "cbam_pool", _ptr(x.t), _ptr(s), N, x.H * x.W, C, _CODE_OF_TORCH[x.dtype])
    mid = torch.empty((N, 2, M), **f32)
    gate = torch.empty((N, C), **f32)
    _call(x.device, "cbam_excite", _ptr(s), _ptr(w1), _ptr(b1), _ptr(w2), _ptr(b2), _ptr(mid), _ptr(gate), N, C, M)
    return gate


def cbam_spatial(x: NHWC, gate: torch.Tensor | None, w7, scale, shift, residual: NHWC | None = None, post_act: int = 0) -> NHWC:
    """CBAM's spatial stage on x * gate (SpatialGate, reference cbamresnet.py:83-102; gate fp32 [N, C], None = ones: the stand-alone
    module): per-pixel max and mean over the channels (pcv_cbam_spatial_pool) -> 7x7 convolution 2 -> 1 (w7 fp32 [2, 7, 7]; `scale` /
    `shift`: one device float each, its folded BatchNorm), sigmoid -> y = post_act((x * gate) * spatial gate + residual)
    (pcv_cbam_apply). x * gate is never stored."""
    _cbam_handle(x)
    if w7.numel() != 98 or scale.numel() != 1 or shift.numel() != 1:
        raise RuntimeError("CBAM weights do not fit {} channels".format(x.C))
    code = _CODE_OF_TORCH[x.dtype]
    N, HW, C = x.N, x.H * x.W, x.C
    if gate is None:
        gate = torch.ones((N, C), dtype=torch.float32, device=x.device)
    p = torch.empty((N, HW, 2), dtype=torch.float32, device=x.device)
    _call(x.device, "cbam_spatial_pool", _ptr(x.t), _ptr(gate), _ptr(p), N, HW, C, code)
    y = torch.empty_like(x.t)
    if residual is not None and (tuple(residual.t.shape) != tuple(x.t.shape) or residual.dtype != x.dtype):
        raise RuntimeError("CBAM residual shape/dtype mismatch: {} vs {}".format(tuple(residual.t.shape), tuple(x.t.shape)))
    _call(x.device, "cbam_apply", _ptr(x.t), _ptr(gate), _ptr(p), _ptr(w7), _ptr(scale), _ptr(shift),
          _ptr(residual.t) if residual is not None else None, _ptr(y), N, x.H, x.W, C, post_act, code)
    return NHWC(y, N, x.H, x.W, C)


def cbam_forward(x: NHWC, w1, b1, w2, b2, w7, scale, shift, residual: NHWC | None = None, post_act: int = 0) -> NHWC:
    """CBAM block on the hot path (CbamBlock, reference cbamresnet.py:105-128): `cbam_channel_gate`, then `cbam_spatial` with that
    gate. Four launches; the only tensor of x's size they write is y."""
    return cbam_spatial(x, cbam_channel_gate(x, w1, b1, w2, b2), w7, scale, shift, residual, post_act)


def classify(logits: torch.Tensor, k: int = 0, labels=None, probs: bool = False, nll: bool = False) -> dict:
    """What follows the logits, one launch (pcv_classify_f32) on the current stream: for fp32 logits [N, J] a dict of device tensors -
    "ids" (int32 [N, k]) and "values" (fp32 [N, k]) when k > 0, "probs" (fp32 [N, k], softmax over the whole row) with `probs`,
    "rank" (int32 [N]) when `labels` are given, "nll" (fp32 [N]) with `nll`. The order: NaN above +inf, larger first, equal values by
    lower index, -0 ties with +0; "rank" counts the entries that precede the label, so top-k error for any k is count(rank >= k).
    Labels of any integer dtype, converted to int64 on the device; one outside [0, J) gives rank J and nll +inf. The limits
    (J <= 16384, k <= min(J, 32), nll needs labels) are the library's: it refuses with PcvError."""
    if not torch.is_tensor(logits) or logits.dim() != 2 or logits.dtype != torch.float32:
        raise TypeError("expected fp32 logits [N, J]")
    dev = logits.device
    logits = logits.contiguous()
    N, J = int(logits.shape[0]), int(logits.shape[1])
    k = int(k)
    out = {}
    if k > 0:
        out["ids"] = torch.empty((N, k), dtype=torch.int32, device=dev)
        out["values"] = torch.empty((N, k), dtype=torch.float32, device=dev)
    if probs:
        out["probs"] = torch.empty((N, max(k, 0)), dtype=torch.float32, device=dev)
    if labels is not None:
        if not torch.is_tensor(labels) or labels.is_floating_point() or labels.is_complex() or labels.dtype == torch.bool:
            raise TypeError("labels must be a tensor of an integer dtype")
        if labels.numel() != N:
            raise ValueError("expected {} labels, got {}".format(N, labels.numel()))
        labels = labels.reshape(N).to(device=dev, dtype=torch.int64).contiguous()
        out["rank"] = torch.empty((N,), dtype=torch.int32, device=dev)
    if nll:
        out["nll"] = torch.empty((N,), dtype=torch.float32, device=dev)
    _call(dev, "classify_f32", _ptr(logits), N, J, k, _ptr(out.get("ids")), _ptr(out.get("values")), _ptr(out.get("probs")), _ptr(labels),
          _ptr(out.get("rank")), _ptr(out.get("nll")))
    return out
