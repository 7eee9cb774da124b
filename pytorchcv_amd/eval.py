"""
    Evaluation harness for the ImageNet-1K classifiers: the preprocessing the reference's pretrained weights assume
    ("ordinary normalization" of a centre crop: README.md:12-13; `img_size`, `img_scale = 0.875` of
    models/common/model_metainfos.csv:1) and top-k error as its README tables quote it. The reference keeps these scripts
    out of tree (imgclsmob); here they sit next to the hot path because the input format is part of it: decoded uint8 frames
    go through ONE kernel straight into the stem convolution.

    Two entries. `preprocess_frames` takes the frames as a decoder hands them back - native size, every frame of a batch its own -
    and does the whole transform in one launch (pcv_resize_crop_u8): torchvision's `Resize(resize_size(...))` as it acts on a PIL
    image (shorter side; PIL's antialiased bilinear resize, an integer algorithm that the kernel reproduces bit for bit), centre
    crop, normalise, NHWC4 layout, cast. That resize is the one the published error rates of the pretrained weights were measured
    with, so it is part of what this package defines, not left to the decoder. `preprocess_u8` is the same without the resize
    (pcv_preprocess_u8), for frames that already have the resized shape, all of one size.

    The output side is one kernel too (pcv_classify_f32, `engine.classify`): `predict` gives top-k ids and softmax probabilities,
    `label_ranks` the rank of every label, and `evaluate` counts errors from the ranks - under ONE order of the logits (NaN above
    +inf, larger first, equal values by lower index), where `torch.topk` leaves ties unspecified. `topk_errors` is the CPU-usable
    form on top of `torch.topk`.
"""

__all__ = ['IMAGENET_MEAN', 'IMAGENET_STD', 'resize_size', 'resize_output_size', 'center_crop_box', 'preprocess_u8',
           'preprocess_frames', 'topk_errors', 'predict', 'label_ranks', 'evaluate']

import math
import ctypes
import torch
from . import engine, _lib

IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)


def resize_size(img_size: int = 224, img_scale: float = 0.875) -> int:
    """Shorter-side size before the centre crop: ceil(img_size / img_scale) = 256 for 224 / 0.875."""
    return int(math.ceil(float(img_size) / img_scale))


def resize_output_size(height: int, width: int, size: int):
    """(oh, ow) of torchvision's `Resize(size)` for an int size: the shorter side becomes `size`, the other int(size * long / short)."""
    if width <= height:
        return int(size * height / width), size
    return size, int(size * width / height)


def center_crop_box(height: int, width: int, img_size: int = 224):
    """(top, left) of the img_size x img_size centre crop, torchvision's rounding."""
    if height < img_size or width < img_size:
        raise ValueError("frame {}x{} is smaller than the {} crop".format(height, width, img_size))
    return int(round((height - img_size) / 2.0)), int(round((width - img_size) / 2.0))


_consts = {}


def _norm_consts(mean, std, c: int, dev):
    """(mean, 1 / std) padded to four channels, on the device; kept per (values, device), so a batch costs no host-to-device copy
    (a pageable copy blocks the host) and the same tensors serve every stream: they are complete when `torch.tensor` returns."""
    key = (tuple(float(v) for v in list(mean)[:c]), tuple(float(v) for v in list(std)[:c]), dev)
    got = _consts.get(key)
    if got is None:                                   # (never evicted: a few bytes, and a launch on any stream may still read them)
        got = (torch.tensor(list(key[0]) + [0.0] * (4 - c), dtype=torch.float32, device=dev),
               torch.tensor([1.0 / v for v in key[1]] + [0.0] * (4 - c), dtype=torch.float32, device=dev))
        _consts[key] = got
    return got


def _input_handle(out, n: int, img_size: int, c: int, dtype: str, dev) -> engine.NHWC:
    """The handle the preprocessing kernels write: `out` if it is one of exactly this shape and dtype, else (None) a new one."""
    tdt = engine.DTYPES[dtype][1]
    wp = (img_size + 1) // 2 * 2
    if out is None:
        return engine.NHWC(torch.empty((n, img_size, wp, 4), dtype=tdt, device=dev), n, img_size, img_size, c, wpitch=wp, cpitch=4)
    if not isinstance(out, engine.NHWC) or not torch.is_tensor(out.t):
        raise ValueError("out= must be an input handle as preprocess_u8 / preprocess_frames return it")
    if (tuple(out.t.shape) != (n, img_size, wp, 4) or (out.N, out.H, out.W, out.C, out.wpitch, out.cpitch) != (n, img_size, img_size, c, wp, 4)
            or not out.t.is_contiguous()):
        raise ValueError("out= handle has shape {} (N, H, W, C = {}), expected {} (N, H, W, C = {})".format(
            tuple(out.t.shape), (out.N, out.H, out.W, out.C), (n, img_size, wp, 4), (n, img_size, img_size, c)))
    if out.t.dtype != tdt:
        raise ValueError("out= handle holds {}, expected {} ({})".format(out.t.dtype, tdt, dtype))
    if out.t.device != dev:
        raise ValueError("out= handle is on {}, the frames are on {}".format(out.t.device, dev))
    return out


def preprocess_u8(frames: torch.Tensor, img_size: int = 224, dtype: str = "bf16", mean=IMAGENET_MEAN, std=IMAGENET_STD,
                  out=None) -> engine.NHWC:
    """uint8 [N, Hs, Ws, C<=4] device tensor -> the stem's input handle (centre crop, normalise, NHWC4, cast). `out`: an existing
    handle of the right shape and dtype to write into instead of allocating (anything else: ValueError)."""
    if frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[3] > 4:
        raise TypeError("expected a uint8 tensor [N, H, W, C <= 4]")
    frames = frames.contiguous()
    n, hs, ws, c = frames.shape
    if len(mean) < c or len(std) < c:
        raise ValueError("mean/std need one value per channel")
    top, left = center_crop_box(hs, ws, img_size)
    code = engine.DTYPES[dtype][0]
    dev = frames.device
    h = _input_handle(out, n, img_size, c, dtype, dev)
    y, wp = h.t, h.wpitch
    m, s = _norm_consts(mean, std, c, dev)
    engine._call(dev, "preprocess_u8", engine._ptr(frames), engine._ptr(y), n, hs, ws, c, top, left, img_size, img_size, wp,
                 engine._ptr(m), engine._ptr(s), code)
    return h


def preprocess_frames(frames, img_size: int = 224, img_scale: float = 0.875, dtype: str = "bf16", mean=IMAGENET_MEAN,
                      std=IMAGENET_STD, out=None) -> engine.NHWC:
    """Decoded uint8 frames of any size -> the stem's input handle, one launch: shorter side to `resize_size(img_size, img_scale)`
    exactly as PIL resizes it (bit for bit), centre crop, normalise, NHWC4, cast. `frames`: a list / tuple of contiguous uint8
    device tensors [Hi, Wi, C], or one [N, H, W, C] tensor; one C <= 4 and one device for all of them. `out`: as `preprocess_u8`'s."""
    if isinstance(frames, torch.Tensor):
        if frames.dtype != torch.uint8 or frames.dim() != 4:
            raise TypeError("expected a uint8 tensor [N, H, W, C <= 4] or a list of uint8 tensors [H, W, C <= 4]")
        frames = list(frames.contiguous().unbind(0))
    elif not isinstance(frames, (list, tuple)):
        raise TypeError("expected a uint8 tensor [N, H, W, C <= 4] or a list of uint8 tensors [H, W, C <= 4]")
    n = len(frames)
    if n == 0:
        raise ValueError("no frames")
    for f in frames:
        if not isinstance(f, torch.Tensor) or f.dtype != torch.uint8 or f.dim() != 3 or f.shape[2] > 4 or f.shape[2] < 1:
            raise TypeError("expected uint8 tensors [H, W, C <= 4]")
    c = int(frames[0].shape[2])
    dev = frames[0].device
    if any(int(f.shape[2]) != c for f in frames):
        raise ValueError("all frames of a batch must have the same number of channels")
    if out is not None:
        _input_handle(out, n, img_size, c, dtype, dev)
    if any(not f.is_cuda for f in frames):
        raise TypeError("frames must be device tensors")
    if any(f.device != dev for f in frames):
        raise ValueError("all frames of a batch must be on one device")
    if any(f.numel() == 0 for f in frames):
        raise ValueError("empty frame")
    if len(mean) < c or len(std) < c:
        raise ValueError("mean/std need one value per channel")
    frames = [f.contiguous() for f in frames]
    size = resize_size(img_size, img_scale)
    L = _lib.lib()
    hs = (ctypes.c_int * n)(*[int(f.shape[0]) for f in frames])
    ws = (ctypes.c_int * n)(*[int(f.shape[1]) for f in frames])
    ptrs = (ctypes.c_void_p * n)(*[engine._ptr(f) for f in frames])
    nbytes = ctypes.c_size_t()
    if L.pcv_resize_plan_bytes(n, hs, ws, c, size, img_size, img_size, ctypes.byref(nbytes)) != 0:
        raise ValueError((L.pcv_last_error(None) or b"").decode())
    plan = torch.empty(nbytes.value, dtype=torch.uint8)
    if L.pcv_resize_plan(ptrs, n, hs, ws, c, size, img_size, img_size, plan.data_ptr(), nbytes.value) != 0:
        raise ValueError((L.pcv_last_error(None) or b"").decode())
    plan_dev = plan.to(dev)
    code = engine.DTYPES[dtype][0]
    h = _input_handle(out, n, img_size, c, dtype, dev)
    y, wp = h.t, h.wpitch
    m, s = _norm_consts(mean, std, c, dev)
    engine._call(dev, "resize_crop_u8", plan.data_ptr(), engine._ptr(plan_dev), nbytes.value, engine._ptr(y), wp, engine._ptr(m),
                 engine._ptr(s), code)
    return h


def topk_errors(logits: torch.Tensor, labels: torch.Tensor, ks=(1, 5)):
    """Number of samples whose label is NOT among the k largest logits, for each k."""
    top = logits.topk(max(ks), dim=1).indices
    hit = top.eq(labels.view(-1, 1))
    return [int(labels.numel() - hit[:, :k].any(dim=1).sum()) for k in ks]


def predict(net, x, k: int = 5):
    """(ids int32 [N, k], probs fp32 [N, k]) of the k first classes of every sample, in the order of `engine.classify`, with their
    softmax probabilities. `x`: an fp32 NCHW tensor or a preprocessing handle (`preprocess_u8` / `preprocess_frames`)."""
    with torch.no_grad():
        r = engine.classify(net(x), k=k, probs=True)
    return r["ids"], r["probs"]


def label_ranks(logits: torch.Tensor, labels: torch.Tensor) -> torch.Tensor:
    """int32 [N] on the logits' device: how many classes precede each sample's label (0 = the label is the top class). The label is
    among the top k exactly when rank < k, for every k at once; a label outside [0, J) has rank J."""
    return engine.classify(logits, labels=labels)["rank"]


def _preprocess(frames, img_size, img_scale, dtype, out=None):
    if img_scale is not None or isinstance(frames, (list, tuple)):
        return preprocess_frames(frames, img_size=img_size, img_scale=0.875 if img_scale is None else img_scale, dtype=dtype, out=out)
    return preprocess_u8(frames, img_size=img_size, dtype=dtype, out=out)


def evaluate(net, batches, img_size: int = 224, ks=(1, 5), img_scale=None, loss: bool = False, pipelined: bool = False):
    """`batches`: iterable of (frames, int64 labels [N]) with the frames on the net's device: one uint8 tensor [N, Hs, Ws, 3] that
    already has the resized shape (`preprocess_u8`), or a list of native-size uint8 frames [Hi, Wi, 3], which go through
    `preprocess_frames` (resize included, `img_scale` 0.875 unless given). With `img_scale` given, tensor batches take that path too.
    Returns {"top1_err": ..., "top5_err": ..., "n": ...} in the README's convention (error rates in %); `loss=True` adds "nll", the
    mean negative log-likelihood over all samples.

    A sample counts as a top-k error when at least k classes PRECEDE its label (`label_ranks`), in one order: NaN above +inf, the
    larger logit first, equal logits by lower class index (-0 equals +0). So a label that ties with other classes across the k-th
    place is a hit exactly when its index is low enough - where `torch.topk` (`topk_errors`) leaves the choice unspecified; without
    such a tie the two agree. The ranks stay on the device: one concatenation and one read-back after the loop, no host
    synchronisation inside it.

    `pipelined=True`: the first batch captures two graphs of the forward (`graph.PipelinedNet`, depth 2) on an input handle of its
    shape; every batch of that size is then preprocessed INTO a slot's handle, replayed and ranked on that slot's stream, two
    batches in flight. A batch of another size (typically the last) runs eagerly. Same kernels on the same data: the result
    equals the eager one exactly."""
    dtype = engine.compute_dtype_of(net)
    ranks, nlls = [], []
    pipe, pipe_n = None, -1

    def rank_of(logits, labels):
        r = engine.classify(logits, labels=labels, nll=loss)
        return r["rank"], r.get("nll")

    def on_slot(tensors, device):                     # made on the caller's stream, read on the slot's: keep them alive for it
        st = torch.cuda.current_stream(device)
        for t in tensors:
            if t.is_cuda:
                t.record_stream(st)

    def fill(h, frames):
        on_slot(frames if isinstance(frames, (list, tuple)) else [frames], h.device)
        return _preprocess(frames, img_size, img_scale, dtype, out=h)

    def then(y, labels):
        on_slot([labels], y.device)
        return rank_of(y, labels)

    with torch.no_grad():
        for frames, labels in batches:
            n = int(labels.numel())
            if pipelined and pipe is None:
                from .graph import PipelinedNet
                pipe_n = n
                pipe = PipelinedNet(net, _preprocess(frames, img_size, img_scale, dtype), depth=2, lanes=1)
            if pipe is not None and n == pipe_n:
                r, l = pipe(fill=lambda h, f=frames: fill(h, f), then=lambda y, lab=labels: then(y, lab))
            else:
                r, l = rank_of(net(_preprocess(frames, img_size, img_scale, dtype)), labels)
            ranks.append(r)
            nlls.append(l)
        if pipe is not None:
            pipe.synchronize()                        # the slots' rank tensors live on the slots' streams
        total = sum(int(r.numel()) for r in ranks)
        out = {"n": total}
        if total:
            rank = torch.cat(ranks).cpu()             # the one read-back
            for k in ks:
                out["top{}_err".format(k)] = 100.0 * int((rank >= k).sum()) / total
            if loss:
                out["nll"] = float(torch.cat(nlls).cpu().double().mean())
        else:
            for k in ks:
                out["top{}_err".format(k)] = 0.0
            if loss:
                out["nll"] = float("nan")
    return out
