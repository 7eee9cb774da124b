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
"""

__all__ = ['IMAGENET_MEAN', 'IMAGENET_STD', 'resize_size', 'resize_output_size', 'center_crop_box', 'preprocess_u8',
           'preprocess_frames', 'topk_errors', 'evaluate']

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


def preprocess_u8(frames: torch.Tensor, img_size: int = 224, dtype: str = "bf16", mean=IMAGENET_MEAN, std=IMAGENET_STD) -> engine.NHWC:
    """uint8 [N, Hs, Ws, C<=4] device tensor -> the stem's input handle (centre crop, normalise, NHWC4, cast)."""
    if frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[3] > 4:
        raise TypeError("expected a uint8 tensor [N, H, W, C <= 4]")
    frames = frames.contiguous()
    n, hs, ws, c = frames.shape
    if len(mean) < c or len(std) < c:
        raise ValueError("mean/std need one value per channel")
    top, left = center_crop_box(hs, ws, img_size)
    code, tdt = engine.DTYPES[dtype]
    wp = (img_size + 1) // 2 * 2
    dev = frames.device
    y = torch.empty((n, img_size, wp, 4), dtype=tdt, device=dev)
    m = torch.tensor(list(mean)[:c] + [0.0] * (4 - c), dtype=torch.float32, device=dev)
    s = torch.tensor([1.0 / v for v in list(std)[:c]] + [0.0] * (4 - c), dtype=torch.float32, device=dev)
    ctx = engine._ctx(dev)
    _lib.check(_lib.lib().pcv_preprocess_u8(ctx, engine._ptr(frames), engine._ptr(y), n, hs, ws, c, top, left, img_size, img_size,
                                            wp, engine._ptr(m), engine._ptr(s), code, engine._stream(dev)), ctx)
    return engine.NHWC(y, n, img_size, img_size, c, wpitch=wp, cpitch=4)


def preprocess_frames(frames, img_size: int = 224, img_scale: float = 0.875, dtype: str = "bf16", mean=IMAGENET_MEAN,
                      std=IMAGENET_STD) -> engine.NHWC:
    """Decoded uint8 frames of any size -> the stem's input handle, one launch: shorter side to `resize_size(img_size, img_scale)`
    exactly as PIL resizes it (bit for bit), centre crop, normalise, NHWC4, cast. `frames`: a list / tuple of contiguous uint8
    device tensors [Hi, Wi, C], or one [N, H, W, C] tensor; one C <= 4 and one device for all of them."""
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
        if not f.is_cuda:
            raise TypeError("frames must be device tensors")
    c = int(frames[0].shape[2])
    dev = frames[0].device
    if any(int(f.shape[2]) != c for f in frames):
        raise ValueError("all frames of a batch must have the same number of channels")
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
    code, tdt = engine.DTYPES[dtype]
    wp = (img_size + 1) // 2 * 2
    y = torch.empty((n, img_size, wp, 4), dtype=tdt, device=dev)
    m = torch.tensor(list(mean)[:c] + [0.0] * (4 - c), dtype=torch.float32, device=dev)
    s = torch.tensor([1.0 / v for v in list(std)[:c]] + [0.0] * (4 - c), dtype=torch.float32, device=dev)
    ctx = engine._ctx(dev)
    _lib.check(L.pcv_resize_crop_u8(ctx, plan.data_ptr(), engine._ptr(plan_dev), nbytes.value, engine._ptr(y), wp, engine._ptr(m),
                                    engine._ptr(s), code, engine._stream(dev)), ctx)
    return engine.NHWC(y, n, img_size, img_size, c, wpitch=wp, cpitch=4)


def topk_errors(logits: torch.Tensor, labels: torch.Tensor, ks=(1, 5)):
    """Number of samples whose label is NOT among the k largest logits, for each k."""
    top = logits.topk(max(ks), dim=1).indices
    hit = top.eq(labels.view(-1, 1))
    return [int(labels.numel() - hit[:, :k].any(dim=1).sum()) for k in ks]


def evaluate(net, batches, img_size: int = 224, ks=(1, 5), img_scale=None):
    """`batches`: iterable of (frames, int64 labels [N]) with the frames on the net's device: one uint8 tensor [N, Hs, Ws, 3] that
    already has the resized shape (`preprocess_u8`), or a list of native-size uint8 frames [Hi, Wi, 3], which go through
    `preprocess_frames` (resize included, `img_scale` 0.875 unless given). With `img_scale` given, tensor batches take that path too.
    Returns {"top1_err": ..., "top5_err": ..., "n": ...} in the README's convention (error rates in %)."""
    dtype = engine.compute_dtype_of(net)
    wrong = [0] * len(ks)
    total = 0
    with torch.no_grad():
        for frames, labels in batches:
            if img_scale is not None or isinstance(frames, (list, tuple)):
                x = preprocess_frames(frames, img_size=img_size, img_scale=0.875 if img_scale is None else img_scale, dtype=dtype)
            else:
                x = preprocess_u8(frames, img_size=img_size, dtype=dtype)
            logits = net(x)
            for i, w in enumerate(topk_errors(logits, labels.to(logits.device), ks)):
                wrong[i] += w
            total += int(labels.numel())
    out = {"n": total}
    for k, w in zip(ks, wrong):
        out["top{}_err".format(k)] = 100.0 * w / max(total, 1)
    return out
