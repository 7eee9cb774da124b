"""GPU: the fused resize (pcv_resize_crop_u8 through pytorchcv_amd.eval.preprocess_frames). The expectation is always
`preprocess_u8(restated resize of the frame)`: the restatement of PIL's integer algorithm runs on the CPU
(tests/test_resize_host.py, held against PIL there), the existing kernel is the yardstick for the last stage, and the comparison is
`torch.equal` on the whole output - pad channel and pad column included."""

import numpy as np
import pytest
import torch
import util
from test_resize_host import resize_restated
from make_golden_resize import real_source

pytestmark = pytest.mark.gpu

# the ragged batch: landscape / portrait / square down-scales, two up-scales, both axes identity and one axis identity at img_size 32
# (size 37), an 8x down-scale, and the two extreme aspects (a 32-row crop out of the middle of a 1608-row resized frame)
RAGGED = [(41, 53), (53, 41), (64, 64), (7, 9), (20, 25), (37, 37), (37, 64), (300, 290), (1000, 23), (23, 1000)]

_sources = {}
_resized = {}


def source(i, c):
    """Seeded uint8 frame i of the ragged batch with c channels (CPU)."""
    if (i, c) not in _sources:
        hs, ws = RAGGED[i]
        g = torch.Generator().manual_seed(900 + 10 * i + c)
        _sources[(i, c)] = torch.randint(0, 256, (hs, ws, c), generator=g, dtype=torch.uint8)
    return _sources[(i, c)]


def resized(key, src, size):
    """The restated resize of a CPU frame to torchvision's output size for `size`, computed once per key."""
    from pytorchcv_amd import eval as ev
    if (key, size) not in _resized:
        oh, ow = ev.resize_output_size(src.shape[0], src.shape[1], size)
        _resized[(key, size)] = torch.from_numpy(resize_restated(src.numpy(), oh, ow))
    return _resized[(key, size)]


def expected(key, src, img_size, dtype, dev, img_scale=0.875):
    from pytorchcv_amd import eval as ev
    r = resized(key, src, ev.resize_size(img_size, img_scale))
    return ev.preprocess_u8(r.unsqueeze(0).to(dev), img_size=img_size, dtype=dtype).t[0]


def assert_frames_equal(got, frames, keys, img_size, dtype, dev):
    wp = (img_size + 1) // 2 * 2
    assert tuple(got.t.shape) == (len(frames), img_size, wp, 4)
    assert (got.N, got.H, got.W, got.C, got.cpitch, got.wpitch) == (len(frames), img_size, img_size, frames[0].shape[2], 4, wp)
    for i, (k, f) in enumerate(zip(keys, frames)):
        want = expected(k, f, img_size, dtype, dev)
        assert torch.equal(got.t[i], want), "frame {} {} differs: {} elements".format(
            i, tuple(f.shape), int((got.t[i] != want).sum()))


@pytest.mark.parametrize("img_size", [32, 33, 40])
@pytest.mark.parametrize("dtype", ["fp32", "bf16", "fp16"])
def test_ragged_sweep(dtype, img_size, cuda_device):
    from pytorchcv_amd import eval as ev
    for c in (3, 1):
        frames = [source(i, c) for i in range(len(RAGGED))]
        got = ev.preprocess_frames([f.to(cuda_device) for f in frames], img_size=img_size, img_scale=0.875, dtype=dtype)
        assert_frames_equal(got, frames, [("ragged", i, c) for i in range(len(RAGGED))], img_size, dtype, cuda_device)


def test_real_geometry(cuda_device):
    from pytorchcv_amd import eval as ev
    frames = [torch.from_numpy(real_source(375, 500)), torch.from_numpy(real_source(500, 333))]
    dev_frames = [f.to(cuda_device) for f in frames]
    for kw in ({}, {"dtype": "fp32"}):
        got = ev.preprocess_frames(dev_frames, **kw)
        assert_frames_equal(got, frames, ["real0", "real1"], 224, kw.get("dtype", "bf16"), cuda_device)


def test_batch_invariance_and_tensor_form(cuda_device):
    from pytorchcv_amd import eval as ev
    frames = [source(i, 3).to(cuda_device) for i in range(len(RAGGED))]
    batch = ev.preprocess_frames(frames, img_size=32, dtype="fp16")
    for i in (0, 3, 7, 8):
        alone = ev.preprocess_frames([frames[i]], img_size=32, dtype="fp16")
        assert torch.equal(alone.t[0], batch.t[i])
    g = torch.Generator().manual_seed(77)
    same = torch.randint(0, 256, (3, 45, 61, 3), generator=g, dtype=torch.uint8).to(cuda_device)
    a = ev.preprocess_frames(same, img_size=33, dtype="bf16")
    b = ev.preprocess_frames([same[0], same[1], same[2]], img_size=33, dtype="bf16")
    assert torch.equal(a.t, b.t)
    assert_frames_equal(a, [f.cpu() for f in same], [("same", i) for i in range(3)], 33, "bf16", cuda_device)


def test_multi_round_under_max_blocks(cuda_device):
    from pytorchcv_amd import eval as ev
    frames = [source(i, 3).to(cuda_device) for i in range(len(RAGGED))]
    free = ev.preprocess_frames(frames, img_size=40, dtype="bf16")
    with util.tuning(max_blocks=3):
        capped = ev.preprocess_frames(frames, img_size=40, dtype="bf16")
        torch.cuda.synchronize()
    assert torch.equal(free.t, capped.t)


def test_refusals(cuda_device):
    from pytorchcv_amd import eval as ev
    ok = source(0, 3).to(cuda_device)
    with pytest.raises((TypeError, ValueError)):
        ev.preprocess_frames([source(0, 3)], img_size=32)                           # a CPU tensor
    with pytest.raises((TypeError, ValueError)):
        ev.preprocess_frames(source(0, 3).unsqueeze(0), img_size=32)                # ... in the tensor form
    with pytest.raises(TypeError):
        ev.preprocess_frames([ok.float()], img_size=32)                             # not uint8
    with pytest.raises(ValueError):
        ev.preprocess_frames([ok, source(1, 1).to(cuda_device)], img_size=32)       # mixed C
    with pytest.raises(ValueError):
        ev.preprocess_frames([], img_size=32)                                       # no frames
    with pytest.raises((TypeError, ValueError)):
        ev.preprocess_frames([torch.zeros((41, 53, 5), dtype=torch.uint8, device=cuda_device)], img_size=32)    # C = 5
    with pytest.raises(ValueError):
        ev.preprocess_frames([ok], img_size=32, img_scale=1.25)                     # the crop is larger than the resized frame
    if torch.cuda.device_count() >= 2:
        with pytest.raises(ValueError):
            ev.preprocess_frames([ok, source(1, 3).to(torch.device("cuda", 1))], img_size=32)
    assert torch.equal(ev.preprocess_frames([ok], img_size=32).t, ev.preprocess_frames([ok], img_size=32).t)    # still usable


def test_end_to_end_resnet18(cuda_device):
    import pytorchcv_amd
    from pytorchcv_amd import eval as ev
    from pytorchcv_amd.model_provider import get_model
    net = get_model("resnet18").eval()
    net.load_state_dict(util.model_state("resnet18", net.state_dict()), strict=True)
    net = pytorchcv_amd.set_compute_dtype(net.to(cuda_device), "fp32")
    g = torch.Generator().manual_seed(11)
    sizes = [(120, 160), (200, 150), (256, 256), (300, 290)]
    frames = [torch.randint(0, 256, (h, w, 3), generator=g, dtype=torch.uint8) for h, w in sizes]
    ragged = [f.to(cuda_device) for f in frames]
    crops = []
    for i, f in enumerate(frames):
        r = resized(("e2e", i), f, 256)
        top, left = ev.center_crop_box(r.shape[0], r.shape[1], 224)
        crops.append(r[top:top + 224, left:left + 224, :])
    pre = torch.stack(crops).to(cuda_device)                    # [4, 224, 224, 3]: resized and cropped on the CPU
    labels = torch.tensor([1, 2, 3, 4], device=cuda_device)
    with torch.no_grad():
        y = net(ev.preprocess_frames(ragged, dtype="fp32"))
        y_ref = net(ev.preprocess_u8(pre, dtype="fp32"))
    assert torch.equal(y, y_ref)
    res = ev.evaluate(net, [(ragged, labels)])
    ref = ev.evaluate(net, [(pre, labels)])
    assert res == ref and res["n"] == 4
    assert ev.evaluate(net, [(pre, labels)], img_scale=1.0) == ref           # a tensor batch through the resize path: identity at 224
    g = torch.Generator().manual_seed(4)
    old = torch.randint(0, 256, (2, 256, 256, 3), generator=g, dtype=torch.uint8).to(cuda_device)
    out = ev.evaluate(net, [(old, labels[:2])])                               # the old call form
    assert out["n"] == 2 and 0.0 <= out["top5_err"] <= out["top1_err"] <= 100.0
