"""
Timing of the fused resize launch (GPU dev tool, not collected by pytest). Prints ONE JSON line:
  - pcv_resize_crop_u8 on a seeded batch of 256 frames with ImageNet-like sizes around 375 x 500 -> 224 (size 256), bf16: device
    events around each of `--launches` launches after a warm-up; median, min, max, and the achieved bytes/s = (source rows the
    bands actually read, from the plan's header, + output bytes) / median;
  - beside it, in the same run, pcv_preprocess_u8 on 256 pre-resized 256 x 341 frames (the launch that exists without the resize);
  - with --pil: images/s of PIL's resize of the same frames on `--workers` host processes (the path this launch replaces).
Launches this long (> 50 us) are measurable eagerly with device events (tests/tools/README.md).
Usage: python tests/tools/resize_time.py [--launches 60] [--pil] [--workers 16] [--out FILE]
"""

import os
import sys
import json
import time
import ctypes
import struct
import argparse

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def frame_sizes(n, seed=5):
    """ImageNet-like (height, width): most frames 500 on the longer side with aspect 3:4 +- spread, some smaller, a few large."""
    import numpy as np
    rng = np.random.RandomState(seed)
    sizes = []
    for _ in range(n):
        u = rng.rand()
        longer = 500 if u < 0.7 else int(rng.randint(200, 500)) if u < 0.9 else int(rng.randint(500, 1600))
        shorter = max(32, int(longer * rng.uniform(0.55, 1.0)))
        sizes.append((shorter, longer) if rng.rand() < 0.75 else (longer, shorter))
    return sizes


def _pil_worker(args):
    import numpy as np
    from PIL import Image
    seed, sizes = args
    rng = np.random.RandomState(seed)
    imgs = [Image.fromarray(rng.randint(0, 256, size=(h, w, 3)).astype(np.uint8)) for h, w in sizes]
    t0 = time.perf_counter()
    for im, (h, w) in zip(imgs, sizes):
        ow, oh = (256, int(256 * h / w)) if w <= h else (int(256 * w / h), 256)
        im.resize((ow, oh), Image.BILINEAR)
    return time.perf_counter() - t0


def pil_rate(sizes, workers):
    """images/s of PIL's resize over `workers` processes, each with its share of the frames already decoded in memory."""
    import multiprocessing as mp
    shares = [(100 + i, sizes[i::workers]) for i in range(workers)]
    with mp.get_context("spawn").Pool(workers) as pool:
        pool.map(_pil_worker, shares)                      # warm-up: imports, allocator
        t0 = time.perf_counter()
        pool.map(_pil_worker, shares)
        wall = time.perf_counter() - t0
    return len(sizes) / wall


def timed(fn, launches, warmup=10):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(launches):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3)               # us
    ts.sort()
    return dict(median_us=round(ts[len(ts) // 2], 2), min_us=round(ts[0], 2), max_us=round(ts[-1], 2),
                p10_us=round(ts[len(ts) // 10], 2), p90_us=round(ts[len(ts) * 9 // 10], 2), launches=launches)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--launches", type=int, default=60)
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--pil", action="store_true")
    ap.add_argument("--workers", type=int, default=16)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    from pytorchcv_amd import engine, _lib, eval as ev
    assert torch.cuda.is_available(), "resize_time.py needs a GPU"
    dev = torch.device("cuda", 0)
    sizes = frame_sizes(a.batch)
    g = torch.Generator().manual_seed(1)
    frames = [torch.randint(0, 256, (h, w, 3), generator=g, dtype=torch.uint8).to(dev) for h, w in sizes]
    n, img, size = a.batch, 224, ev.resize_size(224, 0.875)
    L = _lib.lib()
    hs = (ctypes.c_int * n)(*[h for h, _ in sizes])
    ws = (ctypes.c_int * n)(*[w for _, w in sizes])
    ptrs = (ctypes.c_void_p * n)(*[engine._ptr(f) for f in frames])
    nbytes = ctypes.c_size_t()
    assert L.pcv_resize_plan_bytes(n, hs, ws, 3, size, img, img, ctypes.byref(nbytes)) == 0, L.pcv_last_error(None)
    t0 = time.perf_counter()
    plan = torch.empty(nbytes.value, dtype=torch.uint8)
    assert L.pcv_resize_plan(ptrs, n, hs, ws, 3, size, img, img, plan.data_ptr(), nbytes.value) == 0, L.pcv_last_error(None)
    plan_ms = (time.perf_counter() - t0) * 1e3
    hd = struct.unpack_from("<I7iQQ", bytes(plan[:48].tolist()), 0)
    items, stage_bytes, src_bytes = hd[5], hd[6], hd[9]
    plan_dev = plan.to(dev)
    code, tdt = engine.DTYPES[a.dtype]
    y = torch.empty((n, img, img, 4), dtype=tdt, device=dev)
    m = torch.tensor(list(ev.IMAGENET_MEAN) + [0.0], dtype=torch.float32, device=dev)
    s = torch.tensor([1.0 / v for v in ev.IMAGENET_STD] + [0.0], dtype=torch.float32, device=dev)
    ctx, st = engine._ctx(dev), engine._stream(dev)

    def resize():
        _lib.check(L.pcv_resize_crop_u8(ctx, plan.data_ptr(), engine._ptr(plan_dev), nbytes.value, engine._ptr(y), img,
                                        engine._ptr(m), engine._ptr(s), code, st), ctx)

    pre = torch.randint(0, 256, (n, 256, 341, 3), generator=g, dtype=torch.uint8).to(dev)
    y2 = torch.empty_like(y)

    def plain():
        _lib.check(L.pcv_preprocess_u8(ctx, engine._ptr(pre), engine._ptr(y2), n, 256, 341, 3, 16, 58, img, img, img, engine._ptr(m),
                                       engine._ptr(s), code, st), ctx)

    # alternate the two so that both see the same clock and neighbours
    res_a = timed(resize, a.launches // 2)
    pla_a = timed(plain, a.launches // 2)
    res_b = timed(resize, a.launches - a.launches // 2)
    pla_b = timed(plain, a.launches - a.launches // 2)
    t_res = timed(resize, a.launches)
    t_pla = timed(plain, a.launches)
    out_bytes = y.numel() * y.element_size()
    total = src_bytes + out_bytes
    frame_bytes = sum(h * w * 3 for h, w in sizes)
    res = dict(tool="resize_time", batch=n, dtype=a.dtype, items=items, stage_bytes=stage_bytes, plan_bytes=nbytes.value,
               plan_host_ms=round(plan_ms, 2), frames_bytes=frame_bytes, band_source_bytes=src_bytes, output_bytes=out_bytes,
               resize=t_res, resize_halves=[res_a["median_us"], res_b["median_us"]],
               resize_bytes_per_s=round(total / (t_res["median_us"] * 1e-6), 1),
               resize_img_per_s=round(n / (t_res["median_us"] * 1e-6), 1),
               preprocess_u8=t_pla, preprocess_u8_halves=[pla_a["median_us"], pla_b["median_us"]])
    if a.pil:
        del frames
        res["pil_workers"] = a.workers
        res["pil_resize_img_per_s"] = round(pil_rate(sizes, a.workers), 1)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
