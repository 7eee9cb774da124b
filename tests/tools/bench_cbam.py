"""
CBAM measurement for CBAM-ResNet-50 at batch 256 in the default mode (GPU dev tool, not collected by pytest): prints ONE JSON line with
  - the one-forward latency on one stream (eager, median of 5) and the `capture_best` throughput (images/s) of cbam_resnet50, and
    of seresnet50 from the same run (the nearest family: same body, one gate instead of two);
  - per kernel and per tensor of the net's four stages ([256, 56*56, 256], [256, 28*28, 512], [256, 14*14, 1024], [256, 7*7, 2048]):
    microseconds (median of the timed rounds), algorithmic bytes (each tensor read or written once) and the fraction of 8 TB/s, for
    the four CBAM launches AND for their yardsticks on the same tensors - pcv_se_squeeze (the same read as pcv_cbam_pool and
    pcv_cbam_spatial_pool) and pcv_se_scale with a residual (the same bytes as pcv_cbam_apply, without the stencil). The times
    come from a `rocprofv3 --kernel-trace` run of this script in a child process (launches under ~40 us are not measurable
    eagerly from Python, tests/tools/README.md); the rounds alternate yardstick and kernel.
Usage: python tests/tools/bench_cbam.py [--out profiles/cbam_resnet50_bs256.json] [--no-prof] [--no-net]
"""

import os
import sys
import csv
import json
import glob
import time
import shutil
import argparse
import tempfile
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

HBM = 8.0e12
SHAPES = [(56, 256), (28, 512), (14, 1024), (7, 2048)]         # (map side, channels) of the four stages
ROUNDS = 7                                                      # timed rounds per shape (after one warm-up round)
# one round, in launch order: (label, kernel name in the trace)
ROUND = [("se_squeeze", "spatial_mean_kernel"), ("cbam_pool", "cbam_pool_kernel"), ("cbam_excite_fc1", "se_fc_kernel"),
         ("cbam_excite_gate", "cbam_gate_kernel"), ("cbam_spatial_pool", "cbam_spatial_pool_kernel"), ("se_scale_res", "se_scale_kernel"),
         ("cbam_apply_res_relu", "cbam_apply_kernel")]


def algorithmic_bytes(label, N, side, C, es):
    HW, M = side * side, C // 16
    x = N * HW * C * es
    return {"se_squeeze": x + N * C * 4,
            "cbam_pool": x + N * 2 * C * 4,
            "cbam_excite_fc1": (M * C + M) * 4 + N * 2 * (C + M) * 4,
            "cbam_excite_gate": (C * M + C) * 4 + N * (2 * M + C) * 4,
            "cbam_spatial_pool": x + N * C * 4 + N * HW * 8,
            "se_scale_res": 3 * x + N * C * 4,
            "cbam_apply_res_relu": 3 * x + N * C * 4 + N * HW * 8 + (98 + 2) * 4}[label]


def _net(name, batch):
    import torch
    import pytorchcv_amd
    from pytorchcv_amd.model_provider import get_model
    from pytorchcv_amd.synth import synth_state_dict
    net = get_model(name).eval()
    net.load_state_dict(synth_state_dict(net.state_dict(), seed=1234), strict=True)
    net = pytorchcv_amd.set_compute_dtype(net.cuda(), "auto")
    x = torch.randn(batch, 3, 224, 224, device="cuda")
    return net, x


def child(batch, dtype):
    """The profiled run: per shape one warm-up round and ROUNDS timed rounds of ROUND, nothing else of these kernels' names."""
    import ctypes
    import torch
    from pytorchcv_amd import _lib, engine
    L, ctx = _lib.lib(), _lib.ctx_for(0)
    code, tdt = engine.DTYPES[dtype]
    p = lambda t: ctypes.c_void_p(t.data_ptr())        # noqa: E731
    st = ctypes.c_void_p(torch.cuda.current_stream(0).cuda_stream)
    f32 = dict(dtype=torch.float32, device="cuda")
    for side, C in SHAPES:
        N, HW, M = batch, side * side, C // 16
        x = torch.randn(N, HW, C, device="cuda").to(tdt)
        res = torch.randn(N, HW, C, device="cuda").to(tdt)
        y = torch.empty_like(x)
        w1, b1, w2, b2 = torch.randn(M, C, **f32) * 0.05, torch.zeros(M, **f32), torch.randn(C, M, **f32) * 0.05, torch.zeros(C, **f32)
        w7, scale, shift = torch.randn(2, 7, 7, **f32) * 0.1, torch.ones(1, **f32), torch.zeros(1, **f32)
        mean, s, mid = torch.empty(N, C, **f32), torch.empty(N, 2, C, **f32), torch.empty(N, 2, M, **f32)
        gate, pm = torch.empty(N, C, **f32), torch.empty(N, HW, 2, **f32)
        torch.cuda.synchronize()
        for _ in range(ROUNDS + 1):
            _lib.check(L.pcv_se_squeeze(ctx, p(x), p(mean), N, HW, C, code, st), ctx)
            _lib.check(L.pcv_cbam_pool(ctx, p(x), p(s), N, HW, C, code, st), ctx)
            _lib.check(L.pcv_cbam_excite(ctx, p(s), p(w1), p(b1), p(w2), p(b2), p(mid), p(gate), N, C, M, st), ctx)
            _lib.check(L.pcv_cbam_spatial_pool(ctx, p(x), p(gate), p(pm), N, HW, C, code, st), ctx)
            _lib.check(L.pcv_se_scale(ctx, p(x), p(gate), p(res), p(y), N, HW, C, 1, code, st), ctx)
            _lib.check(L.pcv_cbam_apply(ctx, p(x), p(gate), p(pm), p(w7), p(scale), p(shift), p(res), p(y), N, side, side, C, 1, code,
                                        st), ctx)
        torch.cuda.synchronize()
        del x, res, y
        torch.cuda.empty_cache()


def profile(batch, dtype):
    d = tempfile.mkdtemp(prefix="cbam_prof_")
    try:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "p", "--", sys.executable,
               os.path.abspath(__file__), "--child", "--batch", str(batch), "--dtype", dtype]
        subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=900)
        f = (glob.glob(os.path.join(d, "**", "p_kernel_trace.csv"), recursive=True) or [None])[0]
        rows = list(csv.DictReader(open(f)))
    finally:
        shutil.rmtree(d, ignore_errors=True)
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    names = [k for _, k in ROUND]
    rows = [r for r in rows if any(k in r["Kernel_Name"] for k in names)]
    per = len(ROUND) * (ROUNDS + 1)
    assert len(rows) == per * len(SHAPES), (len(rows), per * len(SHAPES))
    es = 4 if dtype == "fp32" else 2
    out = []
    for si, (side, C) in enumerate(SHAPES):
        block = rows[si * per:(si + 1) * per]
        for ki, (label, kname) in enumerate(ROUND):
            mine = block[ki::len(ROUND)]
            assert all(kname in r["Kernel_Name"] for r in mine), (label, [r["Kernel_Name"][:40] for r in mine])
            us = sorted((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in mine[1:])      # [0] is the warm-up round
            med = us[len(us) // 2]
            nbytes = algorithmic_bytes(label, batch, side, C, es)
            out.append(dict(tensor="{}x{}x{}x{}".format(batch, side, side, C), kind=label, us=round(med, 2), us_min=round(us[0], 2),
                            us_max=round(us[-1], 2), bytes=int(nbytes), frac_8tbs=round(nbytes / (med * 1e-6) / HBM, 3)))
    by = {(o["tensor"], o["kind"]): o["us"] for o in out}
    ratios = []
    for side, C in SHAPES:
        t = "{}x{}x{}x{}".format(batch, side, side, C)
        ratios.append(dict(tensor=t, pool_over_squeeze=round(by[t, "cbam_pool"] / by[t, "se_squeeze"], 3),
                           spatial_pool_over_squeeze=round(by[t, "cbam_spatial_pool"] / by[t, "se_squeeze"], 3),
                           apply_over_scale=round(by[t, "cbam_apply_res_relu"] / by[t, "se_scale_res"], 3),
                           cbam_block_us=round(sum(by[t, k] for k, _ in ROUND if k.startswith("cbam_")), 2)))
    return dict(kernels=out, ratios=ratios)


def throughput(name, batch):
    """(dtype, eager forward ms: median of 5 after 2, capture_best images/s over 20 steps after 3)."""
    import torch
    from pytorchcv_amd import engine
    from pytorchcv_amd.graph import capture_best
    net, x = _net(name, batch)
    ts = []
    with torch.no_grad():
        for _ in range(7):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            net(x)
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1))
        g = capture_best(net, x, own_input=True)
        for _ in range(3):
            g(None)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        steps = 20
        for _ in range(steps):
            g(None)
        torch.cuda.synchronize()
        thr = batch * steps / (time.perf_counter() - t0)
    dtype = engine.compute_dtype_of(net)
    del g, net, x
    torch.cuda.empty_cache()
    return dtype, round(sorted(ts[2:])[len(ts[2:]) // 2], 3), round(thr, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--dtype", default="")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--no-prof", action="store_true")
    ap.add_argument("--no-net", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.child:
        return child(a.batch, a.dtype)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_cbam.py measures on the GPU: no HIP device is visible")
    from pytorchcv_amd import engine
    from pytorchcv_amd.model_provider import get_model
    dtype = a.dtype or engine.compute_dtype_of(get_model("cbam_resnet18"))
    res = dict(workload="cbam_resnet50_bs{}".format(a.batch), dtype=dtype)
    if not a.no_net:
        d, ms, thr = throughput("cbam_resnet50", a.batch)
        assert d == dtype or a.dtype
        res.update(eager_forward_ms=ms, capture_best_img_per_s=thr)
        d, ms, thr = throughput("seresnet50", a.batch)
        res.update(seresnet50=dict(dtype=d, eager_forward_ms=ms, capture_best_img_per_s=thr))
    if not a.no_prof:
        res.update(profile(a.batch, dtype))
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
