"""
GhostNet measurement at batch 256 in the default mode (GPU dev tool, not collected by pytest): prints ONE JSON line with
  (i)  pcv_ghost_dw_fused (without and with the skip tensor) against pcv_dwconv2d_fused on the same m, for the maps of the net's
       ghost modules that move most bytes or have the oddest widths: 112x112x8, 56x56x36, 28x28x60, 14x14x240, 14x14x336, 7x7x480
       (H x W x Cm). Launches of some tens of microseconds cannot be timed eagerly from Python, so each side is a captured graph of
       launches that rotate over distinct input tensors - as many as it takes for the inputs together to exceed ROTATE_BYTES, more
       than the 256 MB last-level cache, so that no launch finds its input left there by an earlier one, and one launch per
       buffer; the three graphs are replayed alternately, REPEATS times each after a warm-up replay, and the medians are reported
       per launch with the algorithmic bytes (depthwise: read and write round8(Cm) channels; ghost: read Cm, write 2 Cm, + read
       2 Cm with the skip tensor), the fraction of 8 TB/s, and the time ratio divided by the byte ratio (1.0 = as fast per byte as
       the depthwise kernel);
  (ii) images/s of ghostnet beside mobilenetv3_large_w1 from the same process: captured forwards replayed in turn, REPEATS rounds,
       medians.
Usage: python tests/tools/bench_ghostnet.py [--out profiles/ghostnet_bs256.json] [--batch 256] [--no-net] [--no-kernel]
"""

import os
import sys
import json
import time
import argparse

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

HBM = 8.0e12
MIN_BUFFERS, REPEATS = 4, 5
ROTATE_BYTES = 320 << 20
MAPS = [(112, 112, 8), (56, 56, 36), (28, 28, 60), (14, 14, 240), (14, 14, 336), (7, 7, 480)]          # H, W, Cm
NETS = ["ghostnet", "mobilenetv3_large_w1"]
STEPS = 10


def _median(v):
    v = sorted(v)
    return v[len(v) // 2]


def _graph_of(fn, n):
    """one launch on each of the n buffers, captured"""
    import torch
    for i in range(2):
        fn(i)                                          # builds the runner's state outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    keep = []
    with torch.cuda.graph(g):
        for i in range(n):
            keep.append(fn(i))
    return g, keep


def _time(g, n):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    g.replay()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / n               # microseconds per launch


def kernels(batch, dtype):
    import torch
    import torch.nn as nn
    from pytorchcv_amd import engine
    tdt = engine.DTYPES[dtype][1]
    es = 4 if dtype == "fp32" else 2
    out = []
    for H, W, Cm in MAPS:
        CP = engine.round8(Cm)
        BUFFERS = max(MIN_BUFFERS, -(-ROTATE_BYTES // (batch * H * W * CP * es)))
        ms = [engine.NHWC(torch.randn(batch, H, W, CP, device="cuda").to(tdt), batch, H, W, Cm, cpitch=CP) for _ in range(BUFFERS)]
        rs = [engine.NHWC(torch.randn(batch, H, W, 2 * Cm, device="cuda").to(tdt), batch, H, W, 2 * Cm) for _ in range(BUFFERS)]
        conv = nn.Conv2d(Cm, Cm, 3, 1, 1, groups=Cm, bias=False).cuda().eval()
        bn = nn.BatchNorm2d(Cm).cuda().eval()
        dw, cheap = engine.ConvRunner(conv, bn), engine.ConvRunner(conv, bn)
        with torch.no_grad():
            graphs = [_graph_of(lambda i: dw.run(ms[i], act=1), BUFFERS),
                      _graph_of(lambda i: engine.ghost_dw(cheap, ms[i], 1), BUFFERS),
                      _graph_of(lambda i: engine.ghost_dw(cheap, ms[i], 1, rs[i]), BUFFERS)]
            for g, _ in graphs:
                _time(g, BUFFERS)
            ts = [[], [], []]
            for _ in range(REPEATS):
                for k, (g, _) in enumerate(graphs):
                    ts[k].append(_time(g, BUFFERS))
        px = batch * H * W
        nbytes = [2 * px * CP * es, 3 * px * Cm * es, 5 * px * Cm * es]
        med = [_median(t) for t in ts]
        row = dict(tensor="{}x{}x{}x{}".format(batch, H, W, Cm), pitch=CP, buffers=BUFFERS)
        for k, tag in enumerate(("dwconv", "ghost", "ghost_res")):
            row[tag + "_us"] = round(med[k], 2)
            row[tag + "_us_min"] = round(min(ts[k]), 2)
            row[tag + "_us_max"] = round(max(ts[k]), 2)
            row[tag + "_bytes"] = nbytes[k]
            row[tag + "_frac_8tbs"] = round(nbytes[k] / (med[k] * 1e-6) / HBM, 3)
        for k, tag in ((1, "ghost"), (2, "ghost_res")):
            row[tag + "_time_ratio"] = round(med[k] / med[0], 3)
            row[tag + "_byte_ratio"] = round(nbytes[k] / nbytes[0], 3)
            row[tag + "_time_per_byte_vs_dwconv"] = round((med[k] / med[0]) / (nbytes[k] / nbytes[0]), 3)
        out.append(row)
        del graphs, ms, rs
        torch.cuda.empty_cache()
    return out


def nets(batch):
    import torch
    import pytorchcv_amd
    from pytorchcv_amd import engine
    from pytorchcv_amd.graph import capture_best
    from pytorchcv_amd.model_provider import get_model
    from pytorchcv_amd.synth import synth_state_dict
    graphs, dtypes = {}, {}
    x = torch.randn(batch, 3, 224, 224, device="cuda")
    with torch.no_grad():
        for name in NETS:
            net = get_model(name).eval()
            net.load_state_dict(synth_state_dict(net.state_dict(), seed=1234), strict=True)
            net = pytorchcv_amd.set_compute_dtype(net.cuda(), "auto")
            dtypes[name] = engine.compute_dtype_of(net)
            graphs[name] = capture_best(net, x.clone(), own_input=True)
            for _ in range(3):
                graphs[name](None)
        torch.cuda.synchronize()
        rates = {n: [] for n in NETS}
        for _ in range(REPEATS):
            for name in NETS:
                t0 = time.perf_counter()
                for _ in range(STEPS):
                    graphs[name](None)
                torch.cuda.synchronize()
                rates[name].append(batch * STEPS / (time.perf_counter() - t0))
    return {n: dict(dtype=dtypes[n], img_per_s=round(_median(r), 1), img_per_s_min=round(min(r), 1), img_per_s_max=round(max(r), 1))
            for n, r in rates.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--dtype", default="")
    ap.add_argument("--no-net", action="store_true")
    ap.add_argument("--no-kernel", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_ghostnet.py measures on the GPU: no HIP device is visible")
    from pytorchcv_amd import engine
    from pytorchcv_amd.model_provider import get_model
    dtype = a.dtype or engine.compute_dtype_of(get_model("ghostnet"))
    res = dict(workload="ghostnet_bs{}".format(a.batch), dtype=dtype)
    if not a.no_kernel:
        res["ghost_vs_dwconv"] = kernels(a.batch, dtype)
    if not a.no_net:
        res["nets"] = nets(a.batch)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
