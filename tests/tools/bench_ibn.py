"""
IBN-Net measurement at batch 256 in the default mode (GPU dev tool, not collected by pytest): prints ONE JSON line with
  (i)  pcv_instnorm_act (statistics + apply, two launches) against pcv_bn_act on the same tensor, for the maps where the nets
       normalise most bytes: 56x56x64 (Cn 32), 56x56x256 (Cn 256), 28x28x128 (Cn 64), 112x112x64 (Cn 64). Launches of some tens
       of microseconds cannot be timed eagerly from Python, so each side is a captured graph of LAUNCHES launches that rotate
       over BUFFERS distinct input tensors (together larger than the 256 MB last-level cache: no launch finds its input left
       there by the previous one); the two graphs are replayed alternately, REPEATS times each after a warm-up replay, and the
       medians are reported per launch, with the algorithmic bytes ((Cn + 2 C) / (2 C) of bn_act's) and the time ratio;
  (ii) images/s of ibn_resnet50, ibnb_resnet50 and ibn_resnext50_32x4d beside resnet50b and resnext50_32x4d - the same nets
       without InstanceNorm - from the same process: captured forwards, the five nets replayed in turn, REPEATS rounds, medians.
Usage: python tests/tools/bench_ibn.py [--out profiles/ibn_resnet50_bs256.json] [--batch 256] [--no-net] [--no-kernel]
"""

import os
import sys
import json
import time
import argparse

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

HBM = 8.0e12
LAUNCHES, BUFFERS, REPEATS = 8, 4, 5
MAPS = [(56, 56, 64, 32), (56, 56, 256, 256), (28, 28, 128, 64), (112, 112, 64, 64)]          # H, W, C, Cn
NETS = ["ibn_resnet50", "resnet50b", "ibnb_resnet50", "ibn_resnext50_32x4d", "resnext50_32x4d"]
STEPS = 10


def _median(v):
    v = sorted(v)
    return v[len(v) // 2]


def _graph_of(fn, xs):
    import torch
    for x in xs[:2]:
        fn(x)                                          # builds the runners' state outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    keep = []
    with torch.cuda.graph(g):
        for i in range(LAUNCHES):
            keep.append(fn(xs[i % BUFFERS]))
    return g, keep


def _time(g):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    g.replay()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / LAUNCHES        # microseconds per launch


def kernels(batch, dtype):
    import torch
    import torch.nn as nn
    from pytorchcv_amd import engine
    tdt = engine.DTYPES[dtype][1]
    es = 4 if dtype == "fp32" else 2
    out = []
    for H, W, C, Cn in MAPS:
        xs = [engine.NHWC(torch.randn(batch, H, W, C, device="cuda").to(tdt), batch, H, W, C) for _ in range(BUFFERS)]
        bn = engine.BnActRunner(nn.BatchNorm2d(C).cuda().eval())
        inorm = engine.InstNormRunner(nn.InstanceNorm2d(Cn, affine=True).cuda().eval())
        with torch.no_grad():
            ga, keep_a = _graph_of(lambda x: bn.run(x, 1), xs)
            gb, keep_b = _graph_of(lambda x: inorm.run(x, 1), xs)
            _time(ga), _time(gb)
            ta, tb = [], []
            for _ in range(REPEATS):
                ta.append(_time(ga))
                tb.append(_time(gb))
        bytes_bn = 2 * batch * H * W * C * es
        bytes_in = bytes_bn + batch * H * W * Cn * es
        a, b = _median(ta), _median(tb)
        out.append(dict(tensor="{}x{}x{}x{}".format(batch, H, W, C), Cn=Cn, bn_act_us=round(a, 2), bn_act_us_min=round(min(ta), 2),
                        bn_act_us_max=round(max(ta), 2), bn_act_frac_8tbs=round(bytes_bn / (a * 1e-6) / HBM, 3),
                        instnorm_us=round(b, 2), instnorm_us_min=round(min(tb), 2), instnorm_us_max=round(max(tb), 2),
                        instnorm_frac_8tbs=round(bytes_in / (b * 1e-6) / HBM, 3), byte_ratio=round(bytes_in / bytes_bn, 3),
                        time_ratio=round(b / a, 3)))
        del ga, gb, keep_a, keep_b, xs
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
        raise SystemExit("bench_ibn.py measures on the GPU: no HIP device is visible")
    from pytorchcv_amd import engine
    from pytorchcv_amd.model_provider import get_model
    dtype = a.dtype or engine.compute_dtype_of(get_model("ibn_resnet50"))
    res = dict(workload="ibn_resnet50_bs{}".format(a.batch), dtype=dtype)
    if not a.no_kernel:
        res["instnorm_vs_bn_act"] = kernels(a.batch, dtype)
    if not a.no_net:
        res["nets"] = nets(a.batch)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
