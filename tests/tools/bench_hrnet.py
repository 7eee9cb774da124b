"""
HRNet measurement at batch 256 in the default mode (GPU dev tool, not collected by pytest). Without --step it is a DRIVER: for
hrnetv2_w18 and hrnetv2_w32 it starts one child process per step, each under `timeout` with a limit of its own, and stops at the first
child that does not exit 0 - a fault, an abort or a hang in one step starts nothing more on the GPU. Every child prints ONE JSON line;
the driver prints them and, with --out, writes them to that file. The steps:

  kernels  per distinct exchange shape of the net (output branch i of a B-branch HRBlock: pitch round8(width_i), map 56 >> i, shifts
           max(0, j - i)), captured graphs of launches that rotate over distinct tensor sets - as many as it takes for the inputs
           together to exceed ROTATE_BYTES, more than the 256 MB last-level cache, so that no launch finds its input left there by an
           earlier one - replayed alternately, REPEATS times each after a warm-up replay; medians per exchange:
             fused        one pcv_hr_fuse launch
             composed     the launches it replaces: engine.interpolate per coarse term + engine.add per term after the first
             se_scale     pcv_se_scale with a residual (two tensors in, one out) on a tensor of y's size: the bandwidth yardstick
           with the algorithmic bytes of each side, fused / composed time, and fused time per byte over se_scale's time per byte.
  nets     images/s of the net with the fused exchange and with the composed one (models/hrnet.py: FUSED) from the same process and
           the same weights: two captured forwards (one lane, one stream) replayed in turn, REPEATS rounds of STEPS steps, medians.

Usage: python tests/tools/bench_hrnet.py [--out profiles/hrnetv2_w18_bs256.json] [--batch 256] [--nets hrnetv2_w18,hrnetv2_w32]
"""

import os
import sys
import json
import time
import argparse
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

HBM = 8.0e12
MIN_BUFFERS, REPEATS = 4, 5
ROTATE_BYTES = 320 << 20
NETS = ["hrnetv2_w18", "hrnetv2_w32"]
STEPS = 10
LIMITS = {"kernels": 300, "nets": 300}                # seconds per child


def _median(v):
    v = sorted(v)
    return v[len(v) // 2]


def _graph_of(fn, n):
    """one call of fn on each of the n buffer sets, captured"""
    import torch
    for i in range(2):
        fn(i)
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
    return e0.elapsed_time(e1) * 1e3 / n               # microseconds per exchange


def exchange_shapes(net):
    """distinct (width, pitch, map size, shifts) of the net's exchanges at 224x224, with how many times a forward runs each"""
    from pytorchcv_amd import engine
    from pytorchcv_amd.models.hrnet import HRBlock
    seen = {}
    for blk in net.modules():
        if isinstance(blk, HRBlock) and blk.num_branches > 1:
            for i in range(blk.num_branches):
                key = (blk.in_channels_list[i], engine.round8(blk.in_channels_list[i]), 56 >> i,
                       tuple(max(0, j - i) for j in range(blk.num_branches)))
                seen[key] = seen.get(key, 0) + 1
    return sorted(seen.items(), key=lambda kv: (len(kv[0][3]), -kv[0][2]))


def kernels(name, batch, dtype):
    import torch
    from pytorchcv_amd import engine
    from pytorchcv_amd.model_provider import get_model
    tdt = engine.DTYPES[dtype][1]
    es = 4 if dtype == "fp32" else 2
    rows = []
    for (width, CP, S, shifts), count in exchange_shapes(get_model(name)):
        px = batch * S * S
        ybytes = px * CP * es
        src_bytes = [ybytes >> (2 * s) for s in shifts]
        BUFFERS = max(MIN_BUFFERS, -(-ROTATE_BYTES // sum(src_bytes)))

        def handle(s):
            return engine.NHWC(torch.randn(batch, S >> s, S >> s, CP, device="cuda").to(tdt), batch, S >> s, S >> s, width, cpitch=CP)
        sets = [[handle(s) for s in shifts] for _ in range(BUFFERS)]

        def fused(i):
            return engine.hr_fuse(sets[i], shifts, 1)

        def composed(i):
            y = None
            for k, (t, s) in enumerate(zip(sets[i], shifts)):
                if s > 0:
                    t = engine.interpolate(t, (S, S), False, False)
                y = t if y is None else engine.add(y, t, post_act=1 if k == len(shifts) - 1 else 0)
            return y

        gate = torch.ones((batch, CP), dtype=torch.float32, device="cuda")
        fine = [handle(0) for _ in range(BUFFERS)]

        def scale(i):
            return engine.se_scale(sets[i][0] if shifts[0] == 0 else fine[i], gate, fine[i], 1)

        coarse = any(s > 0 for s in shifts)
        with torch.no_grad():
            graphs = {"fused": _graph_of(fused, BUFFERS)}
            graphs["composed"] = _graph_of(composed, BUFFERS)
            graphs["se_scale"] = _graph_of(scale, BUFFERS)
            for g, _ in graphs.values():
                _time(g, BUFFERS)
            ts = {k: [] for k in graphs}
            for _ in range(REPEATS):
                for k, (g, _) in graphs.items():
                    ts[k].append(_time(g, BUFFERS))
        n_up = sum(1 for s in shifts if s > 0)
        nbytes = dict(fused=ybytes + sum(src_bytes),
                      composed=sum(b + ybytes for b, s in zip(src_bytes, shifts) if s > 0) + 3 * ybytes * (len(shifts) - 1),
                      se_scale=3 * ybytes)
        med = {k: _median(v) for k, v in ts.items()}
        row = dict(net=name, width=width, pitch=CP, map=S, shifts=list(shifts), per_forward=count, buffers=BUFFERS,
                   composed_launches=n_up + len(shifts) - 1, coarse=coarse)
        for k in graphs:
            row[k + "_us"] = round(med[k], 2)
            row[k + "_us_min"] = round(min(ts[k]), 2)
            row[k + "_us_max"] = round(max(ts[k]), 2)
        for k, b in nbytes.items():
            row[k + "_bytes"] = b
            row[k + "_frac_8tbs"] = round(b / (med[k] * 1e-6) / HBM, 3)
        row["fused_over_composed_time"] = round(med["fused"] / med["composed"], 3)
        row["fused_time_per_byte_vs_se_scale"] = round((med["fused"] / nbytes["fused"]) / (med["se_scale"] / nbytes["se_scale"]), 3)
        rows.append(row)
        del graphs, sets, fine
        torch.cuda.empty_cache()
    return rows


def nets(name, batch):
    import torch
    import pytorchcv_amd
    from pytorchcv_amd import engine
    from pytorchcv_amd.graph import capture
    from pytorchcv_amd.model_provider import get_model
    from pytorchcv_amd.models import hrnet
    from pytorchcv_amd.synth import synth_state_dict
    x = torch.randn(batch, 3, 224, 224, device="cuda")
    graphs = {}
    with torch.no_grad():
        net = get_model(name).eval()
        net.load_state_dict(synth_state_dict(net.state_dict(), seed=1234), strict=True)
        net = pytorchcv_amd.set_compute_dtype(net.cuda(), "auto")
        dtype = engine.compute_dtype_of(net)
        try:
            for tag, flag in (("fused", True), ("composed", False)):
                hrnet.FUSED = flag
                graphs[tag] = capture(net, x.clone(), own_input=True, lanes=1)
        finally:
            hrnet.FUSED = True
        for g in graphs.values():
            for _ in range(3):
                g(None)
        torch.cuda.synchronize()
        rates = {k: [] for k in graphs}
        for _ in range(REPEATS):
            for k, g in graphs.items():
                t0 = time.perf_counter()
                for _ in range(STEPS):
                    g(None)
                torch.cuda.synchronize()
                rates[k].append(batch * STEPS / (time.perf_counter() - t0))
    out = dict(net=name, dtype=dtype, batch=batch)
    for k, r in rates.items():
        out[k + "_img_per_s"] = round(_median(r), 1)
        out[k + "_img_per_s_min"] = round(min(r), 1)
        out[k + "_img_per_s_max"] = round(max(r), 1)
    out["fused_over_composed"] = round(out["fused_img_per_s"] / out["composed_img_per_s"], 4)
    return out


def child(a):
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_hrnet.py measures on the GPU: no HIP device is visible")
    from pytorchcv_amd import engine
    from pytorchcv_amd.model_provider import get_model
    dtype = a.dtype or engine.compute_dtype_of(get_model(a.net))
    res = dict(workload="{}_bs{}".format(a.net, a.batch), step=a.step, dtype=dtype)
    if a.step == "kernels":
        res["exchanges"] = kernels(a.net, a.batch, dtype)
    else:
        res["nets"] = nets(a.net, a.batch)
    print(json.dumps(res))


def driver(a):
    lines = []
    for name in a.nets.split(","):
        for step in ("kernels", "nets"):
            cmd = ["timeout", "-k", "10", str(LIMITS[step]), sys.executable, os.path.abspath(__file__), "--step", step, "--net", name,
                   "--batch", str(a.batch)] + (["--dtype", a.dtype] if a.dtype else [])
            p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
            if p.returncode != 0:                      # a fault, an abort, a time limit: nothing more is started on the GPU
                sys.stdout.write(p.stdout)
                raise SystemExit("bench_hrnet.py: step {} of {} ended with status {} - stopping".format(step, name, p.returncode))
            line = [ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1]
            print(line, flush=True)
            lines.append(line)
            if a.out:
                with open(a.out, "w") as f:
                    f.write("\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--dtype", default="")
    ap.add_argument("--nets", default=",".join(NETS))
    ap.add_argument("--step", default="", choices=["", "kernels", "nets"])
    ap.add_argument("--net", default=NETS[0])
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.step:
        child(a)
    else:
        driver(a)


if __name__ == "__main__":
    main()
