"""
MixNet measurement at batch 256 in the default mode (GPU dev tool, not collected by pytest): prints ONE JSON line with
  - the one-forward latency on one stream (eager, median of 5) and the `capture_best` throughput (images/s) of mixnet_s, and of
    efficientnet_b0 from the same run (the nearest family: the same unit with one window size per layer);
  - for every distinct depthwise MixConv shape of mixnet_s and mixnet_m: microseconds of pcv_mixconv2d_fused (median of the timed
    rounds), algorithmic bytes (x read once, y written once) and the fraction of 8 TB/s, and next to it the yardstick on the same
    tensor: pcv_dwconv2d_fused 5x5 over all channels at the same stride. `accept_35`: every (3, 5) MixConv within 1.05 x its
    yardstick (it does no more arithmetic and moves the same bytes);
  - the two-group 1x1 MixConv layers of mixnet_s (they run at twice their FLOPs on the block-diagonal grouped path): microseconds
    per distinct layer and their share of the kernel time of one forward.
The times come from ONE `rocprofv3 --kernel-trace` run of this script in a fresh child process (launches under ~40 us are not
measurable eagerly from Python, tests/tools/README.md); the rounds alternate yardstick and kernel. No counters in that run.
Usage: python tests/tools/bench_mixnet.py [--out profiles/mixnet_s_bs256.json] [--no-prof] [--no-net]
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
ROUNDS = 7                                                      # timed rounds per shape (after one warm-up round)
MARKER = "nhwc_to_nchw_kernel"                                  # a launch no forward contains: separates the sections of the trace
FORWARDS = 3


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


def layers(names):
    """Distinct MixConv layers of the nets, from one batch-1 forward each: depthwise (C, G, stride, H, W) and - first net only -
    pointwise [(Cin, Cout, H, W, act, residual), count]."""
    import torch
    from pytorchcv_amd import engine
    from pytorchcv_amd.models.mixnet import MixConvBlock
    dw, pw = [], {}
    for i, name in enumerate(names):
        net, x = _net(name, 1)
        hooks = []

        def seen(m, args, kwargs, first=(i == 0)):
            a = args[0]
            if m.conv.depthwise:
                key = (a.C, len(m.conv.convs()), m.conv.convs()[0].stride[0], a.H, a.W)
                if key not in dw:
                    dw.append(key)
            elif first:
                key = (a.C, sum(c.out_channels for c in m.conv.convs()), a.H, a.W, engine.act_code(m.activ) if m.activate else 0,
                       kwargs.get("residual") is not None)
                pw[key] = pw.get(key, 0) + 1
        for m in net.modules():
            if isinstance(m, MixConvBlock):
                hooks.append(m.register_forward_pre_hook(seen, with_kwargs=True))
        with torch.no_grad():
            net(x)
        torch.cuda.synchronize()
        for h in hooks:
            h.remove()
        del net
    return dw, [list(k) + [n] for k, n in pw.items()]


def child(batch, dtype, spec):
    """The profiled run: marker, the depthwise rounds, marker, per pointwise layer its rounds and a marker, FORWARDS forwards of
    mixnet_s, marker."""
    import torch
    import torch.nn as nn
    import pytorchcv_amd
    from pytorchcv_amd import engine
    from pytorchcv_amd.models.mixnet import mixconv1x1_block
    from pytorchcv_amd.models.common.activ import lambda_relu, lambda_swish
    tdt = engine.DTYPES[dtype][1]
    net, xin = _net("mixnet_s", batch)
    with torch.no_grad():
        net(xin)                                                  # packs every layer before the first marker
    tiny = engine.NHWC(torch.zeros(1, 1, 1, 8, device="cuda", dtype=tdt), 1, 1, 1, 8)

    def marker():
        torch.cuda.synchronize()
        engine.to_nchw(tiny)
        torch.cuda.synchronize()

    def handle(N, H, W, C):
        return engine.NHWC(torch.randn(N, H, W, C, device="cuda").to(tdt), N, H, W, C)
    marker()
    for C, G, s, H, W in spec["dw"]:
        convs = [nn.Conv2d(C // G, C // G, 3 + 2 * g, s, 1 + g, groups=C // G, bias=False).cuda().eval() for g in range(G)]
        mix = engine.MixConvRunner(convs, nn.BatchNorm2d(C).cuda().eval())
        five = engine.ConvRunner(nn.Conv2d(C, C, 5, s, 2, groups=C, bias=False).cuda().eval(), nn.BatchNorm2d(C).cuda().eval())
        a = handle(batch, H, W, C)
        for _ in range(ROUNDS + 1):
            five.run(a, act=4)
            mix.run(a, act=4)
        torch.cuda.synchronize()
        del a, mix, five
        torch.cuda.empty_cache()
    marker()
    for cin, cout, H, W, act, res, _ in spec["pw"]:
        blk = mixconv1x1_block(in_channels=cin, out_channels=cout, kernel_count=2,
                               activation={0: None, 1: lambda_relu(), 4: lambda_swish()}[act]).eval().cuda()
        blk = pytorchcv_amd.set_compute_dtype(blk, dtype)
        a = handle(batch, H, W, cin)
        r = handle(batch, H, W, cout) if res else None
        with torch.no_grad():
            for _ in range(ROUNDS + 1):
                blk(a, residual=r)
        del a, r, blk
        torch.cuda.empty_cache()
        marker()                                                  # one section per layer: its setup launches stay out of the next
    with torch.no_grad():
        for _ in range(FORWARDS):
            net(xin)
    marker()


def _us(r):
    return (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3


def _median(rows):
    us = sorted(_us(r) for r in rows)
    return us[len(us) // 2], us[0], us[-1]


def profile(batch, dtype, spec):
    d = tempfile.mkdtemp(prefix="mixnet_prof_")
    try:
        cmd = ["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", d, "-o", "p", "--", sys.executable,
               os.path.abspath(__file__), "--child", "--batch", str(batch), "--dtype", dtype, "--spec", json.dumps(spec)]
        subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=900)
        f = (glob.glob(os.path.join(d, "**", "p_kernel_trace.csv"), recursive=True) or [None])[0]
        rows = list(csv.DictReader(open(f)))
    finally:
        shutil.rmtree(d, ignore_errors=True)
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    marks = [i for i, r in enumerate(rows) if MARKER in r["Kernel_Name"]]
    assert len(marks) == 3 + len(spec["pw"]), len(marks)
    secs = [rows[a + 1:b] for a, b in zip(marks, marks[1:])]
    sec_dw, secs_pw, sec_fwd = secs[0], secs[1:-1], secs[-1]
    es = 4 if dtype == "fp32" else 2
    out = []
    timed = [r for r in sec_dw if "dwconv5_kernel" in r["Kernel_Name"] or "mixdw_kernel" in r["Kernel_Name"]]
    per = 2 * (ROUNDS + 1)
    assert len(timed) == per * len(spec["dw"]), (len(timed), per * len(spec["dw"]))
    for i, (C, G, s, H, W) in enumerate(spec["dw"]):
        block = timed[i * per:(i + 1) * per]
        five, mix = block[0::2][1:], block[1::2][1:]              # [0] of each is the warm-up round
        assert all("dwconv5_kernel" in r["Kernel_Name"] for r in five) and all("mixdw_kernel" in r["Kernel_Name"] for r in mix)
        Ho, Wo = (H - 1) // s + 1, (W - 1) // s + 1
        nbytes = batch * (H * W + Ho * Wo) * C * es
        (m, mlo, mhi), (y, ylo, yhi) = _median(mix), _median(five)
        out.append(dict(tensor="{}x{}x{}x{}".format(batch, H, W, C), kernels=[3 + 2 * g for g in range(G)], stride=s, bytes=int(nbytes),
                        us=round(m, 2), us_min=round(mlo, 2), us_max=round(mhi, 2), frac_8tbs=round(nbytes / (m * 1e-6) / HBM, 3),
                        dw5x5_us=round(y, 2), dw5x5_us_min=round(ylo, 2), dw5x5_us_max=round(yhi, 2),
                        dw5x5_frac_8tbs=round(nbytes / (y * 1e-6) / HBM, 3), over_dw5x5=round(m / y, 3)))
    res = dict(mixconv=out, accept_35=all(o["over_dw5x5"] <= 1.05 for o in out if o["kernels"] == [3, 5]))
    fwd_us = sum(_us(r) for r in sec_fwd) / FORWARDS
    res["forward_kernel_us"] = round(fwd_us, 1)
    res["forward_mixdw_us"] = round(sum(_us(r) for r in sec_fwd if "mixdw_kernel" in r["Kernel_Name"]) / FORWARDS, 1)
    pw, total, odd = [], 0.0, []
    for sec, (cin, cout, H, W, act, r_, count) in zip(secs_pw, spec["pw"]):
        # the layer's own launches: the one kernel name that occurs once per round (pack / fold launches occur once per layer)
        names = [r["Kernel_Name"] for r in sec]
        conv = [r for r in sec if names.count(r["Kernel_Name"]) == ROUNDS + 1]
        if len(conv) != ROUNDS + 1:
            odd.append("{}->{}: {} launches".format(cin, cout, len(conv)))
            continue
        m, lo, hi = _median(conv[1:])
        total += m * count
        pw.append(dict(layer="{}->{} @{}x{}".format(cin, cout, H, W), count=count, kernel=conv[0]["Kernel_Name"].split("<")[0][-24:],
                       us=round(m, 2), us_min=round(lo, 2), us_max=round(hi, 2)))
    if odd:
        res["pointwise_2group"] = "unmeasured: " + "; ".join(odd)
    else:
        res.update(pointwise_2group=pw, pointwise_2group_us_per_forward=round(total, 1),
                   pointwise_2group_share_of_forward=round(total / fwd_us, 3))
    return res


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
    ap.add_argument("--spec", default="")
    ap.add_argument("--no-prof", action="store_true")
    ap.add_argument("--no-net", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.child:
        return child(a.batch, a.dtype, json.loads(a.spec))
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_mixnet.py measures on the GPU: no HIP device is visible")
    from pytorchcv_amd import engine
    from pytorchcv_amd.model_provider import get_model
    dtype = a.dtype or engine.compute_dtype_of(get_model("mixnet_s"))
    res = dict(workload="mixnet_s_bs{}".format(a.batch), dtype=dtype)
    if not a.no_net:
        d, ms, thr = throughput("mixnet_s", a.batch)
        assert d == dtype or a.dtype
        res.update(eager_forward_ms=ms, capture_best_img_per_s=thr)
        d, ms, thr = throughput("efficientnet_b0", a.batch)
        res.update(efficientnet_b0=dict(dtype=d, eager_forward_ms=ms, capture_best_img_per_s=thr))
    if not a.no_prof:
        dw, pw = layers(["mixnet_s", "mixnet_m"])
        res.update(profile(a.batch, dtype, dict(dw=dw, pw=pw)))
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
