"""
Split-attention measurement for ResNeSt-A-50 at batch 256 (GPU dev tool, not collected by pytest): prints ONE JSON line with
  - the one-forward latency on one stream (eager, median of 5) and the `capture_best` throughput (images/s);
  - per split-attention / padded-pool launch of one forward: microseconds, algorithmic bytes (each tensor read or written
    once) and the fraction of 8 TB/s, from a `rocprofv3 --kernel-trace` run of this script in a child process (launches under
    ~40 us are not measurable eagerly from Python, tests/tools/README.md), and their share of the forward's kernel time.
Usage: python tests/tools/bench_splat.py [--out profiles/splat_resnesta50_bs256.json] [--no-prof]
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
SA_KERNELS = ("spatial_mean_kernel", "se_fc_kernel", "splat_softmax_kernel", "splat_combine_kernel", "avgpool_kernel")


def _net(batch):
    import torch
    import pytorchcv_amd
    from pytorchcv_amd.model_provider import get_model
    from pytorchcv_amd.synth import synth_state_dict
    net = get_model("resnesta50").eval()
    net.load_state_dict(synth_state_dict(net.state_dict(), seed=1234), strict=True)
    net = pytorchcv_amd.set_compute_dtype(net.cuda(), "auto")
    x = torch.randn(batch, 3, 224, 224, device="cuda")
    return net, x


def _record_launches(net, x):
    """(kind, bytes) of every split-attention / padded-pool launch of one forward, in launch order."""
    import torch
    from pytorchcv_amd import engine
    seq = []
    sa, pool = engine.splat_forward, engine.avgpool2d_pad

    def rec_sa(a, radix, groups, w1, b1, w2, b2, residual=None, post_act=0):
        es = a.t.element_size()
        n, hw, C = a.N, a.H * a.W, a.C // radix
        seq.append(("squeeze", n * hw * radix * C * es + n * C * 4))
        M = w1.shape[0]
        seq.append(("excite_fc1", (M * C + M) * 4 + n * (C + M) * 4))
        seq.append(("excite_fc2", (radix * C * M + radix * C) * 4 + n * (M + radix * C) * 4))
        seq.append(("excite_softmax", 2 * n * radix * C * 4))
        seq.append(("combine", n * hw * (radix * C + C * (2 if residual is not None else 1)) * es + n * radix * C * 4))
        return sa(a, radix, groups, w1, b1, w2, b2, residual, post_act)

    def rec_pool(a, k, s, p=0, ceil_mode=False, count_include_pad=True):
        y = pool(a, k, s, p, ceil_mode, count_include_pad)
        es = a.t.element_size()
        seq.append(("pool_k{}".format(k), (a.t.numel() + y.t.numel()) * es))
        return y

    engine.splat_forward, engine.avgpool2d_pad = rec_sa, rec_pool
    try:
        with torch.no_grad():
            net(x)
        torch.cuda.synchronize()
    finally:
        engine.splat_forward, engine.avgpool2d_pad = sa, pool
    return seq


def child(batch):
    """The profiled run: warm-up forward, then marker / forward / marker."""
    import torch
    net, x = _net(batch)
    with torch.no_grad():
        net(x)
        torch.cuda.synchronize()
        torch.cuda._sleep(1000)
        net(x)
        torch.cuda._sleep(1000)
    torch.cuda.synchronize()


def profile(batch, seq, stats_dir=None):
    """`stats_dir`: where to keep rocprofv3's per-kernel statistics of the profiled run (none kept when None)."""
    d = tempfile.mkdtemp(prefix="splat_prof_")
    try:
        return _profile(d, batch, seq, stats_dir)
    finally:
        shutil.rmtree(d, ignore_errors=True)


def _profile(d, batch, seq, stats_dir):
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "p", "--", sys.executable,
           os.path.abspath(__file__), "--child", "--batch", str(batch)]
    subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=900)
    f = (glob.glob(os.path.join(d, "**", "p_kernel_trace.csv"), recursive=True) or [None])[0]
    rows = list(csv.DictReader(open(f)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    marks = [i for i, r in enumerate(rows) if "spin_kernel" in r["Kernel_Name"]]      # torch.cuda._sleep
    fwd = rows[marks[-2] + 1:marks[-1]]
    total_us = sum(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in fwd) / 1e3
    sa_rows = [r for r in fwd if any(k in r["Kernel_Name"] for k in SA_KERNELS)]
    if sa_rows and "spatial_mean_kernel" in sa_rows[-1]["Kernel_Name"] and len(sa_rows) == len(seq) + 1:
        sa_rows = sa_rows[:-1]                          # the classifier's global pool, not split attention
    assert len(sa_rows) == len(seq), (len(sa_rows), len(seq))
    launches, sa_us, pool_us = [], 0.0, 0.0
    for r, (kind, nbytes) in zip(sa_rows, seq):
        us = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
        launches.append(dict(kind=kind, us=round(us, 2), bytes=int(nbytes), frac_8tbs=round(nbytes / (us * 1e-6) / HBM, 3)))
        if kind.startswith("pool"):
            pool_us += us
        else:
            sa_us += us
    big = [l for l in launches if l["kind"] in ("squeeze", "combine") and l["bytes"] >= 64 << 20]
    stats = (glob.glob(os.path.join(d, "**", "p_kernel_stats.csv"), recursive=True) or [None])[0]
    if stats and stats_dir:
        shutil.copy(stats, os.path.join(stats_dir, "splat_resnesta50_bs{}_kernel_stats.csv".format(batch)))
    return dict(forward_kernel_us=round(total_us, 1), split_attention_us=round(sa_us, 1), padded_pool_us=round(pool_us, 1),
                split_attention_share=round(sa_us / total_us, 4),
                min_frac_8tbs_squeeze_combine_ge_64MB=min((l["frac_8tbs"] for l in big), default=None),
                launches=launches)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--no-prof", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.child:
        return child(a.batch)
    import torch
    from pytorchcv_amd.graph import capture_best
    net, x = _net(a.batch)
    seq = _record_launches(net, x)
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
        thr = a.batch * steps / (time.perf_counter() - t0)
    from pytorchcv_amd import engine
    res = dict(workload="resnesta50_bs{}".format(a.batch), dtype=engine.compute_dtype_of(net), eager_forward_ms=round(sorted(ts[2:])[len(ts[2:]) // 2], 3),
               capture_best_img_per_s=round(thr, 1))
    if not a.no_prof:
        del g
        torch.cuda.empty_cache()
        res.update(profile(a.batch, seq, os.path.dirname(os.path.abspath(a.out)) if a.out else None))
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
