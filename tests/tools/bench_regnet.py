"""
RegNet measurement at batch 256 in the default mode (GPU dev tool, not collected by pytest). Without --net-step it is a DRIVER: for
regnetx002, regnety016, regnetx032 and regnety080 it starts one child process per net, each under `timeout` with a limit of its own,
and stops at the first child that does not exit 0 - a fault, an abort or a hang in one step starts nothing more on the GPU. Every
child prints ONE JSON line; the driver prints them and, with --out-dir, writes each to <dir>/<net>_bs<batch>.json.

A child measures images/s of the net with the grouped 3x3 layers on csrc/gconvx.hpp (the library's own routing) and on the generic
implicit GEMM (pcv_set_tuning("gconvx", 0)) from the same process and the same weights: two captured forwards (one lane, one stream)
replayed in turn, REPEATS rounds of STEPS steps, medians with minimum and maximum.

Usage: python tests/tools/bench_regnet.py [--out-dir profiles] [--batch 256] [--nets regnetx002,regnety016]
"""

import os
import sys
import json
import time
import argparse
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

NETS = ["regnetx002", "regnety016", "regnetx032", "regnety080"]
REPEATS, STEPS = 5, 10
LIMIT = 300                                            # seconds per child


def _median(v):
    v = sorted(v)
    return v[len(v) // 2]


def measure(name, batch):
    import torch
    import pytorchcv_amd
    from pytorchcv_amd import engine, _lib
    from pytorchcv_amd.graph import capture
    from pytorchcv_amd.model_provider import get_model
    from pytorchcv_amd.synth import synth_state_dict
    L, ctx = _lib.lib(), _lib.ctx_for(0)
    x = torch.randn(batch, 3, 224, 224, device="cuda")
    graphs = {}
    with torch.no_grad():
        net = get_model(name).eval()
        net.load_state_dict(synth_state_dict(net.state_dict(), seed=1234), strict=True)
        net = pytorchcv_amd.set_compute_dtype(net.cuda(), "auto")
        dtype = engine.compute_dtype_of(net)
        try:
            for tag, flag in (("gconvx", 1), ("generic", 0)):
                _lib.check(L.pcv_set_tuning(ctx, b"gconvx", flag), ctx)
                graphs[tag] = capture(net, x.clone(), own_input=True, lanes=1)
        finally:
            _lib.check(L.pcv_set_tuning(ctx, b"gconvx", 1), ctx)
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
    out = dict(workload="{}_bs{}".format(name, batch), net=name, dtype=dtype, batch=batch)
    for k, r in rates.items():
        out[k + "_img_per_s"] = round(_median(r), 1)
        out[k + "_img_per_s_min"] = round(min(r), 1)
        out[k + "_img_per_s_max"] = round(max(r), 1)
    out["gconvx_over_generic"] = round(out["gconvx_img_per_s"] / out["generic_img_per_s"], 4)
    return out


def driver(a):
    for name in a.nets.split(","):
        cmd = ["timeout", "-k", "10", str(LIMIT), sys.executable, os.path.abspath(__file__), "--net-step", name, "--batch", str(a.batch)]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        if p.returncode != 0:                          # a fault, an abort, a time limit: nothing more is started on the GPU
            sys.stdout.write(p.stdout)
            raise SystemExit("bench_regnet.py: {} ended with status {} - stopping".format(name, p.returncode))
        line = [ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1]
        print(line, flush=True)
        if a.out_dir:
            with open(os.path.join(a.out_dir, "{}_bs{}.json".format(name, a.batch)), "w") as f:
                f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--nets", default=",".join(NETS))
    ap.add_argument("--net-step", default="")
    ap.add_argument("--out-dir", default="")
    a = ap.parse_args()
    if a.net_step:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("bench_regnet.py measures on the GPU: no HIP device is visible")
        print(json.dumps(measure(a.net_step, a.batch)))
    else:
        driver(a)


if __name__ == "__main__":
    main()
