"""
Timing of what follows the logits (GPU dev tool, not collected by pytest). Prints ONE JSON line:
  - pcv_classify_f32 at N=256, J=1000, k=5 with labels (ids, values, probabilities, rank, nll): the launch is far below the host's
    eager issue rate, so 20 launches are captured into a hipGraph and the replay is timed with device events (tests/tools/README.md);
    median / min / max per launch over `--replays` warm replays. Beside it the same for rank alone (k = 0), what `evaluate` launches.
  - `eval.evaluate` eager against `pipelined=True` on `--net` at batch 256 from 256 x 256 uint8 frames, `--batches` batches per call:
    device events around the whole call (the pipelined call includes its two graph captures), after one warm call of each;
    medians over `--reps` alternating repetitions, as images/s.
Usage: python tests/tools/classify_time.py [--net resnet50] [--batches 64] [--reps 3] [--out FILE]
"""

import os
import sys
import json
import argparse

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def graph_timed(fn, per_graph=20, replays=30, warmup=5):
    """us per call of `fn`, from replays of a graph of `per_graph` calls."""
    import torch
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fn()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(per_graph):
            fn()
    for _ in range(warmup):
        g.replay()
    torch.cuda.synchronize()
    ts = []
    for _ in range(replays):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        g.replay()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3 / per_graph)
    ts.sort()
    return dict(median_us=round(ts[len(ts) // 2], 2), min_us=round(ts[0], 2), max_us=round(ts[-1], 2), replays=replays,
                launches_per_replay=per_graph)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--net", default="resnet50")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--batches", type=int, default=64)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--replays", type=int, default=30)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    from pytorchcv_amd import engine, _lib, eval as ev
    from pytorchcv_amd.model_provider import get_model
    assert torch.cuda.is_available(), "classify_time.py needs a GPU"
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(1)

    N, J, k = 256, 1000, 5
    logits = torch.randn((N, J), generator=g).to(dev)
    labels = torch.randint(0, J, (N,), generator=g).to(dev)
    ids = torch.empty((N, k), dtype=torch.int32, device=dev)
    val = torch.empty((N, k), dtype=torch.float32, device=dev)
    prob = torch.empty((N, k), dtype=torch.float32, device=dev)
    rank = torch.empty((N,), dtype=torch.int32, device=dev)
    nll = torch.empty((N,), dtype=torch.float32, device=dev)
    L, ctx = _lib.lib(), engine._ctx(dev)

    def full():
        _lib.check(L.pcv_classify_f32(ctx, engine._ptr(logits), N, J, k, engine._ptr(ids), engine._ptr(val), engine._ptr(prob),
                                      engine._ptr(labels), engine._ptr(rank), engine._ptr(nll), engine._stream(dev)), ctx)

    def rank_only():
        _lib.check(L.pcv_classify_f32(ctx, engine._ptr(logits), N, J, 0, None, None, None, engine._ptr(labels), engine._ptr(rank), None,
                                      engine._stream(dev)), ctx)

    res = dict(tool="classify_time", N=N, J=J, k=k, launch_full=graph_timed(full, replays=a.replays),
               launch_rank_only=graph_timed(rank_only, replays=a.replays))

    net = get_model(a.net).eval().to(dev)
    frames = [torch.randint(0, 256, (a.batch, 256, 256, 3), generator=g, dtype=torch.uint8).to(dev) for _ in range(4)]
    labs = [torch.randint(0, 1000, (a.batch,), generator=g).to(dev) for _ in range(4)]
    batches = [(frames[i % 4], labs[i % 4]) for i in range(a.batches)]

    def timed(**kw):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = ev.evaluate(net, batches, **kw)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1), out

    warm_e, warm_p = timed()[1], timed(pipelined=True)[1]
    assert warm_e == warm_p, (warm_e, warm_p)
    te, tp = [], []
    for _ in range(a.reps):                                   # alternating: both see the same clocks
        te.append(timed()[0])
        tp.append(timed(pipelined=True)[0])
    te.sort()
    tp.sort()
    n_img = a.batch * a.batches
    res.update(net=a.net, dtype=engine.compute_dtype_of(net), batch=a.batch, batches=a.batches, reps=a.reps,
               evaluate_eager_ms=round(te[len(te) // 2], 2), evaluate_pipelined_ms=round(tp[len(tp) // 2], 2),
               evaluate_eager_img_per_s=round(n_img / (te[len(te) // 2] * 1e-3), 1),
               evaluate_pipelined_img_per_s=round(n_img / (tp[len(tp) // 2] * 1e-3), 1), results_equal=True)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
