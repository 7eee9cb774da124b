"""GPU: pcv_classify_f32 (top-k ids / values / softmax probabilities, label rank, nll) against the numpy restatement of its order
(tests/classify_ref.py), exactly; probabilities and nll against float64 within bounds derived from fp32 arithmetic; input handles
through the captured launchers; pipelined evaluation against the eager one."""

import ctypes
import numpy as np
import pytest
import torch

import classify_ref as ref
import util

pytestmark = pytest.mark.gpu

JS = (1, 2, 10, 63, 64, 65, 200, 255, 256, 257, 1000, 1001, 4097, 16384)
NS = (1, 3, 257)
_cache = {}


def _sweep_batch(J):
    """257 rows of length J - row i is randn (i % 3 == 0), randn quantised to 4 levels (1) or one of the special rows (2), so the
    first row, the first three and all 257 each hold what their batch size can - with the restatement's order and, per batch size,
    the labels (uniform in [0, J) plus one -1 and one J) and their ranks. Computed once per J, never written to."""
    if J not in _cache:
        g = np.random.default_rng(1000 + J)
        sp = ref.special_rows(J, g)
        x = g.standard_normal((257, J)).astype(np.float32)
        x[1::3] = np.round(x[1::3] * 0.75).clip(-2, 1)                          # 4 levels: heavy ties
        idx = np.arange(2, 257, 3)
        x[idx] = sp[np.arange(len(idx)) % len(sp)]
        order = ref.order(x)[:, :min(J, 32)]
        labels = {}
        for N in NS:
            lab = g.integers(0, J, N).astype(np.int64)
            sets = [lab]
            if N >= 3:
                lab[N - 2], lab[N - 1] = -1, J
            else:                                                               # one row: one launch for each of the two
                sets += [np.full(N, -1, dtype=np.int64), np.full(N, J, dtype=np.int64)]
            labels[N] = [(l, ref.rank(x[:N], l)) for l in sets]
        _cache[J] = (x, order, labels)
    return _cache[J]


def _i32(t):
    return t.view(torch.int32).cpu().numpy()


@pytest.mark.parametrize("J", JS)
def test_exact_sweep(J, cuda_device):
    from pytorchcv_amd import engine
    x, order, labels = _sweep_batch(J)
    xd = torch.from_numpy(x).to(cuda_device)
    bits = x.view(np.int32)
    for N in NS:
        for k in sorted({1, min(J, 5), min(J, 32)}):
            for lab, want_rank in labels[N]:
                r = engine.classify(xd[:N], k=k, labels=torch.from_numpy(lab).to(cuda_device), probs=True, nll=True)
                ids = r["ids"].cpu().numpy()
                assert ids.dtype == np.int32 and ids.shape == (N, k)
                assert np.array_equal(ids, order[:N, :k]), (J, N, k)
                assert np.array_equal(_i32(r["values"]), np.take_along_axis(bits[:N], order[:N, :k], axis=1)), (J, N, k)
                rank = r["rank"].cpu().numpy()
                assert rank.dtype == np.int32 and np.array_equal(rank, want_rank), (J, N, k)
                nll = r["nll"].cpu().numpy()
                outside = (lab < 0) | (lab >= J)
                assert outside.any() or N < 3
                assert (rank[outside] == J).all() and np.isposinf(nll[outside]).all()


@pytest.mark.parametrize("scale", [1.0, 8.0])
def test_probabilities_and_nll_on_finite_rows(scale, cuda_device):
    """Bounds (conditions derived from fp32 arithmetic, not measurements): softmax terms are positive, so nothing cancels; the error
    is expf's ulps, one rounding of x - max (<= 2^-19 relative for |x - max| < 64), the roundings of the longest add chain and the
    division. An fp32 emulation with 256 strided partial sums and a tree stays <= 4.2e-6 relative (4.6 * 2^-24 scaled for nll) for
    every J here; the caps leave about 4x."""
    from pytorchcv_amd import engine
    worst_p, worst_n = 0.0, 0.0
    for J in JS:
        g = np.random.default_rng(77 + J)
        N, k = 5, min(J, 32)
        x = (g.standard_normal((N, J)) * scale).astype(np.float32)
        lab = g.integers(0, J, N).astype(np.int64)
        r = engine.classify(torch.from_numpy(x).to(cuda_device), k=k, labels=torch.from_numpy(lab).to(cuda_device), probs=True, nll=True)
        ids = r["ids"].cpu().numpy().astype(np.int64)
        assert np.array_equal(ids, ref.topk(x, k))
        p = r["probs"].cpu().numpy().astype(np.float64)
        p64 = np.take_along_axis(ref.softmax64(x), ids, axis=1)
        big = p64 >= 2.0 ** -120
        rel = np.abs(p[big] - p64[big]) / p64[big]
        worst_p = max(worst_p, float(rel.max()))
        assert rel.max() <= 2e-5, (J, float(rel.max()))
        assert (p[~big] <= 2.0 ** -119).all(), J
        nll = r["nll"].cpu().numpy().astype(np.float64)
        err = np.abs(nll - ref.nll64(x, lab)) / np.maximum(1.0, np.abs(x).max(axis=1))
        worst_n = max(worst_n, float(err.max()))
        assert err.max() <= 16 * 2.0 ** -24, (J, float(err.max()))
    print("scale {}: worst relative probability error {:.3e}, worst scaled nll error {:.3e} (= {:.2f} * 2^-24)".format(
        scale, worst_p, worst_n, worst_n * 2.0 ** 24))


@pytest.mark.parametrize("J", [1, 10, 257, 1001, 4097])
def test_special_rows_are_not_special_cased(J, cuda_device):
    """A NaN, a +inf or nothing but -inf: the natural computation gives NaN probabilities and a NaN nll, as torch.softmax does;
    every other special row (a -inf among finite values, zeros, equal values, ramps) stays finite."""
    from pytorchcv_amd import engine
    g = np.random.default_rng(5 + J)
    x = ref.special_rows(J, g)
    N, k = x.shape[0], min(J, 5)
    lab = g.integers(0, J, N).astype(np.int64)
    r = engine.classify(torch.from_numpy(x).to(cuda_device), k=k, labels=torch.from_numpy(lab).to(cuda_device), probs=True, nll=True)
    p, nll = r["probs"].cpu().numpy(), r["nll"].cpu().numpy()
    bad = ref.natural_nan_row(x)
    assert bad.sum() >= 7 and (~bad).sum() >= 4 or J == 1
    assert np.isnan(p[bad]).all() and np.isnan(nll[bad]).all()
    tp = torch.softmax(torch.from_numpy(x), dim=1).numpy()
    assert np.array_equal(np.isnan(tp).all(axis=1), bad) and np.array_equal(np.isnan(tp).any(axis=1), bad)
    assert np.isfinite(p[~bad]).all() and not np.isnan(nll[~bad]).any()
    assert np.array_equal(r["ids"].cpu().numpy(), ref.topk(x, k)) and np.array_equal(r["rank"].cpu().numpy(), ref.rank(x, lab))


@pytest.mark.parametrize("J", [1000, 4097])
def test_outputs_do_not_depend_on_the_batch_position(J, cuda_device):
    from pytorchcv_amd import engine
    g = np.random.default_rng(J)
    x = g.standard_normal((257, J)).astype(np.float32)
    x[[0, 1, 256]] = np.round(g.standard_normal(J) * 4).astype(np.float32) / 4      # ties included
    lab = g.integers(0, J, 257).astype(np.int64)
    lab[[0, 1, 256]] = J // 3
    r = engine.classify(torch.from_numpy(x).to(cuda_device), k=32, labels=torch.from_numpy(lab).to(cuda_device), probs=True, nll=True)
    for name in ("ids", "values", "probs", "rank", "nll"):
        v = _i32(r[name])
        assert np.array_equal(v[0], v[1]) and np.array_equal(v[0], v[256]), name


def test_refusals_name_the_limit(cuda_device):
    from pytorchcv_amd import engine, _lib
    x = torch.zeros((2, 10), device=cuda_device)
    with pytest.raises(_lib.PcvError, match=r"k = 11 .*k <= min\(J, 32\)"):
        engine.classify(x, k=11)
    with pytest.raises(_lib.PcvError, match=r"k = 33 .*k <= min\(J, 32\)"):
        engine.classify(torch.zeros((2, 100), device=cuda_device), k=33)
    with pytest.raises(_lib.PcvError, match=r"J = 16385 .*J <= 16384"):
        engine.classify(torch.zeros((1, 16385), device=cuda_device), k=1)
    with pytest.raises(_lib.PcvError, match="need labels"):
        engine.classify(x, k=1, nll=True)
    rank = torch.zeros(2, dtype=torch.int32, device=cuda_device)
    ctx = engine._ctx(cuda_device)
    with pytest.raises(_lib.PcvError, match="rank and nll need labels"):                 # rank requested without labels
        _lib.check(_lib.lib().pcv_classify_f32(ctx, engine._ptr(x), 2, 10, 0, None, None, None, None, engine._ptr(rank), None,
                                               engine._stream(cuda_device)), ctx)
    with pytest.raises(_lib.PcvError, match="k = 0 is allowed only"):
        _lib.check(_lib.lib().pcv_classify_f32(ctx, engine._ptr(x), 2, 10, 0, engine._ptr(rank), None, None, None, None, None,
                                               engine._stream(cuda_device)), ctx)
    torch.cuda.synchronize()
    assert int(rank.abs().sum()) == 0                                                    # nothing was launched


def test_labels_of_any_integer_dtype_and_ranks_alone(cuda_device):
    from pytorchcv_amd import engine, eval as ev
    x, _, _ = _sweep_batch(200)
    lab = np.random.default_rng(3).integers(0, 200, 257)
    want = ref.rank(x, lab)
    xd = torch.from_numpy(x).to(cuda_device)
    for dt in (torch.int64, torch.int32, torch.int16, torch.uint8):
        r = engine.classify(xd, labels=torch.from_numpy(lab).to(dt))                     # k = 0, CPU labels: moved on the device
        assert sorted(r) == ["rank"] and np.array_equal(r["rank"].cpu().numpy(), want)
    assert np.array_equal(ev.label_ranks(xd, torch.from_numpy(lab).to(cuda_device)).cpu().numpy(), want)


# ---- through the nets ------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def resnet18(cuda_device):
    import pytorchcv_amd
    from pytorchcv_amd.model_provider import get_model
    net = get_model("resnet18").eval()
    net.load_state_dict(util.model_state("resnet18", net.state_dict()), strict=True)
    return pytorchcv_amd.set_compute_dtype(net.to(cuda_device), "fp32")


@pytest.fixture(scope="module")
def frame_batches(cuda_device):
    """Seven batches of different 256 x 256 uint8 frames: six of four, one of two."""
    g = torch.Generator().manual_seed(11)
    return [torch.randint(0, 256, (n, 256, 256, 3), generator=g, dtype=torch.uint8).to(cuda_device) for n in (4,) * 6 + (2,)]


@pytest.fixture(scope="module")
def eager_logits(resnet18, frame_batches):
    from pytorchcv_amd import eval as ev
    with torch.no_grad():
        out = [resnet18(ev.preprocess_u8(f, dtype="fp32")).clone() for f in frame_batches]
    torch.cuda.synchronize()
    return out


def test_graphed_net_takes_an_input_handle(resnet18, frame_batches, eager_logits, cuda_device):
    from pytorchcv_amd import eval as ev, graph
    h = ev.preprocess_u8(frame_batches[0], dtype="fp32")
    g = graph.GraphedNet(resnet18, h)
    assert g.static_in is h and g.lanes == 1
    assert torch.equal(g(None), eager_logits[0])
    assert ev.preprocess_u8(frame_batches[1], dtype="fp32", out=h) is h          # refilled in place
    assert torch.equal(g(None), eager_logits[1])
    assert not torch.equal(eager_logits[0], eager_logits[1])
    with pytest.raises(RuntimeError):
        g(torch.zeros((4, 3, 224, 224), device=cuda_device))
    with pytest.raises(ValueError, match="lanes"):
        graph.GraphedNet(resnet18, h, lanes=2)
    with pytest.raises(ValueError, match="lanes"):
        graph.PipelinedNet(resnet18, h, lanes=2)


def test_pipelined_evaluate_equals_eager(resnet18, frame_batches, eager_logits):
    from pytorchcv_amd import eval as ev
    six = eager_logits[:6]
    top = [l.sort(dim=1, descending=True) for l in eager_logits]
    for t in top:                                                               # a precondition of the inputs, not of the code
        assert bool((t.values[:, :7] > t.values[:, 1:8]).all()), "two equal logits among a row's top 8: choose other frames"
    labels = [t.indices[:, 0] if i % 2 == 0 else t.indices[:, 6] for i, t in enumerate(top[:6])]
    labels.append(top[6].indices[:, 0])

    def counts(n_batches):
        w = [0, 0]
        for l, lab in zip(eager_logits[:n_batches], labels):
            for i, c in enumerate(ev.topk_errors(l, lab, ks=(1, 5))):
                w[i] += c
        return w

    batches = list(zip(frame_batches, labels))
    eager = ev.evaluate(resnet18, batches[:6])
    piped = ev.evaluate(resnet18, batches[:6], pipelined=True)                  # depth 2, six batches: every slot is reused twice
    assert eager == piped == {"n": 24, "top1_err": 50.0, "top5_err": 50.0}
    assert counts(6) == [12, 12] and len(six) == 6
    eager7 = ev.evaluate(resnet18, batches, loss=True)
    piped7 = ev.evaluate(resnet18, batches, loss=True, pipelined=True)          # the batch of two takes the eager path
    w = counts(7)
    assert w == [12, 12]
    assert eager7["n"] == piped7["n"] == 26
    assert eager7["top1_err"] == piped7["top1_err"] == 100.0 * w[0] / 26
    assert eager7["top5_err"] == piped7["top5_err"] == 100.0 * w[1] / 26
    assert eager7["nll"] == piped7["nll"] and np.isfinite(eager7["nll"])        # bit for bit
    want = float(np.mean(np.concatenate([ref.nll64(l.cpu().numpy(), lab.cpu().numpy()) for l, lab in zip(eager_logits, labels)])))
    scale = max(1.0, max(float(l.abs().max()) for l in eager_logits))
    assert abs(eager7["nll"] - want) <= 16 * 2.0 ** -24 * scale


def test_predict(resnet18, frame_batches, eager_logits):
    from pytorchcv_amd import eval as ev
    ids, probs = ev.predict(resnet18, ev.preprocess_u8(frame_batches[2], dtype="fp32"), k=5)
    x = eager_logits[2].cpu().numpy()
    want = ref.topk(x, 5)
    assert ids.dtype == torch.int32 and np.array_equal(ids.cpu().numpy(), want)
    p64 = np.take_along_axis(ref.softmax64(x), want, axis=1)
    assert (np.abs(probs.cpu().numpy() - p64) <= 2e-5 * p64).all()
