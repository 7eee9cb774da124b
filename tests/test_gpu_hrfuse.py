"""
GPU: the HRNet fuse launch (csrc/hrfuse.hpp behind pcv_hr_fuse: up to four sources read through h >> shift, w >> shift, fp32 sum in
source order, activation, one rounding) against the CPU model of tests/hrfuse_ref.py with `torch.equal` - adds are IEEE and the
rounding is to nearest even on both sides, so there is no tolerance. The sweep and the power it has against eight bug models are
checked on the CPU by tests/test_hrfuse_model.py. y is filled with a sentinel before every launch: an element nobody writes, and a
refusal that launched anyway, show.
"""

import ctypes
import pytest
import torch
import util
import hrfuse_ref as R

pytestmark = pytest.mark.gpu

DTYPES = ["fp32", "bf16", "fp16"]
CODE = {"fp32": 0, "bf16": 1, "fp16": 2}
PCV_ERR_INVALID, PCV_ERR_TOO_LARGE = -1, -4
SENTINEL = -777.0
_IDS = [R.sweep_id(c) for c in R.SWEEP]


def _lib():
    from pytorchcv_amd import _lib as lb
    return lb, lb.lib(), lb.ctx_for(0)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream(0).cuda_stream)


def _ptrs(tensors):
    return (ctypes.c_void_p * len(tensors))(*[t.data_ptr() if t is not None else None for t in tensors])


def _ints(values):
    return (ctypes.c_int * len(values))(*values)


def _raw(srcs, shifts, y, N, H, W, C, act, code, nsrc=None, y_ptr="y"):
    """pcv_hr_fuse as a C caller makes it: (return code, text)"""
    lb, L, ctx = _lib()
    yp = (ctypes.c_void_p(y.data_ptr()) if y is not None else None) if y_ptr == "y" else y_ptr
    rc = L.pcv_hr_fuse(ctx, _ptrs(srcs), _ints(shifts), len(srcs) if nsrc is None else nsrc, yp, N, H, W, C, act, code, _stream())
    return rc, (L.pcv_last_error(ctx) or b"").decode()


def _launch(sources, shifts, H, W, act, dtype, dev):
    """through engine.hr_fuse, with engine.hr_fuse's own allocation replaced by nothing: the output is checked whole"""
    from pytorchcv_amd import engine
    hs = [engine.NHWC(s.to(dev), s.shape[0], s.shape[1], s.shape[2], s.shape[3]) for s in sources]
    y = engine.hr_fuse(hs, shifts, act)
    torch.cuda.synchronize()
    assert (y.N, y.H, y.W, y.C, y.cpitch) == (sources[0].shape[0], H, W, sources[0].shape[3], sources[0].shape[3])
    return y.t.cpu()


@pytest.mark.parametrize("act", [R.NONE, R.RELU], ids=["none", "relu"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("index", range(len(R.SWEEP)), ids=_IDS)
def test_kernel_equals_the_model_bit_for_bit(index, dtype, act, cuda_device):
    N, C, H, W, shifts = R.SWEEP[index]
    sources, want = R.sweep_reference(index, dtype, act)
    lb, L, ctx = _lib()
    assert L.pcv_hr_fuse_supported(len(shifts), _ints(shifts), N, H, W, C, act, CODE[dtype]) == 1
    got = _launch(sources, shifts, H, W, act, dtype, cuda_device)
    assert got.dtype == want.dtype and got.shape == want.shape
    assert torch.equal(got, want), "{} elements differ, max |d| {:.3e}".format(
        int((got != want).sum()), float((got.float() - want.float()).abs().max()))


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_capped_grid_writes_the_same_bits(dtype, cuda_device):
    """the 56x56 case with max_blocks = 2: 49 blocks' worth of work, so every block walks 24 or 25 rounds of the grid-stride loop; on
    the raw call, into a sentinel-filled y"""
    index = 4
    N, C, H, W, shifts = R.SWEEP[index]
    sources, want = R.sweep_reference(index, dtype, R.RELU)
    dev = cuda_device
    srcs = [s.to(dev) for s in sources]
    for cap in (2, 0):
        y = torch.full((N, H, W, C), SENTINEL, dtype=R.TORCH_DTYPES[dtype], device=dev)
        with util.tuning(max_blocks=cap):
            rc, text = _raw(srcs, shifts, y, N, H, W, C, R.RELU, CODE[dtype])
        torch.cuda.synchronize()
        assert rc == 0, text
        assert torch.equal(y.cpu(), want), "max_blocks={}".format(cap)


def test_fp16_guard_counts_a_sum_beyond_the_range_and_nothing_else(cuda_device):
    from pytorchcv_amd import engine
    dev = cuda_device

    def run(value, dtype):
        a = torch.full((1, 2, 2, 8), value, dtype=dtype, device=dev)
        b = torch.full((1, 1, 1, 8), value, dtype=dtype, device=dev)
        before = engine.fp16_overflow_count(dev)
        y = engine.hr_fuse([engine.NHWC(a, 1, 2, 2, 8), engine.NHWC(b, 1, 1, 1, 8)], [0, 1], R.RELU)
        return engine.fp16_overflow_count(dev) - before, y.t.float().cpu()

    moved, y = run(40000.0, torch.float16)             # two finite fp16 values, their sum 80000 is not one
    assert moved >= 1 and bool(torch.isinf(y).all())
    moved, y = run(30000.0, torch.float16)             # 60000 is
    assert moved == 0 and bool((y == 60000.0).all())
    moved, y = run(40000.0, torch.bfloat16)            # the guard is fp16's alone
    assert moved == 0 and bool(torch.isfinite(y).all())
    moved, y = run(-40000.0, torch.float16)            # relu(-80000) = 0: nothing beyond the range is rounded
    assert moved == 0 and bool((y == 0).all())


# what the launch refuses: (name, changes to an accepted call, a word of the text, expressible without pointers)
def _refusals(a, b, y):
    off = lambda t: ctypes.c_void_p(t.data_ptr() + 8)                              # noqa: E731
    return [
        ("no source", dict(nsrc=0), "sources", True),
        ("five sources", dict(srcs=[a, b, a, b, a], shifts=[0, 1, 0, 1, 0]), "sources", True),
        ("negative shift", dict(shifts=[0, -1]), "shift", True),
        ("shift 4", dict(shifts=[0, 4], H=16, W=16), "shift", True),
        ("relu6", dict(act=2), "activation", True),
        ("C % 8", dict(C=12), "multiple of 8", True),
        ("H does not divide", dict(H=5), "divide", True),
        ("W does not divide", dict(W=7), "divide", True),
        ("unknown dtype", dict(code=3), "dtype", True),
        ("empty", dict(N=0), "empty", True),
        ("NULL source", dict(srcs=[a, None]), "NULL", False),
        ("NULL y", dict(y_ptr=None), "NULL", False),
        ("misaligned source", dict(srcs=[a, off(b)]), "16-byte aligned", False),
        ("misaligned y", dict(y_ptr=off(y)), "16-byte aligned", False),
        ("y is a source", dict(srcs=[y, b]), "in-place", False),
    ]


def test_every_refusal_has_a_text_and_writes_nothing(cuda_device):
    dev = cuda_device
    lb, L, ctx = _lib()
    N, H, W, C = 2, 4, 6, 16
    a = torch.ones((N, H, W, C), dtype=torch.bfloat16, device=dev)
    b = torch.ones((N, H // 2, W // 2, C), dtype=torch.bfloat16, device=dev)
    y = torch.full((N, H, W, C), SENTINEL, dtype=torch.bfloat16, device=dev)
    base = dict(srcs=[a, b], shifts=[0, 1], N=N, H=H, W=W, C=C, act=R.RELU, code=1, nsrc=None, y_ptr="y")

    def call(kw):
        srcs = kw["srcs"]                              # tensors, None, or a raw (misaligned) address
        ptrs = (ctypes.c_void_p * len(srcs))(*[(s.data_ptr() if torch.is_tensor(s) else (s.value if s is not None else None))
                                               for s in srcs])
        yp = ctypes.c_void_p(y.data_ptr()) if kw["y_ptr"] == "y" else kw["y_ptr"]
        nsrc = len(srcs) if kw["nsrc"] is None else kw["nsrc"]
        rc = L.pcv_hr_fuse(ctx, ptrs, _ints(kw["shifts"]), nsrc, yp, kw["N"], kw["H"], kw["W"], kw["C"], kw["act"], kw["code"],
                           _stream())
        ok = L.pcv_hr_fuse_supported(nsrc, _ints(kw["shifts"]), kw["N"], kw["H"], kw["W"], kw["C"], kw["act"], kw["code"])
        return rc, (L.pcv_last_error(ctx) or b"").decode(), ok, (L.pcv_last_error(None) or b"").decode()

    rc, text, ok, _ = call(base)
    torch.cuda.synchronize()
    assert rc == 0 and ok == 1 and bool((y == 2).all())
    y.fill_(SENTINEL)
    for name, change, word, shape_only in _refusals(a, b, y):
        kw = dict(base)
        kw.update(change)
        rc, text, ok, why = call(kw)
        assert rc == PCV_ERR_INVALID, (name, rc)
        assert text.startswith("pcv_hr_fuse: ") and word in text, (name, text)
        # _supported answers the same question where it can be asked without pointers
        assert ok == (0 if shape_only else 1), name
        if shape_only:
            assert why.startswith("pcv_hr_fuse_supported: ") and word in why, (name, why)
    assert L.pcv_hr_fuse(None, _ptrs([a, b]), _ints([0, 1]), 2, ctypes.c_void_p(y.data_ptr()), N, H, W, C, 0, 1, _stream()) == PCV_ERR_INVALID
    # beyond the 2 GiB window: refused before any device call, so the small tensors behind the pointers are never touched
    big = dict(base, srcs=[a], shifts=[0], N=1 << 12, H=1 << 10, W=1 << 10, C=8, code=0)
    rc, text, ok, why = call(big)
    assert rc == PCV_ERR_TOO_LARGE and "2 GiB" in text and ok == 0 and "2 GiB" in why
    torch.cuda.synchronize()
    assert bool((y == SENTINEL).all())                 # nothing was launched


def test_engine_raises_where_the_kernel_refuses(cuda_device):
    from pytorchcv_amd import engine
    dev = cuda_device
    a = torch.ones((1, 4, 4, 8), dtype=torch.bfloat16, device=dev)
    ha = engine.NHWC(a, 1, 4, 4, 8)
    with pytest.raises(RuntimeError, match="activation"):
        engine.hr_fuse([ha, ha], [0, 0], 2)
    with pytest.raises(RuntimeError, match="sources"):
        engine.hr_fuse([ha] * 5, [0] * 5, 0)
    assert not engine.hr_fuse_supported([0, 4], 1, 16, 16, 8, 0, torch.bfloat16)
    assert engine.hr_fuse_supported([0, 3], 1, 16, 16, 8, 1, torch.bfloat16)
    torch.cuda.synchronize()


@pytest.mark.parametrize("dtype", DTYPES)
def test_graph_capture_equals_eager(dtype, cuda_device):
    """the launch neither allocates nor synchronises: captured and replayed it writes the eager bits"""
    dev = cuda_device
    index = 3
    N, C, H, W, shifts = R.SWEEP[index]
    sources, want = R.sweep_reference(index, dtype, R.RELU)
    srcs = [s.to(dev) for s in sources]
    static = torch.full((N, H, W, C), SENTINEL, dtype=R.TORCH_DTYPES[dtype], device=dev)
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):                      # warm-up on a side stream, as torch's capture rules ask
        lb, L, ctx = _lib()
        assert L.pcv_hr_fuse(ctx, _ptrs(srcs), _ints(shifts), len(srcs), ctypes.c_void_p(static.data_ptr()), N, H, W, C, R.RELU,
                             CODE[dtype], ctypes.c_void_p(side.cuda_stream)) == 0
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize()
    static.fill_(SENTINEL)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        assert L.pcv_hr_fuse(ctx, _ptrs(srcs), _ints(shifts), len(srcs), ctypes.c_void_p(static.data_ptr()), N, H, W, C, R.RELU,
                             CODE[dtype], st) == 0
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(static.cpu(), want)
