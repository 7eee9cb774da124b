"""CPU: the yardstick of the classify kernel (tests/classify_ref.py) against torch where torch is defined - rows without ties, NaN
or infinities -, the binding of pcv_classify_f32, its null-context refusal, and the `out=` checks of the preprocessing entries,
which refuse a wrong handle before anything is launched."""

import ctypes
import numpy as np
import pytest
import torch

import classify_ref as ref


def _distinct_rows(n, j, seed, scale=1.0):
    g = np.random.default_rng(seed)
    while True:
        x = (g.standard_normal((n, j)) * scale).astype(np.float32)
        if all(len(np.unique(r)) == j for r in x):
            return x


@pytest.mark.parametrize("j,k", [(1, 1), (2, 2), (10, 5), (257, 32), (1000, 5), (4097, 32)])
def test_restatement_matches_torch_on_plain_rows(j, k):
    from pytorchcv_amd import eval as ev
    x = _distinct_rows(6, j, seed=j, scale=3.0)
    t = torch.from_numpy(x)
    assert np.array_equal(ref.topk(x, k), t.topk(k, dim=1).indices.numpy())
    assert np.array_equal(ref.order(x), np.argsort(-x.astype(np.float64), axis=1, kind="stable"))
    p = torch.softmax(t.double(), dim=1).numpy()
    assert np.abs(ref.softmax64(x) - p).max() <= 1e-12
    g = np.random.default_rng(j + 1)
    labels = g.integers(0, j, x.shape[0])
    nll = torch.nn.functional.cross_entropy(t.double(), torch.from_numpy(labels), reduction="none").numpy()
    assert np.abs(ref.nll64(x, labels) - nll).max() <= 1e-12 * max(1.0, float(np.abs(x).max()))
    ks = tuple(kk for kk in (1, 5) if kk <= j)
    assert [ref.topk_error_count(x, labels, kk) for kk in ks] == ev.topk_errors(t, torch.from_numpy(labels), ks=ks)


def test_restatement_on_the_logits_of_test_topk_errors():
    from pytorchcv_amd import eval as ev
    logits = torch.tensor([[0.1, 0.9, 0.0, 0.3, 0.2, 0.05], [0.9, 0.1, 0.2, 0.3, 0.4, 0.5], [0.0, 0.1, 0.2, 0.3, 0.4, 0.5]])
    for labels, want in ((torch.tensor([1, 1, 0]), [2, 2]), (torch.tensor([1, 0, 5]), [0, 0])):
        assert ev.topk_errors(logits, labels, ks=(1, 5)) == want
        assert [ref.topk_error_count(logits.numpy(), labels.numpy(), k) for k in (1, 5)] == want


def test_restatement_states_the_order():
    """The issue's example row: torch.topk's answer depends on the build; the order's does not."""
    x = np.array([[1.0, np.nan, 3.0, 3.0, -0.0, 0.0, np.inf]], dtype=np.float32)
    assert ref.order(x).tolist() == [[1, 6, 2, 3, 0, 4, 5]]
    assert ref.rank(x, [3]).tolist() == [3] and ref.rank(x, [5]).tolist() == [6] and ref.rank(x, [4]).tolist() == [5]
    assert ref.rank(x, [-1]).tolist() == [7] and ref.rank(x, [7]).tolist() == [7]
    two_nans = np.array([[np.nan, 2.0, -np.nan]], dtype=np.float32)
    assert ref.order(two_nans).tolist() == [[0, 2, 1]]
    assert ref.natural_nan_row(np.array([[1, np.nan], [np.inf, 0], [-np.inf, -np.inf], [-np.inf, 0]], dtype=np.float32)).tolist() == \
        [True, True, True, False]


def test_binding_has_the_symbol_and_abi_is_still_5():
    from pytorchcv_amd import _lib
    L = _lib.lib()
    assert "pcv_classify_f32" in _lib.exported_symbols()
    assert L.pcv_classify_f32.restype is ctypes.c_int and len(L.pcv_classify_f32.argtypes) == 12
    assert L.pcv_abi_version() == _lib.PCV_ABI_VERSION == 5


def test_null_context_is_refused_before_any_device_is_touched():
    from pytorchcv_amd import _lib
    x = (ctypes.c_float * 4)(0.0, 1.0, 2.0, 3.0)
    ids = (ctypes.c_int * 2)()
    assert _lib.lib().pcv_classify_f32(None, ctypes.addressof(x), 2, 2, 1, ctypes.addressof(ids), None, None, None, None, None, None) == -1


def test_engine_classify_refuses_what_is_not_fp32_logits():
    from pytorchcv_amd import engine
    with pytest.raises(TypeError):
        engine.classify(torch.zeros(2, 3, dtype=torch.float64))
    with pytest.raises(TypeError):
        engine.classify(torch.zeros(6))


def _handle(n, size, c, dtype, wp=None):
    from pytorchcv_amd import engine
    wp = (size + 1) // 2 * 2 if wp is None else wp
    return engine.NHWC(torch.empty((n, size, wp, 4), dtype=dtype), n, size, size, c, wpitch=wp, cpitch=4)


@pytest.mark.parametrize("bad", ["batch", "size", "dtype", "channels", "not_a_handle"])
@pytest.mark.parametrize("entry", ["preprocess_u8", "preprocess_frames"])
def test_out_handle_of_wrong_shape_or_dtype_is_refused_before_any_launch(entry, bad):
    """CPU tensors: a launch would need a device context, which raises RuntimeError / TypeError - the ValueError comes first."""
    from pytorchcv_amd import eval as ev
    frames = torch.zeros((2, 64, 64, 3), dtype=torch.uint8)
    out = {"batch": _handle(3, 32, 3, torch.bfloat16), "size": _handle(2, 48, 3, torch.bfloat16), "dtype": _handle(2, 32, 3, torch.float16),
           "channels": _handle(2, 32, 1, torch.bfloat16), "not_a_handle": torch.empty((2, 32, 32, 4), dtype=torch.bfloat16)}[bad]
    with pytest.raises(ValueError, match="out="):
        getattr(ev, entry)(frames, img_size=32, dtype="bf16", out=out)


@pytest.mark.parametrize("entry", ["preprocess_u8", "preprocess_frames"])
def test_right_out_handle_passes_the_check(entry):
    from pytorchcv_amd import eval as ev
    frames = torch.zeros((2, 64, 64, 3), dtype=torch.uint8)
    with pytest.raises((RuntimeError, TypeError)):                     # CPU tensors get no further - but past the ValueError
        getattr(ev, entry)(frames, img_size=32, dtype="bf16", out=_handle(2, 32, 3, torch.bfloat16))
