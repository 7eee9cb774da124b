"""CPU: the split-attention families (ResNeSt-A, SKNet) in the registry - construction through `get_model`, parameter counts
against the reference's (tests/golden/splat_param_counts.json, written by make_golden_splat.py from the imported reference) and
its metainfo table, state_dict layouts key for key against the fixture manifests, and the split-attention entry points of the
ABI refusing what they do not support before any device is touched."""

import os
import json
import pytest
import torch
import util

NAMES = ["resnestabc14", "resnesta18", "resnestabc26", "resnesta50", "resnesta101", "resnesta152", "resnesta200", "resnesta269",
         "sknet50", "sknet101", "sknet152"]
FIXTURE_NETS = ["resnesta18", "resnesta50", "sknet50"]


def _counts():
    with open(os.path.join(util.GOLDEN, "splat_param_counts.json")) as f:
        return json.load(f)


def _blocks_meta():
    with open(os.path.join(util.GOLDEN, "blocks_splat.json")) as f:
        return json.load(f)


def test_registry_holds_the_split_attention_families():
    from pytorchcv_amd.model_provider import _models
    assert len(_models) == 150
    assert all(n in _models for n in NAMES)


@pytest.mark.parametrize("name", NAMES)
def test_constructs_and_counts_match_reference(name):
    from pytorchcv_amd.model_provider import get_model
    from pytorchcv_amd.models.common.model_store import calc_net_weight_count, get_model_weight_count
    net = get_model(name)
    ref = _counts()[name]
    assert calc_net_weight_count(net) == ref["param_count"]
    assert len(net.state_dict()) == ref["key_count"]
    want = {"resnesta200": (256, 256), "resnesta269": (320, 320)}.get(name, (224, 224))
    assert tuple(net.in_size) == want
    if name.startswith("resnesta"):
        assert get_model_weight_count(name) == ref["param_count"]          # the metainfo row (model_metainfos.csv)


def test_lookup_is_case_insensitive_and_counts_are_the_published_ones():
    from pytorchcv_amd.model_provider import get_model
    from pytorchcv_amd.models.common.model_store import calc_net_weight_count
    from pytorchcv.model_provider import get_model as alias_get_model
    assert calc_net_weight_count(get_model("ResNeStA50")) == 27483240
    assert calc_net_weight_count(alias_get_model("SKNet50")) == _counts()["sknet50"]["param_count"]


@pytest.mark.parametrize("name", ["sknet50", "sknet101", "sknet152"])
def test_sknet_has_no_pretrained_weights(name, tmp_path):
    from pytorchcv_amd.model_provider import get_model
    with pytest.raises(ValueError, match="not available"):
        get_model(name, pretrained=True, root=str(tmp_path))


@pytest.mark.parametrize("name", FIXTURE_NETS)
def test_state_dict_matches_reference_manifest(name):
    from pytorchcv_amd.model_provider import get_model
    net = get_model(name)
    man = util.model_manifest(name)
    sd = net.state_dict()
    assert list(sd.keys()) == list(man["keys"].keys())
    for k, v in sd.items():
        shape, dt = man["keys"][k]
        assert list(v.shape) == shape and str(v.dtype).replace("torch.", "") == dt, k
    assert man["param_count"] == _counts()[name]["param_count"]
    net.load_state_dict(util.model_state(name, sd), strict=True)


def build_splat_block(case):
    """The pytorchcv_amd counterpart of a reference block case of blocks_splat.json."""
    from pytorchcv_amd.models.common.att import SABlock, saconv3x3_block
    from pytorchcv_amd.models.resnesta import ResNeStADownBlock, ResNeStAUnit, SEInitBlock
    from pytorchcv_amd.models.sknet import SKConvBlock
    ctor = {"SABlock": SABlock, "saconv3x3_block": saconv3x3_block, "SKConvBlock": SKConvBlock, "SEInitBlock": SEInitBlock,
            "ResNeStADownBlock": ResNeStADownBlock, "ResNeStAUnit": ResNeStAUnit}[case["kind"]]
    return ctor(**case["kwargs"]).eval()


@pytest.mark.parametrize("name", sorted(_blocks_meta()))
def test_block_state_dict_matches_reference_manifest(name):
    m = _blocks_meta()[name]
    blk = build_splat_block(m["case"])
    sd = blk.state_dict()
    assert {k: [list(v.shape), str(v.dtype).replace("torch.", "")] for k, v in sd.items()} == m["manifest"]
    blk.load_state_dict(util.synth_state_dict(util.template_from_manifest(m["manifest"]), seed=m["weight_seed"]), strict=True)


def test_split_attention_symbols_are_in_the_binding():
    from pytorchcv_amd import _lib
    for s in ("pcv_splat_squeeze", "pcv_splat_excite", "pcv_splat_combine", "pcv_avgpool2d_pad"):
        assert s in _lib.exported_symbols()
    assert _lib.PCV_ABI_VERSION == 5


def test_split_attention_entry_points_refuse_a_null_context():
    from pytorchcv_amd import _lib
    L = _lib.lib()
    assert L.pcv_splat_squeeze(None, None, None, 1, 1, 8, 2, 0, None) == -1
    assert L.pcv_splat_excite(None, None, None, None, None, None, None, None, None, 1, 8, 8, 2, 1, None) == -1
    assert L.pcv_splat_combine(None, None, None, None, None, 1, 1, 8, 2, 0, 0, None) == -1
    assert L.pcv_avgpool2d_pad(None, None, None, 1, 4, 4, 8, 3, 2, 1, 0, 1, 0, 0, None) == -1


def test_bn_fold_of_the_attention_mlp_is_exact_in_fp32():
    """SABlock's conv1 -> bn folds into one affine layer (the excite launch gets (w1, b1) already folded)."""
    from pytorchcv_amd.models.common.att import SABlock
    blk = SABlock(out_channels=64, groups=2, radix=2).eval()
    blk.load_state_dict(util.synth_state_dict(blk.state_dict(), seed=3), strict=True)
    w1, b1, w2, b2 = blk._mlp()
    s = torch.randn(3, 64)
    with torch.no_grad():
        ref = blk.bn(torch.nn.functional.conv2d(s[:, :, None, None], blk.conv1.weight, blk.conv1.bias))[:, :, 0, 0]
    assert torch.allclose(s @ w1.t() + b1, ref, rtol=1e-5, atol=1e-5)
    assert w2.shape == (128, 32) and b2.shape == (128,)


@pytest.mark.parametrize("name", ["resnesta18", "sknet50"])
def test_auto_dtype_is_fp16_on_every_module(name, monkeypatch):
    """bf16 misses the 1e-2 bound on resnesta50 / sknet50: "auto" is fp16 (+ range guard) for both families,
    on the net and on every sub-module called on its own."""
    from pytorchcv_amd import engine
    from pytorchcv_amd.model_provider import get_model
    monkeypatch.delenv("PCV_AMD_DTYPE", raising=False)
    net = get_model(name).eval()
    assert {engine.compute_dtype_of(m) for m in net.modules()} == {"fp16"}
