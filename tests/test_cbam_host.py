"""CPU: CBAM-ResNet in the registry - construction through `get_model` and the alias, parameter counts against the reference's
(tests/golden/cbam_param_counts.json, written by make_golden_cbam.py from the imported reference) and its metainfo rows, state_dict
layouts key for key against the fixture manifests, and the four CBAM entry points of the ABI refusing what they do not support
before any device is touched."""

import os
import json
import pytest
import torch
import util

NAMES = ["cbam_resnet18", "cbam_resnet34", "cbam_resnet50", "cbam_resnet101", "cbam_resnet152"]
FIXTURE_NETS = ["cbam_resnet18", "cbam_resnet50"]
PUBLISHED = {"cbam_resnet18": 11779392, "cbam_resnet34": 21960468, "cbam_resnet50": 28089624, "cbam_resnet101": 49330172,
             "cbam_resnet152": 66826848}            # the reference's own asserts
SYMBOLS = ("pcv_cbam_pool", "pcv_cbam_excite", "pcv_cbam_spatial_pool", "pcv_cbam_apply")


def _counts():
    with open(os.path.join(util.GOLDEN, "cbam_param_counts.json")) as f:
        return json.load(f)


def blocks_meta():
    with open(os.path.join(util.GOLDEN, "blocks_cbam.json")) as f:
        return json.load(f)


def build_cbam_block(case):
    """The pytorchcv_amd counterpart of a reference block case of blocks_cbam.json."""
    from pytorchcv_amd.models.cbamresnet import CbamBlock, CbamResUnit
    return {"CbamBlock": CbamBlock, "CbamResUnit": CbamResUnit}[case["kind"]](**case["kwargs"]).eval()


def test_registry_keeps_its_first_table_and_adds_a_second():
    from pytorchcv_amd.model_provider import _models, _models_cbam
    assert len(_models) == 150
    assert sorted(_models_cbam) == sorted(NAMES)
    assert not set(_models) & set(_models_cbam)


@pytest.mark.parametrize("name", NAMES)
def test_constructs_and_counts_match_reference(name):
    from pytorchcv_amd.model_provider import get_model
    from pytorchcv_amd.models.cbamresnet import CbamResNet
    from pytorchcv_amd.models.common.model_store import calc_net_weight_count, get_model_weight_count
    net = get_model(name)
    ref = _counts()[name]
    assert isinstance(net, CbamResNet) and tuple(net.in_size) == (224, 224) and net.num_classes == 1000
    assert calc_net_weight_count(net) == ref["param_count"] == PUBLISHED[name]
    assert len(net.state_dict()) == ref["key_count"]
    assert get_model_weight_count(name) == ref["param_count"]                  # the metainfo row (model_metainfos.csv)


def test_lookup_is_case_insensitive_and_the_alias_resolves_every_name():
    from pytorchcv_amd.model_provider import get_model
    from pytorchcv_amd.models.common.model_store import calc_net_weight_count
    from pytorchcv.model_provider import get_model as alias_get_model
    assert calc_net_weight_count(get_model("CBAM_ResNet50")) == PUBLISHED["cbam_resnet50"]
    for name in NAMES:
        assert type(alias_get_model(name.upper())).__name__ == "CbamResNet"
    with pytest.raises(ValueError, match="Unsupported model: cbam_resnet19"):
        get_model("cbam_resnet19")


def test_metainfo_rows_are_the_references():
    from pytorchcv_amd.models.common.model_store import get_model_metainfo_dict
    from pytorchcv_amd.models.cbamresnet import get_resnet
    table = get_model_metainfo_dict()
    assert table["cbam_resnet50"] == (28089624, "0505", "d8cf8488efb97afecd6b3287a3ca9fa093fc3127", "v0.0.537")
    for name in NAMES:
        if name != "cbam_resnet50":
            assert table[name] == (PUBLISHED[name], "NA", "NA", "NA")
    with pytest.raises(ValueError, match="Unsupported CBAM-ResNet with number of blocks: 26"):
        get_resnet(blocks=26)


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
    keys = "\n".join(sd)
    for attr in ("cbam.ch_gate.mlp.fc1.weight", "cbam.ch_gate.mlp.fc2.bias", "cbam.sp_gate.conv.conv.weight",
                 "cbam.sp_gate.conv.bn.running_var", "body.conv1.conv.weight", "identity_conv.conv.weight"):
        assert attr in keys


@pytest.mark.parametrize("name", sorted(blocks_meta()))
def test_block_state_dict_matches_reference_manifest(name):
    m = blocks_meta()[name]
    blk = build_cbam_block(m["case"])
    sd = blk.state_dict()
    assert {k: [list(v.shape), str(v.dtype).replace("torch.", "")] for k, v in sd.items()} == m["manifest"]
    blk.load_state_dict(util.synth_state_dict(util.template_from_manifest(m["manifest"]), seed=m["weight_seed"]), strict=True)
    lo, hi = m["channel_gate_range"]
    assert hi - lo >= 0.3                              # the fixtures exercise both gates (make_golden_cbam.py refuses less)
    lo, hi = m["spatial_gate_range"]
    assert hi - lo >= 0.4


def test_spatial_gate_stencil_is_the_folded_batchnorm():
    from pytorchcv_amd.models.cbamresnet import SpatialGate
    g = SpatialGate().eval()
    g.load_state_dict(util.synth_state_dict(g.state_dict(), seed=11), strict=True)
    w7, scale, shift = g.stencil()
    assert w7.shape == (2, 7, 7) and scale.shape == (1,) and shift.shape == (1,)
    z = torch.randn(1, 1, 3, 3)
    with torch.no_grad():
        assert torch.allclose(g.conv.bn(z), z * scale + shift, rtol=1e-6, atol=1e-6)
    assert g.stencil()[0] is w7                        # cached until a parameter changes
    with torch.no_grad():
        g.conv.bn.bias.add_(1.0)
    assert torch.allclose(g.stencil()[2], shift + 1.0)


def test_cbam_symbols_are_in_the_binding_and_the_abi_version_stays():
    from pytorchcv_amd import _lib
    for s in SYMBOLS:
        assert s in _lib.exported_symbols()
        assert hasattr(_lib.lib(), s)
    assert _lib.PCV_ABI_VERSION == 5 == _lib.lib().pcv_abi_version()


def test_cbam_entry_points_refuse_a_null_context():
    from pytorchcv_amd import _lib
    L = _lib.lib()
    assert L.pcv_cbam_pool(None, None, None, 1, 1, 8, 0, None) == -1
    assert L.pcv_cbam_excite(None, None, None, None, None, None, None, None, 1, 8, 1, None) == -1
    assert L.pcv_cbam_spatial_pool(None, None, None, None, 1, 1, 8, 0, None) == -1
    assert L.pcv_cbam_apply(None, None, None, None, None, None, None, None, None, 1, 1, 1, 8, 0, 0, None) == -1


def test_engine_refuses_channel_counts_the_kernels_do_not_take():
    """The argument rule (C % 8 == 0) is enforced before any device call: a handle with 12 channels never reaches the library."""
    from pytorchcv_amd import engine
    t = torch.zeros(1, 2, 2, 16)
    a = engine.NHWC(t, 1, 2, 2, 12, cpitch=16)
    with pytest.raises(NotImplementedError, match="multiple of 8"):
        engine.cbam_forward(a, *([torch.zeros(1)] * 7))


def test_default_mode_is_declared_on_every_module(monkeypatch):
    from pytorchcv_amd import engine
    from pytorchcv_amd.model_provider import get_model
    monkeypatch.delenv("PCV_AMD_DTYPE", raising=False)
    net = get_model("cbam_resnet18").eval()
    assert {engine.compute_dtype_of(m) for m in net.modules()} == {engine.compute_dtype_of(net)}
