"""CPU: IBN-Net in the registry - the nine names through `get_model` and the alias, parameter and key counts against the
reference's (tests/golden/ibn_param_counts.json, written by make_golden_ibn.py from the imported reference) and its metainfo rows,
state_dict layouts key for key against the fixture manifests (nets and block cases), what `IBN` refuses at construction, and the
kwargs contract of the factories."""

import os
import json
import pytest
import torch.nn as nn
import util

NAMES = ["ibn_resnet50", "ibn_resnet101", "ibn_resnet152", "ibnb_resnet50", "ibnb_resnet101", "ibnb_resnet152",
         "ibn_resnext50_32x4d", "ibn_resnext101_32x4d", "ibn_resnext101_64x4d"]
FIXTURE_NETS = ["ibn_resnet50", "ibnb_resnet50", "ibn_resnext50_32x4d"]
# the reference's own asserts (ibnresnet.py:427-429 and the same place of ibnbresnet.py / ibnresnext.py)
PUBLISHED = {"ibn_resnet50": 25557032, "ibn_resnet101": 44549160, "ibn_resnet152": 60192808,
             "ibnb_resnet50": 25558568, "ibnb_resnet101": 44550696, "ibnb_resnet152": 60194344,
             "ibn_resnext50_32x4d": 25028904, "ibn_resnext101_32x4d": 44177704, "ibn_resnext101_64x4d": 83455272}
CLASS_OF = {"ibn_resnet": "IBNResNet", "ibnb_resnet": "IBNbResNet", "ibn_resnext": "IBNResNeXt"}
SYMBOLS = ("pcv_instnorm_workspace_bytes", "pcv_instnorm_act")


def class_of(name):
    return [c for p, c in CLASS_OF.items() if name.startswith(p)][0]


def _counts():
    with open(os.path.join(util.GOLDEN, "ibn_param_counts.json")) as f:
        return json.load(f)


def blocks_meta():
    with open(os.path.join(util.GOLDEN, "blocks_ibn.json")) as f:
        return json.load(f)


def build_ibn_block(case):
    """The pytorchcv_amd counterpart of a reference block case of blocks_ibn.json."""
    modname = "common.norm" if case["module"] == "norm" else case["module"]
    mod = __import__("pytorchcv_amd.models." + modname, fromlist=[case["kind"]])
    return getattr(mod, case["kind"])(**case["kwargs"]).eval()


def test_registry_keeps_its_tables_and_adds_a_fourth():
    from pytorchcv_amd.model_provider import _models, _models_cbam, _models_mixnet, _models_ibn
    assert len(_models) == 150
    assert sorted(_models_ibn) == sorted(NAMES)
    for other in (_models, _models_cbam, _models_mixnet):
        assert not set(other) & set(_models_ibn)


@pytest.mark.parametrize("name", NAMES)
def test_constructs_and_counts_match_reference(name):
    from pytorchcv_amd.model_provider import get_model
    from pytorchcv_amd.models.common.model_store import calc_net_weight_count, get_model_weight_count
    net = get_model(name)
    ref = _counts()[name]
    assert type(net).__name__ == class_of(name) and tuple(net.in_size) == (224, 224) and net.num_classes == 1000
    assert calc_net_weight_count(net) == ref["param_count"] == PUBLISHED[name]
    assert len(net.state_dict()) == ref["key_count"]
    assert get_model_weight_count(name) == ref["param_count"]                  # the metainfo row (model_metainfos.csv)


def test_lookup_is_case_insensitive_and_the_alias_resolves_every_name():
    from pytorchcv_amd.model_provider import get_model
    from pytorchcv.model_provider import get_model as alias_get_model
    from pytorchcv_amd.model_provider import _models_ibn
    for name in NAMES:
        assert name in _models_ibn
    for name in ("ibn_resnet50", "ibnb_resnet101", "ibn_resnext50_32x4d"):
        assert type(alias_get_model(name.upper())).__name__ == class_of(name)
    assert type(get_model("IBN_ResNet50")).__name__ == "IBNResNet"
    with pytest.raises(ValueError, match="Unsupported model: ibn_resnet18"):
        get_model("ibn_resnet18")


def test_metainfo_rows_are_the_references():
    from pytorchcv_amd.models.common.model_store import get_model_metainfo_dict
    table = get_model_metainfo_dict()
    assert table["ibn_resnet50"] == (25557032, "0576", "40c420fcbbfd87bf634fc5b351746e124c32e401", "v0.0.495")
    assert table["ibnb_resnet50"] == (25558568, "0597", "383b44324af7bb3842b93df177bdd199864e0e8d", "v0.0.552")
    assert table["ibn_resnext101_32x4d"] == (44177704, "0512", "73534cc42c9f7b1aa859b32e012c31f9ea66fd60", "v0.0.553")
    for name in NAMES:
        assert table[name][0] == PUBLISHED[name]


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
    want = {"ibn_resnet50": ("stage1.unit1.body.conv1.ibn.inst_norm.weight", "stage3.unit6.body.conv1.ibn.batch_norm.running_var",
                             "stage3.unit1.body.conv1.ibn.batch_norm.num_batches_tracked", "stage4.unit1.body.conv1.bn.weight"),
            "ibnb_resnet50": ("features.init_block.conv.inst_norm.weight", "features.init_block.conv.inst_norm.bias",
                              "stage1.unit3.inst_norm.weight", "stage2.unit4.inst_norm.bias"),
            "ibn_resnext50_32x4d": ("stage2.unit1.body.conv1.ibn.inst_norm.bias", "stage4.unit3.body.conv1.bn.running_mean")}[name]
    for attr in want:
        assert attr in keys, attr
    if name == "ibnb_resnet50":
        assert "stage3.unit6.inst_norm" not in keys and "stage1.unit1.inst_norm" not in keys and "init_block.conv.bn" not in keys
    else:
        assert "stage4.unit1.body.conv1.ibn" not in keys


@pytest.mark.parametrize("name", sorted(blocks_meta()))
def test_block_state_dict_matches_reference_manifest(name):
    m = blocks_meta()[name]
    blk = build_ibn_block(m["case"])
    sd = blk.state_dict()
    assert {k: [list(v.shape), str(v.dtype).replace("torch.", "")] for k, v in sd.items()} == m["manifest"]
    blk.load_state_dict(util.synth_state_dict(util.template_from_manifest(m["manifest"]), seed=m["weight_seed"]), strict=True)


def test_block_cases_are_the_listed_ones():
    cases = {n: (m["case"]["kind"], tuple(m["case"]["x"])) for n, m in blocks_meta().items()}
    assert sorted(cases.values()) == sorted([
        ("IBN", (3, 64, 7, 9)), ("ibn_conv1x1_block", (2, 64, 9, 9)), ("IBNResUnit", (2, 64, 8, 8)), ("IBNResUnit", (2, 256, 10, 10)),
        ("IBNResUnit", (2, 1024, 6, 6)), ("IBNResNeXtUnit", (2, 256, 8, 8)), ("IBNbResUnit", (2, 256, 7, 7)),
        ("IBNbResUnit", (2, 256, 8, 8)), ("IBNbResInitBlock", (2, 3, 32, 30))])


def test_ibn_sections_and_refusals():
    from pytorchcv_amd.models.common.norm import IBN
    m = IBN(channels=64)
    assert m.split_sections == [32, 32] and m.inst_first is True
    assert isinstance(m.inst_norm, nn.InstanceNorm2d) and m.inst_norm.affine and not m.inst_norm.track_running_stats
    assert m.inst_norm.eps == 1e-5 and isinstance(m.batch_norm, nn.BatchNorm2d) and m.batch_norm.num_features == 32
    assert IBN(channels=128, first_fraction=0.25).split_sections == [32, 96]
    with pytest.raises(NotImplementedError, match="inst_first"):
        IBN(channels=64, inst_first=False)
    with pytest.raises(NotImplementedError, match="multiples of 8"):
        IBN(channels=24)
    with pytest.raises(NotImplementedError, match="multiples of 8"):
        IBN(channels=64, first_fraction=0.3)


def test_units_without_ibn_are_the_existing_units():
    """Stage 4 and the plain units of the b-variant keep today's fused routes: they ARE ResUnit / ResNeXtUnit, in ResStage."""
    from pytorchcv_amd.model_provider import get_model
    from pytorchcv_amd.models.resnet import ResUnit, ResStage, ResBottleneck
    from pytorchcv_amd.models.resnext import ResNeXtUnit
    from pytorchcv_amd.models.ibnresnet import IBNResUnit
    from pytorchcv_amd.models.ibnbresnet import IBNbResUnit
    a = get_model("ibn_resnet50").features
    assert all(type(u) is IBNResUnit for s in (a.stage1, a.stage2, a.stage3) for u in s.children())
    assert all(type(u) is ResUnit and tuple(u.body.conv2.conv.stride) == ((2, 2) if i == 0 else (1, 1))
               for i, u in enumerate(a.stage4.children()))
    assert not any(getattr(u, "pcv_chainable", False) or isinstance(u, ResUnit) for u in a.stage1.children())
    x = get_model("ibn_resnext50_32x4d").features
    assert all(type(u) is ResNeXtUnit for u in x.stage4.children()) and isinstance(x.stage4, ResStage)
    assert [u.body.conv1.conv.out_channels for u in (x.stage1.unit1, x.stage2.unit1, x.stage3.unit1)] == [128, 256, 512]
    y = get_model("ibn_resnext101_64x4d").features
    assert [u.body.conv1.conv.out_channels for u in (y.stage1.unit1, y.stage2.unit1, y.stage3.unit1)] == [256, 512, 1024]
    b = get_model("ibnb_resnet50").features
    flags = [[u.use_inst_norm for u in s.children()] for s in (b.stage1, b.stage2, b.stage3, b.stage4)]
    assert flags == [[False, False, True], [False, False, False, True], [False] * 6, [False] * 3]
    assert all(isinstance(u, IBNbResUnit) and isinstance(u.body, ResBottleneck) for s in (b.stage1, b.stage4) for u in s.children())


def test_kwargs_contract():
    """`in_channels`, `in_size`, `num_classes` reach the net; an unknown kwarg is a TypeError from the constructor, as in the
    reference (its factories forward **kwargs to the net class); other depths are refused by name."""
    from pytorchcv_amd.model_provider import get_model
    from pytorchcv_amd.models.ibnresnet import get_ibnresnet
    from pytorchcv_amd.models.ibnbresnet import get_ibnbresnet
    from pytorchcv_amd.models.ibnresnext import get_ibnresnext
    net = get_model("ibnb_resnet50", in_channels=1, in_size=(192, 192), num_classes=10)
    assert net.features.init_block.conv.conv.in_channels == 1 and net.in_size == (192, 192) and net.output.out_features == 10
    assert get_model("ibn_resnet50", num_classes=7, pretrained=False, root="unused").output.out_features == 7
    for name in ("ibn_resnet50", "ibnb_resnet50", "ibn_resnext50_32x4d"):
        with pytest.raises(TypeError):
            get_model(name, no_such_option=1)
    with pytest.raises(ValueError, match="Unsupported IBN-ResNet with number of blocks: 18"):
        get_ibnresnet(blocks=18)
    with pytest.raises(ValueError, match=r"Unsupported IBN\(b\)-ResNet with number of blocks: 34"):
        get_ibnbresnet(blocks=34)
    with pytest.raises(ValueError, match="Unsupported IBN-ResNeXt with number of blocks: 152"):
        get_ibnresnext(blocks=152, cardinality=32, bottleneck_width=4)


def test_instnorm_symbols_are_in_the_binding_and_the_abi_version_stays():
    from pytorchcv_amd import _lib
    for s in SYMBOLS:
        assert s in _lib.exported_symbols()
        assert hasattr(_lib.lib(), s)
    assert _lib.PCV_ABI_VERSION == 5 == _lib.lib().pcv_abi_version()


def test_synthetic_gamma_rule_is_the_batchnorm_one_on_its_own_stream():
    import numpy as np
    import torch
    from pytorchcv_amd.synth import synth_state_dict, hash_uniform, name_stream
    sd = synth_state_dict({"a.inst_norm.weight": torch.zeros(16), "a.inst_norm.bias": torch.zeros(16)}, seed=5)
    w = sd["a.inst_norm.weight"].numpy()
    assert w.min() >= 0.5 and w.max() <= 1.5
    assert np.array_equal(w, (0.5 + hash_uniform(5, name_stream("a.inst_norm.weight"), 16)).astype(np.float32))
    assert float(sd["a.inst_norm.bias"].abs().max()) <= 0.1


def test_default_mode_is_declared_on_every_module(monkeypatch):
    from pytorchcv_amd import engine
    from pytorchcv_amd.model_provider import get_model
    monkeypatch.delenv("PCV_AMD_DTYPE", raising=False)
    for name in FIXTURE_NETS:
        net = get_model(name).eval()
        assert {engine.compute_dtype_of(m) for m in net.modules()} == {engine.compute_dtype_of(net)}
