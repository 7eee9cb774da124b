"""CPU: RegNetX / RegNetY in the registry - the 24 names through `get_model` (any case) and the alias, parameter counts, key counts
and state_dict layout hashes against the reference's (tests/golden/regnet_param_counts.json, written by make_golden_regnet.py from the
imported reference) and their metainfo rows, strict loading of synthetic state dicts, the registry tables of the earlier families left
as they were, and the host predicate pcv_gconvx_supported: 1 for every grouped 3x3 layer of the 24 nets with at most 64 channels per
group that the ResNeXt kernels do not own (the layer list rides in the fixture), 0 with a reason text for what the kernel does not
take."""

import os
import json
import ctypes
import hashlib
import pytest
import util

NAMES = ["regnet{}{}".format(v, s) for v in "xy" for s in ("002", "004", "006", "008", "016", "032", "040", "064", "080", "120", "160", "320")]
FIXTURE_NETS = ["regnetx002", "regnety016"]
# parameters (the reference's own asserts, regnet.py:957-980)
PUBLISHED = dict(
    regnetx002=2684792, regnetx004=5157512, regnetx006=6196040, regnetx008=7259656, regnetx016=9190136, regnetx032=15296552,
    regnetx040=22118248, regnetx064=26209256, regnetx080=39572648, regnetx120=46106056, regnetx160=54278536, regnetx320=107811560,
    regnety002=3162996, regnety004=4344144, regnety006=6055160, regnety008=6263168, regnety016=11202430, regnety032=19436338,
    regnety040=20646656, regnety064=30583252, regnety080=39180068, regnety120=51822544, regnety160=83590140, regnety320=145046770)
WIDTHS = (8, 16, 24, 40, 48, 56, 64)


def _counts():
    with open(os.path.join(util.GOLDEN, "regnet_param_counts.json")) as f:
        return json.load(f)


def blocks_meta():
    with open(os.path.join(util.GOLDEN, "blocks_regnet.json")) as f:
        return json.load(f)


def build_unit(case):
    """The pytorchcv_amd counterpart of a reference unit case of blocks_regnet.json"""
    from pytorchcv_amd.models import regnet
    return getattr(regnet, case["kind"])(**dict(case["kwargs"])).eval()


def test_registry_keeps_its_tables_and_adds_one_beside_them():
    from pytorchcv_amd import model_provider as mp
    assert sorted(mp._regnet_models) == sorted(NAMES) and len(NAMES) == 24
    tables = [v for k, v in vars(mp).items() if k.startswith("_models") and isinstance(v, dict)]
    assert len(tables) == 5 and len(mp._models) == 150 and sum(len(t) for t in tables) == 168
    assert not set(mp._regnet_models) & (set().union(*tables) | set(mp._hrnet_models))
    assert len(mp._hrnet_models) == 9


@pytest.mark.parametrize("name", NAMES)
def test_constructs_counts_and_layout_match_reference(name):
    from pytorchcv_amd.model_provider import get_model
    from pytorchcv_amd.models.common.model_store import calc_net_weight_count, get_model_weight_count
    net = get_model(name.upper())
    ref = _counts()[name]
    assert type(net).__name__ == "RegNet" and tuple(net.in_size) == (224, 224) and net.num_classes == 1000
    assert calc_net_weight_count(net) == ref["param_count"] == PUBLISHED[name] == get_model_weight_count(name)
    sd = net.state_dict()
    assert len(sd) == ref["key_count"]
    text = "\n".join("{} {} {}".format(k, list(v.shape), str(v.dtype).replace("torch.", "")) for k, v in sd.items())
    assert hashlib.sha256(text.encode()).hexdigest() == ref["layout_sha256"]       # make_golden_hrnet.layout_sha256
    net.load_state_dict(util.synth_state_dict(sd, seed=1234), strict=True)


def test_spot_counts_of_the_issue():
    c = _counts()
    assert [(c[n]["param_count"], c[n]["key_count"]) for n in ("regnetx002", "regnety002", "regnety016", "regnetx032", "regnety320")] == \
        [(2684792, 266), (3162996, 318), (11202430, 626), (15296552, 482), (145046770, 472)]


def test_lookup_through_both_import_paths_and_unknown_names():
    from pytorchcv_amd.model_provider import get_model
    from pytorchcv.model_provider import get_model as alias_get_model
    from pytorchcv_amd.models.regnet import RegNet
    assert type(alias_get_model("RegNetY016")) is RegNet
    with pytest.raises(ValueError, match="Unsupported model: regnetx003"):
        get_model("regnetx003")
    assert get_model("regnetx002", num_classes=10).output.out_features == 10


@pytest.mark.parametrize("name", FIXTURE_NETS)
def test_fixture_state_loads_strictly_and_the_tree_is_the_reference_s(name):
    from pytorchcv_amd.model_provider import get_model
    net = get_model(name)
    net.load_state_dict(util.model_state(name, net.state_dict()), strict=True)
    keys = "\n".join(net.state_dict())
    for attr in ("features.init_block.conv.weight", "features.stage1.unit1.body.conv2.conv.weight",
                 "features.stage1.unit1.identity_conv.bn.running_var", "features.stage4.unit1.body.conv3.bn.weight", "output.bias"):
        assert attr in keys, attr
    assert ("features.stage2.unit1.body.se.conv1.bias" in keys) == (name == "regnety016")
    f = net.features
    if name == "regnetx002":
        assert [len(s) for s in (f.stage1, f.stage2, f.stage3, f.stage4)] == [1, 1, 4, 7]
        assert [s.unit1.body.conv2.conv.groups for s in (f.stage1, f.stage2, f.stage3, f.stage4)] == [3, 7, 19, 46]
    else:
        assert [s.unit1.body.conv2.conv.in_channels for s in (f.stage1, f.stage2, f.stage3, f.stage4)] == [48, 120, 336, 888]
        u = f.stage2.unit1.body                                   # SE between conv2 and conv3, a quarter of the unit's input wide
        assert (u.se.conv1.in_channels, u.se.conv1.out_channels) == (120, 48 // 4)


@pytest.mark.parametrize("name", sorted(blocks_meta()))
def test_unit_state_dict_has_the_reference_s_key_count_and_loads_strictly(name):
    m = blocks_meta()[name]
    blk = build_unit(m["case"])
    sd = blk.state_dict()
    assert len(sd) == m["key_count"]
    blk.load_state_dict(util.synth_state_dict(sd, seed=m["weight_seed"]), strict=True)


def test_unit_cases_are_the_listed_ones():
    meta = blocks_meta()
    kw = [m["case"]["kwargs"] for m in meta.values()]
    assert {(k["out_channels"], k["groups"]) for k in kw} == {(24, 8), (56, 8), (120, 24), (80, 40), (168, 56), (128, 64)}
    assert {(k["use_se"], k["stride"]) for k in kw} == {(False, 1), (False, 2), (True, 1), (True, 2)}
    assert any(k["stride"] == 1 and k["in_channels"] != k["out_channels"] for k in kw)          # identity_conv at stride 1
    assert any(k["stride"] == 1 and k["in_channels"] == k["out_channels"] for k in kw)          # no identity_conv
    assert all(m["case"]["x"][0] == 2 and 8 <= m["case"]["x"][2] <= 12 for m in meta.values())
    for name in ("blocks_regnet.npz", "blocks_regnet.json", "regnet_param_counts.json", "calib_regnety016.json", "logits_regnety016.npz"):
        assert os.path.getsize(os.path.join(util.GOLDEN, name)) < (1 << 18), name


# ---- the host predicate ------------------------------------------------------------------------------------------------------------
def _desc(C, cg, H, W, stride, N=4, dtype=1, **kw):
    from pytorchcv_amd._lib import ConvDesc
    d = ConvDesc()
    d.N, d.H, d.W, d.Cin, d.Cout, d.kh, d.kw = N, H, W, C, C, 3, 3
    d.stride_h = d.stride_w = stride
    d.pad_t = d.pad_l = d.pad_b = d.pad_r = 1
    d.dil_h = d.dil_w = 1
    d.groups, d.act, d.post_act, d.has_residual = C // cg, 1, 0, 0
    d.dtype = d.out_dtype = dtype
    d.x_cpitch, d.x_wpitch, d.y_cpitch = C, W, 0
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _pays(cg, stride, W):
    from gconvx_ref import gconvx_pays
    return gconvx_pays(cg, stride, W)


def _old_kernels_own(C, cg):
    return C % 64 == 0 and cg in (4, 8, 16, 32)                   # plan_conv's `gconv`


def test_symbol_is_in_the_binding_and_the_abi_version_stays():
    from pytorchcv_amd import _lib
    assert "pcv_gconvx_supported" in _lib.exported_symbols() and hasattr(_lib.lib(), "pcv_gconvx_supported")
    assert _lib.PCV_ABI_VERSION == 5 == _lib.lib().pcv_abi_version()


@pytest.mark.parametrize("name", NAMES)
def test_every_grouped_layer_up_to_64_per_group_is_taken(name):
    from pytorchcv_amd import _lib
    L = _lib.lib()
    layers = _counts()[name]["grouped"]
    assert layers and sum(n for *_, n in layers) == sum(1 for k in _model_conv2(name))
    for C, cg, H, stride, _ in layers:
        for dtype in (1, 2):
            got = L.pcv_gconvx_supported(ctypes.byref(_desc(C, cg, H, H, stride, dtype=dtype)))
            want = int(cg in WIDTHS and C // cg >= 2 and not _old_kernels_own(C, cg) and _pays(cg, stride, H))
            assert got == want, (name, C, cg, H, stride, (L.pcv_last_error(None) or b"").decode())


def _model_conv2(name):
    from pytorchcv_amd.model_provider import get_model
    return [k for k in get_model(name).state_dict() if k.endswith("body.conv2.conv.weight")]


def test_layer_census_of_the_24_nets():
    """464 grouped layers (one per unit: the depths of the 24 nets add up to 237 + 227); the ResNeXt kernels own 39 of them; the new
    kernel takes every other one of the 16 nets up to 64 per group"""
    counts = _counts()
    total = sum(n for name in NAMES for *_, n in counts[name]["grouped"])
    old = sum(n for name in NAMES for C, cg, H, s, n in counts[name]["grouped"] if _old_kernels_own(C, cg))
    assert (total, old) == (464, 39)
    narrow = [name for name in NAMES if all(cg <= 64 for _, cg, _, _, _ in counts[name]["grouped"])]
    assert len(narrow) == 16 and "regnetx080" not in narrow and "regnety064" not in narrow
    for name in narrow:
        assert all(cg in WIDTHS and C // cg >= 2 for C, cg, _, _, _ in counts[name]["grouped"]), name
    # ... of which the measurement sent these shape classes back to the generic kernel (gconvx_pays, profiles/experiments/gconvx_kernel.md)
    back = sorted({(C, cg, H, s) for name in narrow for C, cg, H, s, _ in counts[name]["grouped"] if not _pays(cg, s, H)})
    assert (192, 48, 56, 2) in back and (432, 48, 28, 2) in back and (168, 56, 112, 2) in back and (168, 56, 56, 1) in back
    assert all(cg >= 40 for _, cg, _, _ in back)


def test_predicate_refuses_with_a_reason_and_without_a_context():
    from pytorchcv_amd import _lib
    L = _lib.lib()
    assert L.pcv_gconvx_supported(ctypes.byref(_desc(56, 8, 56, 56, 2))) == 1
    refused = [
        (_desc(56, 8, 56, 56, 2, dtype=0), "16-bit"),                                # fp32
        (_desc(56, 8, 56, 56, 1, dil_h=2, dil_w=2, pad_t=2, pad_l=2, pad_b=2, pad_r=2), "dilation"),
        (_desc(56, 8, 56, 56, 1, Cout=112), "Cin == Cout"),
        (_desc(56, 8, 57, 57, 2), "odd"),
        (_desc(56, 8, 4, 113, 1), "112"),
        (_desc(56, 4, 14, 14, 1), "channels per group"),                             # Cg = 4
        (_desc(72, 12, 14, 14, 1), "channels per group"),                            # Cg = 12
        (_desc(128, 16, 14, 14, 1), "ResNeXt"),                                      # a shape the old kernels own
        (_desc(56, 8, 14, 14, 1, has_residual=1, post_act=1), "generic kernel"),
        (_desc(56, 8, 14, 14, 1, x_cpitch=64), "generic kernel"),
        (_desc(56, 8, 14, 14, 1, y_cpitch=64), "generic kernel"),
        (_desc(192, 48, 56, 56, 2), "measured slower"),
        (_desc(512, 64, 14, 14, 1), "measured slower"),
    ]
    for d, word in refused:
        assert L.pcv_gconvx_supported(ctypes.byref(d)) == 0, word
        text = (L.pcv_last_error(None) or b"").decode()
        assert text.startswith("pcv_gconvx_supported: ") and word in text, (word, text)
    assert L.pcv_gconvx_supported(None) == 0 and b"NULL" in L.pcv_last_error(None)


def test_default_mode_is_one_type_on_every_module(monkeypatch):
    from pytorchcv_amd import engine
    from pytorchcv_amd.model_provider import get_model
    monkeypatch.delenv("PCV_AMD_DTYPE", raising=False)
    net = get_model("regnety016").eval()
    assert engine.compute_dtype_of(net) in ("bf16", "fp16")
    assert {engine.compute_dtype_of(m) for m in net.modules()} == {engine.compute_dtype_of(net)}
