"""CPU: HRNet in the registry - the nine names through `get_model` and the alias, parameter and key counts against the reference's
(tests/golden/hrnet_param_counts.json, written by make_golden_hrnet.py from the imported reference) and their metainfo rows, state_dict
layout key for key against the fixture manifest (hrnet_w18_small_v1) and, for all nine names, against the frozen hash of the
reference's layout, strict loading of the synthetic state dict, the registry tables of the earlier families left as they were, the two new entry points in the binding, the shapes of every
exchange of the nine nets accepted by pcv_hr_fuse_supported, and engine.hr_fuse's refusal of handles that do not fit together."""

import os
import json
import copy
import ctypes
import pytest
import torch
import util

NAMES = ["hrnet_w18_small_v1", "hrnet_w18_small_v2", "hrnetv2_w18", "hrnetv2_w30", "hrnetv2_w32", "hrnetv2_w40", "hrnetv2_w44",
         "hrnetv2_w48", "hrnetv2_w64"]
FIXTURE_NETS = ["hrnet_w18_small_v1", "hrnetv2_w18"]
# parameters (the reference's own asserts, hrnet.py:709-717)
PUBLISHED = dict(hrnet_w18_small_v1=13187464, hrnet_w18_small_v2=15597464, hrnetv2_w18=21299004, hrnetv2_w30=37712220,
                 hrnetv2_w32=41232680, hrnetv2_w40=57557160, hrnetv2_w44=67064984, hrnetv2_w48=77469864, hrnetv2_w64=128059944)
SYMBOLS = ("pcv_hr_fuse_supported", "pcv_hr_fuse")


def _counts():
    with open(os.path.join(util.GOLDEN, "hrnet_param_counts.json")) as f:
        return json.load(f)


def blocks_meta():
    with open(os.path.join(util.GOLDEN, "blocks_hrnet.json")) as f:
        return json.load(f)


def build_hr_block(case):
    """The pytorchcv_amd counterpart of a reference block case of blocks_hrnet.json (the constructors write into their channel
    lists: the kwargs are copied)."""
    from pytorchcv_amd.models import hrnet
    return getattr(hrnet, case["kind"])(**copy.deepcopy(case["kwargs"])).eval()


def case_input(case, seed):
    """One tensor ("x") or a list of tensors ("xs", map i from seed + i), as make_golden_hrnet.py generates them."""
    if "x" in case:
        return util.synth_input(*case["x"], seed=seed)
    return [util.synth_input(*shape, seed=seed + i) for i, shape in enumerate(case["xs"])]


def test_registry_keeps_its_five_tables_and_adds_one_beside_them():
    from pytorchcv_amd import model_provider as mp
    assert sorted(mp._hrnet_models) == sorted(NAMES)
    tables = [v for k, v in vars(mp).items() if k.startswith("_models") and isinstance(v, dict)]
    assert len(tables) == 5 and len(mp._models) == 150 and sum(len(t) for t in tables) == 168
    for name in NAMES:
        assert all(name not in t for t in tables)
    assert not set(mp._hrnet_models) & set().union(*tables)


@pytest.mark.parametrize("name", NAMES)
def test_constructs_and_counts_match_reference(name):
    from pytorchcv_amd.model_provider import get_model
    from pytorchcv_amd.models.common.model_store import calc_net_weight_count, get_model_weight_count, get_model_metainfo_dict
    net = get_model(name)
    ref = _counts()[name]
    assert type(net).__name__ == "HRNet" and tuple(net.in_size) == (224, 224) and net.num_classes == 1000
    assert calc_net_weight_count(net) == ref["param_count"] == PUBLISHED[name]
    assert len(net.state_dict()) == ref["key_count"]
    assert get_model_weight_count(name) == PUBLISHED[name]
    assert get_model_metainfo_dict()[name][0] == PUBLISHED[name]


def test_lookup_is_case_insensitive_through_both_import_paths():
    from pytorchcv_amd.model_provider import get_model
    from pytorchcv.model_provider import get_model as alias_get_model
    from pytorchcv.models.hrnet import HRNet as AliasHRNet
    from pytorchcv_amd.models.hrnet import HRNet
    assert AliasHRNet is HRNet
    assert type(get_model("HRNet_W18_Small_V1")) is HRNet and type(alias_get_model("HRNETV2_W18")) is HRNet
    with pytest.raises(ValueError, match="Unsupported model: hrnetv2_w20"):
        get_model("hrnetv2_w20")
    assert get_model("hrnet_w18_small_v1", num_classes=10).output.out_features == 10


def _layout_sha256(net):
    """make_golden_hrnet.layout_sha256: sha256 over the lines "<key> <shape> <dtype>" of the state_dict, in its order"""
    import hashlib
    text = "\n".join("{} {} {}".format(k, list(v.shape), str(v.dtype).replace("torch.", "")) for k, v in net.state_dict().items())
    return hashlib.sha256(text.encode()).hexdigest()


@pytest.mark.parametrize("name", NAMES)
def test_state_dict_layout_is_the_reference_s_key_for_key(name):
    """every key, shape and dtype in order, against the hash frozen from the imported reference"""
    from pytorchcv_amd.model_provider import get_model
    assert _layout_sha256(get_model(name)) == _counts()[name]["layout_sha256"]


@pytest.mark.parametrize("name", FIXTURE_NETS)
def test_fixture_state_loads_strictly(name):
    from pytorchcv_amd.model_provider import get_model
    net = get_model(name)
    net.load_state_dict(util.model_state(name, net.state_dict()), strict=True)


@pytest.mark.parametrize("name", FIXTURE_NETS[:1])
def test_state_dict_matches_reference_manifest_and_loads_strictly(name):
    from pytorchcv_amd.model_provider import get_model
    net = get_model(name)
    man = util.model_manifest(name)
    sd = net.state_dict()
    assert list(sd.keys()) == list(man["keys"].keys())
    for k, v in sd.items():
        shape, dt = man["keys"][k]
        assert list(v.shape) == shape and str(v.dtype).replace("torch.", "") == dt, k
    assert man["param_count"] == PUBLISHED[name]
    net.load_state_dict(util.model_state(name, sd), strict=True)
    keys = "\n".join(sd)
    for attr in ("features.init_block.conv1.conv.weight", "features.init_block.subblocks.block1.identity_conv.bn.weight",
                 "features.stage1.transition.block1.conv.weight", "features.stage1.transition.block2.subblock1.bn.running_var",
                 "features.stage1.layers.block1.branches.branch2.unit2.body.conv2.conv.weight",
                 "features.stage3.layers.block1.fuse_layers.layer1.block4.conv.bn.weight",
                 "features.stage3.layers.block1.fuse_layers.layer4.block1.subblock3.conv.weight",
                 "features.final_block.inc_blocks.block4.body.conv3.conv.weight", "features.final_block.down_blocks.block3.conv.bias",
                 "features.final_block.final_layer.conv.bias", "output.weight", "output.bias"):
        assert attr in keys, attr
    assert "fuse_layers.layer1.block1" not in keys and "stage2.transition.block1" not in keys        # identities hold nothing


@pytest.mark.parametrize("name", [n for n in NAMES if n not in FIXTURE_NETS])
def test_synthetic_state_dict_loads_strictly(name):
    from pytorchcv_amd.model_provider import get_model
    net = get_model(name)
    sd = net.state_dict()
    net.load_state_dict(util.synth_state_dict(sd, seed=1234), strict=True)
    assert len(sd) == _counts()[name]["key_count"]


def test_transition_widths_follow_the_reference_aliasing():
    """stage 1 narrows the init block's 256 channels; later stages keep the widths and open one branch from the last map"""
    from pytorchcv_amd.model_provider import get_model
    from pytorchcv_amd.models.hrnet import Identity
    f = get_model("hrnetv2_w18").features
    t1, t2, t3 = f.stage1.transition, f.stage2.transition, f.stage3.transition
    assert (t1.block1.conv.in_channels, t1.block1.conv.out_channels, tuple(t1.block1.conv.stride)) == (256, 18, (1, 1))
    assert (t1.block2.subblock1.conv.in_channels, t1.block2.subblock1.conv.out_channels, tuple(t1.block2.subblock1.conv.stride)) == (256, 36, (2, 2))
    assert isinstance(t2.block1, Identity) and isinstance(t2.block2, Identity)
    assert (t2.block3.subblock1.conv.in_channels, t2.block3.subblock1.conv.out_channels) == (36, 72)
    assert all(isinstance(b, Identity) for b in (t3.block1, t3.block2, t3.block3))
    assert (t3.block4.subblock1.conv.in_channels, t3.block4.subblock1.conv.out_channels) == (72, 144)
    assert [b.body.conv1.conv.in_channels for b in f.final_block.inc_blocks] == [18, 36, 72, 144]
    assert (len(f.stage1.layers), len(f.stage2.layers), len(f.stage3.layers)) == (1, 4, 3)
    up = f.stage3.layers.block1.fuse_layers.layer1.block4
    assert (up.conv.conv.in_channels, up.conv.conv.out_channels, up.shift, up.conv.activate) == (144, 18, 3, False)


@pytest.mark.parametrize("name", sorted(blocks_meta()))
def test_block_state_dict_has_the_reference_s_key_count_and_loads_strictly(name):
    """(the key NAMES are checked by the golden outputs: synthetic weights are generated from them)"""
    m = blocks_meta()[name]
    blk = build_hr_block(m["case"])
    sd = blk.state_dict()
    assert len(sd) == m["key_count"]
    blk.load_state_dict(util.synth_state_dict(sd, seed=m["weight_seed"]), strict=True)


def test_block_cases_are_the_listed_ones():
    meta = blocks_meta()
    kinds = sorted((m["case"]["kind"], n) for n, m in meta.items())
    assert [k for k, _ in kinds] == ["HRBlock", "HRBlock", "HRFinalBlock", "HRInitBlock", "HRStage", "HRStage", "UpSamplingBlock",
                                     "UpSamplingBlock"]
    assert sorted(m["case"]["kwargs"]["scale_factor"] for m in meta.values() if m["case"]["kind"] == "UpSamplingBlock") == [2, 8]
    assert meta["block2_16_32"]["case"]["xs"] == [[2, 16, 8, 12], [2, 32, 4, 6]]
    assert meta["block4_18_144"]["case"]["xs"] == [[2, 18, 16, 16], [2, 36, 8, 8], [2, 72, 4, 4], [2, 144, 2, 2]]
    assert len(meta["stage_new_branch"]["y_shapes"]) == len(meta["stage_new_branch"]["case"]["xs"]) + 1
    assert meta["stage_from_init_256_18"]["case"]["kwargs"]["in_channels_list"] == [256]
    assert meta["final_16_128"]["case"]["xs"][0][2:] == [8, 8] and meta["final_16_128"]["case"]["xs"][-1][2:] == [1, 1]
    for name in ("blocks_hrnet.npz", "blocks_hrnet.json", "manifest_hrnet_w18_small_v1.json", "calib_hrnetv2_w18.json"):
        assert os.path.getsize(os.path.join(util.GOLDEN, name)) < (1 << 17), name


def test_hr_fuse_symbols_are_in_the_binding_and_the_abi_version_stays():
    from pytorchcv_amd import _lib
    for s in SYMBOLS:
        assert s in _lib.exported_symbols()
        assert hasattr(_lib.lib(), s)
    assert _lib.PCV_ABI_VERSION == 5 == _lib.lib().pcv_abi_version()


@pytest.mark.parametrize("name", NAMES)
def test_every_exchange_of_the_nets_is_accepted(name):
    """the shapes of all exchanges of a net at 224x224 (branch i: width_i channels on a 56 >> i map; sources j < = i at shift 0,
    j > i at shift j - i), in every storage type"""
    from pytorchcv_amd import _lib
    from pytorchcv_amd.model_provider import get_model
    from pytorchcv_amd.models.hrnet import HRBlock
    L = _lib.lib()
    blocks = [m for m in get_model(name).modules() if isinstance(m, HRBlock)]
    launches = 0
    for blk in blocks:
        B = blk.num_branches
        for i in range(B):
            shifts = [max(0, j - i) for j in range(B)]
            C = (blk.in_channels_list[i] + 7) // 8 * 8
            sh = (ctypes.c_int * B)(*shifts)
            for dtype in (0, 1, 2):
                assert L.pcv_hr_fuse_supported(B, sh, 4, 56 >> i, 56 >> i, C, 1, dtype) == 1, (name, i, L.pcv_last_error(None))
            launches += 1
    if name == "hrnetv2_w18":
        assert launches == 26                                  # 1 x 2 + 4 x 3 + 3 x 4


def test_supported_refuses_with_a_text_and_without_a_context():
    from pytorchcv_amd import _lib
    L = _lib.lib()
    ok = (ctypes.c_int * 2)(0, 1)
    assert L.pcv_hr_fuse_supported(2, ok, 2, 4, 6, 16, 1, 1) == 1
    for args, word in (((0, ok, 2, 4, 6, 16, 1, 1), "sources"), ((2, None, 2, 4, 6, 16, 1, 1), "NULL"),
                       ((2, ok, 2, 5, 6, 16, 1, 1), "divide"), ((2, ok, 2, 4, 6, 12, 1, 1), "multiple of 8"),
                       ((2, ok, 2, 4, 6, 16, 3, 1), "activation"), ((2, ok, 2, 4, 6, 16, 1, 7), "dtype"),
                       ((2, (ctypes.c_int * 2)(0, 4), 2, 16, 16, 16, 1, 1), "shift"),
                       ((2, ok, 1 << 12, 1 << 10, 1 << 10, 16, 1, 1), "2 GiB")):
        assert L.pcv_hr_fuse_supported(*args) == 0, args
        text = (L.pcv_last_error(None) or b"").decode()
        assert text.startswith("pcv_hr_fuse_supported: ") and word in text, (args, text)


def test_engine_hr_fuse_refuses_handles_that_do_not_fit():
    """checked on the host before anything is allocated or launched: CPU tensors are enough"""
    from pytorchcv_amd import engine

    def h(N, H, W, C, dtype=torch.bfloat16, cpitch=None):
        cp = engine.round8(C) if cpitch is None else cpitch
        return engine.NHWC(torch.zeros((N, H, W, cp), dtype=dtype), N, H, W, C, cpitch=cp)

    fine = h(2, 8, 8, 18)
    for sources, shifts in (([fine, h(2, 4, 4, 18)], [0, 2]),                     # 4 << 2 != 8
                            ([fine, h(2, 4, 4, 18)], [0]),                        # one shift for two sources
                            ([fine, h(2, 4, 4, 36)], [0, 1]),                     # another width
                            ([fine, h(1, 4, 4, 18)], [0, 1]),                     # another batch
                            ([fine, h(2, 4, 4, 18, dtype=torch.float16)], [0, 1]),
                            ([fine, h(2, 4, 4, 18, cpitch=32)], [0, 1]),          # not the dense pitch
                            ([fine, h(2, 8, 4, 18)], [0, 1]),
                            ([fine, torch.zeros(2, 4, 4, 24)], [0, 1]),           # not a handle
                            ([], []),
                            ([fine, h(2, 4, 4, 18)], [0, -1])):
        with pytest.raises(RuntimeError, match="hr_fuse"):
            engine.hr_fuse(sources, shifts, 1)


def test_default_mode_is_one_type_on_every_module(monkeypatch):
    from pytorchcv_amd import engine
    from pytorchcv_amd.model_provider import get_model
    monkeypatch.delenv("PCV_AMD_DTYPE", raising=False)
    net = get_model("hrnet_w18_small_v1").eval()
    assert engine.compute_dtype_of(net) in ("bf16", "fp16")
    assert {engine.compute_dtype_of(m) for m in net.modules()} == {engine.compute_dtype_of(net)}


def test_composed_path_switch_exists():
    from pytorchcv_amd.models import hrnet
    assert hrnet.FUSED is True
