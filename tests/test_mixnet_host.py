"""CPU: MixNet in the registry - construction through `get_model` and the alias, parameter and key counts against the reference's
(tests/golden/mixnet_param_counts.json, written by make_golden_mixnet.py from the imported reference) and its metainfo rows,
state_dict layouts key for key against the fixture manifests (nets and block cases), the three MixConv entry points of the ABI
refusing what they do not support before any device is touched, and the grouped-convolution form of the 1x1 MixConv against the
reference's block outputs."""

import os
import json
import ctypes
import numpy as np
import pytest
import torch
import torch.nn.functional as F
import util

NAMES = ["mixnet_s", "mixnet_m", "mixnet_l"]
PUBLISHED = {"mixnet_s": (4134606, 396), "mixnet_m": (5014382, 479), "mixnet_l": (7329252, 479)}      # parameters, state_dict keys
SYMBOLS = ("pcv_mixconv_packed_bytes", "pcv_mixconv_pack", "pcv_mixconv2d_fused")


def _counts():
    with open(os.path.join(util.GOLDEN, "mixnet_param_counts.json")) as f:
        return json.load(f)


def blocks_meta():
    with open(os.path.join(util.GOLDEN, "blocks_mixnet.json")) as f:
        return json.load(f)


def build_mix_block(case):
    """The pytorchcv_amd counterpart of a reference block case of blocks_mixnet.json (`activation` is stored as a name)."""
    from pytorchcv_amd.models import mixnet
    from pytorchcv_amd.models.common.activ import lambda_relu, lambda_swish
    kw = dict(case["kwargs"])
    name = kw["activation"]
    kw["activation"] = None if name is None else {"relu": lambda_relu, "swish": lambda_swish}[name]()
    return getattr(mixnet, case["kind"])(**kw).eval()


def test_registry_keeps_its_tables_and_adds_a_third():
    from pytorchcv_amd.model_provider import _models, _models_cbam, _models_mixnet
    assert len(_models) == 150
    assert sorted(_models_mixnet) == sorted(NAMES)
    assert not set(_models) & set(_models_mixnet) and not set(_models_cbam) & set(_models_mixnet)


@pytest.mark.parametrize("name", NAMES)
def test_constructs_and_counts_match_reference(name):
    from pytorchcv_amd.model_provider import get_model
    from pytorchcv_amd.models.mixnet import MixNet
    from pytorchcv_amd.models.common.model_store import calc_net_weight_count, get_model_weight_count
    net = get_model(name)
    ref = _counts()[name]
    assert isinstance(net, MixNet) and tuple(net.in_size) == (224, 224) and net.num_classes == 1000
    assert calc_net_weight_count(net) == ref["param_count"] == PUBLISHED[name][0]
    assert len(net.state_dict()) == ref["key_count"] == PUBLISHED[name][1]
    assert get_model_weight_count(name) == ref["param_count"]                  # the metainfo row (model_metainfos.csv)


def test_lookup_is_case_insensitive_and_the_alias_resolves_every_name():
    from pytorchcv_amd.model_provider import get_model
    from pytorchcv.model_provider import get_model as alias_get_model
    for name in NAMES:
        assert type(alias_get_model(name.upper())).__name__ == "MixNet"
    assert type(get_model("MixNet_S")).__name__ == "MixNet"
    with pytest.raises(ValueError, match="Unsupported model: mixnet_x"):
        get_model("mixnet_x")


def test_metainfo_rows_are_the_references():
    from pytorchcv_amd.models.common.model_store import get_model_metainfo_dict
    from pytorchcv_amd.models.mixnet import get_mixnet
    table = get_model_metainfo_dict()
    assert table["mixnet_s"] == (4134606, "0717", "ab2c4e37062e7ea34a2cdd112f9354d4e67a0fef", "v0.0.493")
    assert table["mixnet_m"] == (5014382, "0647", "4d90d345a38ba5041ac5cae2921e07d1eca083b2", "v0.0.493")
    assert table["mixnet_l"] == (7329252, "0571", "c686ba17fc6bca5f30ac596b37a7f95f2d4b6f30", "v0.0.500")
    with pytest.raises(ValueError, match="Unsupported MixNet version x"):
        get_mixnet(version="x", width_scale=1.0)


@pytest.mark.parametrize("name", NAMES)
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
    for attr in ("conv1.conv.0.weight", "conv1.conv.1.weight", "exp_conv.conv.0.weight", "conv2.conv.1.weight", "se.conv1.bias",
                 "init_block.conv2.conv1.conv.weight", "final_block.bn.running_var", "output.weight"):
        assert attr in keys, attr


@pytest.mark.parametrize("name", sorted(blocks_meta()))
def test_block_state_dict_matches_reference_manifest(name):
    m = blocks_meta()[name]
    blk = build_mix_block(m["case"])
    sd = blk.state_dict()
    assert {k: [list(v.shape), str(v.dtype).replace("torch.", "")] for k, v in sd.items()} == m["manifest"]
    blk.load_state_dict(util.synth_state_dict(util.template_from_manifest(m["manifest"]), seed=m["weight_seed"]), strict=True)


def test_mixconv_symbols_are_in_the_binding_and_the_abi_version_stays():
    from pytorchcv_amd import _lib
    for s in SYMBOLS:
        assert s in _lib.exported_symbols()
        assert hasattr(_lib.lib(), s)
    assert _lib.PCV_ABI_VERSION == 5 == _lib.lib().pcv_abi_version()


def _desc(C=360, G=4, **over):
    from pytorchcv_amd._lib import ConvDesc
    k = 3 + 2 * (G - 1)
    f = dict(N=2, H=9, W=11, Cin=C, Cout=C, kh=k, kw=k, stride_h=1, stride_w=1, pad_t=k // 2, pad_l=k // 2, pad_b=k // 2, pad_r=k // 2,
             dil_h=1, dil_w=1, groups=C, act=4, post_act=0, has_residual=0, dtype=2, out_dtype=2, x_cpitch=C, x_wpitch=11)
    f.update(over)
    return ConvDesc(**f)


def _kernels(G):
    return (ctypes.c_int * G)(*[3 + 2 * g for g in range(G)])


def test_mixconv_entry_points_refuse_a_null_context():
    from pytorchcv_amd import _lib
    L = _lib.lib()
    d = _desc()
    assert L.pcv_mixconv_pack(None, ctypes.byref(d), _kernels(4), 4, None, None, None) == -1
    assert L.pcv_mixconv2d_fused(None, ctypes.byref(d), _kernels(4), 4, None, None, None, None, None, None) == -1
    assert L.pcv_mixconv_packed_bytes(None, _kernels(4), 4, None) == -1


def test_mixconv_accepts_the_nets_layers_and_sizes_the_blob():
    """The blob holds every channel's own k x k taps at least once, and at most the zero-embedded share of one 4-channel chunk per
    boundary more (the layout of DESIGN.md)."""
    from pytorchcv_amd import _lib
    L = _lib.lib()
    for C, G in ((240, 2), (480, 2), (144, 3), (240, 3), (480, 3), (360, 4), (1200, 4), (720, 5), (192, 4), (504, 3), (1584, 4)):
        for dt, es in ((0, 4), (1, 2), (2, 2)):
            n = ctypes.c_size_t(0)
            d = _desc(C, G, dtype=dt, out_dtype=dt)
            assert L.pcv_mixconv_packed_bytes(ctypes.byref(d), _kernels(G), G, ctypes.byref(n)) == 0, (C, G)
            own = sum((3 + 2 * g) ** 2 * (C // G) for g in range(G)) * es
            assert own <= n.value <= own + (4 * (5 * 5 - 3 * 3) + 4 * (7 * 7 - 5 * 5)) * es + 16 * G, (C, G, n.value, own)


def test_every_depthwise_mixconv_of_the_nets_is_accepted():
    from pytorchcv_amd import _lib
    from pytorchcv_amd.model_provider import get_model
    from pytorchcv_amd.models.mixnet import MixConv
    L = _lib.lib()
    seen = set()
    for name in NAMES:
        for m in get_model(name).modules():
            if isinstance(m, MixConv) and m.depthwise:
                widths = [c.out_channels for c in m.convs()]
                assert len(set(widths)) == 1 and widths[0] % 2 == 0              # equal, even group widths in this family
                seen.add((sum(widths), len(widths), m.convs()[0].stride[0]))
    assert (360, 4, 1) in seen and (720, 5, 2) in seen and len(seen) >= 12
    for C, G, s in sorted(seen):
        n = ctypes.c_size_t(0)
        d = _desc(C, G, stride_h=s, stride_w=s)
        assert L.pcv_mixconv_packed_bytes(ctypes.byref(d), _kernels(G), G, ctypes.byref(n)) == 0, (C, G, s)


@pytest.mark.parametrize("what,over,G,match", [
    ("stale descriptor size", dict(struct_size=96), 4, "struct_size"),
    ("groups != Cin", dict(groups=4), 4, "groups == Cin == Cout"),
    ("Cout != Cin", dict(Cout=368), 4, "groups == Cin == Cout"),
    ("odd group width", dict(Cin=40, Cout=40, groups=40, x_cpitch=40, kh=7, kw=7, pad_t=3, pad_l=3, pad_b=3, pad_r=3), 3, "odd group width"),
    ("residual", dict(has_residual=1), 4, "no residual"),
    ("post activation", dict(post_act=1), 4, "no residual"),
    ("dilation", dict(dil_h=2, dil_w=2), 4, "dilation"),
    ("padded channel pitch", dict(x_cpitch=368), 4, "channel pitch"),
    ("padded row pitch", dict(x_wpitch=12), 4, "row pitch"),
    ("sliced output", dict(y_cpitch=720), 4, "dense"),
    ("TF-same style padding", dict(pad_t=3, pad_l=3), 4, "padding"),
    ("stride 3", dict(stride_h=3, stride_w=3), 4, "stride"),
    ("kh of another window", dict(kh=7, kw=7), 4, "largest window"),
    ("fp32 output of 16-bit input", dict(out_dtype=0), 4, "out_dtype"),
])
def test_mixconv_refusals_need_no_device(what, over, G, match):
    from pytorchcv_amd import _lib
    L = _lib.lib()
    over = dict(over)
    size = over.pop("struct_size", None)
    d = _desc(360, G, **over)
    if size is not None:
        d.struct_size = size
    n = ctypes.c_size_t(0)
    assert L.pcv_mixconv_packed_bytes(ctypes.byref(d), _kernels(G), G, ctypes.byref(n)) == -1, what
    assert match in (L.pcv_last_error(None) or b"").decode(), what


def test_mixconv_refuses_other_kernel_lists():
    from pytorchcv_amd import _lib
    L = _lib.lib()
    n = ctypes.c_size_t(0)
    for ks in ((3,), (3, 7), (5, 7), (3, 5, 7, 9, 11, 13), (1, 1), (3, 5, 9)):
        G = len(ks)
        k = max(ks)
        d = _desc(360, 4, kh=k, kw=k, pad_t=k // 2, pad_l=k // 2, pad_b=k // 2, pad_r=k // 2)
        assert L.pcv_mixconv_packed_bytes(ctypes.byref(d), (ctypes.c_int * G)(*ks), G, ctypes.byref(n)) == -1, ks
        assert "kernel list" in (L.pcv_last_error(None) or b"").decode(), ks
    assert L.pcv_mixconv_packed_bytes(ctypes.byref(_desc()), None, 4, ctypes.byref(n)) == -1


def test_engine_refuses_what_the_launch_does_not_take():
    """Checked before any device call: groups of another form never reach the library."""
    import torch.nn as nn
    from pytorchcv_amd import engine
    ok = [nn.Conv2d(8, 8, 3, 1, 1, groups=8, bias=False), nn.Conv2d(8, 8, 5, 1, 2, groups=8, bias=False)]
    engine.MixConvRunner(ok, None)
    with pytest.raises(NotImplementedError, match="padding k // 2"):
        engine.MixConvRunner([ok[0], nn.Conv2d(8, 8, 5, 1, 0, groups=8, bias=False)], None)
    with pytest.raises(NotImplementedError, match="padding k // 2"):
        engine.MixConvRunner([ok[0], nn.Conv2d(8, 8, 5, 1, 4, dilation=2, groups=8, bias=False)], None)
    with pytest.raises(NotImplementedError, match="2 to 5"):
        engine.MixConvRunner(ok[:1], None)
    r = engine.MixConvRunner(ok, None)
    with pytest.raises(RuntimeError, match="dense handle of 16 channels"):
        r.desc(engine.NHWC(torch.zeros(1, 2, 2, 24), 1, 2, 2, 24), 0)


@pytest.mark.parametrize("name", ["mix1x1_24_144", "mix1x1_144_24"])
def test_pointwise_mixconv_is_a_grouped_convolution(name):
    """The module's weight concatenation run as Conv2d(groups=2) + BatchNorm + activation on the CPU against the reference's
    MixConvBlock output, within fp32 rounding: both sides sum K products per output in fp32, each within (K + 2) u of the exact
    value relative to sum |x||w| |scale| + |shift| (u = 2^-24), so they are within twice that of each other."""
    from pytorchcv_amd.models.mixnet import _GroupedView
    m = blocks_meta()[name]
    blk = build_mix_block(m["case"])
    blk.load_state_dict(util.synth_state_dict(util.template_from_manifest(m["manifest"]), seed=m["weight_seed"]), strict=True)
    view = _GroupedView(blk.conv.convs())
    assert view.groups == 2 and tuple(view.weight.shape) == (view.out_channels, view.in_channels // 2, 1, 1)
    assert view.weight is view.weight                         # cached until a parameter changes
    x = util.synth_input(*m["case"]["x"], seed=m["input_seed"])
    bn = blk.bn
    scale = (bn.weight / torch.sqrt(bn.running_var + bn.eps)).detach()
    shift = (bn.bias - bn.running_mean * scale).detach()
    with torch.no_grad():
        y = F.conv2d(x, view.weight, None, groups=2) * scale[None, :, None, None] + shift[None, :, None, None]
        cond = F.conv2d(x.abs().double(), view.weight.abs().double(), None, groups=2) * scale.abs().double()[None, :, None, None] \
            + shift.abs().double()[None, :, None, None]
    if blk.activate:
        y = y.clamp(min=0)
    g = torch.from_numpy(np.load(os.path.join(util.GOLDEN, "blocks_mixnet.npz"))[name])
    K = view.in_channels // 2
    assert y.shape == g.shape
    assert bool(((y.double() - g.double()).abs() <= 2 * (K + 2) * 2.0 ** -24 * cond).all())
    with torch.no_grad():
        blk.conv.convs()[1].weight.add_(1.0)
    assert torch.equal(view.weight[view.out_channels // 2:], blk.conv.convs()[1].weight)      # rebuilt after a change


def test_default_mode_is_declared_on_every_module(monkeypatch):
    from pytorchcv_amd import engine
    from pytorchcv_amd.model_provider import get_model
    monkeypatch.delenv("PCV_AMD_DTYPE", raising=False)
    net = get_model("mixnet_s").eval()
    assert {engine.compute_dtype_of(m) for m in net.modules()} == {engine.compute_dtype_of(net)}
