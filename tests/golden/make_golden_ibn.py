"""
    Fixture generator for IBN-Net (IBN-ResNet, IBN(b)-ResNet, IBN-ResNeXt) - runs ONLY where the reference (osmr/pytorchcv 0.0.73)
    is checked out (--ref). It imports the reference's `ibnresnet.py` / `ibnbresnet.py` / `ibnresnext.py` / `common/norm.py`, loads
    build-generated synthetic weights into its modules, runs the reference's CPU forward and freezes inputs/outputs as small data
    files under tests/golden/:

      manifest_/calib_/logits_/digests_<model>   ibn_resnet50, ibnb_resnet50, ibn_resnext50_32x4d (the make_golden.py formats)
      blocks_ibn.npz / .json                     the block cases of IBN_CASES below: outputs, manifests, seeds, the case itself
      ibn_param_counts.json                      parameter count and state_dict key count of all nine names

    Nothing of the reference is copied: fixtures are inputs/outputs only. The .npz files are written with fixed zip timestamps, so a
    rerun reproduces every file bit for bit. Usage: python tests/golden/make_golden_ibn.py --ref <reference checkout>
"""

import os
import sys
import json
import argparse
import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

from pytorchcv_amd.synth import synth_state_dict, synth_input  # noqa: E402
import make_golden  # noqa: E402
from make_golden import calibrate, pick_images, images, digest, manifest_of  # noqa: E402
from make_golden_splat import save_npz  # noqa: E402

MODELS = ["ibn_resnet50", "ibnb_resnet50", "ibn_resnext50_32x4d"]
MODULE_OF = {"ibn_resnet": "ibnresnet", "ibnb_resnet": "ibnbresnet", "ibn_resnext": "ibnresnext"}
# the reference's own asserts (ibnresnet.py:427-429, ibnbresnet.py, ibnresnext.py)
PARAM_COUNTS = {"ibn_resnet50": 25557032, "ibn_resnet101": 44549160, "ibn_resnet152": 60192808,
                "ibnb_resnet50": 25558568, "ibnb_resnet101": 44550696, "ibnb_resnet152": 60194344,
                "ibn_resnext50_32x4d": 25028904, "ibn_resnext101_32x4d": 44177704, "ibn_resnext101_64x4d": 83455272}
WEIGHT_SEED, INPUT_SEED = 7700, 7800

# name, module (models/<module>.py or common/norm.py as "norm"), constructor, kwargs, input shape
IBN_CASES = [
    dict(name="ibn_64", module="norm", kind="IBN", kwargs=dict(channels=64), x=(3, 64, 7, 9)),
    dict(name="ibn_conv1x1_64_64", module="ibnresnet", kind="ibn_conv1x1_block", kwargs=dict(in_channels=64, out_channels=64, use_ibn=True),
         x=(2, 64, 9, 9)),
    dict(name="unit_64_256_ibn", module="ibnresnet", kind="IBNResUnit", kwargs=dict(in_channels=64, out_channels=256, stride=1, conv1_ibn=True),
         x=(2, 64, 8, 8)),
    dict(name="unit_256_512_s2_ibn", module="ibnresnet", kind="IBNResUnit", kwargs=dict(in_channels=256, out_channels=512, stride=2, conv1_ibn=True),
         x=(2, 256, 10, 10)),
    dict(name="unit_1024_2048_s2", module="ibnresnet", kind="IBNResUnit", kwargs=dict(in_channels=1024, out_channels=2048, stride=2, conv1_ibn=False),
         x=(2, 1024, 6, 6)),
    dict(name="xunit_256_512_s2_ibn", module="ibnresnext", kind="IBNResNeXtUnit",
         kwargs=dict(in_channels=256, out_channels=512, stride=2, cardinality=32, bottleneck_width=4, conv1_ibn=True), x=(2, 256, 8, 8)),
    dict(name="bunit_256_256_in", module="ibnbresnet", kind="IBNbResUnit", kwargs=dict(in_channels=256, out_channels=256, stride=1, use_inst_norm=True),
         x=(2, 256, 7, 7)),
    dict(name="bunit_256_512_s2_in", module="ibnbresnet", kind="IBNbResUnit", kwargs=dict(in_channels=256, out_channels=512, stride=2, use_inst_norm=True),
         x=(2, 256, 8, 8)),
    dict(name="binit_3_64", module="ibnbresnet", kind="IBNbResInitBlock", kwargs=dict(in_channels=3, out_channels=64), x=(2, 3, 32, 30)),
]


def build_case(case, models_pkg):
    """The block of `case` from the package `models_pkg` ("pytorchcv.models": the reference here; "pytorchcv_amd.models" in the tests)."""
    modname = "common.norm" if case["module"] == "norm" else case["module"]
    mod = __import__(models_pkg + "." + modname, fromlist=[case["kind"]])
    return getattr(mod, case["kind"])(**case["kwargs"]).eval()


def ref_model(name):
    modname = [m for p, m in MODULE_OF.items() if name.startswith(p)][0]
    m = __import__("pytorchcv.models." + modname, fromlist=[name])
    return getattr(m, name)(pretrained=False).eval()


def do_blocks():
    arrays, meta = {}, {}
    for case in IBN_CASES:
        blk = build_case(case, "pytorchcv.models")
        blk.load_state_dict(synth_state_dict(blk.state_dict(), seed=WEIGHT_SEED), strict=True)
        x = synth_input(*case["x"], seed=INPUT_SEED)
        with torch.no_grad():
            y = blk(x)
        arrays[case["name"]] = y.numpy().astype(np.float32)
        meta[case["name"]] = dict(case=case, manifest=manifest_of(blk), weight_seed=WEIGHT_SEED, input_seed=INPUT_SEED,
                                  y_shape=list(y.shape))
        print("{:22s} {} -> {} absmax {:.3f} mean|y| {:.4f}".format(case["name"], case["x"], tuple(y.shape), float(y.abs().max()),
                                                                    float(y.abs().mean())))
    save_npz(os.path.join(HERE, "blocks_ibn.npz"), arrays)
    with open(os.path.join(HERE, "blocks_ibn.json"), "w") as f:
        json.dump(meta, f, indent=0, sort_keys=True)


def do_model(name):
    """make_golden.do_model for a name of this family (its constructor table does not list it)."""
    from pytorchcv.models.common.model_store import calc_net_weight_count
    net = ref_model(name)
    man = manifest_of(net)
    nparams = int(calc_net_weight_count(net))
    assert nparams == PARAM_COUNTS[name]
    net.load_state_dict(synth_state_dict(net.state_dict(), seed=1234), strict=True)
    calib = calibrate(net, synth_input(2, seed=7))
    sd = synth_state_dict(net.state_dict(), seed=1234, calib={k: tuple(v) for k, v in calib.items()})
    net.load_state_dict(sd, strict=True)
    ids = pick_images(net)
    x = images(ids)
    taps, hooks = {}, []
    for cname, child in net.features.named_children():
        if cname == "init_block" or cname.startswith("stage"):
            hooks.append(child.register_forward_hook(lambda m, i, o, cname=cname: taps.__setitem__(cname, o.detach())))
    with torch.no_grad():
        y = net(x)
    for h in hooks:
        h.remove()
    with open(os.path.join(HERE, "manifest_{}.json".format(name)), "w") as f:
        json.dump(dict(model=name, param_count=nparams, keys=man), f, indent=0)
    with open(os.path.join(HERE, "calib_{}.json".format(name)), "w") as f:
        json.dump(calib, f, indent=0)
    save_npz(os.path.join(HERE, "logits_{}.npz".format(name)), dict(logits=y.numpy().astype(np.float32),
                                                                    image_ids=np.array(ids, dtype=np.int64)))
    with open(os.path.join(HERE, "digests_{}.json".format(name)), "w") as f:
        json.dump({k: digest(v) for k, v in taps.items()}, f, indent=0)
    top2 = torch.topk(y, 2, dim=1).values
    print(name, "params", nparams, "keys", len(man), "ids", ids, "margins", [round(float(a - b), 3) for a, b in top2])


def do_counts():
    from pytorchcv.models.common.model_store import calc_net_weight_count
    counts = {}
    for name in sorted(PARAM_COUNTS):
        net = ref_model(name)
        counts[name] = dict(param_count=int(calc_net_weight_count(net)), key_count=len(net.state_dict()))
        assert counts[name]["param_count"] == PARAM_COUNTS[name], name
        print(name, counts[name])
        del net
    with open(os.path.join(HERE, "ibn_param_counts.json"), "w") as f:
        json.dump(counts, f, indent=1, sort_keys=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="checkout of the reference (osmr/pytorchcv)")
    ap.add_argument("--only", default="")
    args = ap.parse_args()
    sys.path.insert(0, args.ref)                     # in front of the repo root: `pytorchcv` below is the reference, not the alias
    import pytorchcv.models.ibnresnet as _ref_ibn
    assert os.path.abspath(_ref_ibn.__file__).startswith(os.path.abspath(args.ref) + os.sep), \
        "pytorchcv resolved to {} - not the reference under {}".format(_ref_ibn.__file__, args.ref)
    assert make_golden.N_IMAGES == 4
    torch.manual_seed(0)
    if args.only in ("", "counts"):
        do_counts()
    if args.only in ("", "blocks"):
        do_blocks()
    for name in MODELS:
        if args.only in ("", name):
            do_model(name)


if __name__ == "__main__":
    main()
