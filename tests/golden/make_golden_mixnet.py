"""
    Fixture generator for MixNet - runs ONLY where the reference (osmr/pytorchcv 0.0.73) is checked out (default /root/reference).
    It imports the reference's `mixnet.py`, loads build-generated synthetic weights into its modules, runs the reference's CPU
    forward and freezes inputs/outputs as small data files under tests/golden/:

      manifest_/calib_/logits_/digests_<model>   mixnet_s, mixnet_m, mixnet_l (the make_golden.py formats)
      blocks_mixnet.npz / .json                  the block cases of MIX_CASES below: outputs, manifests, seeds, the case itself
      mixnet_param_counts.json                   parameter count and state_dict key count of the three names

    Nothing of the reference is copied: fixtures are inputs/outputs only. The .npz files are written with fixed zip timestamps, so a
    rerun reproduces every file bit for bit. Usage: python tests/golden/make_golden_mixnet.py [--ref /root/reference]
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

MODELS = ["mixnet_s", "mixnet_m", "mixnet_l"]
PARAM_COUNTS = {"mixnet_s": 4134606, "mixnet_m": 5014382, "mixnet_l": 7329252}      # the reference's own asserts (mixnet.py:596-598)
WEIGHT_SEED, INPUT_SEED = 7500, 7600


def _mix(channels, count, stride, activation):
    return dict(in_channels=channels, out_channels=channels, kernel_size=[3 + 2 * i for i in range(count)], stride=stride,
                padding=[1 + i for i in range(count)], groups=channels, activation=activation)


def _unit(cin, cout, stride, counts, exp, se, activation):
    return dict(in_channels=cin, out_channels=cout, stride=stride, exp_kernel_count=counts[0], conv1_kernel_count=counts[1],
                conv2_kernel_count=counts[2], exp_factor=exp, se_factor=se, activation=activation)


# name, constructor (in the reference), kwargs (`activation` as a name: "relu", "swish" or None), input shape
MIX_CASES = [
    dict(name="mixdw_c360_k4_s1", kind="MixConvBlock", kwargs=_mix(360, 4, 1, "swish"), x=(2, 360, 9, 11)),
    dict(name="mixdw_c720_k5_s2", kind="MixConvBlock", kwargs=_mix(720, 5, 2, "swish"), x=(2, 720, 9, 10)),
    dict(name="mixdw_c144_k3_s2", kind="MixConvBlock", kwargs=_mix(144, 3, 2, "relu"), x=(3, 144, 15, 16)),
    dict(name="mix1x1_24_144", kind="mixconv1x1_block", kwargs=dict(in_channels=24, out_channels=144, kernel_count=2, activation="relu"),
         x=(2, 24, 7, 9)),
    dict(name="mix1x1_144_24", kind="mixconv1x1_block", kwargs=dict(in_channels=144, out_channels=24, kernel_count=2, activation=None),
         x=(2, 144, 7, 9)),
    dict(name="unit_40_40", kind="MixUnit", kwargs=_unit(40, 40, 1, (2, 2, 2), 6, 2, "swish"), x=(2, 40, 9, 9)),
    dict(name="unit_120_120_w90", kind="MixUnit", kwargs=_unit(120, 120, 1, (2, 4, 2), 3, 2, "swish"), x=(2, 120, 7, 7)),
    dict(name="unit_16_24_s2", kind="MixUnit", kwargs=_unit(16, 24, 2, (2, 1, 2), 6, 0, "relu"), x=(2, 16, 16, 16)),
    dict(name="unit_120_200_s2", kind="MixUnit", kwargs=_unit(120, 200, 2, (1, 5, 1), 6, 2, "swish"), x=(2, 120, 14, 14)),
]


def build_case(case, mod, activ):
    """The block of `case` from `mod` (a mixnet module: the reference's here, the package's in the tests) with the activation
    generators of `activ` (its common.activ)."""
    kw = dict(case["kwargs"])
    name = kw["activation"]
    kw["activation"] = None if name is None else {"relu": activ.lambda_relu, "swish": activ.lambda_swish}[name]()
    return getattr(mod, case["kind"])(**kw).eval()


def ref_model(name):
    m = __import__("pytorchcv.models.mixnet", fromlist=[name])
    return getattr(m, name)(pretrained=False).eval()


def do_blocks():
    import pytorchcv.models.mixnet as ref_mixnet
    import pytorchcv.models.common.activ as ref_activ
    arrays, meta = {}, {}
    for case in MIX_CASES:
        blk = build_case(case, ref_mixnet, ref_activ)
        blk.load_state_dict(synth_state_dict(blk.state_dict(), seed=WEIGHT_SEED), strict=True)
        x = synth_input(*case["x"], seed=INPUT_SEED)
        with torch.no_grad():
            y = blk(x)
        arrays[case["name"]] = y.numpy().astype(np.float32)
        meta[case["name"]] = dict(case=case, manifest=manifest_of(blk), weight_seed=WEIGHT_SEED, input_seed=INPUT_SEED,
                                  y_shape=list(y.shape))
        print("{:22s} {} -> {} absmax {:.3f} mean|y| {:.4f}".format(case["name"], case["x"], tuple(y.shape), float(y.abs().max()),
                                                                    float(y.abs().mean())))
    save_npz(os.path.join(HERE, "blocks_mixnet.npz"), arrays)
    with open(os.path.join(HERE, "blocks_mixnet.json"), "w") as f:
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
    for name in MODELS:
        net = ref_model(name)
        counts[name] = dict(param_count=int(calc_net_weight_count(net)), key_count=len(net.state_dict()))
        assert counts[name]["param_count"] == PARAM_COUNTS[name], name
        print(name, counts[name])
        del net
    with open(os.path.join(HERE, "mixnet_param_counts.json"), "w") as f:
        json.dump(counts, f, indent=1, sort_keys=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    ap.add_argument("--only", default="")
    args = ap.parse_args()
    sys.path.insert(0, args.ref)                     # in front of the repo root: `pytorchcv` below is the reference, not the alias
    import pytorchcv.models.mixnet as _ref_mixnet
    assert os.path.abspath(_ref_mixnet.__file__).startswith(os.path.abspath(args.ref) + os.sep), \
        "pytorchcv resolved to {} - not the reference under {}".format(_ref_mixnet.__file__, args.ref)
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
