"""
    Fixture generator for the split-attention families (ResNeSt-A, SKNet) - runs ONLY where the reference (osmr/pytorchcv 0.0.73)
    is checked out (default /root/reference). It imports the reference's `common/att.py` (SABlock, saconv3x3_block), `resnesta.py`,
    `senet.py` (SEInitBlock) and `sknet.py`, loads build-generated synthetic weights into them, runs the reference's CPU forward
    and freezes inputs/outputs as small data files under tests/golden/:

      manifest_/calib_/logits_/digests_<model>   resnesta18, resnesta50, sknet50 (the make_golden.py formats)
      blocks_splat.npz / .json                   the block cases of SPLAT_CASES below: outputs, manifests, seeds, the case itself
      splat_param_counts.json                    parameter count and state_dict key count of every ResNeSt-A / SKNet name

    Nothing of the reference is copied: fixtures are inputs/outputs only. The .npz files are written with fixed zip timestamps,
    so a rerun reproduces every file bit for bit. Usage: python tests/golden/make_golden_splat.py [--ref /root/reference]
"""

import io
import os
import sys
import json
import zipfile
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

MODELS = ["resnesta18", "resnesta50", "sknet50"]
NAMES = ["resnestabc14", "resnesta18", "resnestabc26", "resnesta50", "resnesta101", "resnesta152", "resnesta200", "resnesta269",
         "sknet50", "sknet101", "sknet152"]

# name, constructor (in the reference), kwargs, input shape
SPLAT_CASES = [
    dict(name="sablock_g1_r2", kind="SABlock", kwargs=dict(out_channels=64, groups=1, radix=2), x=(2, 128, 9, 9)),
    dict(name="sablock_g2_r2", kind="SABlock", kwargs=dict(out_channels=64, groups=2, radix=2), x=(2, 128, 7, 7)),
    dict(name="sablock_g4_r4", kind="SABlock", kwargs=dict(out_channels=32, groups=4, radix=4), x=(2, 128, 8, 8)),
    dict(name="saconv3x3_s1", kind="saconv3x3_block", kwargs=dict(in_channels=32, out_channels=64), x=(2, 32, 15, 15)),
    dict(name="saconv3x3_s2_g2", kind="saconv3x3_block", kwargs=dict(in_channels=64, out_channels=64, stride=2, groups=2),
         x=(2, 64, 15, 15)),
    dict(name="skconv_m2", kind="SKConvBlock", kwargs=dict(in_channels=128, out_channels=128, stride=1), x=(2, 128, 10, 10)),
    dict(name="skconv_m3_s2", kind="SKConvBlock", kwargs=dict(in_channels=128, out_channels=128, stride=2, num_branches=3),
         x=(2, 128, 15, 15)),
    dict(name="resnesta_down_15", kind="ResNeStADownBlock", kwargs=dict(in_channels=64, out_channels=128, stride=2),
         x=(2, 64, 15, 15)),
    dict(name="se_init_block", kind="SEInitBlock", kwargs=dict(in_channels=3, out_channels=64), x=(2, 3, 32, 32)),
    dict(name="resnesta_unit_basic_s2", kind="ResNeStAUnit", kwargs=dict(in_channels=64, out_channels=128, stride=2, bottleneck=False),
         x=(2, 64, 15, 15)),
    dict(name="resnesta_unit_bottleneck_s1", kind="ResNeStAUnit", kwargs=dict(in_channels=64, out_channels=256, stride=1),
         x=(2, 64, 9, 9)),
    dict(name="resnesta_unit_bottleneck_s2", kind="ResNeStAUnit", kwargs=dict(in_channels=256, out_channels=512, stride=2),
         x=(2, 256, 9, 9)),
]


def save_npz(path, arrays):
    """np.savez_compressed with fixed zip member timestamps (byte-reproducible)."""
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED) as z:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, buf.getvalue())


def ref_ctor(kind):
    from pytorchcv.models.common.att import SABlock, saconv3x3_block
    from pytorchcv.models.resnesta import ResNeStADownBlock, ResNeStAUnit
    from pytorchcv.models.senet import SEInitBlock
    from pytorchcv.models.sknet import SKConvBlock
    return {"SABlock": SABlock, "saconv3x3_block": saconv3x3_block, "SKConvBlock": SKConvBlock, "SEInitBlock": SEInitBlock,
            "ResNeStADownBlock": ResNeStADownBlock, "ResNeStAUnit": ResNeStAUnit}[kind]


def ref_model(name):
    m = __import__("pytorchcv.models." + ("sknet" if name.startswith("sknet") else "resnesta"), fromlist=[name])
    return getattr(m, name)(pretrained=False).eval()


def do_blocks():
    arrays, meta = {}, {}
    for ci, case in enumerate(SPLAT_CASES):
        blk = ref_ctor(case["kind"])(**case["kwargs"]).eval()
        wseed, xseed = 7100 + ci, 7200 + ci
        blk.load_state_dict(synth_state_dict(blk.state_dict(), seed=wseed), strict=True)
        x = synth_input(*case["x"], seed=xseed)
        with torch.no_grad():
            y = blk(x)
        arrays[case["name"]] = y.numpy().astype(np.float32)
        meta[case["name"]] = dict(case=case, manifest=manifest_of(blk), weight_seed=wseed, input_seed=xseed, y_shape=list(y.shape))
        print("{:30s} {} -> {} absmax {:.3f}".format(case["name"], case["x"], tuple(y.shape), float(y.abs().max())))
    save_npz(os.path.join(HERE, "blocks_splat.npz"), arrays)
    with open(os.path.join(HERE, "blocks_splat.json"), "w") as f:
        json.dump(meta, f, indent=0, sort_keys=True)


def do_model(name):
    """make_golden.do_model for a name of these families (its constructor table does not list them)."""
    from pytorchcv.models.common.model_store import calc_net_weight_count
    net = ref_model(name)
    man = manifest_of(net)
    nparams = int(calc_net_weight_count(net))
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
    for name in NAMES:
        net = ref_model(name)
        counts[name] = dict(param_count=int(calc_net_weight_count(net)), key_count=len(net.state_dict()))
        print(name, counts[name])
        del net
    with open(os.path.join(HERE, "splat_param_counts.json"), "w") as f:
        json.dump(counts, f, indent=1, sort_keys=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    ap.add_argument("--only", default="")
    args = ap.parse_args()
    sys.path.insert(0, args.ref)                     # in front of the repo root: `pytorchcv` below is the reference, not the alias
    import pytorchcv.models.common.att as _ref_att
    assert os.path.abspath(_ref_att.__file__).startswith(os.path.abspath(args.ref) + os.sep), \
        "pytorchcv resolved to {} - not the reference under {}".format(_ref_att.__file__, args.ref)
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
