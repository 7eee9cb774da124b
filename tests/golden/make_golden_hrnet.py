"""
    Fixture generator for HRNet - runs ONLY where the reference (osmr/pytorchcv 0.0.73) is checked out (--ref). It imports the
    reference's `hrnet.py`, loads build-generated synthetic weights into its modules, runs the reference's CPU forward and freezes
    inputs/outputs as small data files under tests/golden/:

      calib_/logits_/digests_<net>                the make_golden.py formats, for hrnet_w18_small_v1 (widths 16 .. 128) and
                                                  hrnetv2_w18 (widths 18 .. 144: channel pitch != width)
      manifest_hrnet_w18_small_v1.json            the make_golden.py format (552 keys). hrnetv2_w18's 1956 keys would be a 200 KB
                                                  file: its layout, like that of all nine names, is frozen as a hash instead
      blocks_hrnet.npz / .json                    the block cases of HR_CASES below: outputs (one array per output map), key count,
                                                  seeds, the case itself; inputs and weights are regenerated from the seeds (the
                                                  weights from the key names, so a key that differs shows in the output)
      hrnet_param_counts.json                     of all nine names: parameter count, state_dict key count, and the sha256 of the
                                                  state_dict layout (`layout_sha256` below: every key, shape and dtype, in order)

    The JSON files hold one top-level entry per line, without further white space: same content as json.dump(indent=0), a fifth
    of the lines.

    Nothing of the reference is copied: fixtures are inputs/outputs only. The .npz files are written with fixed zip timestamps, so a
    rerun reproduces every file bit for bit. Usage: python tests/golden/make_golden_hrnet.py --ref <reference checkout>
"""

import os
import sys
import json
import copy
import hashlib
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

MODELS = ("hrnet_w18_small_v1", "hrnetv2_w18")
MANIFEST_FOR = ("hrnet_w18_small_v1",)
# the reference's own asserts (hrnet.py:709-717)
PARAM_COUNTS = dict(hrnet_w18_small_v1=13187464, hrnet_w18_small_v2=15597464, hrnetv2_w18=21299004, hrnetv2_w30=37712220,
                    hrnetv2_w32=41232680, hrnetv2_w40=57557160, hrnetv2_w44=67064984, hrnetv2_w48=77469864, hrnetv2_w64=128059944)
WEIGHT_SEED, INPUT_SEED = 8100, 8200

# name, constructor (models/hrnet.py), kwargs, input shapes: "x" one map, "xs" a list of maps (branch i at 1 / 2**i of branch 0)
HR_CASES = [
    dict(name="up_32_16_x2", kind="UpSamplingBlock", kwargs=dict(in_channels=32, out_channels=16, scale_factor=2), x=(2, 32, 4, 6)),
    dict(name="up_144_18_x8", kind="UpSamplingBlock", kwargs=dict(in_channels=144, out_channels=18, scale_factor=8), x=(2, 144, 2, 2)),
    dict(name="block2_16_32", kind="HRBlock",
         kwargs=dict(in_channels_list=[16, 32], out_channels_list=[16, 32], num_branches=2, num_subblocks=[2, 2]),
         xs=[(2, 16, 8, 12), (2, 32, 4, 6)]),
    dict(name="block4_18_144", kind="HRBlock",
         kwargs=dict(in_channels_list=[18, 36, 72, 144], out_channels_list=[18, 36, 72, 144], num_branches=4, num_subblocks=[2, 2, 2, 2]),
         xs=[(2, 18, 16, 16), (2, 36, 8, 8), (2, 72, 4, 4), (2, 144, 2, 2)]),
    dict(name="stage_new_branch", kind="HRStage",
         kwargs=dict(in_channels_list=[16, 32], out_channels_list=[16, 32, 64], num_modules=1, num_branches=3, num_subblocks=[2, 2, 2]),
         xs=[(2, 16, 8, 8), (2, 32, 4, 4)]),
    dict(name="stage_from_init_256_18", kind="HRStage",
         kwargs=dict(in_channels_list=[256], out_channels_list=[18, 36], num_modules=1, num_branches=2, num_subblocks=[2, 2]),
         x=(2, 256, 8, 8)),
    dict(name="init_3_256", kind="HRInitBlock", kwargs=dict(in_channels=3, out_channels=256, mid_channels=64, num_subblocks=2),
         x=(2, 3, 16, 16)),
    dict(name="final_16_128", kind="HRFinalBlock",
         kwargs=dict(in_channels_list=[16, 32, 64, 128], out_channels_list=[128, 256, 512, 1024]),
         xs=[(2, 16, 8, 8), (2, 32, 4, 4), (2, 64, 2, 2), (2, 128, 1, 1)]),
]


def dump_lines(obj, path, nested=None):
    """json with one top-level entry per line (`nested`: one entry of obj[nested] per line instead) and no other white space"""
    def lines(d):
        return ",\n".join("{}:{}".format(json.dumps(k), json.dumps(v, separators=(",", ":"))) for k, v in d.items())
    with open(path, "w") as f:
        if nested is None:
            f.write("{\n" + lines(obj) + "\n}\n")
        else:
            head = {k: v for k, v in obj.items() if k != nested}
            f.write("{" + lines(head).replace("\n", "") + ",\n" + json.dumps(nested) + ":{\n" + lines(obj[nested]) + "\n}}\n")


def layout_sha256(net):
    """sha256 over the lines "<key> <shape> <dtype>" of a state_dict, in its order"""
    text = "\n".join("{} {} {}".format(k, list(v.shape), str(v.dtype).replace("torch.", "")) for k, v in net.state_dict().items())
    return hashlib.sha256(text.encode()).hexdigest()


def build_case(case, models_pkg):
    """The block of `case` from the package `models_pkg` ("pytorchcv.models": the reference here; "pytorchcv_amd.models" in the tests).
    The kwargs are copied: the constructors write into their channel lists."""
    mod = __import__(models_pkg + ".hrnet", fromlist=[case["kind"]])
    return getattr(mod, case["kind"])(**copy.deepcopy(case["kwargs"])).eval()


def case_input(case, seed=INPUT_SEED):
    """One tensor ("x") or a list of tensors ("xs", map i from seed + i)."""
    if "x" in case:
        return synth_input(*case["x"], seed=seed)
    return [synth_input(*shape, seed=seed + i) for i, shape in enumerate(case["xs"])]


def ref_model(name):
    m = __import__("pytorchcv.models.hrnet", fromlist=[name])
    return getattr(m, name)(pretrained=False).eval()


def do_blocks():
    arrays, meta = {}, {}
    for case in HR_CASES:
        blk = build_case(case, "pytorchcv.models")
        blk.load_state_dict(synth_state_dict(blk.state_dict(), seed=WEIGHT_SEED), strict=True)
        x = case_input(case)
        with torch.no_grad():
            y = blk(x)
        ys = list(y) if isinstance(y, (list, tuple)) else [y]
        for i, v in enumerate(ys):
            arrays["{}.{}".format(case["name"], i)] = v.numpy().astype(np.float32)
        meta[case["name"]] = dict(case=case, key_count=len(manifest_of(blk)), weight_seed=WEIGHT_SEED, input_seed=INPUT_SEED,
                                  y_shapes=[list(v.shape) for v in ys], y_is_list=isinstance(y, (list, tuple)))
        print("{:24s} -> {} absmax {:.3f} mean|y| {:.4f}".format(case["name"], [tuple(v.shape) for v in ys],
                                                                 max(float(v.abs().max()) for v in ys),
                                                                 float(np.mean([float(v.abs().mean()) for v in ys]))))
    save_npz(os.path.join(HERE, "blocks_hrnet.npz"), arrays)
    dump_lines({k: meta[k] for k in sorted(meta)}, os.path.join(HERE, "blocks_hrnet.json"))


def do_model(name):
    """make_golden.do_model for this family (its constructor table does not list it)."""
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
            def tap(m, i, o, cname=cname):
                for b, v in enumerate(o if isinstance(o, (list, tuple)) else [o]):
                    taps["{}.{}".format(cname, b)] = v.detach().clone()
            hooks.append(child.register_forward_hook(tap))
    with torch.no_grad():
        y = net(x)
    for h in hooks:
        h.remove()
    if name in MANIFEST_FOR:
        dump_lines(dict(model=name, param_count=nparams, keys=man), os.path.join(HERE, "manifest_{}.json".format(name)), nested="keys")
    dump_lines(calib, os.path.join(HERE, "calib_{}.json".format(name)))
    save_npz(os.path.join(HERE, "logits_{}.npz".format(name)), dict(logits=y.numpy().astype(np.float32),
                                                                    image_ids=np.array(ids, dtype=np.int64)))
    dump_lines({k: digest(v) for k, v in taps.items()}, os.path.join(HERE, "digests_{}.json".format(name)))
    top2 = torch.topk(y, 2, dim=1).values
    print(name, "params", nparams, "keys", len(man), "ids", ids, "margins", [round(float(a - b), 3) for a, b in top2])


def do_counts():
    from pytorchcv.models.common.model_store import calc_net_weight_count
    counts = {}
    for name in sorted(PARAM_COUNTS):
        net = ref_model(name)
        counts[name] = dict(param_count=int(calc_net_weight_count(net)), key_count=len(net.state_dict()), layout_sha256=layout_sha256(net))
        assert counts[name]["param_count"] == PARAM_COUNTS[name]
        print(name, counts[name])
    dump_lines(counts, os.path.join(HERE, "hrnet_param_counts.json"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="checkout of the reference (osmr/pytorchcv)")
    ap.add_argument("--only", default="")
    args = ap.parse_args()
    sys.path.insert(0, args.ref)                     # in front of the repo root: `pytorchcv` below is the reference, not the alias
    import pytorchcv.models.hrnet as _ref_hrnet
    assert os.path.abspath(_ref_hrnet.__file__).startswith(os.path.abspath(args.ref) + os.sep), \
        "pytorchcv resolved to {} - not the reference under {}".format(_ref_hrnet.__file__, args.ref)
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
