"""
    Fixture generator for the fused resize (pcv_resize_crop_u8, pytorchcv_amd/eval.py: preprocess_frames) - runs where PIL is
    installed. The reference's accuracy figures were produced with torchvision's `Resize` on PIL images, i.e. with PIL's antialiased
    bilinear `Image.resize`; this script freezes what PIL answers, so that the tests can hold the package's integer restatement of
    that algorithm against it without PIL:

      resize_pil.npz   src_<case> / out_<case>  small seeded uint8 sources and PIL's `resize((ow, oh), Image.BILINEAR)` of them
                       sha1_<case>              for the two real-size cases only the SHA-1 of PIL's output (their sources come from
                                                the integer formula `real_source`, so nothing large is stored)
                       pil_version              the PIL that answered

    Written with fixed zip timestamps: a rerun reproduces the file bit for bit. Usage: python tests/golden/make_golden_resize.py
"""

import io
import os
import hashlib
import zipfile
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))

# name: (source height, source width, channels, output height, output width). The first seven are the small frames of the GPU
# sweep at size 37 (torchvision's output size); the rest are free (ow, oh) pairs: strong down-scales, mixed directions, 1-pixel axes.
SMALL_CASES = {
    "land_41x53": (41, 53, 3, 37, 47),
    "port_53x41": (53, 41, 3, 47, 37),
    "square_64": (64, 64, 3, 37, 37),
    "up_7x9": (7, 9, 3, 37, 47),
    "up_20x25": (20, 25, 1, 37, 46),
    "ident_37": (37, 37, 3, 37, 37),
    "ident_axis_37x64": (37, 64, 1, 37, 64),
    "down8_64x48": (64, 48, 3, 8, 6),
    "mixed_64x5": (64, 5, 1, 3, 40),
    "one_to_5": (1, 1, 3, 5, 5),
    "to_one_2x3": (2, 3, 1, 1, 1),
    "down40_60x40": (60, 40, 1, 2, 1),
    "odd_33x17": (33, 17, 3, 40, 21),
}
# name: (source height, source width, output height, output width), three channels
REAL_CASES = {
    "real_375x500": (375, 500, 256, 341),
    "real_500x333": (500, 333, 384, 256),
}


def small_source(name):
    """The seeded source of a small case: half noise, half a smooth ramp (so both rounding and range are exercised)."""
    hs, ws, c = SMALL_CASES[name][:3]
    rng = np.random.RandomState(sorted(SMALL_CASES).index(name) + 4100)
    noise = rng.randint(0, 256, size=(hs, ws, c)).astype(np.int64)
    yy, xx = np.mgrid[0:hs, 0:ws]
    ramp = ((yy * 255) // max(hs - 1, 1) + (xx * 255) // max(ws - 1, 1)) // 2
    mix = np.where(((yy // 4 + xx // 4) % 2 == 0)[..., None], noise, ramp[..., None] + 0 * noise)
    return mix.astype(np.uint8)


def real_source(hs, ws):
    """A real-size three-channel source from integers only: a smooth field with hashed low bits."""
    yy, xx, cc = np.meshgrid(np.arange(hs, dtype=np.uint64), np.arange(ws, dtype=np.uint64), np.arange(3, dtype=np.uint64),
                             indexing="ij")
    smooth = (yy * np.uint64(3) + xx * np.uint64(2) + cc * np.uint64(40)) % np.uint64(256)
    h = (yy * np.uint64(7919) + xx * np.uint64(104729) + cc * np.uint64(1299709) + np.uint64(12345)) * np.uint64(2654435761)
    h = (h >> np.uint64(13)) & np.uint64(63)
    return ((smooth + h) % np.uint64(256)).astype(np.uint8)


def save_npz(path, arrays):
    """np.savez_compressed with fixed zip member timestamps (byte-reproducible)."""
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED) as z:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, buf.getvalue())


def pil_resize(src, oh, ow):
    """PIL's answer for a uint8 [H, W, C] array (C = 1: mode L, C = 3: mode RGB)."""
    from PIL import Image
    img = Image.fromarray(src[:, :, 0] if src.shape[2] == 1 else src)
    out = np.asarray(img.resize((ow, oh), Image.BILINEAR))
    return out.reshape(oh, ow, src.shape[2])


def main():
    import PIL
    arrays = {"pil_version": np.frombuffer(PIL.__version__.encode(), dtype=np.uint8)}
    for name in sorted(SMALL_CASES):
        oh, ow = SMALL_CASES[name][3:]
        src = small_source(name)
        arrays["src_" + name] = src
        arrays["out_" + name] = pil_resize(src, oh, ow)
    for name in sorted(REAL_CASES):
        hs, ws, oh, ow = REAL_CASES[name]
        out = pil_resize(real_source(hs, ws), oh, ow)
        arrays["sha1_" + name] = np.frombuffer(hashlib.sha1(out.tobytes()).digest(), dtype=np.uint8)
    path = os.path.join(HERE, "resize_pil.npz")
    save_npz(path, arrays)
    print("PIL", PIL.__version__, "->", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
