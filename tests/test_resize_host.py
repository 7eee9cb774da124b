"""CPU: the host half of the fused resize (pcv_resize_plan_bytes / pcv_resize_plan, pytorchcv_amd/csrc/resize_plan.hpp) and the
arithmetic it implements. `resize_restated` below is a small numpy restatement of PIL's antialiased bilinear resize (the text at
the head of resize_plan.hpp); it is held against PIL's frozen answers (tests/golden/resize_pil.npz) and against live PIL, and the
planner's tables are held against it. tests/test_gpu_resize.py imports it as the expectation of the kernel."""

import os
import math
import ctypes
import shutil
import struct
import hashlib
import subprocess
import numpy as np
import pytest

from make_golden_resize import SMALL_CASES, REAL_CASES, small_source, real_source

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "resize_pil.npz")
PRECISION_BITS = 22


# ---- the restatement -------------------------------------------------------------------------------------------------------------
def axis_coeffs(n_in, n_out):
    """[(xmin, n, [kk])] for every output of an axis n_in -> n_out, and ksize. Python floats: IEEE double, no fused multiply-add."""
    scale = n_in / n_out
    fs = max(scale, 1.0)
    support = fs
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / fs
    out = []
    for xx in range(n_out):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        n = min(int(center + support + 0.5), n_in) - xmin
        w = []
        for x in range(n):
            t = abs((x + xmin - center + 0.5) * ss)
            w.append(1.0 - t if t < 1.0 else 0.0)
        ww = 0.0
        for v in w:                                  # left to right, as the C loop adds them (the builtin sum() compensates)
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        out.append((xmin, n, [int(0.5 + v * (1 << PRECISION_BITS)) for v in w]))
    return out, ksize


def _pass(src, coeffs, axis):
    """One integer pass along `axis` (0 or 1) of a uint8 [H, W, C] array."""
    src = src.astype(np.int64)
    shape = list(src.shape)
    shape[axis] = len(coeffs)
    out = np.empty(shape, dtype=np.uint8)
    for i, (xmin, n, kk) in enumerate(coeffs):
        k = np.array(kk, dtype=np.int64)
        if axis == 1:
            acc = (src[:, xmin:xmin + n, :] * k[None, :, None]).sum(axis=1)
        else:
            acc = (src[xmin:xmin + n, :, :] * k[:, None, None]).sum(axis=0)
        v = np.clip((acc + (1 << (PRECISION_BITS - 1))) >> PRECISION_BITS, 0, 255).astype(np.uint8)
        if axis == 1:
            out[:, i, :] = v
        else:
            out[i, :, :] = v
    return out


def resize_restated(src, oh, ow):
    """PIL's `resize((ow, oh), Image.BILINEAR)` of a uint8 [H, W, C] array: horizontal pass, rounded to uint8, vertical pass."""
    hs, ws, _ = src.shape
    tmp = _pass(src, axis_coeffs(ws, ow)[0], 1)
    return _pass(tmp, axis_coeffs(hs, oh)[0], 0)


# ---- 1. the restatement is PIL ---------------------------------------------------------------------------------------------------
def test_restatement_equals_frozen_pil():
    z = np.load(GOLDEN)
    for name in sorted(SMALL_CASES):
        hs, ws, c, oh, ow = SMALL_CASES[name]
        src = z["src_" + name]
        assert src.shape == (hs, ws, c) and np.array_equal(src, small_source(name))
        assert np.array_equal(resize_restated(src, oh, ow), z["out_" + name]), name
    for name in sorted(REAL_CASES):
        hs, ws, oh, ow = REAL_CASES[name]
        got = resize_restated(real_source(hs, ws), oh, ow)
        assert hashlib.sha1(got.tobytes()).digest() == z["sha1_" + name].tobytes(), name


def test_restatement_equals_live_pil():
    pytest.importorskip("PIL")
    from make_golden_resize import pil_resize
    for name in sorted(SMALL_CASES):
        hs, ws, c, oh, ow = SMALL_CASES[name]
        src = small_source(name)
        assert np.array_equal(resize_restated(src, oh, ow), pil_resize(src, oh, ow)), name
    for name in sorted(REAL_CASES):
        hs, ws, oh, ow = REAL_CASES[name]
        src = real_source(hs, ws)
        assert np.array_equal(resize_restated(src, oh, ow), pil_resize(src, oh, ow)), name


# ---- 2. output size --------------------------------------------------------------------------------------------------------------
def test_resize_output_size():
    from pytorchcv_amd import eval as ev
    assert ev.resize_output_size(375, 500, 256) == (256, 341)
    assert ev.resize_output_size(500, 375, 256) == (341, 256)
    assert ev.resize_output_size(256, 256, 256) == (256, 256)
    assert ev.resize_output_size(100, 333, 37) == (37, 123)
    assert ev.resize_output_size(1000, 23, 37) == (1608, 37)
    for name in ("resize_output_size", "preprocess_frames"):
        assert name in ev.__all__


# ---- the blob, as resize_plan.hpp lays it out -----------------------------------------------------------------------------------
HEADER = struct.Struct("<I7iQQ")          # magic, N, C, H, W, items, stage_bytes, reserved, bytes, src_bytes
FRAME = struct.Struct("<Q14i2I")          # src, Hs, Ws, oh, ow, top, left, row0, row1, hk, vk, band, nbands, item0, reserved, htab, vtab
MAGIC = 0x315A5352
STAGE_BYTES = 64 * 1024


def plan_blob(sizes, c, size, h, w, pointers=None, expect_ok=True):
    """(rc, blob bytes or error text) of the two planning calls for frames of the given (Hs, Ws)."""
    from pytorchcv_amd import _lib
    L = _lib.lib()
    n = len(sizes)
    hs = (ctypes.c_int * max(n, 1))(*[s[0] for s in sizes])
    ws = (ctypes.c_int * max(n, 1))(*[s[1] for s in sizes])
    nbytes = ctypes.c_size_t()
    rc = L.pcv_resize_plan_bytes(n, hs, ws, c, size, h, w, ctypes.byref(nbytes))
    if rc != 0:
        return rc, (L.pcv_last_error(None) or b"").decode()
    ptrs = (ctypes.c_void_p * n)(*(pointers or [0x1000 * (i + 1) for i in range(n)]))
    buf = ctypes.create_string_buffer(nbytes.value)
    rc = L.pcv_resize_plan(ptrs, n, hs, ws, c, size, h, w, buf, nbytes.value)
    if rc != 0:
        return rc, (L.pcv_last_error(None) or b"").decode()
    return 0, buf.raw


def blob_frames(blob):
    hd = HEADER.unpack_from(blob, 0)
    assert hd[0] == MAGIC and hd[8] == len(blob)
    frames = [FRAME.unpack_from(blob, HEADER.size + i * FRAME.size) for i in range(hd[1])]
    return hd, frames


def blob_table(blob, offset, count, ksize):
    t = np.frombuffer(blob, dtype=np.int32, count=count * (2 + ksize), offset=offset)
    return t[:count], t[count:2 * count], t[2 * count:].reshape(count, ksize)


# ---- 3. planner tables -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_out", [1, 2, 37, 224, 256, 341])
def test_planner_tables_equal_the_restatement(n_out):
    """A square n_in x n_in frame at size n_out with the full n_out x n_out crop: both tables cover every output of n_in -> n_out."""
    ins = [1, 2, 3, 7, 17, 37, 41, 53, 64, 100, 255, 256, 257, 500, 1000, 4000]
    rc, blob = plan_blob([(i, i) for i in ins], 1, n_out, n_out, n_out)
    assert rc == 0, blob
    hd, frames = blob_frames(blob)
    assert hd[1:5] == (len(ins), 1, n_out, n_out)
    for n_in, f in zip(ins, frames):
        want, ksize = axis_coeffs(n_in, n_out)
        (src, hs, ws, oh, ow, top, left, row0, row1, hk, vk, band, nbands, item0, _, htab, vtab) = f
        assert (hs, ws, oh, ow, top, left, hk, vk) == (n_in, n_in, n_out, n_out, 0, 0, ksize, ksize)
        assert (row0, row1) == (0, n_in) and nbands == -(-n_out // band) and 1 <= band <= 16
        for off, k in ((htab, hk), (vtab, vk)):
            xmin, n, kk = blob_table(blob, off, n_out, k)
            for xx, (wmin, wn, wkk) in enumerate(want):
                assert (int(xmin[xx]), int(n[xx])) == (wmin, wn), (n_in, n_out, xx)
                assert kk[xx, :wn].tolist() == wkk and not kk[xx, wn:].any(), (n_in, n_out, xx)


def test_planner_crop_and_bands():
    """Cropped tables start at the crop origin, the row range is what the crop rows touch, bands tile the rows, items add up."""
    from pytorchcv_amd import eval as ev
    sizes = [(375, 500), (500, 333), (1000, 23), (23, 1000), (300, 290)]
    rc, blob = plan_blob(sizes, 3, 37, 32, 32, pointers=[0x7000 + 16 * i for i in range(len(sizes))])
    assert rc == 0, blob
    hd, frames = blob_frames(blob)
    items = 0
    for i, ((hs, ws), f) in enumerate(zip(sizes, frames)):
        (src, fhs, fws, oh, ow, top, left, row0, row1, hk, vk, band, nbands, item0, _, htab, vtab) = f
        assert src == 0x7000 + 16 * i and (fhs, fws) == (hs, ws)
        assert (oh, ow) == ev.resize_output_size(hs, ws, 37) and (top, left) == ev.center_crop_box(oh, ow, 32)
        wv, kv = axis_coeffs(hs, oh)
        wh, kh = axis_coeffs(ws, ow)
        assert (hk, vk) == (kh, kv)
        xmin, n, kk = blob_table(blob, vtab, 32, vk)
        assert [(int(a), int(b)) for a, b in zip(xmin, n)] == [(m, c) for m, c, _ in wv[top:top + 32]]
        assert row0 == wv[top][0] and row1 == wv[top + 31][0] + wv[top + 31][1]
        xmin, n, kk = blob_table(blob, htab, 32, hk)
        assert [kk[x, :n[x]].tolist() for x in range(32)] == [k for _, _, k in wh[left:left + 32]]
        assert item0 == items and nbands == -(-32 // band)
        items += nbands
    assert hd[5] == items and 0 < hd[6] <= STAGE_BYTES and hd[6] % 16 == 0
    # frames of one size share their tables: same offsets, own pointer and items; the blob grows by the frame record only
    rc, twice = plan_blob(sizes + [sizes[0]], 3, 37, 32, 32, pointers=[0x7000 + 16 * i for i in range(len(sizes) + 1)])
    assert rc == 0 and len(twice) - len(blob) in (FRAME.size - 8, FRAME.size + 8)          # 72 bytes, 16-byte rounding
    first, last = blob_frames(twice)[1][0], blob_frames(twice)[1][-1]
    assert last[1:13] == first[1:13] and last[15:] == first[15:] and last[0] == 0x7000 + 16 * len(sizes) and last[13] == items


def test_blob_alone_reproduces_the_resize():
    """The kernel's walk, on the CPU: per frame and band, the band's source rows through the horizontal table into a uint8 staging
    of the planned size, then the vertical table out of it. Equal to the crop of the restated resize - so the tables, the crop
    origin, the band windows and the staging size in the blob are all the launch needs."""
    from pytorchcv_amd import eval as ev
    sizes = [(41, 53), (7, 9), (37, 64), (300, 290), (1000, 23), (23, 1000)]
    rng = np.random.RandomState(12)
    for c, img, size in ((3, 32, 37), (1, 33, 38)):
        srcs = [rng.randint(0, 256, size=(h, w, c)).astype(np.uint8) for h, w in sizes]
        rc, blob = plan_blob(sizes, c, size, img, img)
        assert rc == 0, blob
        hd, frames = blob_frames(blob)
        pitch = (img * c + 3) // 4 * 4
        for src, f in zip(srcs, frames):
            (_, hs, ws, oh, ow, top, left, row0, row1, hk, vk, band, nbands, item0, _, htab, vtab) = f
            hx, hn, hkk = blob_table(blob, htab, img, hk)
            vx, vn, vkk = blob_table(blob, vtab, img, vk)
            out = np.zeros((img, img, c), dtype=np.uint8)
            for b in range(nbands):
                y0, y1 = b * band, min(b * band + band, img)
                r0 = int(vx[y0])
                rows = int(vx[y1 - 1] + vn[y1 - 1]) - r0
                assert 0 < rows and rows * pitch <= hd[6] and row0 <= r0 and r0 + rows <= row1
                stage = np.zeros((rows, img, c), dtype=np.int64)
                for x in range(img):
                    taps = src[r0:r0 + rows, hx[x]:hx[x] + hn[x], :].astype(np.int64) * hkk[x, :hn[x]].astype(np.int64)[None, :, None]
                    stage[:, x, :] = np.clip((taps.sum(axis=1) + (1 << 21)) >> 22, 0, 255)
                for y in range(y0, y1):
                    taps = stage[vx[y] - r0:vx[y] - r0 + vn[y]] * vkk[y, :vn[y]].astype(np.int64)[:, None, None]
                    out[y] = np.clip((taps.sum(axis=0) + (1 << 21)) >> 22, 0, 255)
            want = resize_restated(src, oh, ow)[top:top + img, left:left + img]
            assert (top, left) == ev.center_crop_box(oh, ow, img) and np.array_equal(out, want), (hs, ws, c)


# ---- 4. binding ------------------------------------------------------------------------------------------------------------------
def test_binding_and_abi_version():
    from pytorchcv_amd import _lib
    L = _lib.lib()
    for name in ("pcv_resize_plan_bytes", "pcv_resize_plan", "pcv_resize_crop_u8"):
        assert name in _lib.exported_symbols() and hasattr(L, name)
    assert _lib.PCV_ABI_VERSION == 5 and L.pcv_abi_version() == 5
    rc, blob = plan_blob([(41, 53), (7, 9)], 3, 37, 32, 32)             # no device, no context
    assert rc == 0 and len(blob) % 16 == 0
    assert L.pcv_resize_crop_u8(None, blob, 0x1000, len(blob), 0x2000, 32, 0x3000, 0x4000, 1, None) == -1


# ---- 5. refusals -----------------------------------------------------------------------------------------------------------------
def test_planner_refusals():
    from pytorchcv_amd import _lib
    L = _lib.lib()
    ok = [(41, 53), (64, 64)]
    assert plan_blob(ok, 3, 37, 32, 32)[0] == 0
    for why, args in (("C = 5", (ok, 5, 37, 32, 32)), ("C = 0", (ok, 0, 37, 32, 32)), ("N = 0", ([], 3, 37, 32, 32)),
                      ("size 0", (ok, 3, 0, 32, 32)), ("crop larger than the resized frame", (ok, 3, 37, 38, 32)),
                      ("crop wider than the resized frame", ([(41, 53), (64, 40)], 3, 37, 32, 60))):
        rc, text = plan_blob(*args)
        assert rc == -1 and text.startswith("pcv_resize_plan_bytes: "), why
    # a wrong `bytes`
    hs = (ctypes.c_int * 2)(41, 64)
    ws = (ctypes.c_int * 2)(53, 64)
    nbytes = ctypes.c_size_t()
    assert L.pcv_resize_plan_bytes(2, hs, ws, 3, 37, 32, 32, ctypes.byref(nbytes)) == 0
    ptrs = (ctypes.c_void_p * 2)(0x1000, 0x2000)
    buf = ctypes.create_string_buffer(nbytes.value + 16)
    for wrong in (nbytes.value - 16, nbytes.value + 16, 0):
        assert L.pcv_resize_plan(ptrs, 2, hs, ws, 3, 37, 32, 32, buf, wrong) == -1
        assert b"bytes" in L.pcv_last_error(None)
    assert L.pcv_resize_plan(ptrs, 2, hs, ws, 3, 37, 32, 32, buf, nbytes.value) == 0


def test_planner_refuses_a_window_that_cannot_be_staged():
    """A 32 x 32 x 3 crop at size 37 keeps 96 bytes per resampled source row, so one output row fits the kernel's staging (64 KB, and
    the 160 KB of a CU's LDS alike) up to a down-scale of a few hundred. Under torchvision's rule both axes scale by (shorter side /
    size), so the window of about 21,600 source rows (2 MB) belongs to a frame whose SHORTER side is 400000: 400000 x 400000. The
    planner refuses it on the host without anything being allocated. (A 400000 x 8 frame at size 37 has a shorter side of 8: both
    axes up-scale, its row window is 3 rows, and it is planned like any other frame - checked here against the restatement.)"""
    rc, text = plan_blob([(41, 53), (400000, 400000)], 3, 37, 32, 32)
    assert rc == -1 and "staging" in text
    rc, text = plan_blob([(400000, 400000)], 1, 37, 32, 32)
    assert rc == -1 and "staging" in text
    rc, text = plan_blob([(30000, 400000)], 3, 37, 32, 32)              # shorter side 30000: 1622 rows x 96 bytes = 152 KB
    assert rc == -1 and "staging" in text
    rc, blob = plan_blob([(20000, 21000)], 3, 37, 32, 32)               # 1082 rows x 96 bytes = 101 KB
    assert rc == -1 and "staging" in blob
    rc, blob = plan_blob([(12000, 12500)], 3, 37, 32, 32)               # 650 rows x 96 bytes = 61 KB: fits at one row per block
    assert rc == 0
    (_, frames) = blob_frames(blob)
    assert frames[0][11] == 1 and frames[0][12] == 32                   # band 1, 32 bands
    for sizes in ([(400000, 8)], [(8, 400000)]):
        rc, blob = plan_blob(sizes, 3, 37, 32, 32)
        assert rc == 0, blob
        hd, frames = blob_frames(blob)
        hs, ws = sizes[0]
        oh, ow = frames[0][3:5]
        assert max(oh, ow) == 1850000 and min(oh, ow) == 37
        want, ksize = axis_coeffs(8, 37)
        off, crop0 = (frames[0][15], frames[0][6]) if ws == 8 else (frames[0][16], frames[0][5])
        xmin, n, kk = blob_table(blob, off, 32, ksize)
        assert [kk[x, :n[x]].tolist() for x in range(32)] == [k for _, _, k in want[crop0:crop0 + 32]]
        assert frames[0][8] - frames[0][7] <= 10          # 32 crop rows at scale 8 / 37: at most ceil(32 * 0.22) + 2 + 1 source rows


# ---- 6. the planner under the sanitizers, as a stand-alone program ---------------------------------------------------------------
def test_planner_standalone_under_sanitizers(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    src = os.path.join(ROOT, "tests", "tools", "resize_plan_check.cpp")
    exe = str(tmp_path / "resize_plan_check")
    flags = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    probe = str(tmp_path / "probe.cpp")
    with open(probe, "w") as f:
        f.write("int main() { return 0; }\n")
    if subprocess.run([gxx] + flags + [probe, "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("g++ has no sanitizer runtime")
    subprocess.run([gxx] + flags + ["-Wall", "-I", os.path.join(ROOT, "pytorchcv_amd", "csrc"), src, "-o", exe], check=True)
    res = subprocess.run([exe], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
