"""Writes tests/golden/jpeg_cases.npz: small JPEG files and the pixels PIL (libjpeg-turbo, the library behind cv2.imread)
decodes from them -- the fixture of tests/test_jpeg_host.py and tests/test_jpeg_gpu.py, which read only this file, never PIL.

    python tools/make_jpeg_golden.py                 # writes the fixture
    python tools/make_jpeg_golden.py --dump DIR      # also writes every case as DIR/<name>.jpg (tools/jpeg_host_check.cpp)

Per case `jpg_<name>` (the file's bytes) and, for the files the decoder takes, `pix_<name>` (PIL's pixels: RGB, or L for a
grey file).  `meta` is JSON: PIL's and libjpeg-turbo's versions and one record per case -- kind ("good", "refused",
"damaged"), size, sampling, restart interval in MCUs, the number of quantisation / Huffman tables and of restart intervals.
Content is generated from a fixed seed.
"""
import argparse
import io
import json
import os

import numpy as np
from PIL import Image, features

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "jpeg_cases.npz")

# name, height, width, PIL subsampling (or "L"), quality, noisy, save options
GOOD = [
    ("444_16x16", 16, 16, "4:4:4", 85, False, {}),
    ("420_16x16_q100", 16, 16, "4:2:0", 100, False, {}),
    ("420_13x17_q100", 13, 17, "4:2:0", 100, False, {}),
    ("420_40x56", 40, 56, "4:2:0", 90, False, {}),
    ("420_33x47_opt", 33, 47, "4:2:0", 75, False, {"optimize": True}),
    ("420_1x1", 1, 1, "4:2:0", 90, False, {}),
    ("420_9x3", 9, 3, "4:2:0", 90, False, {}),
    ("420_9x5", 9, 5, "4:2:0", 90, False, {}),
    ("420_2x40", 2, 40, "4:2:0", 90, False, {}),
    ("420_32x340", 32, 340, "4:2:0", 92, False, {}),
    ("420_64x96_noisy_q100", 64, 96, "4:2:0", 100, True, {}),
    ("420_24x40_rst1", 24, 40, "4:2:0", 85, False, {"restart_marker_blocks": 1}),
    ("420_35x50_rstrow", 35, 50, "4:2:0", 85, False, {"restart_marker_rows": 1}),
    ("422_31x33", 31, 33, "4:2:2", 85, False, {}),
    ("422_8x2", 8, 2, "4:2:2", 85, False, {}),
    ("422_7x4", 7, 4, "4:2:2", 85, False, {}),
    ("grey_19x21", 19, 21, "L", 85, False, {}),
]
SAMPLING = {"4:4:4": [[1, 1]] * 3, "4:2:2": [[2, 1], [1, 1], [1, 1]], "4:2:0": [[2, 2], [1, 1], [1, 1]], "L": [[1, 1]]}


def picture(rng, h, w, noisy):
    y, x = np.mgrid[0:h, 0:w]
    a = np.stack([128 + 100 * np.sin(x / 5.0 + y / 7.0), 128 + 100 * np.cos(x / 3.0 - y / 4.0), (x * 7 + y * 13) % 256], -1)
    a = a + rng.randn(h, w, 3) * (70 if noisy else 6)
    return np.clip(a, 0, 255).astype(np.uint8)


def tables(data):
    """the file's markers, walked independently of lib/datasets/jpeg.py: (quantisation tables, Huffman tables, scan start)"""
    i, nq, nh = 2, 0, 0
    while True:
        m, length = data[i + 1], (data[i + 2] << 8) | data[i + 3]
        if m == 0xDB:
            nq += (length - 2) // 65
        if m == 0xC4:
            j = i + 4
            while j < i + 2 + length:
                j += 17 + sum(data[j + 1:j + 17])
                nh += 1
        i += 2 + length
        if m == 0xDA:
            return nq, nh, i


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dump", default=None, help="directory to write every case to as <name>.jpg")
    args = ap.parse_args()
    rng = np.random.RandomState(20260)
    arrays, cases = {}, []

    def add(name, data, kind, pix=None, **rec):
        arrays["jpg_" + name] = np.frombuffer(data, dtype=np.uint8)
        if pix is not None:
            arrays["pix_" + name] = pix
        cases.append(dict(name=name, kind=kind, **rec))

    for name, h, w, sub, quality, noisy, opts in GOOD:
        im = Image.fromarray(picture(rng, h, w, noisy))
        buf = io.BytesIO()
        if sub == "L":
            im.convert("L").save(buf, "JPEG", quality=quality, **opts)
        else:
            im.save(buf, "JPEG", quality=quality, subsampling=sub, **opts)
        data = buf.getvalue()
        dec = Image.open(io.BytesIO(data))
        assert dec.mode == ("L" if sub == "L" else "RGB")
        pix = np.asarray(dec).copy()
        nq, nh, scan_start = tables(data)
        hs, vs = SAMPLING[sub][0]
        mcu_cols, mcu_rows = -(-w // (8 * hs)), -(-h // (8 * vs))
        ri = opts.get("restart_marker_blocks", 0) or opts.get("restart_marker_rows", 0) * mcu_cols
        add(name, data, "good", pix, height=h, width=w, sampling=SAMPLING[sub], restart_interval=ri, n_quant=nq, n_huff=nh,
            n_segments=-(-mcu_cols * mcu_rows // ri) if ri else 1, scan_start=scan_start)
        if name == "420_40x56":
            scan_len = len(data) - 2 - scan_start
            mid = scan_start + scan_len // 2
            stray = bytearray(data)
            stray[mid:mid + 2] = b"\xff\xd5"
            for dname, d in (("cut_middle", data[:mid]), ("stray_rst", bytes(stray)), ("minus40", data[:-40])):
                add("420_40x56_" + dname, d, "damaged", height=h, width=w, of=name)

    im = Image.fromarray(picture(rng, 24, 24, False))
    buf = io.BytesIO()
    im.save(buf, "JPEG", quality=85, progressive=True)
    add("progressive_24x24", buf.getvalue(), "refused", reason="progressive")
    buf = io.BytesIO()
    Image.fromarray(np.dstack([picture(rng, 16, 16, False), picture(rng, 16, 16, False)[:, :, :1]]), "CMYK").save(buf, "JPEG", quality=85)
    add("cmyk_16x16", buf.getvalue(), "refused", reason="4 components")
    # luma 1x2 ("h1v2"): this PIL writes no sampling outside the supported set, so the frame header of a 4:2:2 file is
    # patched from 2x1 to 1x2.  The parser refuses it on the header alone; the scan is never decoded.
    buf = io.BytesIO()
    im.save(buf, "JPEG", quality=85, subsampling="4:2:2")
    data = bytearray(buf.getvalue())
    sof = data.index(b"\xff\xc0")
    assert data[sof + 11] == 0x21
    data[sof + 11] = 0x12
    add("h1v2_24x24", bytes(data), "refused", reason="sampling factors")

    meta = dict(pil=Image.__version__, libjpeg_turbo=features.version("libjpeg_turbo"), jpeglib=features.version("jpg"), cases=cases)
    arrays["meta"] = np.frombuffer(json.dumps(meta, sort_keys=True).encode(), dtype=np.uint8)
    np.savez_compressed(OUT, **arrays)
    print("wrote %s: %d cases, %d bytes (PIL %s, libjpeg-turbo %s)" % (OUT, len(cases), os.path.getsize(OUT), meta["pil"],
                                                                        meta["libjpeg_turbo"]))
    if args.dump:
        os.makedirs(args.dump, exist_ok=True)
        for c in cases:
            with open(os.path.join(args.dump, c["name"] + ".jpg"), "wb") as f:
                f.write(arrays["jpg_" + c["name"]].tobytes())


if __name__ == "__main__":
    main()
