"""The JPEG fixture (tests/golden/jpeg_cases.npz, written by tools/make_jpeg_golden.py) as the host and the GPU tests read it:
the files, PIL's pixels as uint8 BGR (grey replicated), and items packed for the two decode entry points."""
import ctypes as C
import functools
import json
import os

import numpy as np

from datasets import jpeg
from vlfb import hip

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpeg_cases.npz")
GUARD = 64                                             # guard bytes on both sides of a destination


@functools.lru_cache(maxsize=None)
def fixture():
    """-> (meta, {name: file bytes}, {name: expected (H, W, 3) uint8 BGR}); loaded once, shared and never modified"""
    z = np.load(PATH)
    meta = json.loads(z["meta"].tobytes().decode())
    files = {c["name"]: z["jpg_" + c["name"]].tobytes() for c in meta["cases"]}
    want = {}
    for c in meta["cases"]:
        if c["kind"] == "good":
            pix = z["pix_" + c["name"]]
            bgr = np.repeat(pix[:, :, None], 3, axis=2) if pix.ndim == 2 else pix[:, :, ::-1]
            want[c["name"]] = np.ascontiguousarray(bgr)
            want[c["name"]].setflags(write=False)
    return meta, files, want


def cases(kind):
    return [c for c in fixture()[0]["cases"] if c["kind"] == kind]


def names(kind):
    return [c["name"] for c in cases(kind)]


def host_item(data):
    """-> (item with HOST addresses for vlfb_jpeg_decode_host, JpegInfo, the arrays the addresses point into)"""
    info = jpeg.parse(data)
    item = info.fill(hip.JpegItem())
    scan = np.frombuffer(data, dtype=np.uint8)[info.scan_start:info.scan_end].copy()
    seg = np.asarray(info.segment_offsets, dtype=np.uint32)
    item.scan, item.seg_offsets = (scan.ctypes.data if scan.size else seg.ctypes.data), seg.ctypes.data
    return item, info, (scan, seg)


def decode_host(data):
    """-> (guarded buffer, its (H, W, 3) window, status) of vlfb_jpeg_decode_host; the guard bytes are 0xA5"""
    item, info, keep = host_item(data)
    n = info.height * info.width * 3
    buf = np.full(n + 2 * GUARD, 0xA5, dtype=np.uint8)
    status = C.c_int32(-1)
    rc = hip.lib().vlfb_jpeg_decode_host(C.byref(item), buf.ctypes.data + GUARD, C.byref(status))
    if rc != 0:
        raise hip.VlfbError(hip.lib().vlfb_last_error().decode())
    return buf, buf[GUARD:GUARD + n].reshape(info.height, info.width, 3), status.value
