"""What the host and the GPU tests of the lane-parallel JPEG decode share: the routing rule as include/vlfb.h states it, the
host checker vlfb_jpeg_decode_host_par behind guard bytes, and the seeded corruptions of two fixture files."""
import ctypes as C
import functools

import numpy as np

import jpeg_cases as jc
from vlfb import hip

DEFAULT_SUBSEQ = 256                                   # include/vlfb.h: subseq_bytes 0
MAX_SCAN = 128 * 1024
STATUS_BITS = hip.JPEG_TRUNCATED | hip.JPEG_BAD_CODE | hip.JPEG_BAD_RESTART
CORRUPTED = ("420_64x96_noisy_q100", "420_32x340")
N_VARIANTS = 200


def is_parallel(info, subseq):
    """vlfb_jpeg_item_is_parallel: no restart interval, one segment, two subsequences or more, at most 128 KiB"""
    subseq = subseq or DEFAULT_SUBSEQ
    return info.restart_interval == 0 and len(info.segment_offsets) == 1 and 2 * subseq <= info.scan_bytes <= MAX_SCAN


def chunks(info, lanes, subseq):
    return -(-info.scan_bytes // (lanes * (subseq or DEFAULT_SUBSEQ)))


def decode(item, info, lanes=None, subseq=0, stats=True):
    """-> (guarded buffer, its (H, W, 3) window, status, stats or None) of vlfb_jpeg_decode_host (lanes None) or
    vlfb_jpeg_decode_host_par on an item with host addresses; the guard bytes are 0xA5"""
    n = info.height * info.width * 3
    buf = np.full(n + 2 * jc.GUARD, 0xA5, dtype=np.uint8)
    status = C.c_int32(-1)
    st = (C.c_int32 * 4)(-1, -1, -1, -1) if stats else None
    if lanes is None:
        rc, st = hip.lib().vlfb_jpeg_decode_host(C.byref(item), buf.ctypes.data + jc.GUARD, C.byref(status)), None
    else:
        rc = hip.lib().vlfb_jpeg_decode_host_par(C.byref(item), buf.ctypes.data + jc.GUARD, C.byref(status), lanes, subseq, st)
    if rc != 0:
        raise hip.VlfbError(hip.lib().vlfb_last_error().decode())
    return buf, buf[jc.GUARD:jc.GUARD + n].reshape(info.height, info.width, 3), status.value, (list(st) if st is not None else None)


@functools.lru_cache(maxsize=None)
def variants():
    """-> ((file name, ((offset in the scan, byte), ...)), ...): N_VARIANTS corruptions of the two CORRUPTED files, each 1..3
    scan bytes overwritten with 0xFF, 0x00 or a random byte; fixed seed.  The header is left alone (the item is the good
    file's: one segment), so a 0xFF written here is a marker both decoders meet in the middle of their data."""
    _, files, _ = jc.fixture()
    rng = np.random.RandomState(20261021)
    out = []
    for v in range(N_VARIANTS):
        name = CORRUPTED[v % 2]
        _, info, _ = jc.host_item(files[name])
        edits = []
        for _ in range(rng.randint(1, 4)):
            kind = rng.randint(0, 4)
            byte = 0xFF if kind == 0 else (0x00 if kind == 1 else int(rng.randint(0, 256)))
            edits.append((int(rng.randint(0, info.scan_bytes)), byte))
        out.append((name, tuple(edits)))
    return tuple(out)


def variant_item(v):
    """-> (item with host addresses, JpegInfo, the arrays it points into) of variants()[v]"""
    _, files, _ = jc.fixture()
    name, edits = variants()[v]
    item, info, (scan, seg) = jc.host_item(files[name])
    for off, byte in edits:
        scan[off] = byte
    return item, info, (scan, seg)


@functools.lru_cache(maxsize=None)
def variant_results():
    """every variant through the serial checker and through the parallel one at (64, 16) and (256, 64), once for all tests:
    -> [(serial pixels, serial status, [(parallel pixels, status, stats), ...])]"""
    out = []
    for v in range(N_VARIANTS):
        item, info, keep = variant_item(v)
        _, ref, ref_status, _ = decode(item, info)
        par = []
        for lanes, subseq in ((64, 16), (256, 64)):
            buf, got, status, stats = decode(item, info, lanes, subseq)
            assert (buf[:jc.GUARD] == 0xA5).all() and (buf[-jc.GUARD:] == 0xA5).all()
            par.append((got.copy(), status, stats))
        out.append((ref.copy(), ref_status, par))
    return out
