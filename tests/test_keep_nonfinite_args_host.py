"""Argument checks of vlfb_topk_hits_keep and vlfb_lfb_count_nonfinite: VLFB_ERR_ARG with a message, before anything is
launched, so no device is needed (the addresses below are never dereferenced by a refused call)."""
import ctypes as C
import os

import pytest

from vlfb import hip

ERR_ARG = -1                                                # include/vlfb.h VLFB_ERR_ARG
ADDR = 4096                                                 # stands for a non-NULL device address


def refused(name, args, match):
    rc = getattr(hip.lib(), name)(*args)
    msg = hip.lib().vlfb_last_error().decode()
    assert rc == ERR_ARG, (name, rc, msg)
    assert match in msg, (match, msg)


def test_topk_hits_keep_argument_checks():
    if not os.path.exists(hip.LIB_PATH):
        pytest.skip("libvlfb_hip.so not built")
    ks, nk = hip.ks_array((1, 5))

    def args(**kw):
        a = dict(scores=ADDR, dtype=hip.F32, labels=ADDR, rows=2, cols=125, ks=ks, nk=nk, hits=ADDR, table=ADDR, tlab=ADDR,
                 total=7, cursor=ADDR)
        a.update(kw)
        return [a[k] for k in ("scores", "dtype", "labels", "rows", "cols", "ks", "nk", "hits", "table", "tlab", "total",
                               "cursor")] + [None]

    name = "vlfb_topk_hits_keep"
    refused(name, args(table=None), "table")
    refused(name, args(tlab=None), "table_labels")
    refused(name, args(cursor=None), "cursor is required")
    refused(name, args(total=0), "total_rows must be positive")
    refused(name, args(total=-3), "total_rows")
    refused(name, args(hits=None), "hits is required")
    refused(name, args(dtype=9), "unknown dtype")
    refused(name, args(rows=-1), "rows")
    refused(name, args(cols=0), "cols")
    refused(name, args(scores=None), "scores and labels")
    # the ks rule of vlfb_topk_hits: 1..4 host values, each within 1..cols
    refused(name, args(ks=None), "nk")
    refused(name, args(nk=5), "nk")
    refused(name, args(ks=hip.ks_array((1, 126))[0]), "k = 126")
    refused(name, args(ks=hip.ks_array((0, 5))[0]), "k = 0")
    # rows == 0 is a no-op, as in vlfb_topk_hits: nothing launched, nothing read
    assert hip.lib().vlfb_topk_hits_keep(*args(rows=0, scores=None, labels=None)) == 0


def test_lfb_count_nonfinite_argument_checks():
    if not os.path.exists(hip.LIB_PATH):
        pytest.skip("libvlfb_hip.so not built")
    name = "vlfb_lfb_count_nonfinite"
    good = hip.LfbDesc(2, 3, 2, 100, hip.BF16, 0)
    refused(name, [None, ADDR, ADDR, ADDR, None], "descriptor")
    refused(name, [C.byref(hip.LfbDesc(2, 0, 2, 100, hip.BF16, 0)), ADDR, ADDR, ADDR, None], "geometry")
    refused(name, [C.byref(hip.LfbDesc(2, 3, 2, 100, 7, 0)), ADDR, ADDR, ADDR, None], "dtype")
    for i in (1, 2, 3):
        a = [C.byref(good), ADDR, ADDR, ADDR, None]
        a[i] = None
        refused(name, a, "NULL buffer")
