"""Argument checks of vlfb_bn_precise_accumulate / _finalize / _update: VLFB_ERR_ARG with a message, before anything is
launched, so no device is needed (the addresses below are never dereferenced by a refused call)."""
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


def test_bn_precise_argument_checks():
    if not os.path.exists(hip.LIB_PATH):
        pytest.skip("libvlfb_hip.so not built")
    acc, fin, upd = "vlfb_bn_precise_accumulate", "vlfb_bn_precise_finalize", "vlfb_bn_precise_update"
    # accumulate(table, layers, eps, sum_mean, sum_mean2, stream)
    refused(acc, [ADDR, 0, 1e-5, ADDR, ADDR, None], "layers")
    refused(acc, [ADDR, -2, 1e-5, ADDR, ADDR, None], "layers")
    refused(acc, [None, 3, 1e-5, ADDR, ADDR, None], "table")
    refused(acc, [ADDR, 3, 1e-5, None, ADDR, None], "NULL accumulator")
    refused(acc, [ADDR, 3, 1e-5, ADDR, None, None], "NULL accumulator")
    # finalize(table, layers, normalize, sum_mean, sum_mean2, bad, stream)
    refused(fin, [ADDR, 0, 3, ADDR, ADDR, ADDR, None], "layers")
    refused(fin, [ADDR, 3, 0, ADDR, ADDR, ADDR, None], "normalize")
    refused(fin, [ADDR, 3, -1, ADDR, ADDR, ADDR, None], "normalize")
    refused(fin, [None, 3, 3, ADDR, ADDR, ADDR, None], "table")
    refused(fin, [ADDR, 3, 3, None, ADDR, ADDR, None], "NULL accumulator")
    refused(fin, [ADDR, 3, 3, ADDR, None, ADDR, None], "NULL accumulator")
    refused(fin, [ADDR, 3, 3, ADDR, ADDR, None, None], "bad is NULL")
    # update(table, layers, mean, var, stream)
    refused(upd, [ADDR, 0, ADDR, ADDR, None], "layers")
    refused(upd, [None, 3, ADDR, ADDR, None], "table")
    refused(upd, [ADDR, 3, None, ADDR, None], "NULL statistics")
    refused(upd, [ADDR, 3, ADDR, None, None], "NULL statistics")


def test_bn_layer_record_matches_the_header():
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "vlfb.h")).read()
    assert "#define VLFB_BN_LAYER_BYTES %d" % hip.BN_LAYER_BYTES in text
    assert [n for n, _ in hip.BnLayer._fields_] == ["save_mean", "save_inv_std", "running_mean", "running_var", "offset", "C",
                                                     "reserved"]
