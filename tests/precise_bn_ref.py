"""The precise-BN arithmetic as a float32 numpy chain (lib/utils/bn_helper.py:163-198 transcribed), and the reference-executed
fixture tests/golden/ref_precise_bn.npz (tools/make_ref_precise_bn_golden.py).  tests/test_precise_bn_host.py proves the
chain against the fixture bit for bit; the GPU tests compare the kernels and vlfb.precise_bn.PreciseBN against the chain."""
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_precise_bn.npz")


def load_golden():
    z = np.load(GOLDEN)
    meta = json.loads(bytes(z["meta"]).decode())
    return meta, {k: z[k] for k in z.files if k != "meta"}


def accumulate(rows_sm, rows_siv, eps):
    """sums over the rows (one per iteration and GPU, in the reference's order) of the batch mean and of the batch mean of
    x^2; every operation in float32, none fused"""
    f = np.float32
    sum_mean = np.zeros(rows_sm.shape[1], f)
    sum_mean2 = np.zeros(rows_sm.shape[1], f)
    for sm, siv in zip(rows_sm.astype(f), rows_siv.astype(f)):
        r = f(1) / siv
        var = r * r - f(eps)
        m2 = var + sm * sm
        sum_mean = sum_mean + sm
        sum_mean2 = sum_mean2 + m2
    assert sum_mean.dtype == f and sum_mean2.dtype == f
    return sum_mean, sum_mean2


def finalize(sum_mean, sum_mean2, normalize):
    """(mean, var), float32; no assertion"""
    f = np.float32
    mean = sum_mean / f(normalize)
    m2 = sum_mean2 / f(normalize)
    var = m2 - mean * mean
    assert mean.dtype == f and var.dtype == f
    return mean, var


def chain(rows_sm, rows_siv, eps, normalize):
    """what the reference feeds as `_bn_rm` / `_bn_riv`; AssertionError where its `var > 0` assertion fires"""
    mean, var = finalize(*accumulate(rows_sm, rows_siv, eps), normalize=normalize)
    assert (var > 0).all(), "var < 0"
    return mean, var
