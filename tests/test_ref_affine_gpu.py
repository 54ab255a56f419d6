"""AffineNd pinned against REFERENCE-BUILT code: oracle/_ref/libref_affine_nd.so is the reference's own
caffe2_customized_ops/video/affine_nd_op.cu (kernels :31-58 and both RunOnDevice bodies :61-107)
compiled unmodified by oracle/build_ref.py; what it computes on the seeded inputs of every shape below is committed as
SHA-256 digests of its outputs (tests/golden/ref_affine_nd.json, oracle/make_ref_affine_golden.py).  Checked here:
  * vlfb_affine_nd_fwd / vlfb_affine_nd_bwd (the drop-in operator of include/vlfb.h) == the reference
    operator, BIT-EXACT (fp32, same fma contraction): equal digests,
  * the CPU oracle's `_affine` restatement == the reference operator to 1 ulp (torch-CPU rounds the
    product before the add, the GPU build fuses it), and its fp64 form to fp32 round-off.
The library is test infrastructure: only tests/ and the fixture generator load it."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from oracle.make_ref_affine_golden import SHAPES, digest, inputs, key

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_SO = os.path.join(ROOT, "oracle", "_ref", "libref_affine_nd.so")
GOLDEN = os.path.join(ROOT, "tests", "golden", "ref_affine_nd.json")


def _ref():
    assert os.path.exists(REF_SO), ("%s is missing: run `python oracle/build_ref.py` where /root/reference is "
                                    "mounted (build() does) -- the prebuilt library travels to the GPU box" % REF_SO)
    lib = C.CDLL(REF_SO)
    P, LL = C.c_void_p, C.c_longlong
    lib.ref_affine_nd_fwd.argtypes = [P, P, P, P, LL, LL, LL, P]
    lib.ref_affine_nd_bwd.argtypes = [P, P, P, LL, LL, LL, P]
    lib.ref_affine_nd_fwd.restype = lib.ref_affine_nd_bwd.restype = C.c_int
    return lib


def test_reference_library_exports_both_entry_points():
    """CPU-side: the reference-built checker exists and exports what the GPU tests bind (no compute)"""
    if not os.path.exists(REF_SO) and not os.path.exists("/root/reference"):
        pytest.skip("neither the prebuilt library nor /root/reference is available here")
    lib = _ref()
    assert lib.ref_affine_nd_fwd and lib.ref_affine_nd_bwd


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES)
def test_affine_nd_matches_the_reference_built_operator_bit_exactly(shape):
    from vlfb import hip
    from oracle import model as om
    n, c, inner = shape
    x, s, b = inputs(shape)
    with open(GOLDEN) as fh:
        want = json.load(fh)["cases"][key(shape)]
    assert digest(x, s, b) == want["inputs"], "the seeded inputs differ from those the fixture was made from"
    xd, sd, bd = x.cuda(), s.cuda(), b.cuda()
    y = torch.full_like(xd, float("nan"))
    hip.call("vlfb_affine_nd_fwd", hip.ptr(xd), hip.ptr(sd), hip.ptr(bd), hip.ptr(y), n, c, inner)
    dx = torch.full_like(xd, float("nan"))
    hip.call("vlfb_affine_nd_bwd", hip.ptr(xd), hip.ptr(sd), hip.ptr(dx), n, c, inner)
    torch.cuda.synchronize()
    assert digest(y) == want["y"], "vlfb_affine_nd_fwd differs from the reference-built AffineNdOp"
    assert digest(dx) == want["dx"], "vlfb_affine_nd_bwd differs from the reference-built AffineNdGradientOp"
    y_ref = y         # (bit for bit the reference operator's output, by the digest)
    # the oracle's restatement (what every model-level parity test leans on)
    P = {"p_s": s, "p_b": b}
    y_or = om._affine(x.view(n, c, inner, 1, 1), P, "p").view(n, c, inner)
    ulp = np.spacing(np.abs(y_ref.cpu().numpy()).astype(np.float32)) + np.spacing(np.abs(b.numpy()).astype(np.float32))[None, :, None]
    assert np.all(np.abs(y_or.numpy() - y_ref.cpu().numpy()) <= ulp), "fp32 oracle _affine is more than 1 ulp away"
    P64 = {"p_s": s.double(), "p_b": b.double()}
    y64 = om._affine(x.double().view(n, c, inner, 1, 1), P64, "p").view(n, c, inner)
    err = (y64 - y_ref.cpu().double()).abs().max() / y64.abs().max()
    assert float(err) < 1e-6
