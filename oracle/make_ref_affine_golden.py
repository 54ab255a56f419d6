"""Commit what the REFERENCE-BUILT AffineNd operator computes, as SHA-256 digests of its outputs.

TEST INFRASTRUCTURE ONLY.  Run on a GPU, with oracle/_ref/libref_affine_nd.so built by oracle/build_ref.py:

    python oracle/make_ref_affine_golden.py [out.json]      # default: tests/golden/ref_affine_nd.json

For every shape of tests/test_ref_affine_gpu.py the seeded inputs (`inputs`) go through the reference's forward and
backward kernels; the fixture holds the digests of the inputs and of both outputs.  A digest pins the fp32 outputs bit for
bit (what the test asserts of vlfb_affine_nd_fwd / _bwd) in 64 bytes instead of the outputs themselves (15 MB).
"""
import ctypes as C
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REF_SO = os.path.join(HERE, "_ref", "libref_affine_nd.so")
OUT = os.path.join(HERE, "..", "tests", "golden", "ref_affine_nd.json")

SHAPES = [(2, 64, 8 * 14 * 14), (1, 256, 4 * 7 * 7), (3, 2048, 1), (2, 3, 5), (1, 1, 4099), (4, 512, 16 * 7 * 7 + 3)]


def key(shape):
    return "x".join(str(d) for d in shape)


def inputs(shape):
    """x (n, c, inner), per-channel scale s and bias b: fp32 CPU tensors from a seeded torch generator"""
    import torch
    n, c, inner = shape
    g = torch.Generator().manual_seed(1234 + n * 7 + c)
    x = torch.randn(n, c, inner, generator=g)
    s = torch.rand(c, generator=g) + 0.5
    b = torch.randn(c, generator=g) * 0.1
    return x, s, b


def digest(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().contiguous().cpu().numpy().tobytes())
    return h.hexdigest()


def main(out):
    import torch
    lib = C.CDLL(REF_SO)
    P, LL = C.c_void_p, C.c_longlong
    lib.ref_affine_nd_fwd.argtypes = [P, P, P, P, LL, LL, LL, P]
    lib.ref_affine_nd_bwd.argtypes = [P, P, P, LL, LL, LL, P]
    lib.ref_affine_nd_fwd.restype = lib.ref_affine_nd_bwd.restype = C.c_int
    stream = torch.cuda.current_stream().cuda_stream
    rec = {"source": "caffe2_customized_ops/video/affine_nd_op.cu of the reference, built by oracle/build_ref.py", "cases": {}}
    for shape in SHAPES:
        n, c, inner = shape
        x, s, b = inputs(shape)
        xd, sd, bd = x.cuda(), s.cuda(), b.cuda()
        y = torch.full_like(xd, float("nan"))
        dx = torch.full_like(xd, float("nan"))
        assert lib.ref_affine_nd_fwd(xd.data_ptr(), sd.data_ptr(), bd.data_ptr(), y.data_ptr(), n, c, inner, stream) == 0
        assert lib.ref_affine_nd_bwd(xd.data_ptr(), sd.data_ptr(), dx.data_ptr(), n, c, inner, stream) == 0
        torch.cuda.synchronize()
        assert not (torch.isnan(y).any() or torch.isnan(dx).any()), shape
        rec["cases"][key(shape)] = {"inputs": digest(x, s, b), "y": digest(y), "dx": digest(dx)}
    with open(out, "w") as fh:
        json.dump(rec, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print("%s: %d cases" % (out, len(rec["cases"])))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else OUT)
