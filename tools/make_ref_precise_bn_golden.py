"""Run the REFERENCE's own precise-BN arithmetic on seeded batch statistics and commit inputs + outputs.

TEST INFRASTRUCTURE ONLY.  Needs the reference checkout:

    python tools/make_ref_precise_bn_golden.py        # writes tests/golden/ref_precise_bn.npz

Called, from where it lies (the Caffe2 stubs of oracle/make_ref_aux_golden.py make the module importable):
  lib/utils/bn_helper.py   BatchNormHelper._clean_and_reset_buffer, _collect_bn_stats (once per iteration),
                           _finalize_bn_stats and _update_bn_stats_gpu, on a helper whose `_bn_layers` the generator sets
The stubbed workspace.FetchBlob reads a dict of float32 `_bn_sm` / `_bn_siv` arrays that the generator refills before
every iteration; workspace.FeedBlob records what the reference feeds as `_bn_rm` / `_bn_riv`.

Per case the file holds `sm` / `siv` as [iterations * NUM_GPUS][sum C] float32 in the order the reference reads them (per
iteration: GPU 0's layers, then GPU 1's), the layer widths, and the fed `rm` / `riv` as [sum C] float32 -- or
"raises": true where the reference's `var > 0` assertion fires (nothing is fed then).
"""
import io
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REF = "/root/reference"
OUT = os.path.join(ROOT, "tests", "golden", "ref_precise_bn.npz")
sys.path.insert(0, ROOT)

ITERS = 3
CASES = [("one_gpu", 1, False, [1, 8, 64, 67, 2051]), ("two_gpus", 2, False, [8, 67, 300]),
         ("constant_channel", 1, True, [8, 67])]
CONSTANT = ("layer1", 5)                                         # (layer, channel) of the constant channel


def main():
    from oracle.make_ref_aux_golden import install_stubs
    config, _ = install_stubs()
    import utils.bn_helper as bn_helper                          # the reference's (install_stubs put its lib/ on the path)
    assert os.path.realpath(bn_helper.__file__).startswith(REF), bn_helper.__file__
    cfg = config.config
    workspace = bn_helper.workspace
    blobs, fed = {}, {}
    workspace.FetchBlob = lambda name: blobs[str(name)]
    workspace.FeedBlob = lambda name, arr: fed.__setitem__(str(name), np.array(arr))

    eps = float(cfg.MODEL.BN_EPSILON)
    rng = np.random.RandomState(20241020)
    arrays, infos = {}, []
    for k, (label, gpus, constant, WIDTHS) in enumerate(CASES):
        names = ["layer%d" % i for i in range(len(WIDTHS))]
        config.cfg_from_list(["NUM_GPUS", str(gpus), "TRAIN.ITER_COMPUTE_PRECISE_BN", str(ITERS)])
        assert cfg.NUM_GPUS == gpus and cfg.ROOT_GPU_ID == 0 and cfg.TRAIN.ITER_COMPUTE_PRECISE_BN == ITERS
        helper = bn_helper.BatchNormHelper()
        helper._bn_layers = list(names)
        helper._clean_and_reset_buffer()
        fed.clear()
        sm_rows, siv_rows = [], []
        for it in range(ITERS):
            blobs.clear()
            for g in range(gpus):
                sm_row, siv_row = [], []
                for name, C in zip(names, WIDTHS):
                    var = np.exp(rng.uniform(np.log(1e-3), np.log(1e2), C))
                    sm = rng.randn(C).astype(np.float32) * np.float32(2.0)
                    siv = (np.float32(1) / np.sqrt(var.astype(np.float32) + np.float32(eps))).astype(np.float32)
                    if constant and name == CONSTANT[0]:
                        # a channel whose every element is 0.5: zero batch variance, siv = 1 / sqrt(eps) as fp32 computes it
                        sm[CONSTANT[1]] = np.float32(0.5)
                        siv[CONSTANT[1]] = np.float32(1) / np.sqrt(np.float32(0) + np.float32(eps))
                        var[CONSTANT[1]] = 1.0
                    # no subnormal intermediate anywhere in the chain
                    assert (var >= 1e-3).all() and (var <= 1e2).all()
                    assert siv.dtype == np.float32 and sm.dtype == np.float32
                    blobs["gpu_%d/%s_bn_sm" % (g, name)] = sm
                    blobs["gpu_%d/%s_bn_siv" % (g, name)] = siv
                    sm_row.append(sm)
                    siv_row.append(siv)
                sm_rows.append(np.concatenate(sm_row))
                siv_rows.append(np.concatenate(siv_row))
            helper._collect_bn_stats()
        raised = False
        try:
            helper._finalize_bn_stats()
        except AssertionError:
            raised = True
        assert raised == constant, (label, raised)
        arrays["case%d_sm" % k], arrays["case%d_siv" % k] = np.stack(sm_rows), np.stack(siv_rows)
        if not raised:
            helper._update_bn_stats_gpu()
            assert sorted(fed) == sorted("gpu_%d/%s_bn_%s" % (g, n, s) for g in range(gpus) for n in names for s in ("rm", "riv"))
            for g in range(1, gpus):                             # every GPU is fed the same arrays
                for n in names:
                    for s in ("rm", "riv"):
                        assert np.array_equal(fed["gpu_%d/%s_bn_%s" % (g, n, s)], fed["gpu_0/%s_bn_%s" % (n, s)])
            rm = [fed["gpu_0/%s_bn_rm" % n] for n in names]
            riv = [fed["gpu_0/%s_bn_riv" % n] for n in names]
            assert all(a.dtype == np.float32 for a in rm + riv)
            assert [a.shape for a in rm] == [(C,) for C in WIDTHS] == [a.shape for a in riv]
            arrays["case%d_rm" % k], arrays["case%d_riv" % k] = np.concatenate(rm), np.concatenate(riv)
            assert (arrays["case%d_riv" % k] > 0).all()
        else:
            assert not fed
        infos.append({"label": label, "num_gpus": gpus, "iters": ITERS, "normalize": ITERS * gpus, "widths": WIDTHS,
                      "raises": raised, "constant": list(CONSTANT) if constant else None})
    meta = {"generator": "tools/make_ref_precise_bn_golden.py", "numpy": np.__version__, "eps": eps, "cases": infos}
    arrays["meta"] = np.frombuffer(json.dumps(meta, sort_keys=True).encode(), dtype=np.uint8)
    buf = io.BytesIO()
    np.savez_compressed(buf, **arrays)
    with open(OUT, "wb") as f:
        f.write(buf.getvalue())
    print("wrote %s: %d arrays, %d bytes" % (os.path.normpath(OUT), len(arrays), os.path.getsize(OUT)))
    print(json.dumps(infos, sort_keys=True))


if __name__ == "__main__":
    main()
