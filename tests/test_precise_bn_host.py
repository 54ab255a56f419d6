"""The numpy float32 chain of tests/precise_bn_ref.py IS the reference's precise-BN arithmetic: it reproduces what the
reference's own bn_helper fed as `_bn_rm` / `_bn_riv` (tests/golden/ref_precise_bn.npz) bit for bit, and raises where the
reference's assertion fired.  The GPU tests compare against this chain."""
import numpy as np
import pytest

import precise_bn_ref as ref


def test_fixture_holds_the_cases():
    meta, arrays = ref.load_golden()
    cases = {c["label"]: c for c in meta["cases"]}
    assert cases["one_gpu"]["widths"] == [1, 8, 64, 67, 2051] and cases["one_gpu"]["iters"] == 3
    assert cases["two_gpus"]["num_gpus"] == 2 and cases["two_gpus"]["normalize"] == 6
    assert cases["constant_channel"]["raises"] is True
    for k, c in enumerate(meta["cases"]):
        rows = c["iters"] * c["num_gpus"]
        assert arrays["case%d_sm" % k].shape == arrays["case%d_siv" % k].shape == (rows, sum(c["widths"]))
        assert arrays["case%d_sm" % k].dtype == arrays["case%d_siv" % k].dtype == np.float32
        if not c["raises"]:
            assert arrays["case%d_rm" % k].dtype == arrays["case%d_riv" % k].dtype == np.float32


def test_numpy_chain_reproduces_the_reference_bit_for_bit():
    meta, arrays = ref.load_golden()
    done = 0
    for k, c in enumerate(meta["cases"]):
        if c["raises"]:
            continue
        mean, var = ref.chain(arrays["case%d_sm" % k], arrays["case%d_siv" % k], meta["eps"], c["normalize"])
        assert mean.tobytes() == arrays["case%d_rm" % k].tobytes(), c["label"]
        assert var.tobytes() == arrays["case%d_riv" % k].tobytes(), c["label"]
        done += 1
    assert done == 2


def test_numpy_chain_raises_on_the_constant_channel():
    meta, arrays = ref.load_golden()
    (k, c), = [(k, c) for k, c in enumerate(meta["cases"]) if c["raises"]]
    with pytest.raises(AssertionError):
        ref.chain(arrays["case%d_sm" % k], arrays["case%d_siv" % k], meta["eps"], c["normalize"])
    # exactly one channel, the constant one
    mean, var = ref.finalize(*ref.accumulate(arrays["case%d_sm" % k], arrays["case%d_siv" % k], meta["eps"]), normalize=c["normalize"])
    layer, ch = c["constant"]
    at = sum(c["widths"][:int(layer[len("layer"):])]) + ch
    assert list(np.nonzero(~(var > 0))[0]) == [at]
