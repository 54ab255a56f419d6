"""Engine.FUSE_POOL2 (Engine._plan_pool_fusion): pool2 inside the epilogue of res2_2_branch2c on the "mix" path changes which
launches a pass issues and NOTHING it computes.  ava_r50_lfb_nl at test_model_gpu.SMALL, switch on against switch off:
every checked blob -- the un-pooled res2_2_branch2c_bn included, which no launch of a fused pass writes and fetch()
re-materialises -- the loss, every parameter gradient and every parameter after recorded and replayed train steps must be
bit-identical; a forward pass after a fetch must be unaffected by the re-materialisation; and the fused pass must not call
vlfb_maxpool_fwd for pool2."""
import numpy as np
import pytest
import torch

from test_model_gpu import CHECK_BLOBS, SMALL, build

pytestmark = pytest.mark.gpu

PRESET = "ava_r50_lfb_nl"


def teardown_module(module):
    # hand the cached blocks back: later test files measure peaks of the caching allocator
    import gc
    gc.collect()
    torch.cuda.empty_cache()


def _test_engine():
    """the test split of the model at the size of SMALL (as test_model_gpu.test_test_mode_forward_and_lfb_inference)"""
    import collections
    from vlfb.presets import load_preset
    from core.config import config as cfg
    from models.model_builder_video import ModelBuilder
    from vlfb.engine import Engine
    from oracle import model as om
    load_preset(PRESET, ["NUM_GPUS", 1, "TEST.BATCH_SIZE", 2, "TRAIN.VIDEO_LENGTH", 16, "TEST.VIDEO_LENGTH", 16,
                         "TEST.CROP_SIZE", 64, "TRAIN.CROP_SIZE", 64])
    inputs = om.synth_inputs(cfg, 2, "test", seed=3, rois_per_clip=[1, 2], crop=64, frames=16)
    params = om.synth_params(cfg, seed=3)
    model = ModelBuilder(train=False, split="test", name="test")
    model.build_model(suffix="_test")
    eng = Engine(model, "mix")
    names = list(model.input_blob_names)
    eng.plan(collections.OrderedDict((n, inputs[n[:-5]].shape) for n in names))
    eng.feed_params({k: v for k, v in params.items() if k in eng.param_views})
    for n in names:
        eng.feed(n, inputs[n[:-5]])
    return eng


def _engine(monkeypatch, fuse, train):
    from vlfb.engine import Engine, PoolStep
    monkeypatch.setattr(Engine, "FUSE_POOL2", fuse)
    if train:
        cfg, model, eng, inputs, params, seed_fn = build(PRESET, "mix", SMALL, train=True)
    else:
        eng = _test_engine()
    fused = [st.name() for st in eng.steps if isinstance(st, PoolStep) and st.fused_into is not None]
    assert fused == (["maxpool:pool2"] if fuse else []), fused
    if fuse:
        conv = [st for st in eng.steps if getattr(st, "fused_pool", None) is not None]
        assert [st.name() for st in conv] == ["conv:res2_2_branch2c_bn"]
    return eng


def _names(eng):
    return [n for n in CHECK_BLOBS if n in eng.env]


def _pool2(eng):
    from vlfb.engine import PoolStep
    return [st for st in eng.steps if isinstance(st, PoolStep) and st.name() == "maxpool:pool2"][0]


def _train_record(monkeypatch, fuse):
    eng = _engine(monkeypatch, fuse, True)
    out = {}
    eng.forward()
    eng.backward()
    torch.cuda.synchronize()
    ps = _pool2(eng)
    pooled0, argmax0 = ps.out.storage().clone(), ps.argmax.clone()
    out["blobs"] = {n: eng.fetch(n) for n in _names(eng)}
    out["loss"] = eng.fetch("loss").copy()
    out["grads"] = {n: eng.fetch_grad(n) for n in eng.trainable}
    # the fetches above re-materialised the un-pooled blob: the pooled planes and the arg-max are what the pass left ...
    assert torch.equal(ps.out.storage(), pooled0) and torch.equal(ps.argmax, argmax0)
    # ... and a second pass is the first one again
    ps.out.storage().fill_(float("nan"))
    ps.argmax.fill_(0xFF)
    eng.forward()
    torch.cuda.synchronize()
    assert torch.equal(ps.out.storage(), pooled0) and torch.equal(ps.argmax, argmax0)
    for n, v in out["blobs"].items():
        assert np.array_equal(eng.fetch(n), v), "%s differs on the second forward pass" % n
    eng.backward()
    # an eager step, the step that records the call list, and a replayed one
    for _ in range(3):
        eng.train_step(0.01)
    torch.cuda.synchronize()
    assert eng._trace is not None
    calls = [name for _, _, name in eng._trace]
    out["pool_calls"] = calls.count("vlfb_maxpool_fwd")
    out["fused_calls"] = calls.count("vlfb_conv_run_maxpool")
    out["params"] = {n: eng.fetch_param(n) for n in eng.trainable}
    out["loss3"] = eng.fetch("loss").copy()
    return out


def test_train_pass_and_recorded_steps_are_bit_identical_with_pool2_fused(monkeypatch):
    on = _train_record(monkeypatch, True)
    off = _train_record(monkeypatch, False)
    assert "res2_2_branch2c_bn" in on["blobs"] and "pool2" in on["blobs"]
    for n in off["blobs"]:
        assert np.array_equal(on["blobs"][n], off["blobs"][n]), "blob %s" % n
    assert np.array_equal(on["loss"], off["loss"])
    for n in off["grads"]:
        assert np.array_equal(on["grads"][n], off["grads"][n]), "gradient of %s" % n
    for n in off["params"]:
        assert np.array_equal(on["params"][n], off["params"][n]), "parameter %s after three steps" % n
    assert np.array_equal(on["loss3"], off["loss3"])
    # the recorded step: one pool launch fewer, the fused launch in its place
    assert on["fused_calls"] == 1 and off["fused_calls"] == 0
    assert on["pool_calls"] == off["pool_calls"] - 1


def test_test_mode_forward_is_bit_identical_with_pool2_fused(monkeypatch):
    got = {}
    for fuse in (True, False):
        eng = _engine(monkeypatch, fuse, False)
        assert _pool2(eng).argmax is None            # inference: the fused launch gets no arg-max pointer
        eng.forward()
        torch.cuda.synchronize()
        got[fuse] = {n: eng.fetch(n) for n in _names(eng)}
        eng.forward()                                # (behind the re-materialising fetches)
        torch.cuda.synchronize()
        for n, v in got[fuse].items():
            assert np.array_equal(eng.fetch(n), v), n
    assert "res2_2_branch2c_bn" in got[True] and "prob" in got[True]
    for n in got[False]:
        assert np.array_equal(got[True][n], got[False][n]), "blob %s" % n
