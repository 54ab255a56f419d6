"""Precise BN on the device: vlfb_bn_precise_accumulate / _finalize / _update (csrc/vlfb_bn_stats.hip) against the
reference-executed fixture and the float32 numpy chain that test_precise_bn_host.py proves against it -- bit for bit --
and vlfb.precise_bn.PreciseBN through an R50 SpatialBN engine."""
import collections

import numpy as np
import pytest
import torch

import precise_bn_ref as ref
from gpu_util import dev

pytestmark = pytest.mark.gpu

GUARD = 7                                                   # NaN elements either side of every buffer a kernel writes


class Layers(object):
    """a layer table over `widths` with NaN guards around the packed accumulators and around every running blob"""

    def __init__(self, widths, seed=0):
        from vlfb import hip
        self.hip = hip
        self.widths = [int(c) for c in widths]
        self.total = sum(self.widths)
        gen = torch.Generator().manual_seed(seed)
        nan = float("nan")
        self.sm = [torch.zeros(c, device=dev()) for c in self.widths]
        self.siv = [torch.ones(c, device=dev()) for c in self.widths]
        self.rm_buf = [torch.full((c + 2 * GUARD,), nan, device=dev()) for c in self.widths]
        self.rv_buf = [torch.full((c + 2 * GUARD,), nan, device=dev()) for c in self.widths]
        self.rm = [b[GUARD:GUARD + c] for b, c in zip(self.rm_buf, self.widths)]
        self.rv = [b[GUARD:GUARD + c] for b, c in zip(self.rv_buf, self.widths)]
        for t in self.rm + self.rv:                         # what the blobs hold before an update
            t.copy_(torch.rand(t.numel(), generator=gen) + 0.25)
        self.before = [t.clone() for t in self.rm + self.rv]
        self.acc = torch.full((2, self.total + 2 * GUARD), nan, device=dev())
        self.sum_mean, self.sum_mean2 = self.acc[0, GUARD:GUARD + self.total], self.acc[1, GUARD:GUARD + self.total]
        self.sum_mean.zero_()
        self.sum_mean2.zero_()
        self.bad = torch.full((3,), -77, device=dev(), dtype=torch.int32)
        self.table, total = hip.bn_layer_table(list(zip(self.sm, self.siv, self.rm, self.rv, self.widths)), dev())
        assert total == self.total

    def load(self, row_sm, row_siv):
        off = 0
        for sm, siv, c in zip(self.sm, self.siv, self.widths):
            sm.copy_(torch.from_numpy(np.ascontiguousarray(row_sm[off:off + c])))
            siv.copy_(torch.from_numpy(np.ascontiguousarray(row_siv[off:off + c])))
            off += c

    def accumulate(self, eps):
        hip = self.hip
        hip.call("vlfb_bn_precise_accumulate", hip.ptr(self.table), len(self.widths), eps, hip.ptr(self.sum_mean),
                 hip.ptr(self.sum_mean2))

    def finalize(self, normalize):
        hip = self.hip
        hip.call("vlfb_bn_precise_finalize", hip.ptr(self.table), len(self.widths), normalize, hip.ptr(self.sum_mean),
                 hip.ptr(self.sum_mean2), hip.ptr(self.bad) + 4)
        bad = self.bad.cpu().tolist()
        assert bad[0] == -77 and bad[2] == -77              # one int32 written
        return bad[1]

    def update(self):
        hip = self.hip
        hip.call("vlfb_bn_precise_update", hip.ptr(self.table), len(self.widths), hip.ptr(self.sum_mean), hip.ptr(self.sum_mean2))

    def running(self):
        return torch.cat(self.rm).cpu(), torch.cat(self.rv).cpu()

    def unchanged(self):
        return all(torch.equal(a, b) for a, b in zip(self.rm + self.rv, self.before))

    def guards_intact(self):
        ok = bool(torch.isnan(self.acc[:, :GUARD]).all()) and bool(torch.isnan(self.acc[:, GUARD + self.total:]).all())
        for b in self.rm_buf + self.rv_buf:
            ok = ok and bool(torch.isnan(b[:GUARD]).all()) and bool(torch.isnan(b[-GUARD:]).all())
        return ok


def run_case(widths, rows_sm, rows_siv, eps, normalize):
    L = Layers(widths)
    for sm, siv in zip(rows_sm, rows_siv):
        L.load(sm, siv)
        L.accumulate(eps)
    return L, L.finalize(normalize)


def test_kernels_reproduce_the_reference_bit_for_bit():
    meta, arrays = ref.load_golden()
    done = 0
    for k, c in enumerate(meta["cases"]):
        if c["raises"]:
            continue
        L, bad = run_case(c["widths"], arrays["case%d_sm" % k], arrays["case%d_siv" % k], meta["eps"], c["normalize"])
        assert bad == 0, c["label"]
        assert L.unchanged(), "finalize must not touch the running statistics"
        L.update()
        rm, rv = L.running()
        assert torch.equal(rm, torch.from_numpy(arrays["case%d_rm" % k])), c["label"]
        assert torch.equal(rv, torch.from_numpy(arrays["case%d_riv" % k])), c["label"]
        assert L.guards_intact(), c["label"]
        L.update()                                          # "BN of iter computed. Update to GPU only."
        rm2, rv2 = L.running()
        assert torch.equal(rm2, rm) and torch.equal(rv2, rv) and L.guards_intact()
        done += 1
    assert done == 2


def test_constant_channel_is_counted_and_nothing_is_written():
    meta, arrays = ref.load_golden()
    (k, c), = [(k, c) for k, c in enumerate(meta["cases"]) if c["raises"]]
    L, bad = run_case(c["widths"], arrays["case%d_sm" % k], arrays["case%d_siv" % k], meta["eps"], c["normalize"])
    assert bad == 1
    assert L.unchanged() and L.guards_intact()
    mean, var = ref.finalize(*ref.accumulate(arrays["case%d_sm" % k], arrays["case%d_siv" % k], meta["eps"]), normalize=c["normalize"])
    assert torch.equal(L.sum_mean.cpu(), torch.from_numpy(mean)) and torch.equal(L.sum_mean2.cpu(), torch.from_numpy(var))
    # NaN statistics count as bad too
    sm, siv = arrays["case%d_sm" % k].copy(), arrays["case%d_siv" % k].copy()
    sm[1, 0] = np.nan
    siv[2, 3] = np.nan
    L, bad = run_case(c["widths"], sm, siv, meta["eps"], c["normalize"])
    assert bad == 3 and L.unchanged()


def test_seventy_layers_against_the_numpy_chain():
    """more layers than one workgroup walks, widths 1..300 either side of the block size"""
    rng = np.random.RandomState(7)
    widths = [int(c) for c in rng.randint(1, 301, 70)]
    widths[3], widths[40] = 256, 257
    total, iters, eps = sum(widths), 4, 1e-5
    var = np.exp(rng.uniform(np.log(1e-3), np.log(1e2), (iters, total)))
    rows_sm = (rng.randn(iters, total) * 2).astype(np.float32)
    rows_siv = (np.float32(1) / np.sqrt(var.astype(np.float32) + np.float32(eps))).astype(np.float32)
    L, bad = run_case(widths, rows_sm, rows_siv, eps, iters)
    mean, var = ref.chain(rows_sm, rows_siv, eps, iters)
    assert bad == 0
    L.update()
    rm, rv = L.running()
    assert torch.equal(rm, torch.from_numpy(mean)) and torch.equal(rv, torch.from_numpy(var))
    assert L.guards_intact()


# ---- through an engine ---------------------------------------------------------------------------------------------------
BN = ["MODEL.USE_AFFINE", False, "NONLOCAL.USE_BN", True, "NONLOCAL.USE_AFFINE", False, "MODEL.DILATIONS_AFTER_CONV5", False]
SHAPES = ["NUM_GPUS", 1, "TRAIN.BATCH_SIZE", 2, "TRAIN.VIDEO_LENGTH", 8, "TRAIN.CROP_SIZE", 64,
          "TEST.BATCH_SIZE", 2, "TEST.VIDEO_LENGTH", 8, "TEST.CROP_SIZE", 64]


class ListLoader(object):
    """the loader interface PreciseBN uses, over a fixed list of synthetic batches"""

    def __init__(self, engine, suffix, batches):
        self.engine, self.suffix, self.batches, self.at = engine, suffix, batches, 0

    def next(self):
        b = self.batches[self.at % len(self.batches)]
        self.at += 1
        return b

    def deliver(self, batch):
        for k, v in batch.items():
            if (k + self.suffix) in self.engine.model.input_blob_names:
                self.engine.feed(k + self.suffix, v)

    def stop(self):
        pass


def test_precise_bn_through_an_engine():
    from test_model_gpu import build
    from oracle import model as om
    from models.model_builder_video import ModelBuilder
    from vlfb.engine import Engine
    from vlfb.precise_bn import PreciseBN
    ITERS = 3
    cfg, model, eng, inputs, params, _ = build("charades_r50_baseline", "fp32", SHAPES + BN + [
        "TRAIN.COMPUTE_PRECISE_BN", True, "TRAIN.ITER_COMPUTE_PRECISE_BN", ITERS])
    batches = [om.synth_inputs(cfg, 2, "train", seed=100 + i, crop=64, frames=8) for i in range(ITERS)]
    eng.train_step(0.01)
    eng.train_step(0.01)                                    # (momentum and running averages are not at their initial values)
    make = lambda e, sfx: ListLoader(e, sfx, batches)
    pbn = PreciseBN(eng, make)
    hand = PreciseBN(eng, make, suffix="_bn_hand")
    assert pbn.layers == len([n for n in model.params if n.endswith("_bn_s")]) >= 53
    assert pbn.total == sum(st.C for st in pbn.steps)
    bn_names = set(n for st in pbn.steps for n in (st.rmname, st.rvname))
    assert all(n.endswith(("_bn_rm", "_bn_riv")) for n in bn_names)

    tmodel = ModelBuilder(train=False, split="test", name="bn_test")
    tmodel.build_model(suffix="_test")
    teng = Engine(tmodel, "fp32", base_seed=cfg.RNG_SEED, share_params_with=eng)
    teng.plan(collections.OrderedDict((k + "_test", v.shape) for k, v in inputs.items() if (k + "_test") in tmodel.input_blob_names))
    for k, v in inputs.items():
        if (k + "_test") in tmodel.input_blob_names:
            teng.feed(k + "_test", v)
    teng.forward()
    prob0 = teng.blob_tensor("prob")[0].clone()

    # the same three batches by hand on a second aux engine: the per-iteration contents of step.save
    rows_sm, rows_siv = [], []
    for _ in range(ITERS):
        hand.loader.deliver(hand.loader.next())
        hand.engine.forward()
        torch.cuda.synchronize()
        saves = [st.save.cpu().numpy() for st in hand.steps]
        rows_sm.append(np.concatenate([s[:st.C] for s, st in zip(saves, hand.steps)]))
        rows_siv.append(np.concatenate([s[st.C:] for s, st in zip(saves, hand.steps)]))
    mean, var = ref.chain(np.stack(rows_sm), np.stack(rows_siv), float(cfg.MODEL.BN_EPSILON), ITERS)

    snap = dict(param=eng.flat_param.clone(), mom=eng.flat_mom.clone(), frozen=eng.flat_frozen.clone(),
                state=(eng.iteration, eng.loss_scale, eng.lr))
    version = eng._pstate[0]
    pbn.compute_and_update_bn_stats(7)
    torch.cuda.synchronize()
    assert pbn.forwards == ITERS and eng._pstate[0] == version + 1
    off = 0
    for st in pbn.steps:
        assert torch.equal(eng.param_tensor(st.rmname).cpu(), torch.from_numpy(mean[off:off + st.C])), st.rmname
        assert torch.equal(eng.param_tensor(st.rvname).cpu(), torch.from_numpy(var[off:off + st.C])), st.rvname
        off += st.C
    # nothing else of the train engine moved
    assert torch.equal(eng.flat_param, snap["param"]) and torch.equal(eng.flat_mom, snap["mom"])
    assert (eng.iteration, eng.loss_scale, eng.lr) == snap["state"]
    for n, (o, cnt, shape) in eng.frozen_layout.items():
        same = torch.equal(eng.flat_frozen[o:o + cnt], snap["frozen"][o:o + cnt])
        assert same == (n not in bn_names), n
    assert bn_names <= set(eng.frozen_layout)

    # the test engine sees the new statistics; feeding the same values by hand gives the same forward
    teng.forward()
    prob1 = teng.blob_tensor("prob")[0].clone()
    assert not torch.equal(prob1, prob0)
    fed, off = {}, 0
    for st in pbn.steps:
        fed[st.rmname], fed[st.rvname] = mean[off:off + st.C], var[off:off + st.C]
        off += st.C
    eng.feed_params(fed)
    teng.forward()
    prob2 = teng.blob_tensor("prob")[0].clone()
    assert torch.equal(prob1, prob2) and bool(torch.isfinite(prob1.float()).all())

    # the same iteration again: no forward, the finalized rows are written again
    eng.param_tensor(pbn.steps[0].rmname).fill_(123.0)
    pbn.compute_and_update_bn_stats(7)
    torch.cuda.synchronize()
    assert pbn.forwards == ITERS
    assert torch.equal(eng.param_tensor(pbn.steps[0].rmname).cpu(), torch.from_numpy(mean[:pbn.steps[0].C]))
    pbn.compute_and_update_bn_stats(8)
    assert pbn.forwards == 2 * ITERS


def test_precise_bn_refuses_a_model_without_batch_norm():
    from test_model_gpu import build
    from vlfb.precise_bn import PreciseBN
    cfg, model, eng, inputs, params, _ = build("charades_r50_baseline", "bf16", SHAPES + ["TRAIN.COMPUTE_PRECISE_BN", True])
    with pytest.raises(ValueError, match="SpatialBN"):
        PreciseBN(eng, lambda e, sfx: None)
