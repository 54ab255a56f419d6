"""Precise BN (reference: lib/utils/bn_helper.py BatchNormHelper): before every checkpoint and every evaluation the running
statistics of a SpatialBN model are replaced by the average over TRAIN.ITER_COMPUTE_PRECISE_BN training batches.

    bn_aux = PreciseBN(train_engine, make_loader)          # make_loader(aux_engine, suffix) -> a started loader
    bn_aux.compute_and_update_bn_stats(curr_iter)

The aux engine is the reference's bn_aux model: the train graph on the training split, forward only, with the train
engine's parameters (share_params_with) -- except `_bn_rm` / `_bn_riv`, of which it keeps private copies: a training-mode
SpatialBN moves them by momentum ("rm/riv is fully irrelevant in bn_aux_model", bn_helper.py:80), and the train engine's
must not move before the new statistics are known to be valid.  The reference fetches `_bn_sm` / `_bn_siv` of every layer
to the host after every batch; here one kernel launch per batch adds them to packed device accumulators
(csrc/vlfb_bn_stats.hip), and the only synchronisation of a whole update is the read of the `bad` counter.
"""
import logging

import torch

from core.config import config as cfg
from vlfb import hip

logger = logging.getLogger(__name__)


def bn_layer_table(engine, owner=None):
    """(device table, packed elements, [BNStep]) over the training-mode SpatialBN steps of a planned engine: `step.save`
    holds mean then inverse std; the running statistics are `owner`'s parameter tensors (default: the engine's own)"""
    from vlfb.engine import BNStep
    steps = [st for st in engine.steps if isinstance(st, BNStep) and not st.is_test]
    owner = engine if owner is None else owner
    rows = []
    for st in steps:
        rm, rv = owner.param_tensor(st.rmname), owner.param_tensor(st.rvname)
        assert st.save is not None and st.save.numel() == 2 * st.C and rm.numel() == st.C and rv.numel() == st.C, st.name()
        assert rm.dtype == torch.float32 and rv.dtype == torch.float32 and rm.is_contiguous() and rv.is_contiguous()
        rows.append((hip.ptr(st.save), hip.ptr(st.save) + 4 * st.C, rm, rv, st.C))
    if not rows:
        return None, 0, steps
    table, total = hip.bn_layer_table(rows, engine.device)
    return table, total, steps


class PreciseBN(object):
    """The BatchNormHelper of this project (see the module docstring)."""

    def __init__(self, train_engine, make_loader, suffix="_bn_aux", dtype=None):
        from models.model_builder_video import ModelBuilder
        from vlfb import dist
        from vlfb.engine import Engine
        import collections
        if dist.world_size() > 1:
            raise NotImplementedError("PreciseBN: the reference sums the statistics of all GPUs in a fixed order; that order "
                                      "is not reproduced for a world size above 1")
        self.train_engine = train_engine
        self._last_update_iter = -1
        self._finalized = False
        self.forwards = 0                                  # aux forwards run so far
        tmodel = train_engine.model
        model = ModelBuilder(train=True, force_fw_only=True, split=cfg.TRAIN.DATA_TYPE,
                             name='{}_bn_aux'.format(cfg.MODEL.MODEL_NAME))
        model.build_model(suffix=suffix)
        if dtype is None:
            dtype = "mix" if train_engine.mix else "split" if train_engine.split else \
                {torch.float32: "fp32", torch.bfloat16: "bf16", torch.float16: "fp16"}[train_engine.tdtype]
        self.engine = Engine(model, dtype, device=train_engine.device, base_seed=train_engine.base_seed,
                             share_params_with=train_engine)
        tsfx = tmodel.suffix
        shapes = collections.OrderedDict()
        for name in tmodel.input_blob_names:
            assert name.endswith(tsfx), name
            shapes[name[:len(name) - len(tsfx)] + suffix] = tuple(train_engine.env[name].root.shape)
        assert list(shapes) == list(model.input_blob_names), (list(shapes), model.input_blob_names)
        self.engine.plan(shapes)
        from vlfb.engine import BNStep
        steps = [st for st in self.engine.steps if isinstance(st, BNStep) and not st.is_test]
        if not steps:
            raise ValueError("TRAIN.COMPUTE_PRECISE_BN is set, but the model has no SpatialBN layer (MODEL.USE_AFFINE / "
                             "NONLOCAL.USE_AFFINE graphs have no batch statistics)")
        # private running statistics for the aux engine: its forwards move them by momentum, the train engine's stay
        eng = self.engine
        for st in steps:
            for n in (st.rmname, st.rvname):
                assert n in eng.shared_params, n
                off, cnt, shape = eng.frozen_layout[n]
                eng.param_views[n] = eng.flat_frozen[off:off + cnt].view(shape)
                eng.shared_params.discard(n)
        missing = [n for st in steps for n in (st.sname, st.bname) if n not in eng.shared_params]
        assert not missing, "the aux engine does not share %r with the train engine" % missing
        self.table, self.total, self.steps = bn_layer_table(eng, owner=train_engine)
        self.layers = len(self.steps)
        self.sum_mean = torch.zeros(self.total, device=eng.device, dtype=torch.float32)
        self.sum_mean2 = torch.zeros(self.total, device=eng.device, dtype=torch.float32)
        self.bad = torch.zeros(1, device=eng.device, dtype=torch.int32)
        self.eps = float(cfg.MODEL.BN_EPSILON)             # every layer, the non-local ones included (bn_helper.py:163)
        self.loader = make_loader(eng, suffix)

    def layer_names(self):
        return [st.rmname[:-len("_bn_rm")] if st.rmname.endswith("_bn_rm") else st.rmname for st in self.steps]

    def _accumulate(self):
        hip.call("vlfb_bn_precise_accumulate", hip.ptr(self.table), self.layers, self.eps, hip.ptr(self.sum_mean),
                 hip.ptr(self.sum_mean2))

    def compute_and_update_bn_stats(self, curr_iter=None):
        """bn_helper.py:103-133: new statistics only when curr_iter changes (a checkpoint and an evaluation of the same
        iteration see the same ones); otherwise the finalized rows are written again"""
        if curr_iter is None or curr_iter != self._last_update_iter or not self._finalized:
            logger.info('Computing and updating BN stats at iter: {}'.format(None if curr_iter is None else curr_iter + 1))
            self._last_update_iter = curr_iter
            self._finalized = False
            iters = int(cfg.TRAIN.ITER_COMPUTE_PRECISE_BN)
            hip.call("vlfb_zero_f32", hip.ptr(self.sum_mean), self.total)
            hip.call("vlfb_zero_f32", hip.ptr(self.sum_mean2), self.total)
            for _ in range(iters):
                self.loader.deliver(self.loader.next())
                self.engine.forward()
                self._accumulate()
                self.forwards += 1
            hip.call("vlfb_bn_precise_finalize", hip.ptr(self.table), self.layers, iters * int(cfg.NUM_GPUS),
                     hip.ptr(self.sum_mean), hip.ptr(self.sum_mean2), hip.ptr(self.bad))
            bad = int(self.bad.item())                     # the one synchronisation, off the step path
            if bad > 0:
                var = self.sum_mean2.cpu()
                off = 0
                for name, st in zip(self.layer_names(), self.steps):
                    if not bool((var[off:off + st.C] > 0).all()):
                        raise AssertionError("layer: {} var < 0".format(name))
                    off += st.C
                raise AssertionError("%d channels with var < 0" % bad)
            self._finalized = True
        else:
            logger.info('BN of iter {} computed. Update to GPU only.'.format(curr_iter + 1))
        hip.call("vlfb_bn_precise_update", hip.ptr(self.table), self.layers, hip.ptr(self.sum_mean), hip.ptr(self.sum_mean2))
        # engines that alias the parameters (the test net) rebuild what they derive from them; the train net derives nothing
        # from running statistics (its SpatialBN uses the batch's), so it stays in step with the new version
        te = self.train_engine
        in_step = te._operand_version == te._pstate[0]
        te._pstate[0] += 1
        if in_step:
            te._operand_version = te._pstate[0]

    def stop(self):
        if self.loader is not None and hasattr(self.loader, "stop"):
            self.loader.stop()
