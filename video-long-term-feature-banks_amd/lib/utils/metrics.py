"""The reference's lib/utils/metrics.py -- import path and names -- on device-resident counters.

The reference's meter fetches `pred` and `labels` from every GPU every iteration (get_multi_gpu_outputs, :514-540)
and calls scikit-learn at the end.  Here the numbers are accumulated by kernels inside the step
(vlfb.metrics.DeviceMeter, attached with Engine.attach_meter) and read once per cfg.LOG_PERIOD; mAP / wAP / ROC-AUC
come from vlfb_class_ap_auc.

Differences that follow from reading once per period:
  * `top1` / `top5` of a log line are the error over the iterations since the previous line (the reference prints the
    last iteration's); the aggregated figures are the reference's (every iteration has the same batch size).
  * `Loss` is the last iteration's, from the engine's device loss ring.
AVA's frame-mAP: the reference does not ship the evaluator its utils/ava_eval_helper.py imports
(utils.ava_evaluation.*), so a MetricsCalculator built WITHOUT `ava_groundtruth` raises NotImplementedError in
finalize_metrics for cfg.DATASET == 'ava'.  With it (read_csv's triple), the head's probabilities are appended to a device
table inside the step, the caller reports every test iteration's metadata and boxes (add_ava_batch), and finalize_metrics
scores the table with the PASCAL-VOC protocol at IoU 0.5 on the device (vlfb.metrics.ava_frame_ap).
"""
from __future__ import absolute_import, division, print_function, unicode_literals

import collections
import datetime
import logging
import os
import pickle

import numpy as np
import torch

from core.config import config as cfg
from vlfb import dist
from vlfb.metrics import DeviceMeter

# (the reference imports these names here as well)
from utils.ava_eval_helper import evaluate_ava, evaluate_ava_from_files, read_csv, read_exclusions, read_labelmap  # noqa: F401

logger = logging.getLogger(__name__)


def get_ava_mini_groundtruth(full_groundtruth):
    """the "mini" validation set: the entries of read_csv's three dictionaries whose second is a multiple of 4"""
    mini = []
    for part in full_groundtruth[:3]:
        kept = collections.defaultdict(list)
        for key in part.keys():
            if int(key.split(',')[1]) % 4 == 0:
                kept[key] = part[key]
        mini.append(kept)
    return mini


def _dev(x, dtype):
    if isinstance(x, torch.Tensor):
        t = x.to(device="cuda", dtype=dtype if dtype is not None else x.dtype)
    else:
        t = torch.from_numpy(np.ascontiguousarray(np.asarray(x))).to(device="cuda", dtype=dtype)
    return t.contiguous()


def _scores(x):
    if isinstance(x, torch.Tensor) and x.dtype in (torch.float16, torch.bfloat16):
        return _dev(x, None)
    return _dev(x, torch.float32)


def compute_topk_correct_hits(top_k, preds, labels):
    """number of rows whose label is among the top_k scores (metrics.py:485-500); numpy arrays or device tensors.
    Ties follow the rank rule of include/vlfb.h (vlfb_topk_hits)."""
    preds = _scores(preds)
    preds = preds.reshape(preds.shape[0], -1)
    meter = DeviceMeter("topk", preds.shape[1], ks=(top_k,), device=preds.device)
    meter.update(preds, _dev(labels, torch.int32).reshape(-1))
    return meter.read()["hits"][int(top_k)]


def mean_ap_metric(predicts, targets):
    """(mean_auc, mean_ap, mean_wap, all_aps) for Charades (metrics.py:444-482) without scikit-learn; numpy arrays,
    lists of them, or device tensors"""
    if isinstance(predicts, (list, tuple)):
        predicts = torch.cat([_scores(p) for p in predicts]) if isinstance(predicts[0], torch.Tensor) else np.vstack(predicts)
        targets = torch.cat([_dev(t, torch.int32) for t in targets]) if isinstance(targets[0], torch.Tensor) else np.vstack(targets)
    predicts, targets = _scores(predicts), _dev(targets, torch.int32)
    logger.info("Getting mAP for {} examples".format(predicts.shape[0]))
    meter = DeviceMeter("map", predicts.shape[1], n_items=predicts.shape[0], device=predicts.device)
    meter.update(predicts, targets)
    r = meter.read()
    return r["mean_auc"], r["mean_ap"], r["mean_wap"], r["all_aps"]


class MetricsCalculator(object):
    """MetricsCalculator(engine, split): owns the DeviceMeter of the engine's head and attaches it.  `model` of the
    reference's signature is the planned vlfb.engine.Engine here; `test_labels` is the int32 device tensor a
    test-mode net (no label blob) is metered against (Engine.attach_meter)."""

    def __init__(self, engine, split, video_idx_to_name=None, total_num_boxes=None, test_labels=None, ava_groundtruth=None,
                 excluded_keys=None, class_whitelist=None, categories=None, ava_table_rows=None, keep_predictions=False):
        """keep_predictions: on a single-label test split the meter also keeps the first TEST.DATASET_SIZE prediction rows
        and labels on the device (vlfb_topk_hits_keep) and finalize_metrics writes them as epic_predictions_<name>.pkl
        (metrics.py:222-226), the input of vlfb.epic_eval.evaluate_actions.
        Under a process group of N ranks every rank keeps only the rows it issued (the slices of vlfb.lfb_pass.rank_source),
        in tables sized for its ceil(P / N) of the P slices; finalize_metrics gathers them, rebuilds the single-process
        stream order (vlfb.metrics.interleave_rows) and scores that with the single-process kernels.
        ava_groundtruth: read_csv's (boxes, labels, scores) -- with it an AVA config is scored (frame-mAP);
        excluded_keys / class_whitelist / categories: read_exclusions' and read_labelmap's results; ava_table_rows: rows of
        the score table (default: every row ceil(TEST.DATASET_SIZE / TEST.BATCH_SIZE) iterations issue, padding included)"""
        self.model = self.engine = engine
        self.split = split
        self.video_idx_to_name = video_idx_to_name
        self._total_num_boxes = total_num_boxes
        self.best_top1 = float('inf')
        self.best_top5 = float('inf')
        self.best_map = float('inf') * (-1.0)
        self.lr = 0
        self.num_test_clips = 1
        if cfg.DATASET == 'charades':
            # (tools/test_net.py / train_net.py set NUM_TEST_CLIPS from _FINAL_EVAL / _DURING_TRAINING before they test)
            self.num_test_clips = cfg.CHARADES.get("NUM_TEST_CLIPS", cfg.CHARADES.NUM_TEST_CLIPS_DURING_TRAINING)
        self.meter = None
        self.ava_groundtruth = ava_groundtruth
        self.excluded_keys = set(excluded_keys) if excluded_keys else set()
        self.class_whitelist = set(class_whitelist) if class_whitelist else None
        self.categories = categories
        self.keep_predictions = bool(keep_predictions) and not cfg.MODEL.MULTI_LABEL and split != 'train'
        self.world = dist.world_size()
        from vlfb.engine import LossStep
        heads = [st for st in engine.steps if isinstance(st, LossStep) and st.prob is not None]
        if cfg.DATASET == 'ava' and ava_groundtruth is not None and heads and split != 'train':
            cols, self.batch_rows = heads[0].cols, heads[0].rows
            if ava_table_rows is None:
                ava_table_rows = self._rank_slices(cfg.TEST.DATASET_SIZE, max(cfg.TEST.BATCH_SIZE // self.world, 1)) * self.batch_rows
            self.meter = DeviceMeter("ava", cols, n_items=int(ava_table_rows), device=engine.device)
            engine.attach_meter(self.meter, labels=test_labels)
        if cfg.DATASET != 'ava' and heads:
            cols, self.batch_rows = heads[0].cols, heads[0].rows
            if cfg.MODEL.MULTI_LABEL:
                if split != 'train':                 # (the reference computes no mAP while training: full_map = 0)
                    total = self.num_test_clips * cfg.TEST.DATASET_SIZE
                    self._map_items, self._map_total = max(total // self.num_test_clips, 1), total
                    if self.world > 1:               # this rank's rows with their labels, merged in finalize_metrics
                        self.meter = DeviceMeter("ava", cols, n_items=self._rank_slices(total, self.batch_rows) * self.batch_rows,
                                                 device=engine.device, keep_labels=True)
                    else:
                        self.meter = DeviceMeter("map", cols, n_items=self._map_items, total_rows=total, device=engine.device)
            else:
                keep = int(cfg.TEST.DATASET_SIZE) if self.keep_predictions else None
                if keep is not None and self.world > 1:
                    keep = self._rank_slices(keep, self.batch_rows) * self.batch_rows
                self.meter = DeviceMeter("topk", cols, ks=(1, 5), device=engine.device, keep_rows=keep)
            if self.meter is not None:
                engine.attach_meter(self.meter, labels=test_labels)
        self.reset()

    def _rank_slices(self, db_size, n):
        """slices of `n` a rank runs of a pass over `db_size`: ceil(P / world) of the P = ceil(db_size / n)"""
        return -(-(-(-int(db_size) // int(n))) // self.world)

    def _gather_parts(self, *tensors):
        """the rows this rank issued (its cursor) of each 2-D device tensor, from every rank: dist.gather_ragged moves bytes,
        exact on gloo and nccl.  -> one list of per-rank tensors for each of `tensors`"""
        rows = dist.gather_objects(self.meter.counters()[2])
        for t in tensors:
            assert max(rows) <= t.shape[0], "%d rows were issued into a table of %d" % (max(rows), t.shape[0])
        return [dist.gather_ragged(t, rows) for t in tensors]

    def reset(self):
        logger.info('Resetting {} metrics...'.format(self.split))
        self.aggr_loss = 0.0
        self._loss_count = 0                         # (the average restarts with the sum)
        self.aggr_batch_size = 0
        self._last = (0, 0, 0)                       # hits@1, hits@5, rows at the previous read
        self.avg_loss = self.avg_err = self.avg_err5 = float('nan')
        self.full_map = 0.0
        self._ava_pos = 0                            # table row the next test iteration starts at
        self._ava_rows, self._ava_keys, self._ava_boxes = [], [], []
        if self.meter is not None:
            self.meter.reset()

    def add_ava_batch(self, metadata, original_boxes):
        """AVA, once per test iteration: metadata [r][2] = (video index, second) and original_boxes [r][5] =
        (batch index, x1, y1, x2, y2) of the r REAL RoIs of the iteration.  The step issued the planned number of rows;
        the rows behind r are padding and are never named to the evaluator."""
        assert self.meter is not None and self.meter.kind == "ava", "add_ava_batch needs ava_groundtruth= on an AVA config"
        metadata = np.asarray(metadata).reshape(-1, 2)
        boxes = np.asarray(original_boxes, np.float64).reshape(-1, 5)
        r = metadata.shape[0]
        assert boxes.shape[0] == r and r <= self.batch_rows, (r, boxes.shape, self.batch_rows)
        self._ava_rows.append(self._ava_pos + np.arange(r, dtype=np.int64))
        for m in metadata:
            video = self.video_idx_to_name[int(np.round(m[0]))]
            self._ava_keys.append(video + ',' + '%04d' % int(np.round(m[1])))
        self._ava_boxes.append(boxes[:, 1:5])
        self._ava_pos += self.batch_rows

    def _read_topk(self):
        """(period err, period err5, aggregated err, aggregated err5) from ONE read, summed over ranks"""
        own_hits, rows, _, _ = self.meter.counters()
        h1, h5, rows = dist.sum_ints(own_hits + [rows], self.engine.device)
        p1, p5, prow = h1 - self._last[0], h5 - self._last[1], rows - self._last[2]
        self._last = (h1, h5, rows)
        err = lambda h, n: (1.0 - float(h) / n) * 100 if n else float('nan')
        self.avg_err, self.avg_err5 = err(h1, rows), err(h5, rows)
        self.aggr_batch_size = rows
        return err(p1, prow), err(p5, prow), self.avg_err, self.avg_err5

    def calculate_and_log_all_metrics_train(self, curr_iter, timer, suffix='', losses=None):
        """losses: the values of a read of the device loss ring the caller already made at this iteration (the training
        driver's NaN guard drains the ring); default: read it here"""
        if (curr_iter + 1) % cfg.LOG_PERIOD != 0:
            return
        self.lr = float(self.engine.lr)
        if losses is None:
            losses = self.engine.recent_losses()
        cur_loss = losses[-1] if losses else float('nan')
        if losses:
            self.aggr_loss += float(np.sum(losses))
            self._loss_count = getattr(self, "_loss_count", 0) + len(losses)
            self.avg_loss = self.aggr_loss / self._loss_count
        rem_iters = cfg.SOLVER.MAX_ITER - curr_iter - 1
        eta = str(datetime.timedelta(seconds=int(timer.average_time * rem_iters)))
        epoch = (curr_iter + 1) / (cfg.TRAIN.DATASET_SIZE / cfg.TRAIN.BATCH_SIZE)
        log_str = ' '.join((
            '| Train ETA: {} LR: {:.8f}',
            ' Iters [{}/{}]',
            '[{:.2f}ep]',
            ' Time {:0.3f}',
            ' Loss {:7.4f}',
        )).format(eta, self.lr, curr_iter + 1, cfg.SOLVER.MAX_ITER, epoch, timer.diff, cur_loss)
        if not cfg.MODEL.MULTI_LABEL and self.meter is not None:
            cur_err, cur_err5, _, _ = self._read_topk()
            log_str += ' top1 {:7.3f} top5 {:7.3f}'.format(cur_err, cur_err5)
        if dist.rank() == 0:
            print(log_str)

    def calculate_and_log_all_metrics_test(self, curr_iter, timer, total_iters, suffix=''):
        cur_batch_size = self.batch_rows * dist.world_size() if self.meter is not None else 0
        if cfg.MODEL.MULTI_LABEL:
            self.aggr_batch_size += cur_batch_size
        if (curr_iter + 1) % cfg.LOG_PERIOD == 0 or curr_iter + 1 == total_iters:
            tail = ''
            if not cfg.MODEL.MULTI_LABEL and self.meter is not None:
                cur_err, cur_err5, avg_err, avg_err5 = self._read_topk()
                tail = (' top1 {:7.3f} ({:7.3f})' + '  top5 {:7.3f} ({:7.3f})').format(cur_err, avg_err, cur_err5, avg_err5)
            test_str = ' '.join((
                '| Test: [{}/{}]',
                ' Time {:0.3f}',
                ' current batch {}',
                ' aggregated batch {}',
            )).format(curr_iter + 1, total_iters, timer.diff, cur_batch_size, self.aggr_batch_size)
            if dist.rank() == 0:
                print(test_str + tail)

    def finalize_metrics(self, is_train=False, name='latest', out_dir=None):
        """the final figures: mAP of the merged table (Charades), or the aggregated top-1 / top-5 error.  A calculator
        built with keep_predictions also writes epic_predictions_<name>.pkl = (float32 [n][cols], int32 [n]), pickle
        protocol 2, into `out_dir` (default: the current directory, as the reference does)."""
        if cfg.DATASET == 'ava' and self.ava_groundtruth is None:
            raise NotImplementedError(
                "AVA frame-mAP: the reference does not ship its evaluator (utils/ava_eval_helper.py imports "
                "utils.ava_evaluation.*, which is absent), so there is nothing to compute it with")
        if cfg.DATASET == 'ava':
            self.full_map = 0.0
            if is_train or self.meter is None:
                return
            # one add_ava_batch per forward pass: a missed or doubled call would shift every later row
            cursor = self.meter.counters()[2]
            assert self._ava_pos == cursor, "add_ava_batch accounted for %d table rows, the steps issued %d" % (self._ava_pos, cursor)
            rows = np.concatenate(self._ava_rows) if self._ava_rows else np.zeros(0, np.int64)
            boxes = np.concatenate(self._ava_boxes) if self._ava_boxes else np.zeros((0, 4))
            keys = list(self._ava_keys)
            if self.world > 1:
                # every rank holds the rows it issued: gather the tables, renumber every rank's rows to global rows
                from vlfb.metrics import ava_frame_ap, merge_ava_ranks
                tables, = self._gather_parts(self.meter.table)
                table, rows, keys, boxes = merge_ava_ranks(tables, dist.gather_objects((rows, keys, boxes)), self.batch_rows)
                self.results = ava_frame_ap(table, rows, keys, boxes, self.ava_groundtruth, self.excluded_keys, self.class_whitelist)
                self.results["rows_seen"] = int(table.shape[0])
            else:
                self.results = self.meter.finalize(rows, keys, boxes, self.ava_groundtruth, self.excluded_keys, self.class_whitelist)
            self.full_map = self.results["mean_ap"]
            return
        if self.meter is None:
            self.full_map = 0.0
            return
        if cfg.MODEL.MULTI_LABEL:
            if is_train:
                self.full_map = 0.0
                return
            if self.world > 1:
                # every rank holds the clips it issued: the stream of the single process, merged by its kernel
                from vlfb.metrics import merge_map_ranks
                tables, labels = self._gather_parts(self.meter.table, self.meter.labels)
                self.merged = merge_map_ranks(tables, labels, self.batch_rows, self._map_items, self._map_total)
                self.results = self.merged.read()
            else:
                self.results = self.meter.read()
            mismatches = self.results["label_mismatches"]
            assert mismatches == 0, "labels of %d merged clip elements differ from their video's" % mismatches
            self.full_map = self.results["mean_ap"]
        else:
            self._read_topk()
            if not is_train and self.meter.keep_rows:
                if self.world > 1:
                    from vlfb.metrics import merge_keep_ranks
                    tables, labels = self._gather_parts(self.meter.table, self.meter.labels.view(-1, 1))
                    table, labels = merge_keep_ranks(tables, labels, self.batch_rows, int(cfg.TEST.DATASET_SIZE))
                    labels = labels.view(-1)
                else:
                    table, labels = self.meter.kept()
                    # stack_predictions (metrics.py:147-163): every row of the split was tested, at most a batch of padding cut
                    assert table.shape[0] == self.meter.keep_rows, "%d of %d predictions were issued" % (table.shape[0], self.meter.keep_rows)
                self.predictions = (table.cpu().numpy(), labels.cpu().numpy())
                self.predictions_file = os.path.join(out_dir if out_dir is not None else os.getcwd(), 'epic_predictions_%s.pkl' % name)
                if dist.rank() == 0:
                    with open(self.predictions_file, 'wb') as f:
                        pickle.dump(self.predictions, f, protocol=2)
                dist.barrier()                       # (no rank returns before the file is there)

    def get_computed_metrics(self):
        json_stats = {}
        if cfg.MODEL.MULTI_LABEL:
            if self.split == 'train':
                json_stats['train_loss'] = self.avg_loss
                json_stats['train_full_map'] = self.full_map
            elif self.split in ['test', 'val']:
                json_stats['test_full_map'] = self.full_map
                json_stats['test_best_map'] = self.best_map
        else:
            if self.split == 'train':
                json_stats['train_loss'] = self.avg_loss
                json_stats['train_err'] = self.avg_err
                json_stats['train_err5'] = self.avg_err5
            elif self.split in ['test', 'val']:
                json_stats['test_err'] = self.avg_err
                json_stats['test_err5'] = self.avg_err5
                json_stats['best_err'] = self.best_top1
                json_stats['best_err5'] = self.best_top5
        return json_stats

    def log_final_metrics(self, model_iter, total_iters=None):
        if total_iters is None:
            total_iters = cfg.SOLVER.MAX_ITER
        if cfg.MODEL.MULTI_LABEL:
            info = ''
            if self.meter is not None and self.meter.kind == "ava" and cfg.AVA.get("DETECTION_SCORE_THRESH") is not None:
                info = 'Box@%.5f ' % cfg.AVA.DETECTION_SCORE_THRESH
            print('* {} testing finished #iters [{}|{}]: mAP: {:.3f}'.format(info, model_iter + 1, total_iters, self.full_map))
        else:
            print('* Finished #iters [{}|{}]: top1: {:.3f} top5: {:.3f}'.format(
                model_iter + 1, total_iters, 100.0 - self.avg_err, 100.0 - self.avg_err5))

    def compute_and_log_best(self):
        if cfg.MODEL.MULTI_LABEL:
            if self.full_map > self.best_map:
                self.best_map = self.full_map
                print('\n* Best model: mAP: {:7.3f}\n'.format(self.best_map))
        elif self.avg_err < self.best_top1:
            self.best_top1 = self.avg_err
            self.best_top5 = self.avg_err5
            print('\n* Best model: top1: {:7.3f} top5: {:7.3f}\n'.format(self.best_top1, self.best_top5))


def get_json_stats_dict(train_meter, test_meter, curr_iter):
    """Define stats that will be logged (reference metrics.py:566-593: the same keys in the same order)."""
    import utils.misc as misc
    json_stats = {
        "eval_period": cfg.TRAIN.EVAL_PERIOD,
        "batchSize": cfg.TRAIN.BATCH_SIZE,
        "dataset": cfg.DATASET,
        "num_classes": cfg.MODEL.NUM_CLASSES,
        "momentum": cfg.SOLVER.MOMENTUM,
        "weightDecay": cfg.SOLVER.WEIGHT_DECAY,
        "nGPU": cfg.NUM_GPUS,
        "LR": cfg.SOLVER.BASE_LR,
        "bn_momentum": cfg.MODEL.BN_MOMENTUM,
        "current_learning_rate": train_meter.lr,
    }
    json_stats.update(train_meter.get_computed_metrics())
    if test_meter is not None:
        json_stats.update(test_meter.get_computed_metrics())
    json_stats['used_gpu_memory'] = misc.get_gpu_stats()
    json_stats['currentIter'] = curr_iter + 1
    json_stats['epoch'] = curr_iter / (cfg.TRAIN.DATASET_SIZE / cfg.TRAIN.BATCH_SIZE)
    return json_stats
