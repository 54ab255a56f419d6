"""Host pieces of the training driver: the index walk of lfb_pass.frame_train_source against a transcription of the
reference's loader (lib/datasets/dataloader.py:180-221, split 'train'), and utils.metrics.get_json_stats_dict /
utils.misc.log_json_stats on stub meters."""
import json
import random

import pytest


@pytest.fixture(autouse=True)
def _cfg_put_back():
    yield
    import clip_loader_cases as cases
    from vlfb.presets import load_preset
    load_preset(*cases.RESET)


class RefWalk(object):
    """dataloader.py: __init__ (:96-97, :123-124), _shuffle_db_indices (:180-189), _get_next_minibatch_indices (:199-211)"""

    def __init__(self, db_size, batch_size, rng):
        self._db_size, self._batch_size, self._rng = db_size, batch_size, rng
        self._current = 0
        self._perm = list(range(db_size))
        self._shuffle_db_indices(db_size)

    def _shuffle_db_indices(self, db_size):
        indices = list(range(db_size))
        self._rng.shuffle(indices)
        self._perm = indices
        self._current = 0

    def next(self):
        if (self._current + self._batch_size) >= self._db_size:
            self._shuffle_db_indices(self._db_size)
        db_indices = self._perm[self._current:self._current + self._batch_size]
        self._current += self._batch_size
        return db_indices


class StubIndex(object):
    """a 5-clip training index at batch 2 that records what it is asked for"""
    split, batch_size = "train", 2

    def __init__(self):
        self.asked = []

    def get_db_size(self):
        return 5

    def get_minibatch_info(self, indices, rng):
        import collections
        self.asked.append(list(indices))
        Clip = collections.namedtuple("Clip", "video center seq labels shift")
        return [Clip(i, rng.randrange(100), [i, i + 1], [i % 3], None) for i in indices]


def test_train_index_walk_is_the_reference_loader_walk():
    from vlfb.presets import load_preset
    from vlfb import lfb_pass
    load_preset("charades_r50_baseline", ["NUM_GPUS", 1])
    ref = RefWalk(5, 2, random.Random(31))
    want = [ref.next() for _ in range(3 * 3)]                   # three epochs: two batches each, the fifth clip's turn never comes
    walk = lfb_pass.train_index_walk(5, 2, random.Random(31))
    assert [next(walk) for _ in range(9)] == want
    assert all(len(b) == 2 for b in want) and len({tuple(b) for b in want}) > 2

    # through the source: the same batches, with the clip draws of get_minibatch_info taken from the same generator in between
    index, store = StubIndex(), object()
    rng, twin = random.Random(31), random.Random(31)
    src = lfb_pass.frame_train_source(index, store, rng, bank_video=lambda v: "v%d" % v, aug_rng="aug")
    ref = RefWalk(5, 2, twin)
    for it in range(9):
        clips, labels, meta, aug, shift = next(src)
        batch = ref.next()
        centers = [twin.randrange(100) for _ in batch]
        assert index.asked[-1] == batch
        assert clips == [(store, i, [i, i + 1]) for i in batch] and labels == [[i % 3] for i in batch]
        assert meta == dict(iteration=it, videos=["v%d" % i for i in batch], centers=centers, padded=[False, False])
        assert aug == "aug" and shift == 1


class StubMeter(object):
    def __init__(self, lr, stats):
        self.lr, self._stats = lr, stats

    def get_computed_metrics(self):
        return dict(self._stats)


def test_json_stats_keys_values_and_line(caplog):
    import logging
    from vlfb.presets import load_preset
    from core.config import config as cfg
    import utils.metrics as metrics
    import utils.misc as misc
    load_preset("charades_r50_baseline", ["NUM_GPUS", 1, "TRAIN.BATCH_SIZE", 4, "TRAIN.EVAL_PERIOD", 20])
    cfg.TRAIN.DATASET_SIZE = 40
    train = StubMeter(0.0125, {"train_loss": 0.5, "train_full_map": 0.0})
    test = StubMeter(0, {"test_full_map": 12.5, "test_best_map": 13.0})
    got = metrics.get_json_stats_dict(train, test, 19)
    # the reference's keys, in its order (metrics.py:569-591)
    assert list(got) == ["eval_period", "batchSize", "dataset", "num_classes", "momentum", "weightDecay", "nGPU", "LR",
                         "bn_momentum", "current_learning_rate", "train_loss", "train_full_map", "test_full_map",
                         "test_best_map", "used_gpu_memory", "currentIter", "epoch"]
    assert got["eval_period"] == 20 and got["batchSize"] == 4 and got["dataset"] == "charades" and got["nGPU"] == 1
    assert got["num_classes"] == cfg.MODEL.NUM_CLASSES and got["momentum"] == cfg.SOLVER.MOMENTUM
    assert got["weightDecay"] == cfg.SOLVER.WEIGHT_DECAY and got["LR"] == cfg.SOLVER.BASE_LR
    assert got["bn_momentum"] == cfg.MODEL.BN_MOMENTUM and got["current_learning_rate"] == 0.0125
    assert (got["train_loss"], got["test_full_map"], got["test_best_map"]) == (0.5, 12.5, 13.0)
    assert got["currentIter"] == 20 and got["epoch"] == 19 / (40 / 4) and isinstance(got["used_gpu_memory"], str)
    no_test = metrics.get_json_stats_dict(train, None, 0)
    assert "test_full_map" not in no_test and no_test["currentIter"] == 1 and no_test["epoch"] == 0
    with caplog.at_level(logging.INFO):
        line = misc.log_json_stats(got)
    assert line == '\njson_stats: ' + json.dumps(got, sort_keys=False) + '\n'
    assert json.loads(line.split("json_stats: ")[1]) == got
    assert any("json_stats: " in r.getMessage() for r in caplog.records)
