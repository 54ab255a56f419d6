"""The training driver (reference: tools/train_net.py:49-212): `train` chains the loaders, the engine step, the NaN guard,
checkpoints, precise BN, the periodic evaluation on shared parameters and the JSON stats line.

    train(make_store)                                    # make_store(device, stream) -> FrameStore with its fetch

One deviation in the build order: the reference builds the test model first ("so that we don't overwrite init") because
both nets initialise the same workspace blobs.  Here the TRAIN engine owns the parameters and the test engine is built
second with share_params_with= it; there is one initialisation, the train engine's.

N ranks (one process per GPU under a process group of cfg.NUM_GPUS ranks): the index walk is ONE walk, drawn from a generator
that is private to the source and seeded alike everywhere, of which rank r trains on slices r, r + N, ... (lfb_pass.rank_source;
slice g of global batch b on gpu_g); the augmentation draws come from a generator of the rank's own.  The engine reduces
the gradients (Engine.enable_data_parallel, which first makes rank 0's parameters everybody's), the evaluation is shared
(passes.run_pass_ranks), rank 0 writes checkpoints, the stats line and the log, and every rank returns the same
last_checkpoint, json_stats and eval_iters.
"""
import collections
import logging
import os
import random

import numpy as np

from core.config import config as cfg
from utils import misc
from vlfb import dist, lfb_pass, passes
from vlfb.passes import Timer

logger = logging.getLogger(__name__)

Wrapper = collections.namedtuple("Wrapper", "model engine index loader store timer meter suffix bank_video")


def create_wrapper(is_train, make_store, lfb, owner=None, dtype="mix", device="cuda:0", n_slots=2, max_src_hw=(256, 340),
                   ava_groundtruth=None, excluded_keys=(), class_whitelist=None, categories=None, suffix=None, force_fw_only=False):
    """train_net.py:49-90: the model, its planned engine, the dataset index, the loader (AvaIndex + MinibatchLoader for AVA,
    CharadesIndex / EpicIndex + FrameLoader otherwise; not started), the frame store on the loader's stream, a timer and the
    MetricsCalculator.  `owner`: the engine whose parameters this one aliases (the train engine, for the test wrapper and
    the precise-BN aux engine).  -> Wrapper"""
    from datasets import ava, charades, epic
    import utils.metrics as metrics
    if is_train:
        suffix, split, part = suffix or '_train', cfg.TRAIN.DATA_TYPE, cfg.TRAIN
    else:
        suffix, split, part = suffix or '_test', cfg.TEST.DATA_TYPE, cfg.TEST
    n = part.BATCH_SIZE // cfg.NUM_GPUS
    rows = None
    if cfg.DATASET == 'ava':
        index = ava.AvaIndex.from_cfg(split, False)
        rows = n * passes.most_boxes(index)
    elif cfg.DATASET == 'charades':
        index = charades.CharadesIndex.from_cfg(split, False)
    else:
        index = epic.EpicIndex.from_cfg(split, False, shift=None if is_train else cfg.TEST.CROP_SHIFT)
    model, engine, loader, store = passes.build(
        make_store, suffix, dtype, n, part.VIDEO_LENGTH, part.CROP_SIZE, rows, train=is_train, split=split, name=split,
        force_fw_only=force_fw_only, bank=lfb, aug=1 if (is_train and split == "train") else 0, owner=owner, device=device,
        n_slots=n_slots, max_src_hw=max_src_hw)
    meter = None
    if not force_fw_only:
        scored = cfg.DATASET == 'ava' and not is_train
        meter = metrics.MetricsCalculator(
            engine, split, video_idx_to_name=index.video_idx_to_name,
            ava_groundtruth=ava_groundtruth if scored else None, excluded_keys=excluded_keys if scored else None,
            class_whitelist=class_whitelist if scored else None, categories=categories if scored else None,
            ava_table_rows=(misc.get_total_test_iters(index) * rows) if scored else None)
    return Wrapper(model, engine, index, loader, store, Timer(), meter, suffix, passes.bank_video(index))


def train_source(w, rng, aug_rng, walk_rng=None):
    """what the wrapper's loader is started with for training: ava.minibatch_source (shuffled per pass with `aug_rng`, a
    numpy generator, or with `walk_rng` when the walk has a generator of its own) or lfb_pass.frame_train_source (`rng`:
    random.Random's methods)"""
    from datasets import ava
    if cfg.DATASET == 'ava':
        if walk_rng is not None:
            return ava.minibatch_source(w.index, w.store, walk_rng, bank=w.loader.bank, aug_rng=aug_rng)
        return ava.minibatch_source(w.index, w.store, aug_rng, bank=w.loader.bank)
    return lfb_pass.frame_train_source(w.index, w.store, rng, w.bank_video, aug_rng=aug_rng)


def rank_train_source(w):
    """the training source of this rank under a process group: the slices rank, rank + world, ... of the one walk whose
    generator is seeded alike on all ranks (random.Random(RNG_SEED) for Charades / EPIC, np.random.RandomState(RNG_SEED) for
    AVA) and consumed by the source alone; the augmentation generator np.random.RandomState(RNG_SEED + 1 + rank) is the
    rank's own.  Skipped slices cost index arithmetic and walk draws (lfb_pass.rank_source)."""
    aug = np.random.RandomState(cfg.RNG_SEED + 1 + dist.rank())
    source = train_source(w, random.Random(cfg.RNG_SEED), aug, walk_rng=np.random.RandomState(cfg.RNG_SEED))
    return lfb_pass.rank_source(source, None)


def eval_pass(test, name='latest', curr_iter=None, rng=None):
    """the in-training evaluation (train_net.py:184-196) on the test wrapper, whose engine aliases the parameters being
    trained: reset, one pass over the test split, finalize_metrics / compute_and_log_best / log_final_metrics.  Charades /
    EPIC: the loop of test_one_crop; nothing is loaded and no predictions are kept.  AVA: the single-crop pass -- the
    test AvaIndex (built under AVA.FULL_EVAL = FULL_EVAL_DURING_TRAINING, DETECTION_SCORE_THRESH = _TRAIN), centre crop,
    add_ava_batch(metadata, original_boxes) per iteration.  Under a process group the pass is shared by the ranks
    (a counted passes.run_pass is run_pass_ranks there) and every rank ends with the same figures.  -> (global) iterations run"""
    from datasets import ava
    meter, loader = test.meter, test.loader
    meter.reset()
    logger.info("=> Testing model")
    total = misc.get_total_test_iters(test.index)
    if cfg.DATASET == 'ava':
        # (its own generator: the training loader's thread draws from np.random while this pass runs)
        source = ava.minibatch_source(test.index, test.store, np.random.RandomState(cfg.RNG_SEED) if rng is None else rng,
                                      bank=loader.bank)
    else:
        source = lfb_pass.frame_minibatch_source(test.index, test.store, test.bank_video)

    def score(it, mb):
        if cfg.DATASET == 'ava' and meter.meter is not None and mb is not None:
            meter.add_ava_batch(mb.metadata[:, :2], mb.original_boxes)
        meter.calculate_and_log_all_metrics_test(it, test.timer, total, test.suffix)
    ran = passes.run_pass(test.engine, loader, test.store, source, total, test.timer, score)
    if cfg.DATASET == 'ava' and meter.ava_groundtruth is None:
        meter.full_map = 0.0                             # (no annotation files were given: nothing to score against)
    else:
        meter.finalize_metrics(name=name)
    meter.compute_and_log_best()
    meter.log_final_metrics(curr_iter if curr_iter is not None else ran - 1, None if curr_iter is not None else total)
    return ran


def train(make_store, dtype="mix", bank_dtype="bf16", device="cuda:0", ava_groundtruth=None, excluded_keys=(),
          class_whitelist=None, categories=None, n_slots=2, max_src_hw=(256, 340), train_lfb=None, test_lfb=None, init_params=None,
          on_eval=None, eval_dtype=None):
    """Train a model (train_net.py:93-212).  make_store(device, stream) -> the FrameStore (with its fetch) of a loader.
    train_lfb / test_lfb: banks already built (default with LFB.ENABLED: lfb_pass.get_lfb for test, then train);
    init_params(train_engine): sets the initial parameters (default: the recorded fillers, Engine.init_params);
    on_eval(curr_iter, train_wrapper, test_wrapper, json_stats): called after every evaluation;
    eval_dtype: the dtype of the forward-only engines -- bank inference, the test engine, test_net (default: `dtype`, and
    "bf16", the default of the test passes, where that is "mix": `mix` is a training path).
    Under a process group (one process per GPU): the module docstring.  TRAIN.COMPUTE_PRECISE_BN, and TRAIN.TEST_AFTER_TRAIN on
    AVA (the multi-crop pass), are single-process and are refused before anything is built.
    -> dict(last_checkpoint=, json_stats=[...], train=, test=, bn_aux=, eval_iters=[...], final=)"""
    import torch
    from utils import checkpoints
    import utils.metrics as metrics
    from vlfb import test_pass

    grouped = dist.initialized()
    lfb_pass.check_world()
    if grouped and cfg.TRAIN.COMPUTE_PRECISE_BN:
        raise NotImplementedError("train: TRAIN.COMPUTE_PRECISE_BN under a process group (%d ranks): the precise-BN pass is "
                                  "single-process; unset it" % dist.world_size())
    if grouped and cfg.TRAIN.TEST_AFTER_TRAIN and cfg.DATASET == 'ava':
        raise NotImplementedError("train: TRAIN.TEST_AFTER_TRAIN on AVA under a process group (%d ranks): the multi-crop test "
                                  "pass is single-process; unset it and run test_net on the last checkpoint" % dist.world_size())
    lead = dist.rank() == 0

    # Generate seed.
    misc.generate_random_seed()
    rng = random.Random(cfg.RNG_SEED)
    checkpoint_dir = checkpoints.create_and_get_checkpoint_directory()
    logger.info('Checkpoint directory created: {}'.format(checkpoint_dir))

    # Setting training-time-specific configurations (put back when the loop ends; test_net sets its own).
    before = (cfg.AVA.get("FULL_EVAL"), cfg.AVA.get("DETECTION_SCORE_THRESH"), cfg.CHARADES.get("NUM_TEST_CLIPS"))
    cfg.AVA.FULL_EVAL = cfg.AVA.FULL_EVAL_DURING_TRAINING
    cfg.AVA.DETECTION_SCORE_THRESH = cfg.AVA.DETECTION_SCORE_THRESH_TRAIN
    cfg.CHARADES.NUM_TEST_CLIPS = cfg.CHARADES.NUM_TEST_CLIPS_DURING_TRAINING

    if eval_dtype is None:
        eval_dtype = "bf16" if dtype == "mix" else dtype
    if cfg.LFB.ENABLED:
        kw = dict(dtype=eval_dtype, bank_dtype=bank_dtype, device=device, n_slots=n_slots, max_src_hw=max_src_hw)
        if test_lfb is None:
            test_lfb = lfb_pass.get_lfb(cfg.LFB.MODEL_PARAMS_FILE, False, make_store, **kw)
        if train_lfb is None:
            train_lfb = lfb_pass.get_lfb(cfg.LFB.MODEL_PARAMS_FILE, True, make_store, **kw)

    common = dict(device=device, n_slots=n_slots, max_src_hw=max_src_hw)
    # The train engine owns the parameters; the test engine aliases them (module docstring).
    tr = create_wrapper(True, make_store, train_lfb, dtype=dtype, **common)
    if init_params is None:
        tr.engine.init_params()
    else:
        init_params(tr.engine)
    te = create_wrapper(False, make_store, test_lfb, owner=tr.engine, ava_groundtruth=ava_groundtruth, excluded_keys=excluded_keys,
                        class_whitelist=class_whitelist, categories=categories, dtype=eval_dtype, **common)
    total_test_iters = misc.get_total_test_iters(te.index)
    logger.info('Test iters: {}'.format(total_test_iters))

    bn_aux, aux = None, []
    out = dict(last_checkpoint=None, json_stats=[], train=tr, test=te, bn_aux=None, eval_iters=[], final=None)
    try:
        if cfg.TRAIN.COMPUTE_PRECISE_BN:
            from vlfb.precise_bn import PreciseBN

            def make_loader(engine, suffix):
                loader = passes.make_loader(engine, suffix, 1 if cfg.TRAIN.DATA_TYPE == "train" else 0, tr.loader.bank, n_slots,
                                            max_src_hw, device)
                w = tr._replace(loader=loader, store=make_store(loader.device, loader.stream))
                aux.append(w)
                # its own walk over the training split, as the reference's bn_aux model has its own data loader
                loader.start(train_source(w, random.Random(cfg.RNG_SEED + 1), np.random.RandomState(cfg.RNG_SEED + 1)))
                return loader
            bn_aux = out["bn_aux"] = PreciseBN(tr.engine, make_loader)

        # Load checkpoint or pre-trained weight.
        start_model_iter = 0
        if cfg.CHECKPOINT.RESUME or cfg.TRAIN.PARAMS_FILE:
            start_model_iter = checkpoints.load_model_from_params_file(tr.model)
        out["start_model_iter"] = start_model_iter
        if grouped:
            tr.engine.enable_data_parallel()                 # rank 0's parameters on every rank; reduced gradients from here on

        logger.info("------------- Training model... -------------")
        tr.meter.reset()
        last_checkpoint = checkpoints.get_checkpoint_resume_file()
        unlogged = []                                        # losses the guard read since the meter's last line
        tr.loader.start(rank_train_source(tr) if grouped else train_source(tr, rng, np.random))
        for curr_iter in range(start_model_iter, cfg.SOLVER.MAX_ITER):
            tr.model.UpdateWorkspaceLr(curr_iter)            # lr_policy.get_lr_at_iter, and the momentum correction
            tr.timer.tic()
            tr.loader.deliver(tr.loader.next())
            tr.engine.train_step(float(tr.model.current_lr))
            tr.timer.toc()

            # the NaN guard reads the device loss ring, one synchronisation: at the iterations the meter reads it anyway
            # (LOG_PERIOD), at least once per ring, and before anything is saved or evaluated
            saves = (curr_iter + 1) % cfg.CHECKPOINT.CHECKPOINT_PERIOD == 0 or curr_iter + 1 == cfg.SOLVER.MAX_ITER
            evals = (curr_iter + 1) % cfg.TRAIN.EVAL_PERIOD == 0
            logs = (curr_iter + 1) % cfg.LOG_PERIOD == 0
            if logs or saves or evals or (curr_iter + 1 - start_model_iter) % 64 == 0:
                # (under a group the guard's one collective also sums the ranks' losses: sum_multi_gpu_blob('loss'))
                unlogged.extend(misc.check_nan_losses(tr.model, sum_ranks=grouped))

            # Checkpoint.
            if saves:
                if bn_aux is not None:
                    bn_aux.compute_and_update_bn_stats(curr_iter)
                last_checkpoint = os.path.join(checkpoint_dir, 'c2_model_iter{}.pkl'.format(curr_iter + 1))
                if not grouped:
                    checkpoints.save_model_params(model=tr.model, params_file=last_checkpoint, model_iter=curr_iter)
                else:                                        # rank 0 writes; nobody goes on before the file is there
                    lfb_pass._on_every_rank(lambda: lead and checkpoints.save_model_params(
                        model=tr.model, params_file=last_checkpoint, model_iter=curr_iter))
                    dist.barrier()

            if logs:
                tr.meter.calculate_and_log_all_metrics_train(curr_iter, tr.timer, suffix='_train', losses=list(unlogged))
                del unlogged[:]

            # Evaluation.
            if evals:
                if bn_aux is not None:
                    bn_aux.compute_and_update_bn_stats(curr_iter)
                ran = eval_pass(te, curr_iter=curr_iter)
                out["eval_iters"].append(ran)
                # Finalize and reset train_meter after test.
                if cfg.DATASET == 'ava':
                    tr.meter.full_map = 0.0              # (no mAP while training; the train meter holds no annotation files)
                else:
                    tr.meter.finalize_metrics(is_train=True)
                json_stats = metrics.get_json_stats_dict(tr.meter, te.meter, curr_iter)
                if grouped:                                  # (used_gpu_memory is a rank's own: the line is rank 0's)
                    json_stats = dist.broadcast_object(json_stats)
                if lead:
                    misc.log_json_stats(json_stats)
                out["json_stats"].append(json_stats)
                if on_eval is not None:
                    on_eval(curr_iter, tr, te, json_stats)
                tr.meter.reset()
        out["last_checkpoint"] = last_checkpoint
    finally:
        tr.loader.stop()
        te.loader.stop()
        for w in aux:
            w.loader.stop()
        for part, key, value in ((cfg.AVA, "FULL_EVAL", before[0]), (cfg.AVA, "DETECTION_SCORE_THRESH", before[1]),
                                 (cfg.CHARADES, "NUM_TEST_CLIPS", before[2])):
            if value is None:
                part.pop(key, None)
            else:
                part[key] = value
    torch.cuda.current_stream().synchronize()

    if cfg.TRAIN.TEST_AFTER_TRAIN:
        kw = dict(dtype=eval_dtype, device=device)
        if cfg.DATASET != 'ava':
            kw.update(n_slots=n_slots, max_src_hw=max_src_hw)
        cfg.TEST.PARAMS_FILE = out["last_checkpoint"]
        out["final"] = test_pass.test_net(out["last_checkpoint"], make_store, lfb=test_lfb, ava_groundtruth=ava_groundtruth,
                                          excluded_keys=excluded_keys, class_whitelist=class_whitelist, **kw)
    return out
