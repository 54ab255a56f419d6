"""The test driver (reference: tools/test_net.py:48-168): `test_net` dispatches on the dataset, `test_one_crop` runs one
pass (vlfb.passes.run_pass) over the Charades / EPIC test split through the frame loader with the metrics accumulated on
the device.

    meter = test_net(cfg.TEST.PARAMS_FILE, make_store)          # make_store(device, stream) -> FrameStore with its fetch

Charades: CHARADES.NUM_TEST_CLIPS_FINAL_EVAL clips per video (3 shifts x 10 segments) merged by max into the score table,
mAP from the table.  EPIC: the centre crop of every annotated segment; top-1 / top-5 error, and the predictions kept for
vlfb.epic_eval.evaluate_actions (epic_predictions_<name>.pkl).  AVA: the multi-crop pass (vlfb.multicrop).
"""
import logging

import numpy as np

from core.config import config as cfg
from utils import misc
from vlfb import lfb_pass, passes
from vlfb.passes import Timer           # (test_pass.Timer: the name callers know it by)

logger = logging.getLogger(__name__)


def test_one_crop(params_file, make_store, lfb=None, shift=None, name='final', dtype="bf16", bank_dtype="bf16", device="cuda:0",
                  n_slots=2, max_src_hw=(256, 340), out_dir=None, keep_predictions=None):
    """One pass over the Charades / EPIC test split (test_net.py:96-168): the test-mode engine with the parameters of
    `params_file`, clips as frame lists into `make_store(device, stream)`, with LFB.ENABLED the bank `lfb` (a DeviceBank;
    default: lfb_pass.get_lfb) sampled per clip on the loader's stream, misc.get_total_test_iters iterations, the device
    meter read once per LOG_PERIOD, finalize_metrics(name=) and log_final_metrics.  `shift`: the spatial position of the EPIC
    crop (default TEST.CROP_SHIFT; a Charades index walks its three shifts itself).  keep_predictions (default: every
    single-label model) keeps the prediction rows for epic_predictions_<name>.pkl, written into `out_dir`; `name` is
    'final' for these datasets in the reference (get_test_name, test_net.py:171-181).
    -> the utils.metrics.MetricsCalculator"""
    import utils.metrics as metrics
    from datasets import charades, epic
    from utils import checkpoints
    assert cfg.DATASET in ('charades', 'epic'), "test_one_crop: the frame-level datasets (AVA: vlfb.multicrop)"
    assert params_file, 'No params files specified for testing model.'
    np.random.seed(cfg.RNG_SEED)
    if lfb is None and cfg.LFB.ENABLED:
        lfb = lfb_pass.get_lfb(cfg.LFB.MODEL_PARAMS_FILE, False, make_store, dtype=dtype, bank_dtype=bank_dtype, device=device,
                               n_slots=n_slots, max_src_hw=max_src_hw)
    logger.warning('Testing started...')
    split = cfg.TEST.DATA_TYPE or "test"
    if shift is None:
        shift = cfg.TEST.CROP_SHIFT
    if cfg.DATASET == 'charades':
        index = charades.CharadesIndex.from_cfg(split, False)
    else:
        index = epic.EpicIndex.from_cfg(split, False, shift=shift)
    suffix = '_final_test'
    p = passes.build(make_store, suffix, dtype, cfg.TEST.BATCH_SIZE // cfg.NUM_GPUS, cfg.TEST.VIDEO_LENGTH, cfg.TEST.CROP_SIZE,
                     split=split, name="test", bank=lfb, shift=shift, device=device, n_slots=n_slots, max_src_hw=max_src_hw)
    total_test_net_iters = misc.get_total_test_iters(index)
    keep = (not cfg.MODEL.MULTI_LABEL) if keep_predictions is None else bool(keep_predictions)
    test_meter = metrics.MetricsCalculator(p.engine, split, video_idx_to_name=index.video_idx_to_name, keep_predictions=keep)
    p.engine.init_params()
    checkpoints.load_model_from_params_file_for_test(p.model, params_file)
    timer = Timer()
    ran = passes.run_pass(
        p.engine, p.loader, p.store, lfb_pass.frame_minibatch_source(index, p.store, passes.bank_video(index)),
        total_test_net_iters, timer,
        lambda it, mb: test_meter.calculate_and_log_all_metrics_test(it, timer, total_test_net_iters, suffix))
    test_meter.finalize_metrics(name=name, out_dir=out_dir)
    test_meter.log_final_metrics(ran - 1, total_test_net_iters)
    return test_meter


def test_net(params_file, make_store, lfb=None, ava_groundtruth=None, excluded_keys=(), class_whitelist=None, out_csv=None,
             **kwargs):
    """tools/test_net.py:48-93.  Charades: CHARADES.NUM_TEST_CLIPS = NUM_TEST_CLIPS_FINAL_EVAL for the pass (put back
    afterwards), then test_one_crop; EPIC: test_one_crop on the centre crop; AVA with AVA.TEST_MULTI_CROP:
    vlfb.multicrop.run_ava_multi_crop (which needs `ava_groundtruth`, read_csv's triple; `kwargs` go to the pass that
    runs).  The AVA single-crop test pass is not built: NotImplementedError."""
    if cfg.DATASET == 'ava':
        if not cfg.AVA.TEST_MULTI_CROP:
            raise NotImplementedError("test_net: the AVA single-crop test pass is not built; set AVA.TEST_MULTI_CROP "
                                      "(vlfb.multicrop.run_ava_multi_crop)")
        from vlfb.multicrop import run_ava_multi_crop
        assert ava_groundtruth is not None, "the AVA multi-crop pass is scored against ava_groundtruth= (read_csv's triple)"
        cfg.LFB.WRITE_LFB = False
        cfg.LFB.LOAD_LFB = False
        if cfg.LFB.ENABLED and lfb is None:
            lfb = lfb_pass.get_lfb(cfg.LFB.MODEL_PARAMS_FILE, False, make_store)
        return run_ava_multi_crop(params_file, make_store, ava_groundtruth, excluded_keys, class_whitelist, bank=lfb,
                                  out_csv=out_csv, **kwargs)
    if cfg.DATASET != 'charades':
        return test_one_crop(params_file, make_store, lfb=lfb, **kwargs)
    had = "NUM_TEST_CLIPS" in cfg.CHARADES
    before = cfg.CHARADES.get("NUM_TEST_CLIPS")
    cfg.CHARADES.NUM_TEST_CLIPS = cfg.CHARADES.NUM_TEST_CLIPS_FINAL_EVAL
    try:
        return test_one_crop(params_file, make_store, lfb=lfb, **kwargs)
    finally:
        if had:
            cfg.CHARADES.NUM_TEST_CLIPS = before
        else:
            del cfg.CHARADES["NUM_TEST_CLIPS"]


# (pytest collects `test_*` callables of a module it imports into a test file: these are drivers, not tests)
test_one_crop.__test__ = False
test_net.__test__ = False
