"""Host side of the frame-level passes (no GPU): the index constructors read the files the reference's _get_data reads, the
append keys of a pass, the iteration count, and the dispatch of lfb_pass.get_lfb / test_pass.test_net."""
import os

import numpy as np
import pytest

import clip_loader_cases as cases
import frame_pass_cases as fc


def test_charades_index_from_cfg_reads_the_split_s_lists(tmp_path):
    from datasets import charades
    with cases.loader_cfg("charades_r50_baseline", clips=2, frames=4, extra=fc.EXTRA) as cfg:
        fc.point_cfg_at(cfg, tmp_path)
        fc.write_charades_lists(tmp_path, [60, 23], [[[k % 3] for k in range(60)], [[]] * 23])
        os.rename(os.path.join(str(tmp_path), "frames.csv"), os.path.join(str(tmp_path), "val.csv"))
        fc.write_charades_lists(tmp_path, [30])
        cfg.CHARADES.TRAIN_LISTS, cfg.CHARADES.TEST_LISTS = ["frames.csv"], ["val.csv"]
        test = charades.CharadesIndex.from_cfg("test", True)
        assert test.num_frames == [60, 23] and test.get_db_size() == 6 and test.lfb_frames[-1] == (1, 11)
        assert test.video_idx_to_name == {0: "V0", 1: "V1"} and test.image_paths[1][22] == "V1/000023.jpg"
        assert sorted(test.labels[0][5]) == [0, 1, 2] and test.labels[1][0] == []      # video-level labels outside train
        for index in (charades.CharadesIndex.from_cfg("test", True, get_train_lfb=True), charades.CharadesIndex.from_cfg("train", False)):
            assert index.num_frames == [30]                        # the train lists, as with the reference's cfg.GET_TRAIN_LFB


def test_epic_index_from_cfg_reads_lists_and_annotations(tmp_path):
    from datasets import epic
    with cases.loader_cfg("epic_verb_r50_baseline", clips=2, frames=4, extra=fc.EXTRA + ["EPIC.VERB_LFB_CLIPS_PER_SECOND", 3]) as cfg:
        fc.point_cfg_at(cfg, tmp_path)
        fc.write_epic_lists(tmp_path, ["P26_01", "P01_02"], [35, 25])
        fc.write_epic_annotations(tmp_path, [("P26", "P26_01", 0.1, 0.5, 3, 17), ("P01", "P01_02", 0.2, 0.6, 7, 9),
                                             ("P26", "P26_01", 0.4, 1.0, 120, 351)])
        bank = epic.EpicIndex.from_cfg("test", True, shift=1)
        assert [(a[1], a[2]) for a in bank.annotations] == [("P26_01", 10), ("P26_01", 20), ("P26_01", 30), ("P01_02", 10), ("P01_02", 20)]
        assert list(bank.image_paths) == ["P26_01", "P01_02"] and bank.video_name_to_idx == {"P26_01": 0, "P01_02": 1}
        test = epic.EpicIndex.from_cfg("test", False)
        assert [a[:2] + a[4:] for a in test.annotations] == [("P26", "P26_01", 3, 17), ("P26", "P26_01", 120, 351)]
        assert test.annotations[0][2:4] == (3, 15) and test.get_minibatch_info([1])[0].labels == 120
        train = epic.EpicIndex.from_cfg("train", False)
        assert [a[1] for a in train.annotations] == ["P01_02"]


def test_pass_keys_iterations_and_name_rows():
    from utils import misc
    from vlfb import hip, lfb_pass
    from vlfb.lfb_bank import DeviceBank
    if not os.path.exists(hip.LIB_PATH):
        pytest.skip("libvlfb_hip.so not built")
    with cases.loader_cfg("epic_verb_r50_baseline", clips=2, frames=4, extra=["EPIC.VERB_LFB_CLIPS_PER_SECOND", 3]) as cfg:
        bank = DeviceBank(2, 4, 1, 8, "f32", device="cpu", video_ids=["P01_01", "P02_03"])
        keys = bank.epic_frame_keys(3, [("P02_03", 20), ("P01_01", 0)], 10)
        assert keys.dtype == np.int32 and keys.tolist() == [[1, 2], [0, 0], [-1, 0]]
        assert bank._rows_of(["P02_03", "nobody", -1]).tolist() == [1, -1, -1]
        with pytest.raises(AssertionError, match="LFB frames"):
            bank.epic_frame_keys(1, [("P01_01", 15)], 10)
        meta = dict(videos=["P01_01", "P01_01"], centers=[30, 30], padded=[False, True])
        assert lfb_pass.frame_pass_keys(bank, "epic_verb", meta, 2).tolist() == [[0, 3], [-1, 0]]
        assert lfb_pass.frame_sample_freq() == 10
        cfg.TEST.BATCH_SIZE = 2
        db = type("Index", (), {"get_db_size": lambda self: 5})()
        assert misc.get_total_test_iters(db) == 3 and misc.get_total_test_iters(type("M", (), {"input_db": db})()) == 3
    with cases.loader_cfg("charades_r50_baseline", clips=2, frames=4) as cfg:
        plain = DeviceBank(2, 5, 1, 8, "f32", device="cpu")
        meta = dict(videos=[1, 1], centers=[23, 23], padded=[False, True])
        assert lfb_pass.frame_pass_keys(plain, "charades", meta, 2).tolist() == [[1, 1], [-1, 0]]
        assert lfb_pass.frame_sample_freq() == 12


def test_the_epic_noun_bank_has_no_inference_pass():
    from vlfb import lfb_pass
    with cases.loader_cfg("epic_noun_r50_lfb_nl", clips=2, frames=4) as cfg:
        cfg.LFB.LOAD_LFB = False
        with pytest.raises(NotImplementedError, match="detector"):
            lfb_pass.get_lfb("baseline.pkl", True, None)
        with pytest.raises(NotImplementedError, match="detector"):
            lfb_pass.write_lfb(None, True)


def test_test_net_dispatch_for_ava(monkeypatch):
    from vlfb import multicrop, test_pass
    with cases.loader_cfg("ava_r50_baseline", clips=2, frames=4) as cfg:
        cfg.AVA.TEST_MULTI_CROP = False
        with pytest.raises(NotImplementedError, match="single-crop"):
            test_pass.test_net("model.pkl", None)
        cfg.AVA.TEST_MULTI_CROP = True
        cfg.LFB.WRITE_LFB = True
        seen = {}
        monkeypatch.setattr(multicrop, "run_ava_multi_crop", lambda *a, **kw: seen.update(args=a, kw=kw) or "results")
        gt = ({}, {}, {})
        assert test_pass.test_net("model.pkl", "make_store", ava_groundtruth=gt, class_whitelist=[3], out_csv="out.csv") == "results"
        assert seen["args"] == ("model.pkl", "make_store", gt, (), [3]) and seen["kw"] == dict(bank=None, out_csv="out.csv")
        assert cfg.LFB.WRITE_LFB is False and cfg.LFB.LOAD_LFB is False
