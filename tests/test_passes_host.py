"""Host side of vlfb.passes (no GPU): the one table of input shapes against the shapes written out here for every
combination its callers produce, in the model's blob order; most_boxes; the EPIC rule of bank_kind / bank_video."""
import types

import pytest

import clip_loader_cases as cases

N, T, CROP = 2, 4, cases.CROP
WINDOW = 4
DATA = (2, 3, 4, 64, 64)


def _model(sfx, *kinds):
    return types.SimpleNamespace(input_blob_names=[k + sfx for k in kinds])


# preset, blob kinds in the model's order, RoI rows (AVA), the shapes in that order: AVA rows x 80 classes, rows x 5,
# rows x (WINDOW * 5 per step) x 2048; Charades 157 multi-hot classes per clip; EPIC one class id per clip; frame-level
# banks clips x WINDOW x 2048
SHAPES = {
    "ava_baseline": ("ava_r50_baseline", ["data", "labels", "proposals"], 6, [DATA, (6, 80), (6, 5)]),
    "ava_lfb": ("ava_r50_lfb_nl", ["data", "lfb", "labels", "proposals"], 6, [DATA, (6, 20, 2048), (6, 80), (6, 5)]),
    "ava_lfb_infer_only": ("ava_r50_lfb_nl", ["proposals", "data", "labels"], 10, [(10, 5), DATA, (10, 80)]),
    "charades_baseline": ("charades_r50_baseline", ["data", "labels"], None, [DATA, (2, 157)]),
    "charades_lfb": ("charades_r50_lfb_nl", ["labels", "lfb", "data"], None, [(2, 157), (2, 4, 2048), DATA]),
    "epic_baseline": ("epic_verb_r50_baseline", ["data", "labels"], None, [DATA, (2,)]),
    "epic_lfb": ("epic_noun_r50_lfb_nl", ["data", "labels", "lfb"], None, [DATA, (2,), (2, 4, 2048)]),
}


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_input_shapes_are_the_shapes_the_loaders_assert_in_the_model_s_order(name):
    from vlfb import passes
    preset, kinds, rows, want = SHAPES[name]
    sfx = "_infer_train" if name == "ava_lfb_infer_only" else "_test"
    with cases.loader_cfg(preset, clips=N, frames=T, extra=["LFB.WINDOW_SIZE", WINDOW]) as cfg:
        assert (cfg.LFB.LFB_DIM, cfg.AVA.LFB_MAX_NUM_FEAT_PER_STEP) == (2048, 5)
        got = passes.input_shapes(_model(sfx, *kinds), sfx, N, T, CROP, rows)
        assert list(got.items()) == [(k + sfx, shape) for k, shape in zip(kinds, want)]
        assert all(type(shape) is tuple for shape in got.values())
        with pytest.raises(KeyError):
            passes.input_shapes(_model(sfx, "data", "boxes"), sfx, N, T, CROP, rows)
        if rows is None:
            with pytest.raises(KeyError):                          # a frame-level plan has no proposals
                passes.input_shapes(_model(sfx, "data", "proposals"), sfx, N, T, CROP)


def test_input_shapes_takes_the_bank_window_it_is_given():
    """the multi-crop tester plans `lfb` with the shape of the rows it is fed"""
    from vlfb import passes
    with cases.loader_cfg("ava_r50_lfb_nl", clips=N, frames=T):
        got = passes.input_shapes(_model("_final_test", "data", "lfb"), "_final_test", N, T, CROP, 3, lfb_shape=[3, 7, 16])
        assert list(got.items()) == [("data_final_test", DATA), ("lfb_final_test", (3, 7, 16))]


def test_most_boxes():
    from vlfb import passes
    boxes = {0: {902: [1, 2], 903: [1, 2, 3, 4], 904: [1] * 9}, 1: {902: [], 910: [1, 2, 3]}}
    index = types.SimpleNamespace(boxes_and_labels=boxes, keyframe_indices=[(0, 902, 0), (0, 903, 1), (1, 902, 2), (1, 910, 3)])
    assert passes.most_boxes(index) == 4                           # (0, 904) has more, and is no keyframe of the index
    index.keyframe_indices = [(1, 902, 0)]
    assert passes.most_boxes(index) == 0


@pytest.mark.parametrize("preset, kind, by_index", [("charades_r50_lfb_nl", "charades", False), ("epic_verb_r50_lfb_nl", "epic_verb", False),
                                                    ("epic_noun_r50_lfb_nl", "epic_noun", True)])
def test_bank_kind_and_bank_video(preset, kind, by_index):
    """only the EPIC noun bank is keyed by video index; the others by what the index calls the video"""
    from vlfb import passes
    index = types.SimpleNamespace(video_name_to_idx={"P01_01": 0, "P02_03": 1})
    with cases.loader_cfg(preset, clips=N, frames=T):
        assert passes.bank_kind() == kind
        to_bank = passes.bank_video(index)
        if by_index:
            assert [to_bank(v) for v in ("P02_03", "P01_01")] == [1, 0]
        else:
            assert to_bank is None
