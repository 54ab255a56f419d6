"""vlfb.passes.run_pass, the loop of the bank, test and evaluation passes, on the small engines of the loader tests: where it
ends, what it leaves of the loader when the source fails, and the `meta` its `each` is handed.  What the passes compute
through it is pinned by their own tests (test_ava_pass_gpu, test_frame_bank_pass_gpu, test_test_pass_gpu,
test_train_pass_gpu)."""
import numpy as np
import pytest

import clip_loader_cases as cases
import frame_pass_cases as fc

pytestmark = pytest.mark.gpu

SFX = "_final_test"
LENGTHS = [12, 9]


def _idle(loader):
    return loader._thread is None and all(s.state == "free" for s in loader.slots)


def _frame_source(store, items=3, fail_at=None):
    """`items` minibatches of fc.N clips of fc.T frames out of `store`, as lfb_pass.frame_minibatch_source lays them out; the
    metas it yielded are kept in .metas"""
    def source():
        for it in range(items):
            if it == fail_at:
                raise ValueError("frame list ends early")
            meta = dict(iteration=it, videos=[0, 1], centers=[it + 2, it + 3], padded=[False, False])
            source.metas.append(meta)
            yield [(store, v, list(range(it, it + fc.T))) for v in (0, 1)], [[it], [it + 1]], meta, None, [1, 1]
    source.metas = []
    return source


def test_run_pass_ends_with_the_source_or_the_count_and_survives_a_failing_source():
    from datasets.clip_loader import FrameLoader
    from vlfb import passes
    vids = fc.videos(LENGTHS, seed=3)
    with cases.loader_cfg("charades_r50_baseline", clips=fc.N, frames=fc.T, extra=fc.EXTRA):
        _, eng, _ = fc.engine(SFX)
        loader = FrameLoader(eng, SFX, 0, n_slots=2, max_src_hw=(fc.H, fc.W), src_sizes=[(fc.H, fc.W)])
        store = fc.store_factory(lambda v, f: vids[v][f])(loader.device, loader.stream)

        # (a) until the source ends; exactly the iterations asked for
        seen, timer = [], passes.Timer()
        src = _frame_source(store)
        assert passes.run_pass(eng, loader, store, src(), timer=timer, each=lambda it, mb: seen.append((it, mb.meta))) == 3
        assert _idle(loader) and timer.calls == 3
        # (c) each gets the iteration and the Minibatch, whose meta is the dict the source yielded
        assert [it for it, _ in seen] == [0, 1, 2] and all(got is want for (_, got), want in zip(seen, src.metas))
        its = []
        assert passes.run_pass(eng, loader, store, _frame_source(store)(), iterations=2, each=lambda it, mb: its.append(it)) == 2
        assert _idle(loader) and its == [0, 1]
        with pytest.raises(StopIteration):                         # a count the source cannot serve is not cut short silently
            passes.run_pass(eng, loader, store, _frame_source(store, items=1)(), iterations=2)
        assert _idle(loader)

        # (b) the source fails while producing its second item: raised here, the loader stopped and fit for the next pass
        its = []
        with pytest.raises(ValueError, match="frame list ends early"):
            passes.run_pass(eng, loader, store, _frame_source(store, fail_at=1)(), each=lambda it, mb: its.append(it))
        assert its == [0] and _idle(loader)
        assert passes.run_pass(eng, loader, store, _frame_source(store)()) == 3
        assert _idle(loader)


def test_each_gets_the_meta_of_a_minibatch_loader_too():
    """the AVA loader: an ava_r50_baseline lfb_infer_only engine at the 8 frames the AVA tests plan it with, one RoI per clip"""
    from datasets.clip_loader import MinibatchLoader
    from models.model_builder_video import ModelBuilder
    from vlfb import passes, synth
    from vlfb.engine import Engine
    sfx, frames = "_infer_test", 8
    vids = fc.videos(LENGTHS, seed=4)
    with cases.loader_cfg("ava_r50_baseline", clips=fc.N, frames=frames) as cfg:
        m = ModelBuilder(train=False, split="test", name="infer")
        m.build_model(suffix=sfx, lfb_infer_only=True, shift=1)
        eng = Engine(m, "bf16", device="cuda:0", base_seed=2)
        eng.plan(passes.input_shapes(m, sfx, fc.N, frames, cases.CROP, rows=fc.N))
        eng.feed_params({k: v for k, v in synth.params(m, seed=2).items() if k in eng.param_views})
        loader = MinibatchLoader(eng, sfx, 0, n_slots=2, max_src_hw=(fc.H, fc.W), src_sizes=[(fc.H, fc.W)])
        store = fc.store_factory(lambda v, f: vids[v][f])(loader.device, loader.stream)
        labels = [np.zeros((1, cfg.MODEL.NUM_CLASSES), np.int32)] * fc.N
        metas = [dict(iteration=it, videos=[0, 1], secs=[902 + it, 903], padded=[False, False]) for it in range(2)]
        source = (([(store, v, list(range(it, it + frames))) for v in (0, 1)], cases.boxes(it, [1, 1]), labels, metas[it],
                   np.random.RandomState(it), 1) for it in range(2))
        seen = []
        assert passes.run_pass(eng, loader, store, source, each=lambda it, mb: seen.append(mb.meta)) == 2
        assert len(seen) == 2 and seen[0] is metas[0] and seen[1] is metas[1]
        assert _idle(loader)
