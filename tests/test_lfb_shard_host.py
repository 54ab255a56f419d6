"""Sharding of the bank-construction pass over ranks (vlfb.lfb_pass.rank_iterations / rank_source), on the host: which
iterations of the single-process walk each rank runs, and that a rank's filtered source touches only the clips of its own
iterations while the AVA source's draws stay those of the single-process walk."""
import numpy as np
import pytest

import clip_loader_cases as cases
import frame_pass_cases as fc
import test_ava_pass_gpu as avap

WORLDS = (1, 2, 3, 8)
TOTALS = (0, 1, 7, 8, 9)


@pytest.mark.parametrize("world", WORLDS)
@pytest.mark.parametrize("total", TOTALS)
def test_rank_iterations_partition_the_walk(total, world):
    from vlfb.lfb_pass import rank_iterations
    shares = [rank_iterations(total, r, world) for r in range(world)]
    seen = [it for s in shares for it in s]
    assert len(seen) == len(set(seen)), "shares overlap"
    assert sorted(seen) == list(range(total))
    assert all(s == sorted(s) and len(set(s)) == len(s) for s in shares)
    sizes = [len(s) for s in shares]
    assert max(sizes) - min(sizes) <= 1
    assert all(it % world == r for r, s in enumerate(shares) for it in s)      # slice g of global batch b on gpu_g


def test_rank_iterations_refuses_a_rank_outside_the_world():
    from vlfb.lfb_pass import rank_iterations
    for bad in ((3, 2, 2), (3, -1, 2), (3, 0, 0), (-1, 0, 1)):
        with pytest.raises(AssertionError):
            rank_iterations(*bad)


class RecordingStore(object):
    """a FrameStore stand-in: records every fetch (the loader's; the sources only name frames)"""

    def __init__(self):
        self.fetches = []

    def fetch(self, video, frame):
        self.fetches.append((int(video), int(frame)))
        return None


def _consume(source):
    """what the loader does with a source's items: fetch every frame of every clip; -> the items"""
    items = []
    for item in source:
        for store, video, seq in item[0]:
            for f in seq:
                store.fetch(video, f)
        items.append(item)
    return items


def test_the_frame_source_of_a_rank_fetches_only_its_own_iterations(tmp_path):
    from datasets import charades
    from vlfb import lfb_pass
    with cases.loader_cfg("charades_r50_baseline", clips=fc.N, frames=fc.T, extra=fc.EXTRA) as cfg:
        fc.point_cfg_at(cfg, tmp_path)
        fc.write_charades_lists(tmp_path, [100, 60, 23])
        index = charades.CharadesIndex.from_cfg("test", True)
        total = lfb_pass.pass_iterations(index.get_db_size(), index.batch_size // cfg.NUM_GPUS)
        assert index.get_db_size() == 14 and total == 7
        whole_store = RecordingStore()
        whole = _consume(lfb_pass.frame_minibatch_source(index, whole_store))
        assert len(whole) == total
        for world in WORLDS:
            union = []
            for rank in range(world):
                store = RecordingStore()
                got = _consume(lfb_pass.rank_source(lfb_pass.frame_minibatch_source(index, store), total, rank, world))
                mine = lfb_pass.rank_iterations(total, rank, world)
                assert [g[2]["iteration"] for g in got] == mine
                want = [(v, f) for it in mine for _, v, seq in whole[it][0] for f in seq]
                assert store.fetches == want, (world, rank)
                for g, it in zip(got, mine):
                    assert g[2] == whole[it][2] and [c[1:] for c in g[0]] == [c[1:] for c in whole[it][0]]
                union += store.fetches
            assert sorted(union) == sorted(whole_store.fetches)


def _same_item(a, b):
    (fa, ba, la, ma, _, sa), (fb, bb, lb, mb, _, sb) = a, b
    return ([(v, list(s)) for _, v, s in fa] == [(v, list(s)) for _, v, s in fb] and ma == mb and sa == sb and
            all(np.array_equal(x, y) for x, y in zip(ba, bb)) and all(np.array_equal(x, y) for x, y in zip(la, lb)))


def test_the_ava_source_of_a_rank_keeps_the_draws_of_the_single_process_walk(tmp_path):
    """a training index draws a keyframe per clip (and shuffles per pass) from `rng`: the kept iterations of a rank see the
    tuples the unfiltered source yields at those iterations under the same seed, and fetch only their own clips"""
    from datasets import ava
    from vlfb import lfb_pass
    avap._write_inputs(tmp_path)
    with cases.loader_cfg("ava_r50_baseline", clips=avap.N, frames=avap.T) as cfg:
        avap._point_cfg_at(cfg, tmp_path)
        index = ava.AvaIndex.from_cfg("train", False)
        assert index.split == "train" and index.get_db_size() == 5
        total = 9
        whole_store = RecordingStore()
        whole = _consume(ava.minibatch_source(index, whole_store, np.random.RandomState(11), iterations=total))
        assert len(whole) == total
        assert len({tuple(v for _, v, _ in w[0]) + tuple(w[3]["secs"]) for w in whole}) > 1       # the draws differ
        for world in WORLDS:
            for rank in range(world):
                store = RecordingStore()
                src = ava.minibatch_source(index, store, np.random.RandomState(11), iterations=total)
                got = _consume(lfb_pass.rank_source(src, total, rank, world))
                mine = lfb_pass.rank_iterations(total, rank, world)
                assert [g[3]["iteration"] for g in got] == mine
                assert all(_same_item(g, whole[it]) for g, it in zip(got, mine)), (world, rank)
                assert store.fetches == [(v, f) for it in mine for _, v, seq in whole[it][0] for f in seq]
