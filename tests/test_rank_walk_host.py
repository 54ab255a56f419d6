"""Host side of a pass or a training walk shared by N ranks: the row formula that vlfb_rows_interleave implements and its
inverse (vlfb.metrics.global_row / rank_row / rank_rows), lfb_pass.rank_source on an endless source, and the split of
ava.minibatch_source's generator into a walk generator and an augmentation generator.  No GPU."""
import collections
import itertools

import numpy as np
import pytest

import clip_loader_cases as cases


@pytest.mark.parametrize("world", [1, 2, 3, 4])
@pytest.mark.parametrize("b", [1, 2, 3, 5])
def test_global_row_formula_and_its_inverse(world, b):
    """slice s of the walk (rows s * b .. s * b + b - 1 of the stream) is the (s // world)-th slice of rank s % world"""
    from vlfb.metrics import global_row, rank_row, rank_rows
    slices = 3 * world + 1
    seen = []
    for s in range(slices):
        rank, k = s % world, s // world
        for j in range(b):
            g = s * b + j
            assert rank_row(g, b, world) == (rank, k * b + j)
            assert global_row(rank, k * b + j, b, world) == g
            seen.append(g)
    assert seen == list(range(slices * b))
    # numpy arrays go through the same expressions
    g = np.arange(slices * b)
    rank, row = rank_row(g, b, world)
    assert np.array_equal(global_row(rank, row, b, world), g)
    # the rows asked of each rank for every prefix of the stream: what the kernel checks the parts against
    for total in range(slices * b + 1):
        want = [0] * world
        for t in range(total):
            want[rank_row(t, b, world)[0]] += 1
        assert rank_rows(total, b, world) == want
        for r in range(world):
            last = [rank_row(t, b, world)[1] for t in range(total) if rank_row(t, b, world)[0] == r]
            assert want[r] == (max(last) + 1 if last else 0)            # a rank's rows are a prefix of its table


@pytest.mark.parametrize("world", [1, 2, 3])
def test_rank_source_without_an_end(world):
    from vlfb.lfb_pass import rank_iterations, rank_source
    drawn = []

    def counting():
        for i in itertools.count():
            drawn.append(i)
            yield i
    for rank in range(world):
        del drawn[:]
        got = list(itertools.islice(rank_source(counting(), None, rank, world), 5))
        assert got == [rank + k * world for k in range(5)]
        assert drawn == list(range(got[-1] + 1))                         # the skipped items were drawn, none beyond the last
        # the finite form picks the same items
        assert list(rank_source(iter(range(11)), 11, rank, world)) == rank_iterations(11, rank, world)
    with pytest.raises(AssertionError):
        list(rank_source(iter(range(4)), 3, 0, world))


Info = collections.namedtuple("Info", "video sec center seq boxes labels shift lfb_slots")


class StubIndex(object):
    """what ava.minibatch_source asks of an AvaIndex: 7 keyframes; in train the keyframe is drawn, as AvaIndex does"""

    def __init__(self, split, n):
        self.split, self.batch_size, self.calls = split, n, []

    def get_db_size(self):
        return 7

    def get_minibatch_info(self, indices, rng=np.random, bank_counts=None, step_base=902):
        out = []
        for i in indices:
            if self.split == "train":
                i = int(rng.choice(range(7)))
            out.append(Info(i, 902 + i, 0, [i, i + 1], [[0.1, 0.1, 0.5, 0.5]], [[1 + i % 3]], None, None))
        self.calls.append([c.video for c in out])
        return out


def _walk(split, steps, rng, aug_rng):
    from datasets import ava
    index = StubIndex(split, 2)
    src = ava.minibatch_source(index, "store", rng, bank=None, aug_rng=aug_rng)
    items = list(itertools.islice(src, steps))
    return items, index.calls


@pytest.mark.parametrize("split", ["train", "val"])
def test_ava_source_walks_alike_with_and_without_its_own_augmentation_generator(split):
    with cases.loader_cfg("ava_r50_baseline", clips=2):
        steps = 9 if split == "train" else 4                               # (train: into the third shuffled pass)
        plain_rng = np.random.RandomState(7)
        plain, plain_calls = _walk(split, steps, plain_rng, None)
        walk_rng, aug = np.random.RandomState(7), np.random.RandomState(8)
        split_, split_calls = _walk(split, steps, walk_rng, aug)
        assert len(plain) == len(split_) == steps
        assert plain_calls == split_calls
        for a, b in zip(plain, split_):
            assert a[0] == b[0] and a[3] == b[3] and a[5] == b[5]          # clips, meta, shift
            assert all(np.array_equal(x, y) for x, y in zip(a[1], b[1]))
            assert all(np.array_equal(x, y) for x, y in zip(a[2], b[2]))
            assert a[4] is plain_rng and b[4] is aug                      # only the yielded generator differs
        # the walk consumed its generator alike; the augmentation generator was never drawn from by the source
        assert plain_rng.randint(1 << 30) == walk_rng.randint(1 << 30)
        assert aug.randint(1 << 30) == np.random.RandomState(8).randint(1 << 30)
        if split == "train":
            # what the ranks of a job rely on: a consumer that draws from the yielded generator between items does not
            # move the walk when that generator is its own
            index = StubIndex(split, 2)
            from datasets import ava
            walk_rng, aug = np.random.RandomState(7), np.random.RandomState(8)
            src = ava.minibatch_source(index, "store", walk_rng, aug_rng=aug)
            for _ in range(steps):
                next(src)[4].uniform(size=3)
            assert index.calls == plain_calls
