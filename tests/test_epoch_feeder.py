"""EpochFeeder (pose6d/store.py): the reference DataLoader's epoch order
(torch.utils.data.RandomSampler under the same torch seed), rank sharding, the
last batch, and -- on the GPU -- one epoch against LineMODSet.batch uncached on the
same indices and the same jitter rng state, bit for bit."""
import numpy as np
import pytest
import torch
from torch.utils.data import RandomSampler

from tests.synth import write_linemod_tree


def _store(n):
    from pose6d.store import FrameStore
    rng = np.random.default_rng(n)
    z = np.zeros
    return FrameStore.from_arrays(z((1, 4, 4, 3), np.uint8), None, z(n, np.int64), rng.integers(1, 9, (n, 4)),
                                  z((n, 9), np.float32), z((n, 4), np.float32), z((n, 3), np.float32), np.arange(n),
                                  rgbd=True, device="cpu")


def _epoch(feeder):
    return [b.tolist() for b in feeder.index_batches()]


# ----------------------------------------------------------------- CPU
@pytest.mark.parametrize("n", [1, 7, 100])
def test_shuffled_order_is_random_samplers(n):
    from pose6d.store import EpochFeeder
    g, g_ref = torch.Generator().manual_seed(11), torch.Generator().manual_seed(11)
    feeder = EpochFeeder(_store(n), 1, drop_last=False, generator=g)
    sampler = RandomSampler(range(n), generator=g_ref)
    for _ in range(3):   # the generator advances from epoch to epoch as the sampler's does
        assert sum(_epoch(feeder), []) == list(sampler)
    # generator=None: the epoch seed is drawn from torch's default generator, like the sampler's
    torch.manual_seed(5)
    got = sum(_epoch(EpochFeeder(_store(n), 1, drop_last=False)), [])
    torch.manual_seed(5)
    assert got == list(RandomSampler(range(n)))
    assert sum(_epoch(EpochFeeder(_store(n), 1, shuffle=False, drop_last=False)), []) == list(range(n))


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("drop_last", [True, False])
def test_rank_shards_are_disjoint_and_cover_the_prefix(world, drop_last):
    from pose6d.store import EpochFeeder
    n, B = 50, 4
    one = sum(_epoch(EpochFeeder(_store(n), 1, drop_last=False, generator=torch.Generator().manual_seed(3))), [])
    shards = [_epoch(EpochFeeder(_store(n), B, drop_last=drop_last, rank=r, world=world,
                                 generator=torch.Generator().manual_seed(3))) for r in range(world)]
    G = B * world
    whole = n // G
    for r in range(world):
        f = EpochFeeder(_store(n), B, drop_last=drop_last, rank=r, world=world, generator=torch.Generator())
        assert len(f) == len(shards[r])
    assert all(len(s) >= whole and all(len(b) == B for b in s[:whole]) for s in shards)
    flat = [i for s in shards for b in s for i in b]
    assert len(flat) == len(set(flat))                       # disjoint
    for gb in range(whole + (0 if drop_last else 1)):       # rank r holds positions r::world of global batch gb
        glob = one[gb * G:(gb + 1) * G]
        for r in range(world):
            want = glob[r::world]
            assert (shards[r][gb] if gb < len(shards[r]) else []) == want
    assert sorted(flat) == sorted(one[:whole * G] if drop_last else one)
    assert all(len(s) == whole for s in shards) or not drop_last


def test_last_batch():
    from pose6d._lib import Pose6dError
    from pose6d.store import EpochFeeder
    s = _store(10)
    assert EpochFeeder(s, 4).drop_last                        # the default: a captured step has one batch size
    a = EpochFeeder(s, 4, shuffle=False)
    assert len(a) == 2 and _epoch(a) == [[0, 1, 2, 3], [4, 5, 6, 7]]
    b = EpochFeeder(s, 4, shuffle=False, drop_last=False)
    assert len(b) == 3 and _epoch(b) == [[0, 1, 2, 3], [4, 5, 6, 7], [8, 9]]
    with pytest.raises(Pose6dError, match="generator"):
        EpochFeeder(s, 4, world=2)
    with pytest.raises(Pose6dError):
        EpochFeeder(s, 4, rank=2, world=2, generator=torch.Generator())
    with pytest.raises(Pose6dError):
        EpochFeeder(s, 0)


def test_feeder_draws_the_jitter_and_makes_one_crop_call_per_batch(monkeypatch):
    """Host side of an epoch with the launch stubbed out: per batch one store.crop
    call carrying jitter_bboxes(host_bbox[idx], rgbd, rng), in the reference's draw
    order; no jitter for a set without augment_bbox; check() when the epoch ends."""
    from pose6d.data import jitter_bboxes
    from pose6d.store import EpochFeeder
    s = _store(10)
    calls, checks = [], []
    monkeypatch.setattr(s, "crop", lambda idx, ba, out=None, augment=None: calls.append((idx, ba, out, augment)) or out)
    monkeypatch.setattr(s, "check", lambda: checks.append(len(calls)))
    assert list(EpochFeeder(s, 4, shuffle=False)) == [None, None] and all(c[1] is None for c in calls)
    assert checks == [2]
    del calls[:]
    s.augment_bbox = True
    out = ("buffers",)
    feeder = EpochFeeder(s, 4, shuffle=False, drop_last=False, rng=np.random.RandomState(2), rgbd=False,
                         augment="aug").into(out)
    got = list(feeder)
    ref_rng = np.random.RandomState(2)
    assert [c[0].tolist() for c in calls] == [[0, 1, 2, 3], [4, 5, 6, 7], [8, 9]]
    for idx, ba, o, aug in calls:
        assert np.array_equal(ba, jitter_bboxes(s.host_bbox[idx], False, ref_rng)) and aug == "aug"
    # the short batch gets tensors of its own
    assert got == [out, out, None] and [c[2] for c in calls] == [out, out, None]


# ----------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("linemod_feed"))
    write_linemod_tree(root, n_frames=30)
    return root


@pytest.mark.gpu
@pytest.mark.parametrize("rgbd", [True, False])
def test_epoch_equals_uncached_batches(tree, rgbd):
    from pose6d.linemod import LineMODSet
    from pose6d.store import EpochFeeder
    ds, plain = LineMODSet(tree, "train", rgbd=rgbd), LineMODSet(tree, "train", rgbd=rgbd)
    del ds.all_data[-2:], plain.all_data[-2:]
    store = ds.cache("cuda")
    n = len(ds)
    assert n % 4 == 2                                          # the epoch ends in a short batch
    feeder = EpochFeeder(store, 4, drop_last=False, generator=torch.Generator().manual_seed(7),
                         rng=np.random.RandomState(5))
    order = list(RandomSampler(range(n), generator=torch.Generator().manual_seed(7)))
    ref_rng = np.random.RandomState(5)
    seen = []
    for k, batch in enumerate(feeder):
        idx = order[4 * k:4 * k + 4]
        ref = plain.batch(idx, "cuda", ref_rng)
        assert len(batch) == len(ref) == (8 if rgbd else 6)
        for i, (g, r) in enumerate(zip(batch, ref)):
            assert torch.equal(g, r), (k, i)
        q, t, ids = batch[3:6] if rgbd else batch[1:4]
        seen += [(int(i), tuple(v.tolist())) for i, v in zip(ids, t)]
    assert k == len(feeder) - 1 == n // 4 and len(batch[0]) == 2
    _, t, ids = ds.labels(ds.all_data)
    assert sorted(seen) == sorted((int(i), tuple(v.tolist())) for i, v in zip(ids, t))
    store.check()                                              # clean (the feeder already checked)


@pytest.mark.gpu
def test_into_leaves_each_batch_in_the_given_tensors(tree):
    from pose6d.linemod import LineMODSet
    from pose6d.store import EpochFeeder
    ds, plain = LineMODSet(tree, "train"), LineMODSet(tree, "train")
    store = ds.cache("cuda")
    out = tuple(torch.zeros_like(t) for t in store.crop([0, 1, 2, 3]))
    ptrs = [t.data_ptr() for t in out]
    feeder = EpochFeeder(store, 4, generator=torch.Generator().manual_seed(1), rng=np.random.RandomState(9)).into(out)
    order = list(RandomSampler(range(len(ds)), generator=torch.Generator().manual_seed(1)))
    ref_rng = np.random.RandomState(9)
    for k, batch in enumerate(feeder):
        assert batch is out and [t.data_ptr() for t in out] == ptrs
        for g, r in zip(out, plain.batch(order[4 * k:4 * k + 4], "cuda", ref_rng)):
            assert torch.equal(g, r)
    assert k + 1 == len(feeder) == len(ds) // 4
