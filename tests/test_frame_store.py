"""FrameStore (pose6d/store.py): the device-resident frames + annotation tables and
the index-gathered crop, pose6d_crop_rgbd_indexed / _train_indexed.

The yardstick is the contiguous path -- CropRGBD on the stacked frames plus
LineMODSet.labels, i.e. LineMODSet.batch uncached -- which tests/test_crop.py and
tests/test_augment.py pin to the oracle.  Every comparison is torch.equal.

CPU: the host range check (no launch), the tables from a synthetic LineMOD tree.
GPU: indexed == contiguous (RGB-D / RGB, jittered / stored boxes, BGR), the train
transform, the geometry corners at S = 8, 64-bit store offsets, indices read at
kernel time under graph replay, the cached LineMODSet.

There is deliberately no test that hands the kernel a bad device-side index: were
its guard wrong, the test would fault the GPU."""
import os

import numpy as np
import pytest
import torch

from tests.synth import write_linemod_tree

N_FRAMES = 40


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("linemod_store"))
    return root, write_linemod_tree(root, n_frames=N_FRAMES)


def _arrays(n_frames, n, H=24, W=32, seed=0, depth=True):
    rng = np.random.default_rng(seed)
    rgb = rng.integers(0, 256, (n_frames, H, W, 3), dtype=np.uint8)
    d = rng.integers(300, 1600, (n_frames, H, W)).astype(np.uint16) if depth else None
    frame_of = rng.integers(0, n_frames, n)
    bbox = np.stack([rng.integers(-3, W - 8, n), rng.integers(-3, H - 8, n), rng.integers(4, 16, n),
                     rng.integers(4, 16, n)], 1)
    K = np.tile(np.array([570.0, 0, W / 2, 0, 571.0, H / 2, 0, 0, 1], np.float32), (n, 1))
    q = rng.standard_normal((n, 4)).astype(np.float32)
    t = rng.standard_normal((n, 3)).astype(np.float32)
    ids = rng.integers(0, 15, n)
    return rgb, d, frame_of, bbox, K, q, t, ids


def _take(depth, frames):
    """depth[frames] of a uint16 device tensor (indexed through its int16 view)."""
    return depth.view(torch.int16)[frames].view(torch.uint16)


def _contiguous(store, idx, bbox_aug=None, augment=None):
    """The store's collated tuple for `idx` made the old way: CropRGBD on the stacked
    frames, the labels indexed on the host."""
    from pose6d.data import CropRGBD
    idx = torch.as_tensor(np.asarray(idx), dtype=torch.long, device=store.device)
    fo = store.frame_of[idx].long()
    bo = store.bbox[idx]
    ba = bo if bbox_aug is None else torch.as_tensor(np.asarray(bbox_aug), dtype=torch.int32, device=store.device)
    crop = CropRGBD(store.img_size, bgr=store.bgr, augment=augment)
    K = store.K[idx].reshape(-1, 3, 3)
    depth = None if store.depth is None else _take(store.depth, fo)
    rgb, depth, raw, center, Kc = crop(store.rgb[fo], depth, bo, ba, K)
    lab = (store.quat[idx], store.trans[idx], store.obj_id[idx])
    if store.rgbd:
        return (rgb, depth, raw) + lab + (center, Kc), crop
    return (rgb,) + lab + (store.center_tab[idx], K), crop


def _same(got, ref):
    assert len(got) == len(ref)
    for i, (g, r) in enumerate(zip(got, ref)):
        assert g.dtype == r.dtype and torch.equal(g, r), f"output {i}"


# ----------------------------------------------------------------- CPU
@pytest.mark.parametrize("bad", [[-1], [7], [0, 3, 7], [2, -5]])
def test_host_index_is_range_checked_before_any_launch(monkeypatch, bad):
    from pose6d import store as ST
    from pose6d._lib import Pose6dError
    reached = []
    monkeypatch.setattr(ST, "call", lambda name, *a: reached.append(name))
    s = ST.FrameStore.from_arrays(*_arrays(3, 7), device="cpu")
    assert len(s) == 7
    with pytest.raises(Pose6dError, match="outside"):
        s.crop(bad)
    with pytest.raises(Pose6dError, match="outside"):
        s.crop(torch.tensor(bad))
    assert reached == []


def test_tables_are_validated():
    from pose6d._lib import Pose6dError
    from pose6d.store import FrameStore
    a = list(_arrays(3, 5))
    a[2] = np.array([0, 1, 2, 3, 0])   # frame 3 of 3
    with pytest.raises(Pose6dError, match="frame_of"):
        FrameStore.from_arrays(*a, device="cpu")
    b = list(_arrays(3, 5))
    b[1] = b[1][:, :-1]
    with pytest.raises(Pose6dError, match="depth"):
        FrameStore.from_arrays(*b, device="cpu")


def test_decode_pool_is_sized_by_the_process_share():
    from pose6d.store import MAX_WORKERS, _decode_workers
    assert _decode_workers() == min(len(os.sched_getaffinity(0)), MAX_WORKERS)
    assert _decode_workers(1000) == MAX_WORKERS == 16 and _decode_workers(0) == 1


@pytest.mark.parametrize("rgbd", [True, False])
def test_tables_from_linemod_tree(tree, rgbd):
    from pose6d.linemod import LineMODSet
    from pose6d.store import FrameStore
    root, written = tree
    ds = LineMODSet(root, "val", rgbd=rgbd)
    s = FrameStore.from_linemod(ds, "cpu", workers=2)
    paths = [it["img_path"] for it in ds.all_data]
    assert s.n_frames == len(set(paths)) == len(s.paths) and len(s) == len(ds)
    assert (s.H, s.W) == (120, 160) and s.rgbd == rgbd and not s.augment_bbox
    assert (s.depth is None) == (not rgbd)
    fo = s.frame_of.tolist()
    seen_missing = False
    for i, it in enumerate(ds.all_data):
        assert s.paths[fo[i]][0] == it["img_path"]
        folder = "%02d" % (it["obj_id"] + 1)
        frame = int(os.path.basename(it["img_path"])[:4])
        rgb, depth = written[folder][frame]
        assert np.array_equal(s.rgb[fo[i]].numpy(), rgb)
        if rgbd:
            got = s.depth[fo[i]].numpy()
            if depth is None:      # frame 18: the missing depth PNG is a zero frame
                seen_missing = True
                assert not got.any()
            else:
                assert np.array_equal(got, depth)
    assert seen_missing == rgbd
    if not rgbd:
        assert any("%s04%s" % (os.sep, os.sep) in p for p in paths)   # the depth-less folder is kept
    q, t, ids = ds.labels(ds.all_data)
    assert torch.equal(s.quat, q) and torch.equal(s.trans, t) and torch.equal(s.obj_id, ids)
    bo = np.array([it["bbox"] for it in ds.all_data])
    assert s.host_bbox.dtype == np.int64 and np.array_equal(s.host_bbox, bo)
    assert s.bbox.dtype == torch.int32 and np.array_equal(s.bbox.numpy(), bo)
    K = np.stack([np.array(it["cam_K"]).astype(np.float32) for it in ds.all_data])
    assert np.array_equal(s.K.numpy(), K)
    if rgbd:
        assert s.center_tab is None
    else:
        ref = torch.tensor([[x + w / 2, y + h / 2] for x, y, w, h in bo.tolist()], dtype=torch.float32)
        assert torch.equal(s.center_tab, ref)


def test_train_set_shares_frames_between_annotations(tree):
    """frame_of is per sample, the store per distinct path: a train set keeps the
    jitter flag, and two samples of one frame would share one store frame."""
    from pose6d.linemod import LineMODSet
    from pose6d.store import FrameStore
    root, _ = tree
    ds = LineMODSet(root, "train", rgbd=True)
    ds.all_data.append(dict(ds.all_data[0], bbox=[1, 2, 30, 30]))   # a second annotation of frame 0
    s = FrameStore.from_linemod(ds, "cpu", workers=2)
    assert s.augment_bbox and len(s) == len(ds) and s.n_frames == len(ds) - 1
    assert s.frame_of[-1] == s.frame_of[0] and s.bbox[-1].tolist() == [1, 2, 30, 30]


def test_mixed_frame_sizes_raise(tree, tmp_path):
    from PIL import Image
    from pose6d._lib import Pose6dError
    from pose6d.linemod import LineMODSet
    from pose6d.store import FrameStore
    root, _ = tree
    ds = LineMODSet(root, "test", rgbd=False, objects=("01",))
    odd = str(tmp_path / "odd.png")
    Image.fromarray(np.zeros((60, 80, 3), np.uint8)).save(odd)
    ds.all_data[1] = dict(ds.all_data[1], img_path=odd)
    with pytest.raises(Pose6dError, match="one size"):
        FrameStore.from_linemod(ds, "cpu", workers=2)


# ----------------------------------------------------------------- GPU
IDX = [5, 2, 9, 2, 0]       # non-monotonic, one sample twice
VAL_IDX = [3, 1, 2, 1, 0]   # the same for the 4-sample val split (sample 1: the missing depth PNG)


@pytest.mark.gpu
@pytest.mark.parametrize("rgbd", [True, False])
def test_indexed_equals_uncached_batch(tree, rgbd):
    """Stored boxes (val set) and jittered boxes (train set, the same rng state)
    against LineMODSet.batch uncached."""
    from pose6d.data import jitter_bboxes
    from pose6d.linemod import LineMODSet
    from pose6d.store import FrameStore
    root, _ = tree
    val = LineMODSet(root, "val", rgbd=rgbd)
    s = FrameStore.from_linemod(val, "cuda")
    assert len(val) >= 4
    _same(s.crop(VAL_IDX), val.batch(VAL_IDX, "cuda"))
    _same(s.crop(np.array(VAL_IDX)), _contiguous(s, VAL_IDX)[0])
    train = LineMODSet(root, "train", rgbd=rgbd)
    s = FrameStore.from_linemod(train, "cuda")
    ba = jitter_bboxes(s.host_bbox[IDX], rgbd, np.random.RandomState(1))
    assert not np.array_equal(ba, s.host_bbox[IDX])
    _same(s.crop(IDX, ba), train.batch(IDX, "cuda", np.random.RandomState(1)))
    _same(s.crop(torch.tensor(IDX).cuda(), torch.from_numpy(ba).cuda()), _contiguous(s, IDX, ba)[0])
    s.check()


@pytest.mark.gpu
@pytest.mark.parametrize("rgbd", [True, False])
def test_indexed_bgr_equals_contiguous(rgbd):
    from pose6d.store import FrameStore
    a = _arrays(6, 10, H=120, W=160, seed=3, depth=rgbd)
    s = FrameStore.from_arrays(*a, rgbd=rgbd, bgr=True)
    rgb_order = FrameStore.from_arrays(*a, rgbd=rgbd)
    ba = s.host_bbox[IDX] + np.array([3, -2, 5, 4])
    for boxes in (None, ba):
        got = s.crop(IDX, boxes)
        _same(got, _contiguous(s, IDX, boxes)[0])
        assert not torch.equal(got[0], rgb_order.crop(IDX, boxes)[0])
    s.check()


@pytest.mark.gpu
@pytest.mark.parametrize("rgbd", [True, False])
def test_train_transform_equals_contiguous(tree, rgbd):
    from pose6d.data import TrainAugment, jitter_bboxes
    from pose6d.linemod import LineMODSet
    from pose6d.store import FrameStore
    root, _ = tree
    s = FrameStore.from_linemod(LineMODSet(root, "train", rgbd=rgbd), "cuda")
    idx = [7, 1, 7]
    a_store, a_ref = TrainAugment(seed=3), TrainAugment(seed=3)
    for call_no in range(2):   # the same seed, rank and call count on both sides
        ba = jitter_bboxes(s.host_bbox[idx], rgbd, np.random.RandomState(call_no))
        got = s.crop(idx, ba, augment=a_store)
        ref, crop = _contiguous(s, idx, ba, augment=a_ref)
        _same(got, ref)
        assert torch.equal(s.last_params, crop.last_params)
    plain = s.crop(idx, ba)
    assert not torch.equal(plain[0], got[0])
    _same(plain[1:], got[1:])
    s.check()


CORNERS = [(-4, -4, 40, 32),    # the 48-pixel crop pads on all four sides of a 24 x 32 frame
           (5, 4, 14, 10),      # int(14 * 1.2) == 16 == 2 S: the exact-2x INTER_AREA branch
           (10, 10, 1, 1)]      # a one-pixel crop


@pytest.mark.gpu
@pytest.mark.parametrize("rgbd", [True, False])
def test_geometry_corners(rgbd):
    from pose6d.store import FrameStore
    a = list(_arrays(3, 3, seed=5, depth=rgbd))
    a[2], a[3] = np.array([2, 0, 1]), np.array(CORNERS)
    s = FrameStore.from_arrays(*a, rgbd=rgbd, img_size=8)
    assert int(max(CORNERS[1][2:]) * 1.2) == 2 * s.img_size
    _same(s.crop([0, 1, 2]), _contiguous(s, [0, 1, 2])[0])
    for i in range(3):   # B = 1
        _same(s.crop([i]), _contiguous(s, [i])[0])
        one = FrameStore.from_arrays(a[0][a[2][i]][None], None if a[1] is None else a[1][a[2][i]][None], [0],
                                     *(x[i:i + 1] for x in a[3:]), rgbd=rgbd, img_size=8)   # n = 1
        _same(one.crop([0]), s.crop([i]))
    s.check()


@pytest.mark.gpu
def test_store_offsets_are_64_bit():
    """2,400 frames of 480 x 640: the RGB store is 2.21 GB (> 2^31 bytes), the depth
    store 1.47 GB; only the first and the last frame hold data."""
    from pose6d.store import FrameStore
    if torch.cuda.mem_get_info()[0] < 8 << 30:
        pytest.skip("needs 8 GB of free device memory for the 3.7 GB store and its reference")
    N, H, W = 2400, 480, 640
    rgb = torch.zeros(N, H, W, 3, dtype=torch.uint8, device="cuda")
    depth = torch.zeros(N, H, W, dtype=torch.int16, device="cuda").view(torch.uint16)
    assert rgb.numel() > 1 << 31
    g = torch.Generator(device="cuda").manual_seed(0)
    for f in (0, N - 1):
        rgb[f] = torch.randint(0, 256, (H, W, 3), device="cuda", generator=g).to(torch.uint8)
        depth.view(torch.int16)[f] = torch.randint(300, 1600, (H, W), device="cuda", generator=g).to(torch.int16)
    _, _, _, _, K, q, t, ids = _arrays(1, 2, seed=9)
    bbox = np.array([[500, 380, 120, 90], [20, 10, 200, 150]])
    s = FrameStore.from_arrays(rgb, depth, [N - 1, 0], bbox, K, q, t, ids)
    assert s.rgb.data_ptr() == rgb.data_ptr()
    ends = torch.tensor([N - 1, 0], device="cuda")
    two = FrameStore.from_arrays(rgb[ends], _take(depth, ends), [0, 1], bbox, K, q, t, ids)
    got = s.crop([0, 1, 0])
    _same(got, _contiguous(two, [0, 1, 0])[0])
    assert got[0][0].std() > 0.5 and got[1][0].max() > 0   # the last frame's data, not the zeros before it
    s.check()


@pytest.mark.gpu
def test_indices_are_read_at_kernel_time():
    from pose6d._lib import Pose6dError
    from pose6d.data import TrainAugment
    from pose6d.store import FrameStore
    s = FrameStore.from_arrays(*_arrays(6, 10, H=120, W=160, seed=4), img_size=64)
    idx_dev = torch.tensor([0, 1, 2], device="cuda")
    bufs = tuple(torch.zeros_like(t) for t in s.crop(idx_dev))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        assert s.crop(idx_dev, out=bufs) is bufs
        with pytest.raises(Pose6dError, match="graph-captured"):
            s.crop(idx_dev, out=bufs, augment=TrainAugment(seed=1))
    graph.replay()
    _same(bufs, s.crop([0, 1, 2]))
    idx_dev.copy_(torch.tensor([9, 4, 4], device="cuda"))
    graph.replay()
    _same(bufs, s.crop([9, 4, 4]))
    s.check()


@pytest.mark.gpu
@pytest.mark.parametrize("rgbd", [True, False])
def test_cached_set_equals_uncached(tree, rgbd):
    from pose6d.linemod import LineMODSet
    root, _ = tree
    cached, plain = LineMODSet(root, "train", rgbd=rgbd), LineMODSet(root, "train", rgbd=rgbd)
    store = cached.cache("cuda")
    assert store.augment_bbox
    for seed, idx in enumerate((IDX, range(3, 8), [len(plain) - 1])):
        _same(cached.batch(idx, "cuda", np.random.RandomState(seed)),
              plain.batch(idx, "cuda", np.random.RandomState(seed)))
    store.check()
