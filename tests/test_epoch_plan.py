"""The device side of a planned epoch (pose6d/fit.py): pose6d_plan_next, pose6d_loss_append,
pose6d_crop_rgbd_train_indexed_dseed, and EpochPlan's host tables against an EpochFeeder walk.

CPU: the argument checks of the three entry points (no launch), the plan's contents and the
state of every random stream afterwards.  GPU: rows in order and the refusal past the end,
eagerly and under graph replay; the loss table bit for bit; the device-seed crop equal to the
by-value one (torch.equal), also when the seed word is rewritten between replays.

As in tests/test_frame_store.py no test hands a kernel a bad device-side index."""
import numpy as np
import pytest
import torch

B, STEPS = 3, 2


# ----------------------------------------------------------------- CPU: argument checks
def test_plan_next_arguments_checked_without_gpu():
    from pose6d import _lib
    lib = _lib.load()
    idx = torch.zeros(STEPS, B, dtype=torch.int64)
    box = torch.zeros(STEPS, B, 4, dtype=torch.int32)
    seeds = torch.zeros(STEPS, dtype=torch.int64)
    state = torch.zeros(2, dtype=torch.int64)
    o_idx, o_box, o_seed = torch.zeros(B, dtype=torch.int64), torch.zeros(B, 4, dtype=torch.int32), \
        torch.zeros(1, dtype=torch.int64)
    p = lambda t: t.data_ptr()
    good = [p(idx), p(box), p(seeds), STEPS, B, p(state), p(o_idx), p(o_box), p(o_seed), None]

    def with_(**kw):
        names = ("idx_plan", "bbox_plan", "seed_plan", "steps", "B", "state", "sample_idx", "bbox_aug", "seed_out")
        a = list(good)
        for k, v in kw.items():
            a[names.index(k)] = v
        return a

    for args in (with_(B=-1), with_(B=65536), with_(steps=-1), with_(idx_plan=None), with_(state=None),
                 with_(sample_idx=None), with_(bbox_aug=None), with_(seed_out=None),
                 with_(bbox_plan=None), with_(seed_plan=None)):      # the last two: an output without its table
        assert lib.pose6d_plan_next(*args) == 1
        assert b"pose6d_plan_next" in lib.pose6d_last_error()
    assert lib.pose6d_plan_next(None, None, None, 0, 0, None, None, None, None, None) == 0   # B == 0: nothing to do
    assert state.tolist() == [0, 0] and not o_idx.any()


def test_loss_append_arguments_checked_without_gpu():
    from pose6d import _lib
    lib = _lib.load()
    loss, table, state = torch.zeros(()), torch.zeros(4), torch.zeros(3, dtype=torch.int64)
    for args in ((loss.data_ptr(), table.data_ptr(), -1, state.data_ptr(), None),
                 (None, table.data_ptr(), 4, state.data_ptr(), None),
                 (loss.data_ptr(), None, 4, state.data_ptr(), None),
                 (loss.data_ptr(), table.data_ptr(), 4, None, None)):
        assert lib.pose6d_loss_append(*args) == 1
        assert b"pose6d_loss_append" in lib.pose6d_last_error()
    assert state.tolist() == [0, 0, 0]


def _dseed_args(**kw):
    """pose6d_crop_rgbd_train_indexed_dseed's arguments over host buffers of the right sizes (the
    checks run before any launch), in the header's order."""
    n, S, Bc = 5, 8, 2
    z = lambda *s, dtype=torch.float32: torch.zeros(*s, dtype=dtype)
    a = dict(rgb_store=z(1, 4, 4, 3, dtype=torch.uint8), bgr=0, depth_store=None, n_frames=1, H=4, W=4,
             frame_of=z(n, dtype=torch.int32), bbox=z(n, 4, dtype=torch.int32), K=z(n, 9), center_tab=None,
             quat=z(n, 4), trans=z(n, 3), obj_id=z(n, dtype=torch.int64), n_samples=n,
             sample_idx=z(Bc, dtype=torch.int64), bbox_aug=None, B=Bc, S=S, mean_std=None, brightness=0.3,
             contrast=0.3, saturation=0.3, hue=0.05, erase_p=0.2, erase_scale_lo=0.02, erase_scale_hi=0.1,
             erase_ratio_lo=0.3, erase_ratio_hi=3.3, seed=z(1, dtype=torch.int64),
             workspace=z(Bc * S * S * 3, dtype=torch.uint8), rgb_out=z(Bc, 3, S, S), depth_out=None,
             depth_raw_out=None, center_out=None, K_out=None, quat_out=None, trans_out=None, obj_out=None,
             params_out=None, status=None, stream=None)
    assert set(kw) <= set(a)
    a.update(kw)
    return a


def test_dseed_crop_arguments_checked_without_gpu():
    from pose6d import _lib
    lib = _lib.load()
    keep = []

    def run(**kw):
        a = _dseed_args(**kw)
        keep.append(a)
        return lib.pose6d_crop_rgbd_train_indexed_dseed(*(v.data_ptr() if isinstance(v, torch.Tensor) else v
                                                          for v in a.values()))

    for kw in (dict(B=-1), dict(B=65536), dict(seed=None), dict(workspace=None), dict(rgb_out=None),
               dict(sample_idx=None), dict(rgb_store=None), dict(S=233), dict(hue=0.6)):
        assert run(**kw) == 1, kw
        assert b"pose6d_crop_rgbd_train_indexed_dseed" in lib.pose6d_last_error()
    assert run(B=0) == 0
    # the by-value entry point still names itself
    a = _dseed_args(B=-1)
    a["seed"] = 7
    assert lib.pose6d_crop_rgbd_train_indexed(*(v.data_ptr() if isinstance(v, torch.Tensor) else v
                                                for v in a.values())) == 1
    assert b"pose6d_crop_rgbd_train_indexed:" in lib.pose6d_last_error()


# ----------------------------------------------------------------- CPU: the plan's contents
def _stub_store(n, augment_bbox=True):
    from pose6d.store import FrameStore
    rng = np.random.default_rng(n)
    z = np.zeros
    s = FrameStore.from_arrays(z((1, 4, 4, 3), np.uint8), None, z(n, np.int64), rng.integers(1, 90, (n, 4)),
                               z((n, 9), np.float32), z((n, 4), np.float32), z((n, 3), np.float32), np.arange(n),
                               rgbd=True, device="cpu", augment_bbox=augment_bbox)
    return s


@pytest.mark.parametrize("rank,world", [(0, 1), (0, 2), (1, 2)])
def test_plan_equals_a_feeder_walk(monkeypatch, rank, world):
    """Two epochs (the constructor's and one build()): indices, jittered boxes and seeds equal
    an EpochFeeder loop's store.crop arguments, and generator, numpy stream and
    TrainAugment.calls end in the same state on both sides."""
    from pose6d.data import TrainAugment
    from pose6d.fit import EpochPlan
    from pose6d.store import EpochFeeder
    n, Bp = 23, 4
    g_a, g_b = torch.Generator().manual_seed(5), torch.Generator().manual_seed(5)
    r_a, r_b = np.random.RandomState(9), np.random.RandomState(9)
    aug_a, aug_b = TrainAugment(seed=3, rank=rank), TrainAugment(seed=3, rank=rank)
    ref_store = _stub_store(n)
    calls = []
    monkeypatch.setattr(ref_store, "crop", lambda idx, ba, out=None, augment=None:
                        calls.append((idx.copy(), ba.copy(), augment.next_seed())))
    monkeypatch.setattr(ref_store, "check", lambda: None)
    feeder = EpochFeeder(ref_store, Bp, rank=rank, world=world, generator=g_b, rng=r_b, augment=aug_b)
    plan = None
    for epoch in range(2):
        del calls[:]
        list(feeder)
        plan = EpochPlan(_stub_store(n), Bp, rank=rank, world=world, generator=g_a, rng=r_a, augment=aug_a) \
            if plan is None else plan.build()
        steps = n // (Bp * world)
        assert plan.steps == steps == len(calls) == len(feeder)
        assert plan.host_idx.shape == (steps, Bp) and plan.host_idx.dtype == np.int64
        assert plan.host_bbox.shape == (steps, Bp, 4) and plan.host_bbox.dtype == np.int32
        assert plan.host_seed.shape == (steps,) and plan.host_seed.dtype == np.uint64
        for k, (idx, ba, seed) in enumerate(calls):
            assert np.array_equal(plan.host_idx[k], idx) and np.array_equal(plan.host_bbox[k], ba)
            assert int(plan.host_seed[k]) == seed
        # the one upload (here onto the CPU "device") carries exactly the host tables
        assert np.array_equal(plan.idx_tab.numpy(), plan.host_idx)
        assert np.array_equal(plan.bbox_tab.numpy(), plan.host_bbox)
        assert np.array_equal(plan.seed_tab.numpy().view(np.uint64), plan.host_seed)
        assert torch.equal(g_a.get_state(), g_b.get_state())
        assert r_a.uniform() == r_b.uniform()
        assert aug_a.calls == aug_b.calls == (epoch + 1) * steps
    assert len(np.unique(plan.host_seed)) == plan.steps


def test_plan_without_jitter_or_transform_and_truncated():
    """A val-like store (no augment_bbox) without a TrainAugment has no box or seed table; steps=
    plans the first batches of the epoch and draws for those alone."""
    from pose6d._lib import Pose6dError
    from pose6d.fit import EpochPlan
    from pose6d.store import EpochFeeder
    s = _stub_store(10, augment_bbox=False)
    plan = EpochPlan(s, 4, shuffle=False)
    assert plan.host_bbox is None and plan.host_seed is None and plan.bbox_tab is None and plan.seed is None
    assert plan.host_idx.tolist() == [[0, 1, 2, 3], [4, 5, 6, 7]]
    s = _stub_store(23)
    r_a, r_b = np.random.RandomState(1), np.random.RandomState(1)
    plan = EpochPlan(s, 4, steps=2, generator=torch.Generator().manual_seed(2), rng=r_a)
    walk = EpochFeeder(s, 4, generator=torch.Generator().manual_seed(2), rng=r_b)
    from pose6d.data import jitter_bboxes
    for k, idx in zip(range(2), walk.index_batches()):
        assert np.array_equal(plan.host_idx[k], idx)
        assert np.array_equal(plan.host_bbox[k], jitter_bboxes(s.host_bbox[idx], True, r_b))
    assert r_a.uniform() == r_b.uniform()
    for bad in (0, 6):
        with pytest.raises(Pose6dError, match="steps"):
            EpochPlan(s, 4, steps=bad, generator=torch.Generator())


# ----------------------------------------------------------------- GPU: plan_next
def _tables(with_box, with_seed):
    g = torch.Generator().manual_seed(4)
    idx = torch.randint(0, 1000, (STEPS, B), generator=g).cuda()
    box = torch.randint(-50, 500, (STEPS, B, 4), generator=g).int().cuda() if with_box else None
    seeds = None
    if with_seed:   # all 64 bits in use, the top one included
        seeds = torch.from_numpy(np.array([0xFEDCBA9876543210, 0x0123456789ABCDEF], np.uint64).view(np.int64)).cuda()
    return idx, box, seeds


@pytest.mark.gpu
@pytest.mark.parametrize("with_box,with_seed", [(True, True), (False, False), (True, False), (False, True)])
def test_plan_next_kernel(with_box, with_seed):
    from pose6d._lib import call, stream
    idx, box, seeds = _tables(with_box, with_seed)
    state = torch.zeros(2, dtype=torch.int64, device="cuda")
    o_idx = torch.full((B,), -7, dtype=torch.int64, device="cuda")
    o_box = torch.full((B, 4), -7, dtype=torch.int32, device="cuda") if with_box else None
    o_seed = torch.full((1,), -7, dtype=torch.int64, device="cuda") if with_seed else None

    def step():
        call("plan_next", idx, box, seeds, STEPS, B, state, o_idx, o_box, o_seed, stream())

    def expect(row, cursor, refused):
        assert state.tolist() == [cursor, refused]
        assert torch.equal(o_idx, idx[row])
        assert o_box is None or torch.equal(o_box, box[row])
        assert o_seed is None or torch.equal(o_seed, seeds[row:row + 1])

    for k in range(STEPS):
        step()
        expect(k, k + 1, 0)
    step()                                    # past the end: no output changes, refused = 1
    expect(STEPS - 1, STEPS, 1)
    call("plan_next", None, None, None, STEPS, 0, None, None, None, None, stream())     # B == 0: a no-op
    expect(STEPS - 1, STEPS, 1)

    # one captured launch, replayed: the same two rows arrive, then the refusal
    state.zero_()
    o_idx.fill_(-7)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        step()
    assert state.tolist() == [0, 0] and o_idx.tolist() == [-7] * B      # capture ran nothing
    for _ in range(2):
        state.zero_()
        for k in range(STEPS):
            graph.replay()
            expect(k, k + 1, 0)
    graph.replay()
    expect(STEPS - 1, STEPS, 1)


# ----------------------------------------------------------------- GPU: loss_append
@pytest.mark.gpu
def test_loss_append_kernel():
    from pose6d._lib import call, stream
    bits = [0x3FC00000, 0x7FC12345, 0x7F800000, -0x00800000, -0x80000000, 0x00000001]
    # 1.5, a NaN with a payload, +inf, -inf (0xFF800000), -0.0 (0x80000000), the smallest subnormal
    vals = torch.tensor(bits, dtype=torch.int32, device="cuda")
    cap = len(bits)
    table = torch.full((cap + 2,), 7.0, device="cuda")
    state = torch.zeros(3, dtype=torch.int64, device="cuda")
    loss = torch.zeros((), device="cuda")
    for k in range(cap):
        loss.view(torch.int32).copy_(vals[k])
        call("loss_append", loss, table, cap, state, stream())
    assert state.tolist() == [cap, 0, 3]                      # NaN, +inf, -inf
    assert torch.equal(table.view(torch.int32)[:cap], vals)
    assert table[cap:].tolist() == [7.0, 7.0]
    assert table[4].item() == 0.0 and np.signbit(table[4].item())

    # overflow at capacity 2: the third append writes nothing and counts itself
    table2 = torch.full((4,), 7.0, device="cuda")
    state.zero_()
    for v in (1.0, 2.0, 3.0, float("nan")):
        loss.fill_(v)
        call("loss_append", loss, table2, 2, state, stream())
    assert state.tolist() == [2, 2, 0]                        # the refused NaN is not counted: it was not stored
    assert table2.tolist() == [1.0, 2.0, 7.0, 7.0]
    call("loss_append", loss, None, 0, state, stream())       # capacity 0 needs no table
    assert state.tolist() == [2, 3, 0]


# ----------------------------------------------------------------- GPU: the device-seed crop
def _arrays(n_frames, n, H=120, W=160, seed=0, depth=True):
    rng = np.random.default_rng(seed)
    rgb = rng.integers(0, 256, (n_frames, H, W, 3), dtype=np.uint8)
    d = rng.integers(300, 1600, (n_frames, H, W)).astype(np.uint16) if depth else None
    bbox = np.stack([rng.integers(-3, W - 40, n), rng.integers(-3, H - 40, n), rng.integers(20, 70, n),
                     rng.integers(20, 70, n)], 1)
    K = np.tile(np.array([570.0, 0, W / 2, 0, 571.0, H / 2, 0, 0, 1], np.float32), (n, 1))
    return (rgb, d, rng.integers(0, n_frames, n), bbox, K, rng.standard_normal((n, 4)).astype(np.float32),
            rng.standard_normal((n, 3)).astype(np.float32), rng.integers(0, 15, n))


class _Seed:
    """A TrainAugment whose next_seed() gives a fixed kernel seed (the by-value side)."""

    def __init__(self, aug, seed):
        self.jitter, self.erase, self._seed = aug.jitter, aug.erase, seed

    def next_seed(self):
        return self._seed


SEEDS = [0x9E3779B97F4A7C15, 12345, 0xFFFFFFFFFFFFFFFF]


@pytest.mark.gpu
@pytest.mark.parametrize("rgbd", [True, False])
def test_device_seed_crop_equals_by_value(rgbd):
    from pose6d.data import TrainAugment
    from pose6d.store import FrameStore
    s = FrameStore.from_arrays(*_arrays(5, 7, seed=2, depth=rgbd), rgbd=rgbd, img_size=64)
    aug = TrainAugment(seed=1)
    idx = torch.tensor([4, 0, 4], device="cuda")
    ba = (s.bbox[idx] + torch.tensor([2, -3, 4, 1], dtype=torch.int32, device="cuda")).contiguous()
    word = torch.zeros(1, dtype=torch.int64, device="cuda")
    out = tuple(torch.full_like(t, 5) for t in s.crop(idx, ba))

    def by_value(seed):
        ref = s.crop(idx, ba, augment=_Seed(aug, seed))
        return ref, s.last_params.clone()

    def same(seed):
        ref, params = by_value(seed)
        assert len(ref) == len(out) == (8 if rgbd else 6)
        for i, (g, r) in enumerate(zip(out, ref)):
            assert g.dtype == r.dtype and torch.equal(g, r), (hex(seed), i)
        assert torch.equal(plan_params, params)

    def set_word(seed):
        word.copy_(torch.from_numpy(np.array([seed], np.uint64).view(np.int64)))

    set_word(SEEDS[0])
    assert s.crop_planned(idx, ba, out, augment=aug, seed=word) is out
    plan_params = s.last_params
    same(SEEDS[0])
    assert not torch.equal(by_value(SEEDS[1])[0][0], out[0])         # the seed matters

    # captured once; the seed word rewritten between replays
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        s.crop_planned(idx, ba, out, augment=aug, seed=word)
    assert s.last_params is plan_params
    for seed in SEEDS[1:] + SEEDS[:1]:
        set_word(seed)
        for t in out:
            t.fill_(5)
        graph.replay()
        same(seed)
    s.check()
