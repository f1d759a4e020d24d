"""A device-resident frame store and the epoch feed built on it.

The reference's epoch (scripts/training/train_*.py:92-112) is a DataLoader over
LineMODDatasetRGB(D): per sample two PNG decodes, the crop on the host, then the
collate.  LineMODSet.batch keeps the decode per sample per batch; that suits the
evaluation harness and cannot feed a whole-step trainer.  Here every frame is decoded
ONCE and kept in HBM (LineMOD_preprocessed: ~16k frames of 640x480 RGB u8 + u16
depth, ~24 GB) beside the per-sample annotation tables, and one
pose6d_crop_rgbd_indexed launch turns a device vector of B sample indices into the B
model inputs and labels -- written straight into the tensors a captured step reads
when `out=` names them.  Per step the host draws the reference's own bbox jitter
(4 B np.random.uniform calls, `jitter_bboxes`) and uploads 16 B bytes of boxes.

FrameStore   the frames + tables, `crop(sample_idx, ...)` -> the collated tuple
EpochFeeder  one epoch of batches in torch.utils.data.RandomSampler's order

The per-sample train transform (ColorJitter + RandomErasing) is TrainAugment's, with
its seed contract unchanged: (seed, rank, calls so far) -> the kernel seed, never
graph-captured (pose6d/data.py).  A planned epoch (pose6d/fit.py) draws those seeds ahead
of time and goes through `crop_planned`, whose launches read index, boxes and seed from
device memory and can all be captured.
"""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from ._lib import Pose6dError, call, query, require_device, stream
from .data import IMAGENET_MEAN, IMAGENET_STD, jitter_bboxes

MAX_WORKERS = 16
STAGE_FRAMES = 32   # frames per pinned staging buffer (two buffers: ~59 MB at 640x480 RGB-D)


def _decode_workers(workers=None):
    """The process's CPU share (its affinity mask, not the machine's core count), capped."""
    if workers is None:
        workers = len(os.sched_getaffinity(0))
    return max(1, min(int(workers), MAX_WORKERS))


def _host(a, dtype):
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    return np.ascontiguousarray(np.asarray(a), dtype=dtype)


class FrameStore:
    """Decoded frames and per-sample tables on one device.

    rgb (N, H, W, 3) uint8, depth (N, H, W) uint16 or None; tables of n samples:
    frame_of int32, bbox (n, 4) int32, K (n, 9) fp32, quat (n, 4), trans (n, 3),
    obj_id int64 and, for the RGB datasets, center_tab (n, 2) -- the original-image
    bbox centre (dataset_rgb.py:96).  `host_bbox` is the int64 host copy the bbox
    jitter is drawn from.  Build with from_linemod / from_arrays.
    """

    def __init__(self, rgb, depth, tables, host_bbox, rgbd, img_size=224, normalize=True, bgr=False,
                 mean=IMAGENET_MEAN, std=IMAGENET_STD, augment_bbox=False):
        self.rgb, self.depth = rgb, depth
        self.frame_of, self.bbox, self.K, self.quat, self.trans, self.obj_id, self.center_tab = tables
        self.host_bbox = host_bbox
        self.rgbd, self.img_size, self.bgr = bool(rgbd), int(img_size), bool(bgr)
        self.augment_bbox = bool(augment_bbox)
        self.device = rgb.device
        self.n_frames, self.H, self.W = (int(v) for v in rgb.shape[:3])
        self.n_samples = int(self.frame_of.shape[0])
        # made here, not at the first crop: a crop under graph capture must not upload
        self._ms = torch.tensor(list(mean) + list(std), dtype=torch.float32).to(self.device) if normalize else None
        self._status = torch.zeros(1, dtype=torch.int32, device=self.device)
        self._ws = None
        self.last_params = None   # (B, 16) per-crop parameters of the last augmented crop

    def __len__(self):
        return self.n_samples

    # ------------------------------------------------------------ construction
    @classmethod
    def from_arrays(cls, rgb, depth, frame_of, bbox, K, quat, trans, obj_id, rgbd=None, device="cuda", **kw):
        """The store of in-memory frames and tables (tests; users with their own
        decoder).  rgb / depth: numpy arrays or tensors -- a tensor already on `device`
        is kept as it is.  rgbd (default: depth is given) selects the collated tuple;
        an RGB store's centre table is computed from bbox like LineMODSet.batch does."""
        device = torch.device(device)
        if rgbd is None:
            rgbd = depth is not None

        def frames(a, dtype, tail):
            if a is None:
                return None
            t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))
            if t.dtype != dtype or t.dim() != 3 + len(tail) or tuple(t.shape[3:]) != tail:
                raise Pose6dError(f"FrameStore: frames must be (N, H, W{', 3' if tail else ''}) {dtype}, got "
                                  f"{tuple(t.shape)} {t.dtype}")
            return t.to(device).contiguous()

        rgb_t = frames(rgb, torch.uint8, (3,))
        depth_t = frames(depth, torch.uint16, ())
        if depth_t is not None and tuple(depth_t.shape) != tuple(rgb_t.shape[:3]):
            raise Pose6dError(f"FrameStore: depth {tuple(depth_t.shape)} does not match rgb {tuple(rgb_t.shape)}")
        return cls(rgb_t, depth_t, *cls._tables(frame_of, bbox, K, quat, trans, obj_id, rgbd, int(rgb_t.shape[0]),
                                                 device), rgbd, **kw)

    @staticmethod
    def _tables(frame_of, bbox, K, quat, trans, obj_id, rgbd, n_frames, device):
        fo = _host(frame_of, np.int64).reshape(-1)
        n = len(fo)
        bo = _host(bbox, np.int64).reshape(n, 4)
        if n and (fo.min() < 0 or fo.max() >= n_frames):
            raise Pose6dError(f"FrameStore: frame_of must lie in [0, {n_frames}), got [{fo.min()}, {fo.max()}]")
        center = None
        if not rgbd:   # dataset_rgb.py:96 (Python floats -> fp32), as LineMODSet.batch builds it
            center = torch.tensor([[x + w / 2, y + h / 2] for x, y, w, h in bo.tolist()],
                                  dtype=torch.float32).reshape(n, 2)
        host = (torch.from_numpy(fo.astype(np.int32)), torch.from_numpy(bo.astype(np.int32)),
                torch.from_numpy(_host(K, np.float32).reshape(n, 9)),
                torch.from_numpy(_host(quat, np.float32).reshape(n, 4)),
                torch.from_numpy(_host(trans, np.float32).reshape(n, 3)),
                torch.from_numpy(_host(obj_id, np.int64).reshape(n)), center)
        return tuple(None if t is None else t.to(device).contiguous() for t in host), bo

    @classmethod
    def from_linemod(cls, ds, device="cuda", workers=None):
        """Decode every distinct frame of LineMODSet `ds` once (load_rgb / load_depth
        on a thread pool, a missing depth PNG reading as zeros) into one (N, H, W, 3)
        uint8 and, for an RGB-D set, one (N, H, W) uint16 device tensor.  Frames pass
        through two pinned staging buffers of STAGE_FRAMES frames; the decoded set is
        never held on the host."""
        from .linemod import load_depth, load_rgb
        device = torch.device(device)
        if not len(ds):
            raise Pose6dError("FrameStore.from_linemod: the set is empty")
        frame_no, paths = {}, []
        for it in ds.all_data:
            key = (it["img_path"], it.get("depth_path"))
            if key not in frame_no:
                frame_no[key] = len(paths)
                paths.append(key)
        frame_of = [frame_no[(it["img_path"], it.get("depth_path"))] for it in ds.all_data]
        first = load_rgb(paths[0][0])
        H, W = first.shape[:2]
        N = len(paths)
        need = N * H * W * (5 if ds.rgbd else 3)
        on_gpu = device.type == "cuda"
        if on_gpu:
            free, _ = torch.cuda.mem_get_info(device)
            if need > free:
                raise Pose6dError(f"FrameStore.from_linemod: {N} frames of {H}x{W} need {need} bytes on {device}, "
                                  f"{free} are free")
        rgb = torch.empty(N, H, W, 3, dtype=torch.uint8, device=device)
        depth = torch.empty(N, H, W, dtype=torch.uint16, device=device) if ds.rgbd else None

        C = min(STAGE_FRAMES, N)
        stage = [(torch.empty(C, H, W, 3, dtype=torch.uint8, pin_memory=on_gpu),
                  torch.empty(C, H, W, dtype=torch.uint16, pin_memory=on_gpu) if ds.rgbd else None) for _ in range(2)]
        done = [None, None]   # the event after each staging buffer's last upload

        def decode(i, rgb_np, depth_np, slot):
            a = first if i == 0 else load_rgb(paths[i][0])
            if a.shape != (H, W, 3):
                raise Pose6dError(f"FrameStore.from_linemod: all frames must share one size; {paths[0][0]} is "
                                  f"{(H, W)}, {paths[i][0]} is {a.shape[:2]}")
            rgb_np[slot] = a
            if depth_np is not None:
                d = load_depth(paths[i][1], (H, W))
                if d.shape != (H, W):
                    raise Pose6dError(f"FrameStore.from_linemod: {paths[i][1]} is {d.shape}, its frame {(H, W)}")
                depth_np[slot] = d

        with ThreadPoolExecutor(_decode_workers(workers)) as pool:
            for k, s in enumerate(range(0, N, C)):
                r_pin, d_pin = stage[k % 2]
                if done[k % 2] is not None:
                    done[k % 2].synchronize()   # the buffer's previous upload has left it
                e = min(s + C, N)
                r_np, d_np = r_pin.numpy(), None if d_pin is None else d_pin.numpy()
                list(pool.map(lambda i: decode(i, r_np, d_np, i - s), range(s, e)))
                rgb[s:e].copy_(r_pin[:e - s], non_blocking=True)
                if depth is not None:
                    depth[s:e].copy_(d_pin[:e - s], non_blocking=True)
                if on_gpu:
                    done[k % 2] = torch.cuda.Event()
                    done[k % 2].record()
        if on_gpu:
            torch.cuda.synchronize(device)
        q, t, ids = ds.labels(ds.all_data)
        K = np.stack([np.array(it["cam_K"]).reshape(3, 3).astype(np.float32) for it in ds.all_data])
        tables, bo = cls._tables(frame_of, [it["bbox"] for it in ds.all_data], K, q, t, ids, ds.rgbd, N, device)
        store = cls(rgb, depth, tables, bo, ds.rgbd, img_size=ds.img_size, augment_bbox=ds.augment_bbox)
        store.paths = paths
        return store

    # ------------------------------------------------------------ the batch
    def _shapes(self, B):
        S = self.img_size
        img = [(B, 3, S, S), (B, 1, S, S), (B, S, S)] if self.rgbd else [(B, 3, S, S)]
        return img + [(B, 4), (B, 3), (B,), (B, 2), (B, 3, 3)]

    def _outputs(self, B):
        return tuple(torch.empty(s, device=self.device, dtype=torch.long if len(s) == 1 else torch.float32)
                     for s in self._shapes(B))

    def crop(self, sample_idx, bbox_aug=None, out=None, augment=None):
        """The reference's collated batch of samples `sample_idx`, in LineMODSet.batch's
        order: RGB-D (rgb, depth, depth_raw, quaternion, translation, obj_id,
        bbox_center, camera_matrix), RGB (rgb, quaternion, translation, obj_id,
        bbox_center, camera_matrix).

        sample_idx: a host sequence / array / CPU tensor -- range-checked here, before
        any launch, then uploaded -- or a device int64 tensor, used as it is and read at
        kernel time (with out= the non-augmented call is graph-capturable; `check()`
        reports a bad device-side index).  bbox_aug: (B, 4) jittered boxes (host or
        device int32) or None = the stored boxes.  out: preallocated tensors in the
        returned order.  augment: a TrainAugment -> the train transform on rgb; like
        CropRGBD's it refuses graph capture, and its parameters land in `last_params`."""
        n = self.n_samples
        if isinstance(sample_idx, torch.Tensor) and sample_idx.is_cuda:
            if sample_idx.dtype != torch.int64 or sample_idx.dim() != 1 or not sample_idx.is_contiguous():
                raise Pose6dError(f"FrameStore.crop: a device sample_idx must be a contiguous 1-D int64 tensor, got "
                                  f"{tuple(sample_idx.shape)} {sample_idx.dtype}")
            idx = sample_idx
        else:
            host = _host(sample_idx, np.int64).reshape(-1)
            if len(host) and (host.min() < 0 or host.max() >= n):
                bad = int(np.flatnonzero((host < 0) | (host >= n))[0])
                raise Pose6dError(f"FrameStore.crop: sample index {int(host[bad])} at batch position {bad} is "
                                  f"outside [0, {n})")
            idx = torch.from_numpy(host).to(self.device, non_blocking=True)
        B = int(idx.shape[0])
        if bbox_aug is not None:
            if not isinstance(bbox_aug, torch.Tensor):
                bbox_aug = torch.from_numpy(_host(bbox_aug, np.int32))
            if tuple(bbox_aug.shape) != (B, 4):
                raise Pose6dError(f"FrameStore.crop: bbox_aug must be ({B}, 4), got {tuple(bbox_aug.shape)}")
            bbox_aug = bbox_aug.to(self.device, torch.int32, non_blocking=True).contiguous()
        seed = augment.next_seed() if augment is not None else None   # refuses capture before anything is queued
        require_device(self.rgb, idx, bbox_aug)
        if out is None:
            out = self._outputs(B)
        want = self._shapes(B)
        if len(out) != len(want) or any(tuple(o.shape) != w for o, w in zip(out, want)):
            raise Pose6dError(f"FrameStore.crop: out must be tensors of shapes {want}, got "
                              f"{[tuple(o.shape) for o in out]}")
        require_device(*out)
        if self.rgbd:
            rgb_o, depth_o, raw_o, q_o, t_o, id_o, c_o, K_o = out
        else:
            rgb_o, q_o, t_o, id_o, c_o, K_o = out
            depth_o = raw_o = None
        S = self.img_size
        store = (self.rgb, int(self.bgr), self.depth, self.n_frames, self.H, self.W, self.frame_of, self.bbox, self.K,
                 self.center_tab, self.quat, self.trans, self.obj_id, n, idx, bbox_aug, B, S, self._ms)
        if augment is None:
            call("crop_rgbd_indexed", *store, rgb_o, depth_o, raw_o, c_o, K_o, q_o, t_o, id_o, self._status, stream())
            return out
        nws = query("crop_train_workspace", B, S)
        if self._ws is None or self._ws.numel() < nws:
            self._ws = torch.empty(nws, device=self.device, dtype=torch.uint8)
        self.last_params = torch.empty(B, 16, device=self.device)
        call("crop_rgbd_train_indexed", *store, *augment.jitter, *augment.erase, seed, self._ws, rgb_o, depth_o, raw_o,
             c_o, K_o, q_o, t_o, id_o, self.last_params, self._status, stream())
        return out

    def reserve_train(self, B):
        """The train transform's workspace and parameter buffer for batches of B, allocated
        here so that crop_planned allocates nothing (pose6d.fit calls it before a capture)."""
        nws = query("crop_train_workspace", B, self.img_size)
        if self._ws is None or self._ws.numel() < nws:
            self._ws = torch.empty(nws, device=self.device, dtype=torch.uint8)
        if getattr(self, "_plan_params", None) is None or self._plan_params.shape[0] != B:
            self._plan_params = torch.empty(B, 16, device=self.device)

    def crop_planned(self, sample_idx, bbox_aug, out, augment=None, seed=None):
        """crop() for a planned epoch (pose6d.fit.EpochPlan): everything is already on the
        device, nothing is checked, uploaded or allocated here, and every launch can be
        captured.  sample_idx int64 [B] and bbox_aug int32 [B, 4] (or None) are read at kernel
        time; out as crop()'s.  augment: a TrainAugment, whose transform then runs with the seed
        in the DEVICE word `seed` (int64 [1], the kernel's uint64; pose6d_crop_rgbd_train_indexed
        _dseed) -- augment.next_seed() is the planner's business, not this call's."""
        B, S = int(sample_idx.shape[0]), self.img_size
        if self.rgbd:
            rgb_o, depth_o, raw_o, q_o, t_o, id_o, c_o, K_o = out
        else:
            rgb_o, q_o, t_o, id_o, c_o, K_o = out
            depth_o = raw_o = None
        store = (self.rgb, int(self.bgr), self.depth, self.n_frames, self.H, self.W, self.frame_of, self.bbox, self.K,
                 self.center_tab, self.quat, self.trans, self.obj_id, self.n_samples, sample_idx, bbox_aug, B, S,
                 self._ms)
        if augment is None:
            call("crop_rgbd_indexed", *store, rgb_o, depth_o, raw_o, c_o, K_o, q_o, t_o, id_o, self._status, stream())
            return out
        if seed is None:
            raise Pose6dError("FrameStore.crop_planned: the train transform needs the device seed word")
        self.reserve_train(B)
        self.last_params = self._plan_params
        call("crop_rgbd_train_indexed_dseed", *store, *augment.jitter, *augment.erase, seed, self._ws, rgb_o, depth_o,
             raw_o, c_o, K_o, q_o, t_o, id_o, self.last_params, self._status, stream())
        return out

    def check(self, status=None):
        """Read the status word of every crop since the last check and reset it; raise
        if a launch met a sample or frame index out of range.  The one host sync of the
        feed: call it once per epoch.  status: the word's value when the caller has already
        read it (pose6d.fit copies it with the epoch's loss table) -- then nothing syncs."""
        v = int(self._status.item()) if status is None else int(status)
        if v:
            self._status.zero_()
            raise Pose6dError(f"FrameStore.check: a crop read an out-of-range sample or frame index at batch "
                              f"position {v - 1} (that crop's outputs are zeros, its obj_id -1)")


class EpochFeeder:
    """One epoch of `store.crop` batches in the reference DataLoader's order.

    shuffle=True draws the epoch's order exactly as torch.utils.data.RandomSampler
    does (the reference's DataLoader(shuffle=True)): with generator=None the epoch
    seed comes from torch's default generator, and the permutation is
    torch.randperm(n, generator=...) -- the same torch seed gives the same order.
    shuffle=False is index order.

    DEPARTURE from the reference: drop_last defaults to True.  The whole-step trainers
    are captured at a fixed batch size and cannot take the DataLoader's short last
    batch; drop_last=False yields it, for eager users.

    world > 1: every rank draws the same permutation from `generator` (required, seeded
    alike on every rank) and takes positions rank::world of each global batch of
    batch_size * world samples; the rank shards are disjoint, and over an epoch their
    union is the permutation's prefix of whole global batches (drop_last=False: all).

    Each batch: the reference's bbox jitter when the store's set is a train set with
    augment_bbox (`jitter_bboxes(store.host_bbox[idx], rgbd, rng)`: 4 B rng.uniform
    draws in the reference's order), then one store.crop call -- with augment=, a
    TrainAugment, the train transform under its own unchanged seed contract.
    `into(out)` makes every full batch land in the given tensors (a trainer's captured
    inputs); store.check() runs when the epoch ends."""

    def __init__(self, store, batch_size, shuffle=True, drop_last=True, rank=0, world=1, generator=None,
                 rng=np.random, augment=None, rgbd=None):
        if batch_size < 1 or world < 1 or not 0 <= rank < world:
            raise Pose6dError(f"EpochFeeder: bad batch_size / rank / world ({batch_size}, {rank}, {world})")
        if world > 1 and shuffle and generator is None:
            raise Pose6dError("EpochFeeder: world > 1 needs a generator seeded alike on every rank (each rank "
                              "must draw the same permutation)")
        self.store, self.batch_size, self.shuffle, self.drop_last = store, int(batch_size), shuffle, drop_last
        self.rank, self.world, self.generator, self.rng, self.augment = int(rank), int(world), generator, rng, augment
        self.rgbd = store.rgbd if rgbd is None else rgbd
        self._out = None

    def into(self, out):
        self._out = out
        return self

    def __len__(self):
        n, g = len(self.store), self.batch_size * self.world
        if self.drop_last:
            return n // g
        return n // g + (1 if n % g > self.rank else 0)

    def order(self):
        """The epoch's global sample order (advances the generator like RandomSampler.__iter__)."""
        n = len(self.store)
        if not self.shuffle:
            return list(range(n))
        generator = self.generator
        if generator is None:
            seed = int(torch.empty((), dtype=torch.int64).random_().item())
            generator = torch.Generator()
            generator.manual_seed(seed)
        order = torch.randperm(n, generator=generator).tolist()
        torch.randperm(n, generator=generator)   # RandomSampler's trailing [: num_samples % n] draw
        return order

    def index_batches(self):
        """This rank's index arrays (int64) for one epoch."""
        order = np.asarray(self.order(), np.int64)
        g = self.batch_size * self.world
        end = len(order) - len(order) % g if self.drop_last else len(order)
        for s in range(0, end, g):
            idx = order[s:min(s + g, end)][self.rank::self.world]
            if len(idx):
                yield idx

    def __iter__(self):
        store = self.store
        for idx in self.index_batches():
            ba = jitter_bboxes(store.host_bbox[idx], self.rgbd, self.rng) if store.augment_bbox else None
            out = self._out if self._out is not None and len(idx) == self.batch_size else None
            yield store.crop(idx, ba, out=out, augment=self.augment)
        store.check()
