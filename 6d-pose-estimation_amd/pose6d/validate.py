"""The validation pass and the plateau schedule of the reference's epoch
(scripts/training/train_rgbd_geometric.py:119-146, and the same lines of train_rgb.py,
train_rgb_geometric.py, train_rgbd.py) for the whole-step trainers of pose6d.train.

Validator runs the eval forward on the TRAINER's engines -- its activation buffers, the
packed weights its AdamW launch keeps current, the BatchNorm running statistics in the
module's buffers -- so there is no second set of engines and no stale packed weight.
Per batch: trainer._forward_eval, pose6d_add_eval[_nbr] on the predictions, then
pose6d_val_append, which moves the batch's per-sample (add, adds, valid, correct) into an
epoch table at a device-resident cursor.  The three can be captured into one graph; the
host reads nothing until finish(), the epoch's one device-to-host copy, and then applies
ADDLoss.aggregate batch by batch: the reference's numbers, bit for bit.

PlateauLR drives trainer.set_lr from a real torch ReduceLROnPlateau.
"""
import torch

from ._lib import Pose6dError, call, stream

_KEYS = ("add_mean", "add_s_mean", "add_01d_acc")


def merge_rank_tables(tables, B):
    """Per-rank epoch tables -> the table of the global batches.  tables[r]: (batches * B, 4)
    rows of rank r, batch k in rows k*B .. (k+1)*B-1 (a short batch is padded with valid = 0
    rows).  Global batch k is the concatenation, in rank order, of every rank's batch k -- the
    batch ADDLoss.eval_metrics_sharded would see -- so the result is (batches * world * B, 4)
    with global batch k in rows k*world*B .. (k+1)*world*B-1.  A pure host function."""
    tables = [torch.as_tensor(t, dtype=torch.float64).reshape(-1, 4) for t in tables]
    if not tables:
        raise Pose6dError("merge_rank_tables: no tables")
    rows = tables[0].shape[0]
    if B <= 0 or any(t.shape[0] != rows for t in tables) or rows % B:
        raise Pose6dError("merge_rank_tables: every rank must hold the same number of whole batches of %d rows "
                          "(got %s)" % (B, [t.shape[0] for t in tables]))
    world = len(tables)
    stacked = torch.stack([t.reshape(rows // B, B, 4) for t in tables])      # (world, batches, B, 4)
    return stacked.permute(1, 0, 2, 3).reshape(rows * world, 4)


class Validator:
    """val = Validator(trainer, add_loss, max_samples=4096)
    val.capture(data, obj_ids)        # optional: the batch body as one replayed graph
    val.begin()
    for data, obj_ids in batches:     # data: the trainer's training tuple, n <= trainer.B rows
        val.batch(data, obj_ids)
    metrics = val.finish()            # add_mean / add_s_mean / add_01d_acc: mean over batches
    """

    def __init__(self, trainer, add_loss, max_samples=4096):
        self.tr, self.crit = trainer, add_loss
        B, dev = trainer.B, trainer.dev
        self.B = B
        self.max_samples = int(max_samples)
        self.capacity = max(1, -(-self.max_samples // B)) * B
        # state int64[2] and the table in ONE allocation: finish() reads them in one copy
        self._buf = torch.zeros(2 + 4 * self.capacity, dtype=torch.int64, device=dev)
        self.state = self._buf[:2]
        self.table = self._buf[2:].view(torch.float64).view(self.capacity, 4)
        f64 = dict(device=dev, dtype=torch.float64)
        i32 = dict(device=dev, dtype=torch.int32)
        self.add, self.adds = torch.zeros(B, **f64), torch.zeros(B, **f64)
        self.valid, self.correct = torch.zeros(B, **i32), torch.zeros(B, **i32)
        self.ids = torch.full((B,), -1, device=dev, dtype=torch.int64)
        self.inputs = None          # static copies of the data tuple (what a captured graph reads)
        self._T = None              # the mesh table the per-sample buffers (and the graph) are bound to
        self.graph = None
        self._batches = 0

    # ------------------------------------------------------------- buffers
    @staticmethod
    def _shared(t, last_two):
        # the one input without a batch dimension: a (3, 3) camera matrix shared by the batch
        return not last_two and t.dim() == 2 and tuple(t.shape) == (3, 3)

    def _load(self, data, obj_ids):
        data = list(data)
        n = data[0].shape[0]
        if n > self.B:
            raise Pose6dError(f"Validator.batch: {n} samples, the trainer was built for batches of {self.B}")
        if self.inputs is None:
            dev = self.tr.dev
            self._is_shared = [self._shared(t, i >= len(data) - 2) for i, t in enumerate(data)]
            self.inputs = [torch.zeros(tuple(t.shape) if sh else (self.B,) + tuple(t.shape[1:]), device=dev,
                                       dtype=torch.float32) for t, sh in zip(data, self._is_shared)]
        if len(data) != len(self.inputs):
            raise Pose6dError("Validator.batch: the data tuple changed its length")
        for buf, t, sh in zip(self.inputs, data, self._is_shared):
            (buf if sh else buf[:n]).copy_(t)
        # a short last batch: rows n .. B-1 keep what they held and get object id -1, which
        # the ADD kernels mark valid = 0 -- they cost nothing in the metrics
        ids = torch.as_tensor(obj_ids).reshape(-1)
        if ids.shape[0] != n:
            raise Pose6dError(f"Validator.batch: {ids.shape[0]} object ids for {n} samples")
        self.ids[:n].copy_(ids)
        if n < self.B:
            self.ids[n:].fill_(-1)

    def _bind_table(self):
        """The mesh table the ADD launch reads; the per-sample workspaces are sized by it and
        allocated once per table (not per call, as ADDLoss.per_sample does).  Returns True
        when the table changed (a captured graph bakes its pointers in)."""
        T = self.crit._mesh_table(self.tr.dev)
        if self._T is not None and T is self._T:
            return False
        self._T = T          # (held: the graph's pointers stay alive until it is re-captured)
        mx = max(T.max_npts, 1)
        self.mind = torch.empty(self.B, mx, device=self.tr.dev, dtype=torch.float32)
        self.ptadd = torch.empty(self.B, mx, device=self.tr.dev, dtype=torch.float32)
        return True

    # ------------------------------------------------------------- the batch body
    def _body(self):
        tr, T, B = self.tr, self._T, self.B
        tr._forward_eval(*self.inputs)
        gt_rot, gt_trans = self.inputs[-2], self.inputs[-1]
        st = stream()
        head = (tr.rot, tr.trans, gt_rot, gt_trans, self.ids, B, T.points, T.off, T.npts, T.sym, T.diam, T.n_slots,
                T.max_npts)
        tail = (self.mind, None, self.ptadd, self.add, self.adds, self.valid, self.correct, st)
        if T.nbr is None:
            call("add_eval", *head, *tail)
        else:
            call("add_eval_nbr", *head, T.nbr, T.K, *tail)
        call("val_append", self.add, self.adds, self.valid, self.correct, B, self.table, self.capacity, self.state, st)

    def _capture(self):
        # eager warm-up first (the trunk's eval fold builds its descriptor table with a
        # host-to-device copy on first use), on a side stream as the trainers do; it appends
        # a batch, so the cursor is put back afterwards
        self.tr._sync_if_stale()
        state = self.state.clone()
        s = torch.cuda.Stream(device=self.tr.dev)
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            self._body()
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, capture_error_mode="thread_local"):
            self._body()
        self.state.copy_(state)
        torch.cuda.synchronize()
        self.graph = g

    def capture(self, data, obj_ids):
        """Capture the batch body (eval forward, ADD, append) into one graph; batch() then
        copies its inputs into the static buffers and replays it."""
        self._load(data, obj_ids)
        self._bind_table()
        self._capture()

    # ------------------------------------------------------------- the epoch
    def begin(self):
        """Start an epoch: the cursor back to row 0 (one device fill, no sync).  A mesh table
        that changed since the capture (ADDLoss.points / diameters edited) is re-captured."""
        if self._bind_table() and self.graph is not None:
            self._capture()
        self.state.zero_()
        self._batches = 0

    def batch(self, data, obj_ids):
        self._load(data, obj_ids)
        if self._T is None:
            self._bind_table()
        self.tr._sync_if_stale()     # masters written from outside the step (load_state_dict, restore)
        if self.graph is not None:
            self.graph.replay()
        else:
            self._body()
        self._batches += 1

    def finish(self):
        """The epoch's one device-to-host copy, then the reference's arithmetic
        (train_rgbd_geometric.py:138-144): ADDLoss.aggregate per batch, sum / batches over
        Python floats.  With trainer.pg set every rank gets the metrics of the global batches."""
        B = self.B
        used = min(self._batches * B, self.capacity)
        host = self._buf[:2 + 4 * used].cpu()
        rows, refused = int(host[0]), int(host[1])
        tab = host[2:].view(torch.float64).view(-1, 4)[:rows]
        group = B
        pg = getattr(self.tr, "pg", None)
        if pg is not None:
            tab, refused = self._gather(tab, refused, pg)
            group = B * torch.distributed.get_world_size(pg)
        if refused > 0:
            raise Pose6dError(f"Validator: {refused} batch(es) did not fit the epoch table of {self.capacity} rows; "
                              f"raise max_samples (now {self.max_samples})")
        nb = tab.shape[0] // group
        out = {k: 0 for k in _KEYS}
        if nb:
            sums = {k: 0.0 for k in _KEYS}
            for k in range(nb):
                r = tab[k * group:(k + 1) * group]
                m = self.crit.aggregate(r[:, 0], r[:, 1], r[:, 2], r[:, 3])
                for key in _KEYS:
                    sums[key] += m[key]
            out = {k: sums[k] / nb for k in _KEYS}
        out["batches"] = nb
        out["samples"] = int((tab[:, 2] > 0).sum())
        return out

    def _gather(self, tab, refused, pg):
        """One gather per epoch: every rank's rows behind a header row (rows, refused), so a
        table that overflowed on any rank raises on all of them."""
        import torch.distributed as tdist
        from .dist import gather_samples
        mine = torch.cat([torch.tensor([[tab.shape[0], refused, 0, 0]], dtype=torch.float64), tab])
        if tdist.get_backend(pg) == "nccl":
            mine = mine.to(self.tr.dev)
        (allrows,) = gather_samples([mine], pg)
        allrows = allrows.cpu()
        tables, at, refused = [], 0, 0
        while at < allrows.shape[0]:
            n = int(allrows[at, 0])
            refused += int(allrows[at, 1])
            tables.append(allrows[at + 1:at + 1 + n])
            at += 1 + n
        if refused > 0:
            return tab, refused
        return merge_rank_tables(tables, self.B), 0


class PlateauLR:
    """torch.optim.lr_scheduler.ReduceLROnPlateau for a whole-step trainer (the reference's
    `ReduceLROnPlateau(optimizer, mode='max', factor=0.5, patience=5)` + `scheduler.step(val_acc)`,
    train_rgbd_geometric.py:69,146).  The rule is torch's own: a real scheduler runs on a
    one-parameter dummy optimizer whose lr starts at the trainer's, and step() hands a changed
    lr to trainer.set_lr -- a device write the captured step reads, so nothing is re-captured.
    `trainer` needs set_lr() and an initial lr (`hp[0]`, or pass lr=)."""

    def __init__(self, trainer, mode="max", factor=0.5, patience=5, min_lr=0.0, lr=None, **kw):
        self.trainer = trainer
        if lr is None:
            lr = float(trainer.hp[0])        # read once
        self._param = torch.nn.Parameter(torch.zeros(1))
        self.optimizer = torch.optim.SGD([self._param], lr=float(lr))
        self.scheduler = torch.optim.lr_scheduler.ReduceLROnPlateau(self.optimizer, mode=mode, factor=factor,
                                                                    patience=patience, min_lr=min_lr, **kw)

    @property
    def lr(self):
        return self.optimizer.param_groups[0]["lr"]

    def step(self, metric):
        before = self.lr
        self.scheduler.step(metric)
        if self.lr != before:
            self.trainer.set_lr(self.lr)
        return self.lr

    def state_dict(self):
        """The scheduler's own state_dict (its `_last_lr` is the current lr)."""
        return self.scheduler.state_dict()

    def load_state_dict(self, sd):
        """The scheduler's load_state_dict; the lr it last set (`_last_lr`, which torch keeps in
        the optimizer's state_dict, not the scheduler's) goes to the dummy optimizer and, if it
        differs from the current one, to the trainer."""
        self.scheduler.load_state_dict(sd)
        last = sd.get("_last_lr")
        if last and float(last[0]) != self.lr:
            self.optimizer.param_groups[0]["lr"] = float(last[0])
            self.trainer.set_lr(float(last[0]))
