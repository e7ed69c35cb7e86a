"""Real training images: a uint8 array file as a device-resident (or host-resident, prefetched) dataset whose batches are formed by one
dxmi_image_batch launch.

The reference reads image folders through DataLoader workers (PIL decode, fp32 collate on the host, a copy per batch:
loader/__init__.py, models/cm/image_datasets.py).  Stored as uint8 at the training resolution CIFAR-10 is 150 MB and ImageNet-64
15.7 GB: they live in HBM, and a batch is a gather + mirror + normalise + NHWC->NCHW launch over device index slices.  An array that
does not fit (LSUN-256: ~590 GB) stays on the host; one background thread gathers the next batch into pinned memory and copies it on a
side stream, one batch ahead, and the same launch runs on the staged rows.

Files: `.npz` with `arr_0` uint8 [M, H, W, C] (what make_npz.py and the evaluator's batches hold) and optionally `arr_1` integer [M]
labels; or `.npy` (memory-mapped) with labels in `PATH.labels.npy` next to it.

Order (identical on every path and every rank count, drawn on the CPU): for epoch e the permutation is
torch.randperm(M, generator=Generator().manual_seed(seed + e)), the same on all ranks; rank r takes perm[r::world][:M // world] and
cuts it into batches of batch_size, dropping the last partial one (drop_last=True, as both reference scripts set).  The M % world
images at the end of the permutation are DROPPED for that epoch, where the reference's DistributedSampler pads by repeating images so
that every rank gets ceil(M / world): here no image is seen twice in an epoch and another permutation drops other images.  The flip
bits of an epoch are torch.rand(M // world, generator=Generator().manual_seed(flip_seed(seed, e, r))) < 0.5.
"""
import itertools
import os
import queue
import threading
import warnings
import weakref

import numpy as np
import torch

NORM_ADM, NORM_TOTENSOR = 0, 1          # DXMI_IMG_NORM_* of include/dxmi_hip.h
_NORMS = {"adm": NORM_ADM, "totensor": NORM_TOTENSOR, NORM_ADM: NORM_ADM, NORM_TOTENSOR: NORM_TOTENSOR}
_M64 = 0xFFFFFFFFFFFFFFFF


def flip_seed(seed, epoch, rank):
    """63-bit counter hash of (seed, epoch, rank): the generator seed of one rank's flip bits for one epoch."""
    x = (int(seed) * 0x9E3779B97F4A7C15 + int(epoch) * 0xD1B54A32D192ED03 + int(rank) * 0x8CB92BA72F3D8DD7 + 0x2545F4914F6CDD1D) & _M64
    x ^= x >> 32
    x = (x * 0xD6E8FEB86659FD93) & _M64
    x ^= x >> 32
    return x & 0x7FFFFFFFFFFFFFFF


def normalise(u8, norm):
    """The two normalisations as torch expressions on a uint8 tensor: what the kernel computes, one rounding per operation.
    NORM_ADM: image_datasets.py:118 `arr.astype(np.float32) / 127.5 - 1`; NORM_TOTENSOR: ToTensor's `.div(255)`, then `2 * images - 1`."""
    if _NORMS[norm] == NORM_ADM:
        return u8.float() / 127.5 - 1
    return 2 * u8.float().div(255) - 1


def form_batch(u8, flip, norm):
    """uint8 [B, H, W, C] rows + bool / uint8 [B] flips (or None) -> fp32 [B, C, H, W]: the torch form of dxmi_image_batch."""
    if flip is not None:
        u8 = torch.where(flip.bool().view(-1, 1, 1, 1), u8.flip(2), u8)
    return normalise(u8, norm).permute(0, 3, 1, 2).contiguous()


def load_arrays(path):
    """(images uint8 [M, H, W, C], labels int64 [M] or None) of an .npz / .npy file; ValueError names the file and what it holds."""
    path = os.fspath(path)
    labels = None
    if path.endswith(".npz"):
        with np.load(path) as z:
            if "arr_0" not in z.files:
                raise ValueError(f"{path}: no arr_0 in the archive (found {z.files})")
            arr = z["arr_0"]
            if "arr_1" in z.files:
                labels = z["arr_1"]
    elif path.endswith(".npy"):
        arr = np.load(path, mmap_mode="r")
        for cand in (path + ".labels.npy", path[:-4] + ".labels.npy"):
            if os.path.exists(cand):
                labels = np.load(cand)
                break
    else:
        raise ValueError(f"{path}: an .npz (arr_0 [, arr_1]) or .npy image array is expected")
    if arr.dtype != np.uint8 or arr.ndim != 4:
        raise ValueError(f"{path}: images must be uint8 [M, H, W, C], found {arr.dtype} {tuple(arr.shape)}")
    if arr.shape[3] not in (1, 3):
        raise ValueError(f"{path}: images must have 3 or 1 channels last, found shape {tuple(arr.shape)}")
    if labels is not None:
        if labels.ndim != 1 or not np.issubdtype(labels.dtype, np.integer):
            raise ValueError(f"{path}: labels must be an integer array [M], found {labels.dtype} {tuple(labels.shape)}")
        if labels.shape[0] != arr.shape[0]:
            raise ValueError(f"{path}: {labels.shape[0]} labels for {arr.shape[0]} images")
        labels = np.ascontiguousarray(labels.astype(np.int64))
    return arr, labels


class _HostFeeder:
    """The host-resident producer: one thread walks the batches of `epochs` in order, gathers each batch's rows (and labels) into one of
    two staging buffers and, on a GPU, copies them to that slot's device buffer on a side stream and records the slot's event.  The
    thread makes no other HIP call: the consumer waits for the copy (host side, so the pinned buffer may be refilled), launches, and
    orders the slot's next copy behind its launch on the side stream before it hands the slot back."""

    def __init__(self, store, epochs, first_batch):
        self.store, self.epochs, self.first_batch = store, epochs, first_batch
        B, (H, W, C) = store.batch_size, store.image_shape
        self.cuda = store.device.type == "cuda"
        self.stage = [torch.empty((B, H, W, C), dtype=torch.uint8, pin_memory=self.cuda) for _ in range(2)]
        self.stage_y = [torch.empty(B, dtype=torch.int64, pin_memory=self.cuda) for _ in range(2)] if store.with_labels else None
        if self.cuda:
            self.dev = [torch.empty((B, H, W, C), dtype=torch.uint8, device=store.device) for _ in range(2)]
            self.dev_y = [torch.empty(B, dtype=torch.int64, device=store.device) for _ in range(2)] if store.with_labels else None
            self.side = torch.cuda.Stream(device=store.device)
            self.copied = [torch.cuda.Event() for _ in range(2)]
        self.free, self.ready = queue.Queue(), queue.Queue()
        self.free.put(0)
        self.free.put(1)
        self.stop = threading.Event()
        self.error = None
        self.thread = threading.Thread(target=self._run, name="dxmi-image-store", daemon=True)
        self.thread.start()

    def _run(self):
        store, first = self.store, self.first_batch
        try:
            for e in self.epochs:
                rows, flips = store.plan(e)
                rows_np = rows.numpy()
                for b in range(first, store.batches_per_epoch):
                    slot = self.free.get()
                    if slot is None or self.stop.is_set():
                        return
                    r = rows_np[b * store.batch_size:(b + 1) * store.batch_size]
                    np.take(store.arr, r, axis=0, out=self.stage[slot].numpy())
                    if self.stage_y is not None:
                        np.take(store.labels, r, out=self.stage_y[slot].numpy())
                    if self.cuda:
                        with torch.cuda.stream(self.side):
                            self.dev[slot].copy_(self.stage[slot], non_blocking=True)
                            if self.stage_y is not None:
                                self.dev_y[slot].copy_(self.stage_y[slot], non_blocking=True)
                            self.copied[slot].record(self.side)
                    self.ready.put((slot, e, b, flips))
                first = 0
        except BaseException as exc:      # handed to the consumer: a failed gather must not look like the end of the data
            self.error = exc
        finally:
            self.ready.put(None)

    def take(self):
        """The next staged batch as (images, labels or None, epoch, batch), or None after the last one."""
        item = self.ready.get()
        if item is None:
            if self.error is not None:
                raise self.error
            return None
        slot, e, b, flips = item
        store = self.store
        fl = store.epoch_flips(e, flips)
        if fl is not None:
            fl = fl[b * store.batch_size:(b + 1) * store.batch_size]
        if self.cuda:
            from . import ops
            self.copied[slot].synchronize()                # the copy was issued a batch ago; the pinned buffer is free after it
            images = ops.image_batch(self.dev[slot], None, fl, store.norm)
            y = self.dev_y[slot].clone() if self.stage_y is not None else None
            self.side.wait_stream(torch.cuda.current_stream(store.device))      # the slot's next copy runs after this launch
        else:
            images = form_batch(self.stage[slot], fl, store.norm)
            y = self.stage_y[slot].clone() if self.stage_y is not None else None
        self.free.put(slot)
        return images, y, e, b

    def close(self):
        self.stop.set()
        self.free.put(None)
        if self.thread is not threading.current_thread():
            self.thread.join()


class ImageStore:
    """A uint8 image array file as a training dataset (module docstring: formats, order, resident modes).

    norm: NORM_ADM / "adm" or NORM_TOTENSOR / "totensor".  batch_size is per rank.  resident: "device" uploads the array once and
    forms a batch from device index slices; "host" keeps it on the host behind a one-batch-ahead prefetch thread; "auto" takes the
    device when the array is at most device_budget_bytes.  On a CPU `device` the batches are the torch expressions of form_batch and
    the library is not needed ("device" then means: indexed in memory; "host" runs the same prefetch thread on plain buffers).
    epoch(e) yields (images, labels or None) once through epoch e; batches() yields (images, {"y": labels} or {}) forever;
    state() gives the position of the next batch, seek() sets where the next batches() call starts.  close() ends every live prefetch thread."""

    def __init__(self, path, device, norm, *, batch_size, rank=0, world=1, seed=0, random_flip=True, class_cond=False,
                 resident="auto", device_budget_bytes=32 << 30):
        self.path = os.fspath(path)
        self.device = torch.device(device)
        if norm not in _NORMS:
            raise ValueError(f"ImageStore: norm {norm!r} is not one of 'adm', 'totensor'")
        self.norm = _NORMS[norm]
        self.arr, labels = load_arrays(self.path)
        self.M = int(self.arr.shape[0])
        self.image_shape = tuple(int(s) for s in self.arr.shape[1:])
        if class_cond and labels is None:
            raise ValueError(f"{self.path}: class_cond needs labels, and the file has none (arr_1 of an .npz, PATH.labels.npy of an .npy)")
        self.has_labels = labels is not None
        self.with_labels = bool(class_cond)
        self.labels = labels if self.with_labels else None
        self.batch_size, self.rank, self.world, self.seed = int(batch_size), int(rank), int(world), int(seed)
        if not (self.world >= 1 and 0 <= self.rank < self.world and self.batch_size >= 1):
            raise ValueError(f"ImageStore: batch_size {batch_size}, rank {rank}, world {world}")
        self.per_rank = self.M // self.world
        if self.per_rank < self.batch_size:
            raise ValueError(f"{self.path}: {self.M} images over {self.world} rank(s) leave {self.per_rank} per rank, fewer than one "
                             f"batch of {self.batch_size}")
        self.batches_per_epoch = self.per_rank // self.batch_size
        self.random_flip = bool(random_flip)
        if resident not in ("auto", "device", "host"):
            raise ValueError(f"ImageStore: resident {resident!r} is not one of 'auto', 'device', 'host'")
        self.resident = resident if resident != "auto" else ("device" if self.arr.nbytes <= device_budget_bytes else "host")
        self._pos, self._seek = (0, 0), None
        self._feeders = weakref.WeakSet()
        self._plan_dev = self._flips_dev = None
        if self.resident == "device" and self.device.type == "cuda":
            with warnings.catch_warnings():      # a memory-mapped .npy is read-only: it is only read from here
                warnings.simplefilter("ignore")
                self.store_dev = torch.from_numpy(np.ascontiguousarray(self.arr)).to(self.device)
            self.labels_dev = torch.from_numpy(self.labels).to(self.device) if self.with_labels else None

    # ------------------------------------------------------------------------------------------------ order
    def plan(self, epoch):
        """(rows int64 [M // world], flips uint8 [M // world] or None) of this rank for `epoch`, on the CPU."""
        perm = torch.randperm(self.M, generator=torch.Generator().manual_seed(self.seed + int(epoch)))
        rows = perm[self.rank::self.world][:self.per_rank].contiguous()
        flips = None
        if self.random_flip:
            g = torch.Generator().manual_seed(flip_seed(self.seed, epoch, self.rank))
            flips = (torch.rand(self.per_rank, generator=g) < 0.5).to(torch.uint8)
        return rows, flips

    def raw(self, rows):
        """(uint8 [B, C, H, W], labels int64 [B] or None) of the file's rows `rows` (int64, any order) on the store's device: the
        stored bytes, neither flipped nor normalised (eval_bpd.py dequantises them itself)."""
        rows = torch.as_tensor(rows, dtype=torch.int64).cpu()
        if rows.numel() and not (0 <= int(rows.min()) and int(rows.max()) < self.M):
            raise ValueError(f"ImageStore.raw: rows must lie in [0, {self.M})")
        if self.resident == "device" and self.device.type == "cuda":
            r = rows.to(self.device)
            u8, y = self.store_dev[r], (self.labels_dev[r] if self.with_labels else None)
        else:
            u8 = torch.from_numpy(np.ascontiguousarray(self.arr[rows.numpy()])).to(self.device)
            y = torch.from_numpy(self.labels[rows.numpy()]).to(self.device) if self.with_labels else None
        return u8.permute(0, 3, 1, 2).contiguous(), y

    def epoch_flips(self, epoch, flips):
        """The epoch's flip bits where the batch is formed, uploaded once per epoch."""
        if flips is None or self.device.type != "cuda":
            return flips
        if self._flips_dev is None or self._flips_dev[0] != epoch:
            self._flips_dev = (epoch, flips.to(self.device))
        return self._flips_dev[1]

    def _resident_batches(self, epochs, first):
        for e in epochs:
            rows, flips = self.plan(e)
            on_gpu = self.device.type == "cuda"
            if on_gpu:
                from . import ops
                rows_d, flips_d = rows.to(self.device), self.epoch_flips(e, flips)
            for b in range(first, self.batches_per_epoch):
                sl = slice(b * self.batch_size, (b + 1) * self.batch_size)
                if on_gpu:
                    images = ops.image_batch(self.store_dev, rows_d[sl], flips_d[sl] if flips_d is not None else None, self.norm)
                    y = self.labels_dev[rows_d[sl]] if self.with_labels else None
                else:
                    r = rows[sl].numpy()
                    images = form_batch(torch.from_numpy(np.ascontiguousarray(self.arr[r])), flips[sl] if flips is not None else None, self.norm)
                    y = torch.from_numpy(self.labels[r]) if self.with_labels else None
                yield images, y, e, b
            first = 0

    def _walk(self, epochs, first):
        """(images, labels, epoch, batch) over `epochs` from batch `first` of the first one, by the resident mode's path."""
        if self.resident == "device":
            yield from self._resident_batches(epochs, first)
            return
        feeder = _HostFeeder(self, epochs, first)
        self._feeders.add(feeder)
        try:
            while True:
                item = feeder.take()
                if item is None:
                    return
                yield item
        finally:
            feeder.close()

    # ------------------------------------------------------------------------------------------------ iteration
    def epoch(self, e):
        """(images fp32 [B, C, H, W], labels int64 [B] or None) for every batch of epoch e."""
        walk = self._walk([int(e)], 0)
        try:
            for images, y, ep, b in walk:
                self._pos = (ep, b + 1) if b + 1 < self.batches_per_epoch else (ep + 1, 0)
                yield images, y
        finally:
            walk.close()

    def batches(self, start_epoch=0):
        """(images, {"y": labels} or {}) forever, epoch after epoch, from the first batch of epoch start_epoch — or, after a seek(), from
        the position it set (one call takes it)."""
        (e0, b0), self._seek = (self._seek or (int(start_epoch), 0)), None
        walk = self._walk(itertools.count(e0), b0)
        try:
            for images, y, ep, b in walk:
                self._pos = (ep, b + 1) if b + 1 < self.batches_per_epoch else (ep + 1, 0)
                yield images, ({"y": y} if y is not None else {})
        finally:
            walk.close()

    def state(self):
        """Position of the batch the running iterator yields next: {"epoch", "batch"}."""
        return {"epoch": self._pos[0], "batch": self._pos[1]}

    def seek(self, epoch, batch=0):
        """Set the position the next batches() call starts from (a running iterator is not moved)."""
        if not (epoch >= 0 and 0 <= batch < self.batches_per_epoch):
            raise ValueError(f"ImageStore.seek: epoch {epoch}, batch {batch} of {self.batches_per_epoch}")
        self._pos = self._seek = (int(epoch), int(batch))

    def close(self):
        for f in list(self._feeders):
            f.close()

    def describe(self):
        """The start-up line of the training scripts."""
        H, W, C = self.image_shape
        return (f"data: {self.path}: {self.M} images {H}x{W}x{C}, labels {'yes' if self.has_labels else 'no'}, resident {self.resident}, "
                f"{self.batches_per_epoch} batches of {self.batch_size} per epoch on each of {self.world} rank(s)")
