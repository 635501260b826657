"""Training and evaluation from a feature cache that is RESIDENT in device memory.

`cache.FeatureShard.batch` serves one contiguous image range per call through a numpy copy, a fresh pinned buffer and an
upload, on the thread that issues the step -- and a shuffled batch is one such call per image plus a `torch.cat` per
tensor.  The fused training step is host-bound, so every microsecond of that lands on the step time.

An MI355X holds 288 GB.  The HICO-DET training set is about 38 k images x at most 30 kept boxes x 12 544 features: 28 GB
in bf16, 57 GB in fp32.  `ResidentFeatureSet` therefore uploads the shards ONCE, as they are on disk, and every batch is
then assembled on the device, in the sampler's order, by one launch of `skg_cache_gather_x` (include/skghoi.h): no
per-batch host copy, no pinned allocation, no host synchronisation, no PCIe traffic.

    rset = ResidentFeatureSet(shard_paths, raw_detections, targets)
    head.box_roi_pool = BatchPool()
    rset.check_alignment(head)                      # the cache was produced under THIS head's thresholds and mode
    trainer.Trainer(head, optimizer, None, rset.loader(batch_size=4), lazy_losses=True)(num_epochs)

The horizontal-flip augmentation (DataFactory, utils.py:85-86, 115-118, 140-143).  A pooled tile of the mirrored image is
not the mirrored tile, so a flip cannot be made from the plain rows after the fact: the set holds a SECOND variant of every
image, pooled from the mirrored maps by `cache.produce_shard(..., mirror=True)`, and serves one of the two per image:

    rset = ResidentFeatureSet(shard_paths, raw_detections, targets, flipped_shard_paths=flipped_paths)
    loader = rset.loader(batch_size=4, flips=trainer.draw_flips(len(rset)))      # the reference's coins, drawn once
    loader = rset.loader(batch_size=4, flips="epoch")                            # or fresh coins at every set_epoch

Every ragged array then holds 2 * n_images entries, entry n_images + i being the flipped variant of image i: its rows and
global row from the flipped shards, its boxes / boxes_h / boxes_o flipped once on the host about the image's own width
(`trainer.horizontal_flip_boxes`), everything else repeated.  The epoch's order becomes i + n_images * coin[i], so a batch
is still ONE gather launch and the device does no arithmetic for the flip.  What this flip is: the `trainer.hflip_sample`
semantics -- every cached map mirrored along its last axis, the boxes with it.  What it is not: the backbone run on the
mirrored image (a convolution of the mirrored image is not the mirror of the convolution once strides and padding are
asymmetric).  Whoever has those maps puts them through the plain producer and passes the shards as flipped_shard_paths.

Not covered: reading the resident rows straight into box_head layer 1, and sets larger than device
memory.
"""
import math
import weakref

import numpy as np
import torch

from . import _capi
from .cache import MAGIC, _DT, _HDR

STAGING_BYTES = 64 << 20          # the ONE pinned staging buffer of the upload (used as two halves)
LIVE_BATCHES = 3                  # batches of one loader that may be alive at once: the one in use + Trainer's two-batch look-ahead
_TORCH_DT = {0: torch.float32, 1: torch.float16, 2: torch.bfloat16}
_TARGET_KEYS = ("boxes_h", "boxes_o", "labels")           # packed first, then "object" and "hoi", then whatever else there is


def epoch_order(n, epoch=0, world_size=1, rank=0, seed=0, shuffle=True, drop_last=False):
    """The indices torch.utils.data.DistributedSampler(range(n), world_size, rank, shuffle, seed, drop_last) yields after
    set_epoch(epoch), as a list: randperm from a generator of its OWN seeded seed + epoch (the global CPU generator --
    the head's TransH and sampling draws -- is not touched), padded by wrapping (or cut with drop_last) to a multiple of
    world_size, then [rank::world_size]."""
    n, world_size, rank = int(n), int(world_size), int(rank)
    if world_size < 1 or not 0 <= rank < world_size:
        raise ValueError("rank %d outside a world of %d" % (rank, world_size))
    if drop_last and n % world_size:
        per = math.ceil((n - world_size) / world_size)
    else:
        per = math.ceil(n / world_size)
    total = per * world_size
    if shuffle:
        g = torch.Generator()
        g.manual_seed(int(seed) + int(epoch))
        idx = torch.randperm(n, generator=g).tolist()
    else:
        idx = list(range(n))
    if not drop_last:
        pad = total - len(idx)
        if pad <= len(idx):
            idx += idx[:pad]
        else:
            idx += (idx * math.ceil(pad / len(idx)))[:pad]
    else:
        idx = idx[:total]
    return idx[rank:total:world_size]


def epoch_coins(n, epoch=0, seed=0):
    """The coins of `flips="epoch"`: one 0/1 int64 per image, a function of (seed, epoch) only, from a generator of their
    own (the global CPU generator is not touched; nor is it the stream `epoch_order` shuffles with)."""
    g = torch.Generator()
    g.manual_seed((int(seed) * 1000003 + int(epoch) + 0x464C4950) & ((1 << 63) - 1))
    return torch.randint(0, 2, (int(n),), generator=g)


class _ShardHeader:
    """The header of a SKGFC001 shard (cache.py), read the way FeatureShard reads it -- without mapping the payload."""

    def __init__(self, path):
        self.path = path
        with open(path, "rb") as f:
            magic, self.code, self.C, self.pool, self.gdim, self.n_images, self.n_boxes = _HDR.unpack(f.read(_HDR.size))
            if magic != MAGIC:
                raise ValueError("%s is not a SKGFC001 feature shard" % path)
            if self.code not in _DT:
                raise ValueError("%s: unknown dtype code %d" % (path, self.code))
            self.box_off = np.frombuffer(f.read(8 * (self.n_images + 1)), dtype=np.int64)
            self.image_hw = np.frombuffer(f.read(8 * self.n_images), dtype=np.float32).reshape(-1, 2)
            self.glob = np.frombuffer(f.read(4 * self.n_images * self.gdim), dtype=np.float32).reshape(self.n_images, -1)
            pos = f.tell()
        self.payload_off = pos + ((-pos) % 4096)
        self.row = self.C * self.pool * self.pool
        self.payload_bytes = self.n_boxes * self.row * np.dtype(_DT[self.code]).itemsize
        if len(self.box_off) != self.n_images + 1 or (self.n_images and int(self.box_off[-1]) != self.n_boxes) or \
                (np.diff(self.box_off) < 0).any():
            raise ValueError("%s: inconsistent box offsets" % path)


class _Ragged:
    """One ragged array of the set: rows in storage order on the device, the per-image offsets (device) and counts (host)."""
    __slots__ = ("name", "src", "off", "counts", "row_elems", "src_code", "dst_code", "dst_dtype", "tail")

    def __init__(self, name, src, off, counts, row_elems, src_code, dst_code, dst_dtype, tail):
        self.name, self.src, self.off, self.counts = name, src, off, counts
        self.row_elems, self.src_code, self.dst_code, self.dst_dtype, self.tail = row_elems, src_code, dst_code, dst_dtype, tail


def _pack(name, per_image, dtype=None, tail=None):
    """Host side of a ragged array: (flat CPU tensor [rows, *tail], counts)."""
    ts = []
    for i, t in enumerate(per_image):
        t = torch.as_tensor(t)
        if dtype is not None:
            t = t.to(dtype)
        if tail is not None:
            t = t.reshape((-1,) + tuple(tail))
        if t.dim() == 0:
            raise ValueError("%s of image %d has no leading dimension" % (name, i))
        ts.append(t)
    if len({(t.dtype, tuple(t.shape[1:])) for t in ts}) > 1:
        raise ValueError("%s: dtype or row shape differs between images" % name)
    if ts and math.prod(ts[0].shape[1:]) == 0:
        raise ValueError("%s: rows without elements" % name)
    counts = np.array([int(t.shape[0]) for t in ts], np.int64)
    return ts, counts


class ResidentFeatureSet:
    """The shards of a feature cache, the raw detections and (optionally) the targets of their images, uploaded once.

    shard_paths: SKGFC001 files (cache.write_feature_shard / produce_shard), in image order; all of one dtype, C, pool and
    gdim.  The payload goes through ONE bounded pinned staging buffer into one device arena IN THE STORED DTYPE -- bf16 stays
    16-bit -- and is widened (exactly) by the gather, or handed out as stored with keep_dtype=True.
    detections: the RAW per-image dicts {boxes, scores, labels} (cache.read_detections_json), not the kept ones: the head's
    `preprocess` runs again on every batch and, being deterministic, reproduces the row order the shard was produced in
    (`check_alignment` verifies it).  targets: per-image dicts of tensors whose leading dimension is the ground-truth
    pair -- boxes_h, boxes_o, labels, and object / hoi when present -- or None.
    flipped_shard_paths: the shards of the horizontally flipped variant (cache.produce_shard(..., mirror=True)) or None.  They
    hold the same images in the same order with the same dtype, C, pool, gdim and image_hw; their per-image box counts may
    differ (a flipped box's width can differ by an ulp, so the NMS may keep another set).  With them every array holds
    2 * n_images entries -- `box_counts`, `image_shapes` and `arrays` alike -- and entry n_images + i is the flipped variant
    of image i (module docstring); `loader(flips=...)` picks a variant per image.
    Everything is validated on the host before the first device call (ValueError); a set that does not fit into the free
    device memory raises MemoryError."""

    def __init__(self, shard_paths, detections, targets=None, device="cuda", keep_dtype=False, flipped_shard_paths=None):
        shard_paths = list(shard_paths)
        if not shard_paths:
            raise ValueError("a resident feature set needs at least one shard")
        hdrs = [_ShardHeader(p) for p in shard_paths]
        ref = next((h for h in hdrs if h.n_images), hdrs[0])        # (a shard without images carries no C / pool)
        for h in hdrs:
            for f in ("code", "C", "pool", "gdim"):
                if h.n_images and getattr(h, f) != getattr(ref, f):
                    raise ValueError("shards differ in %s: %s has %d, %s has %d" % (
                        {"code": "dtype"}.get(f, f), ref.path, getattr(ref, f), h.path, getattr(h, f)))
        self.code, self.C, self.pool, self.gdim, self.row = ref.code, ref.C, ref.pool, ref.gdim, ref.row
        self.n_images = sum(h.n_images for h in hdrs)
        self.flipped = flipped_shard_paths is not None
        fhdrs = []
        if self.flipped:
            flipped_shard_paths = list(flipped_shard_paths)
            if not flipped_shard_paths:
                raise ValueError("flipped_shard_paths holds no shard")
            fhdrs = [_ShardHeader(p) for p in flipped_shard_paths]
            for h in fhdrs:
                for f in ("code", "C", "pool", "gdim"):
                    if h.n_images and getattr(h, f) != getattr(ref, f):
                        raise ValueError("flipped shards differ in %s: %s has %d, %s has %d" % (
                            {"code": "dtype"}.get(f, f), ref.path, getattr(ref, f), h.path, getattr(h, f)))
            if sum(h.n_images for h in fhdrs) != self.n_images:
                raise ValueError("the shards hold %d images, the flipped shards %d"
                                 % (self.n_images, sum(h.n_images for h in fhdrs)))
            hw, fhw = (np.concatenate([h.image_hw for h in hs]) for hs in (hdrs, fhdrs))
            if not np.array_equal(hw, fhw):
                i = int(np.nonzero((hw != fhw).any(axis=1))[0][0])
                raise ValueError("image %d: image_hw %s in the shards, %s in the flipped shards (not the same images in the "
                                 "same order)" % (i, tuple(hw[i]), tuple(fhw[i])))
        self.n_entries = self.n_images * (2 if self.flipped else 1)
        detections = list(detections)
        if len(detections) != self.n_images:
            raise ValueError("the shards hold %d images, %d detections were given" % (self.n_images, len(detections)))
        if self.n_images == 0:
            raise ValueError("the shards hold no image")
        for i, d in enumerate(detections):
            if not isinstance(d, dict) or any(k not in d for k in ("boxes", "scores", "labels")):
                raise ValueError("detections[%d] is not a dict of boxes, scores and labels" % i)
        self.target_keys = None
        if targets is not None:
            targets = list(targets)
            if len(targets) != self.n_images:
                raise ValueError("the shards hold %d images, %d targets were given" % (self.n_images, len(targets)))
            keys = set(targets[0])
            for i, t in enumerate(targets):
                if set(t) != keys:
                    raise ValueError("targets[%d] has keys %s, targets[0] has %s" % (i, sorted(t), sorted(keys)))
            known = _TARGET_KEYS + ("object", "hoi")
            self.target_keys = [k for k in known if k in keys] + sorted(keys - set(known))
            missing = [k for k in ("boxes_h", "boxes_o") if k not in keys]
            if missing:
                raise ValueError("targets lack %s" % ", ".join(missing))
        # ---- host packing (still no device call unless the caller's tensors live on one)
        host = []                                                   # (name, per-image tensors, counts)
        boxes, n_det = _pack("boxes", [d["boxes"] for d in detections], torch.float32, (4,))
        scores, n_s = _pack("scores", [d["scores"] for d in detections], torch.float32, ())
        labels, n_l = _pack("labels", [d["labels"] for d in detections], torch.int64, ())
        if not (np.array_equal(n_det, n_s) and np.array_equal(n_det, n_l)):
            raise ValueError("boxes, scores and labels of an image differ in length")
        host += [("boxes", boxes, n_det), ("scores", scores, n_det), ("labels", labels, n_det)]
        n_gt = None
        if targets is not None:
            for k in self.target_keys:
                ts, c = _pack("targets[%r]" % k, [t[k] for t in targets], None, (4,) if k in ("boxes_h", "boxes_o") else None)
                if n_gt is None:
                    n_gt = c
                elif not np.array_equal(n_gt, c):
                    raise ValueError("targets[%r] differs in length from the other keys of its image" % k)
                host.append(("t:" + k, ts, c))
        if 2 + len(host) > _capi.CACHE_MAX_ARRAYS:
            raise ValueError("%d arrays per batch, the gather takes %d" % (2 + len(host), _capi.CACHE_MAX_ARRAYS))
        self.det_counts, self.gt_counts = n_det, n_gt
        self.image_shapes = [(int(a), int(b)) for h in hdrs for a, b in h.image_hw]
        if self.flipped:                                            # entry n_images + i: the flipped variant of image i
            from .trainer import horizontal_flip_boxes
            widths = [w for _, w in self.image_shapes]
            flip = lambda ts: [horizontal_flip_boxes(w, t) for w, t in zip(widths, ts)]
            host = [(name, ts + (flip(ts) if name in ("boxes", "t:boxes_h", "t:boxes_o") else ts), np.concatenate([c, c]))
                    for name, ts, c in host]
            self.image_shapes = self.image_shapes * 2
        hdrs = hdrs + fhdrs                                         # storage order: the plain shards, then the flipped ones
        self.box_counts = np.concatenate([np.diff(h.box_off) for h in hdrs]).astype(np.int64)
        self.n_boxes = int(self.box_counts.sum())
        self.keep_dtype = bool(keep_dtype)
        item = np.dtype(_DT[self.code]).itemsize
        self.arena_bytes = self.n_boxes * self.row * item
        small = sum(sum(t.numel() * t.element_size() for t in ts) for _, ts, _ in host) + 4 * self.n_entries * self.gdim \
            + 8 * (self.n_entries + 1) * 4
        # ---- device
        dev = torch.device(device)
        if dev.type != "cuda":
            raise _capi.SkgError("a resident feature set lives on a HIP device (device=%s)" % dev)
        if dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        self.device = dev
        need = self.arena_bytes + small
        free, _ = torch.cuda.mem_get_info(dev)
        if need > free:
            raise MemoryError("the resident feature set needs %d bytes of device memory%s, %d are free on %s"
                              % (need, " (both variants: the plain and the flipped shards)" if self.flipped else "", free, dev))
        self.arena = torch.empty(max(self.arena_bytes, 16), dtype=torch.uint8, device=dev)
        self._upload_payload(hdrs)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        offs = lambda c: up(np.concatenate([[0], np.cumsum(c)]).astype(np.int64))
        pooled_src = self.arena[:self.arena_bytes].view(_TORCH_DT[self.code]) if self.arena_bytes else \
            self.arena.view(_TORCH_DT[self.code])
        glob = up(np.concatenate([h.glob for h in hdrs if h.n_images]).astype(np.float32).reshape(self.n_entries, self.gdim))
        self.box_off = offs(self.box_counts)
        out_dt = _TORCH_DT[self.code] if self.keep_dtype else torch.float32
        self.arrays = [
            _Ragged("pooled", pooled_src, self.box_off, self.box_counts, self.row, self.code,
                    self.code if self.keep_dtype else _capi.DTYPE_F32, out_dt, (self.C, self.pool, self.pool)),
            _Ragged("global", glob, offs(np.ones(self.n_entries, np.int64)), np.ones(self.n_entries, np.int64), self.gdim,
                    _capi.DTYPE_F32, _capi.DTYPE_F32, torch.float32, (self.gdim, 1, 1))]
        shared = {}
        for name, ts, c in host:
            tail = tuple(ts[0].shape[1:])
            per_row = math.prod(tail)
            flat = torch.cat([t.reshape(t.shape[0], per_row) for t in ts]).contiguous()
            src = flat.to(dev) if flat.numel() else torch.zeros(16, dtype=torch.uint8, device=dev).view(flat.dtype)
            key = c.tobytes()
            if key not in shared:
                shared[key] = offs(c)
            if flat.dtype == torch.float32:
                code, elems = _capi.DTYPE_F32, per_row
            else:
                code, elems = _capi.DTYPE_BYTES, per_row * flat.element_size()
            self.arrays.append(_Ragged(name, src, shared[key], c, elems, code, code, flat.dtype, tail))

    def _upload_payload(self, hdrs):
        """Disk -> the two halves of one pinned buffer -> the arena, the read of one half beside the copy of the other."""
        if not self.arena_bytes:
            return
        half = max(1 << 12, min(STAGING_BYTES // 2, self.arena_bytes))
        stage = torch.empty(2 * half, dtype=torch.uint8).pin_memory()
        views = [stage[:half].numpy(), stage[half:].numpy()]
        done = [None, None]
        stream = torch.cuda.current_stream(self.device)
        pos, k = 0, 0
        for h in hdrs:
            left = h.payload_bytes
            if not left:
                continue
            with open(h.path, "rb") as f:
                f.seek(h.payload_off)
                while left:
                    n = min(half, left)
                    if done[k] is not None:
                        done[k].synchronize()               # the half's previous copy has left it
                    got = f.readinto(memoryview(views[k])[:n])
                    if got != n:
                        raise ValueError("%s: payload ends %d bytes early" % (h.path, left - (got or 0)))
                    self.arena[pos:pos + n].copy_(stage[k * half:k * half + n], non_blocking=True)
                    done[k] = torch.cuda.Event()
                    done[k].record(stream)
                    pos += n; left -= n; k ^= 1
        for e in done:
            if e is not None:
                e.synchronize()

    def __len__(self):
        return self.n_images

    def loader(self, batch_size=4, shuffle=True, world_size=1, rank=0, seed=0, drop_last=False, flips=None):
        """flips: None (no flip), a 0/1 tensor of n_images fixed coins (the reference's: trainer.draw_flips(n), drawn once
        from the global generator by the caller) or "epoch" (fresh coins at every set_epoch, `epoch_coins`)."""
        return ResidentLoader(self, batch_size, shuffle, world_size, rank, seed, drop_last, flips)

    @torch.no_grad()
    def check_alignment(self, head, batch_size=64):
        """One pass over the set: `head.preprocess`, in the head's CURRENT mode (training appends the ground truth), must keep
        exactly box_off[i + 1] - box_off[i] boxes of every image i.  Raises ValueError naming the first image that differs --
        the guard against a cache produced under other thresholds, another mode or other detections.  A set with flipped
        shards is checked in both variants (the plain one first), and the error names the variant too."""
        if head.training and self.target_keys is None:
            raise ValueError("a head in training mode appends the ground truth: the set was built without targets")
        variants = [(None, "")] if not self.flipped else \
            [(torch.zeros(self.n_images, dtype=torch.int64), " (plain variant)"),
             (torch.ones(self.n_images, dtype=torch.int64), " (flipped variant)")]
        for coins, which in variants:
            first = 0
            loader = self.loader(batch_size=min(int(batch_size), _capi.CACHE_MAX_BATCH), shuffle=False, flips=coins)
            for _, det, _, tg in loader:
                kept = head.preprocess(det, tg)
                for k, d in enumerate(kept):
                    have, want = int(d["boxes"].shape[0]), int(self.box_counts[loader.order[first + k]])
                    if have != want:
                        raise ValueError("image %d%s: the head keeps %d boxes, the cache holds %d rows (produced under other "
                                         "thresholds, another mode or other detections)" % (first + k, which, have, want))
                first += len(det)
        return self.n_images


class _Features(dict):
    """The `features` mapping of a batch ({"3": ..., "pooled": ...}): a dict that can be weakly referenced -- its ring slot
    is free again once nothing refers to it (the batch tuple does, and so does a training step in flight)."""


class _Slot:
    """Output buffers of one batch: a flat buffer per array and the descriptor table the launch reads."""

    def __init__(self, rset, caps):
        self.caps = list(caps)
        self.bufs = []
        self.desc = (_capi.CacheArray * len(rset.arrays))()
        for k, (a, cap) in enumerate(zip(rset.arrays, caps)):
            buf = torch.empty((max(1, cap),) + tuple(a.tail), dtype=a.dst_dtype, device=rset.device)
            self.bufs.append(buf)
            d = self.desc[k]
            d.src, d.src_off, d.row_elems = a.src.data_ptr(), a.off.data_ptr(), a.row_elems
            d.src_dtype, d.dst_dtype, d.dst, d.dst_rows = a.src_code, a.dst_code, buf.data_ptr(), 0
        self.live = None                 # weak reference to the `features` mapping of the batch handed out from this slot


class ResidentLoader:
    """Iterable over the batches of a ResidentFeatureSet in torch.utils.data.DistributedSampler's order (`epoch_order`).
    `set_epoch(e)` forms the epoch's order, validates it on the host and uploads it once; a batch is then its position in
    that order and ONE `skg_cache_gather_x` launch on the current stream.  Each batch is

        (features, detections, image_shapes, targets)

    features = {"3": global features [B, gdim, 1, 1] fp32, "pooled": [sum N, C, p, p]} (fp32, or the stored dtype with
    keep_dtype) for a head whose box_roi_pool is a `BatchPool`; detections / targets: lists of per-image dicts, views of the
    gathered flat buffers split by host-known counts (targets is None for a set without them); image_shapes: host ints.

    Output buffers come from a ring of LIVE_BATCHES + 1 slots sized at set_epoch for the epoch's largest batch, so the
    steady state allocates nothing.  At most LIVE_BATCHES (3) batches may be ALIVE at once -- the one in use and the two
    of Trainer's look-ahead; the fourth slot is the one being filled.  A batch is alive while the tuple the loader yielded
    -- precisely: its `features` mapping -- is referenced: tensors taken out of it and kept beyond that will be
    overwritten, clone them.  Asking for a further
    batch while every slot is alive allocates fresh buffers for it instead of overwriting a live batch.
    `loader.sampler` is the loader itself, so `Trainer.train_epoch` reshuffles it like a DataLoader's sampler.

    flips (a set with flipped shards only): None, fixed coins or "epoch" (ResidentFeatureSet.loader).  set_epoch turns the
    sampler's order -- kept in `base_order`, the coins of the epoch in `coins` -- into entries i + n_images * coin[i] before
    validating and uploading it; `order` holds those entries, and the row counts, the caps and image_shapes follow them."""

    def __init__(self, rset, batch_size=4, shuffle=True, world_size=1, rank=0, seed=0, drop_last=False, flips=None):
        batch_size = int(batch_size)
        if not 1 <= batch_size <= _capi.CACHE_MAX_BATCH:
            raise ValueError("batch_size must be in 1 .. %d" % _capi.CACHE_MAX_BATCH)
        self.flips = None
        if flips is not None:
            if not getattr(rset, "flipped", False):
                raise ValueError("flips were asked of a set without flipped shards (flipped_shard_paths)")
            if isinstance(flips, str):
                if flips != "epoch":
                    raise ValueError("flips must be None, a 0/1 tensor of %d coins or \"epoch\" (got %r)"
                                     % (rset.n_images, flips))
                self.flips = "epoch"
            else:
                coins = torch.as_tensor(flips).detach().cpu().reshape(-1)
                if coins.numel() != rset.n_images:
                    raise ValueError("%d coins for %d images" % (coins.numel(), rset.n_images))
                if not bool(((coins == 0) | (coins == 1)).all()):
                    raise ValueError("coins outside {0, 1}")
                self.flips = coins.to(torch.int64)
        epoch_order(1, 0, world_size, rank)                        # (validates world_size / rank)
        self.set, self.batch_size, self.shuffle = rset, batch_size, bool(shuffle)
        self.world_size, self.rank, self.seed, self.drop_last = int(world_size), int(rank), int(seed), bool(drop_last)
        self.sampler = self
        self.epoch = 0
        self.num_samples = len(epoch_order(rset.n_images, 0, world_size, rank, seed, False, drop_last))
        self.order = None                 # host list of the uploaded epoch (entries: i + n_images * coin[i])
        self.base_order = None            # the sampler's order of that epoch (images)
        self.coins = None                 # int64 [n_images]: the coins of that epoch, or None
        self._order_dev = None
        self._ready = None                # epoch whose order is on the device
        self._ring = []
        self._caps = [0] * len(rset.arrays)
        self.fresh_allocations = 0        # batches served outside the ring (more than LIVE_BATCHES alive)

    def __len__(self):
        return -(-self.num_samples // self.batch_size)

    def set_epoch(self, epoch):
        rset = self.set
        self.epoch = int(epoch)
        order = epoch_order(rset.n_images, self.epoch, self.world_size, self.rank, self.seed, self.shuffle, self.drop_last)
        arr = np.asarray(order, dtype=np.int64).reshape(-1)
        if arr.shape[0] != self.num_samples or (arr.shape[0] and (arr.min() < 0 or arr.max() >= rset.n_images)):
            raise ValueError("epoch order outside 0 .. %d" % (rset.n_images - 1))
        self.base_order, self.coins = order, None
        if self.flips is not None:
            self.coins = epoch_coins(rset.n_images, self.epoch, self.seed) if isinstance(self.flips, str) else self.flips
            arr = arr + rset.n_images * self.coins.numpy()[arr]
            order = arr.tolist()
        self.order = order
        # host-known row counts: per array the counts of every slot of the epoch and the rows of every batch
        starts = np.arange(0, self.num_samples, self.batch_size)
        self._slot_counts, self._batch_rows = [], []
        for k, a in enumerate(rset.arrays):
            c = a.counts[arr]
            rows = np.add.reduceat(c, starts) if len(starts) else np.zeros(0, np.int64)
            self._slot_counts.append(c.tolist())
            self._batch_rows.append(rows.tolist())
            self._caps[k] = max(self._caps[k], int(rows.max()) if len(rows) else 0)
        if arr.shape[0]:
            self._order_dev = torch.from_numpy(arr.astype(np.int32)).to(rset.device)
        self._ready = self.epoch

    def _slot(self):
        rset = self.set
        for i, s in enumerate(self._ring):
            if s.live is None or s.live() is None:
                if any(c < need for c, need in zip(s.caps, self._caps)):
                    s = self._ring[i] = _Slot(rset, self._caps)
                return s
        s = _Slot(rset, self._caps)
        if len(self._ring) <= LIVE_BATCHES:
            self._ring.append(s)
        else:
            self.fresh_allocations += 1
        return s

    def _batch(self, k):
        rset = self.set
        first = k * self.batch_size
        b = min(self.batch_size, self.num_samples - first)
        s = self._slot()
        desc = s.desc
        for a in range(len(rset.arrays)):
            desc[a].dst_rows = self._batch_rows[a][k]
        _capi.check(_capi.lib().skg_cache_gather_x(desc, len(rset.arrays), self._order_dev.data_ptr(), self.num_samples,
                                                   first, b, torch.cuda.current_stream(rset.device.index).cuda_stream),
                    "skg_cache_gather_x")
        flat = {}
        for a, (arr, buf) in enumerate(zip(rset.arrays, s.bufs)):
            rows = self._batch_rows[a][k]
            flat[arr.name] = (buf[:rows], self._slot_counts[a][first:first + b])
        features = _Features({"3": flat["global"][0], "pooled": flat["pooled"][0]})
        split = lambda name: flat[name][0].split(flat[name][1])
        detections = [dict(boxes=x, scores=y, labels=z) for x, y, z in zip(split("boxes"), split("scores"), split("labels"))]
        targets = None
        if rset.target_keys is not None:
            cols = [split("t:" + key) for key in rset.target_keys]
            targets = [dict(zip(rset.target_keys, row)) for row in zip(*cols)]
        shapes = [rset.image_shapes[i] for i in self.order[first:first + b]]
        s.live = weakref.ref(features)
        return features, detections, shapes, targets

    def __iter__(self):
        if self._ready != self.epoch or self.order is None:
            self.set_epoch(self.epoch)
        for k in range(len(self)):
            yield self._batch(k)


class BatchPool(torch.nn.Module):
    """`box_roi_pool` stand-in for batches of a ResidentLoader: returns features["pooled"], the rows the gather put there."""

    def forward(self, features, boxes, image_shapes):
        n = sum(len(b) for b in boxes)
        pooled = features.get("pooled") if hasattr(features, "get") else None
        if pooled is None or pooled.shape[0] != n:
            raise RuntimeError("cached features hold %s rows, the head kept %d boxes" % (
                None if pooled is None else pooled.shape[0], n))
        return pooled
