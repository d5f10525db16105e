"""Loader construction for the fine-tune CLI (reference: evaluation/feature.py:101-190,533-608).

The reference builds its datasets through the ``vision_datasets`` hub (download, manifests, PIL decoding,
torchvision transforms); that dataset layer is outside this build.  What the harness needs from it is kept:
three loaders over ``(image fp32 (3,R,R), target)`` pairs with the reference's batch size (64), the
class-balanced deterministic validation split -- per class the first ceil(20 %) samples go to validation,
feature.py:137-149, or the greedy multi-label rule of feature.py:150-163 -- and train / val being ``Subset`` views of ONE
dataset so that ``merge_trainval_loader`` can put them back together for the final run.

Sources: ``<DATASET.ROOT>/<DATASET.DATASET>.npz`` holding already preprocessed tensors
(``train_images``, ``train_labels``, ``test_images``, ``test_labels``; images float32 (N,3,R,R) or uint8, in
which case INPUT.MEAN / INPUT.STD are applied -- uint8 images may also have their native size (N,3,h,w), and are then resized
and centre-cropped like the reference's transform, by the engine per batch or with ``DATASET.RESIZE_ON_HOST`` at load time; labels
(N,) class indices, or (N, C) multi-hot with C > 1 -- bool, integer
or float -- which become float32 targets for BCEWithLogitsLoss; a RAGGED archive -- every image its own size -- holds
``*_images`` as ONE 1-D uint8 pool of dense (3, h_i, w_i) blocks and ``*_shapes`` (N, 2) = (h, w), see ``_ragged_tensors``), or
``DATASET.DATASET == 'synthetic'`` (seeded random tensors,
for smoke runs and benchmarks).
"""
from __future__ import annotations

import logging
import math
import os

import numpy as np
import torch

from .feature import create_dataloader


class _Tensors:
    """The whole (images, labels) set, resident on one device."""

    def __init__(self, images, labels):
        self.images, self.labels = images, labels

    def __len__(self):
        return self.images.shape[0]

    def __getitem__(self, i):
        return self.images[i], self.labels[i]


class _View:
    """Subset-like view (``.dataset`` is the full set, like torch.utils.data.Subset, which is what
    merge_trainval_loader checks)."""

    def __init__(self, full, indices):
        self.dataset, self.indices = full, indices

    def __len__(self):
        return len(self.indices)

    def __getitem__(self, i):
        return self.dataset[int(self.indices[i])]


class TensorLoader:
    """DataLoader stand-in for in-memory tensor sets: one index-gather per batch instead of stacking 64 samples on
    the host (the stock DataLoader spent 4.6 s of an 8.7 s few-shot run in torch.stack), and -- when the set fits --
    resident on the GPU, so a step does no host-to-device copy at all.  Same iteration contract as the loaders of
    the reference's get_dataloader: no drop_last, reshuffled every epoch when ``shuffle``."""

    def __init__(self, dataset, batch_size=64, shuffle=False, num_workers=0, pin_memory=False):
        self.dataset, self.batch_size, self.shuffle = dataset, batch_size, shuffle
        self.num_workers, self.pin_memory = num_workers, pin_memory

    def _base(self):
        if isinstance(self.dataset, _View):
            full = self.dataset.dataset
            key = (id(self.dataset.indices), len(self.dataset.indices), full.images.device)
            if getattr(self, "_idx_key", None) != key:           # the index list of a view is uploaded once, not per batch
                self._idx = torch.as_tensor(self.dataset.indices, dtype=torch.long, device=full.images.device)
                self._idx_key = key
            return full, self._idx
        return self.dataset, None

    def __len__(self):
        return (len(self.dataset) + self.batch_size - 1) // self.batch_size

    def iter_indices(self):
        """The index tensors of one epoch's batches (on the device the set lives on)."""
        full, idx = self._base()
        n = len(self.dataset)
        dev = full.images.device
        order = torch.randperm(n).to(dev) if self.shuffle else torch.arange(n, device=dev)
        if idx is not None:
            order = idx[order]
        for lo in range(0, n, self.batch_size):
            yield order[lo:lo + self.batch_size]

    def fetch(self, sel, out_images=None, out_labels=None):
        """Gather one batch; with ``out_*`` (pinned staging buffers of _harness.DeviceFeeder) straight into them."""
        full, _ = self._base()
        if out_images is None:
            return full.images[sel], full.labels[sel]
        n = sel.shape[0]
        if full.images.device.type == "cpu":
            # one memcpy per row, single-threaded (numpy): torch.index_select fans a 19 MB gather out over every core of the
            # host -- 69 ms per 128-image batch on the 256-thread GPU box against 1.4 ms this way (scripts/r4_feeder_timing.py)
            idx = sel.numpy()
            np.take(full.images.numpy().reshape(len(full), -1), idx, axis=0, out=out_images[:n].numpy().reshape(n, -1), mode="clip")
            np.take(full.labels.numpy(), idx, axis=0, out=out_labels[:n].numpy(), mode="clip")
        else:
            torch.index_select(full.images, 0, sel, out=out_images[:n])
            torch.index_select(full.labels, 0, sel, out=out_labels[:n])
        return out_images[:n], out_labels[:n]

    def sample_spec(self):
        full, _ = self._base()
        return (tuple(full.images.shape[1:]), full.images.dtype), (tuple(full.labels.shape[1:]), full.labels.dtype), full.images.device

    def __iter__(self):
        for sel in self.iter_indices():
            yield self.fetch(sel)


def class_balanced_split(labels: np.ndarray, val_split: float = 0.2):
    if labels.ndim == 2 and labels.shape[1] > 1:
        return _multilabel_split(labels, val_split)
    val = []
    for c in dict.fromkeys(labels.tolist()):                 # classes in order of first appearance, like Counter
        idx = np.where(labels == c)[0]
        val.append(idx[:math.ceil(len(idx) * val_split)])
    val_idx = set(np.concatenate(val).tolist()) if val else set()
    train_idx = [i for i in range(len(labels)) if i not in val_idx]
    return train_idx, sorted(val_idx)


def _multilabel_split(labels: np.ndarray, val_split: float):
    """feature.py:150-163: count = ceil(column sums * val_split); while some class still has count > 0, the lowest such class
    sends its lowest-index sample not yet taken to validation, and that sample's label row is subtracted from count."""
    y = np.asarray(labels) > 0
    count = np.ceil(y.sum(axis=0) * val_split)
    taken = np.zeros(len(y), dtype=bool)
    val = []
    while True:
        need = np.flatnonzero(count > 0)
        if need.size == 0:
            break
        i = int(np.flatnonzero(y[:, need[0]] & ~taken)[0])
        taken[i] = True
        val.append(i)
        count -= y[i]
    return np.flatnonzero(~taken).tolist(), sorted(val)


def few_shot_subset(labels: np.ndarray, shots: int, seed: int):
    """``shots`` samples per class, drawn with a seeded generator (the hub's sample_few_shot_subset uses its own
    RNG stream, so the *selection* differs from the reference's for the same seed; the sizes do not).

    (N, C) multi-hot labels: the samples are visited in one seeded permutation, and a sample is kept while one of its positive
    classes has fewer than ``shots`` kept samples; a sample with no positive class is never kept.  Every class with at least
    ``shots`` samples ends with ``shots`` or more.  This selection is this build's own, not the hub's."""
    rng = np.random.default_rng(seed)
    if labels.ndim == 2 and labels.shape[1] > 1:
        y = np.asarray(labels) > 0
        have = np.zeros(y.shape[1], dtype=np.int64)
        keep = []
        for i in rng.permutation(len(y)):
            if (have[y[i]] < shots).any():
                keep.append(i)
                have += y[i]
        return np.sort(np.asarray(keep, dtype=np.int64))
    keep = []
    for c in np.unique(labels):
        idx = np.where(labels == c)[0]
        keep.append(rng.permutation(idx)[:shots])
    return np.sort(np.concatenate(keep))


def _target_size(config):
    return int(config.TRAIN.get("IMAGE_SIZE", [224, 224])[0])


def _tensors(images, labels, config):
    """uint8 archives stay uint8: the Classifier hands INPUT.MEAN / INPUT.STD to the engine, which applies the reference's
    ToTensor + Normalize inside its patch gather (bit for bit the host arithmetic; a quarter of the memory and of the bytes to
    upload).  DATASET.NORMALIZE_ON_HOST = True restores the float path.
    uint8 archives at their NATIVE size (32 x 32, 96 x 96, 37 x 53, ...: one size per archive; ``_ragged_tensors`` takes the archives
    with one size per image) stay as they are too: the engine runs
    the reference's Resize(n_px, bicubic) + CenterCrop per batch (HipEngine.set_input_resize), bit for bit Pillow's result.
    DATASET.RESIZE_ON_HOST = True resizes at load time instead, with the same integer arithmetic on the host
    (pevit_amd/preprocess.py); NORMALIZE_ON_HOST on such an archive resizes first when TRAIN.IMAGE_SIZE states the target."""
    x = torch.as_tensor(np.asarray(images))
    if x.dtype == torch.uint8:
        n = _target_size(config)
        native = x.dim() == 4 and tuple(x.shape[2:]) != (n, n)
        # NORMALIZE_ON_HOST is older than the resize and has always normalised whatever size the archive holds: it resizes first only
        # where the configuration states the tower's size (TRAIN.IMAGE_SIZE), RESIZE_ON_HOST always (224 without the key)
        on_host = config.DATASET.get("RESIZE_ON_HOST", False) or \
            (config.DATASET.get("NORMALIZE_ON_HOST", False) and config.TRAIN.get("IMAGE_SIZE", None) is not None)
        if native and on_host:
            if config.DATASET.get("CENTER_CROP", True):
                from ..preprocess import resize_center_crop_u8
                x = resize_center_crop_u8(x.contiguous(), n)
            else:                                            # DATASET.CENTER_CROP False: Resize((n, n)), nothing cropped
                from ..preprocess import resize_u8
                x = resize_u8(x.contiguous(), n, center_crop=False)
        if config.DATASET.get("NORMALIZE_ON_HOST", False):
            mean = torch.tensor(config.INPUT.MEAN).view(1, 3, 1, 1)
            std = torch.tensor(config.INPUT.STD).view(1, 3, 1, 1)
            x = (x.float() / 255.0 - mean) / std
    else:
        x = x.float()
    return x.contiguous(), _labels(labels)


def _labels(labels):
    y = np.asarray(labels)
    if y.ndim == 2 and y.shape[1] > 1:                       # multi-hot (N, C): float32 targets of BCEWithLogitsLoss
        return torch.as_tensor(y.astype(np.float32)).contiguous()
    return torch.as_tensor(y).long()


RAGGED_TABLE_BYTES = 256 << 20       # default of DATASET.RAGGED_TABLE_BYTES: a cap on the table pools of one split, not a tuned value
_LOGGED = set()


def _ragged_stays(config, dev):
    """A ragged set stays ragged only where the engine resizes it: resident on the GPU, and neither RESIZE_ON_HOST nor
    NORMALIZE_ON_HOST asked for.  (Host-fed ragged upload through the staging ring does not exist.)"""
    return dev.type != "cpu" and not config.DATASET.get("RESIZE_ON_HOST", False) and not config.DATASET.get("NORMALIZE_ON_HOST", False)


def _ragged_tensors(pool, shapes, labels, config, stays):
    """A ragged archive split: ``pool`` 1-D uint8, image i a dense (3, h_i, w_i) block, the blocks one after the other (offsets: the
    running sum of 3 h w, int64); ``shapes`` (N, 2) integers (h, w).  Where it ``stays`` ragged it becomes a
    ``preprocess.RaggedImages`` -- the pool as it is, one descriptor per image, one table pair per distinct axis -- which the engine
    resizes batch by batch in one launch (csrc/resize_ragged.hip); images outside the kernel's range (a side above 4096, an axis of
    more than 33 taps) are resized on the host now and stored as n x n blocks.  Otherwise, and when the table pools would exceed
    DATASET.RAGGED_TABLE_BYTES, every image is resized on the host now (``preprocess.resize_u8``: the same bytes) into the dense
    (N, 3, n, n) tensor of the uniform route.  DATASET.CENTER_CROP False: Resize((n, n)) instead of Resize(n) + CenterCrop."""
    from .. import preprocess as pp
    n, crop = _target_size(config), bool(config.DATASET.get("CENTER_CROP", True))
    pool, shapes = np.ascontiguousarray(np.asarray(pool)), np.asarray(shapes).astype(np.int64).reshape(-1, 2)
    if pool.dtype != np.uint8 or pool.ndim != 1:
        raise RuntimeError(f"a ragged archive holds its images as one 1-D uint8 pool; got {pool.dtype} {pool.shape}")
    if stays:
        cap, need = int(config.DATASET.get("RAGGED_TABLE_BYTES", RAGGED_TABLE_BYTES)), pp.ragged_table_bytes(shapes, n, crop)
        if need > cap:
            logging.info(f"=> ragged set: its resize tables would take {need} bytes (DATASET.RAGGED_TABLE_BYTES {cap}): resized on the host")
            stays = False
    if not stays:
        return _tensors(pp.resize_ragged_u8(pool, shapes, n, crop), labels, config)
    images = pp.RaggedImages.build(pool, shapes, n, crop)
    if images.pre_resized and "pre_resized" not in _LOGGED:
        _LOGGED.add("pre_resized")
        logging.info(f"=> ragged set: {images.pre_resized} of {len(images)} images are outside the resize kernel's range (a side above "
                     f"4096 or a downscale beyond 8x) and were resized on the host at load time")
    return images, _labels(labels)


def _synthetic_ragged(config, stays):
    """DATASET.SYNTHETIC_RAGGED: seeded random pixels with a seeded size per image, both sides drawn inside
    DATASET.SYNTHETIC_SOURCE_RANGE (inclusive); takes the route of a ragged archive."""
    lo, hi = [int(v) for v in config.DATASET.get("SYNTHETIC_SOURCE_RANGE", (24, 72))]
    C = config.DATASET.NUM_CLASSES
    g = np.random.default_rng(int(config.DATASET.RANDOM_SEED_SAMPLING))
    out = []
    for n in config.DATASET.get("SYNTHETIC_SIZES", (256, 128)):
        shapes = g.integers(lo, hi + 1, (int(n), 2))
        pool = g.integers(0, 256, int((3 * shapes[:, 0] * shapes[:, 1]).sum()), dtype=np.uint8)
        out.append(_ragged_tensors(pool, shapes, np.arange(int(n)) % C, config, stays))
    return out


def _synthetic(config):
    sizes = config.DATASET.get("SYNTHETIC_SIZES", (256, 128))
    R = int(config.TRAIN.get("IMAGE_SIZE", [224, 224])[0])
    C = config.DATASET.NUM_CLASSES
    g = torch.Generator().manual_seed(int(config.DATASET.RANDOM_SEED_SAMPLING))
    out = []
    for n in sizes:
        if config.DATASET.get("SYNTHETIC_UINT8", False):      # raw pixels, as an image archive would hold them
            h, w = config.DATASET.get("SYNTHETIC_SOURCE_SIZE", None) or (R, R)      # ... at a native size: resized like an archive's
            x = torch.randint(0, 256, (n, 3, int(h), int(w)), generator=g, dtype=torch.uint8)
            if (int(h), int(w)) != (R, R) and config.DATASET.get("RESIZE_ON_HOST", False):
                if config.DATASET.get("CENTER_CROP", True):
                    from ..preprocess import resize_center_crop_u8
                    x = resize_center_crop_u8(x, R)
                else:
                    from ..preprocess import resize_u8
                    x = resize_u8(x, R, center_crop=False)
            out.append((x, torch.arange(n) % C))
        else:
            out.append((torch.randn((n, 3, R, R), generator=g), torch.arange(n) % C))
    return out


def construct_dataloader(config, feature_type="image", test_split_only=False):
    if feature_type != "image":
        raise RuntimeError("only image loaders are built here")
    name = config.DATASET.DATASET
    if name == "synthetic" and config.DATASET.get("SYNTHETIC_RAGGED", False):
        lo, hi = [int(v) for v in config.DATASET.get("SYNTHETIC_SOURCE_RANGE", (24, 72))]
        worst = 3 * hi * hi * sum(int(n) for n in config.DATASET.get("SYNTHETIC_SIZES", (256, 128)))
        (trx, try_), (tex, tey) = _synthetic_ragged(config, _ragged_stays(config, _resident_device(config, worst)))
    elif name == "synthetic":
        (trx, try_), (tex, tey) = _synthetic(config)
    else:
        path = config.DATASET.ROOT if str(config.DATASET.ROOT).endswith(".npz") else os.path.join(config.DATASET.ROOT, name + ".npz")
        if not os.path.isfile(path):
            raise RuntimeError(f"{path} not found: this build reads preprocessed tensor archives; the reference's "
                               "vision_datasets hub / ImageFolder pipeline (feature.py:533-583) is not part of it")
        z = np.load(path)
        if "train_shapes" in z.files and "test_shapes" in z.files:           # a ragged archive: one size per image
            train_pool, test_pool = z["train_images"], z["test_images"]
            stays = _ragged_stays(config, _resident_device(config, train_pool.size + test_pool.size))
            trx, try_ = _ragged_tensors(train_pool, z["train_shapes"], z["train_labels"], config, stays)
            tex, tey = _ragged_tensors(test_pool, z["test_shapes"], z["test_labels"], config, stays)
        else:
            trx, try_ = _tensors(z["train_images"], z["train_labels"], config)
            tex, tey = _tensors(z["test_images"], z["test_labels"], config)
    bs = int(config.DATASET.get("LOADER_BATCH_SIZE", 64))    # get_dataloader's batch_size_per_gpu default is 64 (feature.py:101,597)
    dev = _resident_device(config, trx.numel() * trx.element_size() + tex.numel() * tex.element_size())
    tex, tey = tex.to(dev), tey.to(dev)
    test_loader = TensorLoader(_Tensors(tex, tey), batch_size=bs, shuffle=False)
    if test_split_only:
        return test_loader
    labels = try_.numpy()
    shots = int(config.DATASET.NUM_SAMPLES_PER_CLASS)
    if shots > 0:
        keep = few_shot_subset(labels, shots, int(config.DATASET.RANDOM_SEED_SAMPLING))
        trx = trx.subset(keep) if hasattr(trx, "subset") else trx[keep]      # (a ragged set is indexed, its pool stays as it is)
        try_, labels = try_[keep], labels[keep]
    full = _Tensors(trx.to(dev), try_.to(dev))
    train_idx, val_idx = class_balanced_split(labels, 0.2)
    train_loader = TensorLoader(_View(full, train_idx), batch_size=bs, shuffle=True)
    val_loader = TensorLoader(_View(full, val_idx), batch_size=bs, shuffle=False)
    return train_loader, val_loader, test_loader


def _resident_device(config, nbytes, limit=64 << 30):
    """Keep the tensor set on the training GPU when it fits comfortably (288 GB of HBM per MI355X); DATASET.RESIDENT = False
    keeps it on the host (then _harness.DeviceFeeder uploads batch i+1 while batch i is trained on)."""
    if not config.DATASET.get("RESIDENT", True):
        return torch.device("cpu")
    if torch.cuda.is_available() and nbytes < limit and len(config.GPUS) == 1:
        return torch.device("cuda", int(config.GPUS[0]))
    return torch.device("cpu")
