"""The ShapeNet completion protocol's data path (datasets/grnet_completion.py:344-512, utils/pcd_utils.py:24-51,
train_inpainter.py:175-185): the loader on the host, the per-batch preparation on the device.

- `read_pcd`: PCD v0.7 `DATA ascii` / `DATA binary` -> float32 [n, 3] (open3d is not a dependency).
- `ShapeNetDataLoader(...).get_dataset(DatasetSubset.X)`, `collate_fn`: the reference's file list, rendering choice and
  transforms; items are `(taxonomy_id, model_id, {'partial_cloud', 'gtcloud'})`.
- `completion_items`: what `partial_postproces` does to a batch (drop the zero padding rows, shuffle the rest and top them
  up with repeats, lay sphere noise and the real points out with their labels) as ONE `ct_completion_items` launch after
  the draws; nothing is read back to the host, `count` stays on the device.
- `partial_postproces`: the reference's name, signature and return layout on top of it.
- `CompletionBatches`: a DataLoader over such a dataset -> the device triples `harness.Trainer`'s `completion` loss takes.
- `decode_split`, `DeviceShapeNetCompletion`: every file of a subset read once (an `.npz` cache keyed by paths, sizes and
  mtimes), the clouds concatenated and uploaded once.
- `completion_gather_from_draws`: the raw `ct_completion_gather` launch (include/cloudct.h) on explicit draws: the rendering
  choice, both RandomSamplePoints, RandomMirrorPoints and the collate of B items; a pure function.
- `completion_gather`: the draws of one batch from one generator on the device, then the launch; no host synchronisation.
- `DeviceCompletionBatches`: one iteration = one epoch of the same triples as `CompletionBatches`, in the order of torch's
  own `DistributedSampler`, with no file read and no host-to-device copy of points per step.
"""
import hashlib
import json
import os
import random
from enum import Enum, unique

import numpy as np
import torch

from ..metrics import sphere_noise


# ---------------------------------------------------------------------------------------------------------------------
# device batch assembly
def completion_items_from_draws(partial, perm, u_dup, sphere, scale=2.0):
    """ct_completion_items (include/cloudct.h) on explicit draws: partial f32[B, n_in, 3] (zero rows are padding), perm
    i64[B, n_in] (a permutation per cloud), u_dup f32[B, n_in] in [0, 1), sphere f32[B, 3, gt] ->
    (part f32[B, n_in, 3], noise f32[B, 4, gt], count i32[B]).  A pure function of its arguments."""
    from .. import _lib
    from ..ops import _dev, _on, _stream
    _dev(partial, perm, u_dup, sphere)
    dev = partial.device
    B, n_in, three = partial.shape
    gt = sphere.shape[2]
    if three != 3 or tuple(perm.shape) != (B, n_in) or tuple(u_dup.shape) != (B, n_in) or tuple(sphere.shape) != (B, 3, gt):
        raise ValueError("completion_items: partial [B, n_in, 3], perm / u_dup [B, n_in], sphere [B, 3, gt]; got %s %s %s %s"
                         % (tuple(partial.shape), tuple(perm.shape), tuple(u_dup.shape), tuple(sphere.shape)))
    if partial.dtype != torch.float32 or perm.dtype != torch.int64 or u_dup.dtype != torch.float32 or sphere.dtype != torch.float32:
        raise TypeError("completion_items: partial, u_dup and sphere are float32, perm is int64")
    ins = [t.contiguous() for t in (partial, perm, u_dup, sphere)]
    part = torch.empty(B, n_in, 3, dtype=torch.float32, device=dev)
    noise = torch.empty(B, 4, gt, dtype=torch.float32, device=dev)
    count = torch.empty(B, dtype=torch.int32, device=dev)
    with _on(dev):
        _lib.check(_lib.load().ct_completion_items(*[t.data_ptr() for t in ins], float(scale), B, n_in, gt, part.data_ptr(),
                                                   noise.data_ptr(), count.data_ptr(), _stream(dev)), "ct_completion_items")
    return part, noise, count


def completion_draws(B, n_in, gt_size, device, generator=None):
    """The draws of one batch, from `generator` on `device`, in this order: the permutation keys rand(B, n_in) (their argsort
    is `perm`), `u_dup` rand(B, n_in), then `metrics.sphere_noise(B, gt_size)`'s rand(2, B, gt_size).  The keys are plain: the
    kernel skips the padding rows wherever the permutation puts them."""
    keys = torch.rand(B, n_in, device=device, generator=generator)
    u_dup = torch.rand(B, n_in, device=device, generator=generator)
    sphere = sphere_noise(B, gt_size, device, generator=generator)
    return torch.argsort(keys, dim=1), u_dup, sphere


def completion_items(partial, gt_size, scale=2.0, generator=None, draws=None):
    """(part f32[B, n_in, 3], noise f32[B, 4, gt_size], count i32[B]) of the loader's partial clouds f32[B, n_in, 3] on the
    device: with q = scale * partial, part = the non-zero rows of q in random order, topped up to n_in with uniformly drawn
    repeats (resample_pcd), noise = gt_size - count points on the unit sphere labelled 0, then the non-zero rows in their
    original order labelled 1, channels first.  `draws` = (perm, u_dup, sphere) replaces `completion_draws(...)`.  A cloud
    without a valid row (the reference raises there) gives zeros, pure noise and count 0.  No host synchronisation."""
    from ..ops import _dev
    _dev(partial)
    B, n_in, _ = partial.shape
    with torch.no_grad():
        perm, u_dup, sphere = draws if draws is not None else completion_draws(B, n_in, int(gt_size), partial.device, generator)
        return completion_items_from_draws(partial.float(), perm, u_dup, sphere, scale)


def partial_postproces(partial_pcd, gt_size, generator=None):
    """partial_postproces(partial_pcd, gt_size) of utils/pcd_utils.py:24-51: `partial_pcd` [B, n_in, 3] is what the caller has
    already scaled (train_inpainter.py:180 passes 2 * data['partial_cloud']), on the host or on the device ->
    (part [B, n_in, 3], labelled noise [B, gt_size, 4]) on the device (the second is a view of the kernel's [B, 4, gt_size]
    output, so the caller's `.permute(0, 2, 1).cuda()` is that contiguous tensor again).  Draws come from `generator`
    (default: the device's default generator)."""
    dev = partial_pcd.device if partial_pcd.is_cuda else torch.device("cuda", torch.cuda.current_device())
    part, noise, _ = completion_items(partial_pcd.to(dev, torch.float32), gt_size, scale=1.0, generator=generator)
    return part, noise.permute(0, 2, 1)


# ---------------------------------------------------------------------------------------------------------------------
# PCD files
_PCD_TYPES = {("F", 4): "<f4", ("F", 8): "<f8", ("U", 1): "u1", ("U", 2): "<u2", ("U", 4): "<u4", ("U", 8): "<u8",
              ("I", 1): "i1", ("I", 2): "<i2", ("I", 4): "<i4", ("I", 8): "<i8"}


def read_pcd(path):
    """The x, y, z fields of a PCD v0.7 file (`DATA ascii` or `DATA binary`) as float32 [n, 3]; other fields may be present,
    the coordinates may be F 4 or F 8.  `binary_compressed` is not supported (ValueError)."""
    with open(str(path), "rb") as f:
        raw = f.read()
    head, pos, encoding = {}, 0, None
    while encoding is None:
        end = raw.find(b"\n", pos)
        if end < 0:
            raise ValueError("%s: no DATA line: not a PCD file" % path)
        line = raw[pos:end].decode("ascii", "replace").strip()
        pos = end + 1
        if not line or line.startswith("#"):
            continue
        key, _, rest = line.partition(" ")
        if key.upper() == "DATA":
            encoding = rest.strip().lower()
        else:
            head[key.upper()] = rest.split()
    if encoding not in ("ascii", "binary"):
        raise ValueError("%s: PCD encoding %r is not supported (ascii and binary are)" % (path, encoding))
    try:
        fields = head["FIELDS"]
        sizes = [int(v) for v in head["SIZE"]]
        types = [v.upper() for v in head["TYPE"]]
        counts = [int(v) for v in head.get("COUNT", ["1"] * len(fields))]
        n = int(head["POINTS"][0]) if "POINTS" in head else int(head["WIDTH"][0]) * int(head["HEIGHT"][0])
    except (KeyError, ValueError, IndexError) as ex:
        raise ValueError("%s: bad PCD header (%s)" % (path, ex))
    if not (len(fields) == len(sizes) == len(types) == len(counts)):
        raise ValueError("%s: FIELDS, SIZE, TYPE and COUNT differ in length" % path)
    for name in "xyz":
        if name not in fields:
            raise ValueError("%s: no field %r" % (path, name))
        k = fields.index(name)
        if types[k] != "F" or sizes[k] not in (4, 8) or counts[k] != 1:
            raise ValueError("%s: field %r must be F 4 or F 8 with COUNT 1" % (path, name))
    if encoding == "binary":
        try:
            dt = np.dtype([("f%d" % k, _PCD_TYPES[(types[k], sizes[k])], (counts[k],)) for k in range(len(fields))])
        except KeyError as ex:
            raise ValueError("%s: unknown field type %s" % (path, ex))
        if len(raw) - pos < n * dt.itemsize:
            raise ValueError("%s: %d points of %d bytes declared, %d bytes of data" % (path, n, dt.itemsize, len(raw) - pos))
        rec = np.frombuffer(raw, dtype=dt, count=n, offset=pos)
        return np.stack([rec["f%d" % fields.index(name)][:, 0] for name in "xyz"], axis=1).astype(np.float32)
    starts = np.concatenate([[0], np.cumsum(counts)])
    table = np.array(raw[pos:].split(), dtype=np.float64)
    width = int(starts[-1])
    if table.size < n * width:
        raise ValueError("%s: %d points of %d values declared, %d values of data" % (path, n, width, table.size))
    table = table[:n * width].reshape(n, width)
    return table[:, [int(starts[fields.index(name)]) for name in "xyz"]].astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------------
# dataset
class RandomSamplePoints(object):
    """grnet_completion.py:246-258: a random permutation cut to n_points rows, zero rows appended when the cloud is shorter."""

    def __init__(self, parameters):
        self.n_points = parameters["n_points"]

    def __call__(self, ptcloud):
        choice = np.random.permutation(ptcloud.shape[0])
        ptcloud = ptcloud[choice[:self.n_points]]
        if ptcloud.shape[0] < self.n_points:
            ptcloud = np.concatenate([ptcloud, np.zeros((self.n_points - ptcloud.shape[0], 3))])
        return ptcloud


class RandomMirrorPoints(object):
    """grnet_completion.py:297-314: rnd_value <= 0.25 mirrors x and z, (0.25, 0.5] mirrors x, (0.5, 0.75] mirrors z, above
    that nothing; applied as the reference applies it, a product with the (diagonal) matrix."""

    def __init__(self, parameters=None):
        pass

    def __call__(self, ptcloud, rnd_value):
        sx = -1.0 if rnd_value <= 0.5 else 1.0
        sz = -1.0 if (rnd_value <= 0.25 or 0.5 < rnd_value <= 0.75) else 1.0
        ptcloud[:, :3] = np.dot(ptcloud[:, :3], np.diag([sx, 1.0, sz]).T)
        return ptcloud


class ToTensor(object):
    def __init__(self, parameters=None):
        pass

    def __call__(self, arr):
        return torch.from_numpy(np.array(arr, copy=True)).float()


class Compose(object):
    """grnet_completion.py:107-135: [(transform, objects)] applied in order; ONE np.random.uniform(0, 1) per transform, drawn
    whether the transform takes it or not, handed to every object of a RandomMirrorPoints."""

    def __init__(self, transforms):
        self.transformers = list(transforms)

    def __call__(self, data):
        for transform, objects in self.transformers:
            rnd_value = np.random.uniform(0, 1)
            for k in list(data):
                if k in objects:
                    data[k] = transform(data[k], rnd_value) if isinstance(transform, RandomMirrorPoints) else transform(data[k])
        return data


@unique
class DatasetSubset(Enum):
    TRAIN = 0
    TEST = 1
    VAL = 2


def collate_fn(batch):
    """grnet_completion.py:351-368: (taxonomy ids, model ids, {key: stacked tensors})."""
    taxonomy_ids, model_ids, data = [], [], {}
    for sample in batch:
        taxonomy_ids.append(sample[0])
        model_ids.append(sample[1])
        for k, v in sample[2].items():
            data.setdefault(k, []).append(v)
    return taxonomy_ids, model_ids, {k: torch.stack(v, 0) for k, v in data.items()}


class Dataset(torch.utils.data.dataset.Dataset):
    """grnet_completion.py:371-397.  options: required_items, shuffle, n_renderings."""

    def __init__(self, options, file_list, transforms=None):
        self.options, self.file_list, self.transforms = options, file_list, transforms

    def __len__(self):
        return len(self.file_list)

    def __getitem__(self, idx):
        sample = self.file_list[idx]
        rand_idx = random.randint(0, self.options["n_renderings"] - 1) if self.options["shuffle"] else 0
        data = {}
        for ri in self.options["required_items"]:
            file_path = sample["%s_path" % ri]
            if isinstance(file_path, list):
                file_path = file_path[rand_idx]
            data[ri] = read_pcd(file_path).astype(np.float32)
        if self.transforms is not None:
            data = self.transforms(data)
        return sample["taxonomy_id"], sample["model_id"], data


class ShapeNetDataLoader(object):
    """grnet_completion.py:400-512.  `partial_path % (subset, taxonomy_id, model_id, rendering)` and `complete_path % (subset,
    taxonomy_id, model_id)` name the files; the category JSON is a list of {taxonomy_id, taxonomy_name, train, val, test}.
    TRAIN lists `n_renders` renderings per model and draws one per item (`random.randint`; the reference's `get_dataset`
    leaves `n_renderings` out of the options and so always reads the last one listed), the other subsets list rendering 0."""

    def __init__(self, category_file_path, partial_path, complete_path, n_renders=1, n_input=2048, n_output=16384):
        self.partial_path, self.complete_path = partial_path, complete_path
        self.n_input, self.n_output, self.n_renders = n_input, n_output, n_renders
        self.category_file_path = category_file_path
        with open(str(category_file_path)) as f:
            self.dataset_categories = json.loads(f.read())

    def get_dataset(self, subset):
        n_renderings = self.n_renders if subset == DatasetSubset.TRAIN else 1
        file_list = self._get_file_list(self._get_subset(subset), n_renderings)
        return Dataset({"required_items": ["partial_cloud", "gtcloud"], "shuffle": subset == DatasetSubset.TRAIN,
                        "n_renderings": n_renderings}, file_list, self._get_transforms(subset))

    def _get_transforms(self, subset):
        both = ["partial_cloud", "gtcloud"]
        chain = [(RandomSamplePoints({"n_points": self.n_input}), ["partial_cloud"])]
        if subset != DatasetSubset.TEST:
            chain.append((RandomSamplePoints({"n_points": self.n_output}), ["gtcloud"]))
        if subset == DatasetSubset.TRAIN:
            chain.append((RandomMirrorPoints(), both))
        chain.append((ToTensor(), both))
        return Compose(chain)

    @staticmethod
    def _get_subset(subset):
        return {DatasetSubset.TRAIN: "train", DatasetSubset.VAL: "val"}.get(subset, "test")

    def _get_file_list(self, subset, n_renderings=1):
        file_list = []
        for dc in self.dataset_categories:
            for s in dc[subset]:
                file_list.append({
                    "taxonomy_id": dc["taxonomy_id"],
                    "model_id": s,
                    "partial_cloud_path": [self.partial_path % (subset, dc["taxonomy_id"], s, i) for i in range(n_renderings)],
                    "gtcloud_path": self.complete_path % (subset, dc["taxonomy_id"], s),
                })
        return file_list


def shapenet_loader(data_cfg):
    """ShapeNetDataLoader of the reference config's `data` section (configs/inpainting.yaml)."""
    return ShapeNetDataLoader(category_file_path=data_cfg["category_path"], partial_path=data_cfg["partial_path"],
                              complete_path=data_cfg["gt_path"], n_renders=int(data_cfg.get("n_renders", 1)),
                              n_input=int(data_cfg.get("input_size", 2048)), n_output=int(data_cfg.get("gt_size", 16384)))


class CompletionBatches(object):
    """A DataLoader over a completion dataset -> device triples (noise f32[B, 4, gt], part f32[B, n_in, 3], gt f32[B, gt, 3]),
    what `harness.Trainer._loss`'s completion branch takes: gt = 2 * data['gtcloud'] and `completion_items(partial, gt,
    scale=2)` (train_inpainter.py:178-183).  The items' draws come from a device generator seeded by `seed` and the rank.
    `last_ids` holds the (taxonomy ids, model ids) of the batch just yielded."""

    def __init__(self, dataset, batch_size, device, seed=0, rank=0, shuffle=False, drop_last=False, num_workers=0, sampler=None,
                 worker_init_fn=None):
        self.device = torch.device(device)
        self.sampler = sampler
        self.loader = torch.utils.data.DataLoader(dataset, batch_size=int(batch_size), shuffle=bool(shuffle) and sampler is None,
                                                  num_workers=int(num_workers), sampler=sampler, drop_last=bool(drop_last),
                                                  collate_fn=collate_fn, worker_init_fn=worker_init_fn)
        self.generator = torch.Generator(device=self.device).manual_seed(int(seed) * 1000003 + int(rank))
        self.last_ids = None

    def __len__(self):
        return len(self.loader)

    def set_epoch(self, epoch):
        if self.sampler is not None and hasattr(self.sampler, "set_epoch"):
            self.sampler.set_epoch(epoch)

    def __iter__(self):
        for taxonomy_ids, model_ids, data in self.loader:
            gt = 2 * data["gtcloud"].to(self.device, non_blocking=True)
            part, noise, _ = completion_items(data["partial_cloud"].to(self.device, non_blocking=True), gt.shape[1], scale=2.0,
                                              generator=self.generator)
            self.last_ids = (taxonomy_ids, model_ids)
            yield noise, part, gt


# ---------------------------------------------------------------------------------------------------------------------
# the split on the device
def _split_paths(dataset):
    """Every file of a completion Dataset's file list in storage order: per model its renderings, then its gt cloud."""
    R = int(dataset.options["n_renderings"])
    paths = []
    for sample in dataset.file_list:
        partial = sample["partial_cloud_path"]
        partial = list(partial) if isinstance(partial, (list, tuple)) else [partial]
        if len(partial) != R:
            raise ValueError("model %s lists %d renderings, the dataset's n_renderings is %d" % (sample["model_id"], len(partial), R))
        paths.extend(str(p) for p in partial)
        paths.append(str(sample["gtcloud_path"]))
    return paths, R


def _split_cache_key(dataset):
    """(file tag, key): the key is a sha1 over the files' relative paths, sizes and mtimes (ns) and the ids, so a touched,
    resized, added or removed file changes it (as image_point._cache_key); the tag, a sha1 over the paths alone, names the
    cache file, so a rebuilt subset replaces its own stale file."""
    paths, R = _split_paths(dataset)
    root = os.path.commonpath([os.path.dirname(os.path.abspath(p)) for p in paths]) if paths else ""
    rel = [os.path.relpath(os.path.abspath(p), root) for p in paths]
    rows = []
    for p, r in zip(paths, rel):
        st = os.stat(p)
        rows.append([r, st.st_size, st.st_mtime_ns])
    ids = [[str(s["taxonomy_id"]), str(s["model_id"])] for s in dataset.file_list]
    tag = hashlib.sha1(json.dumps([R, rel]).encode()).hexdigest()[:16]
    return tag, hashlib.sha1(json.dumps([R, rows, ids]).encode()).hexdigest()


def decode_split(dataset, cache_dir=None):
    """{"partial_points" f32[Pt, 3], "partial_offsets" i64[M * R + 1] (cloud m * R + r is rendering r of model m), "gt_points"
    f32[Gt, 3], "gt_offsets" i64[M + 1], "taxonomy_ids", "model_ids" (lists), "R", "key", "cached"} of a completion `Dataset`:
    every file of its `file_list` read once with `read_pcd`.  With `cache_dir` the arrays are kept uncompressed in
    <cache_dir>/shapenet_completion_<tag>.npz and read back from there while `_split_cache_key` matches."""
    paths, R = _split_paths(dataset)
    M = len(dataset.file_list)
    if M < 1:
        raise ValueError("the completion dataset lists no models")
    tag, key = _split_cache_key(dataset)
    cache = os.path.join(str(cache_dir), "shapenet_completion_%s.npz" % tag) if cache_dir else None
    if cache and os.path.exists(cache):
        with np.load(cache, allow_pickle=False) as z:
            if str(z["key"]) == key:
                return {"partial_points": z["partial_points"], "partial_offsets": z["partial_offsets"], "gt_points": z["gt_points"],
                        "gt_offsets": z["gt_offsets"], "taxonomy_ids": z["taxonomy_ids"].tolist(), "model_ids": z["model_ids"].tolist(),
                        "R": R, "key": key, "cached": True}
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as pool:
        clouds = list(pool.map(read_pcd, paths))
    partial = [clouds[m * (R + 1) + r] for m in range(M) for r in range(R)]
    gt = [clouds[m * (R + 1) + R] for m in range(M)]
    offsets = lambda cs: np.concatenate([[0], np.cumsum([c.shape[0] for c in cs])]).astype(np.int64)      # noqa: E731
    out = {"partial_points": np.concatenate(partial).astype(np.float32).reshape(-1, 3), "partial_offsets": offsets(partial),
           "gt_points": np.concatenate(gt).astype(np.float32).reshape(-1, 3), "gt_offsets": offsets(gt),
           "taxonomy_ids": [s["taxonomy_id"] for s in dataset.file_list], "model_ids": [s["model_id"] for s in dataset.file_list],
           "R": R, "key": key, "cached": False}
    if cache:
        os.makedirs(str(cache_dir), exist_ok=True)
        tmp = cache + ".%d.tmp.npz" % os.getpid()
        np.savez(tmp, partial_points=out["partial_points"], partial_offsets=out["partial_offsets"], gt_points=out["gt_points"],
                 gt_offsets=out["gt_offsets"], taxonomy_ids=np.asarray(out["taxonomy_ids"]), model_ids=np.asarray(out["model_ids"]),
                 key=np.array(key))
        os.replace(tmp, cache)
    return out


def _sample_sizes(dataset):
    """(n_in, n_out or None) of the dataset's Compose chain: the RandomSamplePoints of 'partial_cloud' and of 'gtcloud'."""
    n_in = n_out = None
    for transform, objects in getattr(dataset.transforms, "transformers", []):
        if isinstance(transform, RandomSamplePoints):
            if "partial_cloud" in objects:
                n_in = int(transform.n_points)
            if "gtcloud" in objects:
                n_out = int(transform.n_points)
    if n_in is None:
        raise ValueError("the dataset's transforms hold no RandomSamplePoints of 'partial_cloud': the input size is unknown")
    return n_in, n_out


class DeviceShapeNetCompletion(object):
    """A completion `Dataset` on `device`, uploaded once, in fp32 as read: `partial_points` f32[Pt, 3] and `partial_offsets`
    i64[M * R + 1] (cloud m * R + r is rendering r of model m), `gt_points` f32[Gt, 3] and `gt_offsets` i64[M + 1]
    (`*_offsets_host`: the numpy copies); `M` models of `R` renderings, `p_cap` / `g_cap` the longest partial / gt cloud, `n_in`
    / `n_out` the rows of a batch's partial / gt clouds (the dataset's RandomSamplePoints), `sampled_gt` False where gt is not
    resampled (the TEST subset: every gt cloud must then hold `n_out` rows, else ValueError: the device path cannot report a
    ragged batch without a read-back); `taxonomy_ids`, `model_ids` host lists.  `cache_dir`: see `decode_split`."""

    def __init__(self, dataset, device, cache_dir=None):
        dec = decode_split(dataset, cache_dir)
        n_in, n_out = _sample_sizes(dataset)
        self.dataset, self.from_cache = dataset, bool(dec["cached"])
        self._upload(dec["partial_points"], dec["partial_offsets"], dec["gt_points"], dec["gt_offsets"], dec["R"], n_in, n_out, device,
                     n_out is not None, dec["taxonomy_ids"], dec["model_ids"])

    @classmethod
    def from_arrays(cls, partial_points, partial_offsets, gt_points, gt_offsets, R, n_in, n_out, device, sampled_gt=True,
                    taxonomy_ids=None, model_ids=None):
        """The device split of arrays already in memory.  `n_out` may be None when `sampled_gt` is False: the common length."""
        self = cls.__new__(cls)
        self.dataset, self.from_cache = None, False
        self._upload(partial_points, partial_offsets, gt_points, gt_offsets, R, n_in, n_out, device, sampled_gt, taxonomy_ids, model_ids)
        return self

    def _upload(self, partial_points, partial_offsets, gt_points, gt_offsets, R, n_in, n_out, device, sampled_gt, taxonomy_ids, model_ids):
        from .. import _lib
        self.device = torch.device(device)
        self.R, self.sampled_gt = int(R), bool(sampled_gt)
        self.partial_offsets_host = np.ascontiguousarray(partial_offsets, dtype=np.int64)
        self.gt_offsets_host = np.ascontiguousarray(gt_offsets, dtype=np.int64)
        partial_points = np.ascontiguousarray(partial_points, dtype=np.float32)
        gt_points = np.ascontiguousarray(gt_points, dtype=np.float32)
        self.M = M = self.gt_offsets_host.shape[0] - 1
        if self.R < 1 or M < 1 or self.gt_offsets_host.ndim != 1 or self.partial_offsets_host.shape != (M * self.R + 1,):
            raise ValueError("gt_offsets are [M + 1], partial_offsets [M * R + 1], M >= 1, R >= 1; got %s and %s with R %d"
                             % (self.gt_offsets_host.shape, self.partial_offsets_host.shape, self.R))
        p_len, g_len = np.diff(self.partial_offsets_host), np.diff(self.gt_offsets_host)
        for name, off, lens, pts in (("partial", self.partial_offsets_host, p_len, partial_points), ("gt", self.gt_offsets_host, g_len, gt_points)):
            if off[0] != 0 or lens.min() < 1 or tuple(pts.shape) != (int(off[-1]), 3):
                raise ValueError("%s_offsets start at 0 over clouds of at least one point, %s_points are f32[offsets[-1], 3]" % (name, name))
        self.p_cap, self.g_cap = int(p_len.max()), int(g_len.max())
        if not self.sampled_gt:
            n_out = int(g_len[0]) if n_out is None else int(n_out)
            if (g_len != n_out).any():
                k = int(np.flatnonzero(g_len != n_out)[0])
                raise ValueError("gt is not resampled and model %d holds %d points where %d are expected: a batch of the device "
                                 "path holds clouds of one length" % (k, int(g_len[k]), n_out))
        if n_out is None:
            raise ValueError("n_out is needed where gt is resampled (sampled_gt)")
        self.n_in, self.n_out = int(n_in), int(n_out)
        if (max(self.p_cap, self.g_cap) > _lib.GATHER_CAP_MAX or not 1 <= self.n_in <= _lib.COMPLETION_N_MAX
                or not 1 <= self.n_out <= _lib.GATHER_OUT_MAX):
            raise ValueError("clouds of at most %d points, n_in within 1 .. %d, n_out within 1 .. %d (ct_completion_gather, "
                             "include/cloudct.h); got p_cap %d, g_cap %d, n_in %d, n_out %d"
                             % (_lib.GATHER_CAP_MAX, _lib.COMPLETION_N_MAX, _lib.GATHER_OUT_MAX, self.p_cap, self.g_cap, self.n_in, self.n_out))
        self.taxonomy_ids = list(taxonomy_ids) if taxonomy_ids is not None else [None] * M
        self.model_ids = list(model_ids) if model_ids is not None else list(range(M))
        arrays = (partial_points, self.partial_offsets_host, gt_points, self.gt_offsets_host)
        self.nbytes = int(sum(a.nbytes for a in arrays))
        if self.device.type == "cuda":
            free, total = torch.cuda.mem_get_info(self.device)
            if self.nbytes > free:
                raise MemoryError("the resident completion split needs %d bytes (partial %d, gt %d, offsets %d) and %s has %d of %d "
                                  "bytes free" % (self.nbytes, partial_points.nbytes, gt_points.nbytes,
                                                  self.partial_offsets_host.nbytes + self.gt_offsets_host.nbytes, self.device, free, total))
        up = lambda a: torch.from_numpy(a).to(self.device)      # noqa: E731
        self.partial_points, self.partial_offsets, self.gt_points, self.gt_offsets = (up(a) for a in arrays)

    def __len__(self):
        return self.M


def completion_gather_from_draws(ds, item, rendering, perm_in, perm_gt, u_mirror, gt_scale=2.0):
    """ct_completion_gather (include/cloudct.h) on explicit draws: item i64[B] (models), rendering i64[B] in [0, R), perm_in
    i64[B, p_cap] (a permutation of p_cap per row), perm_gt i64[B, g_cap] or None (gt copied in order), u_mirror f32[B] or None
    (no mirror) -> (partial f32[B, n_in, 3] unscaled, gt f32[B, n_out, 3] times gt_scale).  A pure function of its arguments."""
    from .. import _lib
    from ..ops import _dev, _on, _stream
    given = [t for t in (item, rendering, perm_in, perm_gt, u_mirror) if t is not None]
    _dev(ds.partial_points, *given)
    dev = ds.partial_points.device
    if item.dim() != 1 or item.dtype != torch.int64 or item.shape[0] < 1:
        raise TypeError("completion_gather: item is int64 [B], B >= 1")
    B = item.shape[0]
    if rendering.dtype != torch.int64 or tuple(rendering.shape) != (B,):
        raise ValueError("completion_gather: rendering is int64 [B] = [%d]; got %s %s" % (B, rendering.dtype, tuple(rendering.shape)))
    if perm_in.dtype != torch.int64 or tuple(perm_in.shape) != (B, ds.p_cap):
        raise ValueError("completion_gather: perm_in is int64 [B, p_cap] = [%d, %d]; got %s %s" % (B, ds.p_cap, perm_in.dtype, tuple(perm_in.shape)))
    if perm_gt is not None and (perm_gt.dtype != torch.int64 or tuple(perm_gt.shape) != (B, ds.g_cap)):
        raise ValueError("completion_gather: perm_gt is int64 [B, g_cap] = [%d, %d] or None; got %s %s" % (B, ds.g_cap, perm_gt.dtype, tuple(perm_gt.shape)))
    if u_mirror is not None and (u_mirror.dtype != torch.float32 or tuple(u_mirror.shape) != (B,)):
        raise ValueError("completion_gather: u_mirror is float32 [B] = [%d] or None; got %s %s" % (B, u_mirror.dtype, tuple(u_mirror.shape)))
    item, rendering, perm_in = item.contiguous(), rendering.contiguous(), perm_in.contiguous()
    perm_gt = None if perm_gt is None else perm_gt.contiguous()
    u_mirror = None if u_mirror is None else u_mirror.contiguous()
    partial = torch.empty(B, ds.n_in, 3, dtype=torch.float32, device=dev)
    gt = torch.empty(B, ds.n_out, 3, dtype=torch.float32, device=dev)
    with _on(dev):
        _lib.check(_lib.load().ct_completion_gather(
            ds.partial_points.data_ptr(), ds.partial_offsets.data_ptr(), ds.gt_points.data_ptr(), ds.gt_offsets.data_ptr(), ds.M, ds.R,
            ds.p_cap, ds.g_cap, item.data_ptr(), rendering.data_ptr(), perm_in.data_ptr(), None if perm_gt is None else perm_gt.data_ptr(),
            None if u_mirror is None else u_mirror.data_ptr(), float(gt_scale), B, ds.n_in, ds.n_out, partial.data_ptr(), gt.data_ptr(),
            _stream(dev)), "ct_completion_gather")
    return partial, gt


def completion_gather_draws(ds, B, train, generator=None):
    """The draws of one batch of B items from `generator` on the split's device, in this order: `rendering` randint(0, R) [B]
    when training (else zeros: rendering 0), the permutation keys rand(B, p_cap) (their argsort is `perm_in`), the keys
    rand(B, g_cap) (`perm_gt`; only when `ds.sampled_gt`, else None), `u_mirror` rand(B) (only when training, else None).
    -> (rendering i64[B], perm_in i64[B, p_cap], perm_gt, u_mirror)."""
    dev = ds.partial_points.device
    if train:
        rendering = torch.randint(0, ds.R, (B,), device=dev, generator=generator)
    else:
        rendering = torch.zeros(B, dtype=torch.int64, device=dev)
    perm_in = torch.argsort(torch.rand(B, ds.p_cap, device=dev, generator=generator), dim=1)
    perm_gt = torch.argsort(torch.rand(B, ds.g_cap, device=dev, generator=generator), dim=1) if ds.sampled_gt else None
    u_mirror = torch.rand(B, device=dev, generator=generator) if train else None
    return rendering, perm_in, perm_gt, u_mirror


def completion_gather(ds, item, train, generator=None, gt_scale=2.0):
    """(partial f32[B, n_in, 3], gt f32[B, n_out, 3]) of the models `item` i64[B] (on the device): what the host `Dataset`'s
    items give after `collate_fn` — a rendering drawn per item when training, the partial cloud cut to a random n_in rows or
    padded with zero rows, gt resampled to n_out rows (where the subset resamples it), both mirrored by one draw when training —
    with gt times `gt_scale`.  The draws are `completion_gather_draws`'.  No host synchronisation."""
    with torch.no_grad():
        return completion_gather_from_draws(ds, item, *completion_gather_draws(ds, item.shape[0], train, generator), gt_scale=gt_scale)


class DeviceCompletionBatches(object):
    """One iteration is one epoch of the device triples `CompletionBatches` yields, (noise f32[B, 4, n_out], part f32[B, n_in, 3],
    gt f32[B, n_out, 3]), of a DeviceShapeNetCompletion: `completion_gather(..., gt_scale=2)` followed by `completion_items(partial,
    n_out, scale=2)`, both on draws of one device generator seeded by `seed` and the rank (first the gather's, then the items').
    The epoch's order is `torch.utils.data.distributed.DistributedSampler(range(len(ds)), world, rank, shuffle=train, seed=seed)`
    after `set_epoch`, uploaded once per epoch; `drop_last` drops a ragged last batch as a DataLoader does.  `last_ids` holds the
    (taxonomy ids, model ids) of the batch just yielded, from the host's copy of the order."""

    def __init__(self, ds, batch_size, train=False, seed=0, rank=0, world=1, drop_last=False):
        from torch.utils.data.distributed import DistributedSampler
        self.ds, self.batch_size, self.train, self.drop_last = ds, int(batch_size), bool(train), bool(drop_last)
        self.sampler = DistributedSampler(range(len(ds)), num_replicas=int(world), rank=int(rank), shuffle=self.train, seed=int(seed))
        self.generator = None
        if ds.device.type == "cuda":
            self.generator = torch.Generator(device=ds.device).manual_seed(int(seed) * 1000003 + int(rank))
        self.last_ids = None

    def __len__(self):
        n = len(self.sampler)
        return n // self.batch_size if self.drop_last else (n + self.batch_size - 1) // self.batch_size

    def set_epoch(self, epoch):
        self.sampler.set_epoch(int(epoch))

    def epoch_order(self):
        """The model indices of this rank's epoch, batch after batch (host list)."""
        order = list(self.sampler)
        return order[:len(self) * self.batch_size]

    def __iter__(self):
        host = self.epoch_order()
        order = torch.tensor(host, dtype=torch.int64).to(self.ds.device, non_blocking=True)
        for k in range(len(self)):
            sl = slice(k * self.batch_size, (k + 1) * self.batch_size)
            partial, gt = completion_gather(self.ds, order[sl], self.train, self.generator, gt_scale=2.0)
            part, noise, _ = completion_items(partial, self.ds.n_out, scale=2.0, generator=self.generator)
            self.last_ids = ([self.ds.taxonomy_ids[i] for i in host[sl]], [self.ds.model_ids[i] for i in host[sl]])
            yield noise, part, gt
