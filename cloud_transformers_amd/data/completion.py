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
"""
import json
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
