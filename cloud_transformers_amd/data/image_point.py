"""The What3D single-view reconstruction protocol's data path (datasets/image_point.py, train_image_reconstruction.py:68-89,
163-169): the loader on the host without open3d or torchvision, the split on the device, a batch as one launch.

- `read_ply`: the vertex coordinates of an ASCII or binary little-endian PLY file -> float32 [P, 3].
- `ImageToPoint(d_path, split, im_size, points)`: the reference's host dataset, `(image f32[3, OH, OW], pcd f32[3, points])`
  (plus the category name on the test split).  One deviation: categories, objects and renderings are visited in sorted order
  (the reference's `iterdir()` order is the file system's), so an index names the same pair on every machine.
- `resize_tables`, `resize_size`: the coefficient tables of Pillow's 8-bit BILINEAR resample and torchvision's `Resize(int)`
  size rule.
- `DeviceImageToPoint(dataset, device, cache_dir)`: the decoded renderings u8[M, H, W, 3] at source resolution, the clouds
  concatenated, class ids and the tables, uploaded once.
- `image_items_from_draws`: the raw `ct_image_items` launch (include/cloudct.h) on explicit draws; a pure function.
- `image_items`: the draws of one batch from one generator on the device, then the launch; no host synchronisation.
- `ImageBatches`: one iteration = one epoch of `(img [B, 3, OH, OW], pcd [B, 3, points])` on the device, in the order of
  torch's own `DistributedSampler`.
"""
import hashlib
import json
import math
import os
from pathlib import Path

import numpy as np
import torch
from torch.utils.data.distributed import DistributedSampler

IMAGENET_MEAN = [0.485, 0.456, 0.406]
IMAGENET_STD = [0.229, 0.224, 0.225]
PRECISION_BITS = 32 - 8 - 2            # of Pillow's 8-bit resample: coefficients are int(0.5 + w * 2^22)


# ---------------------------------------------------------------------------------------------------------------------
# PLY files
_PLY_TYPES = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "i2", "int16": "i2", "ushort": "u2", "uint16": "u2",
              "int": "i4", "int32": "i4", "uint": "u4", "uint32": "u4", "float": "f4", "float32": "f4", "double": "f8",
              "float64": "f8"}


def read_ply(path):
    """The x, y, z properties of the `vertex` element of a PLY file (`format ascii 1.0` or `format binary_little_endian 1.0`)
    as float32 [P, 3].  The coordinates are `float` or `double`, anywhere among the properties; other scalar properties of
    `vertex` are skipped by their size; elements after `vertex` are ignored.  Anything else — a big-endian file, a list
    property inside `vertex`, an element in front of `vertex`, a missing coordinate, a short file — raises ValueError naming
    the file and the offending line."""
    with open(str(path), "rb") as f:
        raw = f.read()

    def bad(what, line=None):
        return ValueError("%s: %s%s" % (path, what, "" if line is None else " (line %r)" % line))

    pos, lines = 0, []
    while True:
        end = raw.find(b"\n", pos)
        if end < 0:
            raise bad("no end_header line: not a PLY file, or a short one", raw[pos:pos + 40].decode("ascii", "replace"))
        line = raw[pos:end].decode("ascii", "replace").strip()
        pos = end + 1
        if not lines and line != "ply":
            raise bad("the first line is not 'ply'", line)
        lines.append(line)
        if line == "end_header":
            break
    fmt, element, n_vertex, props = None, None, None, []
    for line in lines[1:-1]:
        tok = line.split()
        if not tok or tok[0] in ("comment", "obj_info"):
            continue
        if tok[0] == "format":
            if tok[1:] not in (["ascii", "1.0"], ["binary_little_endian", "1.0"]):
                raise bad("only 'format ascii 1.0' and 'format binary_little_endian 1.0' are read", line)
            fmt = tok[1]
        elif tok[0] == "element":
            if len(tok) != 3 or not tok[2].isdigit():
                raise bad("bad element line", line)
            if n_vertex is None and tok[1] != "vertex":
                raise bad("an element in front of 'vertex'", line)
            element = tok[1]
            if element == "vertex":
                n_vertex = int(tok[2])
        elif tok[0] == "property":
            if element == "vertex":
                if len(tok) != 3 or tok[1] not in _PLY_TYPES:
                    raise bad("a vertex property must be a scalar of a known type", line)
                props.append((tok[2], _PLY_TYPES[tok[1]], line))
            elif element is None:
                raise bad("a property outside an element", line)
        else:
            raise bad("unknown header line", line)
    if fmt is None:
        raise bad("no format line", lines[1] if len(lines) > 1 else "")
    if n_vertex is None:
        raise bad("no 'element vertex'", "end_header")
    names = [p[0] for p in props]
    for name in "xyz":
        if name not in names:
            raise bad("vertex has no property %r" % name, "element vertex %d" % n_vertex)
        kind, line = props[names.index(name)][1:]
        if kind not in ("f4", "f8"):
            raise bad("coordinate %r must be float or double" % name, line)
    cols = [names.index(name) for name in "xyz"]
    if fmt == "ascii":
        rows = raw[pos:].split(b"\n")
        if len(rows) < n_vertex:
            raise bad("%d vertices declared, %d lines of data" % (n_vertex, len(rows)), "element vertex %d" % n_vertex)
        out = np.empty((n_vertex, 3), np.float64)
        for i in range(n_vertex):
            vals = rows[i].split()
            if len(vals) < len(props):
                raise bad("a vertex line with %d of %d values" % (len(vals), len(props)), rows[i].decode("ascii", "replace"))
            try:
                out[i] = [float(vals[c]) for c in cols]
            except ValueError:
                raise bad("a vertex line that is not numbers", rows[i].decode("ascii", "replace"))
        return out.astype(np.float32)
    dt = np.dtype([("p%d" % k, "<" + kind) for k, (_, kind, _) in enumerate(props)])
    if len(raw) - pos < n_vertex * dt.itemsize:
        raise bad("%d vertices of %d bytes declared, %d bytes of data" % (n_vertex, dt.itemsize, len(raw) - pos),
                  "element vertex %d" % n_vertex)
    rec = np.frombuffer(raw, dtype=dt, count=n_vertex, offset=pos)
    return np.stack([rec["p%d" % c] for c in cols], axis=1).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------------
# the image transforms
def pil_loader(path):
    """The PNG as an RGB PIL image (datasets/image_point.py:17-21)."""
    try:
        from PIL import Image
    except ImportError as ex:
        raise ImportError("the What3D loader decodes the renderings with PIL (Pillow), which is not installed") from ex
    with open(str(path), "rb") as f:
        return Image.open(f).convert("RGB")


def resize_size(h, w, im_size):
    """(OH, OW) of torchvision's `Resize(im_size)` for an integer size: the smaller edge becomes im_size, the other
    int(im_size * long / short)."""
    if w <= h:
        return int(im_size * h / w), int(im_size)
    return int(im_size), int(im_size * w / h)


def resize_tables(n_in, n_out):
    """One axis of Pillow's 8-bit BILINEAR resample, n_in -> n_out, in float64 as its precompute_coeffs / normalize_coeffs_8bpc:
    (k int32[n_out, ksize], bounds int32[n_out, 2] = (min, taps)); output i is clamp((2^21 + sum_x pixel[min + x] * k[i, x]) >> 22)."""
    scale = float(n_in) / float(n_out)
    fs = max(scale, 1.0)
    support = fs
    ksize = 2 * int(math.ceil(support)) + 1
    idx = np.arange(n_out, dtype=np.float64)
    center = (idx + 0.5) * scale
    lo = np.maximum((center - support + 0.5).astype(np.int64), 0)          # (the cast truncates towards zero, as int() does)
    hi = np.minimum((center + support + 0.5).astype(np.int64), n_in)
    taps = hi - lo
    x = np.arange(ksize, dtype=np.float64)[None, :]
    w = np.maximum(0.0, 1.0 - np.abs((x + lo[:, None] - center[:, None] + 0.5) / fs))
    w = np.where(x < taps[:, None], w, 0.0)
    total = np.zeros(n_out, np.float64)
    for j in range(ksize):                                                   # Pillow's order of the sum
        total = total + w[:, j]
    w = np.where(total[:, None] != 0.0, w / np.where(total == 0.0, 1.0, total)[:, None], w)
    k = (0.5 + w * float(1 << PRECISION_BITS)).astype(np.int64).astype(np.int32)
    return k, np.stack([lo, taps], axis=1).astype(np.int32)


def to_tensor_normalize(image):
    """ToTensor and Normalize(IMAGENET_MEAN, IMAGENET_STD) of an RGB PIL image, in torch: f32[3, H, W]."""
    a = torch.from_numpy(np.array(image, dtype=np.uint8, copy=True)).permute(2, 0, 1).contiguous()
    t = a.to(torch.float32).div(255)
    mean = torch.tensor(IMAGENET_MEAN, dtype=torch.float32).view(3, 1, 1)
    std = torch.tensor(IMAGENET_STD, dtype=torch.float32).view(3, 1, 1)
    return t.sub_(mean).div_(std)


def resample_pcd(pcd, n):
    """Drop or duplicate points so that pcd has exactly n points (datasets/image_point.py:54-59; np.random)."""
    idx = np.random.permutation(pcd.shape[0])
    if idx.shape[0] < n:
        idx = np.concatenate([idx, np.random.randint(pcd.shape[0], size=n - pcd.shape[0])])
    return pcd[idx[:n]]


# ---------------------------------------------------------------------------------------------------------------------
# host dataset
class ImageToPoint(torch.utils.data.Dataset):
    """datasets/image_point.py:74-154.  `d_path` holds lists/<category>/<split>.txt (object ids), points/<category>/<object>/
    <stem>.ply, renderings/<category>/<object>/<stem>.png and classes.txt (`<name> <id>` per line).  Items are
    `(image f32[3, OH, OW], pcd f32[3, points])`, on the test split with the category's directory name as a third value.
    Categories, objects (in the list's order) and renderings are visited in sorted order."""

    def __init__(self, d_path, split="train", im_size=128, points=4096):
        super().__init__()
        self.d_path = Path(d_path)
        assert self.d_path.exists()
        assert self.d_path.is_dir()
        self.split = split
        list_dir, points_dir, im_dir = (self.d_path.joinpath(n) for n in ("lists", "points", "renderings"))
        assert list_dir.exists()
        assert points_dir.exists()
        assert im_dir.exists()
        self.class_to_id, self.id_to_class = {}, {}
        with open(str(self.d_path.joinpath("classes.txt")), "r") as cls_file:
            for line in cls_file.readlines():
                if line.split():
                    self.class_to_id[line.split()[0]] = line.split()[1]
                    self.id_to_class[line.split()[1]] = line.split()[0]
        self.im_size, self.points = im_size, points
        self.data_pairs = []
        for category in sorted(list_dir.iterdir()):
            if category.is_dir():
                split_list = category.joinpath(split + ".txt")
                assert split_list.exists()
                with open(str(split_list), "r") as split_file:
                    for object_id in split_file.readlines():
                        object_id = object_id.strip()
                        points_obj = points_dir.joinpath(category.name).joinpath(object_id)
                        im_obj = im_dir.joinpath(category.name).joinpath(object_id)
                        assert points_obj.exists()
                        assert im_obj.exists()
                        for img in sorted(im_obj.iterdir()):
                            if img.suffix == ".png":
                                point = points_obj.joinpath(img.stem + ".ply")
                                assert point.exists()
                                self.data_pairs.append((img, point))

    def category(self, index):
        """The category directory's name of pair `index` (the test split's third value)."""
        return self.data_pairs[index][1].parents[1].name

    def transform(self, image):
        """Resize(im_size), ToTensor, Normalize of an RGB PIL image."""
        from PIL import Image
        oh, ow = resize_size(image.height, image.width, self.im_size)
        return to_tensor_normalize(image.resize((ow, oh), Image.BILINEAR))

    def __getitem__(self, index):
        image_path, pcd_path = self.data_pairs[index]
        pcd = resample_pcd(read_ply(pcd_path), self.points)
        image = pil_loader(str(image_path))
        assert pcd.shape[1] == 3
        if self.split == "test":
            return self.transform(image), torch.from_numpy(pcd.astype(np.float32).T), self.category(index)
        return self.transform(image), torch.from_numpy(pcd.astype(np.float32).T)

    def __len__(self):
        return len(self.data_pairs)


# ---------------------------------------------------------------------------------------------------------------------
# the split on the device
def _cache_key(dataset):
    """sha1 over the pairs' relative paths, sizes and mtimes (ns): a touched, resized, added or removed file changes it."""
    rows = []
    for pair in dataset.data_pairs:
        for p in pair:
            st = os.stat(str(p))
            rows.append([os.path.relpath(str(p), str(dataset.d_path)), st.st_size, st.st_mtime_ns])
    return hashlib.sha1(json.dumps([dataset.split, rows]).encode()).hexdigest()


def decode_pairs(dataset, cache_dir=None):
    """{"images" u8[M, H, W, 3], "points" f32[T, 3], "offsets" i64[M + 1], "key"} of an ImageToPoint: every rendering decoded,
    every cloud read, once.  With `cache_dir` the arrays are kept in <cache_dir>/image_point_<split>.npz and read back from
    there while `_cache_key` matches (as s3dis_kpconv.load_areas keeps its Areas)."""
    key = _cache_key(dataset)
    cache = os.path.join(str(cache_dir), "image_point_%s.npz" % dataset.split) if cache_dir else None
    if cache and os.path.exists(cache):
        with np.load(cache, allow_pickle=False) as z:
            if str(z["key"]) == key:
                return {"images": z["images"], "points": z["points"], "offsets": z["offsets"], "key": key, "cached": True}
    images, clouds = [], []
    for image_path, pcd_path in dataset.data_pairs:
        a = np.array(pil_loader(image_path), dtype=np.uint8)
        if images and a.shape != images[0].shape:
            raise ValueError("%s is %d x %d, %s is %d x %d: the device set keeps one H x W" % (
                image_path, a.shape[0], a.shape[1], dataset.data_pairs[0][0], images[0].shape[0], images[0].shape[1]))
        images.append(a)
        cloud = read_ply(pcd_path)
        if cloud.shape[0] < 1:
            raise ValueError("%s holds no points" % pcd_path)
        clouds.append(cloud)
    if not images:
        raise ValueError("%s: no (rendering, cloud) pairs in split %r" % (dataset.d_path, dataset.split))
    out = {"images": np.stack(images), "points": np.concatenate(clouds).astype(np.float32),
           "offsets": np.concatenate([[0], np.cumsum([c.shape[0] for c in clouds])]).astype(np.int64), "key": key, "cached": False}
    if cache:
        os.makedirs(str(cache_dir), exist_ok=True)
        tmp = cache + ".%d.tmp.npz" % os.getpid()
        np.savez(tmp, images=out["images"], points=out["points"], offsets=out["offsets"], key=np.array(key))
        os.replace(tmp, cache)
    return out


class DeviceImageToPoint(object):
    """An `ImageToPoint` on `device`, uploaded once: `images` u8[M, H, W, 3] at source resolution (all of one H x W, else
    ValueError), `points` f32[T, 3] (all clouds concatenated), `offsets` i64[M + 1] (`offsets_host`: the numpy copy; `p_cap`
    the longest cloud), `class_id` i64[M] (an index into `class_names`, the sorted category directory names) and the
    coefficient tables `kx, bx, ky, by` of `resize_tables` for (H, W) -> (OH, OW) = `resize_size(H, W, im_size)`.
    `cache_dir`: see `decode_pairs`."""

    def __init__(self, dataset, device, cache_dir=None):
        dec = decode_pairs(dataset, cache_dir)
        self.dataset, self.from_cache = dataset, bool(dec["cached"])
        cats = [dataset.category(i) for i in range(len(dataset))]
        names = sorted(set(cats))
        self._upload(dec["images"], dec["points"], dec["offsets"], [names.index(c) for c in cats], names, device,
                     resize_size(dec["images"].shape[1], dec["images"].shape[2], int(dataset.im_size)), int(dataset.points))

    @classmethod
    def from_arrays(cls, images, points, offsets, class_id, class_names, device, out_size, num_points):
        """The device set of arrays already in memory: images u8[M, H, W, 3], points f32[T, 3], offsets [M + 1], class_id [M];
        `out_size` = (OH, OW), any size (a dataset's is `resize_size(H, W, im_size)`); `num_points`: the default n of a batch."""
        self = cls.__new__(cls)
        self.dataset, self.from_cache = None, False
        self._upload(images, points, offsets, class_id, class_names, device, out_size, num_points)
        return self

    def _upload(self, images, points, offsets, class_id, class_names, device, out_size, num_points):
        self.device = torch.device(device)
        images = np.ascontiguousarray(images, dtype=np.uint8)
        if images.ndim != 4 or images.shape[3] != 3 or images.shape[0] < 1:
            raise ValueError("images are u8[M, H, W, 3], M >= 1; got %s" % (images.shape,))
        M, H, W, _ = images.shape
        self.H, self.W, self.num_points = H, W, int(num_points)
        self.OH, self.OW = int(out_size[0]), int(out_size[1])
        self.offsets_host = np.asarray(offsets, np.int64)
        lengths = np.diff(self.offsets_host)
        points = np.ascontiguousarray(points, dtype=np.float32)
        if self.offsets_host.shape != (M + 1,) or lengths.min() < 1 or self.offsets_host[0] != 0 or tuple(points.shape) != (int(self.offsets_host[-1]), 3):
            raise ValueError("offsets are [M + 1] from 0 over clouds of at least one point, points f32[offsets[-1], 3]")
        self.p_cap = int(lengths.max())
        self.class_names = list(class_names)
        self.class_id_host = np.asarray(class_id, np.int64)
        kx, bx = resize_tables(W, self.OW)
        ky, by = resize_tables(H, self.OH)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(self.device)      # noqa: E731
        self.images, self.points, self.offsets, self.class_id = up(images), up(points), up(self.offsets_host), up(self.class_id_host)
        self.kx, self.bx, self.ky, self.by = up(kx), up(bx), up(ky), up(by)

    def __len__(self):
        return self.images.shape[0]


def _c_floats(values):
    import ctypes
    return (ctypes.c_float * len(values))(*values)


_MEAN, _STD = _c_floats(IMAGENET_MEAN), _c_floats(IMAGENET_STD)      # (the fp32 roundings of the lists)


def image_items_from_draws(ds, item, perm, u_dup, n, out=None):
    """ct_image_items (include/cloudct.h) on explicit draws: item i64[B], perm i64[B, p_cap] (a permutation of p_cap per row),
    u_dup f32[B, n] in [0, 1) -> (img f32[B, 3, OH, OW], pcd f32[B, 3, n], class i64[B]).  `out`: the three tensors to write
    (contiguous, on the device).  A pure function of its arguments."""
    from .. import _lib
    from ..ops import _dev, _on, _stream
    _dev(ds.images, item, perm, u_dup)
    dev = ds.images.device
    n = int(n)
    B = item.shape[0]
    if item.dim() != 1 or item.dtype != torch.int64 or B < 1:
        raise TypeError("image_items: item is int64 [B], B >= 1")
    if perm.dtype != torch.int64 or tuple(perm.shape) != (B, ds.p_cap):
        raise ValueError("image_items: perm is int64 [B, p_cap] = [%d, %d]; got %s %s" % (B, ds.p_cap, perm.dtype, tuple(perm.shape)))
    if u_dup.dtype != torch.float32 or tuple(u_dup.shape) != (B, n):
        raise ValueError("image_items: u_dup is float32 [B, n] = [%d, %d]; got %s %s" % (B, n, u_dup.dtype, tuple(u_dup.shape)))
    if not (1 <= n <= _lib.IMAGE_N_MAX and ds.p_cap <= _lib.IMAGE_P_MAX):
        raise ValueError("image_items: n within 1 .. %d and clouds of at most %d points; got n %d, p_cap %d"
                         % (_lib.IMAGE_N_MAX, _lib.IMAGE_P_MAX, n, ds.p_cap))
    ksx, ksy = ds.kx.shape[1], ds.ky.shape[1]
    if (max(ksx, ksy) > _lib.IMAGE_TAPS_MAX or ds.W > _lib.IMAGE_W_MAX or max(ds.H, ds.OH, ds.OW) > _lib.IMAGE_SIZE_MAX
            or min(ds.H, ksy) * 3 * ds.OW > _lib.IMAGE_STAGE_BYTES):
        raise ValueError("image_items: %d x %d -> %d x %d is outside ct_image_items' limits (include/cloudct.h)" % (ds.H, ds.W, ds.OH, ds.OW))
    item, perm, u_dup = item.contiguous(), perm.contiguous(), u_dup.contiguous()
    if out is None:
        out = (torch.empty(B, 3, ds.OH, ds.OW, dtype=torch.float32, device=dev), torch.empty(B, 3, n, dtype=torch.float32, device=dev),
               torch.empty(B, dtype=torch.int64, device=dev))
    img, pcd, cls = out
    for t, shape, dtype in ((img, (B, 3, ds.OH, ds.OW), torch.float32), (pcd, (B, 3, n), torch.float32), (cls, (B,), torch.int64)):
        if tuple(t.shape) != shape or t.dtype != dtype or not t.is_contiguous() or t.device != dev:
            raise ValueError("image_items: out is contiguous (f32[B, 3, OH, OW], f32[B, 3, n], i64[B]) on %s" % dev)
    with _on(dev):
        _lib.check(_lib.load().ct_image_items(ds.images.data_ptr(), len(ds), ds.H, ds.W, ds.OH, ds.OW, ds.kx.data_ptr(), ds.bx.data_ptr(),
                                              ksx, ds.ky.data_ptr(), ds.by.data_ptr(), ksy, _MEAN, _STD, ds.points.data_ptr(),
                                              ds.offsets.data_ptr(), ds.class_id.data_ptr(), ds.p_cap, item.data_ptr(), perm.data_ptr(),
                                              u_dup.data_ptr(), B, n, img.data_ptr(), pcd.data_ptr(), cls.data_ptr(), _stream(dev)),
                   "ct_image_items")
    return img, pcd, cls


def image_draws(B, p_cap, n, device, generator=None):
    """The draws of one batch from `generator` on `device`, in this order: the permutation keys rand(B, p_cap) (their argsort
    is `perm`), then `u_dup` rand(B, n).  -> (perm i64[B, p_cap], u_dup f32[B, n])."""
    keys = torch.rand(B, p_cap, device=device, generator=generator)
    u_dup = torch.rand(B, n, device=device, generator=generator)
    return torch.argsort(keys, dim=1), u_dup


def image_items(ds, item, n=None, generator=None):
    """(img f32[B, 3, OH, OW], pcd f32[B, 3, n], class i64[B]) of the pairs `item` i64[B] (on the device): what the reference's
    `ImageToPoint(...)[i]` items give after the collate — the rendering resized as Pillow resizes it, ToTensor, Normalize; the
    cloud resampled to n points (a random subset without replacement, topped up with uniformly drawn repeats when it is
    shorter).  The draws are `image_draws`'.  No host synchronisation."""
    n = ds.num_points if n is None else int(n)
    with torch.no_grad():
        perm, u_dup = image_draws(item.shape[0], ds.p_cap, n, ds.images.device, generator)
        return image_items_from_draws(ds, item, perm, u_dup, n)


class ImageBatches(object):
    """One iteration is one epoch of device batches `(img f32[B, 3, OH, OW], pcd f32[B, 3, points])` of a DeviceImageToPoint.
    The epoch's order is `torch.utils.data.distributed.DistributedSampler(range(len(ds)), world, rank, shuffle=train,
    seed=seed)` after `set_epoch`, uploaded once per epoch; `drop_last` drops a ragged last batch as a DataLoader does.  The
    items' draws come from a device generator seeded by `seed` and the rank.  `last_items` is the index tensor of the batch
    just yielded (a view of the epoch's order on the device), `last_classes` its class ids i64[B] (`ds.class_names`)."""

    def __init__(self, ds, batch_size, train=False, seed=0, rank=0, world=1, drop_last=False, points=None):
        self.ds, self.batch_size, self.train, self.drop_last = ds, int(batch_size), bool(train), bool(drop_last)
        self.points = ds.num_points if points is None else int(points)
        self.sampler = DistributedSampler(range(len(ds)), num_replicas=int(world), rank=int(rank), shuffle=self.train, seed=int(seed))
        self.generator = None
        if ds.device.type == "cuda":
            self.generator = torch.Generator(device=ds.device).manual_seed(int(seed) * 1000003 + int(rank))
        self.last_items = self.last_classes = None

    def __len__(self):
        n = len(self.sampler)
        return n // self.batch_size if self.drop_last else (n + self.batch_size - 1) // self.batch_size

    def set_epoch(self, epoch):
        self.sampler.set_epoch(int(epoch))

    def epoch_order(self):
        """The pair indices of this rank's epoch, batch after batch (host list)."""
        order = list(self.sampler)
        return order[:len(self) * self.batch_size]

    def __iter__(self):
        order = torch.tensor(self.epoch_order(), dtype=torch.int64).to(self.ds.device, non_blocking=True)
        for k in range(len(self)):
            item = order[k * self.batch_size:(k + 1) * self.batch_size]
            img, pcd, cls = image_items(self.ds, item, self.points, self.generator)
            self.last_items, self.last_classes = item, cls
            yield img, pcd
