"""The S3DIS KPConv protocol (configs/s3dis_kpconv.yaml; datasets/s3dis_closer.py, datasets/s3dis_closer_train.py:70-170,
datasets/s3dis_closer_utils.py:252-333) with its neighbour work on the GPU (cloud_transformers_amd.neighbors.GridIndex).

- `load_areas`: the Stanford3dDataset_v1.2 text layout -> one cloud per Area, grid-subsampled on the host
  (data.subsampling.grid_subsampling) or, given a device, there (grid_subsampling_device: the same arrays), cached as
  .npz arrays (s3dis_closer.py:132-201).
- `SphereSampler`: the potential-field sphere picking and the item layout of S3DISSeg (s3dis_closer.py:239-276,302-361),
  batched, on the device (`plan` picks, `items` assembles them in one `ct_kp_items` launch, optionally augmented by
  `Augment`: the training transforms of s3dis_closer_utils.py:38-149).  Same semantics, not the reference's numpy random stream.
- `VoteEvaluator`: the validation voting and the sub-sampled / full-resolution IoUs (s3dis_closer_train.py:134-167,
  s3dis_closer_utils.py:252-333) with device scatters and device confusion matrices.

Unlike the rest of `data`, the sampler and the evaluator keep their tensors on a HIP device."""
import copy
import math
import os
from dataclasses import dataclass

import numpy as np
import torch

from .subsampling import grid_subsampling, grid_subsampling_device

LABEL_TO_NAMES = {0: "ceiling", 1: "floor", 2: "wall", 3: "beam", 4: "column", 5: "window", 6: "door", 7: "chair", 8: "table",
                  9: "bookcase", 10: "sofa", 11: "board", 12: "clutter"}
NAME_TO_LABEL = {v: k for k, v in LABEL_TO_NAMES.items()}
COLOR_MEAN = (0.5136457, 0.49523646, 0.44921124)        # s3dis_closer.py:118-119
COLOR_STD = (0.18308958, 0.18415008, 0.19252081)
TRAIN_AREAS = ["Area_1", "Area_2", "Area_3", "Area_4", "Area_6"]
VAL_AREAS = ["Area_5"]


@dataclass
class Area:
    """One Area as one cloud: the raw points (colours 0..255, labels) and the grid-subsampled cloud (colours / 255)."""
    name: str
    points: np.ndarray       # f32 [N, 3]
    colors: np.ndarray       # f32 [N, 3], 0..255
    labels: np.ndarray       # i32 [N]
    sub_points: np.ndarray   # f32 [M, 3]
    sub_colors: np.ndarray   # f32 [M, 3], 0..1
    sub_labels: np.ndarray   # i32 [M]


def _area_name(a):
    return "Area_%d" % a if isinstance(a, (int, np.integer)) else str(a)


def _object_label(object_name):
    tmp = object_name[:-4].split("_")[0]
    if tmp in NAME_TO_LABEL:
        return NAME_TO_LABEL[tmp]
    if tmp == "stairs":
        return NAME_TO_LABEL["clutter"]
    raise ValueError("Unknown object name: " + str(tmp))


def _read_area(folder):
    """s3dis_closer.py:142-176: every room's Annotations/*.txt (x y z r g b per line), rooms and objects in name order."""
    pts, cols, labs = [], [], []
    for room in sorted(os.listdir(folder)):
        ann = os.path.join(folder, room, "Annotations")
        if not os.path.isdir(ann):
            continue
        for obj in sorted(os.listdir(ann)):
            if obj[-4:] != ".txt":
                continue
            label = _object_label(obj)
            data = np.loadtxt(os.path.join(ann, obj), dtype=np.float64, ndmin=2)
            if data.size == 0:
                continue
            pts.append(data[:, 0:3].astype(np.float32))
            cols.append(data[:, 3:6].astype(np.uint8).astype(np.float32))
            labs.append(np.full(data.shape[0], label, dtype=np.int32))
    if not pts:
        raise ValueError("no annotated objects under %s" % folder)
    return np.concatenate(pts), np.concatenate(cols), np.concatenate(labs)


def _subsample_area(points, colors, labels, sampleDl, device):
    """The Area's grid subsampling: on `device` when one is given (the raw cloud is uploaded whole; one that does not
    fit raises), unless CLOUDCT_GRID_SUBSAMPLE=host; on the host otherwise.  The same arrays either way."""
    if device is None or os.environ.get("CLOUDCT_GRID_SUBSAMPLE", "device") == "host":
        return grid_subsampling(points, features=colors, labels=labels[:, None], sampleDl=sampleDl)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)      # noqa: E731
    return tuple(t.cpu().numpy() for t in grid_subsampling_device(up(points), up(colors), up(labels[:, None]), sampleDl=sampleDl))


def load_areas(data_root, areas, sampleDl=0.04, cache_dir=None, device=None):
    """Areas (names 'Area_k' or numbers k) of `data_root` — the Stanford3dDataset_v1.2 folder or its parent — as `Area`s.
    With `cache_dir`, each Area's arrays are kept in <cache_dir>/<Area>_<sampleDl:.3f>.npz and read back from there.
    With a HIP `device`, the subsampling runs there (`_subsample_area`); arrays and cache files do not depend on it."""
    root = data_root
    if os.path.isdir(os.path.join(data_root, "Stanford3dDataset_v1.2")):
        root = os.path.join(data_root, "Stanford3dDataset_v1.2")
    out = []
    for a in areas:
        name = _area_name(a)
        cache = os.path.join(cache_dir, "%s_%.3f.npz" % (name, sampleDl)) if cache_dir else None
        if cache and os.path.exists(cache):
            with np.load(cache, allow_pickle=False) as z:
                out.append(Area(name, *(z[k] for k in ("points", "colors", "labels", "sub_points", "sub_colors", "sub_labels"))))
            continue
        points, colors, labels = _read_area(os.path.join(root, name))
        if sampleDl > 0:
            sub_points, sub_colors, sub_labels = _subsample_area(points, colors, labels, sampleDl, device)
            sub_colors = sub_colors / np.float32(255.0)
            sub_labels = np.squeeze(sub_labels, axis=1)
        else:
            sub_points, sub_colors, sub_labels = points, colors / np.float32(255.0), labels
        area = Area(name, points, colors, labels, sub_points.astype(np.float32), sub_colors.astype(np.float32),
                    sub_labels.astype(np.int32))
        if cache:
            os.makedirs(cache_dir, exist_ok=True)
            tmp = cache + ".%d.tmp.npz" % os.getpid()
            np.savez(tmp, points=area.points, colors=area.colors, labels=area.labels, sub_points=area.sub_points,
                     sub_colors=area.sub_colors, sub_labels=area.sub_labels)
            os.replace(tmp, cache)
        out.append(area)
    return out


def scene_seg_features(input_features_dim, pc, color, height):
    """get_scene_seg_features (s3dis_closer.py:49-65) over a batch: pc [B,N,3], color [B,N,3], height [B,N,1] -> [B,F,N]."""
    if input_features_dim == 1:
        f = height
    elif input_features_dim == 3:
        f = color
    elif input_features_dim == 4:
        f = torch.cat([color, height], -1)
    elif input_features_dim == 5:
        f = torch.cat([torch.ones_like(height), color, height], -1)
    elif input_features_dim == 6:
        f = torch.cat([color, pc], -1)
    elif input_features_dim == 7:
        f = torch.cat([color, height, pc], -1)
    else:
        raise NotImplementedError("input_features_dim %r" % (input_features_dim,))
    return f.transpose(1, 2).contiguous()


class SphereSampler:
    """Spheres of `in_radius` picked by the potential field of S3DISSeg (s3dis_closer.py:239-276), items laid out as its
    __getitem__ (:302-361), B at a time.  State on `device`: the subsampled clouds, their GridIndex and the potentials
    (`potentials[c]`, f32, views of one concatenated buffer; `min_potentials` f32[clouds]) and the `GridIndexTable` of the
    clouds.  `last_picks` keeps (cloud, point, pick point f32[3]) of every pick of the last `plan` (or `sample`) call, in
    order, so that a test can replay the potential updates; after a device plan it is read back from the plan's tensors the
    first time someone asks, and not before.

    `plan` is one `ct_kp_plan` call (include/cloudct.h): no value comes back to the host while the picks are made, nor in
    `items`.  CLOUDCT_KP_PLAN=0 selects the torch loop it replaced (`_plan_torch`): the same bits and the same draws."""

    def __init__(self, areas, num_points, in_radius=2.0, input_features_dim=4, color_drop=0.2, device="cuda", generator=None,
                 cell=None):
        from .. import _lib
        from ..neighbors import GridIndex, GridIndexTable
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("SphereSampler needs a HIP device; there is no CPU fallback")
        if generator is None:
            generator = torch.Generator(device=self.device)
            generator.seed()
        self.gen = generator
        self.num_points, self.in_radius = int(num_points), float(in_radius)
        self.input_features_dim, self.color_drop = int(input_features_dim), float(color_drop)
        if self.input_features_dim not in (1, 3, 4, 5, 6, 7):
            raise NotImplementedError("input_features_dim %r" % (input_features_dim,))
        dev = self.device
        self.sub_points = [torch.from_numpy(np.ascontiguousarray(a.sub_points, np.float32)).to(dev) for a in areas]
        self.indices = [GridIndex(p, cell) for p in self.sub_points]
        sizes = [p.shape[0] for p in self.sub_points]
        self.offsets = torch.tensor([0] + list(np.cumsum(sizes)[:-1]), dtype=torch.int64, device=dev)
        self._all_points = torch.cat(self.sub_points)
        self._all_colors = torch.from_numpy(np.concatenate([np.asarray(a.sub_colors, np.float32) for a in areas])).to(dev)
        self._all_labels = torch.from_numpy(np.concatenate([np.asarray(a.sub_labels) for a in areas]).astype(np.int64)).to(dev)
        # s3dis_closer.py:241-245: uniform potentials in [0, 1e-3)
        self._all_potentials = torch.cat([torch.rand(n, generator=self.gen, device=dev) * 1e-3 for n in sizes])
        self.potentials = list(torch.split(self._all_potentials, sizes))
        self.min_potentials = torch.stack([p.min() for p in self.potentials])
        self.table = GridIndexTable(self.indices, [0] + [int(v) for v in np.cumsum(sizes)[:-1]])
        self._plan_ws = torch.empty(_lib.load().ct_kp_plan_workspace_bytes(len(sizes), max(sizes)), dtype=torch.uint8, device=dev)
        self._device_plan = None
        self._mean = torch.tensor(COLOR_MEAN, dtype=torch.float32, device=dev)
        self._std = torch.tensor(COLOR_STD, dtype=torch.float32, device=dev)
        self.last_picks = []
        self.last_augment = (None, None, None)

    @property
    def last_picks(self):
        if self._last_picks is None:
            cloud, point, picks = self._device_plan
            self._last_picks = [(c, point[i], picks[i]) for i, c in enumerate(cloud.tolist())]     # the one read
        return self._last_picks

    @last_picks.setter
    def last_picks(self, value):
        self._last_picks = value

    def _pick(self):
        """One item (s3dis_closer.py:247-276): pick, sorted radius query cut to num_points, Tukey update of the potentials."""
        ci = 0 if len(self.potentials) == 1 else int(torch.argmin(self.min_potentials))
        pot = self.potentials[ci]
        pi = torch.argmin(pot)
        r = self.in_radius
        noise = torch.randn(3, generator=self.gen, device=self.device) * (r / 10)
        pick = self.sub_points[ci][pi] + noise
        idx, d2, count = self.indices[ci].query_radius(pick[None], r, self.num_points)
        idx, d2 = idx[0], d2[0]
        valid = idx >= 0
        tukey = torch.where(valid, torch.square(1 - d2 / (r * r)), torch.zeros_like(d2))
        pot.index_add_(0, idx.clamp(min=0), tukey)
        self.min_potentials[ci] = pot.min()
        self.last_picks.append((ci, pi, pick))
        return ci, pick

    def plan(self, n):
        """n picks by the potential field (advancing the potentials): (cloud i64[n], pick points f32[n, 3]), on the device;
        `last_picks` gets them in order.  Draws n times randn(3), as `_pick` does, all before the one `ct_kp_plan` call."""
        from .. import _lib
        from ..ops import _on, _stream
        n = int(n)
        if n < 1 or os.environ.get("CLOUDCT_KP_PLAN", "1") == "0":
            return self._plan_torch(n)
        dev, r = self.device, self.in_radius
        noise = torch.stack([torch.randn(3, generator=self.gen, device=dev) for _ in range(n)]) * (r / 10)
        cloud = torch.empty(n, dtype=torch.int64, device=dev)
        point = torch.empty(n, dtype=torch.int64, device=dev)
        picks = torch.empty(n, 3, dtype=torch.float32, device=dev)
        with _on(dev):
            _lib.check(_lib.load().ct_kp_plan(self.table.table.data_ptr(), self.table.n_clouds, self.table.max_points,
                                              self._all_points.data_ptr(), self._all_potentials.data_ptr(),
                                              self.min_potentials.data_ptr(), noise.data_ptr(), r, self.num_points, n,
                                              cloud.data_ptr(), point.data_ptr(), picks.data_ptr(), self._plan_ws.data_ptr(),
                                              self._plan_ws.numel(), _stream(dev)), "ct_kp_plan")
        self._device_plan, self._last_picks = (cloud, point, picks), None
        return cloud, picks

    def _plan_torch(self, n):
        """`plan` as the loop of `_pick` it was before ct_kp_plan: one device-to-host read per pick with several clouds."""
        self.last_picks = []
        cloud, picks = [], []
        for _ in range(int(n)):
            ci, pick = self._pick()
            cloud.append(ci)
            picks.append(pick)
        return torch.tensor(cloud, dtype=torch.int64, device=self.device), torch.stack(picks)

    def items(self, cloud, picks, augment=None, generator=None):
        """The items of picks (cloud i64[B], pick points f32[B, 3]), the 6-tuple of `sample`: one table-driven radius query for
        the whole batch, then the batch assembly `ct_kp_items`.  Draws, from `generator` (default: the sampler's own): the slot keys
        rand(B, N), the padding rand(B, N), the colour drop rand(B); with `augment` (an `Augment`), then the angles, scales
        and mirrors rand(B, 3) each and the jitter randn(B, N, 3).  `last_augment` keeps the (R, s, j) of the last call."""
        gen = self.gen if generator is None else generator
        dev, N = self.device, self.num_points
        cloud = cloud.to(dev)
        picks = picks.to(dev, torch.float32).contiguous()
        B = picks.shape[0]
        idx, _, count = self.table.query_radius(cloud.long(), picks, self.in_radius, N)
        nvalid = torch.clamp(count, max=N)
        live = torch.arange(N, device=dev)[None, :] < nvalid[:, None]
        # a random permutation of the valid slots (:333-335); the argsort stays in torch, which decides the order of ties
        keys = torch.where(live, torch.rand(B, N, generator=gen, device=dev), torch.full((B, N), 2.0, device=dev))
        perm = torch.argsort(keys, dim=1)
        u_pad = torch.rand(B, N, generator=gen, device=dev)
        drop = (torch.rand(B, generator=gen, device=dev) > self.color_drop).float()
        R = s = j = None
        if augment is not None:
            R, s, j = augment.draw(B, N, gen, dev)
        self.last_augment = (R, s, j)
        points, mask, features, labels, input_inds = kp_items(idx, count, perm, u_pad, self.offsets[cloud], picks, drop,
                                                              self._all_points, self._all_colors, self._all_labels, COLOR_MEAN,
                                                              COLOR_STD, self.input_features_dim, R, s, j)
        return points, mask, features, labels, cloud, input_inds

    def sample(self, B, augment=None):
        """B items: points f32[B,N,3] (centred on the pick point), mask i32[B,N], features f32[B,F,N], labels i64[B,N],
        cloud_index i64[B], input_inds i64[B,N] (indices into the item's subsampled cloud): `items(*plan(B), augment)`."""
        return self.items(*self.plan(B), augment=augment)


def kp_items(idx, count, perm, u_pad, offset, picks, drop, points, colors, labels, mean, std, F, R=None, s=None, j=None):
    """ct_kp_items (include/cloudct.h): (points f32[B,N,3], mask i32[B,N], features f32[B,F,N], labels i64[B,N],
    input_inds i64[B,N]) of B items from their ball queries (idx i64[B,N], count i64[B]), slot order `perm`, padding draws
    `u_pad`, per-item cloud offset and pick point, colour drop, the concatenated sub-clouds, the colour mean / std (host
    sequences of 3) and the optional augmentation."""
    from .. import _lib
    from ..ops import _dev, _on, _stream
    _dev(idx)
    dev = idx.device
    B, N = idx.shape
    if (R is None) != (s is None) or (R is None) != (j is None):
        raise ValueError("kp_items: pass R, s and j together, or none of them")
    mean_c, std_c = _lib.float_array(mean), _lib.float_array(std)
    aug = [t.contiguous() if t is not None else None for t in (R, s, j)]
    ins = [t.contiguous() for t in (idx, count, perm, u_pad, offset, picks, drop, points, colors, labels)]
    out_p = torch.empty(B, N, 3, dtype=torch.float32, device=dev)
    mask = torch.empty(B, N, dtype=torch.int32, device=dev)
    feats = torch.empty(B, int(F), N, dtype=torch.float32, device=dev)
    out_l = torch.empty(B, N, dtype=torch.int64, device=dev)
    inds = torch.empty(B, N, dtype=torch.int64, device=dev)
    ptr = lambda t: None if t is None else t.data_ptr()        # noqa: E731
    with _on(dev):
        _lib.check(_lib.load().ct_kp_items(*[t.data_ptr() for t in ins], points.shape[0], mean_c, std_c, *[ptr(t) for t in aug],
                                           B, N, int(F), out_p.data_ptr(), mask.data_ptr(), feats.data_ptr(), out_l.data_ptr(),
                                           inds.data_ptr(), _stream(dev)), "ct_kp_items")
    return out_p, mask, feats, out_l, inds


def angle_axis(angle, axis):
    """angle_axis (s3dis_closer_utils.py:8-36) over a batch: angles f64[...] about the unit `axis` -> f32[..., 3, 3], built in
    float64 as cos*I + sin*[u]x + (1 - cos)*u u^T, in that order, then rounded to float32."""
    angle = angle.double()
    u = torch.tensor(axis, dtype=torch.float64, device=angle.device)
    u = u / torch.linalg.norm(u)
    cross = torch.tensor([[0.0, -u[2], u[1]], [u[2], 0.0, -u[0]], [-u[1], u[0], 0.0]], dtype=torch.float64, device=angle.device)
    c, s_ = torch.cos(angle)[..., None, None], torch.sin(angle)[..., None, None]
    eye = torch.eye(3, dtype=torch.float64, device=angle.device)
    return (c * eye + s_ * cross + (1.0 - c) * torch.outer(u, u)).float()


def rotation_factors(angles):
    """(Rx, Ry, Rz) f32[B, 3, 3] of angles [B, 3] (x, y, z): PointcloudRandomRotate's factors (s3dis_closer_utils.py:76-93)."""
    return tuple(angle_axis(angles[:, a], ax) for a, ax in enumerate(([1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0])))


@dataclass
class Augment:
    """PointcloudRandomRotate + PointcloudScaleAndJitter with the values of train_segmentation_kpconv.py:84-130: an angle per
    axis uniform in +-range, R = Rz Ry Rx (factors in float64 rounded to f32, composed in f32); a scale per axis uniform in
    [scale_low, scale_high), its sign flipped with probability 1/2 on the axes `symmetries` names; a jitter per point and
    axis, normal with `std`, clipped at +-clip."""
    x_range: float = 0.0
    y_range: float = 0.0
    z_range: float = 3.1415926
    scale_low: float = 0.7
    scale_high: float = 1.3
    std: float = 0.001
    clip: float = 0.05
    symmetries: tuple = (1, 0, 0)

    def draw(self, B, N, generator, device):
        """(R f32[B,3,3], s f32[B,3], j f32[B,N,3]): angles, scales, mirrors rand(B, 3) each, then jitter randn(B, N, 3)."""
        u_ang = torch.rand(B, 3, generator=generator, device=device)
        u_scale = torch.rand(B, 3, generator=generator, device=device)
        u_sym = torch.rand(B, 3, generator=generator, device=device)
        jit = torch.randn(B, N, 3, generator=generator, device=device)
        ranges = torch.tensor([self.x_range, self.y_range, self.z_range], dtype=torch.float64, device=device)
        angles = (u_ang.double() * 2.0 - 1.0) * ranges
        Rx, Ry, Rz = rotation_factors(angles)
        R = torch.matmul(torch.matmul(Rz, Ry), Rx)
        sym = torch.tensor([float(v) for v in self.symmetries], dtype=torch.float64, device=device)
        sign = (torch.round(u_sym.double()) * 2.0 - 1.0) * sym + (1.0 - sym)
        s = ((self.scale_low + (self.scale_high - self.scale_low) * u_scale.double()) * sign).float()
        j = torch.clamp(jit * self.std, -self.clip, self.clip)
        return R.contiguous(), s.contiguous(), j.contiguous()


def iou_from_confusions(confusions):
    """IoU_from_confusions (s3dis_closer_utils.py:252-279) on a torch tensor [..., C, C] (rows truth, columns prediction)."""
    c = confusions if confusions.is_floating_point() else confusions.double()
    tp = torch.diagonal(c, dim1=-2, dim2=-1)
    tp_fn = c.sum(-1)
    tp_fp = c.sum(-2)
    iou = tp / (tp_fp + tp_fn - tp + 1e-6)
    absent = tp_fn < 1e-3
    counts = (~absent).to(c.dtype).sum(-1, keepdim=True)
    miou = iou.sum(-1, keepdim=True) / (counts + 1e-6)
    return iou + absent.to(c.dtype) * miou


def _confusion(truth, pred, C):
    """sklearn confusion_matrix(truth, pred, labels=arange(C)) on the device: i64 [C, C]."""
    return torch.bincount(truth.long() * C + pred.long(), minlength=C * C)[:C * C].view(C, C)


class VoteEvaluator:
    """Validation voting (s3dis_closer_train.py:70-167) on the device.  Per subsampled cloud: the summed logits, the vote
    counts (from 1e-6) and the running smoothed logits; `add` applies the reference's per-item loop (:134-145) item by item
    (items of one batch may share points), `sub_ious` / `full_ious` are sub_s3dis_metrics / s3dis_metrics
    (s3dis_closer_utils.py:282-333), the full-resolution one through the nearest subsampled point of every raw point
    (GridIndex.nearest, computed once and kept on the device)."""

    def __init__(self, areas, num_classes=13, smooth=0.95, device="cuda"):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("VoteEvaluator needs a HIP device; there is no CPU fallback")
        self.areas, self.C, self.smooth = list(areas), int(num_classes), float(smooth)
        dev = self.device
        sizes = [a.sub_points.shape[0] for a in self.areas]
        self.sizes = sizes
        self.offsets = torch.tensor([0] + list(np.cumsum(sizes)[:-1]), dtype=torch.int64, device=dev)
        self.total = int(sum(sizes))
        # one extra column: the write target of masked slots, so that padding never touches a real point
        self.logits_sum = torch.zeros(self.C, self.total + 1, dtype=torch.float32, device=dev)
        self.counts = torch.full((1, self.total + 1), 1e-6, dtype=torch.float32, device=dev)
        self.running = torch.zeros(self.C, self.total + 1, dtype=torch.float32, device=dev)
        self.sub_labels = torch.from_numpy(np.concatenate([np.asarray(a.sub_labels) for a in self.areas]).astype(np.int64)).to(dev)
        props = np.zeros(self.C, dtype=np.float32)
        for k in range(self.C):
            props[k] = np.sum([np.sum(a.labels == k) for a in self.areas])
        self.val_proportions = torch.from_numpy(props).to(dev)
        self._proj = None
        # the confusion of the items' own predictions over one vote pass (s3dis_part_metrics), i64 [C, C] + a dump bin
        self.part_conf = torch.zeros(self.C * self.C + 1, dtype=torch.int64, device=dev)

    def add(self, pred, mask, cloud_index, input_inds):
        """pred f32[B,C,N] (logits), mask [B,N], cloud_index i64[B], input_inds i64[B,N] — one batch of the loop."""
        pred = pred.detach().float()
        B = pred.shape[0]
        live = mask.to(self.device).bool()
        g = input_inds.to(self.device).long() + self.offsets[cloud_index.to(self.device).long()][:, None]
        g = torch.where(live, g, torch.full_like(g, self.total))
        a = 1.0 - self.smooth
        truth = self.sub_labels[torch.clamp(g, max=self.total - 1)]
        cell = torch.where(live, truth * self.C + torch.argmax(pred, dim=1), torch.full_like(g, self.C * self.C))
        self.part_conf += torch.bincount(cell.reshape(-1), minlength=self.C * self.C + 1)
        for b in range(B):
            lg, gb = pred[b], g[b]
            self.logits_sum.index_add_(1, gb, torch.where(live[b][None], lg, torch.zeros_like(lg)))
            self.counts.index_add_(1, gb, live[b][None].float())
            self.running[:, gb] = self.smooth * self.running[:, gb] + a * lg

    def reset_votes(self):
        """A new validation (s3dis_closer_train.py:75-80): zero vote sums, counts back to 1e-6, and a new vote pass.  The
        running smoothed logits persist (train_segmentation_kpconv.py:206-207)."""
        self.logits_sum.zero_()
        self.counts.fill_(1e-6)
        self.start_pass()

    def start_pass(self):
        """A new vote pass: the part confusion starts from zero."""
        self.part_conf.zero_()

    def synced(self, dist):
        """The evaluator with its vote sums, vote counts and part confusion SUMmed over the ranks of `dist` (all-reduces on
        copies: this rank's own state keeps accumulating); itself without an active process group.  The running logits
        stay per rank, as in the reference.  Counts: every rank but 0 contributes its votes without the 1e-6 floor, so that
        the sum keeps one floor."""
        from .. import parallel
        if not parallel._active(dist):
            return self
        self.projections()
        out = copy.copy(self)
        out.logits_sum, out.part_conf = self.logits_sum.clone(), self.part_conf.clone()
        out.counts = self.counts.clone() if dist.get_rank() == 0 else torch.round(self.counts - 1e-6)
        for t in (out.logits_sum, out.counts, out.part_conf):
            dist.all_reduce(t)
        return out

    def part_ious(self):
        """s3dis_part_metrics: IoUs of the items' own predictions over the current vote pass, the confusion rescaled to
        the raw class proportions."""
        conf = self.part_conf[:self.C * self.C].view(self.C, self.C).float()
        conf = conf * (self.val_proportions / (conf.sum(1) + 1e-6))[:, None]
        iou = iou_from_confusions(conf)
        return iou.cpu().numpy(), float(iou.mean())

    def vote_logits(self):
        """vote_logits_sum / vote_counts over all clouds, f32[C, total]."""
        return (self.logits_sum / self.counts)[:, :self.total]

    def _sub(self, logits):
        pred = torch.argmax(logits, dim=0)
        conf = _confusion(self.sub_labels, pred, self.C).float()
        conf = conf * (self.val_proportions / (conf.sum(1) + 1e-6))[:, None]
        iou = iou_from_confusions(conf)
        return iou.cpu().numpy(), float(iou.mean())

    def sub_ious(self, running=False):
        """sub_s3dis_metrics: IoUs of the subsampled clouds, confusion rescaled to the raw class proportions; running=True
        scores the running smoothed logits instead of the vote average."""
        return self._sub(self.running[:, :self.total] if running else self.vote_logits())

    def projections(self):
        """Per Area, the nearest subsampled point of every raw point (s3dis_closer.py:285-299), i64 on the device."""
        if self._proj is None:
            from ..neighbors import GridIndex
            proj = []
            for a in self.areas:
                index = GridIndex(torch.from_numpy(np.ascontiguousarray(a.sub_points, np.float32)).to(self.device))
                idx, _ = index.nearest(torch.from_numpy(np.ascontiguousarray(a.points, np.float32)).to(self.device))
                proj.append(idx)
            self._proj = proj
        return self._proj

    def full_ious(self, k=1):
        """s3dis_metrics: IoUs at full resolution, every raw point taking the vote of its nearest subsampled point (k = 1,
        the reference's projection and the default).  With k > 1 every raw point takes the argmax of the inverse-distance
        interpolation of the vote logits over its k nearest subsampled points (GridIndex.interpolate) instead."""
        k = int(k)
        if k != 1:
            return self._full_ious_knn(k)
        logits = self.vote_logits()
        conf = torch.zeros(self.C, self.C, dtype=torch.int64, device=self.device)
        for a, off, proj in zip(self.areas, self.offsets.tolist(), self.projections()):
            pred = torch.argmax(logits[:, off + proj], dim=0)
            truth = torch.from_numpy(np.asarray(a.labels).astype(np.int64)).to(self.device)
            conf += _confusion(truth, pred, self.C)
        iou = iou_from_confusions(conf)
        return iou.cpu().numpy(), float(iou.mean())

    def _full_ious_knn(self, k):
        from .. import _lib
        from ..neighbors import GridIndex
        if not 1 <= k <= _lib.NBR_KNN_K_MAX:
            raise ValueError("full_ious: k must be in [1, %d]" % _lib.NBR_KNN_K_MAX)
        logits = self.vote_logits()
        conf = torch.zeros(self.C, self.C, dtype=torch.int64, device=self.device)
        for a, off, size in zip(self.areas, self.offsets.tolist(), self.sizes):
            index = GridIndex(torch.from_numpy(np.ascontiguousarray(a.sub_points, np.float32)).to(self.device))
            raw = torch.from_numpy(np.ascontiguousarray(a.points, np.float32)).to(self.device)
            pred = torch.argmax(index.interpolate(logits[:, off:off + size].t().contiguous(), raw, k), dim=1)
            truth = torch.from_numpy(np.asarray(a.labels).astype(np.int64)).to(self.device)
            conf += _confusion(truth, pred, self.C)
        iou = iou_from_confusions(conf)
        return iou.cpu().numpy(), float(iou.mean())
