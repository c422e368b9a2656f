"""Multi-planar MRI slice dataset — drop-in for PMU/utils/mri_dataset.py:11-143 (row a13).

Same constructor (imgs_dir, masks_dir, n_classes, filter=True), attributes (ids, views,
image_dims, index_map, len) and item format ({'image': (1,H,W) f32, 'mask': (1,H,W) f32}), and
the same semantics:
  * pad_dimensions: zeros appended to the end of the argmin axis up to the max dim (:85-98);
  * index map ordered scan -> view -> slice, keeping slices whose mask max > 0 when ``filter``
    (:37-49); views are image[i,:,:], image[:,j,:], image[:,:,k] (:70-82);
  * preprocess: image / its own max when that max is non-zero, mask untouched (:101-112).

MI355X-first differences:
  * every scan is read from disk ONCE and kept resident in HBM (the reference re-reads the
    whole volume from disk for every slice, :124-127), re-laid out per view so that each slice
    is one contiguous block (pmu_slice_view_layout, f64 so that the max normalisation is
    bit-identical to the reference's numpy arithmetic);
  * the index-map filter and the normalisation maxima come from one per-slice max reduction per
    view (pmu_slice_max);
  * items are produced on the GPU; ``get_batch(indices)`` assembles a whole batch in one launch
    per tensor (pmu_gather_slices) — what the training loop uses instead of a DataLoader.

Oblique views (``views=`` an (V,3) array or list of vectors; DESIGN.md "Oblique views"): every listed view
is cut on a P x P x P grid (``sample_dim``, default the largest padded dim of the scans; ``spacing`` voxels
apart) about the volume centre, along the frame ``view_frame`` gives its vector.  Only the padded volume
is resident; slices are sampled on the fly (pmu_oblique_slice_max for the maxima, pmu_oblique_gather for
the batches: trilinear fp64 images, nearest-voxel masks), so every slice of every scan is P x P and any
batch is legal.  ``views=None`` is the standard-axis path above, untouched.

Augmentation (``get_batch(indices, augment=, epoch=)``, ``get_slices(keys, augment=, epoch=)``; DESIGN.md
"Augmentation"): with a pmu_hip.augment.Augment every item is sampled from the resident volume through its
own random affine + elastic warp with an intensity gain / bias, image and mask in one launch
(pmu_warp_gather), on either path; shapes and dtypes are those of the plain batch.  ``augment=None`` is the
code above, untouched.

``loader`` (path -> ndarray) defaults to nibabel's ``nib.load(path).get_fdata()``; nibabel is an
optional dependency.  ``files`` replaces ``listdir(imgs_dir)`` (the reference's, unsorted order).
"""
from __future__ import annotations

import logging
from os import listdir, path

import numpy as np
import torch
from torch.utils.data import Dataset
from torch.utils.data.dataloader import default_collate

from pmu_hip import _lib as L


def _nib_load(p):
    try:
        import nibabel as nib
    except ImportError as e:  # pragma: no cover - depends on the host
        raise ImportError("MRI_Dataset needs nibabel to read NIfTI scans (or pass loader=...)") from e
    return nib.load(p).get_fdata()


def padded_shape(shape):
    """pad_dimensions' output shape: the (first) argmin axis grows by max - min (:85-98)."""
    shape = list(shape)
    diff = max(shape) - min(shape)
    if diff:
        shape[int(np.argmin(shape))] += diff
    return tuple(shape)


def view_slice_shape(pshape, view):
    p0, p1, p2 = pshape
    return [(p1, p2), (p0, p2), (p0, p1)][view]


def view_frame(n):
    """(3,3) float64 rows (n, u, v): the orthonormal frame of a view along ``n``.

    n is normalised and flipped so that its first largest |component| (index m) is positive; with
    e_a, e_b the two other standard axes in increasing order, u = normalise(e_a - (e_a.n) n) and
    v = +-(n x u) with v.e_b > 0.  n = e0, e1, e2 give (u, v) = (e1, e2), (e0, e2), (e0, e1) exactly:
    the standard views as sample_slice orients them (:70-82)."""
    n = np.asarray(n, dtype=np.float64).reshape(-1)
    if n.shape != (3,) or not np.all(np.isfinite(n)) or not np.any(n != 0.0):
        raise ValueError(f"a view needs a non-zero finite 3-vector, got {n}")
    n = n / np.sqrt(np.sum(n * n))
    m = int(np.argmax(np.abs(n)))
    if n[m] < 0:
        n = -n
    a, b = [i for i in range(3) if i != m]
    ea, eb = np.eye(3)[a], np.eye(3)[b]
    u = ea - n[a] * n
    u = u / np.sqrt(np.sum(u * u))
    v = np.cross(n, u)
    if np.dot(v, eb) < 0:
        v = -v
    return np.stack([n + 0.0, u + 0.0, v + 0.0])   # (+ 0.0: no negative zeros)


def draw_views(n_views=6, seed=0, min_angle_deg=30):
    """``n_views`` seeded unit vectors, canonicalised as view_frame does, pairwise at least
    ``min_angle_deg`` apart as lines (|cos| <= cos(min_angle_deg)): draws of
    RandomState(seed).normal(size=3), rejecting one too close to an accepted view."""
    rs = np.random.RandomState(seed)
    lim = np.cos(np.deg2rad(min_angle_deg))
    out = []
    for _ in range(100000):
        if len(out) == n_views:
            return out
        n = view_frame(rs.normal(size=3))[0]
        if all(abs(float(np.dot(n, o))) <= lim for o in out):
            out.append(n)
    raise ValueError(f"cannot place {n_views} views {min_angle_deg} degrees apart")


class _ScanOblique:
    """One scan resident in HBM for oblique views: the padded f64 image and mask volumes."""

    def __init__(self, img: np.ndarray, mask: np.ndarray, device):
        if img.ndim != 3 or mask.ndim != 3:
            raise ValueError("MRI_Dataset expects 3-D scans")
        self.pshape = padded_shape(img.shape)
        if padded_shape(mask.shape) != self.pshape:
            raise AssertionError(f"Image and mask should be the same size, but are {img.shape} and {mask.shape}")
        s = L.stream()
        p0, p1, p2 = self.pshape
        vols = []
        for vol in (img, mask):
            d = torch.from_numpy(np.ascontiguousarray(vol, dtype=np.float64)).to(device)
            d0, d1, d2 = vol.shape
            out = torch.empty(p0 * p1 * p2, dtype=torch.float64, device=device)
            L.call("pmu_slice_view_layout", d.data_ptr(), d0, d1, d2, p0, p1, p2, 0, out.data_ptr(), s)
            vols.append(out)
            del d
        self.img, self.mask = vols
        self.img_max, self.mask_max = [], []   # per view: (P,) f64, filled by MRI_Dataset.set_views


class _ScanViews:
    """One scan resident in HBM: per-view contiguous layouts of image and mask, per-slice maxima."""

    def __init__(self, img: np.ndarray, mask: np.ndarray, device):
        if img.ndim != 3 or mask.ndim != 3:
            raise ValueError("MRI_Dataset expects 3-D scans")
        self.pshape = padded_shape(img.shape)
        if padded_shape(mask.shape) != self.pshape:
            raise AssertionError(f"Image and mask should be the same size, but are {img.shape} and {mask.shape}")
        s = L.stream()
        self.img, self.mask, self.img_max, self.mask_max = [], [], [], []
        for vol, views, maxes in ((img, self.img, self.img_max), (mask, self.mask, self.mask_max)):
            d = torch.from_numpy(np.ascontiguousarray(vol, dtype=np.float64)).to(device)
            d0, d1, d2 = vol.shape
            p0, p1, p2 = self.pshape
            for v in range(3):
                out = torch.empty(p0 * p1 * p2, dtype=torch.float64, device=device)
                L.call("pmu_slice_view_layout", d.data_ptr(), d0, d1, d2, p0, p1, p2, v, out.data_ptr(), s)
                n = self.pshape[v]
                ha, hb = view_slice_shape(self.pshape, v)
                mx = torch.empty(n, dtype=torch.float64, device=device)
                L.call("pmu_slice_max", out.data_ptr(), n, ha * hb, mx.data_ptr(), s)
                views.append(out)
                maxes.append(mx)
            del d


class MRI_Dataset(Dataset):

    def __init__(self, imgs_dir, masks_dir, n_classes, filter=True, loader=None, files=None, device=None,
                 views=None, sample_dim=None, spacing=1.0):
        self.imgs_dir = imgs_dir
        self.masks_dir = masks_dir
        self.n_classes = n_classes
        self.len = 0
        self.oblique = views is not None
        self.views = self.initialize_views(use_standard_axis=True)
        self.ids = list(files) if files is not None else listdir(imgs_dir)
        self._load = loader or _nib_load
        self.device = torch.device(device) if device is not None else torch.device("cuda")
        if self.device.type != "cuda":
            raise RuntimeError("MRI_Dataset keeps scans resident on the GPU (there is no CPU fallback)")
        logging.info("Creating index mapping.")
        self.scans = []
        self.image_dims = None
        self.index_map = []
        if self.oblique:
            self._init_oblique(views, sample_dim, spacing, filter)
            return
        for scan, name in enumerate(self.ids):
            img = self._load(path.join(self.imgs_dir, name))
            mask = self._load(path.join(self.masks_dir, name))
            if self.image_dims is None:   # largest dim of the first scan, per axis (:28-29)
                self.image_dims = tuple([int(np.max(img.shape))] * len(img.shape))
            sv = _ScanViews(np.asarray(img), np.asarray(mask), self.device)
            self.scans.append(sv)
            fg = [(m > 0).cpu().numpy() for m in sv.mask_max]
            for view in range(len(self.views)):
                for sl in range(sv.pshape[view]):
                    if not filter or fg[view][sl]:
                        self.index_map.append((scan, view, sl))
        self.len = len(self.index_map)
        self._build_table()
        logging.info(f"Creating dataset of {len(self.ids)} scans, and {self.len} slices")

    def _build_table(self):
        """Device slice table for pmu_gather_slices: address and max of every (scan, view, slice)."""
        addr_i, addr_m, max_i, self._gid, self._shape = [], [], [], {}, {}
        for scan, sv in enumerate(self.scans):
            for v in range(3):
                ha, hb = view_slice_shape(sv.pshape, v)
                px = ha * hb
                for sl in range(sv.pshape[v]):
                    self._gid[(scan, v, sl)] = len(addr_i)
                    self._shape[(scan, v, sl)] = (ha, hb)
                    addr_i.append(sv.img[v].data_ptr() + sl * px * 8)
                    addr_m.append(sv.mask[v].data_ptr() + sl * px * 8)
            max_i.extend(sv.img_max)
        self._addr_img = torch.tensor(addr_i, dtype=torch.int64).to(self.device)
        self._addr_mask = torch.tensor(addr_m, dtype=torch.int64).to(self.device)
        self._max_img = torch.cat(max_i) if max_i else torch.empty(0, dtype=torch.float64, device=self.device)

    def _init_oblique(self, views, sample_dim, spacing, filter):
        """The oblique path: resident padded volumes, then set_views (maxima, index map, tables)."""
        for n in np.asarray(views, dtype=np.float64).reshape(-1, 3):   # refuse a bad view before loading
            view_frame(n)
        for name in self.ids:
            img = self._load(path.join(self.imgs_dir, name))
            mask = self._load(path.join(self.masks_dir, name))
            if self.image_dims is None:   # largest dim of the first scan, per axis (:28-29)
                self.image_dims = tuple([int(np.max(img.shape))] * len(img.shape))
            self.scans.append(_ScanOblique(np.asarray(img), np.asarray(mask), self.device))
        self.sample_dim = int(sample_dim) if sample_dim is not None else max(max(sv.pshape) for sv in self.scans)
        self.spacing = float(spacing)
        if self.sample_dim < 2 or not self.spacing > 0.0:
            raise ValueError(f"oblique views need sample_dim >= 2 and spacing > 0, got {sample_dim}, {spacing}")
        self._filter = filter
        self.set_views(views)
        logging.info(f"Creating dataset of {len(self.ids)} scans, and {self.len} slices")

    def set_views(self, views):
        """Replace the oblique views (e.g. a fresh initialize_views draw between epochs): the volumes stay
        resident; only the per-slice maxima, the index map and the device tables are rebuilt."""
        if not self.oblique:
            raise RuntimeError("set_views needs a dataset built with views=...")
        self.frames = np.stack([view_frame(n) for n in np.asarray(views, dtype=np.float64).reshape(-1, 3)])
        self.views = [f[0].copy() for f in self.frames]
        P, h, s = self.sample_dim, self.spacing, L.stream()
        dev_frames = torch.from_numpy(self.frames.reshape(-1, 9)).to(self.device)
        self.index_map = []
        for scan, sv in enumerate(self.scans):
            p0, p1, p2 = sv.pshape
            sv.img_max, sv.mask_max = [], []
            for vol, maxes, nearest in ((sv.img, sv.img_max, 0), (sv.mask, sv.mask_max, 1)):
                for v in range(len(self.views)):
                    mx = torch.empty(P, dtype=torch.float64, device=self.device)
                    L.call("pmu_oblique_slice_max", vol.data_ptr(), p0, p1, p2, dev_frames[v].data_ptr(), P, h,
                           nearest, mx.data_ptr(), s)
                    maxes.append(mx)
            fg = [(m > 0).cpu().numpy() for m in sv.mask_max]
            for view in range(len(self.views)):
                for sl in range(P):
                    if not self._filter or fg[view][sl]:
                        self.index_map.append((scan, view, sl))
        self.len = len(self.index_map)
        # device table for pmu_oblique_gather: one row per (scan, view); item id = row * P + slice
        V = len(self.views)
        self._nrows = len(self.scans) * V
        self._vaddr_img = torch.tensor([sv.img.data_ptr() for sv in self.scans for _ in range(V)],
                                       dtype=torch.int64).to(self.device)
        self._vaddr_mask = torch.tensor([sv.mask.data_ptr() for sv in self.scans for _ in range(V)],
                                        dtype=torch.int64).to(self.device)
        self._dims = torch.tensor([list(sv.pshape) for sv in self.scans for _ in range(V)],
                                  dtype=torch.int32).reshape(-1, 3).to(self.device)
        self._frames = dev_frames.repeat(len(self.scans), 1).contiguous()
        maxes = [m for sv in self.scans for m in sv.img_max]
        self._max_img = torch.cat(maxes) if maxes else torch.empty(0, dtype=torch.float64, device=self.device)

    def _get_slices_oblique(self, keys):
        P, V = self.sample_dim, len(self.views)
        for scan, view, sl in keys:
            if not (0 <= scan < len(self.scans) and 0 <= view < V and 0 <= sl < P):
                raise KeyError((scan, view, sl))
        B = len(keys)
        ids = torch.tensor([(scan * V + view) * P + sl for scan, view, sl in keys],
                           dtype=torch.int32).to(self.device, non_blocking=True)
        img = torch.empty(B, 1, P, P, dtype=torch.float32, device=self.device)
        mask = torch.empty(B, 1, P, P, dtype=torch.float32, device=self.device)
        s = L.stream()
        L.call("pmu_oblique_gather", self._vaddr_img.data_ptr(), self._dims.data_ptr(), self._frames.data_ptr(),
               self._max_img.data_ptr(), ids.data_ptr(), B, self._nrows, P, self.spacing, 0, img.data_ptr(), s)
        L.call("pmu_oblique_gather", self._vaddr_mask.data_ptr(), self._dims.data_ptr(), self._frames.data_ptr(),
               None, ids.data_ptr(), B, self._nrows, P, self.spacing, 1, mask.data_ptr(), s)
        return {"image": img, "mask": mask}

    def _warp_tables(self):
        """Device tables of pmu_warp_gather (vaddr_img, vaddr_mask, dims, frames, nrows, maxv).  Oblique: the
        ones set_views keeps.  Standard axes: one row per (scan, view) over view 0's resident layout (the
        padded volume itself) with the frame of e_view, built on first use; the maxima are the slice table's."""
        if self.oblique:
            return self._vaddr_img, self._vaddr_mask, self._dims, self._frames, self._nrows, self._max_img
        if getattr(self, "_warp_std", None) is None:
            frames = np.stack([view_frame(e) for e in np.eye(3)]).reshape(3, 9)
            self._warp_std = (
                torch.tensor([sv.img[0].data_ptr() for sv in self.scans for _ in range(3)],
                             dtype=torch.int64).to(self.device),
                torch.tensor([sv.mask[0].data_ptr() for sv in self.scans for _ in range(3)],
                             dtype=torch.int64).to(self.device),
                torch.tensor([list(sv.pshape) for sv in self.scans for _ in range(3)],
                             dtype=torch.int32).reshape(-1, 3).to(self.device),
                torch.from_numpy(np.tile(frames, (len(self.scans), 1))).to(self.device),
                3 * len(self.scans), self._max_img)
        return self._warp_std

    def _get_slices_warped(self, keys, augment, epoch):
        """Augmented items (DESIGN.md "Augmentation"): ``augment.draw`` gives every item its parameter block
        and control grid, one pmu_warp_gather launch writes image and mask.  Oblique datasets cut P x P at
        their spacing; standard-axis ones the view's slice shape at h = 1 about slice s (ds = s - (p_v-1)/2),
        one shape per batch as in get_slices.  The image is divided by the un-warped slice's maximum."""
        keys = [tuple(int(x) for x in k) for k in keys]
        if self.oblique:
            P, V, h = self.sample_dim, len(self.views), self.spacing
            for scan, view, sl in keys:
                if not (0 <= scan < len(self.scans) and 0 <= view < V and 0 <= sl < P):
                    raise KeyError((scan, view, sl))
            H = W = P
            item = [((scan * V + view), (scan * V + view) * P + sl) for scan, view, sl in keys]
            ds = [h * (sl - (P - 1) / 2.0) for _, _, sl in keys]
        else:
            shapes = {self._shape[k] for k in keys}
            if len(shapes) != 1:
                raise RuntimeError(f"slices of one batch must share a shape, got {sorted(shapes)}")
            (H, W), h = shapes.pop(), 1.0
            item = [(scan * 3 + view, self._gid[(scan, view, sl)]) for scan, view, sl in keys]
            ds = [sl - (self.scans[scan].pshape[view] - 1) / 2.0 for scan, view, sl in keys]
        B = len(keys)
        par, ctrl = augment.draw(keys, epoch, H, W, h)
        par = np.array(par, dtype=np.float64).reshape(B, 9)
        par[:, 0] = ds
        G = 0 if ctrl is None else int(np.shape(ctrl)[-1])
        if G and np.shape(ctrl) != (B, 2, G, G):
            raise ValueError(f"augment.draw must give a (B, 2, G, G) control grid, got {np.shape(ctrl)}")
        # one upload for the doubles: the parameter blocks, then the control grids
        host = par.reshape(-1) if not G else np.concatenate([par.reshape(-1), np.asarray(ctrl, np.float64).reshape(-1)])
        dbl = torch.from_numpy(np.ascontiguousarray(host)).to(self.device, non_blocking=True)
        it = torch.tensor(item, dtype=torch.int32).to(self.device, non_blocking=True)
        vimg, vmask, dims, frames, nrows, maxv = self._warp_tables()
        img = torch.empty(B, 1, H, W, dtype=torch.float32, device=self.device)
        mask = torch.empty(B, 1, H, W, dtype=torch.float32, device=self.device)
        L.call("pmu_warp_gather", vimg.data_ptr(), vmask.data_ptr(), dims.data_ptr(), frames.data_ptr(), nrows,
               it.data_ptr(), maxv.data_ptr(), dbl.data_ptr(), dbl[9 * B:].data_ptr() if G else None, G, B, H, W, h,
               img.data_ptr(), mask.data_ptr(), L.stream())
        return {"image": img, "mask": mask}

    def __len__(self):
        return self.len

    def initialize_views(self, use_standard_axis=False, n_views=6, seed=0, min_angle_deg=30):
        """Standard axes (:60-66); otherwise ``n_views`` seeded oblique view vectors (draw_views), which
        the reference leaves undefined — pass them as ``views=`` or to set_views."""
        standard_axis = [np.array([1, 0, 0]), np.array([0, 1, 0]), np.array([0, 0, 1])]
        if use_standard_axis:
            return standard_axis
        return draw_views(n_views, seed, min_angle_deg)

    def sample_slice(self, image, view, slice_index):
        """Host-side slice of an array (:70-82), kept for API parity."""
        if np.array_equal(view, self.views[0]):
            return image[slice_index, :, :]
        if np.array_equal(view, self.views[1]):
            return image[:, slice_index, :]
        if np.array_equal(view, self.views[2]):
            return image[:, :, slice_index]
        raise ValueError("No valid view")

    def pad_dimensions(self, image):
        """Host-side pad (:85-98), kept for API parity; the resident path pads on the GPU."""
        out = np.zeros(padded_shape(image.shape), dtype=image.dtype)
        out[:image.shape[0], :image.shape[1], :image.shape[2]] = image
        return out

    @classmethod
    def preprocess(cls, img, label=False):
        """(H,W) -> (1,H,W), image / max when max != 0 (:101-112) — host-side, for API parity."""
        if len(img.shape) == 2:
            img = np.expand_dims(img, axis=2)
        img_trans = np.transpose(img, [2, 0, 1])
        if not label and not np.max(img_trans) == 0:
            img_trans = img_trans / np.max(img_trans)
        return img_trans

    def get_batch(self, indices, augment=None, epoch=0):
        """{'image': (B,1,H,W), 'mask': (B,1,H,W)} f32 on the GPU for dataset indices (one launch each).
        ``augment`` (a pmu_hip.augment.Augment) warps every item with its draw for ``epoch``: one
        pmu_warp_gather launch for both tensors (get_slices)."""
        keys = [self.index_map[int(i)] for i in indices]
        if augment is None:
            return self.get_slices(keys)
        return self.get_slices(keys, augment, epoch)

    def get_slices(self, keys, augment=None, epoch=0):
        """Same as get_batch for explicit (scan, view, slice) keys (also slices the filter dropped)."""
        if augment is not None:
            return self._get_slices_warped(keys, augment, epoch)
        if self.oblique:
            return self._get_slices_oblique(keys)
        shapes = {self._shape[k] for k in keys}
        if len(shapes) != 1:
            raise RuntimeError(f"slices of one batch must share a shape, got {sorted(shapes)}")
        ha, hb = shapes.pop()
        B = len(keys)
        ids = torch.tensor([self._gid[k] for k in keys], dtype=torch.int32).to(self.device, non_blocking=True)
        img = torch.empty(B, 1, ha, hb, dtype=torch.float32, device=self.device)
        mask = torch.empty(B, 1, ha, hb, dtype=torch.float32, device=self.device)
        s = L.stream()
        L.call("pmu_gather_slices", self._addr_img.data_ptr(), self._max_img.data_ptr(), ids.data_ptr(), B, ha * hb,
               1, img.data_ptr(), s)
        L.call("pmu_gather_slices", self._addr_mask.data_ptr(), None, ids.data_ptr(), B, ha * hb, 0,
               mask.data_ptr(), s)
        return {"image": img, "mask": mask}

    def __getitem__(self, i):
        b = self.get_batch([i])
        return {"image": b["image"][0], "mask": b["mask"][0]}


def mri_collate(batch):
    """Collate that drops None items (train.py imports it; the reference file does not define it)."""
    return default_collate([b for b in batch if b is not None])
