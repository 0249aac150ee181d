"""Dataset plumbing for ``test.py`` (reference basicsr/data/__init__.py:33-118).  The reference's IO stack
(cv2, lmdb) is out of scope; what the hot path needs from it
is a dict with ``lq``/``gt`` float32 CHW tensors in [0,1] (+ ``dataset_idx``).  A minimal PIL reader covers
paired folders; when a configured root does not exist (the YAMLs point at /mnt/nasv3/...), a seeded synthetic
pair stands in so the CLI still runs end to end."""
from copy import deepcopy
from os import path as osp

import numpy as np
import torch
from torch.utils import data as tdata

from basicsr.utils import get_root_logger, scandir
from basicsr.utils.registry import DATASET_REGISTRY

__all__ = ["build_dataset", "build_dataloader", "paired_random_crop_augment", "degrade_collate", "filter2d_host"]
_IMG_EXT = (".png", ".jpg", ".jpeg", ".bmp", ".tif", ".tiff", ".PNG", ".JPG")


def _read_rgb(path):
    from PIL import Image

    with Image.open(path) as im:
        return torch.from_numpy(np.asarray(im.convert("RGB"), dtype=np.float32) / 255.0).permute(2, 0, 1).contiguous()


def _labelled(sample, opt):
    """a fixed degradation label for a stand-alone (validation) set: ``dataset_idx: k`` in its options"""
    if "dataset_idx" in opt:
        sample["dataset_idx"] = int(opt["dataset_idx"])
    return sample


def paired_random_crop_augment(lq, gt, opt):
    """train phase (reference basicsr/data/paired_image_dataset.py:152-166 with transforms.py paired_random_crop / augment): a
    ``gt_size // scale`` patch of the LQ image and the co-located ``gt_size`` patch of the GT image (``opt["scale"]``, default 1:
    the same crop of both), then the same horizontal flip and 90-degree rotation (vertical flip + transpose) of both images, drawn
    from Python's ``random`` like the reference."""
    import random

    size = opt.get("gt_size")
    if size:
        scale = int(opt.get("scale", 1) or 1)
        _, h, w = lq.shape
        _, h_gt, w_gt = gt.shape
        if h_gt != h * scale or w_gt != w * scale:
            raise ValueError(f"Scale mismatches. GT ({h_gt}, {w_gt}) is not {scale}x multiplication of LQ ({h}, {w}).")
        lsize = size // scale
        if h < lsize or w < lsize:
            raise ValueError(f"image ({h}, {w}) is smaller than the training patch ({lsize}, {lsize})")
        top, left = random.randint(0, h - lsize), random.randint(0, w - lsize)
        lq = lq[:, top:top + lsize, left:left + lsize]
        gt = gt[:, top * scale:top * scale + size, left * scale:left * scale + size]
    hflip = opt.get("use_hflip", opt.get("use_flip", False)) and random.random() < 0.5
    vflip = opt.get("use_rot", False) and random.random() < 0.5
    rot90 = opt.get("use_rot", False) and random.random() < 0.5
    out = []
    for t in (lq, gt):
        if hflip:
            t = t.flip(2)
        if vflip:
            t = t.flip(1)
        if rot90:
            t = t.transpose(1, 2)
        out.append(t.contiguous())
    return out[0], out[1]


@DATASET_REGISTRY.register()
class SyntheticPairedDataset(tdata.Dataset):
    """``num`` seeded image pairs of ``size`` (gt = smooth random field, lq = gt + noise)."""

    def __init__(self, opt):
        super().__init__()
        self.opt = opt
        self.num = int(opt.get("num", 1))
        size = opt.get("size", 256)
        self.size = (size, size) if isinstance(size, int) else tuple(size)
        self.seed = int(opt.get("seed", 0))
        self.sigma = float(opt.get("sigma_range", 25)) / 255.0

    def __len__(self):
        return self.num

    def __getitem__(self, index):
        g = torch.Generator().manual_seed(self.seed * 100003 + index)
        h, w = self.size
        low = torch.rand((1, 3, max(2, h // 16), max(2, w // 16)), generator=g)
        gt = torch.nn.functional.interpolate(low, size=(h, w), mode="bilinear", align_corners=False)[0].clamp(0, 1)
        lq = (gt + self.sigma * torch.randn((3, h, w), generator=g)).clamp(0, 1)
        if self.opt.get("phase") == "train":
            lq, gt = paired_random_crop_augment(lq, gt, self.opt)
        name = f"synthetic_{index:04d}"
        return _labelled({"lq": lq, "gt": gt, "lq_path": name, "gt_path": name}, self.opt)


def _center_crop(t, size):
    """transforms.center_crop on a CHW tensor"""
    size = (size, size) if isinstance(size, int) else tuple(size)
    _, h, w = t.shape
    top, left = (h - size[0]) // 2, (w - size[1]) // 2
    return t[:, top:top + size[0], left:left + size[1]]


@DATASET_REGISTRY.register()
class PairedImageDataset(tdata.Dataset):
    """Paired folders with identical file names (reference basicsr/data/paired_image_dataset.py:25-192, folder mode,
    PIL instead of cv2): train phase = paired random crop + flips / rotation, other phases = optional centre crop."""

    def __init__(self, opt):
        super().__init__()
        self.opt = opt
        self.gt_root, self.lq_root = opt["dataroot_gt"], opt.get("dataroot_lq") or opt["dataroot_gt"]
        self.names = sorted(f for f in scandir(self.gt_root) if f.endswith(_IMG_EXT))

    def __len__(self):
        return len(self.names)

    def __getitem__(self, index):
        name = self.names[index]
        gt = _read_rgb(osp.join(self.gt_root, name))
        lq = _read_rgb(osp.join(self.lq_root, name))
        if self.opt.get("phase") == "train":
            lq, gt = paired_random_crop_augment(lq, gt, self.opt)
        elif self.opt.get("center_crop") is not None:
            lq, gt = _center_crop(lq, self.opt["center_crop"]), _center_crop(gt, self.opt["center_crop"])
        return _labelled({"lq": lq, "gt": gt, "lq_path": osp.join(self.lq_root, name), "gt_path": osp.join(self.gt_root, name)}, self.opt)


@DATASET_REGISTRY.register()
class PairedImageDenoiseDataset(tdata.Dataset):
    """GT folder + on-the-fly Gaussian noise (reference basicsr/data/paired_image_dataset.py:276-421).  The noise reproduces
    the reference's draw exactly (:388-402): ``sigma`` from ``sigma_type`` constant / random / choice (Python's ``random``),
    ``np.random.seed(index)`` in the train phase and ``seed(0)`` otherwise, ``normal(0, sigma / 255, (H, W, 3))`` on the
    **HWC**, RGB-ordered float32 image AFTER the crop / augmentation, added in float32.

    ``noise_backend: host`` (default) is that draw.  ``noise_backend: device``: the sample carries ``gt``, ``noise_sigma`` (a float32
    scalar, from the same ``random`` draw in the same order as the host path), ``noise_key`` (an int64 scalar) and the paths, and no
    ``lq``; the model's ``feed_data`` makes ``lq`` with ``dcpt_amd.functional.gaussian_noise(gt, noise_sigma, noise_key)``, unclipped
    like the host path.  In the train phase the key is ``random.getrandbits(63)``: fresh noise every epoch, reproducible under the
    loader's worker seeding.  In other phases it is ``(noise_seed << 32) | index`` (``noise_seed`` default 0): a validation set sees
    the same noise on every visit.  The device stream is Philox4x32-10, not MT19937, so its noise equals the host path's in
    distribution and not in value: numbers comparable with the paper's ``np.random.seed(0)`` test noise need the ``host`` backend.

    ``noise_type: gaussian`` (default) is all of the above.  ``noise_type: poisson`` (shot noise, ``noise_backend: device`` only: there is
    no host form): ``sigma_type`` / ``sigma_range`` are not read; after the crop and the augmentation the sample draws its scale from
    ``poisson_scale`` (a number, or ``[lo, hi]`` for one ``random.uniform``), then its gray decision (``random.random() < gray_prob``,
    default 0; the draw is always made), then the key as above.  It carries ``gt``, ``poisson_scale`` (float32 scalar), ``poisson_gray``
    (int32 scalar), ``noise_key`` and the paths, and no ``lq``; ``feed_data`` makes ``lq`` with
    ``dcpt_amd.functional.poisson_noise(gt, poisson_scale, noise_key, gray=poisson_gray, clip=True)``, clipped as ``add_poisson_noise_pt``
    defaults.  Poisson samples form batches of their own kind only: they have no ``degrade_kind``, and ``degrade_collate`` refuses them
    next to samples of another kind."""

    def __init__(self, opt):
        super().__init__()
        self.opt = opt
        self.gt_root = opt["dataroot_gt"]
        self.backend = opt.get("noise_backend", "host")
        if self.backend not in ("host", "device"):
            raise ValueError(f"noise_backend must be 'host' or 'device', got {self.backend!r}")
        self.noise_type = opt.get("noise_type", "gaussian")
        if self.noise_type not in ("gaussian", "poisson"):
            raise ValueError(f"noise_type must be 'gaussian' or 'poisson', got {self.noise_type!r}")
        if self.noise_type == "poisson":
            if self.backend != "device":
                raise ValueError("noise_type: poisson needs noise_backend: device (Poisson noise has no host backend)")
            self.poisson_scale = opt.get("poisson_scale", 1.0)
            ok = isinstance(self.poisson_scale, (int, float)) or (isinstance(self.poisson_scale, (list, tuple)) and len(self.poisson_scale) == 2)
            if not ok or min(self.poisson_scale if isinstance(self.poisson_scale, (list, tuple)) else [self.poisson_scale]) < 0:
                raise ValueError(f"poisson_scale must be a non-negative number or [lo, hi], got {self.poisson_scale!r}")
            self.gray_prob = float(opt.get("gray_prob", 0))
        else:
            self.sigma_type = opt.get("sigma_type", "constant")
            self.sigma_range = opt["sigma_range"]
            assert self.sigma_type in ["constant", "random", "choice"]
        self.noise_seed = int(opt.get("noise_seed", 0))
        if not 0 <= self.noise_seed < (1 << 31):
            raise ValueError(f"noise_seed must lie in 0..2^31 - 1, got {self.noise_seed}")
        self.names = sorted(f for f in scandir(self.gt_root) if f.endswith(_IMG_EXT))

    def __len__(self):
        return len(self.names)

    def __getitem__(self, index):
        import random

        path = osp.join(self.gt_root, self.names[index])
        gt = _read_rgb(path)
        if self.opt.get("phase") == "train":
            _, gt = paired_random_crop_augment(gt, gt, {**self.opt, "scale": 1})   # the reference crops at scale 1 here (:368-370)
        elif self.opt.get("center_crop") is not None:
            gt = _center_crop(gt, self.opt["center_crop"])
        if self.noise_type == "poisson":
            scale = random.uniform(*self.poisson_scale) if isinstance(self.poisson_scale, (list, tuple)) else self.poisson_scale
            gray = random.random() < self.gray_prob
            key = random.getrandbits(63) if self.opt.get("phase") == "train" else (self.noise_seed << 32) | index
            return _labelled({"gt": gt.contiguous(), "lq_path": path, "gt_path": path, "poisson_scale": torch.tensor(float(scale), dtype=torch.float32),
                              "poisson_gray": torch.tensor(int(gray), dtype=torch.int32), "noise_key": torch.tensor(key, dtype=torch.int64)},
                             self.opt)
        if self.sigma_type == "constant":
            sigma = self.sigma_range
        elif self.sigma_type == "random":
            sigma = random.uniform(self.sigma_range[0], self.sigma_range[1])
        else:
            sigma = random.choice(self.sigma_range)
        if self.backend == "device":
            key = random.getrandbits(63) if self.opt.get("phase") == "train" else (self.noise_seed << 32) | index
            return _labelled({"gt": gt.contiguous(), "lq_path": path, "gt_path": path, "noise_sigma": torch.tensor(float(sigma), dtype=torch.float32),
                              "noise_key": torch.tensor(key, dtype=torch.int64)}, self.opt)
        rs = np.random.RandomState(index if self.opt.get("phase") == "train" else 0)   # == np.random.seed(...); np.random.normal
        hwc = gt.permute(1, 2, 0).contiguous().numpy().copy()
        hwc += rs.normal(0, sigma / 255.0, hwc.shape)   # float64 noise accumulated into the float32 image, as `img_lq += ...`
        lq = torch.from_numpy(hwc.transpose(2, 0, 1)).float().contiguous()
        return _labelled({"lq": lq, "gt": gt.contiguous(), "lq_path": path, "gt_path": path}, self.opt)


@DATASET_REGISTRY.register()
class PairedImageJPEGCARDataset(tdata.Dataset):
    """GT folder + on-the-fly JPEG compression artifacts (reference basicsr/data/paired_image_dataset.py:425-580, folder mode, PIL
    reader).  Options: ``dataroot_gt``, ``q_type`` constant / random / choice with ``q_range``, ``gt_size`` (default 128), ``use_hflip``,
    ``use_rot``, ``center_crop``.  The train phase crops at scale 1 and augments, other phases apply the optional centre crop (:516-530);
    the quality is drawn from Python's ``random`` exactly as the reference draws it (:532-537), after the crop and the augmentation.

    ``jpeg_backend: pil`` (default): ``lq`` is ``(gt * 255).round()`` as uint8, encoded as a JPEG of that quality by PIL, decoded and
    divided by 255 -- a stand-in for the reference's ``cv2.imencode`` / ``imdecode`` (:539-546).  Both are libjpeg with the standard
    tables and 4:2:0 chroma, but cv2 is not a dependency of this package and the stand-in has not been compared with it byte for byte;
    PIL takes an integer quality, so a ``random`` draw is truncated for the encoder.

    ``jpeg_backend: device``: the sample carries ``gt``, ``jpeg_quality`` (a float32 scalar) and the paths, and no ``lq``; the model's
    ``feed_data`` makes ``lq`` on the device with the DiffJPEG kernel (``dcpt_amd.functional.diffjpeg(gt, quality, uint8_io=True)``), the
    codec the reference's dataset names as its alternative (:466-468, :564-565)."""

    def __init__(self, opt):
        super().__init__()
        self.opt = opt
        self.gt_root = opt["dataroot_gt"]
        self.q_type = opt["q_type"]
        self.q_range = opt["q_range"]
        assert self.q_type in ["constant", "random", "choice"]
        self.backend = opt.get("jpeg_backend", "pil")
        if self.backend not in ("pil", "device"):
            raise ValueError(f"jpeg_backend must be 'pil' or 'device', got {self.backend!r}")
        self.gt_size = opt.get("gt_size", 128)
        self.names = sorted(f for f in scandir(self.gt_root) if f.endswith(_IMG_EXT))

    def __len__(self):
        return len(self.names)

    @staticmethod
    def _pil_round_trip(gt, quality):
        import io

        from PIL import Image

        hwc = (gt.permute(1, 2, 0) * 255).round().to(torch.uint8).contiguous().numpy()
        buf = io.BytesIO()
        Image.fromarray(hwc).save(buf, format="JPEG", quality=int(quality))
        buf.seek(0)
        with Image.open(buf) as im:
            dec = np.asarray(im.convert("RGB"), dtype=np.float32) / 255.0
        return torch.from_numpy(dec).permute(2, 0, 1).contiguous()

    def __getitem__(self, index):
        import random

        path = osp.join(self.gt_root, self.names[index])
        gt = _read_rgb(path)
        if self.opt.get("phase") == "train":
            _, gt = paired_random_crop_augment(gt, gt, {**self.opt, "gt_size": self.gt_size, "scale": 1})
        elif self.opt.get("center_crop") is not None:
            gt = _center_crop(gt, self.opt["center_crop"])
        gt = gt.contiguous()
        if self.q_type == "constant":
            q_value = self.q_range
        elif self.q_type == "random":
            q_value = random.uniform(self.q_range[0], self.q_range[1])
        else:
            q_value = random.choice(self.q_range)
        sample = {"gt": gt, "lq_path": path, "gt_path": path}
        if self.backend == "device":
            sample["jpeg_quality"] = torch.tensor(float(q_value), dtype=torch.float32)
        else:
            sample["lq"] = self._pil_round_trip(gt, q_value)
        return _labelled(sample, self.opt)


DEMOSAIC_METHODS = ("malvar", "bilinear")   # the int a ``demosaic_backend: device`` sample carries in ``mosaic`` is the index


def _round_to_grid(s, unit):
    """rint(clamp(S / unit, 0, 255)) in integers, half to even"""
    q, r = np.divmod(s, unit)
    q = q + ((2 * r > unit) | ((2 * r == unit) & (q % 2 == 1)))
    return np.clip(q, 0, 255)


def demosaic_host(gt, method="malvar"):
    """``dcpt_amd.functional.demosaic(gt[None], method, uint8_io=True)[0]`` on the host, in numpy integers (include/dcpt_hip.h
    dcpt_demosaic_fwd states the arithmetic): the RGGB mosaic of the 8-bit image ``rint(clamp(gt, 0, 1) * 255)``, the Malvar (reflect
    padding, units of 1/16) or bilinear (circular padding, units of 1/4) tap sums, ``rint(clamp(S / unit, 0, 255)) / 255`` half to even.
    Integer-exact, so it equals the kernel's result bit for bit.  gt: (3, H, W) float32 with H, W >= 3; returns (3, H, W) float32."""
    if method not in DEMOSAIC_METHODS:
        raise ValueError(f"demosaic_method must be one of {DEMOSAIC_METHODS}, got {method!r}")
    _, h, w = gt.shape
    if h < 3 or w < 3:
        raise ValueError(f"the demosaic needs an image of at least 3 x 3, got ({h}, {w})")
    v = torch.round(gt.float().clamp(0, 1) * 255).numpy().astype(np.int64)
    rows, cols = np.indices((h, w)) % 2
    site = np.where(rows != cols, 1, np.where(rows == 0, 0, 2))   # the colour of each RGGB site
    cfa = np.take_along_axis(v, site[None], 0)[0]
    out = np.empty((3, h, w), dtype=np.int64)
    if method == "malvar":
        p = np.pad(cfa, 2, mode="reflect")

        def at(dy, dx):
            return p[2 + dy:2 + dy + h, 2 + dx:2 + dx + w]

        c = at(0, 0)
        h1, v1 = at(0, -1) + at(0, 1), at(-1, 0) + at(1, 0)
        h2, v2 = at(0, -2) + at(0, 2), at(-2, 0) + at(2, 0)
        d = at(-1, -1) + at(-1, 1) + at(1, -1) + at(1, 1)
        g = 8 * c + 4 * (h1 + v1) - 2 * (h2 + v2)
        cross = 12 * c + 4 * d - 3 * (h2 + v2)
        hz = 10 * c + 8 * h1 - 2 * h2 + v2 - 2 * d
        vt = 10 * c + 8 * v1 - 2 * v2 + h2 - 2 * d
        out[1] = np.where(site == 1, 16 * c, g)
        out[0] = np.where(site == 0, 16 * c, np.where(site == 2, cross, np.where(rows == 0, hz, vt)))
        out[2] = np.where(site == 2, 16 * c, np.where(site == 0, cross, np.where(rows == 0, vt, hz)))
        unit = 16
    else:
        sparse = np.stack([np.where(site == k, cfa, 0) for k in range(3)])
        p = np.pad(sparse, ((0, 0), (1, 1), (1, 1)), mode="wrap")
        out[:] = 0
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                win = p[:, 1 + dy:1 + dy + h, 1 + dx:1 + dx + w]
                out[0] += (2 - abs(dy)) * (2 - abs(dx)) * win[0]
                out[2] += (2 - abs(dy)) * (2 - abs(dx)) * win[2]
                out[1] += (4 if dy == dx == 0 else (1 if dy == 0 or dx == 0 else 0)) * win[1]
        unit = 4
    return torch.from_numpy(_round_to_grid(out, unit).astype(np.float32) / np.float32(255))


def line_mask_host(lines, n_lines, thick, h, w):
    """the (H, W) boolean stroke mask of dcpt_inpaint_lines_fwd in numpy int64: a pixel within ``thick / 2`` of one of the first
    ``n_lines`` segments ``x1, y1, x2, y2``"""
    py, px = np.indices((h, w), dtype=np.int64)
    mask = np.zeros((h, w), dtype=bool)
    t2 = int(thick) * int(thick)
    for x1, y1, x2, y2 in [[int(v) for v in row] for row in lines[:n_lines]]:
        qx, qy, dx, dy = px - x1, py - y1, x2 - x1, y2 - y1
        a, seg = qx * dx + qy * dy, dx * dx + dy * dy
        head = 4 * (qx * qx + qy * qy) <= t2
        tail = 4 * ((qx - dx) ** 2 + (qy - dy) ** 2) <= t2
        side = 4 * (qx * dy - qy * dx) ** 2 <= t2 * seg
        mask |= np.where(a <= 0, head, np.where(a >= seg, tail, side))
    return mask


class _GTFolderDataset(tdata.Dataset):
    """a GT folder read with PIL; the train phase crops at scale 1 (``gt_size``, default 128) and augments, other phases apply the optional
    ``center_crop``"""

    def __init__(self, opt):
        super().__init__()
        self.opt = opt
        self.gt_root = opt["dataroot_gt"]
        self.gt_size = opt.get("gt_size", 128)
        self.names = sorted(f for f in scandir(self.gt_root) if f.endswith(_IMG_EXT))

    def __len__(self):
        return len(self.names)

    def _gt(self, index):
        path = osp.join(self.gt_root, self.names[index])
        gt = _read_rgb(path)
        if self.opt.get("phase") == "train":
            _, gt = paired_random_crop_augment(gt, gt, {**self.opt, "gt_size": self.gt_size, "scale": 1})
        elif self.opt.get("center_crop") is not None:
            gt = _center_crop(gt, self.opt["center_crop"])
        return gt.contiguous(), path


def _backend(opt, key):
    backend = opt.get(key, "host")
    if backend not in ("host", "device"):
        raise ValueError(f"{key} must be 'host' or 'device', got {backend!r}")
    return backend


@DATASET_REGISTRY.register()
class PairedImageMosaicDataset(_GTFolderDataset):
    """GT folder + on-the-fly Bayer mosaic and demosaic (reference basicsr/data/paired_image_dataset.py:732-870, folder mode, PIL reader):
    ``lq`` is the RGGB mosaic of the 8-bit ``gt`` put back to three channels by a linear demosaic.  Options: ``dataroot_gt``, ``gt_size``
    (default 128), ``use_hflip``, ``use_rot``, ``center_crop``, ``demosaic_method: malvar | bilinear``, ``demosaic_backend``.

    The reference demosaics with cv2's edge-aware ``COLOR_BAYER_BG2BGR_EA``; cv2 is not a dependency of this package.  Malvar-He-Cutler
    (``dm_matlab``) is the form the reference's own ``basicsr/utils/mosaic_util.py`` offers, with ``dm`` (bilinear) beside it; the two have
    NOT been compared with cv2's result here.  Odd image sizes are supported, an extension: the reference's ``mosaic_CFA_Bayer`` refuses them.

    ``demosaic_backend: host`` (default): ``lq`` is computed in the worker in numpy integers (``demosaic_host``) and equals the device
    result bit for bit.  ``demosaic_backend: device``: the sample carries ``gt``, ``mosaic`` (an int32 scalar: 0 malvar, 1 bilinear) and
    the paths, and no ``lq``; the model's ``feed_data`` makes ``lq`` with ``dcpt_amd.functional.demosaic(gt, method, uint8_io=True)``."""

    def __init__(self, opt):
        super().__init__(opt)
        self.backend = _backend(opt, "demosaic_backend")
        self.method = opt.get("demosaic_method", "malvar")
        if self.method not in DEMOSAIC_METHODS:
            raise ValueError(f"demosaic_method must be one of {DEMOSAIC_METHODS}, got {self.method!r}")

    def __getitem__(self, index):
        gt, path = self._gt(index)
        sample = {"gt": gt, "lq_path": path, "gt_path": path}
        if self.backend == "device":
            sample["mosaic"] = torch.tensor(DEMOSAIC_METHODS.index(self.method), dtype=torch.int32)
        else:
            sample["lq"] = demosaic_host(gt, self.method)
        return _labelled(sample, self.opt)


@DATASET_REGISTRY.register()
class PairedImageInpaintingDataset(_GTFolderDataset):
    """GT folder + on-the-fly line masks (reference basicsr/data/paired_image_dataset.py:873-1029, folder mode, PIL reader).  After the crop
    and the augmentation the strokes are drawn from Python's ``random`` in the reference's order (:981-1019): ``randint(5, 10)`` strokes,
    ``randint(5, 10)`` thick, ``choice(['white', 'black'])``, then per stroke ``randint(0, w), randint(0, h), randint(0, w),
    randint(0, h)``.  A masked pixel of ``lq`` is 1 (white) or 0 in every channel, every other pixel ``clamp(gt, 0, 1)``.

    The reference rasterises with ``cv2.polylines(mask, [pts], 0, (1, 1, 1), thick)``, which draws a quad plus round caps; the rule here
    -- a pixel within ``thick / 2`` of the segment, in exact integers (include/dcpt_hip.h dcpt_inpaint_lines_fwd) -- is the ideal shape of
    that and may differ from cv2 at boundary pixels.  UNVERIFIED: cv2 is not a dependency of this package.

    ``inpaint_backend: host`` (default): a numpy mask by that rule in the worker (``line_mask_host``).  ``inpaint_backend: device``: the
    sample carries ``gt``, ``inpaint_lines`` (int32 (10, 4), unused rows zero), ``inpaint_meta`` (int32 (3,): n_lines, thick, white) and
    the paths, and no ``lq``; the model's ``feed_data`` makes ``lq`` with ``dcpt_amd.functional.inpaint_lines``.

    ``stroke_seed: k`` (an extension; default none, the reference's behaviour): image ``index`` draws its strokes from a
    ``random.Random(k + index)`` of its own instead of the process-wide generator, so a validation set shows the same masks on every
    visit and two sets over one folder show the same masks."""

    def __init__(self, opt):
        super().__init__(opt)
        self.backend = _backend(opt, "inpaint_backend")
        self.stroke_seed = opt.get("stroke_seed")

    def __getitem__(self, index):
        import random

        gt, path = self._gt(index)
        _, h, w = gt.shape
        if self.stroke_seed is not None:
            random = random.Random(self.stroke_seed + index)   # (the same calls in the same order, on a generator of the image's own)
        l_num, l_thick = random.randint(5, 10), random.randint(5, 10)
        white = random.choice(["white", "black"]) == "white"
        lines = np.zeros((10, 4), dtype=np.int32)
        for k in range(l_num):
            lines[k] = (random.randint(0, w), random.randint(0, h), random.randint(0, w), random.randint(0, h))
        sample = {"gt": gt, "lq_path": path, "gt_path": path}
        if self.backend == "device":
            sample["inpaint_lines"] = torch.from_numpy(lines)
            sample["inpaint_meta"] = torch.tensor([l_num, l_thick, int(white)], dtype=torch.int32)
        else:
            lq = gt.clamp(0, 1)
            lq[:, torch.from_numpy(line_mask_host(lines, l_num, l_thick, h, w))] = 1.0 if white else 0.0
            sample["lq"] = lq
        return _labelled(sample, self.opt)


BLUR_MAX_K = 51   # the largest kernel of dcpt_filter2d_fwd


def filter2d_host(gt, kernel):
    """``dcpt_amd.functional.filter2d(gt[None], kernel[None])[0]`` on the host, in numpy float64 with the kernel's tap order
    (include/dcpt_hip.h dcpt_filter2d_fwd): the image reflect-padded by K // 2, one accumulator per output, ``acc += kernel[dy][dx] *
    xpad[.. + dy][.. + dx]`` for dy outer and dx inner, both ascending, rounded once to fp32.  A product of two fp32 values is exact in
    float64, so the multiply-add rounds where the kernel's fused one does and the result equals the kernel's bit for bit.  ``gt``:
    (C, H, W) float32 tensor or array, ``kernel``: (K, K), K odd, 1..51, K // 2 < H and W; returns (C, H, W) float32 of gt's kind."""
    as_tensor = torch.is_tensor(gt)
    x = (gt.detach().cpu().numpy() if as_tensor else np.asarray(gt)).astype(np.float32, copy=False)
    k = (kernel.detach().cpu().numpy() if torch.is_tensor(kernel) else np.asarray(kernel)).astype(np.float32, copy=False)
    if x.ndim != 3 or k.ndim != 2 or k.shape[0] != k.shape[1]:
        raise ValueError(f"filter2d_host takes a (C, H, W) image and a (K, K) kernel, got {x.shape} and {k.shape}")
    K, (_, h, w) = k.shape[0], x.shape
    if K % 2 == 0 or not 1 <= K <= BLUR_MAX_K:
        raise ValueError(f"the blur kernel size must be odd and lie in 1..{BLUR_MAX_K}, got {K}")
    if K // 2 >= h or K // 2 >= w:
        raise ValueError(f"the reflect padding K // 2 = {K // 2} must be smaller than the image, got ({h}, {w})")
    r = K // 2
    p = np.pad(x.astype(np.float64), ((0, 0), (r, r), (r, r)), mode="reflect")
    k = k.astype(np.float64)
    acc = np.zeros(x.shape, dtype=np.float64)
    for dy in range(K):
        for dx in range(K):
            acc += k[dy, dx] * p[:, dy:dy + h, dx:dx + w]
    out = acc.astype(np.float32)
    return torch.from_numpy(out) if as_tensor else out


@DATASET_REGISTRY.register()
class PairedImageBlurDataset(_GTFolderDataset):
    """GT folder + on-the-fly synthetic blur: ``lq`` is ``gt`` filtered with a random kernel of the reference's blur toolbox
    (basicsr/data/degradations.py ``random_mixed_kernels`` / ``circular_lowpass_kernel``, the first-order blur of its Real-ESRGAN data sets).
    Options: ``dataroot_gt``, ``gt_size`` (default 128), ``use_hflip``, ``use_rot``, ``center_crop``; ``blur_kernel_size`` (odd, 3..51,
    default 21); ``kernel_list`` (default all six kinds), ``kernel_prob`` (default uniform), ``blur_sigma`` (default [0.2, 3]),
    ``betag_range`` (default [0.5, 4]), ``betap_range`` (default [1, 2]); ``sinc_prob`` (default 0); ``blur_backend``; ``kernel_seed``.

    After the crop and the augmentation, with probability ``sinc_prob`` (one ``uniform`` draw of ``np.random``, made only when
    ``sinc_prob`` > 0) the kernel is ``circular_lowpass_kernel(uniform(pi / 3, pi), K)``, otherwise ``random_mixed_kernels(kernel_list,
    kernel_prob, K, blur_sigma, blur_sigma, [-pi, pi], betag_range, betap_range, noise_range=None)``; it is cast to fp32.  The draws come
    from the process-wide ``random`` / ``np.random``; with ``kernel_seed: k`` (an extension, the idea of ``stroke_seed``) image ``index``
    draws from ``(random.Random(k + index), np.random.RandomState(k + index))`` of its own, so a validation set sees the same blur on
    every visit.

    ``blur_backend: host`` (default): ``lq = filter2d_host(gt, kernel)`` in the worker, equal to the device result bit for bit.
    ``blur_backend: device``: the sample carries ``gt``, ``blur_kernel`` ((K, K) fp32) and the paths, and no ``lq``; the model's
    ``feed_data`` makes ``lq`` with ``dcpt_amd.functional.filter2d(gt, blur_kernel)``."""

    KINDS = ("iso", "aniso", "generalized_iso", "generalized_aniso", "plateau_iso", "plateau_aniso")

    def __init__(self, opt):
        super().__init__(opt)
        self.backend = _backend(opt, "blur_backend")
        self.K = opt.get("blur_kernel_size", 21)
        if not isinstance(self.K, int) or self.K % 2 == 0 or not 3 <= self.K <= BLUR_MAX_K:
            raise ValueError(f"blur_kernel_size must be odd and lie in 3..{BLUR_MAX_K}, got {self.K!r}")
        self.kernel_list = list(opt.get("kernel_list", self.KINDS))
        self.kernel_prob = list(opt.get("kernel_prob", [1.0 / len(self.kernel_list)] * len(self.kernel_list)))
        if not self.kernel_list or not set(self.kernel_list) <= set(self.KINDS):
            raise ValueError(f"kernel_list holds kinds of {self.KINDS}, got {self.kernel_list}")
        if len(self.kernel_prob) != len(self.kernel_list) or min(self.kernel_prob) < 0 or sum(self.kernel_prob) <= 0:
            raise ValueError(f"kernel_prob must hold one non-negative weight per entry of kernel_list, got {self.kernel_prob}")
        self.blur_sigma = self._range(opt, "blur_sigma", [0.2, 3])
        self.betag_range = self._range(opt, "betag_range", [0.5, 4])
        self.betap_range = self._range(opt, "betap_range", [1, 2])
        self.sinc_prob = float(opt.get("sinc_prob", 0))
        if not 0 <= self.sinc_prob <= 1:
            raise ValueError(f"sinc_prob must lie in [0, 1], got {self.sinc_prob}")
        self.kernel_seed = opt.get("kernel_seed")
        if opt.get("phase") == "train" and self.gt_size <= self.K // 2:
            raise ValueError(f"gt_size {self.gt_size} must exceed blur_kernel_size // 2 = {self.K // 2} (the reflect padding of the blur)")

    @staticmethod
    def _range(opt, key, default):
        v = opt.get(key, default)
        if not isinstance(v, (list, tuple)) or len(v) != 2 or not 0 < v[0] < v[1]:
            raise ValueError(f"{key} must be [low, high] with 0 < low < high, got {v!r}")
        return [float(v[0]), float(v[1])]

    def blur_kernel(self, index):
        """the (K, K) fp32 kernel of image ``index``: its own generators under ``kernel_seed``, the process-wide ones otherwise"""
        import math
        import random

        from basicsr.data.degradations import circular_lowpass_kernel, random_mixed_kernels

        rng = (random, np.random) if self.kernel_seed is None else (random.Random(self.kernel_seed + index),
                                                                      np.random.RandomState(self.kernel_seed + index))
        if self.sinc_prob > 0 and rng[1].uniform() < self.sinc_prob:
            kernel = circular_lowpass_kernel(rng[1].uniform(math.pi / 3, math.pi), self.K)
        else:
            kernel = random_mixed_kernels(self.kernel_list, self.kernel_prob, self.K, self.blur_sigma, self.blur_sigma, [-math.pi, math.pi],
                                          self.betag_range, self.betap_range, noise_range=None, rng=rng)
        return torch.from_numpy(kernel.astype(np.float32))

    def __getitem__(self, index):
        gt, path = self._gt(index)
        if min(gt.shape[1:]) <= self.K // 2:
            raise ValueError(f"the image {path} of {tuple(gt.shape[1:])} must exceed blur_kernel_size // 2 = {self.K // 2} in both directions")
        kernel = self.blur_kernel(index)
        sample = {"gt": gt, "lq_path": path, "gt_path": path}
        if self.backend == "device":
            sample["blur_kernel"] = kernel
        else:
            sample["lq"] = filter2d_host(gt, kernel)
        return _labelled(sample, self.opt)


@DATASET_REGISTRY.register()
class RealESRGANDataset(_GTFolderDataset):
    """GT folder + the three blur kernels of the second-order degradation chain (Real-ESRGAN's data set): the sample carries ``gt``,
    ``kernel1``, ``kernel2``, ``sinc_kernel`` (21 x 21 fp32 each) and the paths, and no ``lq``; the model's ``feed_data`` makes ``lq`` on the
    device with ``basicsr.data.degradations.apply_second_order`` from the options of its ``degradation:`` block.  Options: ``dataroot_gt``,
    ``gt_size`` (default 128), ``use_hflip``, ``use_rot``, ``center_crop``; ``kernel_list`` / ``kernel_prob``, ``blur_sigma``,
    ``betag_range``, ``betap_range``, ``sinc_prob`` and their ``*2`` forms for the second kernel (defaults: those of
    PairedImageBlurDataset, a ``*2`` option defaulting to its first-order value); ``final_sinc_prob`` (default 0.8); ``kernel_seed``.

    ``kernel1`` / ``kernel2``: a size from the odd numbers 7..21 (``random.choice``); with ``sinc_prob`` (one ``uniform`` of ``np.random``)
    ``circular_lowpass_kernel(w, size, pad_to=21)`` with w uniform in [pi / 3, pi] for a size below 13 and in [pi / 5, pi] otherwise, else
    ``random_mixed_kernels(kernel_list, kernel_prob, size, blur_sigma, blur_sigma, [-pi, pi], betag_range, betap_range, noise_range=None)``
    zero-padded to 21.  ``sinc_kernel``: with ``final_sinc_prob`` ``circular_lowpass_kernel(uniform(pi / 3, pi), size, pad_to=21)`` for
    another size of that list, else the unit pulse at the centre.  ``kernel_seed`` as for PairedImageBlurDataset: image ``index`` draws
    from generators of its own.  These samples form batches of their own kind: ``degrade_collate`` refuses them in a mixed batch."""

    K = 21
    SIZES = tuple(range(7, 22, 2))

    def __init__(self, opt):
        super().__init__(opt)
        blur = PairedImageBlurDataset
        self.first, self.second = {}, {}
        for cfg, sfx in ((self.first, ""), (self.second, "2")):
            base = {} if sfx == "" else self.first
            cfg["kernel_list"] = list(opt.get("kernel_list" + sfx, base.get("kernel_list", blur.KINDS)))
            n = len(cfg["kernel_list"])
            cfg["kernel_prob"] = list(opt.get("kernel_prob" + sfx, base.get("kernel_prob", [1.0 / n] * n)))
            if not cfg["kernel_list"] or not set(cfg["kernel_list"]) <= set(blur.KINDS):
                raise ValueError(f"kernel_list{sfx} holds kinds of {blur.KINDS}, got {cfg['kernel_list']}")
            if len(cfg["kernel_prob"]) != n or min(cfg["kernel_prob"]) < 0 or sum(cfg["kernel_prob"]) <= 0:
                raise ValueError(f"kernel_prob{sfx} must hold one non-negative weight per entry of kernel_list{sfx}, got {cfg['kernel_prob']}")
            for key, default in (("blur_sigma", [0.2, 3]), ("betag_range", [0.5, 4]), ("betap_range", [1, 2])):
                cfg[key] = blur._range(opt, key + sfx, base.get(key, default))
            cfg["sinc_prob"] = float(opt.get("sinc_prob" + sfx, base.get("sinc_prob", 0)))
        self.final_sinc_prob = float(opt.get("final_sinc_prob", 0.8))
        for name, p in (("sinc_prob", self.first["sinc_prob"]), ("sinc_prob2", self.second["sinc_prob"]), ("final_sinc_prob", self.final_sinc_prob)):
            if not 0 <= p <= 1:
                raise ValueError(f"{name} must lie in [0, 1], got {p}")
        self.kernel_seed = opt.get("kernel_seed")
        if opt.get("phase") == "train" and self.gt_size <= self.K // 2:
            raise ValueError(f"gt_size {self.gt_size} must exceed {self.K // 2}, the reflect padding of the {self.K} x {self.K} blur")

    def _padded(self, kernel):
        pad = (self.K - kernel.shape[0]) // 2
        return torch.from_numpy(np.pad(kernel, ((pad, pad), (pad, pad))).astype(np.float32))

    def _blur_kernel(self, rng, cfg):
        import math

        from basicsr.data.degradations import circular_lowpass_kernel, random_mixed_kernels

        size = rng[0].choice(self.SIZES)
        if rng[1].uniform() < cfg["sinc_prob"]:
            kernel = circular_lowpass_kernel(rng[1].uniform(math.pi / 3 if size < 13 else math.pi / 5, math.pi), size)
        else:
            kernel = random_mixed_kernels(cfg["kernel_list"], cfg["kernel_prob"], size, cfg["blur_sigma"], cfg["blur_sigma"], [-math.pi, math.pi],
                                          cfg["betag_range"], cfg["betap_range"], noise_range=None, rng=rng)
        return self._padded(kernel)

    def kernels(self, index):
        """``(kernel1, kernel2, sinc_kernel)`` of image ``index``: its own generators under ``kernel_seed``, the process-wide ones otherwise"""
        import math
        import random

        from basicsr.data.degradations import circular_lowpass_kernel

        rng = (random, np.random) if self.kernel_seed is None else (random.Random(self.kernel_seed + index),
                                                                      np.random.RandomState(self.kernel_seed + index))
        kernel1, kernel2 = self._blur_kernel(rng, self.first), self._blur_kernel(rng, self.second)
        if rng[1].uniform() < self.final_sinc_prob:
            sinc = self._padded(circular_lowpass_kernel(rng[1].uniform(math.pi / 3, math.pi), rng[0].choice(self.SIZES)))
        else:
            sinc = torch.zeros(self.K, self.K)
            sinc[self.K // 2, self.K // 2] = 1.0
        return kernel1, kernel2, sinc

    def __getitem__(self, index):
        gt, path = self._gt(index)
        if min(gt.shape[1:]) <= self.K // 2:
            raise ValueError(f"the image {path} of {tuple(gt.shape[1:])} must exceed {self.K // 2} pixels in both directions")
        kernel1, kernel2, sinc = self.kernels(index)
        return _labelled({"gt": gt, "kernel1": kernel1, "kernel2": kernel2, "sinc_kernel": sinc, "lq_path": path, "gt_path": path}, self.opt)


@DATASET_REGISTRY.register()
class PairedImageDehazeDataset(tdata.Dataset):
    """Hazy folder + GT folder with several hazy images per GT (reference basicsr/data/paired_image_dataset.py:583-729, folder mode, PIL
    reader): the LQ folder is listed, and the GT of ``<lq_name>`` is ``dataroot_gt/<lq_name.split("_")[0] + suffix>`` (``suffix`` default
    ``.jpg``; SOTS: ``0001_0.8_0.2.jpg`` -> ``0001.png`` with ``suffix: .png``).  Train phase = paired random crop at scale 1 + flips /
    rotation, other phases = optional ``center_crop``.  One departure from the reference: ``lq_path`` is the real LQ path (the reference
    returns the GT path under both keys, so the saved validation images of one GT overwrite each other)."""

    def __init__(self, opt):
        super().__init__()
        self.opt = opt
        self.gt_root, self.lq_root = opt["dataroot_gt"], opt["dataroot_lq"]
        self.suffix = opt.get("suffix", ".jpg")
        self.names = sorted(f for f in scandir(self.lq_root) if f.endswith(_IMG_EXT))

    def __len__(self):
        return len(self.names)

    def __getitem__(self, index):
        name = self.names[index]
        lq_path = osp.join(self.lq_root, name)
        gt_path = osp.join(self.gt_root, osp.basename(name).split("_")[0] + self.suffix)
        lq, gt = _read_rgb(lq_path), _read_rgb(gt_path)
        if self.opt.get("phase") == "train":
            lq, gt = paired_random_crop_augment(lq, gt, {**self.opt, "scale": 1})
        elif self.opt.get("center_crop") is not None:
            lq, gt = _center_crop(lq, self.opt["center_crop"]), _center_crop(gt, self.opt["center_crop"])
        return _labelled({"lq": lq, "gt": gt, "lq_path": lq_path, "gt_path": gt_path}, self.opt)


# which key makes a sample which kind of a mixed batch (``degrade_kind``), and the keys that kind brings along
DEGRADE_KINDS = (("lq", ("lq",)), ("noise_sigma", ("noise_sigma", "noise_key")), ("jpeg_quality", ("jpeg_quality",)), ("mosaic", ("mosaic",)),
                 ("inpaint_meta", ("inpaint_lines", "inpaint_meta")), ("blur_kernel", ("blur_kernel",)))


def degrade_collate(samples):
    """``collate_fn`` of the train loader.  Samples with identical key sets -- every batch of a single data set -- give exactly
    ``default_collate(samples)``.  A batch of a ``ConcatDataset`` over sets with different device backends mixes samples that carry
    different keys, which the default collate refuses; it is collated as: the keys common to all samples (``gt``, the paths,
    ``dataset_idx``) as usual; ``degrade_kind``, an int32 ``[B]`` host tensor: 0 the sample has ``lq``, 1 ``noise_sigma``, 2
    ``jpeg_quality``, 3 ``mosaic``, 4 ``inpaint_meta``, 5 ``blur_kernel``; and each kind's own keys (``lq`` included) stacked over THAT KIND'S samples in
    batch order.  ``BaseModel._lq_on_device`` makes the ``lq`` rows of each kind from its ``gt`` rows.  Poisson-noise samples
    (``noise_type: poisson``: ``poisson_scale``, ``poisson_gray``, ``noise_key``) are none of the six kinds: they collate among themselves
    and are refused in a mixed batch."""
    from torch.utils.data import default_collate

    keys = set(samples[0].keys())
    if all(set(s.keys()) == keys for s in samples[1:]):
        return default_collate(samples)
    kinds = []
    for s in samples:
        kind = [k for k, (key, _) in enumerate(DEGRADE_KINDS) if key in s]
        if len(kind) != 1:
            raise ValueError(f"a sample of a mixed batch carries exactly one of {[key for key, _ in DEGRADE_KINDS]}; got the keys "
                             f"{sorted(s.keys())}")
        kinds.append(kind[0])
    shapes = sorted({tuple(s["gt"].shape) for s in samples})
    if len(shapes) != 1:
        raise ValueError(f"the samples of a mixed batch have gt of different sizes {shapes}: give every train set the same gt_size")
    ksizes = sorted({tuple(s["blur_kernel"].shape) for s in samples if "blur_kernel" in s})
    if len(ksizes) > 1:
        raise ValueError(f"the blur samples of a mixed batch have kernels of different sizes {ksizes}: give every blur train set the same "
                         "blur_kernel_size")
    own = {k for _, ks in DEGRADE_KINDS for k in ks}
    common = set.intersection(*(set(s.keys()) for s in samples)) - own
    loose = set.union(*(set(s.keys()) for s in samples)) - own - common
    if loose:
        raise ValueError(f"the keys {sorted(loose)} are carried by some samples of a mixed batch only")
    batch = default_collate([{k: s[k] for k in s if k in common} for s in samples])
    batch["degrade_kind"] = torch.tensor(kinds, dtype=torch.int32)
    for kind, (_, ks) in enumerate(DEGRADE_KINDS):
        rows = [s for s, kd in zip(samples, kinds) if kd == kind]
        if rows:
            batch.update(default_collate([{k: s[k] for k in ks} for s in rows]))
    return batch


def build_dataset(dataset_opt):
    dataset_opt = deepcopy(dataset_opt)
    logger = get_root_logger()
    root = dataset_opt.get("dataroot_gt")
    if dataset_opt["type"] != "SyntheticPairedDataset" and (root is None or not osp.isdir(root)):
        if dataset_opt.get("phase") == "train" and not dataset_opt.get("allow_synthetic", False):
            raise FileNotFoundError(f"Dataset root {root} of the training set [{dataset_opt.get('name')}] does not exist "
                                    "(set `allow_synthetic: true` in the dataset options to train on seeded synthetic pairs)")
        logger.warning(f"Dataset root {root} of [{dataset_opt.get('name')}] not found: using a seeded synthetic pair instead.")
        dataset = SyntheticPairedDataset(dataset_opt)
    else:
        dataset = DATASET_REGISTRY.get(dataset_opt["type"])(dataset_opt)
    logger.info(f"Dataset [{dataset.__class__.__name__}] - {dataset_opt['name']} is built.")
    return dataset


def build_dataloader(dataset, dataset_opt, num_gpu=1, dist=False, sampler=None, seed=None):
    phase = dataset_opt.get("phase", "test")
    if phase in ("val", "test"):
        return tdata.DataLoader(dataset, batch_size=1, shuffle=False, num_workers=0)
    if phase == "train":  # reference basicsr/data/__init__.py:64-92: per-GPU batch, sampler-driven order, drop_last
        workers = dataset_opt.get("num_worker_per_gpu", 0) * (1 if dist else max(1, num_gpu))
        batch = dataset_opt["batch_size_per_gpu"] * (1 if dist else max(1, num_gpu))
        rank = torch.distributed.get_rank() if dist else 0

        def worker_init(worker_id):
            import random

            s = (seed or 0) + workers * rank + worker_id
            np.random.seed(s)
            random.seed(s)

        return tdata.DataLoader(dataset, batch_size=batch, shuffle=sampler is None, sampler=sampler, num_workers=workers,
                                drop_last=True, worker_init_fn=worker_init if seed is not None else None, collate_fn=degrade_collate,
                                pin_memory=dataset_opt.get("pin_memory", False), persistent_workers=False)
    raise ValueError(f"Wrong dataset phase: {phase}. Supported ones are 'train', 'val' and 'test'.")
