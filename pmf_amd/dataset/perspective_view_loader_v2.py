"""EPMF perspective-view loader on MI355X (pc_processor/dataset/perspective_view_loader_v2.py:9-163).

Same constructor / item contract as the reference for the deterministic paths.  The yaw-cropped float64 projection
(parser.py:229-257), the order-preserving compaction, the bounding box, the last-writer-wins scatter and the RGB window
are HIP kernels (pmf_project_v2_index / pmf_project_v2_scatter); the frame size is data dependent, so one scalar read
(kept count + bounding box) separates the two passes, exactly where the reference computes min / max on the host.
``dataset`` duck type: loadDataByIndex, loadImage, parsePathInfoByIndex, proj_matrix[seq], class_map_lut and
optionally fov_left / fov_right (defaults: +-45 degrees, parser.py:36-37).
Training path (:25-34,50-57,142-153): random image rescale in [1, 1.2] (numpy RNG draw, PIL bilinear resize on the host
as in the reference), coordinates scaled with it inside the projection kernel, bottom / centred horizontal zero padding
to (proj_ht, proj_wt), then flip / rotate(15) / crop as one HIP gather (FlipRotateCrop).  img_aug (:19-23,46-47,
ColorJitter(*PVconfig.img_jitter) before the rescale) runs on the device (perspective_view_loader.ColorJitter ->
pmf_color_jitter, bit-exact Pillow arithmetic); the jittered uint8 frame comes back once for the host-side PIL resize.
A ``NuscenesV2``-type dataset -- one with ``mapLidar2CameraCropYaw(seq_id, pointcloud) -> (camera-frame rows f[K, >=4],
(row, col) f64[K,2], keep bool[P])`` and no ``proj_matrix`` -- keeps its geometry on the host (the devkit's chain of rigid
transforms, dataset_nuscenes_v2.py:301-375); what the loader does with the result (:72-141: truncation, bounding box, depth
of the camera-frame points, last-writer-wins scatter, labelMapping as a 256-entry table, RGB window) is one packed upload +
pmf_project_v2_scatter.  Validation only: the training path on such a dataset is not implemented.
A dataset with ``projectDevice(index, image_dev, img_scale) -> (proj, xy_index, depth, keep, extra)`` and
``loadImageDevice(index)`` (A2D2_PV: pixel coordinates come with the frame, every point is kept; NuscenesV2Native:
pmf_nus_project in front of the scatter) is served in all three
layouts -- training, validation, return_uproj -- and by _eval_item: image on the device, ColorJitter, the same rescale draw
and host resize as above, the dataset's own projection, then the common pad / crop tail (:42-157).  That check comes first."""
import ctypes as C
import math

import numpy as np
import torch
from torch.utils.data import Dataset

from .. import _lib as L


def project_frame_v2_gpu(points, sem_label, image_u8, proj_matrix, label_lut, fov_left, fov_right, device="cuda",
                         img_scale=1.0):
    """-> (proj f32[10,h,w], xy_index f64[K,2], depth f32[K], keep bool[P]) on `device`; img_scale multiplies the
    projected (row, col) coordinates (the caller passes the image already rescaled by it)."""
    return _project_frame_v2(points, sem_label, image_u8, proj_matrix, label_lut, fov_left, fov_right, device,
                             img_scale)[:4]


def _project_frame_v2(points, sem_label, image_u8, proj_matrix, label_lut, fov_left, fov_right, device="cuda",
                      img_scale=1.0):
    """project_frame_v2_gpu + a dict of the device tensors the evaluation post path reads (postproc/frame_eval.py):
    x_data / y_data int32[K] (truncated row / column), src int32[K] (source index of each kept point), sem int32[P],
    lut int32, and the box corner x_min / y_min (host ints)."""
    lib = L.lib()
    dev = torch.device(device)
    from .perspective_view_loader import image_to_device
    pts = points.to(dev, torch.float32).contiguous() if isinstance(points, torch.Tensor) else \
        torch.as_tensor(np.ascontiguousarray(points, np.float32)).to(dev)
    sem = sem_label.to(dev, torch.int32).contiguous() if isinstance(sem_label, torch.Tensor) else \
        torch.as_tensor(np.ascontiguousarray(sem_label, np.int32)).to(dev)
    img = image_to_device(image_u8, dev)
    mat = torch.as_tensor(np.ascontiguousarray(proj_matrix, np.float64).reshape(12)).to(dev)
    lut = torch.as_tensor(np.ascontiguousarray(label_lut, np.int32)).to(dev)
    P = pts.shape[0]
    n = max(P, 1)
    keep = torch.empty(n, dtype=torch.uint8, device=dev)
    src = torch.empty(n, dtype=torch.int32, device=dev)
    xd = torch.empty(n, dtype=torch.int32, device=dev)
    yd = torch.empty(n, dtype=torch.int32, device=dev)
    xy = torch.empty((n, 2), dtype=torch.float64, device=dev)
    depth = torch.empty(n, dtype=torch.float32, device=dev)
    meta = torch.zeros(5, dtype=torch.int32, device=dev)          # n_kept, row_min, row_max, col_min, col_max
    blk = torch.empty((P + 1023) // 1024 + 1, dtype=torch.int32, device=dev)
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    L.check(lib.pmf_project_v2_index_scaled(pts.data_ptr(), P, mat.data_ptr(), float(fov_left), float(fov_right),
                                     float(img_scale), keep.data_ptr(), src.data_ptr(), xd.data_ptr(), yd.data_ptr(), xy.data_ptr(),
                                     depth.data_ptr(), meta.data_ptr(), meta.data_ptr() + 4, blk.data_ptr(), st),
            "pmf_project_v2_index_scaled")
    k, x_min, x_max, y_min, y_max = [int(v) for v in meta.tolist()]    # the one host read (frame size is data)
    if k == 0:
        raise ValueError("PerspectiveViewLoaderV2: no point inside the yaw field of view")
    h, w = x_max - x_min + 1, y_max - y_min + 1
    out = torch.empty((10, h, w), dtype=torch.float32, device=dev)
    pix = torch.empty(h * w, dtype=torch.int32, device=dev)
    L.check(lib.pmf_project_v2_scatter(pts.data_ptr(), sem.data_ptr(), src.data_ptr(), xd.data_ptr(), yd.data_ptr(),
                                       depth.data_ptr(), k, img.data_ptr(), img.shape[0], img.shape[1], lut.data_ptr(),
                                       lut.shape[0], x_min, y_min, h, w, out.data_ptr(), pix.data_ptr(), st),
            "pmf_project_v2_scatter")
    extra = dict(x_data=xd[:k], y_data=yd[:k], src=src[:k], sem=sem, lut=lut, x_min=x_min, y_min=y_min)
    return out, xy[:k], depth[:k], keep[:P].bool(), extra


class PerspectiveViewLoaderV2(Dataset):
    def __init__(self, dataset, config, data_len=-1, is_train=True, img_aug=False, return_uproj=False, device="cuda"):
        self.dataset, self.config = dataset, config
        self.is_train, self.img_aug, self.data_len = is_train, img_aug, data_len
        self.pv_config = config["PVconfig"]
        self.return_uproj, self.device = return_uproj, device
        self.img_jitter = None
        if img_aug:                       # :19-23 (the reference jitters whenever img_aug is set, train or not)
            from .perspective_view_loader import ColorJitter
            self.img_jitter = ColorJitter(*self.pv_config["img_jitter"])
        self.aug_ops = None
        if is_train:                      # :25-34 flip / rotate(15) / crop to (proj_ht, proj_wt) as one HIP gather
            from .perspective_view_loader import FlipRotateCrop
            self.aug_ops = FlipRotateCrop(self.pv_config["proj_ht"], self.pv_config["proj_wt"])
        self._nus_lut = self._ident = None            # NuscenesV2-type datasets: label table, identity source indices

    def _has_project_device(self):
        return hasattr(self.dataset, "projectDevice")

    def _device_frame(self, index, train):
        """a dataset with projectDevice: -> (proj, xy_index, depth, keep, extra); the draws and their order are those of the
        SemanticKITTI path (jitter, then the rescale when ``train``)"""
        dev = torch.device(self.device)
        if dev.type != "cuda":
            raise RuntimeError("PerspectiveViewLoaderV2 runs on the GPU only (device=%s)" % self.device)
        image = self.dataset.loadImageDevice(index)
        if self.img_jitter is not None:
            image = self.img_jitter(image)
        img_scale = 1.0
        if train:
            from PIL import Image               # :50-57, as below: numpy's global RNG, PIL's bilinear resize on the host
            image = Image.fromarray(image.cpu().numpy())
            img_w, img_h = image.size
            img_scale = np.random.uniform(low=1.0, high=1.2)
            image = np.asarray(image.resize((int(img_w * img_scale), int(img_h * img_scale)), Image.BILINEAR))
        return self.dataset.projectDevice(index, image, img_scale)

    def _tail(self, proj):
        """:142-157 bottom / centred horizontal zero padding, then flip / rotate / crop (training) or the centre crop"""
        ch, cw = (self.pv_config["proj_ht"], self.pv_config["proj_wt"]) if self.is_train else \
            (self.pv_config["proj_h"], self.pv_config["proj_w"])
        _, h, w = proj.shape
        mh, mw = max(ch, h), max(cw, w)
        left = (mw - w) // 2
        padded = torch.nn.functional.pad(proj, (left, mw - w - left, 0, mh - h))
        if self.is_train:
            return self.aug_ops(padded)
        top, lft = int(round((mh - ch) / 2.0)), int(round((mw - cw) / 2.0))
        return padded[:, top:top + ch, lft:lft + cw].contiguous()

    def _is_nus_v2(self):
        return hasattr(self.dataset, "mapLidar2CameraCropYaw") and not hasattr(self.dataset, "proj_matrix")

    def _nus_label_lut(self):
        """dataset.labelMapping (np.vectorize over a dictionary) as a 256-entry table, as NusPerspectiveViewLoader"""
        if self._nus_lut is None:
            keys = sorted(self.dataset.map_name_from_general_index_to_segmentation_index.keys())
            lut = np.zeros(256, np.int32)
            lut[keys] = self.dataset.labelMapping(np.asarray(keys, np.uint8)[:, None])
            self._nus_lut = torch.from_numpy(lut).to(self.device)
        return self._nus_lut

    def _nus_item(self, index):
        """one camera view of a NuscenesV2-type dataset -> (proj, xy_index, depth, keep, extra, pointcloud)"""
        if self.is_train:
            raise NotImplementedError("PerspectiveViewLoaderV2: training (is_train=True) on a NuscenesV2-type dataset "
                                      "(mapLidar2CameraCropYaw, no proj_matrix) is not implemented; use is_train=False")
        dev = torch.device(self.device)
        if dev.type != "cuda":
            raise RuntimeError("PerspectiveViewLoaderV2 runs on the GPU only (device=%s)" % self.device)
        from .perspective_view_loader import image_to_device, upload_packed
        image = self.dataset.loadImage(index)
        img_dev = None
        if self.img_jitter is not None:
            img_dev = self.img_jitter(image_to_device(image, dev))
        pointcloud, sem_label, _ = self.dataset.loadDataByIndex(index)
        seq_id, _ = self.dataset.parsePathInfoByIndex(index)
        crop, xy_index, keep_mask = self.dataset.mapLidar2CameraCropYaw(seq_id, pointcloud)
        xy_index = np.ascontiguousarray(xy_index, np.float64)
        keep_mask = np.asarray(keep_mask, np.bool_)
        K = int(xy_index.shape[0])
        if K == 0:
            raise ValueError("PerspectiveViewLoaderV2: no point inside the camera's field of view")
        x_data = np.ascontiguousarray(xy_index[:, 0].astype(np.int32))
        y_data = np.ascontiguousarray(xy_index[:, 1].astype(np.int32))
        x_min, x_max, y_min, y_max = int(x_data.min()), int(x_data.max()), int(y_data.min()), int(y_data.max())
        h, w = x_max - x_min + 1, y_max - y_min + 1
        # depth of the CAMERA-frame points, in the precision the dataset hands them over (:97); it is one of the scatter's
        # inputs and the coordinates are host arrays, so it is taken here and travels with the packed upload
        depth = np.linalg.norm(crop[:, :3], 2, axis=1).astype(np.float32)
        sem_raw = np.ascontiguousarray(sem_label).reshape(-1).astype(np.int32)
        parts = [np.ascontiguousarray(crop[:, :4], np.float32), sem_raw[keep_mask], x_data, y_data, depth,
                 np.flatnonzero(keep_mask).astype(np.int32), sem_raw, xy_index, keep_mask.view(np.uint8)]
        if img_dev is None:
            parts.append(np.ascontiguousarray(np.asarray(image), np.uint8))
        up = upload_packed(parts, dev)                       # one host -> device copy per view
        pts, sem_kept, xd, yd, dep, src, sem, xy, keep = up[:9]
        img = img_dev if img_dev is not None else up[9]
        if self._ident is None or self._ident.shape[0] < K:  # row k of the cropped cloud is its own source
            self._ident = torch.arange(max(K, 1 << 16), dtype=torch.int32, device=dev)
        lut = self._nus_label_lut()
        out = torch.empty((10, h, w), dtype=torch.float32, device=dev)
        pix = torch.empty(h * w, dtype=torch.int32, device=dev)
        st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        L.check(L.lib().pmf_project_v2_scatter(pts.data_ptr(), sem_kept.data_ptr(), self._ident.data_ptr(), xd.data_ptr(),
                                               yd.data_ptr(), dep.data_ptr(), K, img.data_ptr(), img.shape[0], img.shape[1],
                                               lut.data_ptr(), lut.shape[0], x_min, y_min, h, w, out.data_ptr(),
                                               pix.data_ptr(), st), "pmf_project_v2_scatter")
        extra = dict(x_data=xd, y_data=yd, src=src, sem=sem, lut=lut, x_min=x_min, y_min=y_min)
        return out, xy, dep, keep.bool(), extra, pointcloud

    def __getitem__(self, index):
        if self._has_project_device():
            proj, xy, depth, keep, _ = self._device_frame(index, self.is_train)
            if self.return_uproj:
                return proj, xy, depth, keep, torch.as_tensor(np.asarray(self.dataset.loadPointcloud(index)))
            return self._tail(proj)
        if self._is_nus_v2():
            proj, xy, depth, keep, _, pointcloud = self._nus_item(index)
            if not self.return_uproj:
                raise NotImplementedError("PerspectiveViewLoaderV2 on a NuscenesV2-type dataset serves the evaluation "
                                          "layout only (return_uproj=True, is_train=False)")
            return proj, xy, depth, keep, torch.as_tensor(np.asarray(pointcloud))
        image = self.dataset.loadImage(index)
        if self.img_jitter is not None:
            from .perspective_view_loader import image_to_device
            image = self.img_jitter(image_to_device(image, self.device))
            if self.is_train:
                image = image.cpu().numpy()           # the rescale below is PIL's (host), as in the reference
        img_scale = 1.0
        if self.is_train:
            # :50-57 random rescale of the camera image: numpy's global RNG, PIL's bilinear resize (what
            # torchvision's Resize calls for a PIL image) -- host image decoding side, as in the reference
            from PIL import Image
            if not isinstance(image, Image.Image):
                image = Image.fromarray(np.asarray(image))
            img_w, img_h = image.size
            img_scale = np.random.uniform(low=1.0, high=1.2)
            image = image.resize((int(img_w * img_scale), int(img_h * img_scale)), Image.BILINEAR)
        if not isinstance(image, torch.Tensor):
            image = np.asarray(image)
        pointcloud, sem_label, _ = self.dataset.loadDataByIndex(index)
        seq_id, _ = self.dataset.parsePathInfoByIndex(index)
        fl = getattr(self.dataset, "fov_left", -45 / 180.0 * math.pi)
        fr = getattr(self.dataset, "fov_right", 45 / 180.0 * math.pi)
        if not self.return_uproj and not isinstance(image, torch.Tensor) and not isinstance(pointcloud, torch.Tensor):
            from .perspective_view_loader import upload_packed     # one host -> device copy per frame
            pointcloud, sem_label, image = upload_packed(
                [np.asarray(pointcloud, np.float32), np.asarray(sem_label, np.int32), np.ascontiguousarray(image, np.uint8)],
                self.device)
        proj, xy, depth, keep = project_frame_v2_gpu(pointcloud, sem_label, image, self.dataset.proj_matrix[seq_id],
                                                     self.dataset.class_map_lut, fl, fr, self.device, img_scale)
        if self.return_uproj:
            return proj, xy, depth, keep, torch.as_tensor(np.asarray(pointcloud))
        return self._tail(proj)

    def _eval_item(self, index):
        """validation frame for the evaluation task (return_uproj layout): (proj, xy_index, depth, keep, extra) with
        ``extra`` the device tensors of _project_frame_v2; the public return tuple of __getitem__ is unchanged.  On a
        NuscenesV2-type dataset ``src`` is the position of each kept point in the sweep and ``sem`` the sweep's raw labels."""
        if self._has_project_device():
            return self._device_frame(index, False)
        if self._is_nus_v2():
            return self._nus_item(index)[:5]
        image = self.dataset.loadImage(index)
        if self.img_jitter is not None:
            from .perspective_view_loader import image_to_device
            image = self.img_jitter(image_to_device(image, self.device))
        if not isinstance(image, torch.Tensor):
            image = np.asarray(image)
        pointcloud, sem_label, _ = self.dataset.loadDataByIndex(index)
        seq_id, _ = self.dataset.parsePathInfoByIndex(index)
        fl = getattr(self.dataset, "fov_left", -45 / 180.0 * math.pi)
        fr = getattr(self.dataset, "fov_right", 45 / 180.0 * math.pi)
        return _project_frame_v2(pointcloud, sem_label, image, self.dataset.proj_matrix[seq_id],
                                 self.dataset.class_map_lut, fl, fr, self.device)

    def __len__(self):
        if 0 < self.data_len < len(self.dataset):
            return self.data_len
        return len(self.dataset)
