"""SalsaNext range-image loader on MI355X -- pc_processor/dataset/salsanext_loader.py:7-89.

Same constructor / item contract as the reference: (proj_feature [5,H,W], proj_sem_label [H,W], proj_mask [H,W]) and,
with return_uproj, (+ proj_range, uproj_x, uproj_y, uproj_depth).  The sweep goes to the GPU once; augmentation
(pmf_points_transform), projection (pmf_range_project_index) and the tensor assembly incl. normalisation and label
lookup (pmf_range_project_gather) are HIP kernels, and the item stays on the device -- feed it to SalsaNext directly.
``dataset`` duck type: loadDataByIndex(i) -> (pointcloud [P,4], sem_label [P], inst_label), labelMapping(labels).
Evaluation (tasks/salsanext_eval_nuscenes) uses _eval_item: the same item plus the raw per-point ids and the label table on
the device, from ONE loadDataByIndex call."""
import numpy as np
import torch
from torch.utils.data import Dataset

from .preprocess import augmentor, projection


class SalsaNextLoader(Dataset):
    def __init__(self, dataset, config, data_len=-1, is_train=True, return_uproj=False, device="cuda", label_lut=None):
        """label_lut: the raw id -> class table _eval_item scores with, whole (SemanticKITTI's moving classes have raw ids
        up to 259); None = the 256-entry table _label_lut builds from the dataset"""
        self.dataset, self.config = dataset, config
        self.is_train, self.data_len, self.return_uproj = is_train, data_len, return_uproj
        self.device = torch.device(device)
        if self.is_train:
            a = self.config["augmentation"]
            params = augmentor.AugmentParams()
            params.setFlipProb(p_flipx=a["p_flipx"], p_flipy=a["p_flipy"])
            params.setTranslationParams(**{k: a[k] for k in a if "trans" in k})
            params.setRotationParams(**{k: a[k] for k in a if "rot" in k})
            self.augmentor = augmentor.Augmentor(params, device=self.device)
        else:
            self.augmentor = None
        s = self.config["sensor"]
        self.projection = projection.RangeProjection(fov_up=s["fov_up"], fov_down=s["fov_down"], fov_left=s["fov_left"],
                                                     fov_right=s["fov_right"], proj_h=s["proj_h"], proj_w=s["proj_w"],
                                                     device=self.device)
        self.proj_img_mean = torch.tensor(s["img_mean"], dtype=torch.float)
        self.proj_img_stds = torch.tensor(s["img_stds"], dtype=torch.float)
        self._mean_dev = self._stds_dev = None
        self._lut = None
        if label_lut is not None:
            t = np.ascontiguousarray(np.asarray(label_lut).reshape(-1), np.int32)
            if t.shape[0] < 1:
                raise ValueError("label_lut is empty")
            self._lut = torch.from_numpy(t).to(self.device)

    def _label_lut(self):
        """int32[256] on the device: raw id -> class.  The dataset's map_name_from_general_index_to_segmentation_index (nuScenes)
        or class_map_lut table when it has one, else labelMapping evaluated once on all 256 ids."""
        if self._lut is None:
            ds = self.dataset
            lut = np.zeros(256, np.int32)
            table = getattr(ds, "map_name_from_general_index_to_segmentation_index", None)
            if table is not None:
                keys = sorted(k for k in table if 0 <= int(k) < 256)
                lut[keys] = [int(table[k]) for k in keys]
            elif getattr(ds, "class_map_lut", None) is not None:
                t = np.asarray(ds.class_map_lut).astype(np.int32).reshape(-1)[:256]
                lut[:t.shape[0]] = t
            else:
                lut[:] = np.asarray(ds.labelMapping(np.arange(256, dtype=np.uint8)[:, None])).reshape(-1)
            self._lut = torch.from_numpy(lut).to(self.device)
        return self._lut

    def _eval_item(self, index):
        """evaluation item (is_train=False): dict(feature f32[5,H,W], label f32[H,W], mask i32[H,W], proj_range f32[H,W],
        px / py int32[P] (column / row), depth f32[P], sem int32[P] raw ids, lut int32[256] or the constructor's
        label_lut), all on the device.  One loadDataByIndex call and no host label pass: the raw ids go to the device once and the pixel labels are
        lut[sem] there (the reference's loop loads every sweep a second time for its point labels)."""
        pointcloud, sem_label, _ = self.dataset.loadDataByIndex(index)
        pts = self.projection.to_device(pointcloud)
        raw = sem_label if isinstance(sem_label, torch.Tensor) else torch.from_numpy(
            np.ascontiguousarray(np.asarray(sem_label).reshape(-1)).astype(np.int32))
        sem = raw.reshape(-1).to(self.device, torch.int32)
        lut = self._label_lut()
        idx = sem.long()
        inside = (idx >= 0) & (idx < lut.shape[0])
        mapped = torch.where(inside, lut[idx.clamp(0, lut.shape[0] - 1)], torch.zeros_like(sem))   # outside the table: class 0,
        #                                                                                    the rule of the point stage
        if self._mean_dev is None:
            self._mean_dev = self.proj_img_mean.to(self.device)
            self._stds_dev = self.proj_img_stds.to(self.device)
        feat, label, mask, rng = self.projection.loader_item(pts, mapped, self._mean_dev, self._stds_dev)
        c = self.projection.cached_data
        return dict(feature=feat, label=label, mask=mask, proj_range=rng, px=c["uproj_x_idx"], py=c["uproj_y_idx"],
                    depth=c["uproj_depth"], sem=sem, lut=lut)

    def __getitem__(self, index):
        pointcloud, sem_label, inst_label = self.dataset.loadDataByIndex(index)
        pts = self.projection.to_device(pointcloud)
        if self.is_train:
            pts = self.augmentor.doAugmentation(pts.clone() if isinstance(pointcloud, torch.Tensor) else pts)
        mapped = self.dataset.labelMapping(sem_label)
        mapped = torch.as_tensor(np.ascontiguousarray(mapped).astype(np.int32)) if not isinstance(mapped, torch.Tensor) \
            else mapped
        if self._mean_dev is None:
            self._mean_dev = self.proj_img_mean.to(self.device)
            self._stds_dev = self.proj_img_stds.to(self.device)
        feat, label, mask, rng = self.projection.loader_item(pts, mapped, self._mean_dev, self._stds_dev)
        if self.return_uproj:
            c = self.projection.cached_data
            return feat, label, mask, rng, c["uproj_x_idx"].long(), c["uproj_y_idx"].long(), c["uproj_depth"]
        return feat, label, mask

    def __len__(self):
        if 0 < self.data_len < len(self.dataset):
            return self.data_len
        return len(self.dataset)
