"""Point-wise inference on nuScenes: six camera views per LiDAR sweep, merged by confidence (counterpart of the reference's
tasks/pmf_eval_nuscenes/infer.py:18-330).

Per view (:110-170): the view's projection frame (NusPerspectiveViewLoader) -> drop the top rows down to sensor.proj_h ->
normalise * mask -> PMFNet (HIP plan, eval) -> zero-pad back -> per-pixel confidence / argmax -> labels of the points the
camera sees, read at their pixel or voted by the KNN post-processing -> kept together with the points' sweep indices and
confidences.  After the sixth view (:171-200): getMergePred (per point the label of the most confident camera, HIP:
pmf_merge_pred) -- with a LiDAR-only SalsaNext standing in for the points no camera sees when ``fallback`` is configured
(more_experiment_config.md:10) -- then -1 -> 0, int32, ``<save_path>/preds/lidarseg/<split>/<lidar_token>_lidarseg.bin`` and
the point-wise / pixel-wise confusion matrices.  The dataset is read without nuscenes-devkit
(pc_processor.dataset.nuScenes.open_nuscenes); any object with its attributes can be passed in (tests: oracle.cases.SyntheticNus).

    python infer.py config_server_nus.yaml
"""
import argparse
import datetime
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
import pc_processor  # noqa: E402
from option import Option  # noqa: E402
from nus_perspective_loader import NusPerspectiveViewLoader  # noqa: E402

getMergePred = pc_processor.postproc.getMergePred          # (:18-38 of the reference, on the GPU)


class LidarOnlyFallback(object):
    """per-point labels of a SalsaNext range-image model for a whole sweep (tasks/salsanext_eval_nuscenes/infer.py:60-110):
    spherical projection -> normalise * mask -> SalsaNext -> argmax read back at every point's pixel"""

    def __init__(self, model, cfg, device):
        from pmf_amd.dataset.preprocess.projection import RangeProjection
        self.model = model.to(device).eval()
        self.proj = RangeProjection(cfg["fov_up"], cfg["fov_down"], cfg["proj_w"], cfg["proj_h"], device=device)
        self.mean = torch.tensor(cfg["img_mean"], dtype=torch.float32, device=device)
        self.std = torch.tensor(cfg["img_stds"], dtype=torch.float32, device=device)

    @torch.no_grad()
    def __call__(self, pointcloud):
        n = pointcloud.shape[0]
        lab = torch.zeros(n, dtype=torch.int32, device=self.proj.device)
        feat, _, _, _ = self.proj.loader_item(pointcloud, lab, self.mean, self.std)
        pred = self.model(feat[None])
        am = pred[0].argmax(dim=0)
        c = self.proj.cached_data
        return am[c["uproj_y_idx"].long(), c["uproj_x_idx"].long()]


class Inference(object):
    def __init__(self, settings, model, recorder, dataset=None, fallback=None):
        self.settings, self.recorder = settings, recorder
        self.model = model.cuda()
        self.knn_flag = settings.config["post"]["KNN"]["use"]
        self.knn_post = pc_processor.postproc.KNN(params=settings.config["post"]["KNN"]["params"],
                                                  nclasses=settings.n_classes)
        self.fallback = fallback
        self.val_loader, self.nus_loader = self._initDataloader(dataset)
        self.prediction_path = os.path.join(settings.save_path, "preds")
        self.evaluator = pc_processor.metrics.IOUEval(n_classes=settings.n_classes, device=torch.device("cpu"), ignore=[0])
        self.pixel_eval = pc_processor.metrics.IOUEval(n_classes=settings.n_classes, device=torch.device("cpu"), ignore=[0])
        if self.knn_flag:
            self.recorder.logger.info("using KNN Post Process")
        self.data_split = "val" if settings.has_label else "test"

    def _initDataloader(self, dataset):
        s = self.settings
        if dataset is None:
            if s.dataset != "nuScenes":
                raise ValueError("invalid dataset: {}".format(s.dataset))
            if s.is_debug:
                version, split = "v1.0-mini", "val"
            elif s.has_label:
                version, split = "v1.0-trainval", "val"
            else:
                version, split = "v1.0-test", "test"
            dataset = pc_processor.dataset.nuScenes.open_nuscenes(False, s.data_root, version, split,
                                                                  splits_path=s.config.get("nus_splits"))
        loader = NusPerspectiveViewLoader(dataset=dataset, config=s.config)
        return loader, loader            # frames are visited in order, one at a time, on the device (:98-104: batch 1)

    @torch.no_grad()
    def run(self):
        s = self.settings
        self.model.eval()
        self.evaluator.reset()
        self.pixel_eval.reset()
        sensor = s.config["sensor"]
        mean = torch.tensor(sensor["img_mean"], dtype=torch.float32).view(1, -1, 1, 1).cuda()
        std = torch.tensor(sensor["img_stds"], dtype=torch.float32).view(1, -1, 1, 1).cuda()
        img_h = sensor["proj_h"]
        ds = self.nus_loader.dataset
        written = {}
        cam_count, idx_l, conf_l, lab_l = 0, [], [], []
        t_start = time.time()
        for i in range(len(self.val_loader)):
            feat, mask, label, ux, uy, udepth, point_idx, point_size = self.val_loader[i]
            t0 = time.time()
            ux, uy = ux.long(), uy.long()
            proj_depth = feat[0].clone()
            proj_depth = proj_depth - proj_depth.eq(0).float()                    # -1 on empty pixels (:122-123)
            h_pad = feat.size(1) - img_h
            x = feat[None, :, h_pad:, :].clone()
            m = mask[None, h_pad:, :]
            x[:, 0:5] = (x[:, 0:5] - mean) / std * m.unsqueeze(1)
            pred, _ = self.model(x[:, 0:5], x[:, 5:8])
            pred = torch.nn.functional.pad(pred, (0, 0, h_pad, 0))                # ZeroPad2d((0, 0, h_pad, 0)), :141-142
            pred_conf, pred_argmax = pred[0].max(dim=0)
            if s.has_label:
                self.pixel_eval.addBatch(pred.argmax(dim=1), label.long()[None])
            if self.knn_flag:
                unproj = self.knn_post(proj_depth, udepth, pred_argmax, uy, ux)  # (:151-157: x index = row)
            else:
                unproj = pred_argmax[ux, uy]
            cam_count += 1
            idx_l.append(point_idx)
            conf_l.append(pred_conf[ux, uy])
            lab_l.append(unproj)
            if cam_count == 6:
                token = ds.token_list[i]["lidar_token"]
                for j in range(i - 5, i):
                    assert ds.token_list[j]["lidar_token"] == token            # six views of ONE sweep (:173-177)
                pc_size = int(point_size[0].item())
                fb = None
                if self.fallback is not None:
                    fb = self.fallback(ds.loadDataByIndex(i)[0]).long()
                merged = getMergePred(idx_l, conf_l, lab_l, pc_size, fallback=fb)
                valid = merged.ne(-1).long()
                pred_np = (valid * merged).cpu().numpy().reshape(-1).astype(np.int32)
                cam_count, idx_l, conf_l, lab_l = 0, [], [], []
                if s.has_label:
                    _, sem_str, _ = ds.loadDataByIndex(i)
                    sem = ds.labelMapping(sem_str) * valid.cpu().numpy()
                    self.evaluator.addBatch(pred_np, sem)
                out_dir = os.path.join(self.prediction_path, "lidarseg", self.data_split)
                os.makedirs(out_dir, exist_ok=True)
                path = os.path.join(out_dir, "{}_lidarseg.bin".format(token))
                pred_np.tofile(path)
                written[token] = path
            msg = "Iter [{:04d}|{:04d}] Datatime: {:0.3f} ProcessTime: {:0.3f}".format(
                i, len(self.val_loader), t0 - t_start, time.time() - t0)
            if s.has_label:
                msg += " meanIOU {:0.4f}".format(self.pixel_eval.getIoU()[0].item())
            print(msg)
            t_start = time.time()
            if s.is_debug and i > 10:
                break
        if s.has_label:
            for title, ev in (("Point-wise Evaluation Results (3D eval)", self.evaluator),
                              ("Pixel-wise Evaluation Results (2D eval)", self.pixel_eval)):
                m_acc, _ = ev.getAcc()
                m_rec, _ = ev.getRecall()
                m_iou, c_iou = ev.getIoU()
                self.recorder.logger.info("============== {} ===================".format(title))
                self.recorder.logger.info("Acc avg: {:.4f}, IOU avg: {:.4f}, Recall avg: {:.4f}".format(
                    m_acc.item(), m_iou.item(), m_rec.item()))
                self.recorder.logger.info("latex: " + "".join(" & {:0.1f}".format(c_iou[k].item() * 100) for k in range(
                    1, s.n_classes)) + " & {:0.1f}".format(m_iou.item() * 100))
        return written


class Experiment(object):
    def __init__(self, settings, dataset=None):
        self.settings = settings
        settings.check_path()
        torch.manual_seed(settings.seed)
        torch.cuda.manual_seed(settings.seed)
        torch.cuda.set_device(0)
        self.recorder = pc_processor.checkpoint.Recorder(settings, settings.save_path, use_tensorboard=False)
        self.model = pc_processor.models.PMFNet(
            pcd_channels=5, img_channels=3, nclasses=settings.n_classes, base_channels=settings.base_channels,
            image_backbone=settings.img_backbone, imagenet_pretrained=settings.imagenet_pretrained)
        if not os.path.isfile(settings.pretrained_model):
            raise FileNotFoundError("pretrained model not found: {}".format(settings.pretrained_model))
        self.model.load_state_dict(torch.load(settings.pretrained_model, map_location="cpu"))
        self.recorder.logger.info("loading pretrained weight from: {}".format(settings.pretrained_model))
        fallback = None
        fb = settings.config.get("fallback")
        if fb:
            salsa = pc_processor.models.SalsaNext(5, settings.n_classes, settings.base_channels)
            salsa.load_state_dict(torch.load(fb["checkpoint"], map_location="cpu"))
            fallback = LidarOnlyFallback(salsa, fb, torch.device("cuda", 0))
        self.inference = Inference(settings, self.model, self.recorder, dataset=dataset, fallback=fallback)

    def run(self):
        t0 = time.time()
        out = self.inference.run()
        self.recorder.logger.info("==== total cost time: {}".format(datetime.timedelta(seconds=time.time() - t0)))
        return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description="PMF nuScenes inference on MI355X")
    ap.add_argument("config_path", type=str, metavar="config_path")
    ap.add_argument("--id", type=int, default=0)
    exp = Experiment(Option(ap.parse_args().config_path))
    print("===init env success===")
    exp.run()
