"""Point-wise EPMF evaluation on nuScenes (counterpart of the reference's tasks/epmf_eval_nuscenes/infer.py).

Six consecutive items of the dataset are the six camera views of ONE LiDAR sweep.  Per view:
PerspectiveViewLoaderV2(is_train=False, return_uproj=True) on a NuscenesV2-type dataset -- the frame is the bounding box of
the points inside the camera's yaw window, so every view has its own size -> zero pad to multiples of 64, columns centred,
rows at the bottom, + normalisation (pmf_eval_pre) -> EPMFNet (HIP plan, eval; one plan per padded shape) -> pixel
confusion of the view (pmf_eval_argmax) -> per kept point the confidence and label at its pixel, or the KNN votes, merged
into the sweep's running (confidence, label) pair where strictly more confident (pmf_eval_view_merge).  After the sixth
view (pmf_eval_sweep_finish): the points some camera labelled non-zero are scored, and with save_pred_results the uint8
labels go to <save_path>/preds/lidarseg/<val|test>/<lidar_token>_lidarseg.bin.  After the loop the reference's report:
point-wise and pixel-wise mean / per-class IoU, Acc and Recall, the LaTeX row, class distribution, fwIoU, and the
confusion / Acc / Recall matrices.  The dataset is read without nuscenes-devkit (pc_processor.dataset.nuScenes.open_nuscenes);
any object with its attributes can be passed in: Experiment(settings, dataset=...).

With the optional key sub_pred_folder (a folder written by tasks/salsanext_eval_nuscenes: preds/lidarseg/<val|test>/
<lidar_token>_lidarseg.bin, sub_pred_dtype int32 by default) the sweep's LiDAR-only labels are read and uploaded, and the
finish becomes pmf_eval_sweep_finish_fill: the same pass also fills the points no camera labelled (the rule of
tasks/pmf_eval_nuscenes/testset_eval: camera label where non-zero, else the LiDAR-only label, else fill_class), scores ALL
points into a second confusion, and the file written is the FUSED uint8 sweep, with preds/<val|test>/submission.json next to
it.  The camera-only report is unchanged; a "Fused point-wise" block and the share of points by source follow it.

    python infer.py config_server_nus.yaml [--dump-probs DIR]
"""
import argparse
import datetime
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
import pc_processor  # noqa: E402
from option import Option  # noqa: E402

N_CAM = 6


def _table(header, rows):
    w = [max(len(str(x)) for x in col) for col in zip(header, *rows)] if rows else [len(h) for h in header]
    line = lambda r: " | ".join(str(x).ljust(n) for x, n in zip(r, w))
    return "\n".join([line(header), "-+-".join("-" * n for n in w)] + [line(r) for r in rows])


def init_model(settings):
    """_initModel of the reference: EPMFNet only."""
    if settings.net_type != "EPMFNet":
        raise NotImplementedError("invalid net_type: {}".format(settings.net_type))
    return pc_processor.models.EPMFNet(
        pcd_channels=5, img_channels=3, nclasses=settings.n_classes, base_channels=settings.base_channels,
        image_backbone=settings.img_backbone, imagenet_pretrained=settings.imagenet_pretrained)


class Inference(object):
    def __init__(self, settings, model, recorder, dataset=None, dump_probs=None):
        self.settings, self.recorder = settings, recorder
        self.dump_probs = dump_probs
        self.model = model.cuda()
        self.knn_flag = settings.config["post"]["KNN"]["use"]
        pv = settings.config["PVconfig"]
        self.sweep_eval = pc_processor.postproc.SweepEvaluator(
            settings.n_classes, pv["pcd_mean"], pv["pcd_stds"],
            settings.config["post"]["KNN"]["params"] if self.knn_flag else None)
        self.pv_loader = self._initDataloader(dataset)
        self.prediction_path = os.path.join(settings.save_path, "preds")
        dev = torch.device("cuda")
        # confusion matrices on the device: the HIP post path adds each view / sweep to them in place
        self.evaluator = pc_processor.metrics.IOUEval(n_classes=settings.n_classes, device=dev, ignore=[0])
        self.pixel_eval = pc_processor.metrics.IOUEval(n_classes=settings.n_classes, device=dev, ignore=[0])
        self.data_split = "val" if settings.has_label else "test"
        # with sub_pred_folder: the fused full-sweep confusion and the points by source (main / sub / filled)
        self.fused_eval = self.source_counts = None
        if getattr(settings, "sub_pred_folder", None) is not None:
            self.fused_eval = pc_processor.metrics.IOUEval(n_classes=settings.n_classes, device=dev, ignore=[0])
            self.source_counts = torch.zeros(3, dtype=torch.int64, device=dev)
        if self.knn_flag:
            self.recorder.logger.info("using KNN Post Process")

    def _fallback(self, token, n_points):
        """the sweep's LiDAR-only labels from sub_pred_folder -> int32[P] on the device"""
        s = self.settings
        path = os.path.join(s.sub_pred_folder, "preds", "lidarseg", self.data_split, "{}_lidarseg.bin".format(token))
        if not os.path.isfile(path):
            raise FileNotFoundError("no sub prediction for sweep {}: {}".format(token, path))
        sub = np.fromfile(path, dtype=np.dtype(s.sub_pred_dtype)).astype(np.int32, copy=False)
        if sub.shape[0] != n_points:
            raise ValueError("sweep {}: {} points, the sub prediction has {}".format(token, n_points, sub.shape[0]))
        return torch.from_numpy(sub).cuda()

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
            dataset = pc_processor.dataset.nuScenes.open_nuscenes(True, s.data_root, version, split,
                                                                  splits_path=s.config.get("nus_splits"))
        # batch 1, views in order (the reference's DataLoader(batch_size=1, shuffle=False)); the scatter runs on the device
        return pc_processor.dataset.PerspectiveViewLoaderV2(dataset=dataset, config=s.config, is_train=False,
                                                            return_uproj=True)

    @torch.no_grad()
    def run(self):
        s = self.settings
        log = self.recorder.logger.info
        self.model.eval()
        self.evaluator.reset()
        self.pixel_eval.reset()
        fuse = self.fused_eval is not None
        if fuse:
            self.fused_eval.reset()
            self.source_counts.zero_()
        ds = self.pv_loader.dataset
        shapes, written = {}, {}
        n = len(self.pv_loader)
        token = None
        t_start = time.time()
        for i in range(n):
            t0 = time.time()
            proj, _, depth, _, extra = self.pv_loader._eval_item(i)
            pcd, rgb = self.sweep_eval.pre(proj)
            H, W = self.sweep_eval.geometry[:2]
            new_shape = (H, W) not in shapes
            if new_shape:
                n_plans = len(self.model._plans)
                torch.cuda.synchronize()
                tf = time.time()
            pred, _ = self.model(pcd, rgb)
            if new_shape:
                torch.cuda.synchronize()
                shapes[(H, W)] = time.time() - tf
                log("padded shape {}x{} (view {}x{}): {} + first forward {:.3f} s".format(
                    H, W, proj.shape[1], proj.shape[2],
                    "plan built" if len(self.model._plans) > n_plans else "plan cached", shapes[(H, W)]))
            self.sweep_eval.post_view(pred, depth, extra,
                                      pixel_conf=self.pixel_eval.conf_matrix if s.has_label else None)
            if s.has_label:
                self.pixel_eval.external_update()
            if self.dump_probs:
                os.makedirs(self.dump_probs, exist_ok=True)
                np.save(os.path.join(self.dump_probs, "{}.npy".format(i)), pred[0].cpu().numpy())
            current = ds.token_list[i]["lidar_token"]
            if token is None:
                token = current
            assert current == token, "views of different sweeps inside one group of six: {} / {}".format(token, current)
            if self.sweep_eval.views_in_sweep == N_CAM:
                extra_kw = {}
                if fuse:
                    extra_kw = dict(fallback=self._fallback(token, int(extra["sem"].shape[0])), fill_class=s.fill_class,
                                    fused_conf=self.fused_eval.conf_matrix if s.has_label else None,
                                    counts=self.source_counts)
                labels = self.sweep_eval.finish(
                    extra["sem"], extra["lut"], extra["sem"].shape[0],
                    point_conf=self.evaluator.conf_matrix if s.has_label else None, want_labels=s.save_pred_results,
                    **extra_kw)
                if s.has_label:
                    self.evaluator.external_update()
                    if fuse:
                        self.fused_eval.external_update()
                if s.save_pred_results:
                    out_dir = os.path.join(self.prediction_path, "lidarseg", self.data_split)
                    os.makedirs(out_dir, exist_ok=True)
                    path = os.path.join(out_dir, "{}_lidarseg.bin".format(token))
                    labels.cpu().numpy().tofile(path)
                    written[token] = path
                token = None
            if (i + 1) % max(int(s.print_frequency), 1) == 0 or i == n - 1 or s.is_debug:
                torch.cuda.synchronize()
                msg = "Iter [{:04d}|{:04d}] Datatime: {:0.3f} ProcessTime: {:0.3f}".format(
                    i, n, t0 - t_start, time.time() - t0)
                if s.has_label:
                    msg += " meanIOU {:0.4f}".format(self.evaluator.getIoU()[0].item())
                log(msg)
            t_start = time.time()
            if s.is_debug and i > 10:
                break
        if self.sweep_eval.views_in_sweep:
            log("the last {} views do not make a whole sweep: not merged".format(self.sweep_eval.views_in_sweep))
        log("padded shapes: {} distinct; {}".format(len(shapes), ", ".join(
            "{}x{} ({:.3f} s first forward)".format(h, w, t) for (h, w), t in shapes.items())))
        if s.has_label:
            self.report("Point-wise Evaluation Results (3D eval)", self.evaluator, pointwise=True)
            self.report("Pixel-wise Evaluation Results (2D eval)", self.pixel_eval, pointwise=False)
        if fuse:
            if s.has_label:
                self.report("Fused point-wise Evaluation Results (3D eval, all points)", self.fused_eval, pointwise=True)
            c = self.source_counts.cpu().tolist()
            t = max(sum(c), 1)
            log("Label source: main {:.4f} ({}), sub {:.4f} ({}), filled {:.4f} ({}) of {} points".format(
                c[0] / t, c[0], c[1] / t, c[1], c[2] / t, c[2], sum(c)))
            if s.save_pred_results:
                json_dir = os.path.join(self.prediction_path, self.data_split)
                os.makedirs(json_dir, exist_ok=True)
                with open(os.path.join(json_dir, "submission.json"), "w") as f:
                    json.dump({"meta": {"use_camera": True, "use_lidar": True, "use_radar": False, "use_map": False,
                                        "use_external": False}}, f, ensure_ascii=False, indent=4)
        return written

    def report(self, title, ev, pointwise):
        log = self.recorder.logger.info
        names = self.pv_loader.dataset.mapped_cls_name
        n = self.settings.n_classes
        m_acc, c_acc = ev.getAcc()
        m_rec, c_rec = ev.getRecall()
        m_iou, c_iou = ev.getIoU()
        log("============== {} ===================".format(title))
        log("{}Acc avg: {:.4f}, IOU avg: {:.4f}, Recall avg: {:.4f}".format(
            "" if pointwise else "Pixel ", m_acc.item(), m_iou.item(), m_rec.item()))
        log("\n" + _table(["ClassIdx", "class_name", "IOU", "Acc", "Recall"],
                          [[i, names[i], "%.4f" % c_iou[i].item(), "%.4f" % c_acc[i].item(), "%.4f" % c_rec[i].item()]
                           for i in range(1, n)]))
        log("---- Latext Format String -----")
        log("".join(" & {:0.1f}".format(c_iou[i].item() * 100) for i in range(1, n)) +
            " & {:0.1f}".format(m_iou.item() * 100))
        conf = ev.conf_matrix.clone().cpu()
        conf[0] = 0
        conf[:, 0] = 0
        dist = conf.sum(0)
        log("---- Data Distribution -----")
        if pointwise:
            total = max(int(dist.sum().item()), 1)
            log("\n" + _table(["Class Name", "Number of points", "Percentage"],
                              [[names[i], int(dist[i].item()), "%.4f" % (int(dist[i].item()) / total)] for i in range(n)]))
            freqw = dist[1:].double() / dist[1:].sum().clamp_min(1).double()
            log("fwIoU: {}".format((c_iou[1:].cpu().double() * freqw).sum().item()))
        else:
            log("\n" + _table(["Class Name", "Number of points"], [[names[i], int(dist[i].item())] for i in range(n)]))
        log("---- confusion matrix original data -----")
        log("\n" + _table([" "] + [str(j) for j in range(n)],
                          [[str(i)] + [int(v) for v in conf[i].tolist()] for i in range(n)]))
        for what, data in (("ACC", conf.float() / (conf.sum(1, keepdim=True).float() + 1e-8)),
                           ("Recall", conf.float() / (conf.sum(0, keepdim=True).float() + 1e-8))):
            log("---- {} matrix ----------------".format(what))
            log("\n" + _table([" "] + [names[j] for j in range(1, n)],
                              [[names[i]] + ["{:0.1f}".format(data[i, j].item() * 100) for j in range(1, n)]
                               for i in range(1, n)]))


class Experiment(object):
    def __init__(self, settings, dataset=None, dump_probs=None):
        self.settings = settings
        settings.check_path()
        torch.manual_seed(settings.seed)
        torch.cuda.manual_seed(settings.seed)
        torch.cuda.set_device(0)
        self.recorder = pc_processor.checkpoint.Recorder(settings, settings.save_path, use_tensorboard=False)
        self.model = init_model(settings)
        if settings.pretrained_model is not None:
            if not os.path.isfile(settings.pretrained_model):
                raise FileNotFoundError("pretrained model not found: {}".format(settings.pretrained_model))
            self.model.load_state_dict(torch.load(settings.pretrained_model, map_location="cpu"))
            self.recorder.logger.info("loading pretrained weight from: {}".format(settings.pretrained_model))
        self.inference = Inference(settings, self.model, self.recorder, dataset=dataset, dump_probs=dump_probs)

    def run(self):
        t0 = time.time()
        out = self.inference.run()
        self.recorder.logger.info("==== total cost time: {}".format(datetime.timedelta(seconds=time.time() - t0)))
        return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description="EPMF nuScenes inference on MI355X")
    ap.add_argument("config_path", type=str, metavar="config_path")
    ap.add_argument("--id", type=int, default=0)
    ap.add_argument("--dump-probs", type=str, default=None, metavar="DIR",
                    help="also write every view's padded probability map [C, H, W] as DIR/<index>.npy")
    args = ap.parse_args()
    exp = Experiment(Option(args.config_path), dump_probs=args.dump_probs)
    print("===init env success===")
    exp.run()
