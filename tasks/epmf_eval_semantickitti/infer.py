"""Point-wise EPMF evaluation on SemanticKITTI (counterpart of the reference's tasks/epmf_eval_semantickitti/infer.py).

Per frame: PerspectiveViewLoaderV2(is_train=False, return_uproj=True) -- the frame is the bounding box of the points
inside the +-45 degree yaw crop, so every frame has its own size -> centred zero pad to multiples of 64 + normalisation
(pmf_eval_pre) -> EPMFNet (HIP plan, eval; one plan per padded shape) -> argmax over the crop window + pixel confusion
(pmf_eval_argmax) -> labels of the kept points, read at their pixel or voted by KNN, + point confusion and uint32
annotation ids (pmf_eval_points).  With save_preds: <save_path>/preds/sequences/<seq>/predictions/<frame>.label.
After the loop the reference's report: point-wise and pixel-wise mean / per-class IoU, Acc and Recall, the LaTeX row,
class distribution, fwIoU, and the confusion / Acc / Recall matrices.

    python infer.py config.yaml [--dump-probs DIR]
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
    def __init__(self, settings, model, recorder, dump_probs=None):
        self.settings, self.recorder = settings, recorder
        self.dump_probs = dump_probs
        self.model = model.cuda()
        self.knn_flag = settings.config["post"]["KNN"]["use"]
        pv = settings.config["PVconfig"]
        self.frame_eval = pc_processor.postproc.FrameEvaluator(
            settings.n_classes, pv["pcd_mean"], pv["pcd_stds"],
            settings.config["post"]["KNN"]["params"] if self.knn_flag else None)
        self.pv_loader = self._initDataloader()
        self.prediction_path = os.path.join(settings.save_path, "preds")
        dev = torch.device("cuda")
        # confusion matrices on the device: the HIP post path adds each frame to them in place
        self.evaluator = pc_processor.metrics.IOUEval(n_classes=settings.n_classes, device=dev, ignore=[0])
        self.pixel_eval = pc_processor.metrics.IOUEval(n_classes=settings.n_classes, device=dev, ignore=[0])
        self.lut_inv = torch.as_tensor(self.pv_loader.dataset.class_map_lut_inv.astype(np.int32)).to(dev)
        if self.knn_flag:
            self.recorder.logger.info("using KNN Post Process")

    def _initDataloader(self):
        s = self.settings
        if s.dataset != "SemanticKitti":
            raise ValueError("invalid dataset: {}".format(s.dataset))
        cfg_path = s.config.get("data_config_path") or pc_processor.dataset.semantic_kitti.DEFAULT_CONFIG
        valset = pc_processor.dataset.semantic_kitti.SemanticKitti(
            root=s.data_root, sequences=list(s.config.get("sequences", {}).get("valid", [8])), config_path=cfg_path,
            has_label=s.has_label, has_image=True)
        # batch 1, frames in order (the reference's DataLoader(batch_size=1, shuffle=False)); the projection runs on the device
        return pc_processor.dataset.PerspectiveViewLoaderV2(dataset=valset, config=s.config, is_train=False,
                                                            return_uproj=True)

    @torch.no_grad()
    def run(self):
        s = self.settings
        log = self.recorder.logger.info
        self.model.eval()
        self.evaluator.reset()
        self.pixel_eval.reset()
        ds = self.pv_loader.dataset
        shapes = {}
        n = len(self.pv_loader)
        t_start = time.time()
        for i in range(n):
            t0 = time.time()
            proj, _, depth, _, extra = self.pv_loader._eval_item(i)
            pcd, rgb = self.frame_eval.pre(proj)
            H, W = self.frame_eval.geometry[:2]
            new_shape = (H, W) not in shapes
            if new_shape:
                n_plans = len(self.model._plans)
                torch.cuda.synchronize()
                tf = time.time()
            pred, _ = self.model(pcd, rgb)
            if new_shape:
                torch.cuda.synchronize()
                shapes[(H, W)] = time.time() - tf
                log("padded shape {}x{} (frame {}x{}): {} + first forward {:.3f} s".format(
                    H, W, proj.shape[1], proj.shape[2],
                    "plan built" if len(self.model._plans) > n_plans else "plan cached", shapes[(H, W)]))
            _, labels_inv = self.frame_eval.post(
                pred, depth, extra, pixel_conf=self.pixel_eval.conf_matrix if s.has_label else None,
                point_conf=self.evaluator.conf_matrix if s.has_label else None,
                lut_inv=self.lut_inv if s.save_preds else None)
            if s.has_label:
                self.evaluator.external_update()
                self.pixel_eval.external_update()
            seq_id, frame_id = ds.parsePathInfoByIndex(i)
            if self.dump_probs:
                os.makedirs(self.dump_probs, exist_ok=True)
                np.save(os.path.join(self.dump_probs, "{}_{}.npy".format(seq_id, frame_id)), pred[0].cpu().numpy())
            if s.save_preds:
                pred_path = os.path.join(self.prediction_path, "sequences", seq_id, "predictions")
                os.makedirs(pred_path, exist_ok=True)
                labels_inv.cpu().numpy().view(np.uint32).tofile(os.path.join(pred_path, "{}.label".format(frame_id)))
            if (i + 1) % max(int(s.print_frequency), 1) == 0 or i == n - 1 or s.is_debug:
                torch.cuda.synchronize()
                msg = "Iter [{:04d}|{:04d}] {}/{} Datatime: {:0.3f} ProcessTime: {:0.3f}".format(
                    i, n, seq_id, frame_id, t0 - t_start, time.time() - t0)
                if s.has_label:
                    msg += " meanIOU {:0.4f}".format(self.pixel_eval.getIoU()[0].item())
                log(msg)
            t_start = time.time()
            if s.is_debug:
                break
        log("padded shapes: {} distinct; {}".format(len(shapes), ", ".join(
            "{}x{} ({:.3f} s first forward)".format(h, w, t) for (h, w), t in shapes.items())))
        if not s.has_label:
            return
        self.report("Point-wise Evaluation Results (3D eval)", self.evaluator, pointwise=True)
        self.report("Pixel-wise Evaluation Results (2D eval)", self.pixel_eval, pointwise=False)

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
    def __init__(self, settings, dump_probs=None):
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
        self.inference = Inference(settings, self.model, self.recorder, dump_probs)

    def run(self):
        t0 = time.time()
        self.inference.run()
        self.recorder.logger.info("==== total cost time: {}".format(datetime.timedelta(seconds=time.time() - t0)))


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description="EPMF inference on MI355X")
    ap.add_argument("config_path", type=str, metavar="config_path")
    ap.add_argument("--id", type=int, default=0)
    ap.add_argument("--dump-probs", type=str, default=None, metavar="DIR",
                    help="also write every frame's padded probability map [C, H, W] as DIR/<seq>_<frame>.npy")
    args = ap.parse_args()
    exp = Experiment(Option(args.config_path), args.dump_probs)
    print("===init env success===")
    exp.run()
