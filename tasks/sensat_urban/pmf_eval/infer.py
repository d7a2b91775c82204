"""PMF evaluation on SensatUrban (counterpart of the reference's tasks/sensat_urban/pmf_eval/infer.py).

Per block: the bird's-eye-view frame f32[8,h,w] is uploaded once; for every size of img_size it is cut into tiles (the last
row / column shifted back to the border), each tile normalised on the device (pmf_bev_tile_pre), run through PMFNet (HIP plan,
eval; with post.tta.use the tile's six same-size variants as one batch-6 forward plus the 16-pixel padded one) and added
to the confidence map of the frame on the device in the reference's order (pmf_bev_tile_accum) -> argmax + pixel confusion
(pmf_eval_argmax) -> the points' labels at their pixel or voted by KNN over the first height map and the points' z from the
.ply, 0 -> 1, + point confusion (pmf_bev_points).  Written per block: <save_path>/preds/{val,test}_preds/<name>.label
(uint8 pred - 1) and, with save_scores, <save_path>/preds/{val,test}_scors/<name>.npy (f32[1,C,h,w]).  After the loop the
reference's report: point-wise and pixel-wise mean / per-class IoU, Acc and Recall, the LaTeX row, class distribution,
fwIoU, and the confusion / Acc / Recall matrices.

    python infer.py config_server.yaml
"""
import argparse
import datetime
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", ".."))
import pc_processor  # noqa: E402
import sensat_tools  # noqa: E402
from option import Option  # noqa: E402


def _table(header, rows):
    w = [max(len(str(x)) for x in col) for col in zip(header, *rows)] if rows else [len(h) for h in header]
    line = lambda r: " | ".join(str(x).ljust(n) for x, n in zip(r, w))
    return "\n".join([line(header), "-+-".join("-" * n for n in w)] + [line(r) for r in rows])


def report_lines(title, ev, names, n, pointwise):
    """the reference's report for one IOUEval; class i of the network is names[i - 1] (names[-1] = ignore)"""
    out = []
    m_acc, c_acc = ev.getAcc()
    m_rec, c_rec = ev.getRecall()
    m_iou, c_iou = ev.getIoU()
    out.append("============== {} ===================".format(title))
    out.append("{}Acc avg: {:.4f}, IOU avg: {:.4f}, Recall avg: {:.4f}".format(
        "" if pointwise else "Pixel ", m_acc.item(), m_iou.item(), m_rec.item()))
    out.append("\n" + _table(["ClassIdx", "class_name", "IOU", "Acc", "Recall"],
                             [[i, names[i - 1], "%.4f" % c_iou[i].item(), "%.4f" % c_acc[i].item(),
                               "%.4f" % c_rec[i].item()] for i in range(1, n)]))
    out.append("---- Latext Format String -----")
    out.append("".join(" & {:0.1f}".format(c_iou[i].item() * 100) for i in range(1, n)) +
               " & {:0.1f}".format(m_iou.item() * 100))
    conf = ev.conf_matrix.clone().cpu()
    conf[0] = 0
    conf[:, 0] = 0
    dist = conf.sum(0)
    out.append("---- Data Distribution -----")
    if pointwise:
        total = max(int(dist.sum().item()), 1)
        out.append("\n" + _table(["Class Name", "Number of points", "Percentage"],
                                 [[names[i - 1], int(dist[i].item()), "%.4f" % (int(dist[i].item()) / total)]
                                  for i in range(n)]))
        freqw = dist[1:].double() / dist[1:].sum().clamp_min(1).double()
        out.append("fwIoU: {}".format((c_iou[1:].cpu().double() * freqw).sum().item()))
    else:
        out.append("\n" + _table(["Class Name", "Number of points"],
                                 [[names[i - 1], int(dist[i].item())] for i in range(n)]))
    out.append("---- confusion matrix original data -----")
    out.append("\n" + _table([" "] + [str(j) for j in range(n)],
                             [[str(i)] + [int(v) for v in conf[i].tolist()] for i in range(n)]))
    for what, data in (("ACC", conf.float() / (conf.sum(1, keepdim=True).float() + 1e-8)),
                       ("Recall", conf.float() / (conf.sum(0, keepdim=True).float() + 1e-8))):
        out.append("---- {} matrix ----------------".format(what))
        out.append("\n" + _table([" "] + [names[j - 1] for j in range(1, n)],
                                 [[names[i - 1]] + ["{:0.1f}".format(data[i, j].item() * 100) for j in range(1, n)]
                                  for i in range(1, n)]))
    return out


class Inference(object):
    def __init__(self, settings, model, recorder):
        self.settings, self.recorder = settings, recorder
        self.model = model.cuda()
        post = settings.config["post"]
        self.use_knn = post["KNN"]["use"]
        self.use_tta = post["tta"]["use"]
        if self.use_knn:
            recorder.logger.info("use knn")
        if self.use_tta:
            recorder.logger.info("use tta")
        self.data_split = "val" if settings.has_label else "test"
        self.valset = self._initDataloader()
        self.prediction_path = os.path.join(settings.save_path, "preds")
        self.tiles = pc_processor.postproc.BevTileEvaluator(
            self.model, settings.nclasses, settings.feature_mean, settings.feature_std, settings.img_size,
            tta=self.use_tta, knn_params=post["KNN"]["params"] if self.use_knn else None)
        dev = torch.device("cuda")
        # confusion matrices on the device: the HIP passes add each frame to them in place
        self.evaluator = pc_processor.metrics.IOUEval(n_classes=settings.nclasses, device=dev, ignore=[0])
        self.pixel_eval = pc_processor.metrics.IOUEval(n_classes=settings.nclasses, device=dev, ignore=[0])

    def _initDataloader(self):
        s = self.settings
        if s.dataset != "SensatUrban":
            raise ValueError("invalid dataset: {}".format(s.dataset))
        return pc_processor.dataset.SensatUrban(root_path=s.data_root, split=self.data_split, keep_idx=True,
                                                use_crop=False)

    @torch.no_grad()
    def run(self):
        s = self.settings
        log = self.recorder.logger.info
        self.model.eval()
        self.evaluator.reset()
        self.pixel_eval.reset()
        pred_path = os.path.join(self.prediction_path, "{}_preds".format(self.data_split))
        score_path = os.path.join(self.prediction_path, "{}_scors".format(self.data_split))
        os.makedirs(pred_path, exist_ok=True)
        if s.save_scores:
            os.makedirs(score_path, exist_ok=True)
        n = len(self.valset)
        t_start = time.time()
        for i in range(n):
            t0 = time.time()
            frame = self.valset.readDataByIndex(i)
            name = self.valset.readFileNameByIndex(i)
            z = None
            if self.use_knn:
                z = sensat_tools.read_ply(os.path.join(self.valset.split_folder, name.replace(".bin", ".ply")))["z"]
            label = self.valset.readLabelByIndex(i) if s.has_label else None
            pred, conf_map, zero_num = self.tiles.frame(
                frame, z=z, label=label, pixel_conf=self.pixel_eval.conf_matrix if s.has_label else None,
                point_conf=self.evaluator.conf_matrix if s.has_label else None)
            if zero_num > 0:
                print("warning zero_num: ", zero_num, " set zero to ground")
            if s.has_label:
                self.evaluator.external_update()
                self.pixel_eval.external_update()
            pred.cpu().numpy().tofile(os.path.join(pred_path, name.replace(".bin", ".label")))
            if s.save_scores:
                # (the reference's name.strip(".bin") removes a character SET from both ends; the extension is meant)
                np.save(os.path.join(score_path, name[:-len(".bin")]), conf_map.unsqueeze(0).cpu().numpy())
            torch.cuda.synchronize()
            msg = "Iter [{:04d}|{:04d}] Datatime: {:0.3f} ProcessTime: {:0.3f}".format(i, n, t0 - t_start, time.time() - t0)
            if s.has_label:
                msg += " meanIOU {:0.4f}".format(self.pixel_eval.getIoU()[0].item())
            log(msg)
            t_start = time.time()
            if s.is_debug:
                break
        if not s.has_label:
            return
        names = self.valset.mapped_cls_name
        for line in report_lines("Point-wise Evaluation Results (3D eval)", self.evaluator, names, s.nclasses, True):
            log(line)
        for line in report_lines("Pixel-wise Evaluation Results (2D eval)", self.pixel_eval, names, s.nclasses, False):
            log(line)


class Experiment(object):
    def __init__(self, settings):
        self.settings = settings
        settings.check_path()
        torch.manual_seed(settings.seed)
        torch.cuda.manual_seed(settings.seed)
        torch.cuda.set_device(0)
        self.recorder = pc_processor.checkpoint.Recorder(settings, settings.save_path, use_tensorboard=False)
        self.model = pc_processor.models.PMFNet(
            pcd_channels=5, img_channels=3, nclasses=settings.nclasses, base_channels=settings.base_channels,
            image_backbone=settings.img_backbone, imagenet_pretrained=settings.imagenet_pretrained)
        if settings.pretrained_model is not None:
            if not os.path.isfile(settings.pretrained_model):
                raise FileNotFoundError("pretrained model not found: {}".format(settings.pretrained_model))
            self.model.load_state_dict(torch.load(settings.pretrained_model, map_location="cpu"))
            self.recorder.logger.info("loading pretrained weight from: {}".format(settings.pretrained_model))
        self.inference = Inference(settings, self.model, self.recorder)

    def run(self):
        t0 = time.time()
        self.inference.run()
        self.recorder.logger.info("==== total cost time: {}".format(datetime.timedelta(seconds=time.time() - t0)))


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description="PMF inference on SensatUrban, MI355X")
    ap.add_argument("config_path", type=str, metavar="config_path")
    ap.add_argument("--id", type=int, default=0)
    args = ap.parse_args()
    exp = Experiment(Option(args.config_path))
    print("===init env success===")
    exp.run()
