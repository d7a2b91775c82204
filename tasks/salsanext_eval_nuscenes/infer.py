"""Point-wise SalsaNext evaluation on nuScenes (counterpart of the reference's tasks/salsanext_eval_nuscenes/infer.py).

Every sweep is one range image of sensor.proj_h x proj_w (32 x 2048), so sweeps batch: eval_batch_size of them go through
SalsaNext per forward (SalsaNextLoader._eval_item: one loadDataByIndex per sweep, raw labels and the label table on the
device), and everything behind the network is ONE batched pass of two launches (pmf_eval_range_batch through
RangeSweepEvaluator): argmax + pixel confusion of the B maps, then per point the label at its pixel or the KNN vote,
int32 labels + point confusion.  One device-to-host copy per batch; every sweep's labels go to
<save_path>/preds/lidarseg/<val|test>/<lidar_token>_lidarseg.bin as int32 (what the reference's SalsaNext script writes).
The last batch may be short: it runs at its own size (the model keeps one plan per input shape), nothing is padded.
After the loop the reference's report: point-wise and pixel-wise mean / per-class IoU, Acc and Recall, the LaTeX row, class
distribution, fwIoU, and the confusion / Acc / Recall matrices, as plain-text tables.  The dataset is read without
nuscenes-devkit (pc_processor.dataset.nuScenes.open_nuscenes, has_image=False); any object with loadDataByIndex, labelMapping,
map_name_from_general_index_to_segmentation_index (or class_map_lut), mapped_cls_name and token_list can be passed in:
Experiment(settings, dataset=...).

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


def _table(header, rows):
    w = [max(len(str(x)) for x in col) for col in zip(header, *rows)] if rows else [len(h) for h in header]
    line = lambda r: " | ".join(str(x).ljust(n) for x, n in zip(r, w))
    return "\n".join([line(header), "-+-".join("-" * n for n in w)] + [line(r) for r in rows])


def report_lines(title, ev, names, n, pointwise):
    """the reference's report of one IOUEval (infer.py:142-280) as a list of log entries"""
    out = []
    m_acc, c_acc = ev.getAcc()
    m_rec, c_rec = ev.getRecall()
    m_iou, c_iou = ev.getIoU()
    out.append("============== {} ===================".format(title))
    out.append("{}Acc avg: {:.4f}, IOU avg: {:.4f}, Recall avg: {:.4f}".format(
        "" if pointwise else "Pixel ", m_acc.item(), m_iou.item(), m_rec.item()))
    out.append("\n" + _table(["ClassIdx", "class_name", "IOU", "Acc", "Recall"],
                             [[i, names[i], "%.4f" % c_iou[i].item(), "%.4f" % c_acc[i].item(), "%.4f" % c_rec[i].item()]
                              for i in range(1, n)]))
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
                                 [[names[i], int(dist[i].item()), "%.4f" % (int(dist[i].item()) / total)]
                                  for i in range(n)]))
        freqw = dist[1:].double() / dist[1:].sum().clamp_min(1).double()
        out.append("fwIoU: {}".format((c_iou[1:].cpu().double() * freqw).sum().item()))
    else:
        out.append("\n" + _table(["Class Name", "Number of points"], [[names[i], int(dist[i].item())] for i in range(n)]))
    out.append("---- confusion matrix original data -----")
    out.append("\n" + _table([" "] + [str(j) for j in range(n)],
                             [[str(i)] + [int(v) for v in conf[i].tolist()] for i in range(n)]))
    for what, data in (("ACC", conf.float() / (conf.sum(1, keepdim=True).float() + 1e-8)),
                       ("Recall", conf.float() / (conf.sum(0, keepdim=True).float() + 1e-8))):
        out.append("---- {} matrix ----------------".format(what))
        out.append("\n" + _table([" "] + [names[j] for j in range(1, n)],
                                 [[names[i]] + ["{:0.1f}".format(data[i, j].item() * 100) for j in range(1, n)]
                                  for i in range(1, n)]))
    return out


class Inference(object):
    def __init__(self, settings, model, recorder, dataset=None):
        self.settings, self.recorder = settings, recorder
        self.model = model.cuda()
        self.knn_flag = settings.config["post"]["KNN"]["use"]
        self.range_eval = pc_processor.postproc.RangeSweepEvaluator(
            settings.n_classes, settings.config["post"]["KNN"]["params"] if self.knn_flag else None)
        self.salsa_loader = self._initDataloader(dataset)
        self.prediction_path = os.path.join(settings.save_path, "preds")
        dev = torch.device("cuda")
        # confusion matrices on the device: the HIP pass adds each batch to them in place
        self.evaluator = pc_processor.metrics.IOUEval(n_classes=settings.n_classes, device=dev, ignore=[0])
        self.pixel_eval = pc_processor.metrics.IOUEval(n_classes=settings.n_classes, device=dev, ignore=[0])
        self.data_split = "val" if settings.has_label else "test"
        if self.knn_flag:
            self.recorder.logger.info("using KNN Post Process")

    def _initDataloader(self, dataset):
        s = self.settings
        if dataset is None:
            if s.dataset not in ("NuScenes", "nuScenes"):
                raise ValueError("invalid dataset: {}".format(s.dataset))
            version, split = ("v1.0-trainval", "val") if s.has_label else ("v1.0-test", "test")
            dataset = pc_processor.dataset.nuScenes.open_nuscenes(False, s.data_root, version, split, has_image=False,
                                                                  splits_path=s.config.get("nus_splits"))
        return pc_processor.dataset.SalsaNextLoader(dataset=dataset, config=s.config, data_len=s.data_len,
                                                    is_train=False, return_uproj=True)

    @torch.no_grad()
    def run(self):
        s = self.settings
        log = self.recorder.logger.info
        self.model.eval()
        self.evaluator.reset()
        self.pixel_eval.reset()
        ds = self.salsa_loader.dataset
        n, bs = len(self.salsa_loader), s.eval_batch_size
        out_dir = os.path.join(self.prediction_path, "lidarseg", self.data_split)
        os.makedirs(out_dir, exist_ok=True)
        written = {}
        t_start = time.time()
        for it, first in enumerate(range(0, n, bs)):
            idx = list(range(first, min(first + bs, n)))          # the last batch may be short: its own plan
            items = [self.salsa_loader._eval_item(i) for i in idx]
            t0 = time.time()
            pred = self.model(torch.stack([x["feature"] for x in items]))
            labels = self.range_eval.post(pred, items,
                                          pixel_conf=self.pixel_eval.conf_matrix if s.has_label else None,
                                          point_conf=self.evaluator.conf_matrix if s.has_label else None)
            if s.has_label:
                self.pixel_eval.external_update()
                self.evaluator.external_update()
            host = self.range_eval.labels.cpu().numpy()      # one device-to-host copy per batch: all its sweeps, in order
            o = 0
            for i, l in zip(idx, labels):
                k = int(l.shape[0])
                path = os.path.join(out_dir, "{}_lidarseg.bin".format(ds.token_list[i]))
                host[o:o + k].astype(np.int32, copy=False).tofile(path)
                written[ds.token_list[i]] = path
                o += k
            if (it + 1) % max(int(s.print_frequency), 1) == 0 or idx[-1] == n - 1 or s.is_debug:
                msg = "Iter [{:04d}|{:04d}] Datatime: {:0.3f} ProcessTime: {:0.3f}".format(
                    idx[-1], n, t0 - t_start, time.time() - t0)
                if s.has_label:
                    msg += " meanIOU {:0.4f}".format(self.evaluator.getIoU()[0].item())
                log(msg)
            t_start = time.time()
            if s.is_debug and idx[-1] > 10:
                break
        if s.has_label:
            names = ds.mapped_cls_name
            for line in report_lines("Point-wise Evaluation Results (3D eval)", self.evaluator, names, s.n_classes, True):
                log(line)
            for line in report_lines("Pixel-wise Evaluation Results (2D eval)", self.pixel_eval, names, s.n_classes, False):
                log(line)
        return written


class Experiment(object):
    def __init__(self, settings, dataset=None, model=None):
        self.settings = settings
        os.environ["CUDA_VISIBLE_DEVICES"] = settings.gpu       # as the reference: before the first CUDA call of the process
        settings.check_path()
        torch.manual_seed(settings.seed)
        torch.cuda.manual_seed(settings.seed)
        torch.cuda.set_device(0)
        self.recorder = pc_processor.checkpoint.Recorder(settings, settings.save_path, use_tensorboard=False)
        self.model = model if model is not None else pc_processor.models.SalsaNext(in_channels=5,
                                                                                   nclasses=settings.n_classes)
        if settings.pretrained_model is not None:
            if not os.path.isfile(settings.pretrained_model):
                raise FileNotFoundError("pretrained model not found: {}".format(settings.pretrained_model))
            self.model.load_state_dict(torch.load(settings.pretrained_model, map_location="cpu"))
            self.recorder.logger.info("loading pretrained weight from: {}".format(settings.pretrained_model))
        self.inference = Inference(settings, self.model, self.recorder, dataset=dataset)

    def run(self):
        t0 = time.time()
        out = self.inference.run()
        self.recorder.logger.info("==== total cost time: {}".format(datetime.timedelta(seconds=time.time() - t0)))
        return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description="SalsaNext nuScenes inference on MI355X")
    ap.add_argument("config_path", type=str, metavar="config_path")
    ap.add_argument("--id", type=int, default=0)
    args = ap.parse_args()
    exp = Experiment(Option(args.config_path))
    print("===init env success===")
    exp.run()
