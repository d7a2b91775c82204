"""Full-sweep nuScenes result from two prediction folders (counterpart of the reference's
tasks/pmf_eval_nuscenes/testset_eval/main.py, MergePred).

main_pred_folder holds the camera + LiDAR network's labels (tasks/pmf_eval_nuscenes: int32, tasks/epmf_eval_nuscenes: uint8),
0 for every point no camera sees; sub_pred_folder holds the LiDAR-only network's (tasks/salsanext_eval_nuscenes: int32).
Per point: the main label where it is non-zero, else the sub label, and what is still 0 becomes fill_class (11); ALL points
are scored against labelMapping(loadLabelByIndex(i)).  merge_batch_size sweeps go through the device per call: their files
are read on the host, one packed upload, one pmf_eval_fill launch (fused uint8 labels + confusion + source counts), one
device-to-host copy.  Output, as the reference writes it: <save_path>/<experiment_id>/preds/lidarseg/<val|test>/
<lidar_token>_lidarseg.bin (uint8) and preds/<val|test>/submission.json; then the reference's report (point-wise table, LaTeX
row, class distribution, fwIoU, confusion / Acc / Recall matrices) as plain-text tables, plus the share of points by source.
The dataset is read without nuscenes-devkit (pc_processor.dataset.nuScenes.open_nuscenes, has_image=False); any object with
token_list, loadLabelByIndex, labelMapping (or map_name_from_general_index_to_segmentation_index) and mapped_cls_name can be
passed in: Experiment(settings, dataset=...).  check_valid.py validates the written folder.

    python main.py config_server.yaml
"""
import argparse
import datetime
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", ".."))
import pc_processor  # noqa: E402
from pc_processor.dataset.perspective_view_loader import upload_packed  # noqa: E402
from option import Option  # noqa: E402

SUBMISSION_META = {"use_camera": True, "use_lidar": True, "use_radar": False, "use_map": False, "use_external": False}


def _table(header, rows):
    w = [max(len(str(x)) for x in col) for col in zip(header, *rows)] if rows else [len(h) for h in header]
    line = lambda r: " | ".join(str(x).ljust(n) for x, n in zip(r, w))
    return "\n".join([line(header), "-+-".join("-" * n for n in w)] + [line(r) for r in rows])


def pred_file(folder, split, token):
    return os.path.join(folder, "preds", "lidarseg", split, "{}_lidarseg.bin".format(token))


def read_pred(path, dtype, token):
    """one prediction file -> int32[P]; dtype "int32" or "uint8" (what the file holds)"""
    if dtype not in ("int32", "uint8"):
        raise ValueError("prediction dtype must be int32 or uint8, got {!r}".format(dtype))
    if not os.path.isfile(path):
        raise FileNotFoundError("no prediction for sweep {}: {}".format(token, path))
    if dtype == "int32" and os.path.getsize(path) % 4:
        raise ValueError("sweep {}: {} is not a whole number of int32 labels".format(token, path))
    return np.fromfile(path, dtype=np.dtype(dtype)).astype(np.int32, copy=False)


def read_pair(main_folder, sub_folder, split, token, main_dtype="int32", sub_dtype="int32"):
    """the two predictions of one sweep -> (main int32[P], sub int32[P]), one label per point in both"""
    main = read_pred(pred_file(main_folder, split, token), main_dtype, token)
    sub = read_pred(pred_file(sub_folder, split, token), sub_dtype, token)
    if main.shape[0] != sub.shape[0]:
        raise ValueError("sweep {}: the main prediction has {} points, the sub prediction {}".format(
            token, main.shape[0], sub.shape[0]))
    return main, sub


def label_lut(dataset):
    """int32[256]: raw annotation id -> class, as the other nuScenes tasks build it: the dataset's
    map_name_from_general_index_to_segmentation_index when it has one, else labelMapping evaluated once on all 256 ids"""
    lut = np.zeros(256, np.int32)
    table = getattr(dataset, "map_name_from_general_index_to_segmentation_index", None)
    if table is not None:
        keys = sorted(k for k in table if 0 <= int(k) < 256)
        lut[keys] = [int(table[k]) for k in keys]
    else:
        lut[:] = np.asarray(dataset.labelMapping(np.arange(256, dtype=np.uint8)[:, None])).reshape(-1)
    return lut


def report_lines(ev, names, n, counts):
    """the reference's report (main.py:136-206) of the fused confusion as a list of log entries, plus the source shares"""
    out = []
    m_acc, c_acc = ev.getAcc()
    m_rec, c_rec = ev.getRecall()
    m_iou, c_iou = ev.getIoU()
    out.append("============== Point-wise Evaluation Results (3D eval) ===================")
    out.append("Acc avg: {:.4f}, IOU avg: {:.4f}, Recall avg: {:.4f}".format(m_acc.item(), m_iou.item(), m_rec.item()))
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
    total = max(int(dist.sum().item()), 1)
    out.append("---- Data Distribution -----")
    out.append("\n" + _table(["Class Name", "Number of points", "Percentage"],
                             [[names[i], int(dist[i].item()), "%.4f" % (int(dist[i].item()) / total)] for i in range(n)]))
    freqw = dist[1:].double() / dist[1:].sum().clamp_min(1).double()
    out.append("fwIoU: {}".format((c_iou[1:].cpu().double() * freqw).sum().item()))
    out.append("---- confusion matrix original data -----")
    out.append("\n" + _table([" "] + [str(j) for j in range(n)],
                             [[str(i)] + [int(v) for v in conf[i].tolist()] for i in range(n)]))
    for what, data in (("ACC", conf.float() / (conf.sum(1, keepdim=True).float() + 1e-8)),
                       ("Recall", conf.float() / (conf.sum(0, keepdim=True).float() + 1e-8))):
        out.append("---- {} matrix ----------------".format(what))
        out.append("\n" + _table([" "] + [names[j] for j in range(1, n)],
                                 [[names[i]] + ["{:0.1f}".format(data[i, j].item() * 100) for j in range(1, n)]
                                  for i in range(1, n)]))
    out.append(source_line(counts))
    return out


def source_line(counts):
    c = [int(v) for v in counts]
    t = max(sum(c), 1)
    return "Label source: main {:.4f} ({}), sub {:.4f} ({}), filled {:.4f} ({}) of {} points".format(
        c[0] / t, c[0], c[1] / t, c[1], c[2] / t, c[2], sum(c))


class MergePred(object):
    def __init__(self, settings, recorder, dataset=None):
        self.settings, self.recorder = settings, recorder
        self.nus_loader = self._initDataloader(dataset)
        self.prediction_path = os.path.join(settings.save_path, "preds")
        self.device = torch.device("cuda")
        # confusion matrix and source counts on the device: every batch's launch adds to them in place
        self.evaluator = pc_processor.metrics.IOUEval(n_classes=settings.n_classes, device=self.device, ignore=[0])
        self.counts = torch.zeros(3, dtype=torch.int64, device=self.device)
        self.data_split = "val" if settings.has_label else "test"
        self.submission_json = {"meta": dict(SUBMISSION_META)}

    def _initDataloader(self, dataset):
        s = self.settings
        if dataset is None:
            if s.dataset not in ("NuScenes", "nuScenes"):
                raise ValueError("invalid dataset: {}".format(s.dataset))
            if s.is_debug:
                version, split = "v1.0-mini", "val"
            elif s.has_label:
                version, split = "v1.0-trainval", "val"
            else:
                version, split = "v1.0-test", "test"
            dataset = pc_processor.dataset.nuScenes.open_nuscenes(False, s.data_root, version, split, has_image=False,
                                                                  splits_path=s.config.get("nus_splits"))
        return dataset

    def _batch(self, idx, lut):
        """the sweeps idx through the device -> uint8 labels of all of them, concatenated, on the host"""
        s, ds = self.settings, self.nus_loader
        main, sub, sem = [], [], []
        for i in idx:
            token = ds.token_list[i]
            m, b = read_pair(s.main_pred_folder, s.sub_pred_folder, self.data_split, token, s.main_pred_dtype,
                             s.sub_pred_dtype)
            main.append(m)
            sub.append(b)
            if s.has_label:
                raw = np.asarray(ds.loadLabelByIndex(i)).reshape(-1).astype(np.int32)
                if raw.shape[0] != m.shape[0]:
                    raise ValueError("sweep {}: {} predicted points, {} annotated points".format(
                        token, m.shape[0], raw.shape[0]))
                sem.append(raw)
        parts = [np.concatenate(main), np.concatenate(sub)] + ([np.concatenate(sem)] if s.has_label else [])
        up = upload_packed(parts, self.device)                                   # one host -> device copy per batch
        out = torch.empty(up[0].shape[0], dtype=torch.uint8, device=self.device)
        pc_processor.postproc.fill_labels(
            up[0], up[1], s.n_classes, fill_class=s.fill_class, sem=up[2] if s.has_label else None,
            lut=lut if s.has_label else None, conf=self.evaluator.conf_matrix if s.has_label else None,
            counts=self.counts, out_u8=out)
        if s.has_label:
            self.evaluator.external_update()
        return out.cpu().numpy(), [m.shape[0] for m in main]                      # one device -> host copy per batch

    def run(self):
        s = self.settings
        log = self.recorder.logger.info
        self.evaluator.reset()
        self.counts.zero_()
        ds = self.nus_loader
        lut = torch.from_numpy(label_lut(ds)).to(self.device) if s.has_label else None
        out_dir = os.path.join(self.prediction_path, "lidarseg", self.data_split)
        os.makedirs(out_dir, exist_ok=True)
        n, bs = len(ds), s.merge_batch_size
        written = {}
        t_start = time.time()
        for first in range(0, n, bs):
            t0 = time.time()
            idx = list(range(first, min(first + bs, n)))
            host, sizes = self._batch(idx, lut)
            o = 0
            for i, k in zip(idx, sizes):
                path = os.path.join(out_dir, "{}_lidarseg.bin".format(ds.token_list[i]))
                host[o:o + k].tofile(path)
                written[ds.token_list[i]] = path
                o += k
            msg = "Iter [{:04d}|{:04d}] Datatime: {:0.3f} ProcessTime: {:0.3f}".format(
                idx[-1], n, t0 - t_start, time.time() - t0)
            if s.has_label:
                msg += " meanIOU {:0.4f}".format(self.evaluator.getIoU()[0].item())
            log(msg)
            t_start = time.time()
            if s.is_debug and idx[-1] > 10:
                break
        json_dir = os.path.join(self.prediction_path, self.data_split)
        os.makedirs(json_dir, exist_ok=True)
        with open(os.path.join(json_dir, "submission.json"), "w") as f:
            json.dump(self.submission_json, f, ensure_ascii=False, indent=4)
        counts = self.counts.cpu().tolist()
        if not s.has_label:
            log(source_line(counts))
            return written
        for line in report_lines(self.evaluator, ds.mapped_cls_name, s.n_classes, counts):
            log(line)
        return written


class Experiment(object):
    def __init__(self, settings, dataset=None):
        self.settings = settings
        os.environ["CUDA_VISIBLE_DEVICES"] = settings.gpu       # as the reference: before the first CUDA call of the process
        settings.check_path()
        torch.cuda.set_device(0)
        self.recorder = pc_processor.checkpoint.Recorder(settings, settings.save_path, use_tensorboard=False)
        self.merge_pred = MergePred(settings, self.recorder, dataset=dataset)

    def run(self):
        t0 = time.time()
        out = self.merge_pred.run()
        self.recorder.logger.info("==== total cost time: {}".format(datetime.timedelta(seconds=time.time() - t0)))
        return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description="nuScenes full-sweep merge on MI355X")
    ap.add_argument("config_path", type=str, metavar="config_path")
    ap.add_argument("--id", type=int, default=0)
    args = ap.parse_args()
    exp = Experiment(Option(args.config_path))
    print("===init env success===")
    exp.run()
