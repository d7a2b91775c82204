"""Full-sweep SemanticKITTI result from two prediction folders (the counterpart of tasks/pmf_eval_nuscenes/testset_eval/main.py).

main_pred_folder holds the camera + LiDAR network's labels (the preds folder of tasks/pmf_eval_semantickitti): one annotation
id per point the left colour camera sees, in file order -- the points of the SemanticKITTI-FOV tree, or equally the loader's
keep mask on the raw tree.  sub_pred_folder holds the LiDAR-only network's (tasks/salsanext_eval_semantickitti): one id per
point of the raw sweep.  Per point of the raw sweep: the main label where the point is in the camera's view and the label maps
to a class other than 0, else the sub label, and what is still unlabelled becomes fill_class (road); with labels ALL points
are scored.  merge_batch_size frames of one sequence go through the device per call: their files are read on the host, the
image size comes from the PNG header, one packed upload, one pmf_kitti_full_fill call (labels + kept rows per frame +
confusion + source counts), one device-to-host copy (pc_processor.postproc.fov_fill).  A main file that does not hold one
label per point the camera sees is an error naming the frame: predictions of the EPMF evaluation follow another keep rule
(the yaw window of the V2 loader) and are refused that way.
Output: <save_path>/sequences/<seq>/predictions/<frame>.label, int32 annotation ids, the benchmark's submission layout; then
the report of the nuScenes task (its report_lines) and the share of points by source.  check_valid.py validates the folder.

    python main.py config_server.yaml
"""
import argparse
import datetime
import importlib.util
import os
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "..", ".."))
import pc_processor  # noqa: E402
from option import Option  # noqa: E402


def _sibling(name, *path):
    """a module of another task directory, loaded by path under a name of its own (the tasks import `option` by its bare name)"""
    spec = importlib.util.spec_from_file_location(name, os.path.join(HERE, "..", "..", *path))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


_nus = _sibling("pmf_eval_nuscenes_testset_main", "pmf_eval_nuscenes", "testset_eval", "main.py")
report_lines, source_line = _nus.report_lines, _nus.source_line


def pred_file(folder, seq, frame):
    return os.path.join(folder, "sequences", seq, "predictions", "{}.label".format(frame))


def read_words(path, seq, frame, what):
    """one .label file -> uint32 words"""
    if not os.path.isfile(path):
        raise FileNotFoundError("no {} for sequence {} frame {}: {}".format(what, seq, frame, path))
    if os.path.getsize(path) % 4:
        raise ValueError("sequence {} frame {}: {} is not a whole number of 32-bit labels".format(seq, frame, path))
    return np.fromfile(path, dtype=np.uint32)


def image_size(path):
    """(h, w) from the PNG header, nothing is decoded"""
    from PIL import Image
    with Image.open(path) as im:
        w, h = im.size
    return h, w


def open_dataset(settings):
    cfg_path = settings.data_config_path or pc_processor.dataset.semantic_kitti.DEFAULT_CONFIG
    return pc_processor.dataset.semantic_kitti.SemanticKitti(
        root=settings.data_root, sequences=list(settings.sequences), config_path=cfg_path, has_label=settings.has_label,
        has_image=True)


def batches(dataset, batch_size):
    """index lists of at most batch_size frames, in order, none spanning two sequences"""
    out, cur, cur_seq = [], [], None
    for i in range(len(dataset)):
        seq = dataset.parsePathInfoByIndex(i)[0]
        if cur and (seq != cur_seq or len(cur) == batch_size):
            out.append(cur)
            cur = []
        cur.append(i)
        cur_seq = seq
    return out + ([cur] if cur else [])


class MergePred(object):
    def __init__(self, settings, recorder, dataset=None):
        self.settings, self.recorder = settings, recorder
        self.dataset = dataset if dataset is not None else open_dataset(settings)
        self.device = torch.device("cuda")
        # confusion matrix and source counts on the device: every batch's call adds to them in place
        self.evaluator = pc_processor.metrics.IOUEval(n_classes=settings.n_classes, device=self.device, ignore=[0])
        self.counts = torch.zeros(3, dtype=torch.int64, device=self.device)

    def _batch(self, idx):
        """the frames idx (one sequence) through the device -> list of uint32 annotation ids per frame"""
        s, ds = self.settings, self.dataset
        seq = ds.parsePathInfoByIndex(idx[0])[0]
        frames, dims, main, sub, gt = [], [], [], [], []
        for i in idx:
            _, frame = ds.parsePathInfoByIndex(i)
            pts = np.fromfile(ds.pointcloud_files[i], dtype=np.float32)
            if pts.size % 4:
                raise ValueError("{}: {} floats are no whole number of x, y, z, intensity rows".format(
                    ds.pointcloud_files[i], pts.size))
            pts = pts.reshape(-1, 4)
            frames.append(pts)
            dims.append(image_size(ds.image_files[i]))
            main.append(read_words(pred_file(s.main_pred_folder, seq, frame), seq, frame, "main prediction"))
            b = read_words(pred_file(s.sub_pred_folder, seq, frame), seq, frame, "sub prediction")
            if b.shape[0] != pts.shape[0]:
                raise ValueError("sequence {} frame {}: the sweep has {} points, the sub prediction {}".format(
                    seq, frame, pts.shape[0], b.shape[0]))
            sub.append(b)
            if s.has_label:
                raw = read_words(ds.label_files[i], seq, frame, "label file")
                if raw.shape[0] != pts.shape[0]:
                    raise ValueError("sequence {} frame {}: the sweep has {} points, the label file {}".format(
                        seq, frame, pts.shape[0], raw.shape[0]))
                gt.append(raw)
        try:
            out = pc_processor.postproc.fov_fill(
                frames, dims, ds.proj_matrix[seq], main, sub, ds.class_map_lut, int(ds.class_map_lut_inv[s.fill_class]),
                s.n_classes, gt=gt if s.has_label else None,
                conf=self.evaluator.conf_matrix if s.has_label else None, counts=self.counts)
        except ValueError as e:
            raise ValueError("sequence {}, frames {} .. {} (frame numbers of the message count from the first): {}".format(
                seq, ds.parsePathInfoByIndex(idx[0])[1], ds.parsePathInfoByIndex(idx[-1])[1], e))
        if s.has_label:
            self.evaluator.external_update()
        return out

    def run(self):
        s, ds = self.settings, self.dataset
        log = self.recorder.logger.info
        self.evaluator.reset()
        self.counts.zero_()
        written = {}
        n = len(ds)
        t_start = time.time()
        for idx in batches(ds, s.merge_batch_size):
            t0 = time.time()
            for i, lab in zip(idx, self._batch(idx)):
                written[ds.parsePathInfoByIndex(i)] = pc_processor.dataset.semantic_kitti.write_prediction(
                    ds, i, lab, s.save_path, original_ids=True)
            msg = "Iter [{:04d}|{:04d}] Datatime: {:0.3f} ProcessTime: {:0.3f}".format(
                idx[-1], n, t0 - t_start, time.time() - t0)
            if s.has_label:
                msg += " meanIOU {:0.4f}".format(self.evaluator.getIoU()[0].item())
            log(msg)
            t_start = time.time()
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
        os.environ["CUDA_VISIBLE_DEVICES"] = settings.gpu       # before the first CUDA call of the process
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
    ap = argparse.ArgumentParser(description="SemanticKITTI full-sweep merge on MI355X")
    ap.add_argument("config_path", type=str, metavar="config_path")
    ap.add_argument("--id", type=int, default=0)
    args = ap.parse_args()
    exp = Experiment(Option(args.config_path))
    print("===init env success===")
    exp.run()
