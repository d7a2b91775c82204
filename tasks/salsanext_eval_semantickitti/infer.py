"""Point-wise SalsaNext evaluation on the raw SemanticKITTI sequences: every point of every sweep gets a label.

The structure is that of tasks/salsanext_eval_nuscenes/infer.py: eval_batch_size sweeps go through SalsaNext per forward
(SalsaNextLoader._eval_item: one loadDataByIndex per sweep, raw labels and the label table on the device), everything behind
the network is ONE batched pass of two launches (pmf_eval_range_batch through RangeSweepEvaluator: argmax + pixel confusion,
then per point the label at its pixel or the KNN vote, int32 labels + point confusion), the classes become annotation ids
on the device (class_map_lut_inv), and one device-to-host copy per batch carries all its sweeps.  Files:
<save_path>/preds/sequences/<seq>/predictions/<frame>.label, int32 annotation ids, one per point of the raw sweep -- the
benchmark's layout, and the sub_pred_folder of tasks/pmf_eval_semantickitti/fullsweep_eval.  The last batch may be short.
The loader scores with the WHOLE class_map_lut: SemanticKITTI's moving classes have raw ids 252..259, beyond the 256 entries
the loader keeps by default.  The report is the nuScenes task's (its report_lines).

    python infer.py config_server_kitti.yaml
"""
import argparse
import datetime
import importlib.util
import os
import sys
import time

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
import pc_processor  # noqa: E402
from option import Option  # noqa: E402


def _sibling(name, *path):
    """a module of another task directory, loaded by path under a name of its own (the tasks import `option` by its bare name)"""
    spec = importlib.util.spec_from_file_location(name, os.path.join(HERE, "..", *path))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


report_lines = _sibling("salsanext_eval_nuscenes_infer", "salsanext_eval_nuscenes", "infer.py").report_lines


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
        # class -> annotation id, applied on the device before the copy back
        self.lut_inv = torch.from_numpy(self.salsa_loader.dataset.class_map_lut_inv).to(dev, torch.int32)
        if self.knn_flag:
            self.recorder.logger.info("using KNN Post Process")

    def _initDataloader(self, dataset):
        s = self.settings
        if dataset is None:
            if s.dataset != "SemanticKitti":
                raise ValueError("invalid dataset: {}".format(s.dataset))
            cfg_path = s.data_config_path or pc_processor.dataset.semantic_kitti.DEFAULT_CONFIG
            dataset = pc_processor.dataset.semantic_kitti.SemanticKitti(
                root=s.data_root, sequences=list(s.sequences), config_path=cfg_path, has_label=s.has_label, has_image=False)
        # the whole table: raw ids 256..259 (moving classes) keep their class
        return pc_processor.dataset.SalsaNextLoader(dataset=dataset, config=s.config, data_len=s.data_len, is_train=False,
                                                    return_uproj=True, label_lut=dataset.class_map_lut)

    @torch.no_grad()
    def run(self):
        s = self.settings
        log = self.recorder.logger.info
        self.model.eval()
        self.evaluator.reset()
        self.pixel_eval.reset()
        ds = self.salsa_loader.dataset
        n, bs = len(self.salsa_loader), s.eval_batch_size
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
            # classes -> annotation ids on the device, then one device-to-host copy per batch: all its sweeps, in order
            host = self.lut_inv[self.range_eval.labels.long()].cpu().numpy()
            o = 0
            for i, l in zip(idx, labels):
                k = int(l.shape[0])
                written[ds.parsePathInfoByIndex(i)] = pc_processor.dataset.semantic_kitti.write_prediction(
                    ds, i, host[o:o + k], self.prediction_path, original_ids=True)
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
        os.environ["CUDA_VISIBLE_DEVICES"] = settings.gpu       # before the first CUDA call of the process
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
    ap = argparse.ArgumentParser(description="SalsaNext SemanticKITTI inference on MI355X")
    ap.add_argument("config_path", type=str, metavar="config_path")
    ap.add_argument("--id", type=int, default=0)
    args = ap.parse_args()
    exp = Experiment(Option(args.config_path))
    print("===init env success===")
    exp.run()
