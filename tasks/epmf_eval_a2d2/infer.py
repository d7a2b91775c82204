"""Pixel-wise EPMF evaluation on the A2D2 test split (counterpart of the reference's tasks/epmf_eval_a2d2/infer.py).

The reference script builds ``pc_processor.dataset.a2d2.A2D2`` and wraps it in ``pc_processor.dataset.a2d2.A2D2EvalLoader``;
neither name exists in the reference (its a2d2 package exports ``A2D2_PV`` only), so the script cannot run as it stands.  What
it slices out of an item -- channels 0-7 features, 8 mask, 9 label -- is the layout of PerspectiveViewLoaderV2(is_train=False),
and that is what runs here, on ``A2D2_PV(split='test')``.

Per frame: the loader's [10, proj_h, proj_w] item (PNG decode on the host; undistortion, label lookup and projection on the
device) -> normalisation (pmf_eval_pre, no padding: proj_h and proj_w are the network's input size) -> EPMFNet (HIP plan,
eval) -> argmax and confusion in one pass on the device (pmf_eval_argmax).  The confusion matrix comes to the host once,
after the loop, so the per-frame log line carries the times only, not the running mean IoU.  Then the reference's report:
Acc / IoU / Recall (mean and per class), the LaTeX row, the point distribution, fwIoU, the confusion matrix and its row- and
column-normalised forms.  Honours has_label (no labels: forward only, no report) and is_debug (one frame).

    python infer.py config.yaml
"""
import argparse
import datetime
import os
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
import pc_processor  # noqa: E402
from pmf_amd.postproc.frame_eval import eval_pre, window_argmax  # noqa: E402
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
    def __init__(self, settings, model, recorder):
        self.settings, self.recorder = settings, recorder
        self.model = model.cuda()
        self.val_loader = self._initDataloader()
        dev = torch.device("cuda")
        pv = settings.config["PVconfig"]
        self.mean = torch.tensor(pv["pcd_mean"], dtype=torch.float32).to(dev)
        self.stds = torch.tensor(pv["pcd_stds"], dtype=torch.float32).to(dev)
        # on the device: pmf_eval_argmax adds each frame to it in place
        self.evaluator = pc_processor.metrics.IOUEval(n_classes=settings.n_classes, device=dev, ignore=[0])

    def _initDataloader(self):
        s = self.settings
        if s.dataset != "a2d2":
            raise ValueError("invalid dataset: {}".format(s.dataset))
        dataset = pc_processor.dataset.a2d2.A2D2_PV(
            root=s.data_root, camsLidars_path=s.cams_lidars_path, classIndex_path=s.class_index_path, split="test",
            has_label=s.has_label, **(s.config.get("a2d2_subset") or {}))
        return pc_processor.dataset.PerspectiveViewLoaderV2(dataset=dataset, config=s.config, is_train=False)

    @torch.no_grad()
    def run(self, keep_outputs=None):
        """keep_outputs: a list that receives (item, prediction) of every frame (tests)"""
        s = self.settings
        log = self.recorder.logger.info
        self.model.eval()
        self.evaluator.reset()
        n = len(self.val_loader)
        t_start = time.time()
        for i in range(n):
            t0 = time.time()
            item = self.val_loader[i]                                   # [10, proj_h, proj_w] on the device
            _, h, w = item.shape
            pcd, rgb, _, _ = eval_pre(item, self.mean, self.stds, geometry=lambda hh, ww: (hh, ww, 0, 0))
            pred, _ = self.model(pcd, rgb)
            if s.has_label:
                window_argmax(pred, 0, 0, h, w, label=item[9], conf=self.evaluator.conf_matrix, want_map=False)
                self.evaluator.external_update()
            if keep_outputs is not None:
                keep_outputs.append((item, pred.clone()))
            if (i + 1) % max(int(s.print_frequency), 1) == 0 or i == n - 1 or s.is_debug:
                torch.cuda.synchronize()
                log("Iter [{:04d}|{:04d}] Datatime: {:0.3f} ProcessTime: {:0.3f}".format(i, n, t0 - t_start, time.time() - t0))
            t_start = time.time()
            if s.is_debug:
                break
        if s.has_label:
            self.report()

    def report(self):
        log = self.recorder.logger.info
        names = self.val_loader.dataset.mapped_class_name
        n = self.settings.n_classes
        ev = pc_processor.metrics.IOUEval(n_classes=n, device=torch.device("cpu"), ignore=[0])
        ev.conf_matrix = self.evaluator.conf_matrix.cpu()               # the one copy
        m_acc, c_acc = ev.getAcc()
        m_rec, c_rec = ev.getRecall()
        m_iou, c_iou = ev.getIoU()
        log("============== Pixel-wise Evaluation Results (2D eval) ===================")
        log("Acc avg: {:.4f}, IOU avg: {:.4f}, Recall avg: {:.4f}".format(m_acc.item(), m_iou.item(), m_rec.item()))
        log("\n" + _table(["ClassIdx", "class_name", "IOU", "Acc", "Recall"],
                          [[i, names[i], "%.4f" % c_iou[i].item(), "%.4f" % c_acc[i].item(), "%.4f" % c_rec[i].item()]
                           for i in range(1, n)]))
        log("---- Latext Format String -----")
        log("".join(" & {:0.1f}".format(c_iou[i].item() * 100) for i in range(1, n)) +
            " & {:0.1f}".format(m_iou.item() * 100))
        conf = ev.conf_matrix.clone()
        conf[0] = 0
        conf[:, 0] = 0
        dist = conf.sum(0)
        total = max(int(dist.sum().item()), 1)
        log("---- Data Distribution -----")
        log("\n" + _table(["Class Name", "Number of points", "Percentage"],
                          [[names[i], int(dist[i].item()), "%.4f" % (int(dist[i].item()) / total)] for i in range(n)]))
        freqw = dist[1:].double() / dist[1:].sum().clamp_min(1).double()
        log("fwIoU: {}".format((c_iou[1:].double() * freqw).sum().item()))
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
    def __init__(self, settings):
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
        self.inference = Inference(settings, self.model, self.recorder)

    def run(self):
        t0 = time.time()
        self.inference.run()
        self.recorder.logger.info("==== total cost time: {}".format(datetime.timedelta(seconds=time.time() - t0)))


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description="EPMF inference on A2D2, MI355X")
    ap.add_argument("config_path", type=str, metavar="config_path")
    ap.add_argument("--id", type=int, default=0)
    args = ap.parse_args()
    exp = Experiment(Option(args.config_path))
    print("===init env success===")
    exp.run()
