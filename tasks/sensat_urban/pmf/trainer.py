"""Trainer of the SensatUrban PMF task (counterpart of the reference's tasks/sensat_urban/pmf/trainer.py:14-538).

Same constructor / ``run(epoch, mode)`` contract: SensatUrban(train) and SensatUrban(val, use_crop=True) behind two
SensatLoaders (:99-126), the SensatUrban focal weights (:174-181), AdamW(amsgrad) over the LiDAR stream + SGD-Nesterov over
the camera stream (:79-97), two WarmupCosineLR (:62-74), two IOUEval (:50-60); ``run`` returns {"Acc", "IOU", "Recall",
"last"} (:530-535).  The per-iteration work (:275-340, :342-376) is pmf_amd.engine.SensatEngine.

Differences that do not change what is computed:
  * SensatLoader gathers the items on the device (csrc/bev_train.hip), so the loaders are its ``batches`` iterators and not
    torch DataLoaders with worker processes; a DistributedSampler plugs into them as it does into a DataLoader;
  * the meters of the reference (loss, focal + Dice, Lovasz, entropy of both heads, perception) are summed on the device
    every iteration and read at the print frequency -- one host sync per log line, not nine .item() calls per iteration;
  * scalars go to the Recorder (tensorboard only if tensorboardX is installed); the per-epoch image logging is left out."""
import datetime
import math
import time

import torch

import pc_processor
from pmf_amd.engine import SensatEngine, sensat_focal_alpha

# the reference's meters, in logging order: tensorboard tag -> how to read it from the engine's terms
METERS = ("Loss", "LossFocal", "LossLovasz", "entropy", "LossImageFocal", "LossImageLovasz", "ImageEntropy", "LossPerception")


class _Engine(SensatEngine):
    """SensatEngine that also keeps the mean normalised entropy of both heads of the last iteration (trainer.py:291-305),
    which the reference logs and the fused objective does not report"""

    def forward_loss(self, pcd, rgb, label):
        out = super().forward_loss(pcd, rgb, label)
        with torch.no_grad():
            norm = math.log(self.nclasses)
            self.last_entropy = [(-(p * torch.log(p.clamp(min=1e-8))).sum(1) / norm).mean() for p in (out[2], out[3])]
        return out


class Trainer(object):
    def __init__(self, settings, model, recorder=None):
        self.settings, self.recorder = settings, recorder
        self.model = model.cuda()
        self.remain_time = pc_processor.utils.RemainTime(settings.n_epochs)
        self.train_loader, self.val_loader, self.train_sampler, self.val_sampler = self._initDataloader()
        s, total = settings, len(self.train_loader)
        self.engine = _Engine(
            self.model, s.nclasses, lr=s.lr, momentum=s.momentum, weight_decay=s.weight_decay, ignore_class=self.ignore_class,
            warmup_steps=s.warmup_epochs * total, max_steps=total * (s.n_epochs - s.warmup_epochs),
            feature_mean=s.feature_mean, feature_std=s.feature_std,
            distributed=s.distributed and s.world_size > 1, device_ids=[s.gpu] if s.distributed else None)
        if recorder is not None:
            recorder.logger.info("focal_loss alpha: {}".format(sensat_focal_alpha(s.nclasses)))
        # main.py reads / restores these two: reference checkpoint layout on top of the flat state
        self.optimizer, self.aux_optimizer = self.engine.optimizer_view, self.engine.aux_optimizer_view
        self.metrics, self.metrics_img = self.engine.metrics, self.engine.metrics_img
        self.scheduler, self.aux_scheduler = self.engine.scheduler, self.engine.aux_scheduler
        self.last_summary = {}

    def _initDataloader(self):
        s = self.settings
        if s.dataset != "SensatUrban":
            raise ValueError("invalid dataset: {}".format(s.dataset))
        trainset = pc_processor.dataset.SensatUrban(root_path=s.data_root, split="train", keep_idx=False)
        self.ignore_class = [0]
        self.mapped_cls_name = trainset.mapped_cls_name
        valset = pc_processor.dataset.SensatUrban(root_path=s.data_root, split="val", keep_idx=False, use_crop=True,
                                                  img_h=s.val_img_h, img_w=s.val_img_w)
        train_items = pc_processor.dataset.SensatLoader(dataset=trainset, img_h=s.img_h, img_w=s.img_w,
                                                        n_samples_split=s.n_samples_split)
        val_items = pc_processor.dataset.SensatLoader(dataset=valset)
        tsamp = vsamp = None
        if s.distributed and s.world_size > 1:
            tsamp = torch.utils.data.distributed.DistributedSampler(train_items, shuffle=True, drop_last=True)
            vsamp = torch.utils.data.distributed.DistributedSampler(val_items, shuffle=False, drop_last=False)
        return (train_items.batches(s.batch_size[0], shuffle=True, drop_last=True, sampler=tsamp),
                val_items.batches(s.batch_size[1], shuffle=False, drop_last=False, sampler=vsamp), tsamp, vsamp)

    def run(self, epoch, mode="Train"):
        s, eng = self.settings, self.engine
        if mode == "Train":
            loader, step = self.train_loader, eng.train_step
            if self.train_sampler is not None:
                self.train_sampler.set_epoch(epoch)
        elif mode == "Validation":
            loader, step = self.val_loader, eng.eval_step
        else:
            raise ValueError("invalid mode: {}".format(mode))
        self.metrics.reset()
        self.metrics_img.reset()
        sums = torch.zeros(len(METERS), dtype=torch.float64, device="cuda")        # sum of (meter x batch)
        count = 0
        total_iter = len(loader)
        t_start = time.time()
        lr = self.optimizer.param_groups[0]["lr"]
        for i, (input_feature, input_label) in enumerate(loader):
            t0 = time.time()
            total, terms = step(input_feature, input_label)
            m = eng.meter_values(terms)
            sums += torch.stack([total.detach(), m["LossFocal"], m["LossLovasz"], eng.last_entropy[0], m["LossFocal_img"],
                                 m["LossLovasz_img"], eng.last_entropy[1], m["LossPerception"]]).detach().double() \
                * input_feature.size(0)
            count += input_feature.size(0)
            if (i + 1) % max(int(s.print_frequency), 1) == 0 or i + 1 == total_iter or s.is_debug:      # the host syncs
                avg = dict(zip(METERS, (sums / count).tolist()))
                miou, _ = self.metrics.getIoU()
                macc, _ = self.metrics.getAcc()
                mrec, _ = self.metrics.getRecall()
                miou_i, _ = self.metrics_img.getIoU()
                macc_i, _ = self.metrics_img.getAcc()
                mrec_i, _ = self.metrics_img.getRecall()
                self.remain_time.update(cost_time=(time.time() - t_start), mode=mode)
                rt = datetime.timedelta(seconds=int(self.remain_time.getRemainTime(epoch, i, total_iter, mode)))
                lr = self.optimizer.param_groups[0]["lr"]
                if self.recorder is not None:
                    self.recorder.logger.info(
                        ">>> {} E[{:03d}|{:03d}] I[{:04d}|{:04d}] DT[{:.3f}] PT[{:.3f}] "
                        "LR {:0.5f} Loss {:0.4f} Acc {:0.4f} IOU {:0.4F} Recall {:0.4f} Entropy {:0.4f} "
                        "ImgAcc {:0.4f} ImgIOU {:0.4F} ImgRecall {:0.4f} ImgEntropy {:0.4f} RT {}".format(
                            mode, s.n_epochs, epoch + 1, total_iter, i + 1, t0 - t_start, time.time() - t0,
                            lr, total.item(), macc.item(), miou.item(), mrec.item(), avg["entropy"],
                            macc_i.item(), miou_i.item(), mrec_i.item(), avg["ImageEntropy"], rt))
            t_start = time.time()
            if s.is_debug:
                break
        avg = dict(zip(METERS, (sums / max(count, 1)).tolist()))
        miou, ciou = self.metrics.getIoU()
        macc, cacc = self.metrics.getAcc()
        mrec, crec = self.metrics.getRecall()
        miou_i, ciou_i = self.metrics_img.getIoU()
        macc_i, _ = self.metrics_img.getAcc()
        mrec_i, _ = self.metrics_img.getRecall()
        if self.recorder is not None:
            tb = self.recorder.tensorboard
            for k, v in avg.items():
                tb.add_scalar("{}_{}".format(mode, k), v, epoch)
            tb.add_scalar("{}_lr".format(mode), lr, epoch)
            for k, v in (("meanAcc", macc), ("meanIOU", miou), ("meanRecall", mrec), ("Image_meanAcc", macc_i),
                         ("Image_meanIOU", miou_i), ("Image_meanRecall", mrec_i)):
                tb.add_scalar("{}_{}".format(mode, k), v.item(), epoch)
            for c, (_, name) in enumerate(self.mapped_cls_name.items()):         # -1: ignore -> class 0 of the network
                tb.add_scalar("{}_{:02d}_{}_Acc".format(mode, c, name), cacc[c].item(), epoch)
                tb.add_scalar("{}_{:02d}_{}_Recall".format(mode, c, name), crec[c].item(), epoch)
                tb.add_scalar("{}_{:02d}_{}_IOU".format(mode, c, name), ciou[c].item(), epoch)
                tb.add_scalar("{}_{:02d}_{}_ImageIOU".format(mode, c, name), ciou_i[c].item(), epoch)
            self.recorder.logger.info(">>> {} Loss {:0.4f} Acc {:0.4f} IOU {:0.4F} Recall {:0.4f}".format(
                mode, avg["Loss"], macc.item(), miou.item(), mrec.item()))
        self.last_summary = dict(avg, class_IOU=ciou.tolist(), ImgIOU=miou_i.item())
        return {"Acc": macc.item(), "IOU": miou.item(), "Recall": mrec.item(), "last": 0}
