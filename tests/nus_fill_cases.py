"""Shared pieces of the full-sweep fusion tests (TEST INFRASTRUCTURE, not a conftest): three synthetic sweeps by recipe, a
devkit-free dataset with what the merge task reads, and the numpy statement of the rule of the reference's
tasks/pmf_eval_nuscenes/testset_eval/main.py (MergePred: camera labels where non-zero, else the LiDAR-only labels, else one
fixed class; every point scored)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

NCLASSES = 17
FILL_CLASS = 11
COUNTS = (700, 900, 1100)                    # points per sweep: different sizes, none a multiple of the 256-lane workgroup
GOLDEN = os.path.join(ROOT, "tests", "golden", "g18_nus_fill.npz")


def class_table(nclasses=NCLASSES):
    """raw annotation id (32 of them, as nuScenes-lidarseg) -> class, by recipe; every class occurs, id 0 -> class 0"""
    rng = np.random.Generator(np.random.PCG64(4100 + nclasses))
    t = np.concatenate([np.arange(min(nclasses, 32)), rng.integers(0, nclasses, max(32 - nclasses, 0))])
    return {i: int(t[i]) for i in range(32)}


def label_lut(nclasses=NCLASSES):
    """the 256-entry int32 table the nuScenes tasks build from the dataset's mapping"""
    lut = np.zeros(256, np.int32)
    for k, v in class_table(nclasses).items():
        lut[k] = v
    return lut


def sweep_case(index, npts=None, nclasses=NCLASSES):
    """(main int32[P], sub int32[P], sem int32[P] raw ids) of synthetic sweep ``index``: main is 0 on ~55 % of the points
    (no camera sees them), sub is 0 on ~12 % of all points independently, so every sweep has points taken from main, taken
    from sub, and filled; all labels inside [0, nclasses)."""
    P = COUNTS[index] if npts is None else int(npts)
    rng = np.random.Generator(np.random.PCG64(4200 + index))
    main = rng.integers(1, nclasses, P).astype(np.int32)
    main[rng.random(P) < 0.55] = 0
    sub = rng.integers(1, nclasses, P).astype(np.int32)
    sub[rng.random(P) < 0.12] = 0
    sem = rng.integers(0, 32, P).astype(np.int32)
    return main, sub, sem


def fill_rule_np(main, sub, fill_class=FILL_CLASS):
    """-> (pred int64[P], source int64[P]: 0 from main, 1 from sub, 2 filled)"""
    main, sub = np.asarray(main).astype(np.int64), np.asarray(sub).astype(np.int64)
    pred = np.where(main != 0, main, sub)
    source = np.where(main != 0, 0, 1)
    filled = pred == 0
    return np.where(filled, fill_class, pred), np.where(filled, 2, source)


def fill_np(main, sub, sem, lut, nclasses=NCLASSES, fill_class=FILL_CLASS, base=None):
    """-> (uint8[P] labels, int64[C,C] confusion over ALL points with a label inside [0, C), int64[3] source counts);
    sem raw ids, ids outside the lut -> class 0"""
    pred, source = fill_rule_np(main, sub, fill_class)
    sem = np.asarray(sem).astype(np.int64).reshape(-1)
    lut = np.asarray(lut).astype(np.int64)
    inside = (sem >= 0) & (sem < lut.shape[0])
    gt = np.where(inside, lut[np.clip(sem, 0, lut.shape[0] - 1)], 0)
    ok = (pred >= 0) & (pred < nclasses) & (gt >= 0) & (gt < nclasses)
    conf = np.bincount(pred[ok] * nclasses + gt[ok], minlength=nclasses * nclasses).reshape(nclasses, nclasses)
    if base is not None:
        conf = conf + base
    return pred.astype(np.uint8), conf, np.bincount(source, minlength=3).astype(np.int64)


def miou_np(conf, ignore=0):
    """IOUEval.getIoU()[0] on an int64 confusion (rows = prediction, columns = ground truth)"""
    c = conf.astype(np.float64).copy()
    c[ignore] = 0
    c[:, ignore] = 0
    tp = np.diag(c)
    iou = tp / (c.sum(1) + c.sum(0) - tp + 1e-15)
    return float(np.delete(iou, ignore).mean())


class SyntheticNusSweeps(object):
    """What the merge task reads of pc_processor/dataset/nuScenes/dataset_nuscenes.py (has_image=False): token_list of plain
    strings, loadLabelByIndex -> uint8[P,1] raw ids, labelMapping, map_name_from_general_index_to_segmentation_index,
    mapped_cls_name.  Sweep i has counts[i] points; main_sub(i) gives the two predictions a test writes to files."""

    def __init__(self, counts=(1500, 1201, 1777, 900, 1310), nclasses=NCLASSES):
        self.counts, self.nclasses = tuple(counts), nclasses
        self.map_name_from_general_index_to_segmentation_index = class_table(nclasses)
        self.mapped_cls_name = {i: "class_%d" % i for i in range(nclasses)}
        self.token_list = ["sweep%03d" % i for i in range(len(counts))]

    def __len__(self):
        return len(self.token_list)

    def main_sub(self, index):
        main, sub, _ = sweep_case(100 + index, self.counts[index], self.nclasses)
        return main, sub

    def loadLabelByIndex(self, index):
        return sweep_case(100 + index, self.counts[index], self.nclasses)[2].astype(np.uint8)[:, None]

    def labelMapping(self, sem_label):
        return label_lut(self.nclasses).astype(np.int64)[np.asarray(sem_label)[:, 0]]
