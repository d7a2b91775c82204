"""tests/golden/g18_nus_fill.npz: the reference's MergePred._mergeResult (tasks/pmf_eval_nuscenes/testset_eval/main.py) and
its IOUEval(17, ignore=[0]) executed on the three synthetic sweeps of tests/nus_fill_cases.py.

    python tools/make_golden_nus_fill.py /path/to/reference

The reference's main.py is imported by file path with stub ``option`` and ``prettytable`` modules in sys.modules (its own
option.py wants a config file, prettytable is not a dependency of this repository).  Arrays only: per sweep main, sub, the raw
annotation ids, the fused uint8 labels; over the three sweeps the confusion matrix and the three source counts."""
import importlib.util
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import nus_fill_cases as F  # noqa: E402


def _load(modname, path):
    spec = importlib.util.spec_from_file_location(modname, path)
    m = importlib.util.module_from_spec(spec)
    sys.modules[modname] = m
    spec.loader.exec_module(m)
    return m


def main(ref):
    opt = types.ModuleType("option")
    opt.Option = object
    sys.modules["option"] = opt
    pt = types.ModuleType("prettytable")
    pt.PrettyTable = object
    sys.modules["prettytable"] = pt
    M = _load("ref_testset_eval_main", os.path.join(ref, "tasks", "pmf_eval_nuscenes", "testset_eval", "main.py"))
    IOU = _load("ref_iou_eval", os.path.join(ref, "pc_processor", "metrics", "iou_eval.py"))
    C = F.NCLASSES
    ev = IOU.IOUEval(C, ignore=[0])
    lut = F.label_lut(C).astype(np.int64)
    out, counts = {}, np.zeros(3, np.int64)
    for i in range(len(F.COUNTS)):
        main_pred, sub_pred, sem = F.sweep_case(i)
        pred = M.MergePred._mergeResult(None, main_pred, sub_pred)
        ev.addBatch(pred, lut[sem])
        from_main = main_pred != 0
        from_sub = np.logical_and(~from_main, sub_pred != 0)
        filled = np.logical_and(~from_main, sub_pred == 0)
        c = np.array([from_main.sum(), from_sub.sum(), filled.sum()], np.int64)
        assert c.min() > 0 and c.sum() == main_pred.shape[0], c                      # all three sources in every sweep
        assert (main_pred == 0).mean() >= 0.4, (main_pred == 0).mean()
        assert np.all(pred[filled] == 11) and np.all(pred != 0)
        counts += c
        out.update({"s%d.main" % i: main_pred, "s%d.sub" % i: sub_pred, "s%d.sem" % i: sem,
                    "s%d.fused" % i: pred.astype(np.uint8)})
    out["conf"] = ev.conf_matrix.numpy().astype(np.int64)
    out["counts"] = counts
    np.savez_compressed(F.GOLDEN, **out)
    print("g18_nus_fill: %d points, counts %s, %d bytes" % (int(counts.sum()), counts.tolist(), os.path.getsize(F.GOLDEN)))


if __name__ == "__main__":
    main(sys.argv[1])
