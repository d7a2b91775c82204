"""tests/golden/g17_salsa_eval.npz: the per-sweep composition of the reference's tasks/salsanext_eval_nuscenes/infer.py:90-119
executed with the reference's own SalsaNextLoader / RangeProjection (return_uproj=True, is_train=False), KNN and IOUEval
on the synthetic LiDAR-only dataset and the probability maps by recipe of tests/salsa_eval_cases.py.

    python tools/make_golden_salsa_eval.py /path/to/reference

The reference modules are imported by file path.  Arrays only: per sweep the reference loader's outputs that the device
pass takes as inputs (px, py, depth, proj_range, label -- stored, not recomputed, because a device projection may put a
point that sits on a pixel boundary one pixel away), the int32 labels for gather and for KNN; the pixel confusion and the
two point confusions over the three sweeps.  The maps are NOT stored (prob_maps(seed) regenerates them).  The seed is
the first one for which the argmax rests on no tie, KNN changes >= 1 % of the labels, and no vote depends on the order
among equal distances (torch.topk leaves that order open)."""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import salsa_eval_cases as S  # noqa: E402


def _load(ref, modname, relpath):
    spec = importlib.util.spec_from_file_location(modname, os.path.join(ref, relpath))
    m = importlib.util.module_from_spec(spec)
    sys.modules[modname] = m
    spec.loader.exec_module(m)
    return m


def main(ref):
    for name in ("pc_processor", "pc_processor.dataset", "pc_processor.dataset.preprocess"):
        pkg = types.ModuleType(name)
        pkg.__path__ = []
        sys.modules[name] = pkg
    pre = sys.modules["pc_processor.dataset.preprocess"]
    pre.augmentor = _load(ref, "pc_processor.dataset.preprocess.augmentor", "pc_processor/dataset/preprocess/augmentor.py")
    pre.projection = _load(ref, "pc_processor.dataset.preprocess.projection", "pc_processor/dataset/preprocess/projection.py")
    SL = _load(ref, "refpc_salsanext_loader", "pc_processor/dataset/salsanext_loader.py")
    KNN = _load(ref, "refpc_knn", "pc_processor/postproc/knn.py")
    IOU = _load(ref, "refpc_iou_eval", "pc_processor/metrics/iou_eval.py")
    assert isinstance(SL.SalsaNextLoader(S.SyntheticSalsaNus(), S.CONFIG, is_train=False).projection,
                      pre.projection.RangeProjection)

    ds = S.SyntheticSalsaNus()
    ld = SL.SalsaNextLoader(ds, S.CONFIG, is_train=False, return_uproj=True)
    items = [ld[i] for i in range(len(ds))]
    C, B = S.NCLASSES, len(ds)
    knn = KNN.KNN(S.KNN_PARAMS, C)
    inv_gauss = (1 - KNN.get_gaussian_kernel(S.KNN_PARAMS["search"], S.KNN_PARAMS["sigma"], 1)).reshape(-1).numpy()
    for seed in range(17, 64):
        prob = S.prob_maps(seed, B)
        if S.top2_gap(prob) <= 0.0:          # (the bits of the maps are the same everywhere: any gap decides)
            continue
        out = {"seed": np.int64(seed)}
        pix = IOU.IOUEval(C, ignore=[0])
        pt_g, pt_k = IOU.IOUEval(C, ignore=[0]), IOU.IOUEval(C, ignore=[0])
        changed = total = 0
        stable = True
        for i, (_, label, _, rng, ux, uy, ud) in enumerate(items):
            pred = torch.from_numpy(prob[i:i + 1])
            pred_argmax = pred[0].argmax(dim=0)
            pix.addBatch(pred.argmax(dim=1), label[None].long())
            gather = pred_argmax[uy, ux].numpy().reshape(-1).astype(np.int32)
            voted = knn(rng, ud, pred_argmax, ux, uy).numpy().reshape(-1).astype(np.int32)
            args = (rng.numpy(), ud.numpy(), pred_argmax.numpy(), ux.numpy(), uy.numpy(), inv_gauss, C)
            fwd, rev = S.knn_vote_np(*args, **{k: S.KNN_PARAMS[k] for k in ("knn", "search", "cutoff")}), \
                S.knn_vote_np(*args, reverse=True, **{k: S.KNN_PARAMS[k] for k in ("knn", "search", "cutoff")})
            stable = stable and np.array_equal(fwd, rev) and np.array_equal(fwd, voted)
            sem = ds.labelMapping(ds.loadDataByIndex(i)[1])
            pt_g.addBatch(gather, sem)
            pt_k.addBatch(voted, sem)
            changed += int((gather != voted).sum())
            total += gather.shape[0]
            out.update({"s%d.px" % i: ux.numpy().astype(np.int32), "s%d.py" % i: uy.numpy().astype(np.int32),
                        "s%d.depth" % i: ud.numpy(), "s%d.proj_range" % i: rng.numpy(), "s%d.label" % i: label.numpy(),
                        "s%d.gather" % i: gather, "s%d.knn" % i: voted})
        if not stable:
            print("seed %d: a vote depends on the order among equal distances -- next seed" % seed)
            continue
        assert changed >= 0.01 * total, (changed, total)
        out.update({"pixel_conf": pix.conf_matrix.numpy(), "point_conf_gather": pt_g.conf_matrix.numpy(),
                    "point_conf_knn": pt_k.conf_matrix.numpy()})
        np.savez_compressed(S.GOLDEN, **out)
        print("g17_salsa_eval: seed %d, KNN changes %d of %d labels, %d bytes" % (seed, changed, total,
                                                                               os.path.getsize(S.GOLDEN)))
        return
    raise SystemExit("no seed qualified")


if __name__ == "__main__":
    main(sys.argv[1])
