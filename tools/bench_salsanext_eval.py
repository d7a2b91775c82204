#!/usr/bin/env python3
"""Per-sweep SalsaNext nuScenes evaluation pipeline (tasks/salsanext_eval_nuscenes) on synthetic sweeps of nuScenes size:
34 720 points per sweep (a 32-beam sweep of the public dataset), range images of 32 x 2048, 17 classes; everything is
generated from --seed.

Stages, per sweep, at B = 1 and B = --batch sweeps per forward: loader (SalsaNextLoader._eval_item: one upload, the HIP
range projection), forward (SalsaNext eval on the stacked features), post (RangeSweepEvaluator.post: the concatenation of
the ragged point arrays, pmf_eval_range_batch, and the ONE device-to-host copy of the batch's labels the task does).  The
yardstick is the reference's loop body composed from torch ops on the SAME network outputs, sweep by sweep: argmax,
IOUEval.addBatch on the pixels (host matrices, as the reference keeps them), KNN or fancy indexing, .cpu().numpy(),
IOUEval.addBatch on the points.  Labels and both confusion matrices of the two paths are compared.  In --knn mode the
yardstick's KNN is this project's pmf_knn_vote module (what a per-sweep loop here would call), which shares its device
code with the pass under test: that comparison checks the batching, the counting and the copies, not the vote.  The vote
itself is checked once per batch size, untimed, against the numpy oracle (oracle/knn_ref.py) on the first batch.  Device-event medians
and host wall clock between synchronisations (the composition is host-bound) are reported per sweep.

    python tools/bench_salsanext_eval.py [--knn] [--batch 4] [--sweeps 8] [--steps 10]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

C, P_SWEEP, H, W = 17, 34720, 32, 2048
KNN_PARAMS = {"knn": 5, "search": 5, "sigma": 1.0, "cutoff": 1.0}
CONFIG = {"sensor": dict(name="HDL32", type="spherical", proj_h=H, proj_w=W, fov_up=10., fov_down=-30., fov_left=-180,
                         fov_right=180, img_mean=[12.12, 10.88, 0.23, -1.04, 0.21], img_stds=[12.32, 11.47, 6.91, 0.86, 0.16])}


class Sweeps(object):
    """the LiDAR-only nuScenes duck type over in-memory sweeps"""

    def __init__(self, seed, sweeps):
        g = np.random.Generator(np.random.PCG64(seed))
        self.sweeps = []
        for _ in range(sweeps):
            az = g.uniform(-np.pi, np.pi, P_SWEEP)
            el = np.deg2rad(g.choice(np.linspace(-30.0, 10.0, 32), P_SWEEP))
            r = g.uniform(2.0, 70.0, P_SWEEP)
            r = np.where(el < 0, np.minimum(r, 1.84 / np.maximum(np.sin(-el), 1e-3)), r)
            pts = np.stack([r * np.cos(el) * np.cos(az), r * np.cos(el) * np.sin(az), r * np.sin(el), g.random(P_SWEEP)], 1)
            self.sweeps.append((pts.astype(np.float32), g.integers(0, 32, (P_SWEEP, 1)).astype(np.uint8)))
        self.map_name_from_general_index_to_segmentation_index = {i: int(g.integers(0, C)) for i in range(32)}
        self.mapped_cls_name = {i: "class_%d" % i for i in range(C)}
        self.token_list = ["sweep%03d" % i for i in range(sweeps)]

    def __len__(self):
        return len(self.token_list)

    def loadDataByIndex(self, i):
        pts, raw = self.sweeps[i]
        return pts, raw, None

    def labelMapping(self, sem):
        return np.vectorize(self.map_name_from_general_index_to_segmentation_index.__getitem__)(sem)[:, 0]


def median(v):
    return float(np.median(np.asarray(v, np.float64)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--knn", action="store_true")
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--sweeps", type=int, default=8)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    import torch
    import pc_processor
    from pmf_amd.utils.detinit import deterministic_init
    dev = torch.device("cuda")
    ds = Sweeps(a.seed, a.sweeps)
    loader = pc_processor.dataset.SalsaNextLoader(ds, CONFIG, is_train=False, return_uproj=True)
    model = deterministic_init(pc_processor.models.SalsaNext(in_channels=5, nclasses=C)).cuda().eval()
    knn_params = KNN_PARAMS if a.knn else None
    knn_mod = pc_processor.postproc.KNN(KNN_PARAMS, C)
    mapped = [ds.labelMapping(ds.loadDataByIndex(i)[1]) for i in range(a.sweeps)]

    def timed(fn):
        """(device ms, host wall ms) of fn() between synchronisations"""
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        return out, e0.elapsed_time(e1), (time.perf_counter() - t0) * 1e3

    def reference_post(pred, items, pixel_eval, evaluator, idx):
        """the reference's loop body (infer.py:91-119), one sweep at a time, on the maps of this batch"""
        out = []
        for j, it in enumerate(items):
            pred_output = pred[j:j + 1]
            pred_argmax = pred_output[0].argmax(dim=0)
            argmax = pred_output.argmax(dim=1)
            torch.cuda.synchronize()
            pixel_eval.addBatch(argmax.cpu(), it["label"][None].long().cpu())
            ux, uy = it["px"].long(), it["py"].long()
            if a.knn:
                unproj = knn_mod(it["proj_range"], it["depth"], pred_argmax, ux, uy)
            else:
                unproj = pred_argmax[uy, ux]
            torch.cuda.synchronize()
            pred_np = unproj.cpu().numpy().reshape(-1).astype(np.int32)
            evaluator.addBatch(pred_np, mapped[idx[j]])
            out.append(pred_np)
        return out

    result = {"what": "salsanext_eval", "knn": bool(a.knn), "points": P_SWEEP, "map": [H, W], "classes": C}
    with torch.no_grad():
        for B in sorted({1, a.batch}):
            ev = pc_processor.postproc.RangeSweepEvaluator(C, knn_params)
            pix = torch.zeros(C, C, dtype=torch.int64, device=dev)
            pts = torch.zeros(C, C, dtype=torch.int64, device=dev)
            ref_pix = pc_processor.metrics.IOUEval(C, torch.device("cpu"), ignore=[0])
            ref_pts = pc_processor.metrics.IOUEval(C, torch.device("cpu"), ignore=[0])
            t = {k: [] for k in ("loader", "forward", "post", "post_wall", "ref", "ref_wall", "fwd_post_wall")}
            same = oracle_same = True
            batches = [list(range(i, i + B)) for i in range(0, a.sweeps - B + 1, B)]
            for step in range(a.steps + 2):
                idx = batches[step % len(batches)]
                items, d, _ = timed(lambda: [loader._eval_item(i) for i in idx])
                pred, f, fw = timed(lambda: model(torch.stack([x["feature"] for x in items])))
                pix0, pts0 = pix.clone(), pts.clone()

                def post():
                    ev.post(pred, items, pixel_conf=pix, point_conf=pts)
                    return ev.labels.cpu().numpy()
                got, p, pw = timed(post)
                r0 = (ref_pix.conf_matrix.clone(), ref_pts.conf_matrix.clone())
                want, r, rw = timed(lambda: reference_post(pred, items, ref_pix, ref_pts, idx))
                same = same and np.array_equal(got, np.concatenate(want))
                if a.knn and step == 0:               # independent of the HIP vote: the numpy oracle on the same argmax maps
                    from oracle import knn_ref
                    am = pred.argmax(dim=1).cpu().numpy()
                    orc = [knn_ref.knn_vote(x["proj_range"].cpu().numpy(), x["depth"].cpu().numpy(), am[j],
                                            x["px"].cpu().numpy(), x["py"].cpu().numpy(), nclasses=C, **KNN_PARAMS)
                           for j, x in enumerate(items)]
                    oracle_same = oracle_same and np.array_equal(got, np.concatenate(orc).astype(np.int32))
                same = same and torch.equal((pix - pix0).cpu(), ref_pix.conf_matrix - r0[0])
                same = same and torch.equal((pts - pts0).cpu(), ref_pts.conf_matrix - r0[1])
                if step >= 2:                     # two warm-up batches (plans, workspaces)
                    for k, v in (("loader", d), ("forward", f), ("post", p), ("post_wall", pw), ("ref", r), ("ref_wall", rw),
                                 ("fwd_post_wall", fw + pw)):
                        t[k].append(v / B)
            assert same, "labels or confusion matrices differ from the torch composition"
            assert oracle_same, "KNN labels differ from the numpy oracle"
            result["B%d" % B] = dict({k + "_ms_per_sweep": round(median(v), 4) for k, v in t.items()},
                                     identical=bool(same), knn_oracle_identical=bool(oracle_same) if a.knn else None,
                                     steps=a.steps)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
