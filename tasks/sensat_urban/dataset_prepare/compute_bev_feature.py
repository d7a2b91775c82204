"""Dataset preparation of SensatUrban, step 1: NAME.ply -> NAME.pth (the bird's-eye-view frame the SensatUrban dataset loads).

    python compute_bev_feature.py ROOT [--split train val test] [--grid_size 0.1] [--skip_existing]

ROOT/<split>/ holds the blocks' .ply files; every frame is computed on the GPU (pmf_amd.dataset.compute_bev_feature) and
saved next to its .ply as a dict of numpy arrays: feature_map f64[8,h,w], label_map f64[h,w], h_idx / w_idx int32[P].
The pixel arithmetic is the one numpy's promotion picks in the reference: float32 on the labelled splits, float64 on the
test split, whose points have no class (label 0 where a cell is occupied).  Files are taken in sorted order."""
import argparse
import os
import sys
import time

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.abspath(os.path.join(HERE, "..", "..", "..")))
sys.path.insert(0, os.path.join(HERE, "..", "pmf_eval"))

import sensat_tools  # noqa: E402  (the one read_ply of the SensatUrban tasks)
from pmf_amd.dataset.sensat_urban.prepare import SPLIT_ARITH, compute_bev_feature  # noqa: E402

SPLITS = ("train", "val", "test")


def ply_files(root, split, valid=SPLITS):
    if split not in valid:
        raise ValueError("invalid split: {}".format(split))
    folder = os.path.join(root, split)
    return folder, [f for f in sorted(os.listdir(folder)) if f.endswith(".ply")]


def run(root, splits=("train",), grid_size=0.1, skip_existing=False, compute=compute_bev_feature, log=print):
    """-> [(path of the .pth written, arith)] in the order written"""
    written = []
    for split in splits:
        folder, names = ply_files(root, split)
        arith = SPLIT_ARITH[split]
        for i, name in enumerate(names):
            out = os.path.join(folder, name[:-len(".ply")] + ".pth")
            if skip_existing and os.path.exists(out):
                log("[{}] {} exists, skipped".format(i, out))
                continue
            t_start = time.time()
            data = sensat_tools.read_ply(os.path.join(folder, name))
            has_label = split != "test"
            if has_label and "class" not in data.dtype.names:
                raise ValueError("%s: no class property on a %s block" % (name, split))
            frame = compute(data["x"], data["y"], data["z"], data["red"], data["green"], data["blue"],
                            label=data["class"] if has_label else None, grid_size=grid_size, arith=arith)
            torch.save(frame, out)
            written.append((out, arith))
            log("[{}] {} {} x {}, cost time: {}".format(i, name, frame["feature_map"].shape[1],
                                                        frame["feature_map"].shape[2], time.time() - t_start))
    return written


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("root")
    ap.add_argument("--split", nargs="+", default=["train"], choices=SPLITS)
    ap.add_argument("--grid_size", type=float, default=0.1)
    ap.add_argument("--skip_existing", action="store_true")
    a = ap.parse_args(argv)
    run(a.root, a.split, a.grid_size, a.skip_existing)


if __name__ == "__main__":
    main()
