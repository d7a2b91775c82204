"""Dataset preparation of SensatUrban, step 2: NAME.ply -> NAME.bin, the uint8 class of every point in file order (what
SensatUrban.readLabelByIndex reads).  Only the labelled splits have classes.

    python extract_label.py ROOT [--split train val] [--skip_existing]"""
import argparse
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "pmf_eval"))

import sensat_tools  # noqa: E402  (the one read_ply of the SensatUrban tasks)

SPLITS = ("train", "val")


def run(root, splits=("val",), skip_existing=False, log=print):
    """-> [path of every .bin written] in the order written (sorted file names per split)"""
    written = []
    for split in splits:
        if split not in SPLITS:
            raise ValueError("invalid split: {}".format(split))
        folder = os.path.join(root, split)
        for i, name in enumerate(f for f in sorted(os.listdir(folder)) if f.endswith(".ply")):
            out = os.path.join(folder, name[:-len(".ply")] + ".bin")
            if skip_existing and os.path.exists(out):
                log("[{}] {} exists, skipped".format(i, out))
                continue
            t_start = time.time()
            data = sensat_tools.read_ply(os.path.join(folder, name))
            data["class"].astype(np.uint8).tofile(out)
            written.append(out)
            log("[{}] cost time: {}".format(i, time.time() - t_start))
    return written


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("root")
    ap.add_argument("--split", nargs="+", default=["val"], choices=SPLITS)
    ap.add_argument("--skip_existing", action="store_true")
    a = ap.parse_args(argv)
    run(a.root, a.split, a.skip_existing)


if __name__ == "__main__":
    main()
