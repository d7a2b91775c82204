"""Validate the folder main.py wrote (the counterpart of tasks/pmf_eval_nuscenes/testset_eval/check_valid.py), on the host
alone: under <save_path>/sequences/<seq>/predictions one .label file per sweep of the raw sequence, one 32-bit word per point
of the sweep, and every word an annotation id the label file's learning_map_inv can produce (high half zero).

    python check_valid.py config_server.yaml
"""
import argparse
import os
import sys

import numpy as np
import yaml

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", ".."))
from option import Option  # noqa: E402


def allowed_ids(config_path):
    """the annotation ids a prediction may hold: the values of learning_map_inv"""
    from pmf_amd.dataset.semantic_kitti.parser import label_tables
    with open(config_path, "r") as f:
        cfg = label_tables(yaml.safe_load(f))
    return sorted({int(v) for v in cfg["learning_map_inv"].values()})


def check_submission(pred_root, data_root, sequences, ids):
    """pred_root: the folder that holds sequences/; -> list of faults, one sentence each, naming the sequence and the frame;
    empty = valid."""
    faults = []
    ids = np.asarray(sorted(ids), np.int64)
    for seq in sorted("{0:02d}".format(int(s)) for s in sequences):
        velo = os.path.join(data_root, seq, "velodyne")
        if not os.path.isdir(velo):
            faults.append("sequence {}: no velodyne folder {}".format(seq, velo))
            continue
        pred_dir = os.path.join(pred_root, "sequences", seq, "predictions")
        present = set(os.listdir(pred_dir)) if os.path.isdir(pred_dir) else set()
        for f in sorted(x for x in os.listdir(velo) if x.endswith(".bin")):
            frame = f[:-4]
            name = frame + ".label"
            if name not in present:
                faults.append("sequence {} frame {}: no file {}".format(seq, frame, name))
                continue
            present.discard(name)
            npts = os.path.getsize(os.path.join(velo, f)) // 16
            nbytes = os.path.getsize(os.path.join(pred_dir, name))
            if nbytes != 4 * npts:
                faults.append("sequence {} frame {}: {} bytes for a sweep of {} points (4 bytes per point)".format(
                    seq, frame, nbytes, npts))
                continue
            lab = np.fromfile(os.path.join(pred_dir, name), dtype=np.uint32).astype(np.int64)
            bad = lab[~np.isin(lab, ids)]
            if bad.size:
                faults.append("sequence {} frame {}: {} points carry an id outside learning_map_inv, the first: {}".format(
                    seq, frame, bad.size, int(bad[0])))
        for name in sorted(present):
            faults.append("sequence {}: file {} belongs to no sweep".format(seq, name))
    return faults


class Experiment(object):
    def __init__(self, settings):
        self.settings = settings

    def run(self):
        from pmf_amd.dataset.semantic_kitti.parser import DEFAULT_CONFIG
        s = self.settings
        faults = check_submission(s.save_path, s.data_root, s.sequences, allowed_ids(s.data_config_path or DEFAULT_CONFIG))
        for f in faults:
            print(f)
        if faults:
            raise ValueError("{} is not a valid submission: {} faults, the first: {}".format(
                s.save_path, len(faults), faults[0]))
        print("valid submission: sequences {} in {}".format(s.sequences, s.save_path))


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description="validate a SemanticKITTI prediction folder")
    ap.add_argument("config_path", type=str, metavar="config_path")
    ap.add_argument("--id", type=int, default=0)
    args = ap.parse_args()
    exp = Experiment(Option(args.config_path))
    print("===init env success===")
    exp.run()
