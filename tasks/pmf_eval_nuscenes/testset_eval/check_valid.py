"""Validate the folder main.py wrote (counterpart of the reference's tasks/pmf_eval_nuscenes/testset_eval/check_valid.py).

With the nuscenes-devkit installed: its validate_submission (and, with labels, LidarSegEval) on <save_path>/preds, as the
reference runs them.  Without it, or with a dataset object passed in (Experiment(settings, dataset=...): any object with
token_list and loadLabelByIndex or loadDataByIndex, which give the sweeps' point counts): check_submission(), the same
conditions stated without the devkit -- one uint8 file per sweep token and none besides, as many bytes as the sweep has
points, every label inside 1..n_classes-1, and a submission.json whose meta block carries the five boolean flags.

    python check_valid.py config_server.yaml
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", ".."))
from option import Option  # noqa: E402

META_FLAGS = ("use_camera", "use_lidar", "use_radar", "use_map", "use_external")


def check_submission(results_folder, split, point_counts, n_classes):
    """results_folder: the ``preds`` directory; point_counts: {lidar_token: points of the sweep}.  -> list of faults, one
    sentence each, naming the token or file; empty = valid."""
    faults = []
    meta_path = os.path.join(results_folder, split, "submission.json")
    if not os.path.isfile(meta_path):
        faults.append("submission.json missing: {}".format(meta_path))
    else:
        try:
            with open(meta_path) as f:
                meta = json.load(f).get("meta")
        except (ValueError, AttributeError):
            meta = None
        if not isinstance(meta, dict):
            faults.append("submission.json has no meta block")
        else:
            for k in META_FLAGS:
                if not isinstance(meta.get(k), bool):
                    faults.append("submission.json meta flag {} missing or not a boolean".format(k))
    seg_dir = os.path.join(results_folder, "lidarseg", split)
    present = set(os.listdir(seg_dir)) if os.path.isdir(seg_dir) else set()
    for token, npts in point_counts.items():
        name = "{}_lidarseg.bin".format(token)
        if name not in present:
            faults.append("token {}: no file {}".format(token, name))
            continue
        present.discard(name)
        lab = np.fromfile(os.path.join(seg_dir, name), dtype=np.uint8)
        if lab.shape[0] != int(npts):
            faults.append("token {}: {} bytes for a sweep of {} points".format(token, lab.shape[0], int(npts)))
            continue
        if lab.shape[0] and int(lab.min()) < 1:
            faults.append("token {}: {} points labelled 0 (labels must be in 1..{})".format(
                token, int((lab == 0).sum()), n_classes - 1))
        if lab.shape[0] and int(lab.max()) >= n_classes:
            faults.append("token {}: label {} >= n_classes {} (labels must be in 1..{})".format(
                token, int(lab.max()), n_classes, n_classes - 1))
    for name in sorted(present):
        faults.append("file {} belongs to no token of the split".format(name))
    return faults


def dataset_point_counts(dataset):
    """{token: points} from the dataset's own files: the annotation where there is one, else the point cloud"""
    out = {}
    for i in range(len(dataset)):
        token = dataset.token_list[i]
        token = token["lidar_token"] if isinstance(token, dict) else token
        lab = dataset.loadLabelByIndex(i) if hasattr(dataset, "loadLabelByIndex") else None
        out[token] = int(np.asarray(lab).reshape(-1).shape[0]) if lab is not None else \
            int(dataset.loadDataByIndex(i)[0].shape[0])
    return out


class Experiment(object):
    def __init__(self, settings, dataset=None):
        self.settings, self.dataset = settings, dataset
        self.eval_set = "val" if settings.has_label else "test"
        self.results_folder = os.path.join(settings.save_path, "preds")

    def run(self):
        s = self.settings
        try:
            import nuscenes  # noqa: F401
            have_devkit = True
        except ImportError:
            have_devkit = False
        if have_devkit and self.dataset is None:
            from nuscenes.nuscenes import NuScenes
            from nuscenes.eval.lidarseg.validate_submission import validate_submission
            from nuscenes.eval.lidarseg.evaluate import LidarSegEval
            nusc = NuScenes(version="v1.0-trainval" if s.has_label else "v1.0-test", dataroot=s.data_root, verbose=False)
            validate_submission(nusc, eval_set=self.eval_set, verbose=True, results_folder=self.results_folder,
                                zip_out=s.save_path)
            if s.has_label:
                LidarSegEval(nusc, eval_set=self.eval_set, verbose=True, results_folder=self.results_folder).evaluate()
            return
        dataset = self.dataset
        if dataset is None:
            import pc_processor
            dataset = pc_processor.dataset.nuScenes.open_nuscenes(
                False, s.data_root, "v1.0-trainval" if s.has_label else "v1.0-test", self.eval_set, has_image=False,
                splits_path=s.config.get("nus_splits"))
        faults = check_submission(self.results_folder, self.eval_set, dataset_point_counts(dataset), s.n_classes)
        for f in faults:
            print(f)
        if faults:
            raise ValueError("{} is not a valid submission: {} faults, the first: {}".format(
                self.results_folder, len(faults), faults[0]))
        print("valid submission: {} sweeps in {}".format(len(dataset), self.results_folder))


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description="validate a nuScenes lidarseg submission folder")
    ap.add_argument("config_path", type=str, metavar="config_path")
    ap.add_argument("--id", type=int, default=0)
    args = ap.parse_args()
    exp = Experiment(Option(args.config_path))
    print("===init env success===")
    exp.run()
