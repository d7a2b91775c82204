"""Options of the SemanticKITTI full-sweep merge (the counterpart of tasks/pmf_eval_nuscenes/testset_eval/option.py): yaml
keys -> attributes.  data_root, main_pred_folder, sub_pred_folder, sequences, has_label and save_path are required;
merge_batch_size (16, at most PMF_FOV_MAX_FRAMES = 64), fill_class (a LEARNING class, 9 = road), n_classes (20), gpu and
data_config_path (the package's semantic-kitti.yaml) are optional.  An existing save_path is reused."""
import os

import yaml

MAX_BATCH = 64          # PMF_FOV_MAX_FRAMES of include/pmf_amd_fov.h


class Option(object):
    def __init__(self, config_path):
        self.config_path = config_path
        with open(config_path, "r") as f:
            self.config = yaml.safe_load(f)
        c = self.config
        self.save_path = c["save_path"]
        self.data_root = c["data_root"]
        self.main_pred_folder = c["main_pred_folder"]
        self.sub_pred_folder = c["sub_pred_folder"]
        self.sequences = [int(s) for s in c["sequences"]]
        self.has_label = c["has_label"]
        # ---------------------------- optional ------------------------
        self.gpu = str(c.get("gpu", "0"))
        self.n_classes = int(c.get("n_classes", 20))
        self.fill_class = int(c.get("fill_class", 9))
        self.merge_batch_size = int(c.get("merge_batch_size", 16))
        self.data_config_path = c.get("data_config_path")
        self._prepare()

    def _prepare(self):
        if not self.sequences:
            raise ValueError("sequences is empty")
        for key in ("main_pred_folder", "sub_pred_folder"):
            if not os.path.isdir(getattr(self, key)):
                raise FileNotFoundError("{} not found: {}".format(key, getattr(self, key)))
        if not 1 <= self.merge_batch_size <= MAX_BATCH:
            raise ValueError("merge_batch_size must be in 1..{}, got {}".format(MAX_BATCH, self.merge_batch_size))
        if not 1 <= self.n_classes <= 64:
            raise ValueError("n_classes must be in 1..64, got {}".format(self.n_classes))
        if not 1 <= self.fill_class < self.n_classes:
            raise ValueError("fill_class must be a learning class in 1..{}, got {}".format(self.n_classes - 1, self.fill_class))

    def check_path(self):
        os.makedirs(self.save_path, exist_ok=True)
