"""Options of the SalsaNext SemanticKITTI evaluation task: yaml keys -> attributes, the keys of tasks/salsanext_eval_nuscenes
plus ``sequences`` (the raw sequences to evaluate, default [8]) and ``data_config_path`` (the label file, default the
package's semantic-kitti.yaml).  The results go to <save_path>/Eval-SV_<dataset>_<net_type>_<KNN-search|>_<experiment_id>,
an existing directory is reused."""
import os

import yaml


class Option(object):
    def __init__(self, config_path):
        self.config_path = config_path
        with open(config_path, "r") as f:
            self.config = yaml.safe_load(f)
        c = self.config
        self.save_path, self.seed, self.gpu = c["save_path"], c.get("seed", 1), str(c.get("gpu", "0"))
        self.rank, self.world_size, self.distributed = 0, 1, False
        self.n_gpus = len(self.gpu.split(","))
        self.print_frequency, self.n_threads = int(c.get("print_frequency", 1)), c.get("n_threads", 0)
        self.experiment_id, self.is_debug = c["experiment_id"], c.get("is_debug", False)
        self.dataset, self.data_root, self.has_label = c["dataset"], c["data_root"], c["has_label"]
        self.n_classes = self.nclasses = c["n_classes"]
        self.net_type = c.get("net_type", "SalsaNext")
        self.data_len = c.get("data_len", -1)
        self.sequences = [int(s) for s in c.get("sequences", [8])]
        if not self.sequences:
            raise ValueError("sequences is empty")
        self.data_config_path = c.get("data_config_path")
        self.eval_batch_size = int(c.get("eval_batch_size", 4))
        if self.eval_batch_size < 1:
            raise ValueError("eval_batch_size must be >= 1, got {}".format(self.eval_batch_size))
        self.pretrained_model = c.get("pretrained_model")
        knn = c["post"]["KNN"]
        knn_str = "KNN-{}".format(knn["params"]["search"]) if knn["use"] else ""
        self.save_path = os.path.join(self.save_path, "Eval-SV_{}_{}_{}_{}".format(
            self.dataset, self.net_type, knn_str, self.experiment_id))

    def check_path(self):
        os.makedirs(self.save_path, exist_ok=True)
