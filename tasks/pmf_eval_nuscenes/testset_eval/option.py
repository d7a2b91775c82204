"""Options of the nuScenes full-sweep merge (tasks/pmf_eval_nuscenes/testset_eval/option.py of the reference): yaml keys ->
attributes.  The reference's ten keys are required; main_pred_dtype / sub_pred_dtype ("int32" or "uint8"), fill_class and
merge_batch_size are optional and default to the reference's behaviour.  The results go to <save_path>/<experiment_id>,
created without the reference's interactive delete / quit prompt (an existing directory is reused)."""
import os

import yaml

PRED_DTYPES = ("int32", "uint8")


class Option(object):
    def __init__(self, config_path):
        self.config_path = config_path
        with open(config_path, "r") as f:
            self.config = yaml.safe_load(f)
        c = self.config
        # ---------------------------- general options -----------------
        self.save_path = c["save_path"]
        self.gpu = str(c["gpu"])
        self.experiment_id = c["experiment_id"]
        self.is_debug = c["is_debug"]
        self.dataset = c["dataset"]
        self.data_root = c["data_root"]
        self.n_classes = c["n_classes"]
        self.has_label = c["has_label"]
        self.main_pred_folder = c["main_pred_folder"]
        self.sub_pred_folder = c["sub_pred_folder"]
        # ---------------------------- optional ------------------------
        self.main_pred_dtype = c.get("main_pred_dtype", "int32")
        self.sub_pred_dtype = c.get("sub_pred_dtype", "int32")
        self.fill_class = int(c.get("fill_class", 11))
        self.merge_batch_size = int(c.get("merge_batch_size", 8))
        self._prepare()

    def _prepare(self):
        self.save_path = os.path.join(self.config["save_path"], self.experiment_id)
        if not os.path.isdir(self.main_pred_folder):
            raise FileNotFoundError("main prediction folder not found: {}".format(self.main_pred_folder))
        if not os.path.isdir(self.sub_pred_folder):
            raise FileNotFoundError("sub prediction folder not found: {}".format(self.sub_pred_folder))
        for key in ("main_pred_dtype", "sub_pred_dtype"):
            if getattr(self, key) not in PRED_DTYPES:
                raise ValueError("{} must be one of {}, got {!r}".format(key, PRED_DTYPES, getattr(self, key)))
        if self.merge_batch_size < 1:
            raise ValueError("merge_batch_size must be >= 1, got {}".format(self.merge_batch_size))
        if not 1 <= self.n_classes <= 64:
            raise ValueError("n_classes must be in 1..64, got {}".format(self.n_classes))

    def check_path(self):
        os.makedirs(self.save_path, exist_ok=True)
