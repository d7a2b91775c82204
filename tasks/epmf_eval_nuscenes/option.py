"""Options of the EPMF nuScenes evaluation task (tasks/epmf_eval_nuscenes/option.py of the reference): yaml keys ->
attributes.  The results go to <pretrained_path>/Eval-<dataset>-PMFNet-<best_model.strip(".pth")>-<KNN-search|noKNN>-
<experiment_id>, created without the reference's interactive delete / quit prompt (an existing directory is reused).
Optional keys beyond the reference's: sub_pred_folder (+ sub_pred_dtype "int32" / "uint8", fill_class 11) -- with it the
sweeps are completed from that LiDAR-only prediction folder as they finish (infer.py)."""
import os

import yaml


class Option(object):
    def __init__(self, config_path):
        self.config_path = config_path
        with open(config_path, "r") as f:
            self.config = yaml.safe_load(f)
        c = self.config
        self.save_path = c["pretrained_path"]
        self.seed, self.gpu = c.get("seed", 1), str(c.get("gpu", "0"))
        self.rank, self.world_size, self.distributed = 0, 1, False
        self.n_gpus = len(self.gpu.split(","))
        self.print_frequency = c.get("print_frequency", 1)
        self.n_threads = c.get("n_threads", 0)
        self.experiment_id = c["experiment_id"]
        self.is_debug = c["is_debug"]
        self.save_pred_results = c["save_pred_results"]
        # data
        self.dataset = c["dataset"]
        self.n_classes = self.nclasses = c["nclasses"]
        self.data_root = c["data_root"]
        self.has_label = c["has_label"]
        # model
        self.net_type = c["net_type"]
        self.base_channels = c["base_channels"]
        self.img_backbone = c["img_backbone"]
        self.imagenet_pretrained = c.get("imagenet_pretrained", False)
        # checkpoint
        self.pretrained_model = os.path.join(c["pretrained_path"], "checkpoint", c["best_model"])
        # optional: a LiDAR-only prediction folder (tasks/salsanext_eval_nuscenes) to fill the points no camera sees
        self.sub_pred_folder = c.get("sub_pred_folder")
        self.sub_pred_dtype = c.get("sub_pred_dtype", "int32")
        self.fill_class = int(c.get("fill_class", 11))
        self._prepare()

    def _prepare(self):
        if not os.path.isdir(self.save_path):
            raise ValueError("pretrained model is required, please train your model first. Path not exist: {}".format(
                self.save_path))
        if self.sub_pred_folder is not None and not os.path.isdir(self.sub_pred_folder):
            raise FileNotFoundError("sub prediction folder not found: {}".format(self.sub_pred_folder))
        if self.sub_pred_dtype not in ("int32", "uint8"):
            raise ValueError("sub_pred_dtype must be int32 or uint8, got {!r}".format(self.sub_pred_dtype))
        knn = self.config["post"]["KNN"]
        knn_str = "KNN-{}".format(knn["params"]["search"]) if knn["use"] else "noKNN"
        # (str.strip removes a character SET from both ends -- kept as the reference writes it)
        self.save_path = os.path.join(self.save_path, "Eval-{}-PMFNet-{}-{}-{}".format(
            self.dataset, self.config["best_model"].strip(".pth"), knn_str, self.experiment_id))

    def check_path(self):
        os.makedirs(self.save_path, exist_ok=True)
