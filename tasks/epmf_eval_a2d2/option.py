"""Options of the A2D2 evaluation task (tasks/epmf_eval_a2d2/option.py of the reference): yaml keys -> attributes.  The
results go to <pretrained_path>/Eval-<dataset>-PMFNet-<best_model.strip(".pth")>-<KNN-search><TTA-num>-<experiment_id>,
created without the reference's interactive delete / quit prompt (an existing directory is reused)."""
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
        # data
        self.dataset = c["dataset"]
        self.n_classes = self.nclasses = c["nclasses"]
        self.data_root = c["data_root"]
        self.has_label = c["has_label"]
        here = os.path.dirname(os.path.abspath(__file__))
        self.cams_lidars_path = os.path.join(here, c["cams_lidars_path"])
        self.class_index_path = os.path.join(here, c["class_index_path"])
        # model
        self.net_type = c["net_type"]
        self.base_channels = c["base_channels"]
        self.img_backbone = c["img_backbone"]
        self.imagenet_pretrained = c.get("imagenet_pretrained", False)
        # checkpoint
        self.pretrained_model = os.path.join(c["pretrained_path"], "checkpoint", c["best_model"])
        self._prepare()

    def _prepare(self):
        if not os.path.isdir(self.save_path):
            raise ValueError("pretrained model is required, please train your model first. Path not exist: {}".format(
                self.save_path))
        post = self.config.get("post", {})
        knn, tta = post.get("KNN", {"use": False}), post.get("tta", {"use": False})
        tag = "KNN-{}".format(knn["params"]["search"]) if knn["use"] else ""
        if tta["use"]:
            tag += "TTA-{}".format(tta["num"])
        # (str.strip removes a character SET from both ends -- kept as the reference writes it)
        self.save_path = os.path.join(self.save_path, "Eval-{}-PMFNet-{}-{}-{}".format(
            self.dataset, self.config["best_model"].strip(".pth"), tag, self.experiment_id))

    def check_path(self):
        os.makedirs(self.save_path, exist_ok=True)
