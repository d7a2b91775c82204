"""Options of the SensatUrban PMF evaluation task (tasks/sensat_urban/pmf_eval/option.py of the reference): yaml keys ->
attributes.  The results go to <training_folder>/Eval-PMFNet_<dataset>_<experiment_id>, created without the reference's
interactive delete / quit prompt (an existing directory is reused).  save_scores (not in the reference, default true):
write every frame's confidence map f32[1,C,h,w] as .npy -- hundreds of MB per block at full size."""
import os

import yaml


class Option(object):
    def __init__(self, config_path):
        self.config_path = config_path
        with open(config_path, "r") as f:
            self.config = yaml.safe_load(f)
        c = self.config
        self.save_path = c["training_folder"]
        self.seed, self.gpu = c["seed"], str(c["gpu"])
        self.rank, self.world_size, self.distributed = 0, 1, False
        self.n_gpus = len(self.gpu.split(","))
        self.print_frequency = c["print_frequency"]
        self.n_threads = c["n_threads"]
        self.experiment_id = c["experiment_id"]
        self.is_debug = c["is_debug"]
        # data
        self.dataset = c["dataset"]
        self.nclasses = self.n_classes = c["n_classes"]
        self.data_root = c["data_root"]
        self.has_label = c["has_label"]
        # model
        self.img_backbone = c["img_backbone"]
        self.base_channels = c["base_channels"]
        self.imagenet_pretrained = c["imagenet_pretrained"]
        self.feature_mean = c["feature_mean"]
        self.feature_std = c["feature_std"]
        self.img_size = c["img_size"]
        self.save_scores = bool(c.get("save_scores", True))
        # checkpoint (null: the model keeps its initial weights -- for dry runs of the pipeline)
        self.pretrained_model = None if c["pretrained_model"] is None else os.path.join(
            c["training_folder"], "checkpoint", c["pretrained_model"])
        self._prepare()

    def _prepare(self):
        if not os.path.isdir(self.save_path):
            raise ValueError("training path not exists: {}".format(self.save_path))
        self.save_path = os.path.join(self.save_path, "Eval-PMFNet_{}_{}".format(self.dataset, self.experiment_id))

    def check_path(self):
        os.makedirs(self.save_path, exist_ok=True)
