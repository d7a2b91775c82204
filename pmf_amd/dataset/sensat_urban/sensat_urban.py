"""SensatUrban bird's-eye-view frames -- call surface of pc_processor/dataset/sensat_urban/sensat_urban.py.

<root_path>/<split>/ holds per block NAME.pth (what the dataset preparation writes: a dict of numpy arrays, feature_map
f64[8,h,w], label_map [h,w] with -1 = ignore, h_idx / w_idx int64[P] = the pixel of every point), NAME.bin (uint8 point
labels) and NAME.ply (the points).  All frames of the split are loaded at construction, as the reference does.
Differences that do not change what a frame holds: files are taken in sorted order (the reference takes os.listdir order),
and torch.load is told weights_only=False (the frames are dicts of numpy arrays, which newer torch refuses by default)."""
import math
import os

import numpy as np
import torch

CLASS_NAMES = ("Ground", "High Vegetation", "Buildings", "Walls", "Bridge", "Parking", "Rail", "traffic Roads",
               "Street Furniture", "Cars", "Footpath", "Bikes", "Water")
SKIPPED_BLOCK = "cambridge_block_1"          # a tiny block, smaller than the tiles: the reference leaves it out by name


def tile_windows(h, w, size_h, size_w=None):
    """the tile enumeration shared by the dataset's use_crop and the evaluation loop: ceil(h / size) rows by ceil(w / size)
    columns, row-major; a tile that would run past the frame is shifted back to end at its border (so it overlaps its
    neighbour), and starts at 0 when the frame is smaller than the tile.  -> [(h_start, h_end, w_start, w_end)]"""
    size_w = size_h if size_w is None else size_w

    def spans(n, size):
        out = []
        for k in range(int(math.ceil(n / size))):
            lo, hi = k * size, (k + 1) * size
            if hi > n:
                lo, hi = max(n - size, 0), n
            out.append((lo, hi))
        return out
    return [(h0, h1, w0, w1) for h0, h1 in spans(h, size_h) for w0, w1 in spans(w, size_w)]


class SensatUrban(object):
    def __init__(self, root_path, split="train", keep_idx=False, img_h=320, img_w=320, use_crop=False):
        if split not in ("train", "test", "val"):
            raise ValueError("invalid split: {}".format(split))
        self.root_path, self.split, self.keep_idx = root_path, split, keep_idx
        self.img_h, self.img_w, self.use_crop = img_h, img_w, use_crop
        self.split_folder = os.path.join(root_path, split)
        self.data_split = [f for f in sorted(os.listdir(self.split_folder)) if ".pth" in f and SKIPPED_BLOCK not in f]
        self.all_data_frame = self.loadDataCache()
        print("Using {} data frame from {} split".format(len(self.all_data_frame), split))
        self.mapped_cls_name = {-1: "ignore"}
        self.mapped_cls_name.update(enumerate(CLASS_NAMES))

    def _crops(self, frame):
        fm, lm = frame["feature_map"], frame["label_map"]
        for h0, h1, w0, w1 in tile_windows(fm.shape[1], fm.shape[2], self.img_h, self.img_w):
            feature = np.zeros((8, self.img_h, self.img_w))
            label = np.zeros((self.img_h, self.img_w))
            feature[:, :h1 - h0, :w1 - w0] = fm[:, h0:h1, w0:w1]
            label[:h1 - h0, :w1 - w0] = lm[h0:h1, w0:w1]
            yield {"feature_map": feature, "label_map": label}

    def loadDataCache(self):
        frames = []
        for name in self.data_split:
            frame = torch.load(os.path.join(self.split_folder, name), weights_only=False)
            if not self.keep_idx:
                frame["h_idx"] = frame["w_idx"] = None
            if self.use_crop:
                frames.extend(self._crops(frame))
            else:
                frames.append(frame)
        return frames

    def readFileNameByIndex(self, index):
        return self.data_split[index].replace(".pth", ".bin")

    def readLabelByIndex(self, index):
        return np.fromfile(os.path.join(self.split_folder, self.readFileNameByIndex(index)), dtype=np.uint8)

    def readDataByIndex(self, index):
        return self.all_data_frame[index]

    def __len__(self):
        return len(self.all_data_frame)
