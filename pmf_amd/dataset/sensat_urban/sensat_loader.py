"""SensatLoader -- call surface of pc_processor/dataset/sensat_urban/sensat_loader.py, as a device gather.

The reference builds every training item on the host: the whole float64 frame to float32, the label plane concatenated,
  RandomCrop(2H,2W) -> RandomRotation(360) -> RandomCrop(H,W) -> RandomHorizontalFlip -> RandomVerticalFlip
over nine planes, repeated until at least 10 % of the label plane is >= 0, then two scalar jitters (:57-73).  All of it is
one map from an output pixel to one frame pixel or to zero.  Here every frame of the train split is converted and uploaded
ONCE at construction (features pixel-major f32[h][w][8], labels int8[h][w]: 33 bytes per frame pixel stay resident), the
random draws are made on the host in torchvision's order, and a batch is
  * per acceptance round: one upload of the candidate structs, one pmf_bev_sample_count, one copy of int32[n] back (on a
    stream of the loader's own, so that the copy does not wait for the training step enqueued before it);
  * one upload of the accepted structs and one pmf_bev_sample_gather (csrc/bev_train.hip)
-- nothing of a frame crosses the host-device link per item.

Random streams.  ``draw`` consumes the torch global generator exactly as the torchvision chain does (first crop i, j --
no draw when the frame is exactly 2H x 2W --, angle, second crop i, j, horizontal flip, vertical flip) and ``draw_jitter``
Python's ``random`` (rgb first), once per item after acceptance.  For a batch of ONE the consumed streams equal the
reference's item for item.  For B > 1 a round draws one candidate for every sample not yet accepted, in index order, and
the jitters follow for all samples in index order: that differs from a loop over items only when a rejection happens
(the re-draw of a rejected sample then comes after the first draws of the samples behind it).

torchvision is not installed where this was written: the rotation follows the restatement of its tensor path with torch's
own grid_sample (oracle/tensor_aug_ref.py), so the torchvision parity of this loader is UNPINNED in the same sense as
FlipRotateCrop's.  There is no CPU path: ``batch`` on a CPU device raises; the draws, the index list and the validation of
frames and candidates need no GPU."""
import ctypes as C
import math
import random

import numpy as np
import torch

from ... import _lib as L


class _Batches(object):
    """what the trainer iterates in place of a torch DataLoader: index lists -> SensatLoader.batch.  Items are born on the
    device, so there is nothing for worker processes to do."""

    def __init__(self, loader, batch_size, shuffle, drop_last, sampler):
        self.loader, self.batch_size, self.shuffle, self.drop_last, self.sampler = loader, int(batch_size), shuffle, drop_last, sampler
        if self.batch_size < 1:
            raise ValueError("batch_size must be positive")

    def _n(self):
        return len(self.sampler) if self.sampler is not None else len(self.loader)

    def __len__(self):
        n = self._n()
        return n // self.batch_size if self.drop_last else -(-n // self.batch_size)

    def __iter__(self):
        if self.sampler is not None:
            order = list(self.sampler)
        elif self.shuffle:
            order = torch.randperm(len(self.loader)).tolist()          # the torch global generator
        else:
            order = list(range(len(self.loader)))
        bs = self.batch_size
        for k in range(0, len(order), bs):
            idx = order[k:k + bs]
            if len(idx) < bs and self.drop_last:
                return
            yield self.loader.batch(idx)


class SensatLoader(object):
    def __init__(self, dataset, img_h=800, img_w=800, n_samples_split=200, device=None):
        self.dataset, self.img_h, self.img_w = dataset, int(img_h), int(img_w)
        self.split = dataset.split
        if device is None:
            device = "cuda" if torch.cuda.is_available() else "cpu"
        self.device = torch.device(device)
        self.frames = []                        # train: (features f32[h,w,8], labels int8[h,w]) on self.device
        self._side = None                       # the stream of the acceptance rounds (count)
        if self.split == "train":
            self.frame_idx_list = []
            for i in range(len(dataset)):
                frame = dataset.readDataByIndex(i)
                h, w = frame["feature_map"].shape[1], frame["feature_map"].shape[2]
                self.frame_idx_list += [i] * int(n_samples_split * h / 4000 * w / 4000)
                self.frames.append(self._resident(frame, i))
            self.total_samples = len(self.frame_idx_list)
            self.is_train = True
            if self.device.type == "cuda":
                torch.cuda.synchronize(self.device)        # the frames are in place before any stream reads them
        else:
            self.total_samples = len(dataset)
            self.is_train = False
        print("Generate {} samples from {} split".format(self.total_samples, self.split))

    def _resident(self, frame, i):
        fm, lm = np.asarray(frame["feature_map"]), np.asarray(frame["label_map"])
        if fm.ndim != 3 or fm.shape[0] != 8 or lm.shape != fm.shape[1:]:
            raise ValueError("frame {}: feature_map {} / label_map {} are not [8,h,w] / [h,w]".format(i, fm.shape, lm.shape))
        if lm.size and (lm.min() < -1 or lm.max() > 127 or (lm != np.floor(lm)).any()):
            raise ValueError("frame {}: labels outside [-1, 127] (min {}, max {}): the resident label plane is int8".format(
                i, lm.min(), lm.max()))
        feat = torch.from_numpy(fm).float().permute(1, 2, 0).contiguous()        # the reference's .float(), pixel-major
        label = torch.from_numpy(lm.astype(np.int8))
        return feat.to(self.device), label.to(self.device)

    def resident_bytes(self):
        return sum(f.numel() * 4 + l.numel() for f, l in self.frames)

    def __len__(self):
        return self.total_samples

    # ---- host side: the draws -------------------------------------------------------------------------------------------
    def draw(self, h, w):
        """one candidate for an h x w frame from the torch global generator, in torchvision's order ->
        (top1, left1, angle, top2, left2, hflip, vflip)"""
        H, W = self.img_h, self.img_w

        def crop(h, w, th, tw):                 # RandomCrop.get_params
            if h < th or w < tw:
                raise ValueError("Required crop size {} is larger than input image size {}".format((th, tw), (h, w)))
            if (h, w) == (th, tw):
                return 0, 0
            return (int(torch.randint(0, h - th + 1, size=(1,)).item()), int(torch.randint(0, w - tw + 1, size=(1,)).item()))
        top1, left1 = crop(h, w, 2 * H, 2 * W)
        angle = float(torch.empty(1).uniform_(-360., 360.).item())
        top2, left2 = crop(2 * H, 2 * W, H, W)
        hflip = bool(torch.rand(1) < 0.5)
        vflip = bool(torch.rand(1) < 0.5)
        return top1, left1, angle, top2, left2, hflip, vflip

    @staticmethod
    def draw_jitter():
        """(jit_rgb, jit_h) from Python's random, in the order of sensat_loader.py:70-71"""
        jit_rgb = random.uniform(-0.2, 0.2)
        jit_h = random.uniform(-2, 2)
        return jit_rgb, jit_h

    def pack(self, frame_idx, cand, jitter=(0.0, 0.0)):
        """one candidate of frame `frame_idx` -> L.BevSample, validated against the frame and the crop sizes"""
        feat, label = self.frames[frame_idx]
        h, w = label.shape
        top1, left1, angle, top2, left2, hflip, vflip = cand
        H, W = self.img_h, self.img_w
        if not (0 <= top1 <= h - 2 * H and 0 <= left1 <= w - 2 * W and 0 <= top2 <= H and 0 <= left2 <= W):
            raise ValueError("candidate {} does not fit a {} x {} frame at crop {} x {}".format(cand, h, w, H, W))
        r = math.radians(-angle)
        return L.BevSample(feat=feat.data_ptr(), label=label.data_ptr(), h=h, w=w, top1=top1, left1=left1, m0=math.cos(r),
                           m1=math.sin(r), m3=-math.sin(r), m4=math.cos(r), top2=top2, left2=left2,
                           flags=(L.BEV_HFLIP if hflip else 0) | (L.BEV_VFLIP if vflip else 0), jit_rgb=jitter[0],
                           jit_h=jitter[1])

    # ---- device side ----------------------------------------------------------------------------------------------------
    def _need_gpu(self):
        if self.device.type != "cuda":
            raise RuntimeError("SensatLoader runs on the GPU only (no CPU fallback)")

    def _upload(self, structs):
        arr = (L.BevSample * len(structs))(*structs)
        return torch.frombuffer(bytearray(arr), dtype=torch.uint8).to(self.device)

    def _side_stream(self):
        if self._side is None:
            self._side = torch.cuda.Stream(device=self.device)
        return self._side

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def count(self, structs):
        """int32[n] on the host: output pixels with label >= 0 (zero fill included) of every candidate.  Runs on a stream of
        the loader's own: it reads only the label planes, which never change, and the copy back then waits for the count
        alone -- on the caller's stream it would wait for everything enqueued there (a whole training step), and the host
        could no longer run ahead of the device."""
        self._need_gpu()
        with torch.cuda.stream(self._side_stream()):
            dev = self._upload(structs)
            counts = torch.empty(len(structs), dtype=torch.int32, device=self.device)
            L.check(L.lib().pmf_bev_sample_count(dev.data_ptr(), len(structs), self.img_h, self.img_w, counts.data_ptr(),
                                                 self._stream()), "pmf_bev_sample_count")
            return counts.cpu()

    def gather(self, structs):
        """-> (f32[B,8,H,W], f32[B,H,W]) on the device"""
        self._need_gpu()
        # the structs come from pageable host memory: such a copy returns when it is done, and on the caller's stream it
        # would be done only after everything enqueued there -- so they travel on the loader's stream and the gather waits
        cur = torch.cuda.current_stream(self.device)
        with torch.cuda.stream(self._side_stream()):
            dev = self._upload(structs)
        cur.wait_stream(self._side)
        dev.record_stream(cur)
        B, H, W = len(structs), self.img_h, self.img_w
        feature = torch.empty((B, 8, H, W), dtype=torch.float32, device=self.device)
        label = torch.empty((B, H, W), dtype=torch.float32, device=self.device)
        L.check(L.lib().pmf_bev_sample_gather(dev.data_ptr(), B, H, W, feature.data_ptr(), label.data_ptr(), self._stream()),
                "pmf_bev_sample_gather")
        return feature, label

    def batch(self, indices):
        """(f32[B,8,H,W], f32[B,H,W]) on the device for the given sample indices (see the module docstring for the order
        of the draws)"""
        indices = [int(i) for i in indices]
        if not self.is_train:
            items = [self._frame(i) for i in indices]
            return torch.stack([f for f, _ in items]), torch.stack([l for _, l in items])
        self._need_gpu()
        frame_of = [self.frame_idx_list[i] for i in indices]
        accepted = [None] * len(indices)
        pending = list(range(len(indices)))
        numel = self.img_h * self.img_w
        while pending:
            cands = [self.draw(*self.frames[frame_of[k]][1].shape) for k in pending]
            counts = self.count([self.pack(frame_of[k], c) for k, c in zip(pending, cands)])
            still = []
            for k, c, n in zip(pending, cands, counts):
                if bool(n.float() / numel < 0.1):        # float32, as `valid_percent < 0.1` (sensat_loader.py:66-68)
                    still.append(k)
                else:
                    accepted[k] = c
            pending = still
        return self.gather([self.pack(f, c, self.draw_jitter()) for f, c in zip(frame_of, accepted)])

    def _frame(self, index):
        frame = self.dataset.readDataByIndex(index)
        return (torch.from_numpy(np.asarray(frame["feature_map"])).float().to(self.device),
                torch.from_numpy(np.asarray(frame["label_map"])).float().to(self.device))

    def __getitem__(self, index):
        if not self.is_train:
            return self._frame(index)
        feature, label = self.batch([index])
        return feature[0], label[0]

    def batches(self, batch_size, shuffle=True, drop_last=True, sampler=None):
        """the iterator the trainer uses in place of torch.utils.data.DataLoader (``len()`` = batches per epoch); other
        splits stack equal-size frames (the use_crop=True validation set)"""
        return _Batches(self, batch_size, shuffle, drop_last, sampler)
