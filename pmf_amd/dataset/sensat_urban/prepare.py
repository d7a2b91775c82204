"""Dataset preparation of SensatUrban on the device: the points of one block -> the bird's-eye-view frame that SensatUrban
loads (tasks/sensat_urban/dataset_prepare/compute_bev_feature.py of the reference, its _compute_feature).

The reference walks the points in a Python loop over a float64 map.  Here the points are scattered into their cells by an
inverted index and every cell replays the reference's update rule over its points in ascending point index
(csrc/bev_prepare.hip), so every value equals the loop bit for bit: no floating-point atomics, the pixel arithmetic in the
type numpy's promotion picks in the reference (arith), log10 from a table filled by numpy on the host.  No GPU work falls
back to torch or numpy: a missing kernel is an error.
"""
import ctypes as C

import numpy as np
import torch

from ... import _lib as L

ARITH = ("float32", "float64")
# what the reference's promotion picks: the labelled splits stack float32 columns, the test split adds a float64 zero column
SPLIT_ARITH = {"train": "float32", "val": "float32", "test": "float64"}


def _column(a, dtype, name, P=None):
    """numpy array or tensor [P] of exactly this dtype (nothing is converted silently: a float64 x is not the file's x)"""
    t = a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))
    if t.dim() != 1 or t.dtype != dtype:
        raise ValueError("%s must be a one-dimensional %s array, got %s %s" % (name, dtype, t.dtype, tuple(t.shape)))
    if P is not None and t.shape[0] != P:
        raise ValueError("%s has %d entries, x has %d" % (name, t.shape[0], P))
    return t


def log10_table(max_count):
    """float64[max_count + 2]: entry k = numpy's log10(k); the kernel reads entry count + 1"""
    with np.errstate(divide="ignore"):
        return np.log10(np.arange(int(max_count) + 2))


class BevPrepare(object):
    """The stages of compute_bev_feature on tensors that are already on the device (the benchmark times them one by one).
    x y z float32[P], red green blue uint8[P], label uint8[P] or None."""

    def __init__(self, x, y, z, red, green, blue, label=None, grid_size=0.1, arith="float32"):
        if arith not in ARITH:
            raise ValueError("arith must be one of %r, got %r" % (ARITH, arith))
        grid_size = float(grid_size)
        if not (grid_size > 0.0 and np.isfinite(grid_size) and np.float32(grid_size) > 0):
            raise ValueError("grid_size must be positive and finite, got %r" % (grid_size,))
        self.P = P = int(x.shape[0])
        if P == 0:
            raise ValueError("an empty point cloud has no extent")
        if P >= 2 ** 31 - 1:
            raise ValueError("at most 2^31 - 2 points per block, got %d" % P)
        cols = [("x", x, torch.float32), ("y", y, torch.float32), ("z", z, torch.float32), ("red", red, torch.uint8),
                ("green", green, torch.uint8), ("blue", blue, torch.uint8)]
        if label is not None:
            cols.append(("label", label, torch.uint8))
        for name, t, dt in cols:
            if not (torch.is_tensor(t) and t.is_cuda and t.dtype == dt and t.dim() == 1 and t.shape[0] == P
                    and t.is_contiguous()):
                raise ValueError("%s must be a contiguous %s CUDA tensor [%d]" % (name, dt, P))
        self.x, self.y, self.z, self.red, self.green, self.blue, self.label = x, y, z, red, green, blue, label
        self.grid, self.f64, self.dev = grid_size, int(arith == "float64"), x.device
        self.lib = L.lib()
        self.ext = torch.zeros(8, dtype=torch.int32, device=self.dev)
        self.h = self.w = self.max_count = None

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.dev).cuda_stream)

    def _flags(self, flags):
        if flags & L.BEV_NONFINITE:
            raise ValueError("the point cloud holds a non-finite x, y or z")
        if flags & L.BEV_RANGE:
            raise ValueError("the extent of the points spans 2^31 cells or more along one axis at this grid size")
        if flags:
            raise RuntimeError("pmf_bev_prepare: a point fell outside the extent of its own cloud (flags %d)" % flags)

    def extent(self):
        """-> (h, w); raises ValueError for non-finite points or an extent the int32 cell index cannot hold"""
        n = self.lib.pmf_bev_prepare_workspace(self.P, 0, 0)
        if n < 0:
            raise ValueError("pmf_bev_prepare_workspace refused P = %d" % self.P)
        ws = torch.empty(n, dtype=torch.uint8, device=self.dev)
        L.check(self.lib.pmf_bev_prepare_extent(self.x.data_ptr(), self.y.data_ptr(), self.z.data_ptr(), self.P, self.grid,
                                                self.f64, ws.data_ptr(), self.ext.data_ptr(), self._stream()),
                "pmf_bev_prepare_extent")
        e = self.ext.cpu()
        self._flags(int(e[6]))
        self.h, self.w = int(e[4]), int(e[5])
        if self.h * self.w > 2 ** 31 - 2:
            raise ValueError("%d x %d cells are more than the int32 cell index holds" % (self.h, self.w))
        n = self.lib.pmf_bev_prepare_workspace(self.P, self.h, self.w)
        if n < 0:
            raise ValueError("pmf_bev_prepare_workspace refused P = %d, %d x %d" % (self.P, self.h, self.w))
        self.ws = torch.empty(n, dtype=torch.uint8, device=self.dev)
        self.h_idx = torch.empty(self.P, dtype=torch.int32, device=self.dev)
        self.w_idx = torch.empty(self.P, dtype=torch.int32, device=self.dev)
        return self.h, self.w

    def bin(self):
        L.check(self.lib.pmf_bev_prepare_bin(self.x.data_ptr(), self.y.data_ptr(), self.P, self.grid, self.f64,
                                             self.ext.data_ptr(), self.h, self.w, self.ws.data_ptr(), self.h_idx.data_ptr(),
                                             self.w_idx.data_ptr(), self._stream()), "pmf_bev_prepare_bin")

    def scan(self):
        L.check(self.lib.pmf_bev_prepare_scan(self.P, self.h, self.w, self.ws.data_ptr(), self.ext.data_ptr(), self._stream()),
                "pmf_bev_prepare_scan")

    def place(self):
        L.check(self.lib.pmf_bev_prepare_place(self.h_idx.data_ptr(), self.w_idx.data_ptr(), self.P, self.h, self.w,
                                               self.ws.data_ptr(), self.ext.data_ptr(), self._stream()),
                "pmf_bev_prepare_place")

    def table(self):
        """reads the maximum count back and uploads numpy's log10 of 0 .. max_count + 1"""
        e = self.ext.cpu()
        self._flags(int(e[6]))
        self.max_count = int(e[7])
        self.tab = torch.from_numpy(log10_table(self.max_count)).to(self.dev)

    def cells(self):
        self.feature_map = torch.empty((8, self.h, self.w), dtype=torch.float64, device=self.dev)
        self.label_map = torch.empty((self.h, self.w), dtype=torch.float64, device=self.dev)
        lab = None if self.label is None else self.label.data_ptr()
        L.check(self.lib.pmf_bev_prepare_cells(self.z.data_ptr(), self.red.data_ptr(), self.green.data_ptr(),
                                               self.blue.data_ptr(), lab, self.P, self.h, self.w, self.ws.data_ptr(),
                                               self.tab.data_ptr(), self.tab.numel(), self.max_count,
                                               self.feature_map.data_ptr(), self.label_map.data_ptr(), self._stream()),
                "pmf_bev_prepare_cells")

    def run(self):
        self.extent()
        self.bin()
        self.scan()
        self.place()
        self.table()
        self.cells()
        self.ws = None
        return {"feature_map": self.feature_map, "label_map": self.label_map, "h_idx": self.h_idx, "w_idx": self.w_idx}


def compute_bev_feature(x, y, z, red, green, blue, label=None, grid_size=0.1, arith="float32", device="cuda", to_host=True):
    """x y z float32[P], red green blue uint8[P], label uint8[P] or None (the test split: class 0 where a cell is occupied);
    numpy arrays or tensors.  arith: the type of the pixel arithmetic, "float32" where the reference stacks the file's
    columns with a uint8 class (train / val) and "float64" where it stacks them with a float64 zero column (test); see
    SPLIT_ARITH.  -> the reference's dict: feature_map f64[8,h,w], label_map f64[h,w], h_idx / w_idx int32[P], as numpy
    arrays (to_host) or as tensors on the device."""
    if arith not in ARITH:
        raise ValueError("arith must be one of %r, got %r" % (ARITH, arith))
    if not (float(grid_size) > 0.0 and np.isfinite(float(grid_size)) and np.float32(grid_size) > 0):
        raise ValueError("grid_size must be positive and finite, got %r" % (grid_size,))
    cols = [_column(x, torch.float32, "x")]
    P = int(cols[0].shape[0])
    if P == 0:
        raise ValueError("an empty point cloud has no extent")
    for name, a, dt in (("y", y, torch.float32), ("z", z, torch.float32), ("red", red, torch.uint8),
                        ("green", green, torch.uint8), ("blue", blue, torch.uint8)):
        cols.append(_column(a, dt, name, P))
    lab = None if label is None else _column(label, torch.uint8, "label", P)
    dev = torch.device(device)
    if dev.type != "cuda":
        raise ValueError("compute_bev_feature runs on the GPU only (there is no host path), got device %r" % (device,))
    up = [c.contiguous().to(dev) for c in cols]
    out = BevPrepare(*up, label=None if lab is None else lab.contiguous().to(dev), grid_size=grid_size, arith=arith).run()
    if to_host:
        out = {k: v.cpu().numpy() for k, v in out.items()}
    return out
