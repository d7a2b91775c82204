"""A2D2 camera / LiDAR frames for EPMF on MI355X (pc_processor/dataset/a2d2/dataset_a2d2.py:66-306).

Same constructor and public surface as the reference's ``A2D2_PV``.  The two per-frame host steps of the reference run on the
device (include/pmf_amd_a2d2.h):

  * the undistortion of the 1208 x 1920 camera image (:158-186, cv2.undistort / cv2.fisheye.undistortImage) is one
    ``pmf_remap_u8c3`` through a per-camera map that ``pmf_undistort_map`` builds on first use -- OpenCV is not needed;
  * ``getLabel`` (:244-254, a Python loop that formats a hex string per point and looks it up in a dictionary) is a host
    gather ``sem_image[rows, cols]`` with numpy's own index semantics and a table search on the device; the label image is
    never uploaded.  A colour that is not in the table raises the ``KeyError`` the dictionary would have raised, for the
    first such point.

PNG decoding is the only per-frame host work left.  ``projectDevice`` is what PerspectiveViewLoaderV2 calls: the per-point
pass ``pmf_a2d2_index`` (float32 rows, float64 depth, scaled coordinates, bounding box, classes), one host read of its
``meta`` (the frame size is data, as in the reference) and the existing ``pmf_project_v2_scatter`` with an identity source
index and an identity label table -- A2D2 keeps every point and ``labelMapping`` is the identity.

Parity statement.  The kernels follow OpenCV's published algorithm (initUndistortRectifyMap and its fisheye counterpart in
float64, remap INTER_LINEAR / BORDER_CONSTANT 0 in its fixed-point form with 5 fractional bits); parity with OpenCV's own
output is unpinned, in the sense the README uses for torchvision: ``cv2`` is not available where this project is built, so
no fixture could be produced with it.  One known deviation: OpenCV's ``short`` map wraps beyond +-32767 px, this map
saturates at the int32 range.

The constructor's extra keyword arguments default to the reference's values and exist so that a small tree can be loaded:
the reference's ``np.delete`` with its fixed indices raises on any tree smaller than the real one."""
import ctypes as C
import glob
import json
import os

import numpy as np
import torch
from PIL import Image
from torch.utils import data

from ... import _lib as L

mapped_class_name = {
    0: 'ignore', 1: 'car', 2: 'bicycle', 3: 'pedestrian', 4: 'truck', 5: 'small_vehicles', 6: 'traffic_signal',
    7: 'traffic_sign', 8: 'utility_vehicle', 9: 'sidebars', 10: 'speed_bumper', 11: 'curbstone', 12: 'solid_line',
    13: 'irrelevant_signs', 14: 'road_blocks', 15: 'tractor', 16: 'non-drivable_street', 17: 'zebra_crossing',
    18: 'obstacles/trash', 19: 'poles', 20: 'RD_restricted_area', 21: 'animals', 22: 'grid_structure', 23: 'signal_corpus',
    24: 'drivable_cobblestone', 25: 'electronic_traffic', 26: 'slow_drive_area', 27: 'nature_object', 28: 'parking_area',
    29: 'sidewalk', 30: 'ego_car', 31: 'painted_driv._instr.', 32: 'traffic_guide_obj.', 33: 'dashed_line',
    34: 'RD_normal_street', 35: 'sky', 36: 'buildings', 37: 'blurred_area', 38: 'rain_dirt'}

cls_freq = [0, 16638586, 816746, 885671, 4205546, 166147, 209321, 1277733, 544559, 32109, 3, 5093660, 1705323, 2194196,
            1044710, 5349, 3029528, 161433, 1668462, 2647306, 956223, 4182, 4622371, 439294, 6069454, 9990, 1138946,
            78342740, 2156414, 21557480, 8634634, 660671, 1394186, 1719920, 85871754, 2745726, 63773755, 9046, 45]

# frames of the full data set that the reference leaves out (positions in the sorted list of lidar files)
unused_index = [942] + list(range(12124, 12135)) + list(range(20720, 20728)) + list(range(21299, 21303)) + [27427, 27428]
# ... and, after those, the frames without points
zero_size_index = list(range(12907, 12913)) + list(range(13649, 13653))

_CAMERAS = ('frontleft', 'frontcenter', 'frontright', 'sideleft', 'sideright', 'rearcenter')
_LENS = {'Telecam': L.LENS_TELECAM, 'Fisheye': L.LENS_FISHEYE}
MAX_COLOURS = 64        # size of the colour table pmf_a2d2_index takes


def colour_table(class_index):
    """the '#rrggbb' -> class dictionary as (keys u32[n] = r << 16 | g << 8 | b, cls i32[n]), in the dictionary's order"""
    if any(len(k) != 7 or k[0] != '#' for k in class_index) or not 1 <= len(class_index) <= MAX_COLOURS:
        raise ValueError("A2D2_PV: the class index must hold 1 to %d '#rrggbb' colours" % MAX_COLOURS)
    keys = np.array([int(k[1:], 16) for k in class_index], np.uint32)
    return keys, np.array(list(class_index.values()), np.int32)


def _stream(dev):
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def undistort_map_gpu(lens, cam_matrix, cam_matrix_original, distortion, h, w, device="cuda"):
    """-> int32[h, w, 2] device map of pmf_undistort_map; ``lens`` is 'Telecam' or 'Fisheye'"""
    dev = torch.device(device)
    ir = np.ascontiguousarray(np.linalg.inv(np.asarray(cam_matrix, np.float64)).reshape(9))
    k = np.asarray(cam_matrix_original, np.float64)
    d = np.zeros(5, np.float64)
    flat = np.asarray(distortion, np.float64).reshape(-1)[:5]
    d[:flat.shape[0]] = flat
    out = torch.empty((h, w, 2), dtype=torch.int32, device=dev)
    L.check(L.lib().pmf_undistort_map(_LENS[lens], ir.ctypes.data, k[0, 0], k[1, 1], k[0, 2], k[1, 2], d.ctypes.data, h, w,
                                      out.data_ptr(), _stream(dev)), "pmf_undistort_map")
    return out


def remap_gpu(src, map_dev):
    """uint8[sh, sw, 3] device tensor, int32[h, w, 2] map -> uint8[h, w, 3]"""
    if not (src.is_cuda and src.dtype == torch.uint8 and src.dim() == 3 and src.shape[2] == 3):
        raise RuntimeError("remap_gpu takes a uint8 [h, w, 3] GPU tensor (no CPU fallback)")
    src = src.contiguous()
    h, w = int(map_dev.shape[0]), int(map_dev.shape[1])
    dst = torch.empty((h, w, 3), dtype=torch.uint8, device=src.device)
    L.check(L.lib().pmf_remap_u8c3(src.data_ptr(), src.shape[0], src.shape[1], map_dev.data_ptr(), h, w, dst.data_ptr(),
                                   _stream(src.device)), "pmf_remap_u8c3")
    return dst


def a2d2_index_gpu(points, reflectance, rows, cols, rgb, keys, cls, img_scale=1.0, device="cuda"):
    """pmf_a2d2_index on host arrays (one packed upload) -> dict of device tensors pts, depth, xy, x_data, y_data, sem and
    the host list ``meta`` = row_min, row_max, col_min, col_max, n_unknown, first_unknown.  ``rgb`` None: no labels."""
    from ..perspective_view_loader import upload_packed
    dev = torch.device(device)
    P = int(np.asarray(points).shape[0])
    if P == 0:
        raise ValueError("A2D2_PV: the frame has no points")
    parts = [np.ascontiguousarray(points, np.float64).reshape(P, 3), np.ascontiguousarray(reflectance, np.float64).reshape(P),
             np.ascontiguousarray(rows, np.int32).reshape(P), np.ascontiguousarray(cols, np.int32).reshape(P)]
    if rgb is not None:
        # (the keys travel as their int32 bit pattern: the packed upload views each part through a torch dtype)
        parts += [np.ascontiguousarray(rgb, np.uint8).reshape(P, 3), np.ascontiguousarray(keys, np.uint32).view(np.int32),
                  np.ascontiguousarray(cls, np.int32)]
    up = upload_packed(parts, dev)
    o = dict(pts=torch.empty((P, 4), dtype=torch.float32, device=dev), depth=torch.empty(P, dtype=torch.float32, device=dev),
             xy=torch.empty((P, 2), dtype=torch.float64, device=dev), x_data=torch.empty(P, dtype=torch.int32, device=dev),
             y_data=torch.empty(P, dtype=torch.int32, device=dev), sem=torch.empty(P, dtype=torch.int32, device=dev))
    meta = torch.empty(6, dtype=torch.int32, device=dev)
    rgb_p, key_p, cls_p, n = (up[4].data_ptr(), up[5].data_ptr(), up[6].data_ptr(), int(up[5].shape[0])) \
        if rgb is not None else (None, None, None, 0)
    L.check(L.lib().pmf_a2d2_index(up[0].data_ptr(), up[1].data_ptr(), up[2].data_ptr(), up[3].data_ptr(), rgb_p, P, key_p,
                                   cls_p, n, float(img_scale), o["pts"].data_ptr(), o["depth"].data_ptr(),
                                   o["xy"].data_ptr(), o["x_data"].data_ptr(), o["y_data"].data_ptr(), o["sem"].data_ptr(),
                                   meta.data_ptr(), _stream(dev)), "pmf_a2d2_index")
    o["meta"] = [int(v) for v in meta.tolist()]       # the one host read (frame size is data)
    return o


class A2D2_PV(data.Dataset):
    def __init__(self, root, camsLidars_path, classIndex_path, split='train', has_label=True, unused_index=unused_index,
                 zero_size_index=zero_size_index, split_bounds=(22407, 25181), device="cuda"):
        self.root, self.split, self.has_label, self.device = root, split, has_label, device
        self.mapped_class_name = mapped_class_name
        self.unused_index, self.zero_size_index = unused_index, zero_size_index
        self.cls_freq = np.array(cls_freq)
        self.cls_freq = self.cls_freq / self.cls_freq.sum()
        self.cls_freq[0] = 0
        with open(camsLidars_path, 'r') as f:
            self.cams_lidars = json.load(f)
        with open(classIndex_path, 'r') as f:
            self.class_index = json.load(f)
        self._keys, self._cls = colour_table(self.class_index)
        if os.path.isdir(self.root):
            print("Dataset found: {}".format(self.root))
        else:
            raise ValueError("dataset not found: {}".format(self.root))
        files = np.array(sorted(glob.glob(os.path.join(self.root, '*/lidar/*/*.npz'))), dtype=object)
        if self.unused_index is not None:
            files = np.delete(files, self.unused_index)
        if self.zero_size_index is not None:
            files = np.delete(files, self.zero_size_index)
        lo, hi = split_bounds
        if split == 'train':
            files = files[:lo]
        elif split == 'valid':
            files = files[lo:hi]
        elif split == 'test':
            files = files[hi:]
        elif split != 'all':
            raise ValueError("invalid split: {}".format(self.split))
        self.lidar_files = [str(f) for f in files]
        self.camera_files = self.extract_file_name_from_lidar_file_name(self.lidar_files, "camera")
        self.label_files = self.extract_file_name_from_lidar_file_name(self.lidar_files, "label")
        self._maps = {}           # camera name -> device map, or None for a lens without a model
        self._ident = self._lut = None

    @staticmethod
    def extract_file_name_from_lidar_file_name(lidar_files, name="camera"):
        if name != "camera" and name != "label":
            raise ValueError("parameter error: {}".format(name))
        files = []
        for lidar_file in lidar_files:
            parts = lidar_file.split('/')
            parts[-3] = parts[-3].replace('lidar', name)
            parts[-1] = parts[-1].replace('lidar', name).replace('npz', 'png')
            files.append(os.path.join('/', *parts))
        return files

    @staticmethod
    def get_save_file_name(file_name):
        return file_name.split('/')[-1].replace('label', 'pred').replace('png', 'label')

    # ---- files ----------------------------------------------------------------------------------------------------
    @staticmethod
    def loadLidarData(path):
        return np.load(path)

    @staticmethod
    def loadSemImage(path):
        return np.array(Image.open(path))

    def parsePathInfoByIndex(self, index):
        return index, ''

    # ---- camera image ---------------------------------------------------------------------------------------------
    def _camera_key(self, index):
        """'frontcenter' of '..._camera_frontcenter_000000091.png' -> 'front_center'; None for a name without a camera"""
        name = self.camera_files[index].split('/')[-1].split('.')[0].split('_')[2]
        if name not in _CAMERAS:
            return None
        cut = 5 if name[0] == 'f' else 4
        return name[:cut] + '_' + name[cut:]

    def undistortMap(self, cam_key, h, w):
        """the camera's int32[h, w, 2] device map, built on first use; None where the reference returns the image as it is
        (no camera of that name, or a lens that is neither 'Telecam' nor 'Fisheye')"""
        key = (cam_key, h, w)
        if key not in self._maps:
            cam = self.cams_lidars['cameras'][cam_key] if cam_key is not None else None
            if cam is None or cam['Lens'] not in _LENS:
                self._maps[key] = None
            else:
                self._maps[key] = undistort_map_gpu(cam['Lens'], cam['CamMatrix'], cam['CamMatrixOriginal'],
                                                    cam['Distortion'], h, w, self.device)
        return self._maps[key]

    def loadImageDevice(self, index):
        """the undistorted camera frame, uint8[h, w, 3] on the device: PNG decode, one upload, one remap"""
        image = np.array(Image.open(self.camera_files[index]))
        if image.ndim != 3 or image.shape[2] < 3 or image.dtype != np.uint8:
            raise ValueError("A2D2_PV: %s is not an 8-bit colour image" % self.camera_files[index])
        src = torch.from_numpy(np.ascontiguousarray(image[:, :, :3])).to(self.device)
        m = self.undistortMap(self._camera_key(index), src.shape[0], src.shape[1])
        return src if m is None else remap_gpu(src, m)

    def loadImage(self, index):
        return Image.fromarray(self.loadImageDevice(index).cpu().numpy())

    # ---- points and labels ----------------------------------------------------------------------------------------
    @staticmethod
    def rgb_to_hex(color):
        return '#%02x%02x%02x' % (int(color[0]), int(color[1]), int(color[2]))

    @staticmethod
    def _pixel_index(lidar_data):
        return (lidar_data['row'] + 0.5).astype(np.int32), (lidar_data['col'] + 0.5).astype(np.int32)

    def _unknown(self, rgb, first):
        return KeyError(self.rgb_to_hex(rgb[first]))

    def getLabel(self, lidar_data, sem_image):
        points = lidar_data['points']
        if len(points) == 0:
            return np.zeros(0, np.int32)
        rows, cols = self._pixel_index(lidar_data)
        rgb = np.ascontiguousarray(sem_image[rows, cols][:, :3])
        o = a2d2_index_gpu(points, lidar_data['reflectance'], rows, cols, rgb, self._keys, self._cls, 1.0, self.device)
        if o["meta"][4]:
            raise self._unknown(rgb, o["meta"][5])
        return o["sem"].cpu().numpy()

    def labelMapping(self, label):
        return label

    def loadPointcloud(self, index):
        """float64[P, 4] = x, y, z, reflectance: the first item of loadDataByIndex, without the label lookup"""
        lidar_data = self.loadLidarData(self.lidar_files[index])
        return np.concatenate((lidar_data['points'], np.expand_dims(lidar_data['reflectance'], axis=1)), axis=1)

    def loadDataByIndex(self, index):
        lidar_data = self.loadLidarData(self.lidar_files[index])
        pointcloud = np.concatenate((lidar_data['points'], np.expand_dims(lidar_data['reflectance'], axis=1)), axis=1)
        if self.has_label:
            semantic_label = self.getLabel(lidar_data, self.loadSemImage(self.label_files[index]))
        else:
            semantic_label = np.zeros(pointcloud.shape[0], dtype=np.int32)
        return pointcloud, semantic_label, np.zeros(pointcloud.shape[0], dtype=np.int32)

    def loadLabelByIndex(self, index):
        lidar_data = self.loadLidarData(self.lidar_files[index])
        nums = len(lidar_data['points'])
        if self.has_label:
            semantic_label = self.getLabel(lidar_data, self.loadSemImage(self.label_files[index]))
        else:
            semantic_label = np.zeros(nums, dtype=np.int32)
        return semantic_label, np.zeros(nums, dtype=np.int32)

    def mapLidar2Camera(self, index, pointcloud, img_h, img_w):
        lidar_data = self.loadLidarData(self.lidar_files[index])
        rows, cols = self._pixel_index(lidar_data)
        return np.stack((rows, cols), 1), np.full(len(lidar_data['points']), True, dtype=bool)

    def mapLidar2CameraCropYaw(self, index, pointcloud):
        mapped_points, keep_mask = self.mapLidar2Camera(index, pointcloud, None, None)
        return pointcloud, mapped_points.reshape(-1, 2), keep_mask

    # ---- the frame on the device ----------------------------------------------------------------------------------
    def projectDevice(self, index, image_dev, img_scale=1.0):
        """-> (proj f32[10,h,w], xy_index f64[P,2], depth f32[P], keep bool[P], extra) as _project_frame_v2 returns them;
        ``image_dev``: the camera frame already rescaled by ``img_scale`` (uint8 [ih, iw, 3] on the device)."""
        from ..perspective_view_loader import image_to_device
        dev = torch.device(self.device)
        lidar_data = self.loadLidarData(self.lidar_files[index])
        points = lidar_data['points']
        P = len(points)
        if P == 0:
            raise ValueError("A2D2_PV: frame %s has no points" % self.lidar_files[index])
        rows, cols = self._pixel_index(lidar_data)
        rgb = None
        if self.has_label:
            rgb = np.ascontiguousarray(self.loadSemImage(self.label_files[index])[rows, cols][:, :3])
        o = a2d2_index_gpu(points, lidar_data['reflectance'], rows, cols, rgb, self._keys, self._cls, img_scale, dev)
        x_min, x_max, y_min, y_max, n_unknown, first = o["meta"]
        if n_unknown:
            raise self._unknown(rgb, first)
        h, w = x_max - x_min + 1, y_max - y_min + 1
        img = image_to_device(image_dev, dev)
        if self._ident is None or self._ident.shape[0] < P:     # every point is kept: row k is its own source
            self._ident = torch.arange(max(P, 1 << 16), dtype=torch.int32, device=dev)
        if self._lut is None:                                    # labelMapping is the identity
            self._lut = torch.arange(MAX_COLOURS, dtype=torch.int32, device=dev)
        proj = torch.empty((10, h, w), dtype=torch.float32, device=dev)
        pix = torch.empty(h * w, dtype=torch.int32, device=dev)
        L.check(L.lib().pmf_project_v2_scatter(o["pts"].data_ptr(), o["sem"].data_ptr(), self._ident.data_ptr(),
                                               o["x_data"].data_ptr(), o["y_data"].data_ptr(), o["depth"].data_ptr(), P,
                                               img.data_ptr(), img.shape[0], img.shape[1], self._lut.data_ptr(),
                                               self._lut.shape[0], x_min, y_min, h, w, proj.data_ptr(), pix.data_ptr(),
                                               _stream(dev)), "pmf_project_v2_scatter")
        extra = dict(x_data=o["x_data"], y_data=o["y_data"], src=self._ident[:P], sem=o["sem"], lut=self._lut, x_min=x_min,
                     y_min=y_min)
        return proj, o["xy"], o["depth"], torch.ones(P, dtype=torch.bool, device=dev), extra

    def __len__(self):
        return len(self.lidar_files)

    def __getitem__(self, index):
        """(lidar_data, undistorted image uint8[h, w, 3], labels), the reference's raw triple (:301-306)"""
        lidar_data = self.loadLidarData(self.lidar_files[index])
        image = np.asarray(self.loadImage(index))
        return lidar_data, image, self.getLabel(lidar_data, self.loadSemImage(self.label_files[index]))
