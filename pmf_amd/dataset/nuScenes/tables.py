"""nuScenes without the devkit: the JSON tables, the quaternions and the two dataset classes of the reference
(pc_processor/dataset/nuScenes/dataset_nuscenes.py:74-345 ``Nuscenes``, dataset_nuscenes_v2.py:77-413 ``NuscenesV2``).

Host side, stdlib ``json`` + numpy + Pillow: ``NuTables`` joins the handful of tables the readers use, the scene lists of the
splits come from ``nuscenes.utils.splits`` when that imports and from a JSON file otherwise.  The per-point work of
``mapLidar2Camera`` / ``mapLidar2CameraCropYaw`` -- four rigid transforms of the float32 sweep and the pinhole, which the
reference runs in numpy per camera view after reading the sweep file again -- is ``pmf_nus_project``
(include/pmf_amd_nus.h): the raw ``.pcd.bin`` rows are uploaded once per sweep and kept for its following views, the 57
doubles of a (lidar, camera) pair are built once.  ``NuscenesV2Native.projectDevice`` adds ``pmf_project_v2_scatter``, so
``PerspectiveViewLoaderV2`` serves the dataset in its training, validation and return_uproj layouts.

Parity with the devkit's own output is unpinned (no fixture could be made with it): np.dot's summation order in the
rotations and, with NumPy < 2, a translation vector rounded to float32 before the addition move a coordinate by at most one
float32 ulp per step.  No CPU path for the projection: without a GPU the two map methods raise."""
import ctypes as C
import json
import math
import os
import threading

import numpy as np

VERSIONS = ("v1.0-trainval", "v1.0-test", "v1.0-mini")
TABLES = ("scene", "sample", "sample_data", "calibrated_sensor", "ego_pose", "sensor", "category", "lidarseg")
CAMERA_CHANNELS = ("CAM_FRONT", "CAM_FRONT_RIGHT", "CAM_BACK_RIGHT", "CAM_BACK", "CAM_BACK_LEFT", "CAM_FRONT_LEFT")
# the key of the scene list that plays `train_scenes` in the reference's constructors (:84-91 / :87-94)
TRAIN_LIST = {"v1.0-trainval": "train", "v1.0-test": "test", "v1.0-mini": "mini_train"}
SPLIT_KEYS = ("train", "val", "test", "mini_train", "mini_val")
MINI_SPLITS_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "mini_splits.json")

# the reference's settings for nuScenes-lidarseg, as data: the 32 category names -> its 16 classes + `ignore`, the class
# numbers, and the yaw window of each camera in degrees (dataset_nuscenes.py:20-72, dataset_nuscenes_v2.py:137-144)
CLASSES_PATH = os.path.join(os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))),
                            "tests", "golden", "nuscenes", "lidarseg_classes.json")


def quaternion_rotation_matrix(w, x, y, z):
    """float64[3, 3] of the quaternion (w, x, y, z), normalised first as pyquaternion's ``rotation_matrix`` does"""
    q = np.array([w, x, y, z], np.float64)
    n = math.sqrt(float(np.dot(q, q)))
    if not n > 0.0:
        raise ValueError("quaternion_rotation_matrix: the zero quaternion has no rotation")
    w, x, y, z = (float(v) for v in q / n)
    return np.array([[1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - z * w), 2.0 * (x * z + y * w)],
                     [2.0 * (x * y + z * w), 1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z - x * w)],
                     [2.0 * (x * z - y * w), 2.0 * (y * z + x * w), 1.0 - 2.0 * (x * x + y * y)]], np.float64)


class NuTables(object):
    """The tables of ``<root>/<version>/*.json`` with the devkit's token index and its reverse index: ``sample['data']
    [channel]`` is the token of the key-frame ``sample_data`` record of that channel (``calibrated_sensor`` -> ``sensor``)."""

    def __init__(self, root, version):
        self.dataroot, self.version = root, version
        folder = os.path.join(root, version)
        if not os.path.isdir(folder):
            raise FileNotFoundError("NuTables: no table folder %s" % folder)
        self._index = {}
        for name in TABLES:
            path = os.path.join(folder, name + ".json")
            if name == "lidarseg" and not os.path.exists(path):
                rows = []                                     # the test set ships without labels
            else:
                with open(path) as f:
                    rows = json.load(f)
            setattr(self, name, rows)
            self._index[name] = {r["token"]: r for r in rows}
        for s in self.sample:
            s["data"] = {}
        for sd in self.sample_data:
            cs = self.get("calibrated_sensor", sd["calibrated_sensor_token"])
            sensor = self.get("sensor", cs["sensor_token"])
            sd["sensor_modality"], sd["channel"] = sensor["modality"], sensor["channel"]
            if sd["is_key_frame"]:
                self.get("sample", sd["sample_token"])["data"][sd["channel"]] = sd["token"]

    def get(self, table, token):
        if table not in self._index:
            raise KeyError("NuTables: no table %r (have %s)" % (table, ", ".join(TABLES)))
        return self._index[table][token]

    @property
    def lidarseg_idx2name_mapping(self):
        out = {}
        for c in self.category:
            if "index" not in c:
                raise ValueError("NuTables: category.json of %s has no `index` field -- it is the one of the nuScenes-lidarseg "
                                 "table set (category.json and lidarseg.json of the lidarseg download replace the detection "
                                 "set's)" % os.path.join(self.dataroot, self.version))
            out[c["index"]] = c["name"]
        return out

    def path(self, sample_data_token):
        return os.path.join(self.dataroot, self.get("sample_data", sample_data_token)["filename"])


def scene_splits(version, splits_path=None):
    """{list name: scene names}, or None when every scene of the tables belongs to the version's own list (v1.0-test).  A
    file given by the caller comes first, then nuscenes.utils.splits if it imports, then what needs no list."""
    if splits_path is None:
        try:
            from nuscenes.utils import splits
            return {k: list(getattr(splits, k)) for k in SPLIT_KEYS}
        except ImportError:
            pass
        if version == "v1.0-mini":
            splits_path = MINI_SPLITS_PATH
    if splits_path is not None:
        with open(splits_path) as f:
            lists = json.load(f)
        if TRAIN_LIST[version] not in lists and version == "v1.0-test":
            return None             # a file with the train / val names only: every scene of the test tables is a test scene
        if TRAIN_LIST[version] not in lists:
            raise ValueError("nuScenes: %s has no `%s` list, which %s needs" % (splits_path, TRAIN_LIST[version], version))
        return lists
    if version == "v1.0-test":
        return None
    raise ValueError("nuScenes %s: the scene names of the train / val split are not part of the data set.  Pass "
                     "splits_path= (config key nus_splits): a JSON file with the keys %s, written from "
                     "nuscenes-devkit's python-sdk/nuscenes/utils/splits.py" % (version, ", ".join(SPLIT_KEYS)))


def _stream(dev):
    import torch
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


class _NativeBase(object):
    def __init__(self, root, version='v1.0-trainval', split='train', return_ref=False, has_image=True, has_pcd=True,
                 has_label=True, splits_path=None, classes_path=None, device="cuda"):
        if version not in VERSIONS:
            raise ValueError("nuScenes: version %r is none of %s" % (version, ", ".join(VERSIONS)))
        self.split, self.data_path, self.return_ref, self.has_image = split, root, return_ref, has_image
        self.device = device
        self.nusc = NuTables(root, version)
        lists = scene_splits(version, splits_path)
        self._train_names = None if lists is None else set(lists[TRAIN_LIST[version]])
        with open(CLASSES_PATH if classes_path is None else classes_path) as f:
            settings = json.load(f)
        number = settings["class_index"]
        self.map_name_from_general_index_to_segmentation_index = {
            raw: number[settings["general_to_class"][name]] for raw, name in self.nusc.lidarseg_idx2name_mapping.items()}
        self.mapped_cls_name = {k: name for name, k in number.items()}
        self.fov_angle = {ch: {"fov_left": lo, "fov_right": hi} for ch, (lo, hi) in settings["fov_angle"].items()}
        self._chains = {}               # (lidar token, camera token) -> the 57 doubles of pmf_nus_project
        self._local = threading.local()  # per thread: the sweep on the device (_sweep_device)
        self.token_list = self._token_list()
        print("{}: {} sample: {}".format(version, self.split, len(self.token_list)))

    def __getstate__(self):             # a DataLoader worker process starts without device state
        state = dict(self.__dict__)
        state.pop("_local", None)
        return state

    def __setstate__(self, state):
        self.__dict__.update(state)
        self._local = threading.local()

    def _is_train_scene(self, scene):
        return self._train_names is None or scene["name"] in self._train_names

    def _first_lidar_path(self, scene):
        sample = self.nusc.get("sample", scene["first_sample_token"])
        return self.nusc.path(sample["data"]["LIDAR_TOP"])

    # ---- the reference's surface ------------------------------------------------------------------------------------
    def __len__(self):
        return len(self.token_list)

    def parsePathInfoByIndex(self, index):
        return index, ''

    def _lidar_token(self, index):
        return self.token_list[index]['lidar_token'] if self.has_image else self.token_list[index]

    def _raw_rows(self, index):
        """the sweep file as it is: f32[P, 5] = x, y, z, intensity, ring"""
        return np.fromfile(self.nusc.path(self._lidar_token(index)), dtype=np.float32).reshape((-1, 5))

    def loadLabelByIndex(self, index):
        """uint8[P, 1] raw lidarseg ids; None on the test split, which has no label files"""
        if self.split == 'test':
            return None
        record = self.nusc.get('lidarseg', self._lidar_token(index))
        return np.fromfile(os.path.join(self.data_path, record['filename']), dtype=np.uint8).reshape((-1, 1))

    def loadDataByIndex(self, index):
        """(points f32[P, 4], raw labels [P, 1] -- zeros of the platform's int on the test split --, instance ids i32[P] = 0)"""
        points = self._raw_rows(index)[:, :4]
        labels = self.loadLabelByIndex(index)
        if labels is None:
            labels = np.zeros((points.shape[0], 1), dtype=int)
        return points, labels, np.zeros(points.shape[0], dtype=np.int32)

    def labelMapping(self, sem_label):
        """raw ids [n, 1] -> class numbers [n]; an id outside the category table is a KeyError"""
        sem_label = np.asarray(sem_label)
        if sem_label.ndim != 2 or sem_label.shape[1] != 1:
            raise ValueError("labelMapping: labels are [n, 1], got %s" % (sem_label.shape,))
        table = self.map_name_from_general_index_to_segmentation_index
        ids, where = np.unique(sem_label[:, 0], return_inverse=True)
        return np.array([table[int(v)] for v in ids], dtype=np.int64)[where.reshape(-1)]

    def loadImage(self, index):
        from PIL import Image
        return Image.open(self.nusc.path(self.token_list[index]['cam_token']))

    # ---- the projection chain on the device ---------------------------------------------------------------------------
    def _chain(self, index):
        """R1 t1 R2 t2 t3 R3 t4 R4 K of the view's (lidar, camera) pair: transposes and signs are taken here, exactly"""
        pair = self.token_list[index]
        key = (pair['lidar_token'], pair['cam_token'])
        chain = self._chains.get(key)
        if chain is None:
            get = self.nusc.get
            lidar, cam = get('sample_data', key[0]), get('sample_data', key[1])
            if not lidar['is_key_frame'] or lidar['sensor_modality'] != 'lidar':
                raise ValueError("nuScenes: %s is no key-frame lidar record (only those carry lidarseg labels)" % key[0])
            R = lambda rec: quaternion_rotation_matrix(*rec['rotation'])
            t = lambda rec: np.asarray(rec['translation'], np.float64)
            cs_l, pose_l = get('calibrated_sensor', lidar['calibrated_sensor_token']), get('ego_pose', lidar['ego_pose_token'])
            cs_c, pose_c = get('calibrated_sensor', cam['calibrated_sensor_token']), get('ego_pose', cam['ego_pose_token'])
            parts = [R(cs_l), t(cs_l), R(pose_l), t(pose_l), -t(pose_c), R(pose_c).T, -t(cs_c), R(cs_c).T,
                     np.asarray(cs_c['camera_intrinsic'], np.float64)]
            chain = np.ascontiguousarray(np.concatenate([np.ravel(p) for p in parts]))
            assert chain.shape == (57,)
            self._chains[key] = chain           # two threads may both build it: equal values, one assignment each
        return chain

    def _sweep_device(self, index):
        """(raw rows f32[P, 5], raw labels i32[P], label table i32[256]) of the view's sweep on the device: one packed upload
        per sweep, kept for the following views of the same lidar token.  The entry belongs to the calling thread and to the
        HIP stream it was made on -- the loaders' prefetch threads build items concurrently, each on a stream of its own -- so
        no thread ever sees another's tensors, and a thread that changes streams uploads again.  The caller takes the tuple
        once per item."""
        import torch
        token = self._lidar_token(index)
        dev = torch.device(self.device)
        if dev.type != "cuda":
            raise RuntimeError("nuScenes: the projection chain runs on the GPU only (device=%s)" % self.device)
        stream = torch.cuda.current_stream(dev).cuda_stream
        entry = getattr(self._local, "sweep", None)
        if entry is None or entry[0] != (token, stream):
            from ..perspective_view_loader import upload_packed
            raw = self._raw_rows(index)
            labels = self.loadLabelByIndex(index)
            sem = np.zeros(raw.shape[0], np.int32) if labels is None else labels.reshape(-1).astype(np.int32)
            if sem.shape[0] != raw.shape[0]:
                raise ValueError("nuScenes: sweep %s has %d points and %d labels" % (token, raw.shape[0], sem.shape[0]))
            keys = sorted(self.map_name_from_general_index_to_segmentation_index)
            lut = np.zeros(256, np.int32)           # labelMapping as a 256-entry table, as the loaders build it
            lut[keys] = self.labelMapping(np.asarray(keys, np.uint8)[:, None])
            entry = ((token, stream),) + tuple(upload_packed([raw, sem, lut], dev))
            self._local.sweep = entry
        return entry[1:]

    def _project(self, index, pts, mode, min_dist, bound_h=0.0, bound_w=0.0, row_scale=1.0, col_scale=1.0, img_scale=1.0):
        """pmf_nus_project of view ``index`` on ``pts``, the device rows of its sweep"""
        fov = (0.0, 0.0)
        if mode == 1:
            angle = self.fov_angle[self.token_list[index]["cam_channel"]]
            quarter = math.pi / 2.0                  # yaw is measured from the camera's x axis, the windows from its z axis
            fov = (math.radians(angle["fov_left"]) - quarter, math.radians(angle["fov_right"]) - quarter)
        return nus_project_gpu(pts, self._chain(index), mode, min_dist, fov[0], fov[1], bound_h, bound_w, row_scale,
                               col_scale, img_scale)

    def mapLidar2Camera(self, index, pointcloud, img_h, img_w, min_dist: float = 1.0, **unused):
        """-> ((row, col) f64[K, 2], mask bool[P]); ``pointcloud`` is not read, the sweep of ``index`` is (as in the
        reference, which loads the file again).  ``img_h`` bounds the COLUMN and ``img_w`` the row, as there."""
        if img_h is None or img_w is None:
            raise ValueError("mapLidar2Camera: img_h / img_w are needed (the unbounded form is not part of pmf_nus_project)")
        o = self._project(index, self._sweep_device(index)[0], 0, min_dist, float(img_h), float(img_w))
        return o["xy"].cpu().numpy(), o["keep"].cpu().numpy().astype(np.bool_)


def nus_project_gpu(points, chain, mode, min_dist, fov_lo, fov_hi, bound_h, bound_w, row_scale, col_scale, img_scale):
    """pmf_nus_project on the rows ``points`` f32[P, 4 or 5] (device tensor) -> dict of device tensors keep u8[P], src,
    crop, xy, x_data, y_data, depth (K rows each) and the host ints K, x_min, x_max, y_min, y_max -- the one host read, the
    frame size being data.  K = 0 raises ValueError."""
    import torch
    from ... import _lib as L
    assert points.is_cuda and points.dtype == torch.float32 and points.is_contiguous() and points.dim() == 2
    dev, (P, stride) = points.device, points.shape
    chain = np.ascontiguousarray(chain, np.float64)
    assert chain.shape == (L.NUS_CHAIN,)
    n = max(P, 1)
    keep = torch.empty(n, dtype=torch.uint8, device=dev)
    i32 = torch.empty((3, n), dtype=torch.int32, device=dev)
    crop = torch.empty((n, 4), dtype=torch.float32, device=dev)
    xy = torch.empty((n, 2), dtype=torch.float64, device=dev)
    depth = torch.empty(n, dtype=torch.float32, device=dev)
    meta = torch.zeros(5, dtype=torch.int32, device=dev)
    blk = torch.empty((n + L.NUS_BLOCK - 1) // L.NUS_BLOCK + 1, dtype=torch.int32, device=dev)
    L.check(L.lib().pmf_nus_project(points.data_ptr(), P, stride, chain.ctypes.data, int(mode), float(min_dist),
                                    float(fov_lo), float(fov_hi), float(bound_h), float(bound_w), float(row_scale),
                                    float(col_scale), float(img_scale), keep.data_ptr(), i32[0].data_ptr(), crop.data_ptr(),
                                    xy.data_ptr(), i32[1].data_ptr(), i32[2].data_ptr(), depth.data_ptr(), meta.data_ptr(),
                                    blk.data_ptr(), _stream(dev)), "pmf_nus_project")
    K, x_min, x_max, y_min, y_max = [int(v) for v in meta.tolist()]
    if K == 0:
        raise ValueError("nuScenes: the camera view keeps no point of the sweep")
    return dict(keep=keep[:P], src=i32[0, :K], crop=crop[:K], xy=xy[:K], x_data=i32[1, :K], y_data=i32[2, :K],
                depth=depth[:K], K=K, x_min=x_min, x_max=x_max, y_min=y_min, y_max=y_max)


class NuscenesNative(_NativeBase):
    """dataset_nuscenes.py:74-345.  Scenes whose first LIDAR_TOP file is missing are skipped; as in the reference the token
    lists walk the ``sample`` table, and a sample of a scene that is not a (present) training scene goes to ``val``."""

    def _token_list(self):
        train_scenes = set(s["token"] for s in self.nusc.scene
                           if os.path.exists(self._first_lidar_path(s)) and self._is_train_scene(s))
        train_list, val_list = [], []
        for sample in self.nusc.sample:
            lidar_token = sample['data']['LIDAR_TOP']
            out = train_list if sample['scene_token'] in train_scenes else val_list
            if self.has_image:
                out.extend({'lidar_token': lidar_token, 'cam_token': sample['data'][c]} for c in CAMERA_CHANNELS)
            else:
                out.append(lidar_token)
        if self.split == "train" or self.split == "test":
            return train_list
        if self.split == "val":
            return val_list
        raise ValueError("invalid split mode: {}".format(self.split))


class NuscenesV2Native(_NativeBase):
    """dataset_nuscenes_v2.py:77-413, plus what PerspectiveViewLoaderV2 asks of a dataset that projects on the device:
    loadImageDevice, loadPointcloud and projectDevice."""
    BACK_SCALE = (0.5, 0.6)         # (row, col) of every camera but CAM_BACK: loadImage halves those images (:207-209,369-371)

    def _token_list(self):
        scenes = []
        for scene in self.nusc.scene:
            path = self._first_lidar_path(scene)
            if not os.path.exists(path):
                raise FileNotFoundError(path)
            if self._is_train_scene(scene):
                if self.split == "train" or self.split == "test":
                    scenes.append(scene)
            elif self.split == "val":
                scenes.append(scene)
        out = []
        for scene in scenes:
            sample_token = scene['first_sample_token']
            while True:
                sample = self.nusc.get('sample', sample_token)
                lidar_token = sample['data']['LIDAR_TOP']
                if self.has_image:
                    out.extend({'lidar_token': lidar_token, 'cam_token': sample['data'][c], 'cam_channel': c,
                                'description': scene["description"]} for c in CAMERA_CHANNELS)
                else:
                    out.append(lidar_token)
                if sample['next'] == "":
                    break
                sample_token = sample['next']
        return out

    def _scales(self, index):
        return (1.0, 1.0) if self.token_list[index]['cam_channel'] == "CAM_BACK" else self.BACK_SCALE

    def loadImage(self, index):
        from PIL import Image
        image = super().loadImage(index)
        if self.token_list[index]['cam_channel'] != "CAM_BACK":
            w, h = image.size                    # torchvision's resize of a PIL image: Pillow's bilinear
            image = image.resize((int(w * 0.6), int(h * 0.5)), Image.BILINEAR)
        return image

    def mapLidar2CameraCropYaw(self, index, pointcloud, min_dist: float = 0.1):
        """-> (camera-frame rows f32[K, 4], (row, col) f64[K, 2], keep bool[P]); ``pointcloud`` is not read (see
        mapLidar2Camera)"""
        rs, cs = self._scales(index)
        o = self._project(index, self._sweep_device(index)[0], 1, min_dist, row_scale=rs, col_scale=cs)
        return o["crop"].cpu().numpy(), o["xy"].cpu().numpy(), o["keep"].cpu().numpy().astype(np.bool_)

    # ---- the frame on the device --------------------------------------------------------------------------------------
    def loadImageDevice(self, index):
        from ..perspective_view_loader import image_to_device
        return image_to_device(np.asarray(self.loadImage(index).convert("RGB")), self.device)

    def loadPointcloud(self, index):
        """f32[P, 4]: the first item of loadDataByIndex, without the label file"""
        return self._raw_rows(index)[:, :4]

    def projectDevice(self, index, image_dev, img_scale=1.0, min_dist=0.1):
        """-> (proj f32[10, h, w], xy_index f64[K, 2], depth f32[K], keep bool[P], extra) as _project_frame_v2 returns them;
        ``image_dev``: the camera frame already rescaled by ``img_scale``.  ``extra``: x_data / y_data, ``src`` the position
        of each kept point in the sweep, ``sem`` the sweep's raw labels, ``lut`` the 256-entry label table, x_min / y_min."""
        import torch
        from ... import _lib as L
        from ..perspective_view_loader import image_to_device
        rs, cs = self._scales(index)
        pts, sem, lut = self._sweep_device(index)         # taken once: points, labels and table of ONE sweep
        o = self._project(index, pts, 1, min_dist, row_scale=rs, col_scale=cs, img_scale=img_scale)
        dev = sem.device
        img = image_to_device(image_dev, dev)
        K, x_min, y_min = o["K"], o["x_min"], o["y_min"]
        h, w = o["x_max"] - x_min + 1, o["y_max"] - y_min + 1
        sem_kept = sem[o["src"].long()]               # row k of the crop is its own source
        ident = torch.arange(K, dtype=torch.int32, device=dev)
        proj = torch.empty((10, h, w), dtype=torch.float32, device=dev)
        pix = torch.empty(h * w, dtype=torch.int32, device=dev)
        L.check(L.lib().pmf_project_v2_scatter(o["crop"].data_ptr(), sem_kept.data_ptr(), ident.data_ptr(),
                                               o["x_data"].data_ptr(), o["y_data"].data_ptr(), o["depth"].data_ptr(), K,
                                               img.data_ptr(), img.shape[0], img.shape[1], lut.data_ptr(), lut.shape[0],
                                               x_min, y_min, h, w, proj.data_ptr(), pix.data_ptr(), _stream(dev)),
                "pmf_project_v2_scatter")
        extra = dict(x_data=o["x_data"], y_data=o["y_data"], src=o["src"], sem=sem, lut=lut, x_min=x_min, y_min=y_min)
        return proj, o["xy"], o["depth"], o["keep"].bool(), extra
