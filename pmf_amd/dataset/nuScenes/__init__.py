"""``pc_processor.dataset.nuScenes``.  The reference's readers (pc_processor/dataset/nuScenes/dataset_nuscenes.py:74-282,
dataset_nuscenes_v2.py:77-375) sit on the third-party nuscenes-devkit; here ``tables.py`` reads the JSON tables itself and
runs the per-point chain of transforms on the device (``open_nuscenes`` -> ``NuscenesNative`` / ``NuscenesV2Native``), which
is what the task entry points build.  ``Nuscenes`` / ``NuscenesV2`` keep their names and only raise, as before.  Everything
behind the dataset -- the per-camera-view loader (nus_perspective_loader.py), the six-camera inference loop
(tasks/pmf_eval_nuscenes/infer.py), the merge with the LiDAR-only fallback (postproc/merge.py) -- takes any object with the
readers' attributes (tests: oracle/cases.py SyntheticNus)."""
from .nus_perspective_loader import NusPerspectiveViewLoader  # noqa: F401
from . import tables  # noqa: F401
from .tables import NuTables, NuscenesNative, NuscenesV2Native, quaternion_rotation_matrix  # noqa: F401


def open_nuscenes(v2, root, version="v1.0-trainval", split="train", **kw):
    """The devkit-free readers of tables.py under one name: ``NuscenesV2Native`` (the EPMF reader) when ``v2``, else
    ``NuscenesNative``.  ``kw``: has_image, splits_path (JSON scene lists, needed for v1.0-trainval when nuscenes-devkit
    is absent), device.  What the task entry points call; ``Nuscenes`` / ``NuscenesV2`` below keep their behaviour."""
    return (NuscenesV2Native if v2 else NuscenesNative)(root, version=version, split=split, **kw)


class Nuscenes(object):
    def __init__(self, root, version="v1.0-trainval", split="train", **kw):
        try:
            import nuscenes  # noqa: F401
        except ImportError as e:
            raise ImportError("pc_processor.dataset.nuScenes.Nuscenes needs the nuscenes-devkit package (pip install "
                              "nuscenes-devkit), which is not installed in this environment") from e
        raise NotImplementedError("nuScenes table reader: install nuscenes-devkit and plug a dataset object with "
                                  "loadDataByIndex / loadImage / parsePathInfoByIndex / proj_matrix / class_map_lut "
                                  "into PerspectiveViewLoader (INTEGRATION.md)")


class NuscenesV2(object):
    """pc_processor/dataset/nuScenes/dataset_nuscenes_v2.py (the EPMF reader: mapLidar2CameraCropYaw, per-camera yaw
    windows): the same devkit dependency as Nuscenes.  PerspectiveViewLoaderV2 and tasks/epmf_eval_nuscenes take any
    object with its attributes."""

    def __init__(self, root, version="v1.0-trainval", split="train", **kw):
        try:
            import nuscenes  # noqa: F401
        except ImportError as e:
            raise ImportError("pc_processor.dataset.nuScenes.NuscenesV2 needs the nuscenes-devkit package (pip install "
                              "nuscenes-devkit), which is not installed in this environment") from e
        raise NotImplementedError("nuScenes table reader: install nuscenes-devkit and plug a dataset object with "
                                  "loadDataByIndex / loadImage / parsePathInfoByIndex / mapLidar2CameraCropYaw / "
                                  "labelMapping / token_list into PerspectiveViewLoaderV2 (INTEGRATION.md)")
