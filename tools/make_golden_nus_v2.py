"""tests/golden/g16_nus_v2.npz: the reference's own PerspectiveViewLoaderV2 (return_uproj=True, is_train=False) executed on
the synthetic NuscenesV2-type dataset of tests/nus_v2_cases.py -- every view's proj / xy_index / depth / keep_mask.

    python tools/make_golden_nus_v2.py /path/to/reference

The reference is imported by file path; cv2 and torchvision (not installed; the return_uproj path only constructs their
objects) get the same name-only stand-ins oracle/make_golden.py uses.  Arrays only."""
import importlib.util
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests.nus_v2_cases import GOLDEN, SyntheticNusV2  # noqa: E402


def main(ref):
    from PIL import Image
    cv2 = types.ModuleType("cv2")
    cv2.rotate = lambda *a, **k: None
    tv = types.ModuleType("torchvision")
    tvt = types.ModuleType("torchvision.transforms")
    for n in ("ColorJitter", "Pad", "Compose", "RandomHorizontalFlip", "RandomRotation", "RandomCrop", "CenterCrop", "Resize"):
        setattr(tvt, n, type(n, (), {"__init__": lambda self, *a, **k: None}))
    tv.transforms = tvt
    sys.modules.update({"cv2": cv2, "torchvision": tv, "torchvision.transforms": tvt})
    spec = importlib.util.spec_from_file_location(
        "refpc_loader_v2", os.path.join(ref, "pc_processor", "dataset", "perspective_view_loader_v2.py"))
    V2 = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(V2)

    class PilImages(SyntheticNusV2):          # the reference loader reads image.size: a PIL image
        def loadImage(self, index):
            return Image.fromarray(SyntheticNusV2.loadImage(self, index))

    ds = PilImages()
    cfg = {"PVconfig": {"proj_h": 64, "proj_w": 128, "proj_ht": 64, "proj_wt": 128, "img_jitter": [0.4, 0.4, 0.4]}}
    ld = V2.PerspectiveViewLoaderV2(ds, cfg, is_train=False, return_uproj=True)
    out = {}
    for i in range(len(ds)):
        proj, xy, depth, keep, _ = ld[i]
        out["v%d.proj" % i] = proj.numpy()
        out["v%d.xy" % i] = xy.numpy()
        out["v%d.depth" % i] = depth.numpy()
        out["v%d.keep" % i] = keep.numpy()
    np.savez_compressed(GOLDEN, **out)
    print("g16_nus_v2:", [out["v%d.proj" % i].shape for i in range(len(ds))], os.path.getsize(GOLDEN), "bytes")


if __name__ == "__main__":
    main(sys.argv[1])
