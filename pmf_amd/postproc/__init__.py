from .knn import KNN  # noqa: F401
from .merge import getMergePred  # noqa: F401
from .frame_eval import FrameEvaluator, SweepEvaluator, pad_geometry, pad_geometry_bottom  # noqa: F401
