from .knn import KNN  # noqa: F401
from .merge import getMergePred  # noqa: F401
from .frame_eval import FrameEvaluator, pad_geometry  # noqa: F401
