from .knn import KNN  # noqa: F401
from .merge import getMergePred  # noqa: F401
from .frame_eval import (FrameEvaluator, SweepEvaluator, RangeSweepEvaluator, range_batch_eval, pad_geometry,  # noqa: F401
                         pad_geometry_bottom, fill_labels, sweep_finish_fill)
from .fov_fill import fov_fill  # noqa: F401
from .bev_eval import BevTileEvaluator, tile_windows, bev_tile_pre, bev_tile_accum, bev_points  # noqa: F401
