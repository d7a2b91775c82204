from .parser import SemanticKitti, write_prediction, DEFAULT_CONFIG  # noqa: F401
from .fov import fov_filter_gpu, create_fov_dataset  # noqa: F401
