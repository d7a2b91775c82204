from .sensat_urban import SensatUrban, tile_windows  # noqa: F401
from .prepare import compute_bev_feature  # noqa: F401
from .sensat_loader import SensatLoader  # noqa: F401
