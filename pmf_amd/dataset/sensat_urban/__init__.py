from .sensat_urban import SensatUrban, tile_windows  # noqa: F401
