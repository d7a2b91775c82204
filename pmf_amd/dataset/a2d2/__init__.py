from .dataset_a2d2 import (A2D2_PV, a2d2_index_gpu, colour_table, remap_gpu, undistort_map_gpu,  # noqa: F401
                           mapped_class_name, cls_freq, unused_index, zero_size_index)
