"""Extract the SemanticKITTI-FOV data set from SemanticKITTI: for every sweep the points the left colour camera sees.

    python create_fov_dataset.py --src /path/to/semantic-kitti/sequences --dst /path/to/semantic-kitti-fov/sequences
                                 [--sequences 0 1 ... 10] [--batch-frames 16] [--io-threads 4] [--no-labels] [--overwrite]

The reference's script of the same name with its paths as arguments.  The keep rule runs on the GPU, a batch of frames per
pass, and is the loader's own (pmf_amd.dataset.semantic_kitti.create_fov_dataset): the written tree is exactly what
PerspectiveViewLoader keeps of the raw one.  One line per sequence: frames, kept share, frames/s."""
import argparse
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.abspath(os.path.join(HERE, "..", "..")))

from pmf_amd.dataset.semantic_kitti import create_fov_dataset, fov_filter_gpu  # noqa: E402


def run(src, dst, sequences=tuple(range(11)), batch_frames=16, io_threads=4, has_label=True, overwrite=False,
        config_path=None, filter_fn=fov_filter_gpu, log=print):
    """-> the counts of create_fov_dataset; every destination is checked before the first sequence is written"""
    stats = create_fov_dataset(src, dst, list(sequences), config_path=config_path, batch_frames=batch_frames,
                               io_threads=io_threads, has_label=has_label, overwrite=overwrite, filter_fn=filter_fn)
    for seq in sorted(stats):
        s = stats[seq]
        log("sequence {}: {} frames, kept {:.1f} % of {} points, {:.1f} frames/s".format(
            seq, s["frames"], 100.0 * s["points_kept"] / max(s["points_read"], 1), s["points_read"],
            s["frames"] / max(s["seconds"], 1e-9)))
    return stats


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--src", required=True, help="the sequences folder of SemanticKITTI")
    ap.add_argument("--dst", required=True, help="the sequences folder of SemanticKITTI-FOV to write")
    ap.add_argument("--sequences", type=int, nargs="+", default=list(range(11)))
    ap.add_argument("--batch-frames", type=int, default=16)
    ap.add_argument("--io-threads", type=int, default=4)
    ap.add_argument("--no-labels", action="store_true", help="test sequences: no labels folder is read or written")
    ap.add_argument("--overwrite", action="store_true")
    ap.add_argument("--config", default=None, help="label file (default: the package's semantic-kitti.yaml)")
    a = ap.parse_args(argv)
    run(a.src, a.dst, a.sequences, a.batch_frames, a.io_threads, not a.no_labels, a.overwrite, a.config)


if __name__ == "__main__":
    main()
