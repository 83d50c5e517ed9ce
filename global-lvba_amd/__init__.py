"""global-lvba_amd -- MI355X-native LM-refinement hot path of Global-LVBA behind a C-ABI.

The directory name (with a hyphen) is fixed by the build contract; import it with
`importlib.import_module("global-lvba_amd")` or through the `lvba_amd` alias module at the repo root.
"""
from . import _lib
from .balm import BALM2, IMUST, VOX_HESS, BalmProblem, Prior, shard_range
from .visual import DepthImages, VisualProblem, fuse_tracks, optimize_camera_poses
from .voxel import Scans, VoxelMap
from .mapq import map_quality_points, map_quality_scans
from . import register
from . import features
from .features import extract as extract_features, sift_opts

__all__ = ["BALM2", "IMUST", "VOX_HESS", "BalmProblem", "Prior", "shard_range", "VisualProblem", "optimize_camera_poses", "VoxelMap", "Scans",
           "map_quality_scans", "map_quality_points", "register", "features", "extract_features", "sift_opts",
           "_lib"]
