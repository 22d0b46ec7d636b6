"""loftr_amd -- MI355X-native LoFTR matching path (hand-written HIP kernels behind a C-ABI).

Public surface mirrors ``src.loftr`` of zju3dv/LoFTR (src/loftr/__init__.py:1-2):
``LoFTR`` and ``default_cfg``.
"""
from .config import default_cfg, full_default_cfg, get_cfg       # noqa: F401
from .loftr import LoFTR                                           # noqa: F401
from .pairs import FeatureBank                                     # noqa: F401
from .atlas import KeypointAtlas, SfmResult                       # noqa: F401
from .triangulation import Points3D, triangulate_tracks           # noqa: F401
from .bundle import BundleResult, bundle_adjust                   # noqa: F401
from .radial import undistort_points, distort_points              # noqa: F401
from .registration import Reconstruction, Registration, reconstruct_tracks, register_images    # noqa: F401
from .completion import Completion, complete_tracks                # noqa: F401
from .merging import Merge, merge_tracks                            # noqa: F401
from .splitting import Split, split_tracks                          # noqa: F401
from .rotations import GlobalRotations, average_rotations     # noqa: F401
from .positions import GlobalPositions, global_positions      # noqa: F401
from .calibration import ViewGraphCalibration, calibrate_view_graph   # noqa: F401
from .refinement import Refinement, RefinePlan, plan_track_refinement, apply_refinement    # noqa: F401
from .alignment import Alignment, align_centres                    # noqa: F401
from .proposals import Overlap, view_overlap, select_pairs, select_database      # noqa: F401
from .localization import LocalizationModel, QueryLocalizer, QueryPoses   # noqa: F401
