"""collab_splats_amd -- MI355X-native (gfx950) RaDe-GS splat rasterizer behind the
gsplat-rade call surface that BasisResearch/collab-splats uses.

Only the hot path of BASELINE.json's north_star lives here.  Compute is in
``libmisplat.so`` (hand-written HIP, C ABI: include/misplat.h); this package is the thin Python
host side.  There is no CPU fallback.
"""
from ._lib import MisplatError, load as load_library  # noqa: F401
from .rendering import rasterization  # noqa: F401
from .wrapper import fully_fused_projection, spherical_harmonics  # noqa: F401
from .strategy import DefaultStrategy, MCMCStrategy  # noqa: F401
from .mcmc import (RelocationStrategy, compute_relocation, inject_noise_to_position, relocate, sample_add,  # noqa: F401
                   sample_by_opacity)
from .ops import set_deterministic  # noqa: F401
from .optim import FusedAdam, step_all as fused_adam_step_all  # noqa: F401
from .optim import SelectiveAdam, selective_step_all as selective_adam_step_all, visibility_from_radii  # noqa: F401
from .tsdf import TSDFVolume, write_ply  # noqa: F401
from .meshmap import features2vertex, normals2vertex  # noqa: F401
from .meshquery import cluster_labels, mesh_clustering, query_similarity, similarity_colors  # noqa: F401
from .pointcloud import (calculate_accuracy, calculate_completeness, clean_pcd, density_filter,  # noqa: F401
                         knn_mean_distance, radius_count, remove_far_points, remove_statistical_outlier,
                         statistical_outlier_mask, voxel_down_sample)
from .meshclean import (align_floor, fill_holes, filter_mesh_components, mesh_components, mesh_edge_stats,  # noqa: F401
                        mesh_holes, plane_inlier_counts, ransac_planes, sample_surface, segment_plane, smooth_laplacian)
from .decimate import simplify_quadric_decimation  # noqa: F401
from .meshfill import fair_vertices, fair_vertices_curvature, fill_holes_nicely, flip_edges, subdivide_mesh, triangulate_holes  # noqa: F401
from .depthcloud import backproject, depth_edges, depth_normal_cloud, gaussian_mask_filter, sample_pixels  # noqa: F401
from .featureloss import TwoLayerMLP, feature_decode, feature_loss  # noqa: F401
from .bilagrid import BilateralGrid, bilagrid_slice, bilagrid_tv_loss  # noqa: F401
from .camera_opt import CameraOptimizer  # noqa: F401
from .textquery import TextQuery, fold_text_queries, gaussian_similarity, similarity_map  # noqa: F401
from .poisson import (poisson_grid, poisson_reconstruct, poisson_solve, poisson_splat, poisson_system,  # noqa: F401
                      poisson_trim)
from .density import DensityField, gaussian_density, gaussian_density_grad, level_surface_points  # noqa: F401
from .pointtsdf import PointTSDFVolume  # noqa: F401
from .identity import (IdentityField, IdentityNeighbours, identity_3d_loss, identity_labels, identity_loss,  # noqa: F401
                       identity_neighbours)
from .metrics import (color_correct, color_corrected_metrics, depth_metrics, image_metrics, mean_angular_error,  # noqa: F401
                      normal_metrics, psnr, ssim)
from .grouping import FrontGaussians, MemoryBank, convert_matched_mask, front_gaussians, project_gaussians  # noqa: F401

__version__ = "0.1.0"


def install_gsplat_alias() -> None:
    """Make ``from gsplat.rendering import rasterization``, ``from gsplat.strategy import
    DefaultStrategy`` and ``from gsplat.cuda._wrapper import fully_fused_projection,
    spherical_harmonics`` (the reference's imports: rade_gs_model.py:15-20) resolve to this build."""
    import sys
    import types
    from . import rendering, strategy, wrapper

    if "gsplat" in sys.modules and not getattr(sys.modules["gsplat"], "__misplat_alias__", False):
        raise RuntimeError("a real 'gsplat' is already imported; refusing to shadow it")
    pkg = types.ModuleType("gsplat")
    pkg.__misplat_alias__ = True
    pkg.__path__ = []
    pkg.__version__ = "1.5.0+misplat"
    cuda = types.ModuleType("gsplat.cuda")
    cuda.__path__ = []
    cuda._wrapper = wrapper
    pkg.rendering, pkg.strategy, pkg.cuda = rendering, strategy, cuda
    pkg.rasterization = rendering.rasterization
    pkg.DefaultStrategy = strategy.DefaultStrategy
    pkg.MCMCStrategy = strategy.MCMCStrategy

    def _missing(modname):
        def __getattr__(name):
            if name.startswith("__"):
                raise AttributeError(name)
            raise ImportError(f"'{modname}.{name}' is not provided by collab_splats_amd's gsplat alias: only the "
                              f"RaDe-GS rasterizer path is built (rasterization, fully_fused_projection, "
                              f"spherical_harmonics, DefaultStrategy; MCMCStrategy is a placeholder)")
        return __getattr__

    pkg.__getattr__ = _missing("gsplat")
    cuda.__getattr__ = _missing("gsplat.cuda")
    sys.modules.update({"gsplat": pkg, "gsplat.rendering": rendering, "gsplat.strategy": strategy,
                        "gsplat.cuda": cuda, "gsplat.cuda._wrapper": wrapper})
