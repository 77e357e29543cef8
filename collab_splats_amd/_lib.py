"""ctypes binding of libmisplat.so (the C ABI declared in include/misplat.h).

``SYMBOLS`` holds the signature of every entry point; ``load()`` sets ``restype`` and ``argtypes`` from it, so call sites pass
plain Python values and ctypes converts each to the C type the header declares (a float for an ``int64_t`` raises).  ``run``
calls an entry that returns a status on the current stream.  A new entry point needs its prototype in the header and its
signature string here; tests/test_abi.py derives the strings from the header and requires the two equal.

There is NO fallback: if the HIP library is missing or a call fails this module raises.  The
CPU restatements under ``oracle/`` are test infrastructure and are never imported from here.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libmisplat.so")

MISPLAT_TILE = 16
MISPLAT_REC = 16

_ERR = {-1: "MISPLAT_EINVAL (bad size / unsupported option)",
        -2: "MISPLAT_ELAUNCH (kernel launch failed)",
        -3: "MISPLAT_EWORKSPACE (scratch buffer too small)"}


class MisplatError(RuntimeError):
    pass


class Params(C.Structure):
    """Mirror of ``misplat_params`` (include/misplat.h)."""
    _fields_ = [("n_gauss", C.c_int32), ("n_cams", C.c_int32), ("width", C.c_int32),
                ("height", C.c_int32), ("tile_size", C.c_int32), ("tile_w", C.c_int32),
                ("tile_h", C.c_int32), ("antialiased", C.c_int32),
                ("opacity_aware_radius", C.c_int32), ("eps2d", C.c_float), ("near_plane", C.c_float),
                ("far_plane", C.c_float), ("radius_clip", C.c_float), ("radius_sigma", C.c_float),
                ("alpha_max", C.c_float), ("alpha_min", C.c_float), ("t_stop", C.c_float),
                ("median_t", C.c_float), ("jacobian_margin", C.c_float), ("plane_eps", C.c_float),
                ("ed_slot", C.c_int32), ("reserved_q", C.c_int32),
                ("unit_perm", C.c_void_p), ("unit_work", C.c_void_p), ("touched", C.c_void_p),
                ("activations", C.c_int32), ("unit_stride", C.c_int32), ("unit_sel", C.c_void_p),
                ("unit_slots", C.c_int32), ("front_pass", C.c_int32), ("front_n", C.c_void_p), ("tile_flag", C.c_void_p),
                ("unit_reach", C.c_void_p), ("front_depths", C.c_void_p)]


class RasterArgs(C.Structure):
    """Mirror of ``misplat_raster_args`` (include/misplat.h)."""
    _P = C.c_void_p
    _fields_ = ([(n, C.c_void_p) for n in ("means", "quats", "scales", "opacities", "colors", "colors_rest", "viewmats", "Ks")]
                + [(n, C.c_int32) for n in ("sh_degree", "K_or_D", "n_color", "per_cam", "depth_channel", "color_dim",
                                            "reserved_c", "lazy_colour")]
                + [(n, C.c_void_p) for n in ("radii", "means2d", "depths", "compensations", "grec", "sh_aux", "v_grec_zero",
                                             "tiles_per_gauss", "rect2", "cellhist", "cell_count", "cell_offs", "cell_cursor", "order",
                                             "rect_sorted", "counters", "tile_count", "offsets", "payload", "flatten_ids", "scratch")]
                + [("cap_isects", C.c_int64)]
                + [(n, C.c_void_p) for n in ("n_isects_host", "v_abs_zero", "render", "alpha", "exp_depth", "med_depth",
                                             "normal", "last_ids", "median_ids", "unit_perm_in", "unit_work",
                                             "unit_perm_out", "ev_blend_begin", "ev_blend_end", "order_table", "order_sel")]
                + [("order_slots", C.c_int32), ("order_stride", C.c_int32)]
                + [(n, C.c_void_p) for n in ("unit_reach", "front_n", "tile_flag")]
                + [("front_margin", C.c_float), ("front_min_bucket", C.c_int32), ("depth_sorted", C.c_void_p)]
                + [(n, C.c_void_p) for n in ("features", "featx", "v_featx_zero")] + [("n_feat", C.c_int32), ("nxq", C.c_int32)]
                + [("est_isects", C.c_int64)])


class RasterBwdArgs(C.Structure):
    """Mirror of ``misplat_raster_bwd_args`` (include/misplat.h)."""
    _fields_ = ([(n, C.c_void_p) for n in ("Ks", "grec", "flatten_ids", "offsets")] + [("n_isects", C.c_int64)]
                + [(n, C.c_void_p) for n in ("alpha", "last_ids", "median_ids", "render", "v_render", "v_alpha", "v_exp_depth",
                                             "v_med_depth", "v_normal", "v_grec", "v_abs", "unit_perm")]
                + [(n, C.c_int32) for n in ("color_dim", "zero_flags", "sh_degree", "K_or_D", "n_color", "per_cam",
                                            "depth_slot", "reserved")]
                + [(n, C.c_void_p) for n in ("means", "quats", "scales", "opacities", "colors", "colors_rest", "viewmats",
                                             "radii", "compensations", "sh_aux", "v_means2d", "v_colors", "v_colors_rest",
                                             "v_means_dir", "v_means", "v_quats", "v_scales", "v_opacities", "ev_blend_begin", "ev_blend_end",
                                             "v_means2d_out", "unit_sel")]
                + [("unit_stride", C.c_int32), ("unit_slots", C.c_int32)]
                + [(n, C.c_void_p) for n in ("featx", "features", "v_featx", "v_features")]
                + [(n, C.c_int32) for n in ("n_feat", "nxq", "depth_channel", "reserved_x")] + [("depths", C.c_void_p)])


def make_params(n_gauss: int, n_cams: int, width: int, height: int, tile_size: int = 16,
                antialiased: bool = False, opacity_aware_radius: bool = True, eps2d: float = 0.3,
                near_plane: float = 0.01, far_plane: float = 1e10, radius_clip: float = 0.0,
                radius_sigma: float = 3.33, alpha_max: float = 0.999, alpha_min: float = 1.0 / 255.0,
                t_stop: float = 1e-4, median_t: float = 0.5, jacobian_margin: float = 0.3,
                plane_eps: float = 1e-6, ed_slot: int = -1) -> Params:
    if tile_size != MISPLAT_TILE:
        raise ValueError(f"tile_size must be {MISPLAT_TILE} (got {tile_size})")
    tw = (width + tile_size - 1) // tile_size
    th = (height + tile_size - 1) // tile_size
    return Params(n_gauss, n_cams, width, height, tile_size, tw, th, int(antialiased),
                  int(opacity_aware_radius), eps2d, near_plane, far_plane, radius_clip, radius_sigma,
                  alpha_max, alpha_min, t_stop, median_t, jacobian_margin, plane_eps,
                  int(ed_slot), 0, None, None, None)


# The signature of every symbol include/misplat.h declares: one letter for the return, a space, one letter per argument.
#   arguments: p pointer, s misplat_stream_t, i int / int32_t, q int64_t, f float, d double, u uint32_t, Q size_t
#   returns:   i status, q int64_t, p pointer, v void, z const char*
# tests/test_abi.py derives the same strings from the header's prototypes and requires them equal.
_ARG = {"p": C.c_void_p, "s": C.c_void_p, "i": C.c_int32, "q": C.c_int64, "f": C.c_float, "d": C.c_double,
        "u": C.c_uint32, "Q": C.c_uint64}
_RET = {"i": C.c_int, "q": C.c_int64, "p": C.c_void_p, "v": None, "z": C.c_char_p}
SYMBOLS = {
    "misplat_project_fwd": "i ppppppppppppppps", "misplat_project_bwd": "i ppppppppppppppppps",
    "misplat_project_bwd_pose_workspace": "q ii", "misplat_project_bwd_pose": "i pppppppppppppppps",
    "misplat_project_pack_fwd": "i pppppppppppppipps", "misplat_color_fwd": "i piiiiippppppppps",
    "misplat_color_bwd": "i piiiipppppppppps", "misplat_project_pack_bwd": "i pippppppppppppppppis",
    "misplat_sh_fwd": "i iiiipppps", "misplat_sh_bwd": "i iiiipppppps", "misplat_isect_ids": "i pppqps",
    "misplat_tile_sort": "i piqpppppis", "misplat_adam_step": "i ipppppppddds", "misplat_pack": "i qipppppppps",
    "misplat_blend_fwd": "i pippppqppppppps", "misplat_blend_fwd_lazy": "i pippppqpppppppppppiipps",
    "misplat_blend_bwd": "i pipppppqpppppppppppps", "misplat_color_fwd_x": "i piiiippppps",
    "misplat_color_bwd_x": "i piiipppps", "misplat_blend_fwd_x": "i piipppppqppppppps",
    "misplat_blend_bwd_x_atomic": "i piipppppqpppppppppppps", "misplat_blend_planes": "i p",
    "misplat_blend_bwd_atomic": "i pippppqpppppppppppis", "misplat_slab_reduce": "i pqqppppppps",
    "misplat_depth_normal_fwd": "i iiffppppps", "misplat_depth_normal_bwd": "i iiffppppppppis",
    "misplat_outputs_fwd": "i qipppppppppppps", "misplat_outputs_bwd": "i qippppppppppppps",
    "misplat_loss_fwd": "i qppppffppps", "misplat_loss_bwd": "i qppppffppps", "misplat_ssim_scratch_floats": "q ii",
    "misplat_ssim_fwd": "i iippppfpps", "misplat_ssim_bwd": "i iippppfps",
    "misplat_featloss_scratch_floats": "q iiiiipi", "misplat_featloss_fwd": "i iiiipippiiipppppfppps",
    "misplat_featloss_bwd": "i iiiipiiipppppfppppppps", "misplat_feature_decode": "i iiiipippiiippppips",
    "misplat_textquery_fold": "i iiippppps", "misplat_textquery_map": "i iiiipippiippifiips",
    "misplat_textquery_rows": "i qiipippiippifps", "misplat_textquery_upsample": "i iipiips",
    "misplat_bucket_plan": "i ppp", "misplat_bucket_count": "i ppppppppis", "misplat_bucket_rows": "i ppppppppppppis",
    "misplat_bucket_tiles": "i pppppppqpps", "misplat_unit_order": "i ppps", "misplat_raster_fwd": "i ppisp",
    "misplat_raster_bwd": "i ppsp", "misplat_raster_bwd_plan": "i pp", "misplat_graph_cache_create": "p i",
    "misplat_graph_cache_destroy": "v p", "misplat_graph_cache_stats": "i ppp", "misplat_wait_count": "q pq",
    "misplat_zero_bytes": "i pQs", "misplat_stream_copy": "i ppqis", "misplat_touched_bits": "i pqps",
    "misplat_union_count": "i piqps", "misplat_union_scan": "i pqpps", "misplat_union_ids": "i piqppqs",
    "misplat_rows_pack": "i ipppqpps", "misplat_rows_unpack": "i ipppqpps",
    "misplat_adam_step_rows": "i ipppppqppdddpqps", "misplat_visible_rows": "i piqps",
    "misplat_debug_memset_replay": "i ppips", "misplat_tsdf_mark": "i pppiiippps", "misplat_tsdf_alloc": "i ppppps",
    "misplat_tsdf_integrate": "i ppippppiiippps", "misplat_unit_lists": "i ppppqipqppps",
    "misplat_tsdf_order": "i pppps", "misplat_tsdf_mc_count": "i pppipppppps",
    "misplat_tsdf_mc_emit": "i pppipppppppps", "misplat_meshmap_workspace": "q qqii",
    "misplat_meshmap_knn": "i pqpqifpqppps", "misplat_meshmap_aggregate": "i qqippppiipqps",
    "misplat_cluster_workspace": "q q", "misplat_cluster_radius": "i pqpfipqppps",
    "misplat_pointcloud_workspace": "q qi", "misplat_pointcloud_cells": "i pqfpqps",
    "misplat_pointcloud_knn": "i pqpqifipqpps", "misplat_pointcloud_radius_count": "i pqpqfpqps",
    "misplat_pointcloud_outlier_mask": "i pqdpqps", "misplat_pointcloud_voxel_group": "i pqddddpqppps",
    "misplat_pointcloud_voxel_mean": "i pqippqps", "misplat_meshclean_workspace": "q qqi",
    "misplat_meshclean_edge_stats": "i pqpqpqpps", "misplat_meshclean_components": "i pqqpqppps",
    "misplat_meshclean_holes": "i pqpqpqpppps", "misplat_meshclean_segment_sum": "i pppqps",
    "misplat_meshclean_smooth": "i pqpqpiidpqpppps", "misplat_meshclean_plane_build": "i pqpuipps",
    "misplat_meshclean_plane_count": "i pqpifips", "misplat_meshclean_plane_moments": "i pqpfpqpps",
    "misplat_decimate_workspace": "q qq", "misplat_decimate_round": "i pqpqpqpipqps",
    "misplat_decimate_apply": "i pqpqpqpippqqpqs", "misplat_decimate_resolve": "i pqps",
    "misplat_meshfill_workspace": "q qq", "misplat_meshfill_round": "i pqpqpfpqps",
    "misplat_meshfill_apply": "i pqpqpppiqqpqps", "misplat_meshfill_fair_workspace": "q qqqq",
    "misplat_meshfill_fair_count": "i pqpqpqps", "misplat_meshfill_fair_build": "i pqpqqqpqpps",
    "misplat_meshfill_fair_step": "i ppqqiqqiifipqpps", "misplat_meshfill_fair_lds": "i pqqqqifipqpps",
    "misplat_meshfill_fair_finish": "i qipps", "misplat_meshfill_curv_patches": "i ppqpqpps",
    "misplat_meshfill_curv_workspace": "q qq", "misplat_meshfill_curv_solve": "i ppqpppppppqqqpidipqppps",
    "misplat_meshtri_order": "i ppppqqpps", "misplat_meshtri_workspace": "q q",
    "misplat_meshtri_dp": "i pqpppqipqpqpqpqpps", "misplat_meshtri_rim_workspace": "q q",
    "misplat_meshtri_order_rim": "i ppppqqpqpqppps", "misplat_meshtri_angle_workspace": "q q",
    "misplat_meshtri_angle_dp": "i pqppppqipqpqpqpqppps", "misplat_meshtri_flip_workspace": "q qq",
    "misplat_meshtri_flip_round": "i pqpqpdpqps", "misplat_depthcloud_workspace": "q qqqi",
    "misplat_depthcloud_edges": "i piiifipqps", "misplat_depthcloud_candidates": "i ppppqps",
    "misplat_depthcloud_sample": "i ppiiiiuupqpppps", "misplat_depthcloud_backproject": "i pppppiiippqppps",
    "misplat_depthcloud_gaussian_filter": "i pqpppiiips", "misplat_poisson_workspace": "q iq",
    "misplat_poisson_splat": "i pppqiffffppps", "misplat_poisson_system": "i ppifpqppps",
    "misplat_poisson_cg_init": "i ppiipqpppps", "misplat_poisson_cg_iterate": "i piidipqppppps",
    "misplat_poisson_sample": "i piiffffpqps", "misplat_poisson_mean": "i pqpqps",
    "misplat_poisson_mc_pool": "i pifps", "misplat_grouping_workspace": "q q",
    "misplat_grouping_project": "i ppqiipps", "misplat_grouping_mask_ids": "i pqpqpps",
    "misplat_grouping_front": "i pppqpiiiidpqpps", "misplat_grouping_relabel": "i pqpqpps",
    "misplat_grouping_overlap": "i pqppiips", "misplat_grouping_assign": "i ppiifpps",
    "misplat_grouping_merge_count": "i pqpipppqps", "misplat_grouping_merge_copy": "i pqpipppqppis",
    "misplat_grouping_members": "i ppqips", "misplat_bilagrid_scratch_floats": "q iiiii",
    "misplat_bilagrid_slice_fwd": "i iippiiips", "misplat_bilagrid_slice_bwd": "i iippiiiiipppps",
    "misplat_bilagrid_tv_fwd": "i piiiipps", "misplat_bilagrid_tv_bwd": "i piiiipps",
    "misplat_density_workspace": "q qq", "misplat_density_records": "i ppppqffps",
    "misplat_density_count": "i pppppqffpqpps", "misplat_density_emit": "i pppppqffpqppps",
    "misplat_density_accumulate": "i ppipppfips", "misplat_density_query": "i pppppfpqpipppps",
    "misplat_density_raycast": "i pppppfppppqffffipps", "misplat_ptsdf_workspace": "q qq",
    "misplat_ptsdf_count": "i pppiqipqpps", "misplat_ptsdf_emit": "i pppiqipqppps",
    "misplat_ptsdf_accumulate": "i ppippipippqpqpppps", "misplat_ptsdf_finalize": "i ippppips",
    "misplat_identity_scratch_floats": "q qiii", "misplat_identity_loss_fwd": "i iiiipipppppps",
    "misplat_identity_loss_bwd": "i iiiipippppppppps", "misplat_identity_labels": "i qiipipppps",
    "misplat_identity_3d_fwd": "i qipippiippppps", "misplat_identity_3d_bwd": "i qipippiipppppppppps",
    "misplat_eval_image_scratch_floats": "q iii", "misplat_eval_image": "i iiippipps",
    "misplat_eval_pixels_scratch_floats": "q iii", "misplat_eval_normals": "i iiipppiippps",
    "misplat_eval_depth": "i iiipppfpps", "misplat_colorcorrect_scratch_floats": "q iii",
    "misplat_colorcorrect": "i iiippifpppps", "misplat_mcmc_noise": "i qppppfuus",
    "misplat_mcmc_sample_workspace_bytes": "q q", "misplat_mcmc_sample": "i qpifquupqppps",
    "misplat_mcmc_relocation": "i qppppipps", "misplat_version": "z",
}

_lib: Optional[C.CDLL] = None


def load() -> C.CDLL:
    """Load libmisplat.so; raises MisplatError if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    path = os.environ.get("MISPLAT_LIB", LIB_PATH)      # developer knob: an alternative build of the same ABI
    if not os.path.exists(path):
        raise MisplatError(
            f"{path} not found: build it with `python -m collab_splats_amd.build` "
            "(hipcc --offload-arch=gfx950).  There is no CPU fallback.")
    lib = C.CDLL(path)
    for name, sig in SYMBOLS.items():
        fn = getattr(lib, name)
        fn.restype = _RET[sig[0]]
        fn.argtypes = [_ARG[k] for k in sig[2:]]
        setattr(lib, name, _counted(name, fn, len(fn.argtypes)))
    _lib = lib
    return lib


def _counted(name: str, fn, n_args: int):
    """``argtypes`` converts every argument to the C type of the signature, but a cdecl call with one argument too many
    passes ctypes unnoticed: every entry point is called through this check of the count."""
    def call(*args):
        if len(args) != n_args:
            raise MisplatError(f"{name}: {len(args)} arguments passed, the C ABI takes {n_args}")
        return fn(*args)
    call.__name__ = name
    return call


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)
_raw_device = getattr(torch._C, "_cuda_getDevice", None)


def stream_ptr() -> C.c_void_p:
    """The current HIP stream of the current device (what every entry point launches on).  Uses torch's raw
    accessors when present: the public ``torch.cuda.current_stream()`` costs ~10 us per call, 11 calls a step."""
    if _raw_stream is not None and _raw_device is not None:
        return C.c_void_p(_raw_stream(_raw_device()))
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def ptr(t: Optional[torch.Tensor]) -> C.c_void_p:
    if t is None:
        return C.c_void_p(0)
    assert t.is_contiguous(), "misplat: tensor must be contiguous"
    return C.c_void_p(t.data_ptr())


def check(code: int, what: str) -> None:
    if code != 0:
        raise MisplatError(f"{what} failed: {_ERR.get(code, code)}")


def run(name: str, *args) -> None:
    """Call the entry point ``name``, which returns a status, and raise unless that is 0.  The current stream is appended
    where the signature ends in one.  The entry is looked up on every call: a test that patches it is honoured."""
    if SYMBOLS[name][-1] == "s":
        args += (stream_ptr(),)
    check(getattr(load(), name)(*args), name)


def require_gpu(*tensors: torch.Tensor) -> None:
    cur = None
    for t in tensors:
        if t is None:
            continue
        if not t.is_cuda:
            raise MisplatError("misplat runs on the MI355X only: got a CPU tensor "
                               "(there is no CPU fallback; oracle/ is test infrastructure)")
        if cur is None:
            cur = _raw_device() if _raw_device is not None else torch.cuda.current_device()
        if t.device.index is not None and t.device.index != cur:
            # kernels are launched on the current device's current stream: a tensor of another GPU would be
            # dereferenced on the wrong device (one process per GPU is the supported layout)
            raise MisplatError(f"tensor on cuda:{t.device.index} but the current device is cuda:{cur}: "
                               "call torch.cuda.set_device() (one process per GPU) first")
