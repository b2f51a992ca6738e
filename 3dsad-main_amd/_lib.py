"""ctypes binding of ``csrc/libsad_amd.so`` (C-ABI declared in ``include/sad_amd.h``).

No reference FFI exists to mirror (``/root/reference/README.md:1-2`` is the whole upstream
repository); the entry points are the ones BASELINE.json ``north_star`` names.  Loading fails loudly
when the library is missing — there is no CPU fallback anywhere in this package.
"""
import ctypes
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, "csrc")
# SAD_AMD_LIB points at an alternative build of the same C-ABI (A/B measurements of kernel variants)
SO_PATH = os.environ.get("SAD_AMD_LIB") or os.path.join(CSRC, "libsad_amd.so")

MAX_LAYERS = 4
MAX_RADII = 4
ABI_VERSION = 4            # SAD_ABI_VERSION of include/sad_amd.h this binding was written against
# instrumentation ints of a row-packing table (include/sad_amd.h, SAD_WS_*)
WS_REFILLS, WS_INUSE, WS_CONFLICT = 5, 6, 7

c_f32p = ctypes.POINTER(ctypes.c_float)
c_i32p = ctypes.POINTER(ctypes.c_int32)
vp = ctypes.c_void_p
c_i3p = ctypes.POINTER(ctypes.c_int)      # a host array of 3 ints (z,y,x): shapes, kernel sizes, strides, paddings


class MlpArgs(ctypes.Structure):
    """``struct sad_mlp_args`` (include/sad_amd.h)."""
    _fields_ = [
        ("struct_size", ctypes.c_size_t),
        ("xyz", vp), ("new_xyz", vp), ("idx", vp), ("cnt", vp), ("workspace", vp), ("feat", vp),
        ("ld_feat", ctypes.c_int),
        ("B", ctypes.c_int), ("N", ctypes.c_int), ("M", ctypes.c_int), ("S", ctypes.c_int),
        ("C", ctypes.c_int),
        ("L", ctypes.c_int), ("dims", ctypes.c_int * (MAX_LAYERS + 1)),
        ("packed", vp), ("relu_mask", ctypes.c_int),
        ("out", vp), ("ld_out", ctypes.c_int), ("col_off", ctypes.c_int),
        ("geometry", ctypes.c_int),
        ("scratch", vp), ("scratch_bytes", ctypes.c_size_t),
        ("prescanned", ctypes.c_int),
        ("c_out", ctypes.c_int),           # ABI 3: != 0 = a chain packed zero-padded onto wider dims (in the ABI-2 struct's tail padding)
    ]


class MlpBf16Args(ctypes.Structure):
    """``struct sad_mlp_bf16_args`` (include/sad_amd.h)."""
    _fields_ = [
        ("struct_size", ctypes.c_size_t),
        ("xyz", vp), ("new_xyz", vp), ("idx", vp), ("feat", vp),
        ("feat_bf16", ctypes.c_int), ("ld_feat", ctypes.c_int),
        ("B", ctypes.c_int), ("N", ctypes.c_int), ("M", ctypes.c_int), ("S", ctypes.c_int),
        ("C", ctypes.c_int),
        ("L", ctypes.c_int), ("dims", ctypes.c_int * (MAX_LAYERS + 1)),
        ("packed", vp), ("relu_mask", ctypes.c_int),
        ("out", vp), ("out_bf16", ctypes.c_int), ("ld_out", ctypes.c_int), ("col_off", ctypes.c_int),
        ("cnt", vp), ("workspace", vp), ("geometry", ctypes.c_int), ("prescanned", ctypes.c_int),
        # ABI 4, split pooling: continuation rows of a grouped chain / the pooled chains behind a plain layer's input rows
        ("cont", vp), ("n_pool", ctypes.c_int),
        ("pool_ws", vp * MAX_RADII), ("pool_cont", vp * MAX_RADII),
        ("pool_S", ctypes.c_int * MAX_RADII), ("pool_cols", ctypes.c_int * MAX_RADII),
    ]


LAYOUTS = {"nchw": 0, "nhwc": 1}      # SAD_LAYOUT_*


class AnchorDecodeArgs(ctypes.Structure):
    """``struct sad_anchor_decode_args`` (include/sad_amd.h)."""
    _fields_ = [
        ("struct_size", ctypes.c_size_t),
        ("cls", vp), ("reg", vp), ("dir", vp), ("index", vp),
        ("B", ctypes.c_int), ("H", ctypes.c_int), ("W", ctypes.c_int), ("C", ctypes.c_int), ("nb", ctypes.c_int),
        ("ns", ctypes.c_int), ("nr", ctypes.c_int), ("layout", ctypes.c_int), ("P", ctypes.c_int),
        ("sizes", ctypes.c_float * 48), ("z_center", ctypes.c_float * 16), ("rotations", ctypes.c_float * 8),
        ("x0", ctypes.c_float), ("y0", ctypes.c_float), ("sx", ctypes.c_float), ("sy", ctypes.c_float),
        ("dir_offset", ctypes.c_float), ("dir_limit_offset", ctypes.c_float),
        ("boxes", vp), ("scores", vp), ("labels", vp),
    ]


class CenterDecodeArgs(ctypes.Structure):
    """``struct sad_center_decode_args`` (include/sad_amd.h)."""
    _fields_ = [
        ("struct_size", ctypes.c_size_t),
        ("hm", vp), ("reg", vp), ("height", vp), ("dim", vp), ("rot", vp), ("vel", vp), ("index", vp),
        ("B", ctypes.c_int), ("H", ctypes.c_int), ("W", ctypes.c_int), ("C", ctypes.c_int), ("layout", ctypes.c_int),
        ("P", ctypes.c_int), ("log_dim", ctypes.c_int), ("peak", ctypes.c_int),
        ("lo_x", ctypes.c_float), ("lo_y", ctypes.c_float), ("sx", ctypes.c_float), ("sy", ctypes.c_float),
        ("boxes", vp), ("scores", vp), ("labels", vp),
    ]


class AnchorTargetsArgs(ctypes.Structure):
    """``struct sad_anchor_targets_args`` (include/sad_amd.h)."""
    _fields_ = [
        ("struct_size", ctypes.c_size_t),
        ("gt_boxes", vp), ("gt_labels", vp),
        ("B", ctypes.c_int), ("G", ctypes.c_int), ("D", ctypes.c_int), ("H", ctypes.c_int), ("W", ctypes.c_int),
        ("ns", ctypes.c_int), ("nr", ctypes.c_int), ("nb", ctypes.c_int), ("use_size_class", ctypes.c_int),
        ("sizes", ctypes.c_float * 48), ("z_center", ctypes.c_float * 16), ("rotations", ctypes.c_float * 8),
        ("pos_thr", ctypes.c_float * 16), ("neg_thr", ctypes.c_float * 16), ("size_class", ctypes.c_int32 * 16),
        ("x0", ctypes.c_float), ("y0", ctypes.c_float), ("sx", ctypes.c_float), ("sy", ctypes.c_float),
        ("dir_offset", ctypes.c_float),
        ("labels", vp), ("match", vp), ("reg_target", vp), ("max_iou", vp), ("dir_target", vp), ("workspace", vp),
    ]


class CenterTargetsArgs(ctypes.Structure):
    """``struct sad_center_targets_args`` (include/sad_amd.h)."""
    _fields_ = [
        ("struct_size", ctypes.c_size_t),
        ("gt_boxes", vp), ("gt_labels", vp),
        ("B", ctypes.c_int), ("G", ctypes.c_int), ("D", ctypes.c_int), ("C", ctypes.c_int), ("H", ctypes.c_int),
        ("W", ctypes.c_int), ("layout", ctypes.c_int), ("min_radius", ctypes.c_int), ("vel", ctypes.c_int),
        ("lo_x", ctypes.c_float), ("lo_y", ctypes.c_float), ("sx", ctypes.c_float), ("sy", ctypes.c_float),
        ("min_overlap", ctypes.c_float),
        ("heatmap", vp), ("ind", vp), ("anno", vp),
    ]


class AnchorHeadLossArgs(ctypes.Structure):
    """``struct sad_anchor_head_loss_args`` (include/sad_amd.h)."""
    _fields_ = [
        ("struct_size", ctypes.c_size_t),
        ("cls", vp), ("reg", vp), ("dir", vp), ("labels", vp), ("reg_target", vp), ("dir_target", vp),
        ("B", ctypes.c_int), ("H", ctypes.c_int), ("W", ctypes.c_int), ("A", ctypes.c_int), ("C", ctypes.c_int),
        ("nb", ctypes.c_int), ("layout", ctypes.c_int), ("sin_diff", ctypes.c_int), ("normalize", ctypes.c_int),
        ("alpha", ctypes.c_float), ("beta", ctypes.c_float),
        ("code_weights", ctypes.c_float * 7), ("scale", ctypes.c_float * 3),
        ("loss", vp), ("num_pos", vp), ("grad_cls", vp), ("grad_reg", vp), ("grad_dir", vp), ("per_anchor", vp),
        ("workspace", vp),
    ]


class CenterHeadLossArgs(ctypes.Structure):
    """``struct sad_center_head_loss_args`` (include/sad_amd.h)."""
    _fields_ = [
        ("struct_size", ctypes.c_size_t),
        ("hm", vp), ("reg", vp), ("height", vp), ("dim", vp), ("rot", vp), ("vel", vp),
        ("heatmap", vp), ("ind", vp), ("anno", vp),
        ("B", ctypes.c_int), ("H", ctypes.c_int), ("W", ctypes.c_int), ("C", ctypes.c_int), ("G", ctypes.c_int),
        ("layout", ctypes.c_int), ("normalize", ctypes.c_int),
        ("code_weights", ctypes.c_float * 10), ("scale", ctypes.c_float * 2),
        ("loss", vp), ("num_pos", vp),
        ("grad_hm", vp), ("grad_reg", vp), ("grad_height", vp), ("grad_dim", vp), ("grad_rot", vp), ("grad_vel", vp),
        ("workspace", vp),
    ]


ROI_CLS_MODES = {"roi_iou": 0, "cls": 1}      # SAD_ROI_CLS_*


class RoiTargetsArgs(ctypes.Structure):
    """``struct sad_roi_targets_args`` (include/sad_amd.h)."""
    _fields_ = [
        ("struct_size", ctypes.c_size_t),
        ("rois", vp), ("roi_count", vp), ("roi_labels", vp), ("gt_boxes", vp), ("gt_labels", vp),
        ("B", ctypes.c_int), ("R", ctypes.c_int), ("D", ctypes.c_int), ("G", ctypes.c_int), ("Dg", ctypes.c_int),
        ("S", ctypes.c_int), ("fg_max", ctypes.c_int), ("cls_mode", ctypes.c_int), ("seed", ctypes.c_uint),
        ("fg_thr", ctypes.c_float), ("bg_lo", ctypes.c_float), ("hard_ratio", ctypes.c_float), ("reg_fg_thr", ctypes.c_float),
        ("cls_fg_thr", ctypes.c_float), ("cls_bg_thr", ctypes.c_float),
        ("index", vp), ("match", vp), ("labels", vp), ("iou", vp), ("cls_target", vp), ("reg_valid", vp),
        ("rois_s", vp), ("gt_local", vp), ("reg_target", vp), ("workspace", vp),
    ]


class RoiHeadLossArgs(ctypes.Structure):
    """``struct sad_roi_head_loss_args`` (include/sad_amd.h)."""
    _fields_ = [
        ("struct_size", ctypes.c_size_t),
        ("rcnn_cls", vp), ("rcnn_reg", vp), ("cls_target", vp), ("reg_valid", vp), ("reg_target", vp), ("rois", vp), ("gt_local", vp),
        ("B", ctypes.c_int), ("S", ctypes.c_int), ("D", ctypes.c_int), ("normalize", ctypes.c_int),
        ("beta", ctypes.c_float), ("code_weights", ctypes.c_float * 7), ("scale", ctypes.c_float * 3),
        ("loss", vp), ("num", vp), ("grad_cls", vp), ("grad_reg", vp), ("grad_corner", vp), ("per_roi", vp),
    ]


class RoiGridPointsArgs(ctypes.Structure):
    """``struct sad_roi_grid_points_args`` (include/sad_amd.h)."""
    _fields_ = [
        ("struct_size", ctypes.c_size_t),
        ("rois", vp), ("roi_count", vp),
        ("B", ctypes.c_int), ("R", ctypes.c_int), ("D", ctypes.c_int), ("G", ctypes.c_int),
        ("pts", vp),
    ]


class VoxelQueryArgs(ctypes.Structure):
    """``struct sad_voxel_query_args`` (include/sad_amd.h)."""
    _fields_ = [
        ("struct_size", ctypes.c_size_t),
        ("coors", vp), ("offsets", vp), ("new_xyz", vp),
        ("Nv", ctypes.c_int), ("B", ctypes.c_int), ("M", ctypes.c_int), ("S", ctypes.c_int),
        ("spatial_shape", ctypes.c_int * 3), ("max_range", ctypes.c_int * 3),
        ("voxel_size", ctypes.c_float * 3), ("lo", ctypes.c_float * 3), ("radius", ctypes.c_float),
        ("idx", vp), ("cnt", vp), ("workspace", vp),
    ]


POINT_CLS_LOSSES = {"bce": 0, "focal": 1}      # SAD_POINT_CLS_*


class PointTargetsArgs(ctypes.Structure):
    """``struct sad_point_targets_args`` (include/sad_amd.h)."""
    _fields_ = [
        ("struct_size", ctypes.c_size_t),
        ("xyz", vp), ("cand", vp), ("gt_boxes", vp), ("gt_labels", vp),
        ("B", ctypes.c_int), ("M", ctypes.c_int), ("G", ctypes.c_int), ("D", ctypes.c_int), ("C", ctypes.c_int),
        ("anchors", ctypes.c_float * 48), ("size_anchor", ctypes.c_float * 3),
        ("shift_max", ctypes.c_float), ("extra_width", ctypes.c_float),
        ("labels", vp), ("match", vp), ("centerness", vp), ("shift_target", vp), ("size_target", vp), ("reg_target", vp),
    ]


class PointHeadLossArgs(ctypes.Structure):
    """``struct sad_point_head_loss_args`` (include/sad_amd.h)."""
    _fields_ = [
        ("struct_size", ctypes.c_size_t),
        ("o", vp), ("c", vp), ("labels", vp), ("centerness", vp), ("reg_target", vp), ("shift_target", vp), ("size_target", vp),
        ("B", ctypes.c_int), ("M", ctypes.c_int), ("C", ctypes.c_int), ("cls_loss", ctypes.c_int), ("normalize", ctypes.c_int),
        ("alpha", ctypes.c_float), ("beta", ctypes.c_float), ("shift_max", ctypes.c_float),
        ("code_weights", ctypes.c_float * 7), ("scale", ctypes.c_float * 4),
        ("loss", vp), ("num_pos", vp), ("grad_o", vp), ("grad_c", vp), ("per_point", vp), ("workspace", vp),
    ]


IOU_MODES = {"bev": 0, "3d": 1}               # SAD_IOU_BEV, SAD_IOU_3D
IOU_LOSS_KINDS = {"iou": 0, "diou": 1}        # SAD_IOU_LOSS_*
IOU_CODES = {"box": 0, "roi": 1}              # SAD_IOU_CODE_*


class RotatedIouLossArgs(ctypes.Structure):
    """``struct sad_rotated_iou_loss_args`` (include/sad_amd.h)."""
    _fields_ = [
        ("struct_size", ctypes.c_size_t),
        ("pred", vp), ("target", vp), ("weight", vp), ("rois", vp),
        ("N", ctypes.c_int), ("Dp", ctypes.c_int), ("Dt", ctypes.c_int), ("Dr", ctypes.c_int),
        ("mode", ctypes.c_int), ("kind", ctypes.c_int), ("code", ctypes.c_int), ("need_grad", ctypes.c_int),
        ("loss", vp), ("iou", vp), ("grad", vp), ("decoded", vp),
    ]


class GlobalAugmentArgs(ctypes.Structure):
    """``struct sad_global_augment_args`` (include/sad_amd.h)."""
    _fields_ = [
        ("struct_size", ctypes.c_size_t),
        ("points", vp), ("offsets", vp), ("gt_boxes", vp),
        ("B", ctypes.c_int), ("N", ctypes.c_int), ("total", ctypes.c_int), ("Cp", ctypes.c_int), ("G", ctypes.c_int), ("D", ctypes.c_int),
        ("seed", ctypes.c_uint),
        ("flip_x", ctypes.c_int), ("flip_y", ctypes.c_int), ("with_velocity", ctypes.c_int),
        ("rot_lo", ctypes.c_float), ("rot_hi", ctypes.c_float), ("scale_lo", ctypes.c_float), ("scale_hi", ctypes.c_float),
        ("translate", ctypes.c_float * 3),
        ("points_out", vp), ("boxes_out", vp), ("params", vp),
    ]


PASTE_MAX_CLASSES = 16                         # SAD_PASTE_MAX_CLASSES


class GtPasteArgs(ctypes.Structure):
    """``struct sad_gt_paste_args`` (include/sad_amd.h)."""
    _fields_ = [
        ("struct_size", ctypes.c_size_t),
        ("points", vp), ("offsets", vp), ("gt_boxes", vp), ("gt_labels", vp),
        ("db_points", vp), ("db_offsets", vp), ("db_boxes", vp), ("params", vp),
        ("B", ctypes.c_int), ("total", ctypes.c_int), ("Cp", ctypes.c_int), ("G", ctypes.c_int), ("D", ctypes.c_int), ("C", ctypes.c_int),
        ("Ndb", ctypes.c_int), ("max_obj_points", ctypes.c_int), ("with_velocity", ctypes.c_int),
        ("class_offsets", ctypes.c_int * (PASTE_MAX_CLASSES + 1)), ("sample_num", ctypes.c_int * PASTE_MAX_CLASSES),
        ("seed", ctypes.c_uint), ("remove_extra_width", ctypes.c_float),
        ("R", ctypes.c_longlong),
        ("keep", vp), ("db_index", vp), ("boxes_out", vp), ("labels_out", vp), ("num_pasted", vp), ("out_points", vp),
        ("out_offsets", vp), ("workspace", vp),
    ]


DET_METRICS = {"iou_bev": 0, "iou3d": 1, "dist": 2}      # SAD_DET_*


class DetMatchArgs(ctypes.Structure):
    """``struct sad_det_match_args`` (include/sad_amd.h)."""
    _fields_ = [
        ("struct_size", ctypes.c_size_t),
        ("det_boxes", vp), ("det_scores", vp), ("det_labels", vp), ("det_count", vp),
        ("gt_boxes", vp), ("gt_labels", vp), ("gt_ignore", vp), ("thr", vp),
        ("B", ctypes.c_int), ("K", ctypes.c_int), ("D", ctypes.c_int), ("G", ctypes.c_int), ("Dg", ctypes.c_int),
        ("C", ctypes.c_int), ("T", ctypes.c_int), ("metric", ctypes.c_int),
        ("code", vp), ("match", vp), ("value", vp), ("gt_det", vp), ("n_gt", vp),
    ]


class DetApArgs(ctypes.Structure):
    """``struct sad_det_ap_args`` (include/sad_amd.h)."""
    _fields_ = [
        ("struct_size", ctypes.c_size_t),
        ("keys", vp), ("perm", vp), ("code", vp), ("n_gt", vp),
        ("N", ctypes.c_longlong),
        ("C", ctypes.c_int), ("T", ctypes.c_int), ("points", ctypes.c_int), ("first", ctypes.c_int),
        ("floor", ctypes.c_float),
        ("ap", vp), ("prec", vp), ("max_recall", vp), ("n_det", vp),
    ]


GRAD_FEAT, GRAD_XYZ, GRAD_NEW_XYZ, GRAD_PARAMS = 1, 2, 4, 8      # SAD_GRAD_*


class MlpGradArgs(ctypes.Structure):
    """``struct sad_mlp_grad_args`` (include/sad_amd.h)."""
    _fields_ = [
        ("struct_size", ctypes.c_size_t),
        ("xyz", vp), ("new_xyz", vp), ("feat", vp), ("idx", vp), ("cnt", vp),
        ("ld_feat", ctypes.c_int),
        ("B", ctypes.c_int), ("N", ctypes.c_int), ("M", ctypes.c_int), ("S", ctypes.c_int), ("C", ctypes.c_int),
        ("L", ctypes.c_int), ("dims", ctypes.c_int * (MAX_LAYERS + 1)),
        ("W", vp * MAX_LAYERS), ("b", vp * MAX_LAYERS),
        ("relu_mask", ctypes.c_int), ("skip_empty", ctypes.c_int),
        ("pooled", vp), ("ld_pooled", ctypes.c_int), ("pooled_off", ctypes.c_int),
        ("grad_out", vp), ("ld_grad", ctypes.c_int), ("col_off", ctypes.c_int),
        ("need", ctypes.c_int),
        ("grad_feat", vp), ("grad_xyz", vp), ("grad_new_xyz", vp),
        ("grad_W", vp * MAX_LAYERS), ("grad_b", vp * MAX_LAYERS),
        ("workspace", vp), ("workspace_bytes", ctypes.c_size_t),
    ]


# name -> (restype, argtypes); every symbol include/sad_amd.h declares
SIGNATURES = {
    "sad_version": (ctypes.c_int, []),
    "sad_last_error": (ctypes.c_char_p, []),
    "sad_set_option": (ctypes.c_int, [ctypes.c_char_p, ctypes.c_int]),
    "sad_fps_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int, ctypes.c_int]),
    "sad_fps_f32": (ctypes.c_int, [vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, vp, vp, vp]),
    "sad_ffps_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int, ctypes.c_int]),
    "sad_pairdist_f32": (ctypes.c_int, [vp, vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                       ctypes.c_float, vp, vp]),
    "sad_ffps_f32": (ctypes.c_int, [vp, vp] + [ctypes.c_int] * 5 + [ctypes.c_float, vp, vp, vp]),
    "sad_gather_xyz_f32": (ctypes.c_int, [vp, vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, vp, vp]),
    "sad_gather_points": (ctypes.c_int, [vp, vp] + [ctypes.c_int] * 5 + [vp, vp]),
    "sad_group_points": (ctypes.c_int, [vp, vp] + [ctypes.c_int] * 6 + [vp, vp]),
    "sad_group_points_grad_f32": (ctypes.c_int, [vp, vp] + [ctypes.c_int] * 5 + [vp, vp]),
    "sad_group_points_grad_pm_f32": (ctypes.c_int, [vp, vp] + [ctypes.c_int] * 5 + [vp, vp]),
    "sad_max_pool_s_f32": (ctypes.c_int, [vp] + [ctypes.c_int] * 4 + [vp, vp, vp]),
    "sad_max_pool_s_grad_f32": (ctypes.c_int, [vp, vp] + [ctypes.c_int] * 4 + [vp, vp]),
    "sad_ball_query_f32": (ctypes.c_int, [vp, vp, ctypes.c_float, vp] + [ctypes.c_int] * 4 + [vp, vp]),
    "sad_ball_query_multi_f32": (ctypes.c_int, [vp, vp, ctypes.c_int, c_f32p, vp,
                                               ctypes.POINTER(ctypes.c_int), ctypes.POINTER(vp),
                                               ctypes.POINTER(vp),
                                               ctypes.c_int, ctypes.c_int, ctypes.c_int, vp]),
    "sad_ball_query_grid_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int, ctypes.c_int]),
    "sad_ball_query_grid_f32": (ctypes.c_int, [vp, vp, ctypes.c_int, c_f32p, ctypes.POINTER(ctypes.c_int),
                                              ctypes.POINTER(vp), ctypes.POINTER(vp),
                                              ctypes.c_int, ctypes.c_int, ctypes.c_int, vp, vp]),
    "sad_subsample_pad_f32": (ctypes.c_int, [vp, vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_uint, vp, vp]),
    "sad_copy_rows_u32": (ctypes.c_int, [vp, ctypes.c_longlong, vp, ctypes.c_longlong, ctypes.c_longlong, ctypes.c_longlong, vp]),
    "sad_knn_f32": (ctypes.c_int, [vp, vp] + [ctypes.c_int] * 4 + [vp, vp]),
    "sad_three_nn_f32": (ctypes.c_int, [vp, vp] + [ctypes.c_int] * 3 + [vp, vp, vp, vp]),
    "sad_three_interpolate_f32": (ctypes.c_int, [vp, vp, vp] + [ctypes.c_int] * 5 + [vp, ctypes.c_int, ctypes.c_int, vp]),
    "sad_three_interpolate_grad_f32": (ctypes.c_int, [vp, vp, vp] + [ctypes.c_int] * 5 + [vp, vp]),
    "sad_boxes_iou_f32": (ctypes.c_int, [vp, vp] + [ctypes.c_int] * 6 + [vp, vp]),
    "sad_points_in_boxes_f32": (ctypes.c_int, [vp, vp] + [ctypes.c_int] * 4 + [vp, vp]),
    "sad_roipoint_pool3d_f32": (ctypes.c_int, [vp, vp, vp] + [ctypes.c_int] * 5 + [ctypes.c_float, ctypes.c_int, vp, vp, vp, vp]),
    "sad_voxel_workspace_bytes": (ctypes.c_int, [ctypes.c_int] * 3 + [ctypes.POINTER(ctypes.c_size_t)]),
    "sad_voxel_coords_f32": (ctypes.c_int, [vp, vp] + [ctypes.c_int] * 3 + [c_f32p, c_f32p, vp, vp]),
    "sad_voxel_index_f32": (ctypes.c_int, [vp, vp] + [ctypes.c_int] * 3 + [c_f32p, c_f32p, ctypes.c_int, vp, vp, vp, vp, vp, vp]),
    "sad_voxelize_f32": (ctypes.c_int, [vp, vp] + [ctypes.c_int] * 3 + [c_f32p, c_f32p, ctypes.c_int, ctypes.c_int, vp, vp, vp, vp, vp, vp]),
    "sad_voxel_reduce_f32": (ctypes.c_int, [vp, vp, vp] + [ctypes.c_int] * 5 + [vp, vp, vp, vp, vp]),
    "sad_voxel_reduce_grad_f32": (ctypes.c_int, [vp, vp, vp] + [ctypes.c_int] * 5 + [vp, vp, vp]),
    "sad_voxel_encode_workspace_bytes": (ctypes.c_int, [ctypes.c_int] * 5 + [ctypes.POINTER(ctypes.c_size_t)]),
    "sad_voxel_decorate_f32": (ctypes.c_int, [vp] * 5 + [ctypes.c_int] * 5 + [c_f32p, c_f32p, ctypes.c_int, ctypes.c_int, vp, vp, vp]),
    "sad_voxel_encode_f32": (ctypes.c_int, [vp] * 5 + [ctypes.c_int] * 5 + [c_f32p, c_f32p, vp, vp] + [ctypes.c_int] * 3 + [vp] * 5),
    "sad_spconv_workspace_bytes": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, c_i3p, c_i3p, ctypes.c_int, ctypes.POINTER(ctypes.c_size_t)]),
    "sad_spconv_index_subm": (ctypes.c_int, [vp, vp, ctypes.c_int, ctypes.c_int, c_i3p, c_i3p, vp, vp, vp]),
    "sad_spconv_index_count": (ctypes.c_int, [vp, vp, ctypes.c_int, ctypes.c_int, c_i3p, c_i3p, c_i3p, c_i3p, vp, vp, vp]),
    "sad_spconv_index_fill": (ctypes.c_int, [vp, vp, ctypes.c_int, ctypes.c_int, c_i3p, c_i3p, c_i3p, c_i3p, vp, ctypes.c_int, vp, vp, vp, vp]),
    "sad_spconv_packed_floats": (ctypes.c_size_t, [ctypes.c_int] * 3),
    "sad_spconv_pack_f32": (ctypes.c_int, [vp, vp] + [ctypes.c_int] * 3 + [vp, vp]),
    "sad_spconv_f32": (ctypes.c_int, [vp, vp, vp, vp] + [ctypes.c_int] * 6 + [vp, vp]),
    "sad_sparse_to_dense_workspace_bytes": (ctypes.c_int, [ctypes.c_int, c_i3p, ctypes.POINTER(ctypes.c_size_t)]),
    "sad_sparse_to_dense_f32": (ctypes.c_int, [vp, vp, vp] + [ctypes.c_int] * 3 + [c_i3p, vp, vp, vp]),
    "sad_spconv_index_transpose": (ctypes.c_int, [vp] + [ctypes.c_int] * 3 + [vp, vp, vp]),
    "sad_spconv_grad_weight_workspace_bytes": (ctypes.c_int, [ctypes.c_int] * 4 + [ctypes.POINTER(ctypes.c_size_t)]),
    "sad_spconv_grad_weight_f32": (ctypes.c_int, [vp, vp, vp] + [ctypes.c_int] * 5 + [vp, vp, vp, vp]),
    "sad_spconv_max_pool_f32": (ctypes.c_int, [vp, vp] + [ctypes.c_int] * 4 + [vp, vp, vp]),
    "sad_spconv_max_pool_grad_f32": (ctypes.c_int, [vp, vp, vp] + [ctypes.c_int] * 4 + [vp, vp]),
    "sad_mlp_packed_floats": (ctypes.c_size_t, [ctypes.c_int, ctypes.POINTER(ctypes.c_int), ctypes.c_int]),
    "sad_mlp_pack_f32": (ctypes.c_int, [ctypes.c_int, ctypes.POINTER(ctypes.c_int), ctypes.c_int,
                                       ctypes.POINTER(vp), ctypes.POINTER(vp), vp, vp]),
    "sad_mlp_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    "sad_mlp_rowscan": (ctypes.c_int, [ctypes.c_int, ctypes.POINTER(vp), ctypes.POINTER(vp), ctypes.POINTER(ctypes.c_int),
                                       ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.POINTER(vp), vp]),
    "sad_mlp_rowscan_init": (ctypes.c_int, [ctypes.c_int, ctypes.POINTER(vp), ctypes.POINTER(vp), ctypes.POINTER(ctypes.c_int),
                                            ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.POINTER(vp), ctypes.POINTER(vp),
                                            ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int), vp]),
    "sad_mlp_rowscan_split": (ctypes.c_int, [ctypes.c_int, ctypes.POINTER(vp), ctypes.POINTER(vp), ctypes.POINTER(ctypes.c_int),
                                             ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.POINTER(vp), ctypes.POINTER(vp),
                                             ctypes.POINTER(ctypes.c_int), vp]),
    "sad_mlp_cont_bytes": (ctypes.c_size_t, [ctypes.c_int] * 4),
    "sad_mlp_preferred_geometry": (ctypes.c_int, [ctypes.c_int, ctypes.POINTER(ctypes.c_int)]),
    "sad_mlp_padded_dims": (ctypes.c_int, [ctypes.c_int, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]),
    "sad_mlp_scratch_bytes": (ctypes.c_size_t, [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                               ctypes.POINTER(ctypes.c_int)]),
    "sad_mlp_chain_f32": (ctypes.c_int, [ctypes.POINTER(MlpArgs), vp]),
    "sad_mlp_chain_multi_f32": (ctypes.c_int, [ctypes.POINTER(ctypes.POINTER(MlpArgs)), ctypes.c_int, vp]),
    "sad_mlp_packed_bytes_bf16": (ctypes.c_size_t, [ctypes.c_int, ctypes.POINTER(ctypes.c_int), ctypes.c_int]),
    "sad_mlp_pack_bf16": (ctypes.c_int, [ctypes.c_int, ctypes.POINTER(ctypes.c_int), ctypes.c_int,
                                        ctypes.POINTER(vp), ctypes.POINTER(vp), vp, vp]),
    "sad_mlp_preferred_geometry_bf16": (ctypes.c_int, [ctypes.c_int, ctypes.POINTER(ctypes.c_int)]),
    "sad_mlp_chain_bf16": (ctypes.c_int, [ctypes.POINTER(MlpBf16Args), vp]),
    "sad_mlp_chain_multi_bf16": (ctypes.c_int, [ctypes.POINTER(ctypes.POINTER(MlpBf16Args)), ctypes.c_int, vp]),
    "sad_candidates_f32": (ctypes.c_int, [vp, vp, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                         ctypes.c_float, ctypes.c_float, ctypes.c_float, c_f32p,
                                         vp, vp, vp]),
    "sad_candidates_grad_f32": (ctypes.c_int, [vp, vp, ctypes.c_int, ctypes.c_int, ctypes.c_float, vp, vp]),
    "sad_prefix_rows_grad_f32": (ctypes.c_int, [vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, vp, vp]),
    "sad_nms_bev_f32": (ctypes.c_int, [vp, ctypes.c_int, ctypes.c_int, ctypes.c_float, ctypes.c_float,
                                      vp, vp, vp, vp]),
    "sad_nms_bev_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int, ctypes.c_int]),
    "sad_nms_bev_ws_f32": (ctypes.c_int, [vp, ctypes.c_int, ctypes.c_int, ctypes.c_float, ctypes.c_float,
                                         vp, vp, vp, vp, vp]),
    "sad_nms_boxes_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int] * 3),
    "sad_nms_boxes_f32": (ctypes.c_int, [vp, ctypes.c_int, vp, vp, ctypes.c_int, ctypes.c_int, ctypes.c_float, ctypes.c_float,
                                        ctypes.c_int, ctypes.c_int, vp, vp, vp, vp, vp]),
    "sad_decode_boxes_f32": (ctypes.c_int, [vp, vp, ctypes.c_int, ctypes.c_int, c_f32p, vp, vp]),
    "sad_anchor_decode_f32": (ctypes.c_int, [ctypes.POINTER(AnchorDecodeArgs), vp]),
    "sad_center_decode_f32": (ctypes.c_int, [ctypes.POINTER(CenterDecodeArgs), vp]),
    "sad_anchor_targets_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int, ctypes.c_int]),
    "sad_anchor_targets_f32": (ctypes.c_int, [ctypes.POINTER(AnchorTargetsArgs), vp]),
    "sad_center_targets_f32": (ctypes.c_int, [ctypes.POINTER(CenterTargetsArgs), vp]),
    "sad_anchor_head_loss_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int] * 4),
    "sad_anchor_head_loss_f32": (ctypes.c_int, [ctypes.POINTER(AnchorHeadLossArgs), vp]),
    "sad_center_head_loss_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int] * 4),
    "sad_center_head_loss_f32": (ctypes.c_int, [ctypes.POINTER(CenterHeadLossArgs), vp]),
    "sad_roi_targets_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int, ctypes.c_int]),
    "sad_roi_targets_f32": (ctypes.c_int, [ctypes.POINTER(RoiTargetsArgs), vp]),
    "sad_roi_decode_f32": (ctypes.c_int, [vp, ctypes.c_int, vp, ctypes.c_int, ctypes.c_int, vp, vp]),
    "sad_roi_head_loss_f32": (ctypes.c_int, [ctypes.POINTER(RoiHeadLossArgs), vp]),
    "sad_roi_grid_points_f32": (ctypes.c_int, [ctypes.POINTER(RoiGridPointsArgs), vp]),
    "sad_voxel_query_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int]),
    "sad_voxel_query_f32": (ctypes.c_int, [ctypes.POINTER(VoxelQueryArgs), vp]),
    "sad_point_targets_f32": (ctypes.c_int, [ctypes.POINTER(PointTargetsArgs), vp]),
    "sad_point_head_loss_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int, ctypes.c_int]),
    "sad_point_head_loss_f32": (ctypes.c_int, [ctypes.POINTER(PointHeadLossArgs), vp]),
    "sad_mlp_grad_workspace_bytes": (ctypes.c_int, [ctypes.c_int] * 6 + [ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_size_t),
                                                                          ctypes.POINTER(ctypes.c_size_t)]),
    "sad_mlp_grad_f32": (ctypes.c_int, [ctypes.POINTER(MlpGradArgs), vp]),
    "sad_rotated_iou_loss_f32": (ctypes.c_int, [ctypes.POINTER(RotatedIouLossArgs), vp]),
    "sad_global_augment_f32": (ctypes.c_int, [ctypes.POINTER(GlobalAugmentArgs), vp]),
    "sad_gt_paste_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int] * 3),
    "sad_gt_paste_f32": (ctypes.c_int, [ctypes.POINTER(GtPasteArgs), vp]),
    "sad_det_match_f32": (ctypes.c_int, [ctypes.POINTER(DetMatchArgs), vp]),
    "sad_det_ap_keys_f32": (ctypes.c_int, [vp, vp, ctypes.c_longlong, ctypes.c_int, vp, vp]),
    "sad_det_ap_f32": (ctypes.c_int, [ctypes.POINTER(DetApArgs), vp]),
}

_lib = None

# A step plan being recorded on this thread (plan.Recorder, else None): lib() then hands out a stand-in that passes every
# launch through and appends it to the plan (3dsad-main_amd/plan.py).  Thread-local: another thread's launches are its own.
import threading
_tls = threading.local()


def recorder():
    return getattr(_tls, "rec", None)


def set_recorder(rec) -> None:
    _tls.rec = rec


def is_launch(name: str) -> bool:
    """Does this entry point enqueue device work (last argument: the stream)?  Size queries, options and the version do not."""
    return (name.startswith("sad_") and not name.endswith(("_bytes", "_floats", "_bytes_bf16"))
            and "preferred_geometry" not in name and name not in ("sad_version", "sad_last_error", "sad_set_option", "sad_mlp_padded_dims"))


def build(force: bool = False) -> str:
    """Compile every HIP source for gfx950 with hipcc (csrc/Makefile).  Works without a GPU."""
    cmd = ["make", "-C", CSRC, "-j4"] + (["-B"] if force else [])
    subprocess.check_call(cmd, stdout=subprocess.DEVNULL)
    return SO_PATH


def lib():
    """The loaded library.  Raises if it has not been built — the HIP path is the only path."""
    global _lib
    if _lib is None:
        if not os.path.exists(SO_PATH):
            raise RuntimeError(
                f"{SO_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; "
                "g.build()'` (hipcc, gfx950).  sad_amd has no CPU fallback.")
        # torch first: it brings its own HIP runtime (libamdhip64), and libsad_amd.so must bind to
        # THAT copy — loaded the other way round the process ends up with the system runtime under
        # torch's allocator and device-to-device copies of torch memory fail
        import torch  # noqa: F401
        handle = ctypes.CDLL(SO_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(handle, name)  # AttributeError here = header/library mismatch
            fn.restype = res
            fn.argtypes = args
        if handle.sad_version() != ABI_VERSION:
            raise RuntimeError(f"{SO_PATH}: ABI version {handle.sad_version()}, this binding needs {ABI_VERSION} "
                               "(stale build: run __graft_entry__.build())")
        _lib = handle
    rec = getattr(_tls, "rec", None)
    return _lib if rec is None else rec.lib


def check(code: int, what: str) -> None:
    """Turn a negative SAD_E* return code into a RuntimeError carrying sad_last_error()."""
    if code != 0:
        msg = lib().sad_last_error()
        raise RuntimeError(f"{what} failed ({code}): {msg.decode() if msg else ''}")


def set_option(key: str, value: int) -> None:
    check(lib().sad_set_option(key.encode(), int(value)), "sad_set_option")
