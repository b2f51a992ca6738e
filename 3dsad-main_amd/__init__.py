"""MI355X-native set-abstraction + size-adaptive-clustering hot path (import as ``sad_amd``).

Operator surface named by BASELINE.json ``north_star`` (the upstream reference,
``/root/reference/README.md:1-2``, ships no code): ``fps``, ``ball_query``, ``knn_query``,
``group_points``, ``gather_points``, ``sa_module`` — Python host code on PyTorch-ROCm calling
hand-written gfx950 HIP kernels through the C-ABI library declared in ``include/sad_amd.h``.

``config`` and ``synth`` are numpy-only; everything that touches the GPU is imported lazily so the
data modules stay importable without torch.  There is no CPU fallback: operators raise if the HIP
library is missing or a tensor is not on a GPU.
"""
__version__ = "0.1.0"

# the package owns its runtime preconditions (GPU_MAX_HW_QUEUES before HIP initialises): _runtime.py
from . import _runtime
HW_QUEUES_STATE = _runtime.ensure_hw_queues()

_LAZY = {
    "fps": "ops", "ball_query": "ops", "ball_query_multi": "ops", "knn_query": "ops",
    "group_points": "ops", "gather_points": "ops", "gather_xyz": "ops",
    "mlp_chain": "mlp", "PackedMLP": "mlp", "nms_bev": "ops", "nms_boxes": "ops", "nms_boxes_buffers": "ops",
    "three_nn": "ops", "three_interpolate": "ops", "FPModule": "fp_module",
    "boxes_iou_bev": "ops", "boxes_iou3d": "ops", "points_in_boxes": "ops", "roipoint_pool3d": "ops",
    "voxel_coords": "ops", "voxel_index": "ops", "voxelize": "ops", "voxel_reduce": "ops",
    "voxel_decorate": "ops", "voxel_encode": "ops",
    "anchor_decode": "ops", "center_decode": "ops", "anchor_grid": "dense_head",
    "AnchorHeadDecoder": "dense_head", "CenterHeadDecoder": "dense_head",
    "anchor_targets": "ops", "center_targets": "ops",
    "AnchorTargetAssigner": "dense_head", "CenterTargetAssigner": "dense_head",
    "anchor_head_loss": "ops", "center_head_loss": "ops", "anchor_head_loss_workspace": "ops", "center_head_loss_workspace": "ops",
    "AnchorHeadLoss": "dense_head", "CenterHeadLoss": "dense_head",
    "roi_targets": "ops", "roi_targets_workspace": "ops", "roi_decode": "ops", "ProposalTargetLayer": "roi_head",
    "roi_head_loss": "ops", "RoIHeadLoss": "roi_head",
    "rotated_iou_loss": "ops", "boxes_iou_aligned": "ops", "RotatedIoULoss": "iou_loss", "RoIIoULoss": "roi_head",
    "point_targets": "ops", "point_head_loss": "ops", "point_head_loss_workspace": "ops",
    "PointTargetAssigner": "point_head", "PointHeadLoss": "point_head",
    "roi_grid_points": "ops", "voxel_query": "ops", "voxel_query_workspace": "ops", "VoxelRoIPool": "voxel_roi_pool",
    "Voxelization": "voxel", "DynamicScatter": "voxel", "PillarFeatureNet": "voxel",
    "sparse_conv_index": "ops", "sparse_conv": "ops", "sparse_to_dense": "ops", "PackedSparseWeight": "ops",
    "sparse_conv_index_transpose": "ops", "sparse_conv_grad_weight": "ops", "sparse_conv_grad_input": "ops",
    "sparse_max_pool": "ops", "sparse_max_pool_grad": "ops", "SparseMaxPool3d": "spconv", "SparseInverseConv3d": "spconv",
    "SparseTensor": "spconv", "Rulebook": "spconv", "SubMConv3d": "spconv", "SparseConv3d": "spconv", "SparseSequential": "spconv",
    "SAModuleMSG": "sa_module", "SAModule": "sa_module", "sa_module": "sa_module", "SAModuleMSGTrain": "sa_module",
    "SharedMLP": "shared_mlp", "BranchGroup": "shared_mlp", "grouped_mlp_grad": "mlp", "mlp_rows_grad": "mlp",
    "candidates": "ops", "candidates_grad": "ops", "prefix_rows_grad": "ops", "SADDetectorTrain": "detector_train",
    "global_augment": "ops", "gt_paste": "ops", "gt_paste_workspace": "ops", "gt_paste_rows": "ops",
    "GTDatabase": "augment", "GTSampler": "augment", "GlobalAugment": "augment", "TrainAugment": "augment",
    "det_match": "ops", "det_ap": "ops", "det_ap_workspace": "ops", "DetectionEval": "evaluate",
    "SADDetector": "detector", "IngestPipeline": "pipeline",
    "shard_range": "dist", "all_gather_boxes": "dist", "run_sharded": "dist",
}


def __getattr__(name):
    if name in _LAZY:
        import importlib
        mod = importlib.import_module(f"{__name__}.{_LAZY[name]}")
        return getattr(mod, name)
    raise AttributeError(name)
