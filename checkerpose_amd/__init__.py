"""checkerpose_amd -- MI355X-native forward hot path of CheckerPose.

    from checkerpose_amd.model.init import InitNet_GNN
    from checkerpose_amd.model.pipeline import PoseNet_GNNskip

are drop-ins for the reference's `model.init` / `model.pipeline` classes (same constructor, forward and
state-dict keys); the arithmetic runs in libcheckerpose_hip.so (include/checkerpose_hip.h).
"""
__version__ = "0.1.0"


def set_deterministic(on=True):
    """Deterministic training mode (also: environment CHECKERPOSE_AMD_DETERMINISTIC=1, or `net.deterministic = True`): the training
    program accumulates BatchNorm sums, weight gradients and Index2Feat's scatter in a fixed order instead of with floating-point
    atomics -- two runs of the same steps give bit-identical parameters, as the reference's CPU step (train.py:303-320) does.
    The switch is process-wide (the library reads it when a launch program is built): models drop their training programs when it
    changes through their own `deterministic` attribute; after calling THIS function directly, call `net.invalidate()`."""
    from . import _abi
    _abi.load().cp_set_deterministic(1 if on else 0)


def is_deterministic():
    from . import _abi
    return bool(_abi.load().cp_get_deterministic())


_RENDER_NAMES = ("render_rgb", "sample_views", "render_views", "synthetic_batch", "render_scene", "scene_masks", "scene_training_batch",
                 "sample_scene_poses")
_COCO_NAMES = ("annotate_masks", "calc_gt_coco", "mask_ious", "box_ious", "CocoSet", "eval_bop22_coco", "check_coco_results",
               "save_coco_results")
_VISIBILITY_NAMES = ("compute_vis_hpr", "hpr_visibility", "overall_visibility")
_VIS_NAMES = ("vis_poses", "depth_diff_vis", "select_estimates", "vis_est_poses", "vis_gt_poses")
_REFINE_NAMES = ("refine_poses_lm", "pose_covariance")


def __getattr__(name):
    """row N14's entry points, imported on first use (render.py pulls in torch): checkerpose_amd.render_rgb, .sample_views,
    .render_views, .synthetic_batch (and row N19's .render_scene, .scene_masks, .scene_training_batch, .sample_scene_poses);
    row N15's likewise (coco_eval.py): .annotate_masks, .calc_gt_coco, .mask_ious, .box_ious, .CocoSet,
    .eval_bop22_coco, .check_coco_results, .save_coco_results (coco_eval.evaluate is reached through the module); row N16's likewise
    (visibility.py): .compute_vis_hpr, .hpr_visibility, .overall_visibility; row N18's likewise (vis.py): .vis_poses, .depth_diff_vis,
    .select_estimates, .vis_est_poses, .vis_gt_poses; row N22's likewise (postprocess.py): .refine_poses_lm, .pose_covariance"""
    if name in _RENDER_NAMES:
        from . import render
        return getattr(render, name)
    if name in _COCO_NAMES:
        from . import coco_eval
        return getattr(coco_eval, name)
    if name in _VISIBILITY_NAMES:
        from . import visibility
        return getattr(visibility, name)
    if name in _VIS_NAMES:
        from . import vis
        return getattr(vis, name)
    if name in _REFINE_NAMES:
        from . import postprocess
        return getattr(postprocess, name)
    raise AttributeError("module %r has no attribute %r" % (__name__, name))
