// Version / error strings and hipGraph capture helpers of the C ABI.
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include "common.h"

// 0.2.45: cp_verify_poses_photo, cp_verify_poses_photo_tex, cp_verify_poses_photo_scratch_bytes;
// 0.2.44: cp_code_reliability, cp_code_reliability_scratch_bytes, cp_fit_code_scale, cp_fit_code_scale_scratch_bytes,
//         cp_fit_code_scale_info_doubles, cp_sigma2_consistency;
// 0.2.43: cp_rank_correspondences, cp_pnp_conf, cp_pnp_conf_scratch_bytes;
// 0.2.42: cp_code_confidence, cp_pnp_refine_wlm, cp_pnp_refine_wlm_info_doubles;
// 0.2.39: cp_coco_rle_unpack, cp_coco_rle_unpack_scratch_bytes;
// 0.2.37: cp_paste_masks, cp_paste_rle_count, cp_paste_rle_write, cp_coco_unpack;
// 0.2.36: cp_verify_poses, cp_verify_poses_scratch_bytes, cp_select_poses;
// 0.2.35: cp_lift_correspondences, cp_pose_depth_ransac, cp_pose_depth_ransac_scratch_bytes, cp_pose_depth_record_doubles;
// 0.2.34: cp_surface_samples, cp_surface_samples_scratch_bytes, cp_icp_refine, cp_icp_refine_record_doubles,
//         cp_icp_refine_info_doubles;
// 0.2.33: cp_pose_rete, cp_rete_pass_counts, cp_rete_pass_columns;
// 0.2.32: cp_pnp_refine_lm, cp_pnp_refine_lm_record_doubles, cp_pnp_refine_lm_info_doubles;
// 0.2.31: cp_warp_affine_u8, cp_warp_mask_bits;
// 0.2.20: cp_render_scene, cp_render_scene_scratch_bytes, cp_crop_mask_bits;
// 0.2.19: cp_vis_poses, cp_vis_poses_scratch_bytes, cp_depth_diff_vis, cp_depth_diff_vis_scratch_bytes;
// 0.2.18: cp_radius_graph_count, cp_radius_graph_fill, cp_graphcut_label, cp_pnp_gc, cp_pnp_gc_scratch_bytes;
// 0.2.17: cp_hpr_visibility, cp_hpr_visibility_scratch_bytes;
// 0.2.16: cp_coco_pack, cp_coco_rle_count, cp_coco_rle_write, cp_coco_mask_iou, cp_coco_box_iou, cp_coco_match,
//         cp_coco_match_scratch_bytes, cp_coco_accumulate;
// 0.2.15: cp_render_rgb, cp_render_rgb_scratch_bytes;
// 0.2.12: cp_bop_match, cp_bop_match_scratch_bytes, cp_bop_scores;
// 0.2.11: cp_gt_info, cp_gt_info_from_depth, cp_gt_info_scratch_bytes;
// 0.2.10: cp_fps, cp_fps_scratch_bytes, cp_pts_diameter, cp_pts_diameter_scratch_bytes;
// 0.2.9: cp_vsd_errors, cp_vsd_errors_scratch_bytes, cp_vsd_from_depth, cp_render_depth;
// 0.2.8: cp_bop_errors, cp_bop_errors_scratch_bytes, cp_bop_errors_map_scratch_bytes;
// 0.2.7: cp_encode_targets, cp_code_report; 0.2.6: cp_pose_errors, cp_pose_errors_scratch_bytes;
// 0.2.5: cp_bn_train_fused, cp_bn_bwd_fused, cp_conv3x3_halo_group, cp_conv3x3_halo_group_supported, cp_conv3x3_halo_item,
//        cp_graph_capture_set_deps and cp_graph_capture_tail removed (opt-in launch paths that lost their A/B measurements);
// 0.2.4: cp_set_deterministic, cp_status_*; 0.2.3: cp_kernel_log (0.2.2: cp_graph_capture_set_deps / _tail; 0.2.1:
// cp_pack_hr_chain_weight takes the folded-BN scale)
extern "C" int cp_version(void) { return 245; }

// process-wide mode switch of the TRAINING entry points (include/checkerpose_hip.h): every accumulation in a fixed order
std::atomic<int> g_cp_deterministic{0};
extern "C" void cp_set_deterministic(int on) { g_cp_deterministic.store(on ? 1 : 0, std::memory_order_relaxed); }
extern "C" int cp_get_deterministic(void) { return g_cp_deterministic.load(std::memory_order_relaxed); }

// ---- device-side error channel: ONE sticky uint32 per device (allocated on the first call of that device, outside any capture),
// OR-ed into by kernels that can detect a failure of their own (bit list: include/checkerpose_hip.h), read back by cp_device_status()
static std::atomic<uint32_t*> g_status_word[256];
uint32_t* cp_status_word(bool create) {
  const int dev = cp_current_device();
  if (dev < 0 || dev > 255) return nullptr;
  uint32_t* p = g_status_word[dev].load(std::memory_order_acquire);
  if (p || !create) return p;
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(nullptr, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone) return nullptr;
  uint32_t* q = nullptr;
  if (hipMalloc((void**)&q, 256) != hipSuccess) return nullptr;
  if (hipMemset(q, 0, 256) != hipSuccess) { (void)hipFree(q); return nullptr; }
  uint32_t* expect = nullptr;
  if (!g_status_word[dev].compare_exchange_strong(expect, q, std::memory_order_acq_rel)) { (void)hipFree(q); return expect; }
  return q;
}
extern "C" int cp_device_status(uint32_t* status_out, int clear) {
  if (!status_out) return CP_ERR_INVALID;
  uint32_t* p = cp_status_word(true);
  if (!p) return CP_ERR_HIP;
  if (hipMemcpy(status_out, p, sizeof(uint32_t), hipMemcpyDeviceToHost) != hipSuccess) return CP_ERR_HIP;      // synchronises with the device
  if (clear && *status_out && hipMemset(p, 0, sizeof(uint32_t)) != hipSuccess) return CP_ERR_HIP;
  return CP_OK;
}

static thread_local char g_last_kernel[128] = "";
static thread_local char g_kernel_log[1024] = "";   // every symbol since cp_kernel_log_begin(), " + " between them
void cp_mark_kernel(const char* fmt, ...) {
  char tmp[128];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(tmp, sizeof(tmp), fmt, ap);
  va_end(ap);
  // "(name<args>)" from a stringified launch expression -> "name<args>"
  const char* b = tmp;
  size_t n = strlen(tmp);
  if (n >= 2 && tmp[0] == '(' && tmp[n - 1] == ')') { b = tmp + 1; n -= 2; }
  memcpy(g_last_kernel, b, n);
  g_last_kernel[n] = 0;
  const size_t have = strlen(g_kernel_log);
  if (have + n + 4 < sizeof(g_kernel_log))
    snprintf(g_kernel_log + have, sizeof(g_kernel_log) - have, "%s%s", have ? " + " : "", g_last_kernel);
}
extern "C" const char* cp_last_kernel(void) { return g_last_kernel; }
extern "C" void cp_kernel_log_begin(void) { g_kernel_log[0] = 0; }
extern "C" const char* cp_kernel_log(void) { return g_kernel_log; }

extern "C" const char* cp_strerror(int code) {
  switch (code) {
    case CP_OK: return "ok";
    case CP_ERR_INVALID: return "invalid argument or unsupported shape";
    case CP_ERR_HIP: return "HIP runtime error (kernel launch / graph call failed)";
    case CP_ERR_ALIGN: return "pointer, channel count or stride not aligned to 16 bytes / 4 channels";
    case CP_ERR_RANGE: return "buffer exceeds 2 GiB 32-bit buffer addressing";
    default: return "unknown checkerpose_hip error code";
  }
}

// hipGraph: the forward is ~350 short launches; replaying them as one graph removes the per-launch host
// cost.  Capture mode is thread-local so other threads (e.g. a data loader touching HIP) are not affected.
extern "C" int cp_graph_begin_capture(cp_stream_t stream) {
  return hipStreamBeginCapture((hipStream_t)stream, hipStreamCaptureModeThreadLocal) == hipSuccess ? CP_OK : CP_ERR_HIP;
}

extern "C" int cp_graph_end_capture(cp_stream_t stream, void** graph_exec_out) {
  if (!graph_exec_out) return CP_ERR_INVALID;
  hipGraph_t graph = nullptr;
  if (hipStreamEndCapture((hipStream_t)stream, &graph) != hipSuccess || !graph) return CP_ERR_HIP;
  hipGraphExec_t exec = nullptr;
  hipError_t e = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
  (void)hipGraphDestroy(graph);
  if (e != hipSuccess) return CP_ERR_HIP;
  *graph_exec_out = (void*)exec;
  return CP_OK;
}

extern "C" int cp_graph_launch(void* graph_exec, cp_stream_t stream) {
  if (!graph_exec) return CP_ERR_INVALID;
  return hipGraphLaunch((hipGraphExec_t)graph_exec, (hipStream_t)stream) == hipSuccess ? CP_OK : CP_ERR_HIP;
}

extern "C" int cp_graph_destroy(void* graph_exec) {
  if (!graph_exec) return CP_OK;
  return hipGraphExecDestroy((hipGraphExec_t)graph_exec) == hipSuccess ? CP_OK : CP_ERR_HIP;
}
