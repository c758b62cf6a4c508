// extern "C" boundary of libmtrssm_hip.so (declared in include/mtrssm.h).
#include <stdarg.h>
#include <stdio.h>

#include "scan_common.h"

namespace mtrssm {

static thread_local char g_err[512] = "";
static thread_local const char* g_kernel = "";

void set_last_kernel(const char* name) { g_kernel = name; }

void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

int mrssm_fwd_launch(const MtrssmMrssmDims*, const MtrssmMrssmFwdWeights*, const MtrssmMrssmFwdIO*, hipStream_t);
int mrssm_bwd_launch(const MtrssmMrssmDims*, const MtrssmMrssmBwdWeights*, const MtrssmMrssmBwdIO*, hipStream_t);
int mmtrssm_fwd_launch(const MtrssmMmtrssmDims*, const MtrssmMmtrssmFwdWeights*, const MtrssmMmtrssmFwdIO*, hipStream_t);
int mmtrssm_bwd_launch(const MtrssmMmtrssmDims*, const MtrssmMmtrssmBwdWeights*, const MtrssmMmtrssmBwdIO*, hipStream_t);
int conv_gather_gemm_launch(const MtrssmConvGeom*, const float*, const float*, const float*, const unsigned short*, const float*, const float*, const float*, float*, hipStream_t);
int episode_gather_launch(const float*, const int64_t*, const float*, int64_t, int64_t, int64_t, int64_t, int64_t, float, float*, float*, hipStream_t);
int episode_gather_window_launch(const float*, const int64_t*, const int32_t*, const float*, int64_t, int64_t, int64_t, int64_t, int64_t, float, float*,
                                 float*, hipStream_t);
int state_select_launch(const MtrssmStateTable*, const unsigned char*, int64_t, hipStream_t);
int state_save_launch(const MtrssmStateTable*, int64_t, int64_t, hipStream_t);
int state_save_at_launch(const MtrssmStateTable*, const int32_t*, int64_t, int64_t, hipStream_t);
int episode_gather_ragged_launch(const float*, const int64_t*, const int32_t*, const int32_t*, const float*, int64_t, int64_t, int64_t, int64_t,
                                 int64_t, float, float*, float*, int32_t*, hipStream_t);
int episode_gather_seeded_launch(const float*, const int64_t*, const int32_t*, const int32_t*, int32_t*, uint32_t, uint32_t, uint32_t, int64_t, int64_t,
                                 int64_t, int64_t, int64_t, float, float*, float*, hipStream_t);
int episode_gather_augmented_launch(const MtrssmFeedAugment*, const float*, const int64_t*, const int32_t*, const int32_t*, int32_t*, uint32_t, uint32_t,
                                    uint32_t, uint32_t, uint32_t, int64_t, int64_t, int64_t, int64_t, int64_t, int64_t, int64_t, int32_t, float, float*,
                                    float*, hipStream_t);
int step_mask_ragged_launch(const int32_t*, const float*, int64_t, int64_t, int64_t, float, float, int64_t, int64_t, int32_t*, float*, float*, float*,
                            unsigned char*, int32_t*, float*, hipStream_t);
int step_mask_forecast_launch(const int32_t*, const float*, const float*, int64_t, int64_t, int64_t, float, float, int64_t, int64_t, int64_t, int64_t,
                              int32_t*, float*, float*, float*, float*, unsigned char*, int32_t*, float*, hipStream_t);
int elbo_combine_counted_fwd_launch(const float*, const float*, const float*, const float*, const float*, const float*, int64_t, float, float, float*,
                                    float*, float*, float*, hipStream_t);
int elbo_combine_counted_bwd_launch(const float*, const float*, const float*, const float*, const float*, const float*, int64_t, float, float, float*,
                                    float*, float*, float*, hipStream_t);
int elbo_schedule_fwd_launch(const float*, const float*, const float*, const float*, const float*, const float*, const float*, int64_t,
                             MtrssmElboSchedule, float*, float*, float*, float*, float*, float*, hipStream_t);
int elbo_schedule_bwd_launch(const float*, const float*, const float*, const float*, const float*, const float*, const float*, const float*,
                             const float*, int64_t, MtrssmElboSchedule, float*, float*, float*, float*, hipStream_t);
int conv_gather_gemm_pair_launch(const MtrssmConvGeom*, const float*, const float*, const float*, const unsigned short*, const float*, const float*, const float*, float*,
                                 const MtrssmConvGeom*, const float*, const float*, const float*, const unsigned short*, const float*, const float*, const float*, float*, hipStream_t);
int conv_residual_fwd_supported(const MtrssmConvGeom*);
int conv_residual_fwd_launch(const MtrssmConvGeom*, const float*, const unsigned short*, const float*, const float*, const float*, float*, float*,
                             const MtrssmConvGeom*, const float*, const unsigned short*, const float*, const float*, const float*, float*, float*, hipStream_t);
int pack_conv_weight_launch(const float*, int, int, int, int, long, long, long, long, int, int, int, float*, unsigned short*, hipStream_t);
int pack_conv_weights_launch(const int64_t*, int, int, hipStream_t);
int conv_gather_pair_merges(const MtrssmConvGeom*, const MtrssmConvGeom*, bool);
int conv_weight_grad_launch(const MtrssmConvGeom*, const float*, const float*, const float*, int, float*, float*, void*, size_t, size_t*, hipStream_t);
int conv_weight_grad_deferred_launch(const MtrssmConvGeom*, const float*, const float*, const float*, int, float*, float*, void*, size_t, hipStream_t);
int conv_weight_grad_reduce_flush(hipStream_t);
int conv_residual_bwd1x1_supported(const MtrssmConvGeom*);
int conv_residual_bwd1x1_launch(const MtrssmConvGeom*, const float*, const float*, const unsigned short*, float*, float*, float*, void*, size_t, int,
                                hipStream_t);
int conv_residual_bwd1x1_pair_supported(const MtrssmConvGeom*, const MtrssmConvGeom*);
int conv_residual_bwd1x1_pair_launch(const MtrssmConvGeom*, const float*, const float*, const unsigned short*, float*, float*, float*, void*, size_t,
                                     const MtrssmConvGeom*, const float*, const float*, const unsigned short*, float*, float*, float*, void*, size_t, int,
                                     hipStream_t);
int conv_weight_grad_pair_supported(const MtrssmConvGeom*, const MtrssmConvGeom*);
int conv_weight_grad_pair_launch(const MtrssmConvGeom*, const float*, const float*, float*, float*, void*, size_t, const MtrssmConvGeom*, const float*,
                                 const float*, float*, float*, void*, size_t, int, hipStream_t);
int conv_weight_grad_src_bias_supported(const MtrssmConvGeom*, int);
int conv_weight_grad_src_bias_launch(const MtrssmConvGeom*, const float*, const float*, int, float*, float*, void*, size_t, int, hipStream_t);
int channel_sum_launch(const float*, int, int, int, float*, hipStream_t);
int convt_k4s2_band_supported(int, int, int, int, int);
int convt_k4s2_band_launch(int, int, int, int, int, const float*, const float*, const float*, int, int, float*, hipStream_t);
int encoder_stem_supported(const MtrssmEncoderStem*);
int encoder_stem_launch(const MtrssmEncoderStem*, const MtrssmEncoderStem*, hipStream_t);
int convt_k4s2_thin_launch(int, int, int, int, int, const float*, const float*, const float*, int, int, float*, hipStream_t);
int conv_convt_quad_supported(const MtrssmConvGeom*);
int conv_convt_quad_launch(const MtrssmConvGeom*, const float*, const unsigned short* const*, const float*, const float*, float*,
                           const MtrssmConvGeom*, const float*, const unsigned short* const*, const float*, const float*, float*, hipStream_t);
int conv_tgather_thin_launch(int, int, int, int, int, int, int, int, int, int, int, const float*, const float*, const float*, int, int, const float*,
                             const float*, float*, hipStream_t);
int categorical_sample_fwd_launch(const float*, const float*, int64_t, int, int, float*, float*, float*, hipStream_t);
int categorical_sample_bwd_launch(const float*, const float*, const float*, int64_t, int, int, float*, hipStream_t);
int elbo_combine_fwd_launch(const float*, const float*, const float*, const float*, int64_t, float, float, float*, float*, float*, float*, hipStream_t);
int elbo_combine_bwd_launch(const float*, const float*, const float*, const float*, int64_t, float, float, float*, float*, float*, float*, hipStream_t);
int nll_fwd_launch(const float*, const float*, int64_t, int64_t, int, float*, hipStream_t);
int nll_bwd_launch(const float*, const float*, const float*, int64_t, int64_t, int, float*, hipStream_t);
int nll_masked_fwd_launch(const float*, const float*, const float*, const float*, int64_t, int64_t, int, float*, hipStream_t);
int nll_masked_bwd_launch(const float*, const float*, const float*, const float*, const float*, int64_t, int64_t, int, float*, hipStream_t);
int ensemble_score_launch(const float*, const float*, const int32_t*, int64_t, int64_t, int64_t, int64_t, int, float*, float*, float*, float*, float*,
                          hipStream_t);
int horizon_table_launch(const float*, int64_t, const int32_t*, const int32_t*, int64_t, int64_t, float*, float*, hipStream_t);
int latent_log_ratio_launch(const float*, const float*, const float*, int64_t, int64_t, int64_t, int, float*, hipStream_t);
int iw_bound_launch(const float*, const float*, const float*, const int32_t*, int64_t, int64_t, int64_t, int64_t, int64_t, float*, hipStream_t);
int particle_fold_launch(const float*, const float*, const float*, const int32_t*, const float*, int64_t, int64_t, int64_t, int64_t, int64_t, int64_t,
                         int64_t, double, int, double*, float*, int32_t*, hipStream_t);
int particle_gather_launch(const MtrssmStateTable*, const int32_t*, int64_t, int64_t, int64_t, hipStream_t);
int overshoot_gather_launch(const MtrssmStateTable*, const float*, float*, int64_t, int64_t, int64_t, int64_t, int64_t, int64_t, int64_t, hipStream_t);
int overshoot_scatter_launch(const MtrssmStateTable*, int64_t, int64_t, int64_t, int64_t, int64_t, hipStream_t);
int64_t overshoot_kl_workspace_bytes(int64_t, int64_t, int64_t);
int overshoot_kl_fwd_launch(const float*, const float*, const int32_t*, int64_t, int64_t, int64_t, int64_t, int64_t, int64_t, int64_t, int64_t, int64_t,
                            int64_t, float*, double*, float*, float*, void*, int64_t, hipStream_t);
int overshoot_kl_bwd_launch(const float*, const float*, const int32_t*, const float*, const float*, int64_t, int64_t, int64_t, int64_t, int64_t, int64_t,
                            int64_t, int64_t, int64_t, int64_t, float, float, float*, float*, hipStream_t);
int64_t latent_census_workspace_bytes(int64_t, int64_t, int64_t, int64_t, int64_t);
int latent_census_launch(const float*, const float*, const float*, const int32_t*, int64_t, int64_t, int64_t, int64_t, int64_t, float*, double*, void*,
                         int64_t, hipStream_t);
int64_t coherence_fold_workspace_bytes(int64_t, int64_t, int64_t, int64_t);
int coherence_fold_launch(const float*, const float*, const int32_t*, const int32_t*, int64_t, int64_t, int64_t, int64_t, int64_t, float*, double*, void*,
                          int64_t, hipStream_t);
int64_t feature_moments_workspace_bytes(int64_t, int, int);
int feature_moments_launch(const float*, int64_t, const int32_t*, int64_t, int, int, double*, void*, int64_t, hipStream_t);
int64_t linear_probe_workspace_bytes(int64_t, int64_t, int64_t, int64_t);
int linear_probe_step_launch(const float*, int64_t, int64_t, const int32_t*, const float*, const float*, int64_t, int64_t, int64_t, int64_t, int, float*,
                             float*, float*, float*, float*, int32_t*, void*, int64_t, hipStream_t);
int64_t episode_panel_bytes(const MtrssmPanelGeom*, int32_t*, int32_t*);
int episode_panel_launch(const MtrssmPanelGeom*, const float*, const float*, const float*, const float*, const float*, const float*, const int32_t*,
                         const int32_t*, const int32_t*, unsigned char*, hipStream_t);
int digit_features_launch(const float*, int64_t, const int32_t*, int64_t, int, const float*, const float*, const float*, const float*, float*,
                          hipStream_t);
int digit_head_launch(const float*, const float*, const float*, int64_t, const int32_t*, int64_t, int32_t*, float*, hipStream_t);
int word_counts_launch(const int32_t*, const int32_t*, int64_t, float*, hipStream_t);
int digit_features_train_launch(const float*, int64_t, const int32_t*, int64_t, int, const float*, const float*, const float*, const float*, float*,
                                unsigned char*, hipStream_t);
int64_t digit_trunk_bwd_workspace_bytes(int64_t);
int digit_trunk_bwd_launch(const float*, int64_t, const int32_t*, int64_t, int, const unsigned char*, const float*, const int32_t*, const float*,
                           const float*, const float*, float*, float*, float*, float*, int, void*, int64_t, hipStream_t);
int64_t digit_head_train_workspace_bytes(int64_t);
int digit_head_train_launch(const float*, const float*, const float*, const int32_t*, const int32_t*, int64_t, int64_t, int64_t, uint32_t, uint32_t, float, int, float*,
                            int32_t*, float*, float*, float*, float*, int, void*, int64_t, hipStream_t);
int modality_dropout_launch(const float*, int64_t, int64_t, int64_t, float, float, int64_t, int64_t, int32_t*, float*, float*, unsigned char*, float*,
                            hipStream_t);
int sumsq_launch(const float*, int64_t, float*, hipStream_t);
int adamw_launch(float*, const float*, float*, float*, int64_t, const float*, float, float, float, float, float, float, float, int, hipStream_t);
int gemm_launch(const MtrssmGemm*, hipStream_t);
int gemm_group_launch(const MtrssmGemm*, int, hipStream_t);
int debug_set_cluster_profile(void*);
int debug_set_resident_profile(void*);
int debug_set_wide_profile(void*);
int debug_set_mmt_profile(void*);
int mrssm_cluster_supported(const MtrssmMrssmDims*);
size_t mrssm_cluster_workspace_bytes(const MtrssmMrssmDims*);
size_t mrssm_cluster_bwd_workspace_bytes(const MtrssmMrssmDims*);
int mrssm_bwd_cluster_launch(const MtrssmMrssmDims*, const MtrssmMrssmClusterWeights*, const MtrssmMrssmBwdIO*, void*, size_t, hipStream_t);
int mrssm_fwd_cluster_launch(const MtrssmMrssmDims*, const MtrssmMrssmClusterWeights*, const MtrssmMrssmFwdIO*, void*, size_t, hipStream_t);
int unpack_conv_grads_launch(const int64_t*, int, int, hipStream_t);
int mrssm_wide_supported(const MtrssmMrssmDims*, int);
size_t mrssm_wide_workspace_bytes(const MtrssmMrssmDims*, int);
size_t mrssm_wide_bwd_workspace_bytes(const MtrssmMrssmDims*, int);
int mrssm_wide_fwd_launch(const MtrssmMrssmDims*, const MtrssmMrssmClusterWeights*, const MtrssmMrssmFwdIO*, int, void*, size_t, hipStream_t);
int mrssm_wide_bwd_launch(const MtrssmMrssmDims*, const MtrssmMrssmClusterWeights*, const MtrssmMrssmBwdIO*, int, void*, size_t, hipStream_t);
int64_t mrssm_scan_prepare_layout(int, int, int, int64_t*);
int initial_state_supported(const MtrssmInitialState*);
int initial_state_fwd_launch(const MtrssmInitialState*, hipStream_t);
int initial_state_bwd_launch(const MtrssmInitialState*, hipStream_t);
int mrssm_scan_prepare_launch(const MtrssmScanPrepare*, hipStream_t);
int adamw_prepare_launch(const float*, int64_t, float*, float*, const int*, float, float, hipStream_t);
int adamw_apply_launch(float*, const float*, float*, float*, const unsigned char*, int64_t, const float*, const float*, const int*, float, float, float,
                       float, float, float, hipStream_t);

// Compute units of the calling thread's current device (0 when there is no device): the kernels whose workgroups wait for each
// other size their grids by it.  A cache of an immutable device property, not state.
int mmtrssm_wide_supported(const MtrssmMmtrssmDims*, int);
size_t mmtrssm_wide_workspace_bytes(const MtrssmMmtrssmDims*, int);
size_t mmtrssm_wide_bwd_workspace_bytes(const MtrssmMmtrssmDims*, int);
int mmtrssm_wide_fwd_launch(const MtrssmMmtrssmDims*, const MtrssmMmtrssmFwdWeights*, const MtrssmMmtrssmFwdIO*, int, void*, size_t, hipStream_t);
int mmtrssm_wide_bwd_launch(const MtrssmMmtrssmDims*, const MtrssmMmtrssmBwdWeights*, const MtrssmMmtrssmBwdIO*, int, void*, size_t, hipStream_t);

int device_cu_count() {
  static int cached[64] = {0};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) { (void)hipGetLastError(); return 0; }
  if (dev < 0 || dev >= 64) return 0;
  if (cached[dev] > 0) return cached[dev];
  int v = 0;
  if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || v <= 0) { (void)hipGetLastError(); return 0; }
  cached[dev] = v;
  return v;
}

}  // namespace mtrssm

using namespace mtrssm;
#define MTRSSM_API extern "C" __attribute__((visibility("default")))

// expert_logw (weighted MoPoE) is read by the masked scan instances only: it needs the modality codes (all "both" when nothing is
// missing).  A prior-only rollout has no mixture and ignores the field.
template <typename IO>
static bool expert_logw_ok(const IO* io, bool post, const char* entry) {
  if (io && post && io->expert_logw && !io->modality) {
    set_error("%s: expert_logw needs modality (pass code 3 everywhere when no modality is missing)", entry);
    return false;
  }
  return true;
}
template <typename IO>
static bool g_expert_logw_ok(const IO* io, const char* entry) {
  if (!expert_logw_ok(io, true, entry)) return false;
  if (io && io->g_expert_logw && !io->expert_logw) {
    set_error("%s: g_expert_logw needs expert_logw", entry);
    return false;
  }
  return true;
}

MTRSSM_API int mtrssm_version(void) { return MTRSSM_VERSION; }
MTRSSM_API const char* mtrssm_last_error(void) { return g_err; }
MTRSSM_API const char* mtrssm_last_kernel(void) { return g_kernel; }

MTRSSM_API int mtrssm_mrssm_rollout_fwd(const MtrssmMrssmDims* d, const MtrssmMrssmFwdWeights* w, const MtrssmMrssmFwdIO* io, void* stream) {
  if (!expert_logw_ok(io, d && d->post, "mrssm_rollout_fwd")) return MTRSSM_EINVAL;
  return mrssm_fwd_launch(d, w, io, static_cast<hipStream_t>(stream));
}
MTRSSM_API int mtrssm_mrssm_rollout_bwd(const MtrssmMrssmDims* d, const MtrssmMrssmBwdWeights* w, const MtrssmMrssmBwdIO* io, void* stream) {
  if (!g_expert_logw_ok(io, "mrssm_rollout_bwd")) return MTRSSM_EINVAL;
  return mrssm_bwd_launch(d, w, io, static_cast<hipStream_t>(stream));
}
MTRSSM_API int mtrssm_mmtrssm_rollout_fwd(const MtrssmMmtrssmDims* d, const MtrssmMmtrssmFwdWeights* w, const MtrssmMmtrssmFwdIO* io, void* stream) {
  if (!expert_logw_ok(io, d && d->post, "mmtrssm_rollout_fwd")) return MTRSSM_EINVAL;
  return mmtrssm_fwd_launch(d, w, io, static_cast<hipStream_t>(stream));
}
MTRSSM_API int mtrssm_mmtrssm_rollout_bwd(const MtrssmMmtrssmDims* d, const MtrssmMmtrssmBwdWeights* w, const MtrssmMmtrssmBwdIO* io, void* stream) {
  if (!g_expert_logw_ok(io, "mmtrssm_rollout_bwd")) return MTRSSM_EINVAL;
  return mmtrssm_bwd_launch(d, w, io, static_cast<hipStream_t>(stream));
}
MTRSSM_API int mtrssm_categorical_sample_fwd(const float* logits, const float* u, int64_t rows, int32_t K, int32_t C, float* logp, float* probs,
                                            float* onehot, void* stream) {
  return categorical_sample_fwd_launch(logits, u, rows, K, C, logp, probs, onehot, static_cast<hipStream_t>(stream));
}
MTRSSM_API int mtrssm_categorical_sample_bwd(const float* probs, const float* g_probs, const float* g_logp, int64_t rows, int32_t K, int32_t C,
                                            float* d_logits, void* stream) {
  return categorical_sample_bwd_launch(probs, g_probs, g_logp, rows, K, C, d_logits, static_cast<hipStream_t>(stream));
}
MTRSSM_API int mtrssm_elbo_combine_fwd(const float* nll_a, const float* nll_v, const float* kl0, const float* kl1, int64_t n, float c0, float c1,
                                      float* o_recon, float* o_k0, float* o_k1, float* o_loss, void* stream) {
  return elbo_combine_fwd_launch(nll_a, nll_v, kl0, kl1, n, c0, c1, o_recon, o_k0, o_k1, o_loss, static_cast<hipStream_t>(stream));
}
MTRSSM_API int mtrssm_elbo_combine_bwd(const float* g_recon, const float* g_k0, const float* g_k1, const float* g_loss, int64_t n, float c0,
                                      float c1, float* g_nll_a, float* g_nll_v, float* g_kl0, float* g_kl1, void* stream) {
  return elbo_combine_bwd_launch(g_recon, g_k0, g_k1, g_loss, n, c0, c1, g_nll_a, g_nll_v, g_kl0, g_kl1, static_cast<hipStream_t>(stream));
}
MTRSSM_API int mtrssm_gaussian_nll_fwd(const float* pred, const float* target, int64_t frames, int64_t event, int32_t act, float* out, void* stream) {
  return nll_fwd_launch(pred, target, frames, event, act, out, static_cast<hipStream_t>(stream));
}
MTRSSM_API int mtrssm_gaussian_nll_bwd(const float* pred, const float* target, const float* g_out, int64_t frames, int64_t event, int32_t act,
                                       float* g_pred, void* stream) {
  return nll_bwd_launch(pred, target, g_out, frames, event, act, g_pred, static_cast<hipStream_t>(stream));
}
MTRSSM_API int mtrssm_gaussian_nll_masked_fwd(const float* pred, const float* target, const float* present, const float* count, int64_t frames,
                                              int64_t event, int32_t act, float* out, void* stream) {
  return nll_masked_fwd_launch(pred, target, present, count, frames, event, act, out, static_cast<hipStream_t>(stream));
}
MTRSSM_API int mtrssm_gaussian_nll_masked_bwd(const float* pred, const float* target, const float* present, const float* count,
                                              const float* g_out, int64_t frames, int64_t event, int32_t act, float* g_pred, void* stream) {
  return nll_masked_bwd_launch(pred, target, present, count, g_out, frames, event, act, g_pred, static_cast<hipStream_t>(stream));
}
MTRSSM_API int mtrssm_modality_dropout(const float* u, int64_t b_global, int64_t steps, int64_t span, float p_audio, float p_vision, int64_t row0,
                                       int64_t b_local, int32_t* codes, float* present_audio, float* present_vision, uint8_t* mask0,
                                       float* counts, void* stream) {
  return modality_dropout_launch(u, b_global, steps, span, p_audio, p_vision, row0, b_local, codes, present_audio, present_vision, mask0, counts,
                                 static_cast<hipStream_t>(stream));
}
MTRSSM_API int mtrssm_sumsq(const float* x, int64_t n, float* out, void* stream) {
  return sumsq_launch(x, n, out, static_cast<hipStream_t>(stream));
}
MTRSSM_API int mtrssm_adamw_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, const float* sumsq,
                                 float clip_norm, float grad_scale, float lr, float beta1, float beta2, float eps, float weight_decay,
                                 int32_t step, void* stream) {
  return adamw_launch(param, grad, exp_avg, exp_avg_sq, n, sumsq, clip_norm, grad_scale, lr, beta1, beta2, eps, weight_decay, step,
                      static_cast<hipStream_t>(stream));
}
MTRSSM_API int mtrssm_unpack_conv_grads(const int64_t* table, int32_t count, int32_t blocks_per_entry, void* stream) {
  return unpack_conv_grads_launch(table, count, blocks_per_entry, static_cast<hipStream_t>(stream));
}
MTRSSM_API int mtrssm_mrssm_cluster_supported(const MtrssmMrssmDims* d) { return mrssm_cluster_supported(d); }
MTRSSM_API int64_t mtrssm_mrssm_cluster_workspace_bytes(const MtrssmMrssmDims* d) { return (int64_t)mrssm_cluster_workspace_bytes(d); }
MTRSSM_API int mtrssm_mrssm_rollout_fwd_cluster(const MtrssmMrssmDims* d, const MtrssmMrssmClusterWeights* w, const MtrssmMrssmFwdIO* io,
                                                void* workspace, int64_t workspace_bytes, void* stream) {
  if (!expert_logw_ok(io, true, "mrssm_rollout_fwd_cluster")) return MTRSSM_EINVAL;
  return mrssm_fwd_cluster_launch(d, w, io, workspace, workspace_bytes < 0 ? 0 : (size_t)workspace_bytes, static_cast<hipStream_t>(stream));
}
/* development aid, not part of the documented ABI (tools/cluster_probe.py) */
extern "C" __attribute__((visibility("default"))) int mtrssm_debug_set_cluster_profile(void* buf) { return debug_set_cluster_profile(buf); }
extern "C" __attribute__((visibility("default"))) int mtrssm_debug_set_resident_profile(void* buf) { return debug_set_resident_profile(buf); }
extern "C" __attribute__((visibility("default"))) int mtrssm_debug_set_wide_profile(void* buf) { return debug_set_wide_profile(buf); }
extern "C" __attribute__((visibility("default"))) int mtrssm_debug_set_mmt_profile(void* buf) { return debug_set_mmt_profile(buf); }
MTRSSM_API int64_t mtrssm_mrssm_cluster_bwd_workspace_bytes(const MtrssmMrssmDims* d) { return (int64_t)mrssm_cluster_bwd_workspace_bytes(d); }
MTRSSM_API int mtrssm_mrssm_rollout_bwd_cluster(const MtrssmMrssmDims* d, const MtrssmMrssmClusterWeights* w, const MtrssmMrssmBwdIO* io,
                                                void* workspace, int64_t workspace_bytes, void* stream) {
  if (!g_expert_logw_ok(io, "mrssm_rollout_bwd_cluster")) return MTRSSM_EINVAL;
  return mrssm_bwd_cluster_launch(d, w, io, workspace, workspace_bytes < 0 ? 0 : (size_t)workspace_bytes, static_cast<hipStream_t>(stream));
}
MTRSSM_API int mtrssm_mrssm_wide_supported(const MtrssmMrssmDims* d, int32_t pieces) { return mrssm_wide_supported(d, pieces); }
MTRSSM_API int64_t mtrssm_mrssm_wide_workspace_bytes(const MtrssmMrssmDims* d, int32_t pieces) { return (int64_t)mrssm_wide_workspace_bytes(d, pieces); }
MTRSSM_API int64_t mtrssm_mrssm_wide_bwd_workspace_bytes(const MtrssmMrssmDims* d, int32_t pieces) {
  return (int64_t)mrssm_wide_bwd_workspace_bytes(d, pieces);
}
MTRSSM_API int mtrssm_mrssm_rollout_fwd_wide(const MtrssmMrssmDims* d, const MtrssmMrssmClusterWeights* w, const MtrssmMrssmFwdIO* io, int32_t pieces,
                                             void* workspace, int64_t workspace_bytes, void* stream) {
  if (!expert_logw_ok(io, true, "mrssm_rollout_fwd_wide")) return MTRSSM_EINVAL;
  return mrssm_wide_fwd_launch(d, w, io, pieces, workspace, workspace_bytes < 0 ? 0 : (size_t)workspace_bytes, static_cast<hipStream_t>(stream));
}
MTRSSM_API int mtrssm_mrssm_rollout_bwd_wide(const MtrssmMrssmDims* d, const MtrssmMrssmClusterWeights* w, const MtrssmMrssmBwdIO* io, int32_t pieces,
                                             void* workspace, int64_t workspace_bytes, void* stream) {
  if (!g_expert_logw_ok(io, "mrssm_rollout_bwd_wide")) return MTRSSM_EINVAL;
  return mrssm_wide_bwd_launch(d, w, io, pieces, workspace, workspace_bytes < 0 ? 0 : (size_t)workspace_bytes, static_cast<hipStream_t>(stream));
}
MTRSSM_API int mtrssm_mmtrssm_wide_supported(const MtrssmMmtrssmDims* d, int32_t pieces) { return mmtrssm_wide_supported(d, pieces); }
MTRSSM_API int64_t mtrssm_mmtrssm_wide_workspace_bytes(const MtrssmMmtrssmDims* d, int32_t pieces) { return (int64_t)mmtrssm_wide_workspace_bytes(d, pieces); }
MTRSSM_API int64_t mtrssm_mmtrssm_wide_bwd_workspace_bytes(const MtrssmMmtrssmDims* d, int32_t pieces) {
  return (int64_t)mmtrssm_wide_bwd_workspace_bytes(d, pieces);
}
MTRSSM_API int mtrssm_mmtrssm_rollout_fwd_wide(const MtrssmMmtrssmDims* d, const MtrssmMmtrssmFwdWeights* w, const MtrssmMmtrssmFwdIO* io, int32_t pieces,
                                               void* workspace, int64_t workspace_bytes, void* stream) {
  if (!expert_logw_ok(io, true, "mmtrssm_rollout_fwd_wide")) return MTRSSM_EINVAL;
  return mmtrssm_wide_fwd_launch(d, w, io, pieces, workspace, workspace_bytes < 0 ? 0 : (size_t)workspace_bytes, static_cast<hipStream_t>(stream));
}
MTRSSM_API int mtrssm_mmtrssm_rollout_bwd_wide(const MtrssmMmtrssmDims* d, const MtrssmMmtrssmBwdWeights* w, const MtrssmMmtrssmBwdIO* io, int32_t pieces,
                                               void* workspace, int64_t workspace_bytes, void* stream) {
  if (!g_expert_logw_ok(io, "mmtrssm_rollout_bwd_wide")) return MTRSSM_EINVAL;
  return mmtrssm_wide_bwd_launch(d, w, io, pieces, workspace, workspace_bytes < 0 ? 0 : (size_t)workspace_bytes, static_cast<hipStream_t>(stream));
}
MTRSSM_API int mtrssm_gemm(const MtrssmGemm* g, void* stream) { return gemm_launch(g, static_cast<hipStream_t>(stream)); }
MTRSSM_API int mtrssm_gemm_group(const MtrssmGemm* problems, int32_t count, void* stream) {
  return gemm_group_launch(problems, count, static_cast<hipStream_t>(stream));
}
MTRSSM_API int mtrssm_initial_state_supported(const MtrssmInitialState* p) { return initial_state_supported(p); }
MTRSSM_API int mtrssm_initial_state_fwd(const MtrssmInitialState* p, void* stream) {
  return initial_state_fwd_launch(p, static_cast<hipStream_t>(stream));
}
MTRSSM_API int mtrssm_initial_state_bwd(const MtrssmInitialState* p, void* stream) {
  return initial_state_bwd_launch(p, static_cast<hipStream_t>(stream));
}
MTRSSM_API int64_t mtrssm_mrssm_scan_prepare_layout(int32_t D, int32_t H, int32_t S, int64_t* offsets) {
  return mrssm_scan_prepare_layout(D, H, S, offsets);
}
MTRSSM_API int mtrssm_mrssm_scan_prepare(const MtrssmScanPrepare* p, void* stream) {
  return mrssm_scan_prepare_launch(p, static_cast<hipStream_t>(stream));
}
MTRSSM_API int mtrssm_clear(void* p, int64_t bytes, void* stream) {
  return clear_async(p, bytes < 0 ? 0 : (size_t)bytes, static_cast<hipStream_t>(stream));
}
MTRSSM_API int mtrssm_adamw_prepare(const float* grad, int64_t n, float* sumsq, float* state, const int32_t* status, float beta1, float beta2,
                                    void* stream) {
  return adamw_prepare_launch(grad, n, sumsq, state, status, beta1, beta2, static_cast<hipStream_t>(stream));
}
MTRSSM_API int mtrssm_adamw_apply(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, const uint8_t* active, int64_t n,
                                  const float* sumsq, const float* state, const int32_t* status, float clip_norm, float grad_scale, float beta1,
                                  float beta2, float eps, float weight_decay, void* stream) {
  return adamw_apply_launch(param, grad, exp_avg, exp_avg_sq, active, n, sumsq, state, status, clip_norm, grad_scale, beta1, beta2, eps,
                            weight_decay, static_cast<hipStream_t>(stream));
}
MTRSSM_API int mtrssm_conv_gather_gemm(const MtrssmConvGeom* g, const float* src, const float* src2, const float* wp, const uint16_t* wq,
                                       const float* bias, const float* actgrad_in, const float* add_in, float* out, void* stream) {
  return conv_gather_gemm_launch(g, src, src2, wp, wq, bias, actgrad_in, add_in, out, static_cast<hipStream_t>(stream));
}
MTRSSM_API int mtrssm_episode_gather(const float* store, const int64_t* idx, const float* noise, int64_t n_episodes, int64_t B, int64_t T,
                                     int64_t Tfull, int64_t E, float std_, float* input, float* target, void* stream) {
  return episode_gather_launch(store, idx, noise, n_episodes, B, T, Tfull, E, std_, input, target, static_cast<hipStream_t>(stream));
}
MTRSSM_API int mtrssm_episode_gather_window(const float* store, const int64_t* idx, const int32_t* start, const float* noise, int64_t n_episodes,
                                            int64_t B, int64_t T, int64_t Tfull, int64_t E, float std_, float* input, float* target, void* stream) {
  return episode_gather_window_launch(store, idx, start, noise, n_episodes, B, T, Tfull, E, std_, input, target, static_cast<hipStream_t>(stream));
}
MTRSSM_API int mtrssm_state_select(const MtrssmStateTable* table, const uint8_t* reset, int64_t B, void* stream) {
  return state_select_launch(table, reset, B, static_cast<hipStream_t>(stream));
}
MTRSSM_API int mtrssm_state_save(const MtrssmStateTable* table, int64_t B, int64_t steps, void* stream) {
  return state_save_launch(table, B, steps, static_cast<hipStream_t>(stream));
}
MTRSSM_API int mtrssm_state_save_at(const MtrssmStateTable* table, const int32_t* last, int64_t B, int64_t steps, void* stream) {
  return state_save_at_launch(table, last, B, steps, static_cast<hipStream_t>(stream));
}
MTRSSM_API int mtrssm_episode_gather_ragged(const float* store, const int64_t* idx, const int32_t* start, const int32_t* lengths,
                                            const float* noise, int64_t n_episodes, int64_t B, int64_t T, int64_t Tfull, int64_t E, float std_,
                                            float* input, float* target, int32_t* valid_out, void* stream) {
  return episode_gather_ragged_launch(store, idx, start, lengths, noise, n_episodes, B, T, Tfull, E, std_, input, target, valid_out,
                                      static_cast<hipStream_t>(stream));
}
MTRSSM_API int mtrssm_episode_gather_seeded(const float* store, const int64_t* idx, const int32_t* start, const int32_t* lengths,
                                            int32_t* valid_out, uint32_t key0, uint32_t key1, uint32_t epoch, int64_t n_episodes, int64_t B,
                                            int64_t T, int64_t Tfull, int64_t E, float std_, float* input, float* target, void* stream) {
  return episode_gather_seeded_launch(store, idx, start, lengths, valid_out, key0, key1, epoch, n_episodes, B, T, Tfull, E, std_, input, target,
                                      static_cast<hipStream_t>(stream));
}
MTRSSM_API int mtrssm_episode_gather_augmented(const MtrssmFeedAugment* aug, const float* store, const int64_t* idx, const int32_t* start,
                                               const int32_t* lengths, int32_t* valid_out, uint32_t key0, uint32_t key1, uint32_t akey0,
                                               uint32_t akey1, uint32_t epoch, int64_t n_episodes, int64_t B, int64_t T, int64_t Tfull, int64_t C,
                                               int64_t H, int64_t W, int32_t noisy, float std_, float* input, float* target, void* stream) {
  return episode_gather_augmented_launch(aug, store, idx, start, lengths, valid_out, key0, key1, akey0, akey1, epoch, n_episodes, B, T, Tfull, C, H,
                                         W, noisy, std_, input, target, static_cast<hipStream_t>(stream));
}
MTRSSM_API int mtrssm_step_mask_ragged(const int32_t* valid, const float* u, int64_t b_global, int64_t steps, int64_t span, float p_audio,
                                       float p_vision, int64_t row0, int64_t b_local, int32_t* codes, float* present_audio,
                                       float* present_vision, float* live, uint8_t* mask0, int32_t* last, float* counts, void* stream) {
  return step_mask_ragged_launch(valid, u, b_global, steps, span, p_audio, p_vision, row0, b_local, codes, present_audio, present_vision, live,
                                 mask0, last, counts, static_cast<hipStream_t>(stream));
}
MTRSSM_API int mtrssm_step_mask_forecast(const int32_t* valid, const float* u_mask, const float* u_context, int64_t b_global, int64_t steps,
                                         int64_t span, float p_audio, float p_vision, int64_t lo, int64_t hi, int64_t row0, int64_t b_local,
                                         int32_t* codes, float* seen_audio, float* seen_vision, float* target, float* observed, uint8_t* mask0,
                                         int32_t* last, float* counts, void* stream) {
  return step_mask_forecast_launch(valid, u_mask, u_context, b_global, steps, span, p_audio, p_vision, lo, hi, row0, b_local, codes, seen_audio,
                                   seen_vision, target, observed, mask0, last, counts, static_cast<hipStream_t>(stream));
}
MTRSSM_API int mtrssm_elbo_schedule_fwd(const float* nll_a, const float* nll_v, const float* kl0, const float* kl1, const float* live,
                                       const float* count, const float* step, int64_t n, MtrssmElboSchedule p, float* o_recon, float* o_k0,
                                       float* o_k1, float* o_loss, float* o_beta, float* o_stats, void* stream) {
  return elbo_schedule_fwd_launch(nll_a, nll_v, kl0, kl1, live, count, step, n, p, o_recon, o_k0, o_k1, o_loss, o_beta, o_stats,
                                  static_cast<hipStream_t>(stream));
}
MTRSSM_API int mtrssm_elbo_schedule_bwd(const float* g_recon, const float* g_k0, const float* g_k1, const float* g_loss, const float* kl0,
                                       const float* kl1, const float* live, const float* count, const float* beta, int64_t n,
                                       MtrssmElboSchedule p, float* g_nll_a, float* g_nll_v, float* g_kl0, float* g_kl1, void* stream) {
  return elbo_schedule_bwd_launch(g_recon, g_k0, g_k1, g_loss, kl0, kl1, live, count, beta, n, p, g_nll_a, g_nll_v, g_kl0, g_kl1,
                                  static_cast<hipStream_t>(stream));
}
MTRSSM_API int mtrssm_elbo_combine_counted_fwd(const float* nll_a, const float* nll_v, const float* kl0, const float* kl1, const float* live,
                                               const float* count, int64_t n, float c0, float c1, float* o_recon, float* o_k0, float* o_k1,
                                               float* o_loss, void* stream) {
  return elbo_combine_counted_fwd_launch(nll_a, nll_v, kl0, kl1, live, count, n, c0, c1, o_recon, o_k0, o_k1, o_loss,
                                         static_cast<hipStream_t>(stream));
}
MTRSSM_API int mtrssm_elbo_combine_counted_bwd(const float* g_recon, const float* g_k0, const float* g_k1, const float* g_loss, const float* live,
                                               const float* count, int64_t n, float c0, float c1, float* g_nll_a, float* g_nll_v, float* g_kl0,
                                               float* g_kl1, void* stream) {
  return elbo_combine_counted_bwd_launch(g_recon, g_k0, g_k1, g_loss, live, count, n, c0, c1, g_nll_a, g_nll_v, g_kl0, g_kl1,
                                         static_cast<hipStream_t>(stream));
}
MTRSSM_API int mtrssm_conv_gather_gemm_pair(const MtrssmConvGeom* ga, const float* srca, const float* src2a, const float* wpa, const uint16_t* wqa,
                                            const float* biasa, const float* actgrada, const float* adda, float* outa,
                                            const MtrssmConvGeom* gb, const float* srcb, const float* src2b, const float* wpb, const uint16_t* wqb,
                                            const float* biasb, const float* actgradb, const float* addb, float* outb, void* stream) {
  return conv_gather_gemm_pair_launch(ga, srca, src2a, wpa, wqa, biasa, actgrada, adda, outa, gb, srcb, src2b, wpb, wqb, biasb, actgradb, addb,
                                      outb, static_cast<hipStream_t>(stream));
}
MTRSSM_API int mtrssm_residual_block_fwd_supported(const MtrssmConvGeom* g3) { return conv_residual_fwd_supported(g3) != 0; }
MTRSSM_API int mtrssm_residual_block_fwd(const MtrssmConvGeom* ga, const float* xa, const uint16_t* wq3a, const float* b3a, const float* w1a,
                                         const float* b1a, float* ha, float* ya, const MtrssmConvGeom* gb, const float* xb, const uint16_t* wq3b,
                                         const float* b3b, const float* w1b, const float* b1b, float* hb, float* yb, void* stream) {
  return conv_residual_fwd_launch(ga, xa, wq3a, b3a, w1a, b1a, ha, ya, gb, xb, wq3b, b3b, w1b, b1b, hb, yb, static_cast<hipStream_t>(stream));
}
MTRSSM_API int mtrssm_pack_conv_weight(const float* w, int32_t O, int32_t I, int32_t KH, int32_t KW, int64_t so, int64_t si, int64_t sh,
                                       int64_t sw, int32_t OPad, int32_t IPad, int32_t pieces, float* wp, uint16_t* wq, void* stream) {
  return pack_conv_weight_launch(w, O, I, KH, KW, so, si, sh, sw, OPad, IPad, pieces, wp, wq, static_cast<hipStream_t>(stream));
}
MTRSSM_API int mtrssm_conv_gather_pair_merges(const MtrssmConvGeom* ga, const MtrssmConvGeom* gb, int32_t has_wq) {
  return conv_gather_pair_merges(ga, gb, has_wq != 0);
}
MTRSSM_API int mtrssm_pack_conv_weights(const int64_t* table, int32_t count, int32_t blocks_per_weight, void* stream) {
  return pack_conv_weights_launch(table, count, blocks_per_weight, static_cast<hipStream_t>(stream));
}
MTRSSM_API int mtrssm_conv_weight_grad(const MtrssmConvGeom* g, const float* a, const float* src, const float* src2, int32_t pre_act_a,
                                       float* dwp, float* dbias, void* workspace, int64_t workspace_bytes, void* stream) {
  return conv_weight_grad_launch(g, a, src, src2, pre_act_a, dwp, dbias, workspace, workspace_bytes < 0 ? 0 : (size_t)workspace_bytes, nullptr,
                                 static_cast<hipStream_t>(stream));
}
MTRSSM_API int mtrssm_conv_weight_grad_deferred(const MtrssmConvGeom* g, const float* a, const float* src, const float* src2, int32_t pre_act_a,
                                               float* dwp, float* dbias, void* workspace, int64_t workspace_bytes, void* stream) {
  return conv_weight_grad_deferred_launch(g, a, src, src2, pre_act_a, dwp, dbias, workspace, workspace_bytes < 0 ? 0 : (size_t)workspace_bytes,
                                          static_cast<hipStream_t>(stream));
}
MTRSSM_API int mtrssm_residual_bwd1x1_supported(const MtrssmConvGeom* g) { return conv_residual_bwd1x1_supported(g) != 0; }
MTRSSM_API int mtrssm_residual_bwd1x1(const MtrssmConvGeom* g, const float* gy, const float* h, const uint16_t* wq1t, float* gh, float* dwp,
                                      float* dbias, void* workspace, int64_t workspace_bytes, int32_t defer, void* stream) {
  return conv_residual_bwd1x1_launch(g, gy, h, wq1t, gh, dwp, dbias, workspace, workspace_bytes < 0 ? 0 : (size_t)workspace_bytes, defer,
                                     static_cast<hipStream_t>(stream));
}
MTRSSM_API int mtrssm_residual_bwd1x1_pair_supported(const MtrssmConvGeom* ga, const MtrssmConvGeom* gb) {
  return conv_residual_bwd1x1_pair_supported(ga, gb) != 0;
}
MTRSSM_API int mtrssm_residual_bwd1x1_pair(const MtrssmConvGeom* ga, const float* gya, const float* ha, const uint16_t* wq1ta, float* gha, float* dwpa,
                                           float* dbiasa, void* workspace_a, int64_t workspace_a_bytes, const MtrssmConvGeom* gb, const float* gyb,
                                           const float* hb, const uint16_t* wq1tb, float* ghb, float* dwpb, float* dbiasb, void* workspace_b,
                                           int64_t workspace_b_bytes, int32_t defer, void* stream) {
  return conv_residual_bwd1x1_pair_launch(ga, gya, ha, wq1ta, gha, dwpa, dbiasa, workspace_a, workspace_a_bytes < 0 ? 0 : (size_t)workspace_a_bytes, gb,
                                          gyb, hb, wq1tb, ghb, dwpb, dbiasb, workspace_b, workspace_b_bytes < 0 ? 0 : (size_t)workspace_b_bytes, defer,
                                          static_cast<hipStream_t>(stream));
}
MTRSSM_API int mtrssm_conv_weight_grad_pair_supported(const MtrssmConvGeom* ga, const MtrssmConvGeom* gb) {
  return conv_weight_grad_pair_supported(ga, gb) != 0;
}
MTRSSM_API int mtrssm_conv_weight_grad_pair(const MtrssmConvGeom* ga, const float* aa, const float* srca, float* dwpa, float* dbiasa, void* workspace_a,
                                            int64_t workspace_a_bytes, const MtrssmConvGeom* gb, const float* ab, const float* srcb, float* dwpb,
                                            float* dbiasb, void* workspace_b, int64_t workspace_b_bytes, int32_t defer, void* stream) {
  return conv_weight_grad_pair_launch(ga, aa, srca, dwpa, dbiasa, workspace_a, workspace_a_bytes < 0 ? 0 : (size_t)workspace_a_bytes, gb, ab, srcb, dwpb,
                                      dbiasb, workspace_b, workspace_b_bytes < 0 ? 0 : (size_t)workspace_b_bytes, defer,
                                      static_cast<hipStream_t>(stream));
}
MTRSSM_API int mtrssm_conv_weight_grad_src_bias_supported(const MtrssmConvGeom* g, int32_t pre_act_a) {
  return conv_weight_grad_src_bias_supported(g, pre_act_a);
}
MTRSSM_API int mtrssm_conv_weight_grad_src_bias(const MtrssmConvGeom* g, const float* a, const float* src, int32_t pre_act_a, float* dwp,
                                                float* dsrc_bias, void* workspace, int64_t workspace_bytes, int32_t defer, void* stream) {
  return conv_weight_grad_src_bias_launch(g, a, src, pre_act_a, dwp, dsrc_bias, workspace, workspace_bytes < 0 ? 0 : (size_t)workspace_bytes,
                                          defer, static_cast<hipStream_t>(stream));
}
MTRSSM_API int mtrssm_conv_weight_grad_reduce(void* stream) { return conv_weight_grad_reduce_flush(static_cast<hipStream_t>(stream)); }
MTRSSM_API int64_t mtrssm_conv_weight_grad_workspace_bytes(const MtrssmConvGeom* g, int32_t pre_act_a) {
  size_t need = 0;
  if (conv_weight_grad_launch(g, nullptr, nullptr, nullptr, pre_act_a, nullptr, nullptr, nullptr, 0, &need, nullptr) != MTRSSM_OK) return -1;
  return (int64_t)need;
}
MTRSSM_API int mtrssm_channel_sum(const float* x, int32_t N, int32_t C, int32_t HW, float* out, void* stream) {
  return channel_sum_launch(x, N, C, HW, out, static_cast<hipStream_t>(stream));
}
MTRSSM_API int mtrssm_conv_tgather_thin(int32_t N, int32_t O, int32_t Hs, int32_t Ws, int32_t Cout, int32_t KH, int32_t KW, int32_t stride,
                                        int32_t pad, int32_t Ho, int32_t Wo, const float* y, const float* w, const float* bias, int32_t pre_act,
                                        int32_t act, const float* actgrad_in, const float* add_in, float* out, void* stream) {
  return conv_tgather_thin_launch(N, O, Hs, Ws, Cout, KH, KW, stride, pad, Ho, Wo, y, w, bias, pre_act, act, actgrad_in, add_in, out,
                                  static_cast<hipStream_t>(stream));
}
MTRSSM_API int mtrssm_convt_quad_supported(const MtrssmConvGeom* g4) { return conv_convt_quad_supported(g4); }
MTRSSM_API int mtrssm_convt_quad(const MtrssmConvGeom* ga4, const float* srca, const uint16_t* const* wqa4, const float* biasa,
                                 const float* actgrada, float* outa, const MtrssmConvGeom* gb4, const float* srcb,
                                 const uint16_t* const* wqb4, const float* biasb, const float* actgradb, float* outb, void* stream) {
  return conv_convt_quad_launch(ga4, srca, reinterpret_cast<const unsigned short* const*>(wqa4), biasa, actgrada, outa, gb4, srcb,
                                reinterpret_cast<const unsigned short* const*>(wqb4), biasb, actgradb, outb,
                                static_cast<hipStream_t>(stream));
}
MTRSSM_API int mtrssm_encoder_stem_supported(const MtrssmEncoderStem* p) { return encoder_stem_supported(p); }
MTRSSM_API int mtrssm_encoder_stem_fwd(const MtrssmEncoderStem* a, const MtrssmEncoderStem* b, void* stream) {
  return encoder_stem_launch(a, b, static_cast<hipStream_t>(stream));
}
MTRSSM_API int mtrssm_convt_k4s2_band_supported(int32_t N, int32_t C, int32_t Hs, int32_t Ws, int32_t Cout) {
  return convt_k4s2_band_supported(N, C, Hs, Ws, Cout);
}
MTRSSM_API int mtrssm_convt_k4s2_band(int32_t N, int32_t C, int32_t Hs, int32_t Ws, int32_t Cout, const float* src, const float* w,
                                     const float* bias, int32_t pre_act, int32_t act, float* out, void* stream) {
  return convt_k4s2_band_launch(N, C, Hs, Ws, Cout, src, w, bias, pre_act, act, out, static_cast<hipStream_t>(stream));
}
MTRSSM_API int mtrssm_convt_k4s2_thin(int32_t N, int32_t C, int32_t Hs, int32_t Ws, int32_t Cout, const float* src, const float* w,
                                      const float* bias, int32_t pre_act, int32_t act, float* out, void* stream) {
  return convt_k4s2_thin_launch(N, C, Hs, Ws, Cout, src, w, bias, pre_act, act, out, static_cast<hipStream_t>(stream));
}

MTRSSM_API int mtrssm_ensemble_score(const float* pred, const float* target, const int32_t* valid, int64_t B, int64_t S, int64_t T, int64_t E,
                                     int32_t act, float* mean, float* ens, float* best, float* spread, float* se_samples, void* stream) {
  return ensemble_score_launch(pred, target, valid, B, S, T, E, act, mean, ens, best, spread, se_samples, static_cast<hipStream_t>(stream));
}
MTRSSM_API int mtrssm_horizon_table(const float* planes, int64_t P, const int32_t* context, const int32_t* valid, int64_t B, int64_t T,
                                    float* sums, float* counts, void* stream) {
  return horizon_table_launch(planes, P, context, valid, B, T, sums, counts, static_cast<hipStream_t>(stream));
}
MTRSSM_API int mtrssm_latent_log_ratio(const float* post_logits, const float* prior_logits, const float* stoch, int64_t rows, int64_t K,
                                       int64_t C, int32_t accumulate, float* out, void* stream) {
  return latent_log_ratio_launch(post_logits, prior_logits, stoch, rows, K, C, accumulate, out, static_cast<hipStream_t>(stream));
}
MTRSSM_API int mtrssm_iw_bound(const float* se_audio, const float* se_vision, const float* log_ratio, const int32_t* valid, int64_t B, int64_t S,
                               int64_t T, int64_t event_audio, int64_t event_vision, float* planes, void* stream) {
  return iw_bound_launch(se_audio, se_vision, log_ratio, valid, B, S, T, event_audio, event_vision, planes, static_cast<hipStream_t>(stream));
}
MTRSSM_API int mtrssm_particle_fold(const float* se_audio, const float* se_vision, const float* log_ratio, const int32_t* valid, const float* u,
                                    int64_t u_stride, int64_t t0, int64_t B, int64_t S, int64_t c, int64_t event_audio, int64_t event_vision,
                                    double threshold, int32_t last_segment, double* carry, float* planes, int32_t* ancestor, void* stream) {
  return particle_fold_launch(se_audio, se_vision, log_ratio, valid, u, u_stride, t0, B, S, c, event_audio, event_vision, threshold, last_segment,
                              carry, planes, ancestor, static_cast<hipStream_t>(stream));
}
MTRSSM_API int mtrssm_particle_gather(const MtrssmStateTable* table, const int32_t* ancestor, int64_t B, int64_t S, int64_t steps, void* stream) {
  return particle_gather_launch(table, ancestor, B, S, steps, static_cast<hipStream_t>(stream));
}
MTRSSM_API int mtrssm_overshoot_gather(const MtrssmStateTable* table, const float* actions, float* windows, int64_t B, int64_t T, int64_t N,
                                       int64_t s, int64_t o, int64_t D, int64_t A, void* stream) {
  return overshoot_gather_launch(table, actions, windows, B, T, N, s, o, D, A, static_cast<hipStream_t>(stream));
}
MTRSSM_API int mtrssm_overshoot_scatter(const MtrssmStateTable* table, int64_t B, int64_t T, int64_t N, int64_t s, int64_t o, void* stream) {
  return overshoot_scatter_launch(table, B, T, N, s, o, static_cast<hipStream_t>(stream));
}
MTRSSM_API int64_t mtrssm_overshoot_kl_workspace_bytes(int64_t b_local, int64_t N, int64_t D) { return overshoot_kl_workspace_bytes(b_local, N, D); }
MTRSSM_API int mtrssm_overshoot_kl_fwd(const float* post_logits, const float* os_logits, const int32_t* valid, int64_t b_global, int64_t row0,
                                       int64_t b_local, int64_t T, int64_t N, int64_t s, int64_t o, int64_t D, int64_t K, int64_t C, float* plane,
                                       double* table, float* count, float* term, void* workspace, int64_t workspace_bytes, void* stream) {
  return overshoot_kl_fwd_launch(post_logits, os_logits, valid, b_global, row0, b_local, T, N, s, o, D, K, C, plane, table, count, term, workspace,
                                 workspace_bytes, static_cast<hipStream_t>(stream));
}
MTRSSM_API int mtrssm_overshoot_kl_bwd(const float* post_logits, const float* os_logits, const int32_t* valid, const float* g_term,
                                       const float* count, int64_t b_global, int64_t row0, int64_t b_local, int64_t T, int64_t N, int64_t s,
                                       int64_t o, int64_t D, int64_t K, int64_t C, float w_prior, float w_post, float* g_os_logits,
                                       float* g_post_logits, void* stream) {
  return overshoot_kl_bwd_launch(post_logits, os_logits, valid, g_term, count, b_global, row0, b_local, T, N, s, o, D, K, C, w_prior, w_post,
                                 g_os_logits, g_post_logits, static_cast<hipStream_t>(stream));
}
MTRSSM_API int64_t mtrssm_latent_census_workspace_bytes(int64_t B, int64_t G, int64_t T, int64_t K, int64_t C) {
  return latent_census_workspace_bytes(B, G, T, K, C);
}
MTRSSM_API int mtrssm_latent_census(const float* post_logits, const float* prior_logits, const float* stoch, const int32_t* valid, int64_t B,
                                    int64_t G, int64_t T, int64_t K, int64_t C, float* planes, double* table, void* workspace,
                                    int64_t workspace_bytes, void* stream) {
  return latent_census_launch(post_logits, prior_logits, stoch, valid, B, G, T, K, C, planes, table, workspace, workspace_bytes,
                              static_cast<hipStream_t>(stream));
}
MTRSSM_API int64_t mtrssm_coherence_fold_workspace_bytes(int64_t B, int64_t G, int64_t S, int64_t T) {
  return coherence_fold_workspace_bytes(B, G, S, T);
}
MTRSSM_API int mtrssm_coherence_fold(const float* logits_v, const float* logits_a, const int32_t* labels, const int32_t* valid, int64_t B, int64_t G,
                                     int64_t S, int64_t T, int64_t context, float* planes, double* table, void* workspace, int64_t workspace_bytes,
                                     void* stream) {
  return coherence_fold_launch(logits_v, logits_a, labels, valid, B, G, S, T, context, planes, table, workspace, workspace_bytes,
                               static_cast<hipStream_t>(stream));
}
MTRSSM_API int64_t mtrssm_feature_moments_workspace_bytes(int64_t N, int D, int J) { return feature_moments_workspace_bytes(N, D, J); }
MTRSSM_API int mtrssm_feature_moments(const float* x, int64_t ldx, const int32_t* bin, int64_t N, int D, int J, double* table, void* workspace,
                                      int64_t workspace_bytes, void* stream) {
  return feature_moments_launch(x, ldx, bin, N, D, J, table, workspace, workspace_bytes, static_cast<hipStream_t>(stream));
}
MTRSSM_API int64_t mtrssm_linear_probe_workspace_bytes(int64_t G, int64_t N, int64_t C, int64_t F) {
  return linear_probe_workspace_bytes(G, N, C, F);
}
MTRSSM_API int mtrssm_linear_probe_step(const float* x, int64_t ld, int64_t col0, const int32_t* labels, const float* weight, const float* bias,
                                        int64_t G, int64_t N, int64_t C, int64_t F, int32_t normalize, float* g_weight, float* g_bias, float* stats,
                                        float* nll, float* hit, int32_t* pred, void* workspace, int64_t workspace_bytes, void* stream) {
  return linear_probe_step_launch(x, ld, col0, labels, weight, bias, G, N, C, F, normalize, g_weight, g_bias, stats, nll, hit, pred, workspace,
                                  workspace_bytes, static_cast<hipStream_t>(stream));
}
MTRSSM_API int64_t mtrssm_episode_panel_bytes(const MtrssmPanelGeom* geom, int32_t* Hc, int32_t* Wc) { return episode_panel_bytes(geom, Hc, Wc); }
MTRSSM_API int mtrssm_episode_panel(const MtrssmPanelGeom* geom, const float* obs_a, const float* post_a, const float* prior_a, const float* obs_v,
                                    const float* post_v, const float* prior_v, const int32_t* codes, const int32_t* valid, const int32_t* context,
                                    uint8_t* out, void* stream) {
  return episode_panel_launch(geom, obs_a, post_a, prior_a, obs_v, post_v, prior_v, codes, valid, context, out, static_cast<hipStream_t>(stream));
}
MTRSSM_API int mtrssm_digit_features(const float* pred, int64_t frames, const int32_t* select, int64_t N, int32_t act, const float* conv1_w,
                                     const float* conv1_b, const float* conv2_w, const float* conv2_b, float* features, void* stream) {
  return digit_features_launch(pred, frames, select, N, act, conv1_w, conv1_b, conv2_w, conv2_b, features, static_cast<hipStream_t>(stream));
}
MTRSSM_API int mtrssm_digit_head(const float* hidden, const float* w, const float* b, int64_t N, const int32_t* select, int64_t frames,
                                 int32_t* digit, float* logits, void* stream) {
  return digit_head_launch(hidden, w, b, N, select, frames, digit, logits, static_cast<hipStream_t>(stream));
}
MTRSSM_API int mtrssm_word_counts(const int32_t* word, const int32_t* digit, int64_t N, float* counts, void* stream) {
  return word_counts_launch(word, digit, N, counts, static_cast<hipStream_t>(stream));
}
MTRSSM_API int mtrssm_digit_features_train(const float* pred, int64_t frames, const int32_t* select, int64_t N, int32_t act, const float* conv1_w,
                                           const float* conv1_b, const float* conv2_w, const float* conv2_b, float* features, uint8_t* tape,
                                           void* stream) {
  return digit_features_train_launch(pred, frames, select, N, act, conv1_w, conv1_b, conv2_w, conv2_b, features, tape, static_cast<hipStream_t>(stream));
}
MTRSSM_API int64_t mtrssm_digit_trunk_bwd_workspace_bytes(int64_t N) { return digit_trunk_bwd_workspace_bytes(N); }
MTRSSM_API int mtrssm_digit_trunk_bwd(const float* pred, int64_t frames, const int32_t* select, int64_t N, int32_t act, const uint8_t* tape,
                                      const float* g_features, const int32_t* labels, const float* conv1_w, const float* conv1_b,
                                      const float* conv2_w, float* g_conv1_w, float* g_conv1_b, float* g_conv2_w, float* g_conv2_b,
                                      int32_t accumulate, void* workspace, int64_t workspace_bytes, void* stream) {
  return digit_trunk_bwd_launch(pred, frames, select, N, act, tape, g_features, labels, conv1_w, conv1_b, conv2_w, g_conv1_w, g_conv1_b, g_conv2_w,
                                g_conv2_b, accumulate, workspace, workspace_bytes, static_cast<hipStream_t>(stream));
}
MTRSSM_API int64_t mtrssm_digit_head_train_workspace_bytes(int64_t N) { return digit_head_train_workspace_bytes(N); }
MTRSSM_API int mtrssm_digit_head_train(const float* hidden, const float* w, const float* b, const int32_t* labels, const int32_t* rows, int64_t N,
                                       int64_t row0, int64_t step, uint32_t key0, uint32_t key1, float p, int32_t normalize, float* nll, int32_t* pred,
                                       float* stats, float* g_hidden, float* g_w, float* g_b, int32_t accumulate, void* workspace,
                                       int64_t workspace_bytes, void* stream) {
  return digit_head_train_launch(hidden, w, b, labels, rows, N, row0, step, key0, key1, p, normalize, nll, pred, stats, g_hidden, g_w, g_b, accumulate,
                                 workspace, workspace_bytes, static_cast<hipStream_t>(stream));
}
