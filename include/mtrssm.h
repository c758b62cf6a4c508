/* mtrssm.h -- C-ABI of libmtrssm_hip.so: MI355X (gfx950) kernels for the MoPoE-M(MT)RSSM
 * sequential-rollout train step.
 *
 * The reference (Mamo1031/Multimodal-MTRSSM) is pure Python and has no FFI of its own; its boundary
 * for this path is the Python class API.  This header is the build-defined C
 * boundary underneath the drop-in Python classes of `multimodal_mtrssm_amd/`: every entry point
 * names the reference code it replaces.
 *
 * Conventions
 *   - plain C: pointers and sizes only, no torch / HIP types.  `stream` is a hipStream_t passed as
 *     void* (NULL = the null stream).  Kernels are launched asynchronously on it.
 *   - all device buffers are caller-owned, fp32, row-major contiguous; sequence tensors are
 *     [B, T, dim] (a row's T steps contiguous).  The library never allocates, frees or keeps
 *     global mutable state and is re-entrant across streams.
 *   - return 0 on success, a negative MTRSSM_E* code otherwise; mtrssm_last_error() gives the
 *     thread-local message.  There is NO CPU fallback.
 *   - S = K*C flat stochastic size, K = category_size (number of categoricals), C = class_size.
 *   - a matrix-vector product with a WIDE output streams its matrix reduction-major (row r of the
 *     buffer = all outputs for input r; threads own outputs, loads coalesce); one with a NARROW
 *     output (the S-wide heads) streams it output-major (one wave per output row).  Hence the
 *     forward scan takes "_t" (= W^T, [in][out]) copies of the wide layers and the PyTorch
 *     [out][in] layout of the narrow ones, and the backward scan the opposite.
 */
#ifndef MTRSSM_H
#define MTRSSM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MTRSSM_VERSION 100 /* 0.1.0 */

#define MTRSSM_OK 0
#define MTRSSM_EINVAL (-1)  /* bad dims / null pointer */
#define MTRSSM_ELAUNCH (-2) /* HIP launch error */
#define MTRSSM_ELDS (-3)    /* dims do not fit the 160 KiB LDS of a CU in this kernel regime */

/* activation ids (torch.nn names the reference YAML uses: Identity, ReLU, ELU, Tanh) */
#define MTRSSM_ACT_IDENTITY 0
#define MTRSSM_ACT_RELU 1
#define MTRSSM_ACT_ELU 2
#define MTRSSM_ACT_TANH 3

int mtrssm_version(void);
const char* mtrssm_last_error(void);
/* name of the device kernel the calling thread's most recent entry-point call launched (as rocprofv3 prints it,
 * without the argument list), e.g. "mtrssm::conv_gather_gemm_patch_kernel<2>": lets a caller key its own HIP-event
 * timings exactly like a kernel trace. */
const char* mtrssm_last_kernel(void);

/* ------------------------------------------------------------------------------------------
 * MoPoE-MRSSM scan.  Replaces the T loop of MoPoE_MRSSM.rollout_representation
 * (mrssm/mopoe_mrssm/core.py:221-256): Transition.forward (networks.py:151-173), the two posterior
 * heads (core.py:62-84), flat log-softmax + PoE + MoE (core.py:241-243, 112-163), State sampling
 * (state.py:17) and the per-step KL term of BaseRSSM.shared_step (core.py:212-216).
 * With post == 0 it is BaseRSSM.rollout_transition (core.py:170-185): prior-only.
 *
 * Contractions that do not depend on the recurrence are hoisted out of the loop by the caller:
 *   xa[b,t,:] = W1[:, :A] a[b,t] + b1          (action part of action_state_projector.0)
 *   pa[b,t,:] = Wa1[:, D:] ea[b,t] + ba1       (embedding part of audio rnn_to_post_projector.0)
 *   pv[b,t,:] = Wv1[:, D:] ev[b,t] + bv1
 * ------------------------------------------------------------------------------------------ */
typedef struct MtrssmMrssmDims {
  int32_t B, T;          /* sequences, timesteps */
  int32_t D, H;          /* deterministic size, hidden (num_cells) */
  int32_t K, C;          /* categoricals, classes */
  int32_t act;           /* MTRSSM_ACT_* of the three MLPs */
  int32_t post;          /* 1: posterior rollout; 0: prior-only rollout */
  float kl_w_post;       /* d(loss)/d(KL) share sent to the posterior (1-alpha with balancing, else 1) */
  float kl_w_prior;      /* share sent to the prior (alpha with balancing, else 1) */
  int32_t rows_per_block; /* 0 = library default */
  int32_t threads;        /* 0 = library default */
  float unimix;           /* eps in [0, 1): every categorical the scan forms (the prior, the posterior after the MoPoE mix) is
                             (1 - eps) * softmax(logits) + eps / C, applied as logits <- log of that before anything reads the
                             logits; 0 = off (no new arithmetic runs).  Outside [0, 1) or NaN: MTRSSM_EINVAL ("unimix") from every
                             scan entry point, before the pointer checks.  The *_supported functions ignore it. */
} MtrssmMrssmDims;

typedef struct MtrssmMrssmFwdWeights {
  const float* w1s_t;  /* [S][H]   action_state_projector.0.weight[:, A:]^T */
  const float* w2_t;   /* [H][H]   action_state_projector.2.weight^T */
  const float* b2;     /* [H] */
  const float* wih_t;  /* [H][3D]  rnn_cell.weight_ih^T (gate order r,z,n) */
  const float* bih;    /* [3D] */
  const float* whh_t;  /* [D][3D]  rnn_cell.weight_hh^T */
  const float* bhh;    /* [3D] */
  const float* wh1_t;  /* [D][3H]  [prior.0.weight ; audio post.0.weight[:, :D] ; vision post.0.weight[:, :D]]^T
                                   (prior-only: [D][H]) */
  const float* b3;     /* [H]      rnn_to_prior_projector.0.bias */
  const float* w4;     /* [S][H]   rnn_to_prior_projector.2.weight (PyTorch layout: narrow output, one wave per row) */
  const float* b4;     /* [S] */
  const float* wa2;    /* [S][H]   audio rnn_to_post_projector.2.weight */
  const float* ba2;    /* [S] */
  const float* wv2;    /* [S][H]   vision rnn_to_post_projector.2.weight */
  const float* bv2;    /* [S] */
} MtrssmMrssmFwdWeights;

typedef struct MtrssmMrssmFwdIO {
  /* inputs */
  const float* xa;      /* [B,T,H] */
  const float* pa;      /* [B,T,H]  (post only) */
  const float* pv;      /* [B,T,H]  (post only) */
  const float* deter0;  /* [B,D] */
  const float* stoch0;  /* [B,S] */
  const float* u_post;  /* [B,T,K] uniforms for the posterior sample (post only) */
  const float* u_prior; /* [B,T,K] uniforms for the prior sample (NULL: not sampled when post=1) */
  /* outputs */
  float* deter;         /* [B,T,D] */
  float* prior_logits;  /* [B,T,S] raw prior logits; with dims.unimix > 0 the log-probabilities of the mixed prior */
  float* prior_stoch;   /* [B,T,S] one-hot prior sample (NULL allowed when post=1) */
  float* post_logits;   /* [B,T,S] MoPoE-mixed log-probs (post only); with dims.unimix > 0 the log-probabilities of the
                           uniform-mixed posterior (a per-categorical softmax of either output gives the distribution the
                           scan sampled from and took the KL of) */
  float* post_stoch;    /* [B,T,S] one-hot posterior sample (post only) */
  float* kl;            /* [B,T]   sum_K KL(q_k || p_k) (post only, NULL allowed) */
  /* activations saved for the backward scan (all NULL = inference) */
  float* sv_h1;         /* [B,T,H]  act(MLP1 layer 0) */
  float* sv_h2;         /* [B,T,H]  MLP1 output */
  float* sv_gates;      /* [B,T,4D] r, z, n, (W_hn h + b_hn) */
  float* sv_heads;      /* [B,T,3H] act of prior / audio / vision head layer 0 */
  float* sv_la;         /* [B,T,S]  audio logits */
  float* sv_lv;         /* [B,T,S]  vision logits */
  const float* expert_logw; /* [B,T,3] log-weights of the (audio, vision, fused) MoPoE experts, taken as given (not normalised);
                               read where both are present; NULL = 1/3 everywhere; needs `modality`; prior-only: ignored */
  const int32_t* modality; /* [B,T] bit0 audio, bit1 vision; NULL = both everywhere */
} MtrssmMrssmFwdIO;

int mtrssm_mrssm_rollout_fwd(const MtrssmMrssmDims* dims, const MtrssmMrssmFwdWeights* w,
                             const MtrssmMrssmFwdIO* io, void* stream);

/* The same forward scan with one batch row on a CLUSTER of four compute units (csrc/mrssm_cluster.hip): every workgroup
 * keeps its quarter of the weights resident in registers / LDS for all T steps and the four exchange D/4 deter values and
 * 3S logit partial sums per step through 8-byte {epoch, value} granules (no weight is re-streamed; 31 -> ~5 us per step at
 * D = H = 200).  Posterior rollout only (post = 1).  The GRU input path is fused by the caller:
 *   wf_t = w2_t . wih_t  ([H][3D] = (W_ih W2)^T),   bf = W_ih b2 + b_ih,
 * so sv_h2 is NOT written (recompute h2 = W2 h1 + b2 as one batched GEMM where dW_ih needs it).
 * workspace: caller-owned device memory of mtrssm_mrssm_cluster_workspace_bytes() bytes, 16-byte aligned; the call zeroes
 * everything but its first 16 bytes.  Its first int32 is a STICKY status word: the caller zeroes it once when allocating; a
 * launch in which a spin gave up stores a non-zero code there (results invalid) and no launch clears it, so one check at any
 * later synchronisation point sees every earlier failure (mtrssm_adamw_apply can be given the word: it then skips the update).
 * The grid is 4 x min(B, 64) workgroups that must be co-resident (one per CU): launch it on a GPU this process has to
 * itself.  mtrssm_mrssm_cluster_supported() says whether the dims AND the current device (CU count >= grid) fit this regime
 * (else use mtrssm_mrssm_rollout_fwd). */
typedef struct MtrssmMrssmClusterWeights {
  const float* w1s_t;  /* [S][H] */
  const float* wf_t;   /* [H][3D]  (W_ih W2)^T */
  const float* bf;     /* [3D]     W_ih b2 + b_ih */
  const float* whh_t;  /* [D][3D] */
  const float* bhh;    /* [3D] */
  const float* wh1_t;  /* [D][3H] */
  const float* b3;     /* [H] */
  const float* w4;     /* [S][H] */
  const float* b4;     /* [S] */
  const float* wa2;    /* [S][H] */
  const float* ba2;    /* [S] */
  const float* wv2;    /* [S][H] */
  const float* bv2;    /* [S] */
} MtrssmMrssmClusterWeights;
int mtrssm_mrssm_cluster_supported(const MtrssmMrssmDims* dims);
int64_t mtrssm_mrssm_cluster_workspace_bytes(const MtrssmMrssmDims* dims);
int mtrssm_mrssm_rollout_fwd_cluster(const MtrssmMrssmDims* dims, const MtrssmMrssmClusterWeights* weights, const MtrssmMrssmFwdIO* io,
                                     void* workspace, int64_t workspace_bytes, void* stream);

typedef struct MtrssmMrssmBwdWeights {
  const float* w1s_t; /* [S][H]  action_state_projector.0.weight[:, A:]^T (same buffer as the forward's) */
  const float* w2;   /* [H][H] */
  const float* wih;  /* [3D][H] */
  const float* whh;  /* [3D][D] */
  const float* wh1;  /* [3H][D]  [prior.0.weight ; audio post.0.weight[:, :D] ; vision post.0.weight[:, :D]] */
  const float* w4;   /* [S][H] */
  const float* wa2;  /* [S][H] */
  const float* wv2;  /* [S][H] */
} MtrssmMrssmBwdWeights;

typedef struct MtrssmMrssmBwdIO {
  /* forward inputs / outputs / saved activations */
  const float* deter0;       /* [B,D] */
  const float* deter;        /* [B,T,D] */
  const float* prior_logits; /* [B,T,S] */
  const float* post_logits;  /* [B,T,S] */
  const float* sv_h1;
  const float* sv_h2;
  const float* sv_gates;
  const float* sv_heads;
  const float* sv_la;
  const float* sv_lv;
  /* incoming gradients (any may be NULL = zero) */
  const float* g_deter;        /* [B,T,D] */
  const float* g_post_stoch;   /* [B,T,S] straight-through */
  const float* g_prior_stoch;  /* [B,T,S] straight-through */
  const float* g_post_logits;  /* [B,T,S] */
  const float* g_prior_logits; /* [B,T,S] */
  const float* g_kl;           /* [B,T] */
  /* outgoing gradients */
  float* g_deter0;  /* [B,D] */
  float* g_stoch0;  /* [B,S] */
  float* d_z1;      /* [B,T,H]  = d xa        (pre-activation of MLP1 layer 0) */
  float* d_h2;      /* [B,T,H]  grad at MLP1 output */
  float* d_gi;      /* [B,T,3D] */
  float* d_gh;      /* [B,T,3D] */
  float* d_zh;      /* [B,T,3H] pre-activation grads of prior / audio / vision head layer 0 (audio = d pa, vision = d pv) */
  float* d_lp;      /* [B,T,S]  grad at prior logits */
  float* d_la;      /* [B,T,S]  grad at audio logits */
  float* d_lv;      /* [B,T,S]  grad at vision logits */
  const float* expert_logw; /* [B,T,3] as in the forward call; NULL = 1/3 everywhere; needs `modality` */
  float* g_expert_logw;     /* [B,T,3] grad at expert_logw, written once per (b, t): exactly 0 where not both are present;
                               NULL = not wanted; needs expert_logw */
  const int32_t* modality; /* [B,T] bit0 audio, bit1 vision; NULL = both everywhere */
} MtrssmMrssmBwdIO;

/* The reverse-time scan on the same four-CU clusters (csrc/mrssm_cluster.hip: mrssm_bwd_cluster_kernel): weights as in
 * MtrssmMrssmClusterWeights (bias fields unused).  io->sv_h2 is not read and io->d_h2 is NOT written (the fused input path
 * has no h2 inside the scan): form d_h2 = d_gi . W_ih afterwards (one GEMM).  Workspace / status word / co-residency as for
 * the forward cluster call; S <= 32. */
int64_t mtrssm_mrssm_cluster_bwd_workspace_bytes(const MtrssmMrssmDims* dims);
int mtrssm_mrssm_rollout_bwd_cluster(const MtrssmMrssmDims* dims, const MtrssmMrssmClusterWeights* weights, const MtrssmMrssmBwdIO* io,
                                     void* workspace, int64_t workspace_bytes, void* stream);

/* The same scans for LARGE deterministic / hidden sizes (D or H >= 256; BASELINE configs[4]: D = H = 1024, S = 128), ALL compute
 * units of the chip on one tile of 32 batch rows (csrc/mrssm_wide.hip): every matrix product of a timestep is cut into
 * 16-column output tiles, each streamed by one CU per step as bf16 pieces in MFMA operand order (packed by the call, once per
 * launch), the batch rows are the MFMA N dimension (v_mfma_f32_16x16x32_bf16), consecutive layers meet through exchange vectors
 * in L2 and a grid-wide barrier (4 per forward timestep, 5 per backward one).  pieces = 3: every fp32 operand as three bf16
 * pieces, six products per k-block (exact to 2^-24: fp32-grade; the default of the Python layer); 2: two pieces, three products
 * (16 significant bits).  Weights / fused input path / sv_h2 / d_h2 exactly as for the cluster calls above.
 * workspace: caller-owned, 256-byte aligned, mtrssm_mrssm_wide_workspace_bytes() / _bwd_workspace_bytes() bytes.  Its first
 * int32 is a STICKY status word: the caller zeroes it once when allocating; a launch whose barrier gave up stores a non-zero
 * code there (results invalid) and no launch ever clears it (mtrssm_adamw_apply can be given the word and then skips the update).
 * The grid is one workgroup per CU, all of which must be resident: a GPU this process has to itself.
 * mtrssm_mrssm_wide_supported() = 1 when dims and device fit (D, H multiples of 16, K <= 64, D/16 + H/16 <= CU count). */
int mtrssm_mrssm_wide_supported(const MtrssmMrssmDims* dims, int32_t pieces);
int64_t mtrssm_mrssm_wide_workspace_bytes(const MtrssmMrssmDims* dims, int32_t pieces);
int64_t mtrssm_mrssm_wide_bwd_workspace_bytes(const MtrssmMrssmDims* dims, int32_t pieces);
int mtrssm_mrssm_rollout_fwd_wide(const MtrssmMrssmDims* dims, const MtrssmMrssmClusterWeights* weights, const MtrssmMrssmFwdIO* io,
                                  int32_t pieces, void* workspace, int64_t workspace_bytes, void* stream);
int mtrssm_mrssm_rollout_bwd_wide(const MtrssmMrssmDims* dims, const MtrssmMrssmClusterWeights* weights, const MtrssmMrssmBwdIO* io,
                                  int32_t pieces, void* workspace, int64_t workspace_bytes, void* stream);

/* Reverse-time scan (BPTT).  Weight gradients are NOT accumulated inside the serial loop: the
 * kernel emits the per-step pre-activation gradients above and the caller forms every dW as one
 * batched [out x B*T] . [B*T x in] library GEMM (rocBLAS), which is where MFMA belongs. */
int mtrssm_mrssm_rollout_bwd(const MtrssmMrssmDims* dims, const MtrssmMrssmBwdWeights* w,
                             const MtrssmMrssmBwdIO* io, void* stream);

/* The initial state of a rollout in one launch each way (csrc/init_state.hip; replaces core.py:121-135 = the mean of the two
 * frame-0 embeddings, init_proj, the prior head, the categorical head -- and their autograd):
 *   e = mean over the present modalities of (ea, ev);  z1 = wi1 e + bi1;  deter0 = wi2 act_i(z1) + bi2;
 *   zp = wp1 deter0 + bp1;  logits = wp2 act_p(zp) + bp2;  (logp, probs, stoch) = the categorical head of
 *   mtrssm_categorical_sample_fwd (same device code) on K categoricals of C classes with the uniforms u.
 * _bwd: from g_deter0 / g_stoch0 / g_logp / g_probs (each may be NULL = zero) it writes the pre-activation gradients d_logits,
 * d_zp, g_deter (= g_deter0 + the head's), d_z1 and the frame-0 embedding gradients g_ea / g_ev (either may be NULL; a row's
 * absent modality gets zeros; _bwd never reads through ea / ev, it only asks whether each is NULL, so any non-NULL pointer
 * with a stride >= E stands for "given").  Weight and bias gradients are GEMMs of these with (e, z1, deter0, zp): the caller's.
 * One workgroup per batch row, no workspace, capturable.  _supported() = 0 for everything the kernels were not written for (an
 * unknown activation id, depth != 1, a layer wider than 1024, more than 2 MB of weights -- every row's workgroup streams them
 * all, which pays only while they are a small L2-resident set): run the layer-by-layer path then. */
typedef struct MtrssmInitialState {
  const float* ea;         /* frame-0 audio embedding rows, row b at ea + b * ea_stride; NULL = absent for every row */
  const float* ev;         /* the same for vision; at least one of the two */
  int64_t ea_stride, ev_stride;
  const uint8_t* mask0;    /* [B][2] (audio, vision) presence at t = 0, NULL = both; read when both embeddings are given */
  const float* u;          /* [B][K] uniforms */
  const float* wi1;        /* [cells][E]  init_proj.0 */
  const float* bi1;
  const float* wi2;        /* [D][cells]  init_proj.2 */
  const float* bi2;
  const float* wp1;        /* [H][D]      rnn_to_prior_projector.0 */
  const float* bp1;
  const float* wp2;        /* [K*C][H]    rnn_to_prior_projector.2 */
  const float* bp2;
  int32_t ld_wi1, ld_wi2, ld_wp1, ld_wp2;   /* floats per weight row */
  int32_t B, E, cells, D, H, K, C, act_i, act_p, depth_i, depth_p;
  float* e;                /* [B][E]      forward outputs (the backward reads z1, zp, probs) */
  float* z1;               /* [B][cells] */
  float* deter0;           /* [B][D] */
  float* zp;               /* [B][H] */
  float* logp;             /* [B][K][C] */
  float* probs;            /* [B][K][C] */
  float* stoch;            /* [B][K*C]    one-hot sample */
  const float* g_deter0;   /* [B][D]      backward inputs */
  const float* g_stoch0;   /* [B][K*C] */
  const float* g_logp;     /* [B][K][C] */
  const float* g_probs;    /* [B][K][C] */
  float* d_logits;         /* [B][K*C]    backward outputs */
  float* d_zp;             /* [B][H] */
  float* g_deter;          /* [B][D] */
  float* d_z1;             /* [B][cells] */
  float* g_ea;             /* [B][E] */
  float* g_ev;             /* [B][E] */
} MtrssmInitialState;
int mtrssm_initial_state_supported(const MtrssmInitialState* p);
int mtrssm_initial_state_fwd(const MtrssmInitialState* p, void* stream);
int mtrssm_initial_state_bwd(const MtrssmInitialState* p, void* stream);

/* The weight layouts of MtrssmMrssmClusterWeights in ONE launch from the raw parameters (csrc/scan_prepare.hip), into one
 * caller-owned buffer `out` of mtrssm_mrssm_scan_prepare_layout() floats:
 *   w1s_t [S][H] = w1[:, A:]^T,  whh_t [D][3D] = whh^T,  wh1_t [D][3H] = [w3 ; wa1[:, :D] ; wv1[:, :D]]^T   (exact copies)
 *   wf_t [H][3D]: wf_t[k][j] = sum_h w2[h][k] wih[j][h],  bf [3D]: bf[j] = sum_h b2[h] wih[j][h] + bih[j]      (product != 0)
 * each sum ONE fp32 fma chain over ascending h starting from zero (bih added last): mtrssm_gemm's arithmetic when it does not
 * split its reduction.  product = 0 leaves wf_t and bf unwritten (the caller forms them with mtrssm_gemm: at large H the
 * MFMA tile kernel is the faster tool); w2, b2, wih, bih may then be NULL.  Every matrix comes with its leading dimension
 * (floats per row): views of a flat parameter buffer need no copy.  Independent tiles, no workspace, capturable. */
typedef struct MtrssmScanPrepare {
  const float* w1;   /* [H][A+S] action_state_projector.0.weight */
  const float* w2;   /* [H][H] */
  const float* b2;   /* [H] */
  const float* wih;  /* [3D][H] */
  const float* bih;  /* [3D] */
  const float* whh;  /* [3D][D] */
  const float* w3;   /* [H][D]   prior head, layer 0 */
  const float* wa1;  /* [H][D+E] audio posterior head, layer 0 (columns [0, D) are read) */
  const float* wv1;  /* [H][D+E] vision posterior head, layer 0 */
  int32_t ld_w1, ld_w2, ld_wih, ld_whh, ld_w3, ld_wa1, ld_wv1;
  int32_t D, H, S, A;
  int32_t product;
  float* out;
  int64_t out_floats;
} MtrssmScanPrepare;
/* Size of `out` in floats (0: bad dims); offsets[5] (may be NULL) receives where w1s_t, whh_t, wh1_t, wf_t, bf start, each a
 * multiple of 64 floats. */
int64_t mtrssm_mrssm_scan_prepare_layout(int32_t D, int32_t H, int32_t S, int64_t* offsets);
int mtrssm_mrssm_scan_prepare(const MtrssmScanPrepare* p, void* stream);

/* ------------------------------------------------------------------------------------------
 * MoPoE-MMTRSSM scan (two-timescale MTState variant).  Replaces the T loop of
 * MoPoE_MMTRSSM.rollout_representation (mmtrssm/mopoe_mmtrssm/core.py:405-490): MTRNN (:59-60),
 * _compute_lower_prior (:263-287), the two posterior heads (:241-261), inline MoPoE (:436-453),
 * _compute_higher_prior_posterior (:289-319), MTState sampling (mmtrssm/state.py:47-49) and the
 * per-step kl / kl_h terms of shared_step (:586-600).  post == 0: rollout_transition (:496-544).
 * Hoisted by the caller:  xl[b,t,:] = Wx_l[:, :A] a[b,t] + bx_l + bd_l ; pa / pv as above.
 * ------------------------------------------------------------------------------------------ */
typedef struct MtrssmMmtrssmDims {
  int32_t B, T;
  int32_t LD, HD;        /* lower / higher deterministic sizes */
  int32_t H;             /* num_cells of l_prior, h_prior, h_posterior and the posterior heads */
  int32_t KL, CL;        /* lower categoricals, classes  (ls = KL*CL) */
  int32_t KH, CH;        /* higher categoricals, classes (hs = KH*CH) */
  int32_t act;
  int32_t post;
  float tau_l, tau_h;    /* MTRNN time constants (> 1) */
  float keep_l, keep_h;  /* (float)(1.0 - 1.0/tau), computed in double by the caller (core.py:59) */
  float kl_w_post, kl_w_prior;
  int32_t rows_per_block;
  int32_t threads;
  float unimix;          /* eps in [0, 1), as MtrssmMrssmDims.unimix: the lower prior, the lower posterior after the mix, the
                            higher prior and the higher posterior (CL resp. CH in the eps / C term); 0 = off */
} MtrssmMmtrssmDims;

typedef struct MtrssmMmtrssmFwdWeights {
  const float* wxl_s_t;  /* [LS+HS][LD]  l_rnn._input2h.weight[:, A:]^T */
  const float* wdl_t;    /* [LD][LD]     l_rnn._d2h.weight^T (bias folded into xl) */
  const float* wxh_t;    /* [HS][HD]     h_rnn._input2h.weight^T */
  const float* wdh_t;    /* [HD][HD]     h_rnn._d2h.weight^T */
  const float* bh;       /* [HD]         h_rnn._input2h.bias + h_rnn._d2h.bias */
  const float* wl1_t;    /* [LD][4H]     [l_prior.0 ; audio post.0[:, :LD] ; vision post.0[:, :LD] ; h_posterior.0[:, :LD]]^T
                                         (prior-only: [LD][H]) */
  const float* bl1;      /* [H]          l_prior.0.bias */
  const float* wh1_t;    /* [HD][2H]     [h_prior.0 ; h_posterior.0[:, LD:]]^T (prior-only: [HD][H]) */
  const float* bh1;      /* [2H]         [h_prior.0.bias ; h_posterior.0.bias] */
  const float* wlp2;     /* [LS][H]  l_prior.2.weight (PyTorch layout) */
  const float* blp2;     /* [LS] */
  const float* wa2;      /* [LS][H]  audio rnn_to_post_projector.2.weight */
  const float* ba2;
  const float* wv2;      /* [LS][H] */
  const float* bv2;
  const float* whp2;     /* [HS][H]  h_prior.2.weight */
  const float* bhp2;
  const float* whq2;     /* [HS][H]  h_posterior.2.weight */
  const float* bhq2;
} MtrssmMmtrssmFwdWeights;

typedef struct MtrssmMmtrssmFwdIO {
  const float* xl;        /* [B,T,LD] */
  const float* pa;        /* [B,T,H] (post only) */
  const float* pv;        /* [B,T,H] (post only) */
  const float* deter_l0;  /* [B,LD] */
  const float* deter_h0;  /* [B,HD] */
  const float* hidden_l0; /* [B,LD] */
  const float* hidden_h0; /* [B,HD] */
  const float* stoch_l0;  /* [B,LS] */
  const float* stoch_h0;  /* [B,HS] */
  const float* u_post_l;  /* [B,T,KL] */
  const float* u_post_h;  /* [B,T,KH] */
  const float* u_prior_l; /* [B,T,KL] (NULL allowed when post=1) */
  const float* u_prior_h; /* [B,T,KH] */
  float* deter_l;         /* [B,T,LD] */
  float* deter_h;         /* [B,T,HD] */
  float* hidden_l;        /* [B,T,LD] */
  float* hidden_h;        /* [B,T,HD] */
  float* prior_logits_l;  /* [B,T,LS] raw; with dims.unimix > 0 all four logits outputs are the log-probabilities of the */
  float* prior_logits_h;  /* [B,T,HS] uniform-mixed distributions, as in MtrssmMrssmFwdIO */
  float* prior_stoch_l;   /* [B,T,LS] (NULL allowed when post=1) */
  float* prior_stoch_h;   /* [B,T,HS] */
  float* post_logits_l;   /* [B,T,LS] mixed log-probs */
  float* post_logits_h;   /* [B,T,HS] raw h_posterior logits */
  float* post_stoch_l;    /* [B,T,LS] */
  float* post_stoch_h;    /* [B,T,HS] */
  float* kl_l;            /* [B,T] */
  float* kl_h;            /* [B,T] */
  float* sv_l1;           /* [B,T,4H] act of l_prior.0 / audio post.0 / vision post.0 / h_posterior.0 */
  float* sv_h1;           /* [B,T,H]  act of h_prior layer 0 */
  float* sv_la;           /* [B,T,LS] */
  float* sv_lv;           /* [B,T,LS] */
  const float* expert_logw; /* [B,T,3] log-weights of the (audio, vision, fused) MoPoE experts, taken as given (not normalised);
                               read where both are present; NULL = 1/3 everywhere; needs `modality`; prior-only: ignored */
  const int32_t* modality; /* [B,T] bit0 audio, bit1 vision; NULL = both everywhere */
} MtrssmMmtrssmFwdIO;

int mtrssm_mmtrssm_rollout_fwd(const MtrssmMmtrssmDims* dims, const MtrssmMmtrssmFwdWeights* w,
                               const MtrssmMmtrssmFwdIO* io, void* stream);

typedef struct MtrssmMmtrssmBwdWeights {
  const float* wxl_s_t; /* [LS+HS][LD] (the forward's buffer: narrow output) */
  const float* wdl;    /* [LD][LD] */
  const float* wxh_t;  /* [HS][HD]    (the forward's buffer: narrow output) */
  const float* wdh;    /* [HD][HD] */
  const float* wl1;    /* [4H][LD] */
  const float* wh1;    /* [2H][HD] */
  const float* wlp2;   /* [LS][H] */
  const float* wa2;    /* [LS][H] */
  const float* wv2;    /* [LS][H] */
  const float* whp2;   /* [HS][H] */
  const float* whq2;   /* [HS][H] */
} MtrssmMmtrssmBwdWeights;

typedef struct MtrssmMmtrssmBwdIO {
  const float* deter_l0;
  const float* deter_h0;
  const float* deter_l;
  const float* deter_h;
  const float* prior_logits_l;
  const float* prior_logits_h;
  const float* post_logits_l;
  const float* post_logits_h;
  const float* sv_l1;
  const float* sv_h1;
  const float* sv_la;
  const float* sv_lv;
  /* incoming gradients (NULL = zero) */
  const float* g_deter_l;
  const float* g_deter_h;
  const float* g_hidden_l;
  const float* g_hidden_h;
  const float* g_post_stoch_l;
  const float* g_post_stoch_h;
  const float* g_prior_stoch_l;
  const float* g_prior_stoch_h;
  const float* g_post_logits_l;
  const float* g_post_logits_h;
  const float* g_prior_logits_l;
  const float* g_prior_logits_h;
  const float* g_kl_l;
  const float* g_kl_h;
  /* outgoing gradients */
  float* g_deter_l0;
  float* g_deter_h0;
  float* g_hidden_l0;
  float* g_hidden_h0;
  float* g_stoch_l0;
  float* g_stoch_h0;
  float* d_ul;    /* [B,T,LD] grad at the lower MTRNN pre-activation sum (already / tau_l) = d xl */
  float* d_uh;    /* [B,T,HD] grad at the higher MTRNN pre-activation sum (already / tau_h) */
  float* d_zl1;   /* [B,T,4H] pre-activation grads: l_prior.0, audio.0 (= d pa), vision.0 (= d pv), h_posterior.0 */
  float* d_zh1;   /* [B,T,H]  pre-activation grad of h_prior.0 */
  float* d_lpl;   /* [B,T,LS] grad at lower prior logits */
  float* d_la;    /* [B,T,LS] */
  float* d_lv;    /* [B,T,LS] */
  float* d_lph;   /* [B,T,HS] grad at higher prior logits */
  float* d_lqh;   /* [B,T,HS] grad at higher posterior logits */
  const float* expert_logw; /* [B,T,3] as in the forward call; NULL = 1/3 everywhere; needs `modality` */
  float* g_expert_logw;     /* [B,T,3] grad at expert_logw, written once per (b, t): exactly 0 where not both are present;
                               NULL = not wanted; needs expert_logw */
  const int32_t* modality; /* [B,T] bit0 audio, bit1 vision; NULL = both everywhere */
} MtrssmMmtrssmBwdIO;

int mtrssm_mmtrssm_rollout_bwd(const MtrssmMmtrssmDims* dims, const MtrssmMmtrssmBwdWeights* w,
                               const MtrssmMmtrssmBwdIO* io, void* stream);

/* The same two scans on ALL compute units (csrc/mmtrssm_wide.hip; regime of mtrssm_mrssm_rollout_*_wide above): up to 64 batch rows
 * per pass as the MFMA N dimension, every product of a timestep cut into 16-column output tiles streamed by one CU each, four grid
 * barriers per timestep in either direction (one-CU form at ld = hd = H = 200: 38 / 46 us per timestep).  Weights, io and results
 * exactly as for mtrssm_mmtrssm_rollout_fwd / _bwd (posterior rollout, post = 1); pieces / workspace / sticky status word /
 * co-residency as for the MRSSM wide calls.  mtrssm_mmtrssm_wide_supported() = 1 when dims and device fit (LD, HD, H multiples of 4,
 * LD or HD >= 128, KL, KH <= 64, (LD + HD + LS + HS) / 16 column tiles <= CU count). */
int mtrssm_mmtrssm_wide_supported(const MtrssmMmtrssmDims* dims, int32_t pieces);
int64_t mtrssm_mmtrssm_wide_workspace_bytes(const MtrssmMmtrssmDims* dims, int32_t pieces);
int64_t mtrssm_mmtrssm_wide_bwd_workspace_bytes(const MtrssmMmtrssmDims* dims, int32_t pieces);
int mtrssm_mmtrssm_rollout_fwd_wide(const MtrssmMmtrssmDims* dims, const MtrssmMmtrssmFwdWeights* w, const MtrssmMmtrssmFwdIO* io,
                                    int32_t pieces, void* workspace, int64_t workspace_bytes, void* stream);
int mtrssm_mmtrssm_rollout_bwd_wide(const MtrssmMmtrssmDims* dims, const MtrssmMmtrssmBwdWeights* w, const MtrssmMmtrssmBwdIO* io,
                                    int32_t pieces, void* workspace, int64_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Conv encoder / decoder kernels (fp32 MFMA implicit GEMM, NCHW).  Replace the layers of the
 * `cnn.Encoder` / `cnn.Decoder` stacks the reference YAML instantiates
 * (mrssm/mopoe_mrssm/configs/default.yaml:31-92; called at mrssm core.py:179-180,215-216,272-273).
 *
 * mtrssm_conv_gather_gemm computes, for every frame n and output channel co,
 *   out[n, co, oy*OS+QY, ox*OS+QX] = (bias[co] + sum_{ty<KH, tx<KW} sum_{c<C+C2} wp[co][ty*KW+tx][c] * pre(S[n,c,sy,sx])) * egrad + add
 *   sy = oy*SS + ty*TS + OFFY, sx = ox*SS + tx*TS + OFFX (zero outside [0,Hs)x[0,Ws)),  oy < Hq, ox < Wq
 * where S = src for c < C and the frame-independent src2 (coordinate channels) for C <= c < C+C2,
 * pre() = act() if pre_act, egrad = act'(actgrad_in[same element as out]) when actgrad_in != NULL, and
 * add = add_in[same element as out] when add_in != NULL (residual skip connection forward; its gradient backward).
 *   Conv2d forward (k,s,p):            KH=KW=k, SS=s, TS=+1, OFF=-p, OS=1, Hq=Ho
 *   Conv2d backward-data / ConvTranspose2d forward: one call per output parity class (qy,qx) in [0,s)^2 with
 *     the taps ky = ky0 + s*ty (ky0 = (qy+p) mod s): SS=1, TS=-1, OFFY=(qy+p-ky0)/s, OS=s, QY=qy.
 * wp is the packed weight matrix [CoutPad][KH*KW][Cpad], zero padded (Cpad % 16 == 0, CoutPad % 32 == 0,
 * CoutPad % 64 == 0 when Cout > 32), 16-byte aligned; wq: its bf16 pieces (see mtrssm_pack_conv_weight), 16-byte aligned, or NULL.
 *
 * mtrssm_conv_weight_grad accumulates (the caller zeroes dwp)
 *   dwp[co][ty*KW+tx][c] += sum_{n, y<Hq, x<Wq} preA(a[n,co,y,x]) * pre(S[n,c,y*SS+ty*TS+OFFY,x*SS+tx*TS+OFFX])
 * with a of shape [N, Cout, Hq, Wq] (geometry must have OS=1, QY=QX=0).  When dbias != NULL (allowed only with
 * pre_act_a == 0) it also accumulates the bias gradient dbias[co] += sum_{n,y,x} a[n,co,y,x] in the same pass.
 * Kernel selection (mfma_split > 0; csrc/conv_split.h): 1x1 layers and 3x3 / stride 1 / pad 1 layers on 8- or 4-pixel-wide
 * planes read both operands straight from HBM into the MFMA register layout (k = pixels is contiguous in NCHW); layers with
 * <= 32 output channels and <= 32 (tap, channel) columns on power-of-two-wide planes run one MFMA tile with a per-lane
 * gathered operand; everything else stages 64-pixel groups through LDS (persistent workgroups); mfma_split = 0 and odd
 * geometries use the fp32 kernels of csrc/conv.hip.  Those accumulate with fp32 atomics: results are equal up to the
 * arrival order of the partial sums.
 * The layer shapes of the reference's default encoders / decoders (mfma_split 1 or 2, pre_act_a as those layers set it: the
 * 3x3 and 1x1 layers of the residual stacks on 64-pixel planes, the three 3x3 / stride-2 convolutions, the three k = 4 /
 * stride-2 transposed convolutions; csrc/conv_wgrad_resident.h) run staged kernels instead: every workgroup stores ONE
 * partial set of its tiles and bias sums into `workspace` -- caller-owned device memory, 256-byte aligned, at least
 * mtrssm_conv_weight_grad_workspace_bytes() bytes, free for reuse as soon as the call's kernels have run (calls on one stream may
 * share one buffer) -- and a second kernel on the same stream adds the sets to dwp / dbias by plain read-modify-write: bitwise
 * reproducible from run to run.  The caller must therefore not accumulate into the same dwp / dbias from ANOTHER stream at the
 * same time (the atomics of the other kernels allow that); calls on one stream are ordered.  With workspace NULL or too small
 * (and with MTRSSM_WGRAD_PARTIALS=0) the same kernels add their tiles by atomics.  The library itself allocates nothing.
 * ------------------------------------------------------------------------------------------ */
typedef struct MtrssmConvGeom {
  int32_t N;                    /* frames (B*T) */
  int32_t C, Hs, Ws;            /* gathered tensor [N, C, Hs, Ws] */
  int32_t C2;                   /* extra frame-independent channels src2 [C2, Hs, Ws] appended after C */
  int32_t Cpad;                 /* channel extent of wp */
  int32_t KH, KW;
  int32_t SS, TS, OFFY, OFFX;
  int32_t Hq, Wq;               /* output sub-grid enumerated by this call */
  int32_t OS, QY, QX;
  int32_t Ho, Wo;               /* full output plane */
  int32_t Cout, CoutPad;
  int32_t pre_act;              /* apply act() to gathered values */
  int32_t act;                  /* MTRSSM_ACT_* */
  int32_t mfma_split;           /* MFMA operand format of the patch-staged kernels: 0 = fp32 (v_mfma_f32_32x32x2_f32, exact);
                                   3 = three bf16 pieces per operand, six v_mfma_f32_32x32x16_bf16 products (fp32-grade, ~2^-24);
                                   1 = plain bf16 operands.  Accumulation is fp32.  Layers the split kernels do not cover
                                   (thin layers, odd geometries) run the fp32 kernels whatever this says. */
} MtrssmConvGeom;

int mtrssm_conv_gather_gemm(const MtrssmConvGeom* g, const float* src, const float* src2, const float* wp, const uint16_t* wq,
                            const float* bias, const float* actgrad_in, const float* add_in, float* out, void* stream);
/* Two independent gather problems (the same layer of the audio and of the vision stack: same channels and taps, different
 * planes) in ONE launch when both map to the same split-bf16 kernel, else two launches: a layer is ~2 rounds of workgroup tiles
 * with a nearly empty last one, two of them back to back in one grid waste one round instead of two.  Arguments as
 * mtrssm_conv_gather_gemm, once per problem. */
int mtrssm_conv_gather_gemm_pair(const MtrssmConvGeom* ga, const float* srca, const float* src2a, const float* wpa, const uint16_t* wqa,
                                 const float* biasa, const float* actgrada, const float* adda, float* outa,
                                 const MtrssmConvGeom* gb, const float* srcb, const float* src2b, const float* wpb, const uint16_t* wqb,
                                 const float* biasb, const float* actgradb, const float* addb, float* outb, void* stream);
/* 1 if mtrssm_conv_gather_gemm_pair would run the two problems as one grid (same split-bf16 kernel for both; has_wq: both
 * have bf16 pieces), 0 if it would fall back to two launches -- a host-side query, nothing is launched. */
int mtrssm_conv_gather_pair_merges(const MtrssmConvGeom* ga, const MtrssmConvGeom* gb, int32_t has_wq);
/* Forward of a whole residual block of the encoders' / decoders' stacks (the builder's `cnn` stand-in, oracle/ref_cnn.py:57-58:
 * `x + conv1(act(conv3(act(x))))`; called through cnn.Encoder / cnn.Decoder at mrssm core.py:179-180,215-216) in ONE launch:
 *   h[n, m, p] = b3[m] + sum_{tap, c} wq3[m][tap][c] * act(x)[n, c, p + tap]          (stored: the backward pass reads it)
 *   y[n, c, p] = x[n, c, p] + b1[c] + sum_m w1[c][m] * act(h[n, m, p])
 * g3 is the 3x3's geometry exactly as mtrssm_conv_gather_gemm takes it (pre_act = 1, mfma_split = 2), wq3 its packed bf16 pieces
 * (mtrssm_pack_conv_weight(s)), w1 [C][Cout] and b1 [C] the 1x1 module's own fp32 parameters (contiguous); two bf16 pieces per
 * operand and fp32 accumulation in both products, as the two separate launches compute.  A second block on another tensor
 * (gb != NULL: the other modality) rides in the same grid.  _supported: 1 when the shape has a fused instance (64 channels,
 * 128 intermediate channels -- or 64 with an even frame count --, 64-pixel planes), else 0 -- a host-side query; mtrssm_residual_block_fwd on an unsupported shape
 * returns MTRSSM_EINVAL. */
int mtrssm_residual_block_fwd_supported(const MtrssmConvGeom* g3);
int mtrssm_residual_block_fwd(const MtrssmConvGeom* ga, const float* xa, const uint16_t* wq3a, const float* b3a, const float* w1a,
                              const float* b1a, float* ha, float* ya, const MtrssmConvGeom* gb, const float* xb, const uint16_t* wq3b,
                              const float* b3b, const float* w1b, const float* b1b, float* hb, float* yb, void* stream);
/* Packs a conv weight view w[O][I][KH][KW] (element strides so, si, sh, sw: any permuted / strided view of the module's
 * parameter, e.g. the per-parity-class tap subset of a ConvTranspose2d weight) into the kernels' layout:
 *   wp fp32 [OPad][KH*KW][IPad], zero padded;
 *   wq (pieces = mfma_split > 0) bf16 bit patterns [pieces][OPad][KH*KW][IPad]: piece s of each wp element, wp = sum_s wq_s
 *   up to 2^-(8 pieces) relative.  mtrssm_conv_gather_gemm reads wq when g->mfma_split > 0 and wq != NULL, wp otherwise
 *   (thin / odd-geometry layers always read wp). */
int mtrssm_pack_conv_weight(const float* w, int32_t O, int32_t I, int32_t KH, int32_t KW, int64_t so, int64_t si, int64_t sh,
                            int64_t sw, int32_t OPad, int32_t IPad, int32_t pieces, float* wp, uint16_t* wq, void* stream);
/* The same for `count` weights in one launch (the train step packs every conv weight once, in both the forward and the
 * backward-data layout, right after the optimizer changed them).  `table` is DEVICE memory: MTRSSM_PACK_DESC_WORDS int64 words
 * per weight = { w, wp, wq (addresses), O, I, KH, KW, so, si, sh, sw, OPad, IPad, pieces, VH, VW } with the meanings above;
 * VH, VW > 0: the view holds only the leading VH x VW taps of the KH x KW tap grid, the rest are packed as zeros (the
 * parity-class sub-kernels of a 3 x 3 kernel run as a zero-padded 4 x 4 transposed convolution); 0, 0: every tap.
 * blocks_per_weight workgroups of 256 threads stride over each weight. */
#define MTRSSM_PACK_DESC_WORDS 16
int mtrssm_pack_conv_weights(const int64_t* table, int32_t count, int32_t blocks_per_weight, void* stream);
int mtrssm_conv_weight_grad(const MtrssmConvGeom* g, const float* a, const float* src, const float* src2,
                            int32_t pre_act_a, float* dwp, float* dbias, void* workspace, int64_t workspace_bytes, void* stream);
/* mtrssm_conv_weight_grad with the sum of its partial tile sets DEFERRED: the main kernel is launched, the small launch that
 * adds the sets into dwp / dbias is recorded for `stream` instead (38 such launches of 6-15 us per train step otherwise).
 * mtrssm_conv_weight_grad_reduce(stream) then runs every recorded sum in one launch.  Contract: the workspace of a deferred
 * call stays untouched -- no other call may be given the same bytes -- and dwp / dbias are not read until the reduce; a
 * second deferred call on the same dwp or workspace first flushes the recorded ones (order is kept).  Kernels without
 * partial sets (general geometry, atomics mode) behave exactly like mtrssm_conv_weight_grad. */
int mtrssm_conv_weight_grad_deferred(const MtrssmConvGeom* g, const float* a, const float* src, const float* src2,
                                     int32_t pre_act_a, float* dwp, float* dbias, void* workspace, int64_t workspace_bytes, void* stream);
int mtrssm_conv_weight_grad_reduce(void* stream);
/* mtrssm_conv_weight_grad of a TRANSPOSED layer (a = the layer input, src = its output gradient) that also accumulates the
 * layer's bias gradient, the per-channel sums of src, in the same pass:
 *   dsrc_bias[c] += sum_{n, y < Hs, x < Ws} src[n, c, y, x]
 * -- the staged kernels of the three k = 4 / stride-2 transposed convolutions (csrc/conv_wgrad_resident.h) load every frame of
 * src exactly once and add it up while they stage it; the sums travel with the workgroup's partial set and the reduce adds
 * them to dsrc_bias (run-to-run deterministic; with workspace NULL or too small: fp32 atomics).  A separate
 * mtrssm_channel_sum re-reads the whole output gradient.  defer != 0: the partial-set sum is recorded as by
 * mtrssm_conv_weight_grad_deferred.  _supported: 1 when the kernel mtrssm_conv_weight_grad picks for (g, pre_act_a) is one of
 * those three, else 0 -- a host-side query; mtrssm_conv_weight_grad_src_bias on another geometry returns MTRSSM_EINVAL (use
 * mtrssm_conv_weight_grad + mtrssm_channel_sum there). */
int mtrssm_conv_weight_grad_src_bias_supported(const MtrssmConvGeom* g, int32_t pre_act_a);
/* The whole backward of a residual block's 1x1 layer (y = x + W1 act(h) + b1) in ONE pass over g_y and h:
 *   gh[n, m, p]  = (sum_o W1[o][m] * gy[n, o, p]) * act'(h[n, m, p])          (written)
 *   dwp[o][m]   += sum_{n, p} gy[n, o, p] * act(h[n, m, p])                    (as mtrssm_conv_weight_grad: partial sets + reduce)
 *   dbias[o]    += sum_{n, p} gy[n, o, p]                                      (dbias may be NULL)
 * g is the layer's geometry exactly as mtrssm_conv_weight_grad takes it (C = the 128 or 64 mid channels, Cout = 64, 64-pixel
 * planes, KH = KW = 1, pre_act = 1, mfma_split = 2); wq1t the two bf16 pieces of W1 transposed, [2][C][64], as
 * mtrssm_pack_conv_weight(s) packs the permuted view for the backward-data gather.  Same arithmetic, product order and partial
 * sets as mtrssm_conv_gather_gemm (backward-data) followed by mtrssm_conv_weight_grad: gh, dwp and dbias come out bit-identical
 * to theirs; both tensors are read once instead of twice.  workspace: mtrssm_conv_weight_grad_workspace_bytes(g, 0) bytes
 * (NULL / too small: atomics); defer != 0 records the partial-set sum as mtrssm_conv_weight_grad_deferred does.  _supported:
 * 1 / 0, a host-side query; mtrssm_residual_bwd1x1 on an unsupported shape returns MTRSSM_EINVAL. */
int mtrssm_residual_bwd1x1_supported(const MtrssmConvGeom* g);
int mtrssm_residual_bwd1x1(const MtrssmConvGeom* g, const float* gy, const float* h, const uint16_t* wq1t, float* gh, float* dwp,
                           float* dbias, void* workspace, int64_t workspace_bytes, int32_t defer, void* stream);
/* mtrssm_residual_bwd1x1 for TWO blocks with the same mid width C (the audio and the vision stack's block; frame counts and
 * plane shapes may differ) in ONE grid of one workgroup per CU, half of them for each problem.  Every argument as in the single
 * call, once per problem; each problem has its own workspace (mtrssm_conv_weight_grad_workspace_bytes of ITS geometry is enough:
 * a paired call leaves at most as many partial sets per problem as the single call) and its own reduce (defer != 0: two
 * recorded sums).  gh is bit-identical to the single call's; dwp / dbias are sums over half as many partial sets, so they
 * agree within rounding.  A problem whose workspace is NULL / too small adds by fp32 atomics.  _supported: 1 / 0, a host-side
 * query (0 for every shape with MTRSSM_PAIR_WGRAD=0 in the environment); the call on an unsupported pair returns MTRSSM_EINVAL. */
int mtrssm_residual_bwd1x1_pair_supported(const MtrssmConvGeom* ga, const MtrssmConvGeom* gb);
int mtrssm_residual_bwd1x1_pair(const MtrssmConvGeom* ga, const float* gya, const float* ha, const uint16_t* wq1ta, float* gha, float* dwpa,
                                float* dbiasa, void* workspace_a, int64_t workspace_a_bytes, const MtrssmConvGeom* gb, const float* gyb,
                                const float* hb, const uint16_t* wq1tb, float* ghb, float* dwpb, float* dbiasb, void* workspace_b,
                                int64_t workspace_b_bytes, int32_t defer, void* stream);
/* mtrssm_conv_weight_grad (pre_act_a = 0, no src2) for TWO 3x3 / stride-1 layers of the residual stacks in ONE grid: the same
 * layer (C = 64 or 32, Cout, activation, mfma_split = 2) on a 4-wide and on an 8-wide 64-pixel plane, in either order; the
 * frame counts may differ.  One wave per SIMD over the chip in total, half of the x blocks for each problem, so a workgroup's
 * run of frames is twice as long as in two launches and each problem leaves half as many partial sets.  Workspaces, reduce
 * jobs, defer and the atomics form: per problem, as in mtrssm_residual_bwd1x1_pair.  _supported: 1 / 0, a host-side query (0
 * with MTRSSM_PAIR_WGRAD=0); the call on an unsupported pair returns MTRSSM_EINVAL. */
int mtrssm_conv_weight_grad_pair_supported(const MtrssmConvGeom* ga, const MtrssmConvGeom* gb);
int mtrssm_conv_weight_grad_pair(const MtrssmConvGeom* ga, const float* aa, const float* srca, float* dwpa, float* dbiasa, void* workspace_a,
                                 int64_t workspace_a_bytes, const MtrssmConvGeom* gb, const float* ab, const float* srcb, float* dwpb,
                                 float* dbiasb, void* workspace_b, int64_t workspace_b_bytes, int32_t defer, void* stream);
int mtrssm_conv_weight_grad_src_bias(const MtrssmConvGeom* g, const float* a, const float* src, int32_t pre_act_a, float* dwp,
                                     float* dsrc_bias, void* workspace, int64_t workspace_bytes, int32_t defer, void* stream);
/* Bytes of workspace the kernel chosen for this geometry wants for its partial tile sets (0: none; -1: invalid geometry; up to
 * ~38 MB for the reference's layer shapes at B*T = 3200 frames).  A host-side query, nothing is launched. */
int64_t mtrssm_conv_weight_grad_workspace_bytes(const MtrssmConvGeom* g, int32_t pre_act_a);
/* End of backward: add every packed conv weight gradient [OPad][taps][IPad] of the step into its parameter-layout target
 * [O][I][KH][KW] (a view of the flat gradient buffer) and clear the packed buffers, in ONE launch.  table (device memory):
 * `count` rows of 8 int64 = { packed pointer, target pointer, O, I, taps = KH*KW, IPad, 0, 0 }. */
int mtrssm_unpack_conv_grads(const int64_t* table, int32_t count, int32_t blocks_per_entry, void* stream);
/* Decoder ConvTranspose2d (k = 4, s = 2, p = 1; default.yaml:61-92) forward, ALL FOUR output parity classes in one pass over the
 * source (mtrssm_conv_gather_gemm takes one launch per class: each re-reads the source).  g4[q], wq4[q]: geometry and packed
 * sub-kernel (mtrssm_pack_conv_weight(s), two bf16 pieces) of class q = 2 * QY + QX exactly as for mtrssm_conv_gather_gemm
 * (KH = KW = 2, TS = -1, SS = 1, OS = 2, same source / output).  Optionally a second tensor (gb4 != NULL: the other modality) in
 * the same launch.  actgrad (may be NULL): out *= act'(actgrad[same index]) -- the backward-data of a Conv2d(k = 3, s = 2, p = 1)
 * is this transposed conv with the kernel zero-padded to 4 x 4 (the encoders' third conv).
 * mtrssm_convt_quad_supported: 1 / 2 = the instantiated forward shapes (64 -> 32 on 64-pixel planes, 32 -> 16 on 256-pixel planes),
 * 3 = 32 -> 16 on 64-pixel planes WITH actgrad, 4 = 16 -> 8 on 256-pixel planes WITH actgrad; 0 = use the general path.
 * Kernel selection inside: shapes 1 and 3 run one wave per parity class (csrc/conv_resident.h: convt_quad_resident_kernel),
 * shapes 2 and 4 the classes as rows of the MFMA tile (csrc/conv_s2_band.h: convt4s2_rows_kernel); same arithmetic (two bf16
 * pieces per operand, fp32 accumulation), another summation order. */
int mtrssm_convt_quad_supported(const MtrssmConvGeom* g4);
int mtrssm_convt_quad(const MtrssmConvGeom* ga4, const float* srca, const uint16_t* const* wqa4, const float* biasa, const float* actgrada,
                      float* outa, const MtrssmConvGeom* gb4, const float* srcb, const uint16_t* const* wqb4, const float* biasb,
                      const float* actgradb, float* outb, void* stream);
/* Last decoder layer (default.yaml:70-74, channels [.., 1]): out[N, Cout<=2, 2Hs, 2Ws] = bias + ConvTranspose2d_{k=4,s=2,p=1}(pre(src[N,C,Hs,Ws]))
 * with w in the ConvTranspose2d layout [C][Cout][4][4].  All four output parity classes in one pass, one activation per
 * source element. */
int mtrssm_convt_k4s2_thin(int32_t N, int32_t C, int32_t Hs, int32_t Ws, int32_t Cout, const float* src, const float* w,
                           const float* bias, int32_t pre_act, int32_t act, float* out, void* stream);
/* The same layer on the MFMA for the reference's shapes (16 input channels, Cout <= 2, frames of 1024 positions: 64 x 16 or
 * 32 x 32; two bf16 pieces per operand, fp32 accumulation = the bf16x2 conv mode): the four output parity classes of an input
 * position are rows of an MFMA tile, a frame is staged once (csrc/conv_s2_band.h: convt4s2_band_kernel).  _supported: 1 / 0, a
 * host-side query. */
int mtrssm_convt_k4s2_band_supported(int32_t N, int32_t C, int32_t Hs, int32_t Ws, int32_t Cout);
int mtrssm_convt_k4s2_band(int32_t N, int32_t C, int32_t Hs, int32_t Ws, int32_t Cout, const float* src, const float* w,
                           const float* bias, int32_t pre_act, int32_t act, float* out, void* stream);
/* The encoders' strided stem (default.yaml:31-60) in ONE launch: three Conv2d(k = 3, s = 2, p = 1) layers with channels
 * (frame + 2 coordinate planes) -> 8 -> 16 -> 32 and the activation between them,
 *   y1 = b1 + Conv(src ++ coords),  y2 = b2 + Conv(act(y1)),  y3 = b3 + Conv(act(y2)),
 * one pass per frame: the frame is read once, y1 / y2 / y3 are written once (the backward pass reads all three), the activated
 * bf16 pieces of y1 and y2 stay on the chip (csrc/conv_stem.h: encoder_stem_kernel).  Arithmetic of the bf16x2 conv mode (two
 * bf16 pieces per operand, three products, fp32 accumulation); the coordinate planes' contribution is formed once per
 * workgroup in fp32.  y2 is bit-identical to mtrssm_conv_gather_gemm's on the same y1; y1 and y3 sum in another order.
 * wp1 / wq1, wq2, wq3: the layers' packed weights (mtrssm_pack_conv_weight(s): OPad = 32, IPad = 16, two pieces); biases may be
 * NULL; every tensor contiguous and 16-byte aligned.  A second problem (b != NULL: the other modality, its own plane shape and
 * frame count) rides in the same grid.
 * mtrssm_encoder_stem_supported: 1 / 0, a host-side query of the SHAPE fields only (mfma_split == 2, C == 1, C2 == 2,
 * Cout1..3 == 8, 16, 32, Hs x Ws == 64 x 64 or 128 x 32, act Identity / ReLU / ELU, N * 8192 < 2^31); mtrssm_encoder_stem_fwd on
 * anything else returns MTRSSM_EINVAL and the caller keeps the per-layer path. */
typedef struct MtrssmEncoderStem {
  const float* src;    /* [N][1][Hs][Ws] */
  const float* coords; /* [2][Hs][Ws] */
  const float* wp1;
  const uint16_t* wq1;
  const float* bias1;
  const uint16_t* wq2;
  const float* bias2;
  const uint16_t* wq3;
  const float* bias3;
  float* y1; /* [N][8][Hs/2][Ws/2] */
  float* y2; /* [N][16][Hs/4][Ws/4] */
  float* y3; /* [N][32][Hs/8][Ws/8] */
  int32_t N, C, C2, Hs, Ws, Cout1, Cout2, Cout3, act, mfma_split;
} MtrssmEncoderStem;
int mtrssm_encoder_stem_supported(const MtrssmEncoderStem* p);
int mtrssm_encoder_stem_fwd(const MtrssmEncoderStem* a, const MtrssmEncoderStem* b, void* stream);
/* Conv2d backward-data / ConvTranspose2d forward with <= 8 output channels, all output parity classes in ONE pass (the general
 * path, mtrssm_conv_gather_gemm, takes one launch per parity class of a strided layer; replaces the backward-data of the
 * encoders' second conv, cnn.Encoder at mrssm core.py:179-180):
 *   out[n, c, iy, ix] = (bias[c] + sum_{o, ky, kx} w[o][c][ky][kx] * pre(y)[n, o, (iy + pad - ky) / stride, (ix + pad - kx) / stride])
 *                       * act'(actgrad_in[n, c, iy, ix]) + add_in[n, c, iy, ix]
 * over the taps whose (iy + pad - ky), (ix + pad - kx) are non-negative multiples of the stride inside the source plane.
 * y [N, O, Hs, Ws], w [O][Cout][KH][KW] contiguous (the Conv2d weight), out [N, Cout, Ho, Wo]; KH * KW * O <= 256; stride 2, even Ho and Wo. */
int mtrssm_conv_tgather_thin(int32_t N, int32_t O, int32_t Hs, int32_t Ws, int32_t Cout, int32_t KH, int32_t KW, int32_t stride, int32_t pad,
                             int32_t Ho, int32_t Wo, const float* y, const float* w, const float* bias, int32_t pre_act, int32_t act,
                             const float* actgrad_in, const float* add_in, float* out, void* stream);
/* out[c] += sum_{n, i<HW} x[n, c, i]   (bias gradients; the caller zeroes out) */
int mtrssm_channel_sum(const float* x, int32_t N, int32_t C, int32_t HW, float* out, void* stream);

/* ------------------------------------------------------------------------------------------
 * Episode feed.  Replaces EpisodeDataset.__getitem__ + the default collate of the 6-tuple
 * StackDataset (models/dataset.py:84-112, models/mrssm/dataset.py:155-183) for the YAML's transform chains
 * TakeFirstN(n) [+ GaussianNoise(std)] (models/transform.py:31-72, default.yaml:176-220): from the HBM-resident store
 * [n_episodes, Tfull, E] (fp32, already preprocessed) it writes, for the B episodes idx[0..B) (int64, device memory),
 *   target[b, t, :] = store[idx[b], t, :]                t < T <= Tfull
 *   input [b, t, :] = target[b, t, :] + noise[b, t, :] * std     (mul then add, each rounded: bitwise torch's expression)
 * noise (caller-drawn standard normals [B, T, E]) may be NULL (input = target); input or target may be NULL.
 * E % 4 == 0; every buffer 16-byte aligned.  idx values are NOT range-checked on the device.
 * ------------------------------------------------------------------------------------------ */
int mtrssm_episode_gather(const float* store, const int64_t* idx, const float* noise, int64_t n_episodes, int64_t B, int64_t T,
                          int64_t Tfull, int64_t E, float std_, float* input, float* target, void* stream);
/* The same pair from a WINDOW of each episode (replaces the TakeFirstN of the chain by a slice
 * [start, start + T), which the reference cannot express: it trains on the first T frames only):
 *   target[b, t, :] = store[idx[b], start[b] + t, :]          input = target + noise * std as above (same two roundings)
 * start: [B] int32 in DEVICE memory, read by the kernel, so that a captured graph replays with new windows and no host round
 * trip.  The launcher therefore cannot range-check the starts: the kernel clamps start[b] into [0, Tfull - T], and the
 * caller validates them where it makes them (dataset.DeviceEpisodeLoader draws them on the host).  start == NULL returns -1
 * (mtrssm_episode_gather is the entry for the first T frames); everything else as mtrssm_episode_gather. */
int mtrssm_episode_gather_window(const float* store, const int64_t* idx, const int32_t* start, const float* noise, int64_t n_episodes,
                                 int64_t B, int64_t T, int64_t Tfull, int64_t E, float std_, float* input, float* target, void* stream);
/* The window gather for episodes of different lengths: lengths [n_episodes] int32 in DEVICE memory,
 *   target[b, t, :] = (start[b] + t < lengths[idx[b]]) ? store[idx[b], start[b] + t, :] : 0
 *   input = target + noise * std (the same two roundings) on a live frame, exactly 0 on a dead one; a dead frame issues no load.
 * start[b] is clamped into [0, Tfull] -- a chunk may hang over the end of the store, the length test keeps every read inside
 * it --, lengths into [0, Tfull], idx[b] into [0, n_episodes).  valid_out (int32 [B], may be NULL) receives
 * clamp(lengths[idx[b]] - start[b], 0, T), the live steps of row b.  A null start or lengths returns -1; everything else as
 * mtrssm_episode_gather_window. */
int mtrssm_episode_gather_ragged(const float* store, const int64_t* idx, const int32_t* start, const int32_t* lengths, const float* noise,
                                 int64_t n_episodes, int64_t B, int64_t T, int64_t Tfull, int64_t E, float std_, float* input, float* target,
                                 int32_t* valid_out, void* stream);
/* The three gathers above with the standard normals GENERATED in the kernel instead of read from `noise`:
 * start == NULL: the first T frames (mtrssm_episode_gather); start alone: windows, start[b] clamped into [0, Tfull - T]
 * (mtrssm_episode_gather_window); start and lengths: ragged, clamps, zeros on dead frames and valid_out (may be NULL) as
 * mtrssm_episode_gather_ragged.  target is bitwise what those entries write; input = target + z * std, mul then add, each rounded.
 * z is a pure function of (key, epoch, episode, absolute frame, element), independent of the batch row, B and the window start.
 * For the four elements 4 e4 .. 4 e4 + 3 of frame f = clamped start[b] + t (f = t without start) of episode idx[b]:
 *   x[0..3] = Philox4x32-10(counter = (e4, f, idx[b] & 0xffffffff, epoch), key = (key0, key1))
 *             (Salmon et al., SC'11: multipliers 0xD2511F53 on counter word 0 and 0xCD9E8D57 on word 2, the key advancing by
 *             0x9E3779B9, 0xBB67AE85 between the ten rounds; Random123's philox4x32_R(10, ...))
 *   pair (x0, x1) -> z[4 e4], z[4 e4 + 1]; pair (x2, x3) -> z[4 e4 + 2], z[4 e4 + 3]; for a pair (xa, xb), in fp32:
 *     u1 = ((xa >> 8) + 1) * 2^-24 in (0, 1]    u2 = (xb >> 8) * 2^-24 in [0, 1)    r = sqrt(-2 log(u1))
 *     z_first = r * cos(2 pi u2)                z_second = r * sin(2 pi u2)
 * (log, sqrt, sincospi are the accurate device functions: a second implementation agrees to a few ulp, not bitwise.)
 * dataset.stream_key gives the loader's keys: key0 = seed & 0xffffffff, key1 = (seed >> 32) ^ (0x9E3779B9 * (stream + 1) mod 2^32),
 * stream = 0, 1, 2 for action, audio, vision; epoch = the loader's epoch counter (0 for a fixed stream).
 * lengths without start, valid_out without lengths, E % 4 != 0, E / 4 >= 2^32 or a misaligned buffer return -1; a dead frame
 * issues no load and no generator work. */
int mtrssm_episode_gather_seeded(const float* store, const int64_t* idx, const int32_t* start, const int32_t* lengths, int32_t* valid_out,
                                 uint32_t key0, uint32_t key1, uint32_t epoch, int64_t n_episodes, int64_t B, int64_t T, int64_t Tfull,
                                 int64_t E, float std_, float* input, float* target, void* stream);
/* The seeded gather with a seeded AUGMENTATION of the frames: one integer shift per episode and up to
 * MTRSSM_AUGMENT_MAX_BANDS (row band, column band) masks per frame or per episode, then the seeded noise.  The event is [C, H, W],
 * E = C H W.  Everything below is exact 32-bit integer arithmetic, umulhi(a, n) = (a * n) >> 32 for a 32-bit a; Philox4x32-10, the
 * absolute frame f, the form selection by start / lengths, the clamps of start, lengths and idx, the dead frames (exactly zero, no
 * load, no generator work) and valid_out are those of mtrssm_episode_gather_seeded.  (akey0, akey1) is the augmentation's key:
 * dataset.augment_key(seed, stream) = stream_key(seed, stream + 3), apart from the noise keys of streams 0, 1, 2.
 *   shift, one draw per (key, epoch, episode), the same for every frame of the episode:
 *     P = Philox4x32-10(counter = (0, 0, idx[b] & 0xffffffff, epoch), key = (akey0, akey1))
 *     dy = umulhi(P0, 2 sy + 1) - sy    dx = umulhi(P1, 2 sx + 1) - sx     (positive: content moves down / right)
 *   band j = 0 .. bands - 1:
 *     Q = Philox4x32-10(counter = (1 + j, per_frame ? f + 1 : 0, idx[b] & 0xffffffff, epoch), key = (akey0, akey1))
 *     h = umulhi(Q0, max_rows + 1)   r0 = umulhi(Q1, H - h + 1)   w = umulhi(Q2, max_cols + 1)   c0 = umulhi(Q3, W - w + 1)
 *     pixel (y, x) of every channel is masked iff, for some j, r0 <= y < r0 + h or c0 <= x < c0 + w   (output coordinates)
 *   live frame, channel c, pixel (y, x), output element e = (c H + y) W + x:
 *     target = (0 <= y - dy < H and 0 <= x - dx < W) ? store[idx[b], f, c, y - dy, x - dx] : fill    (shifted, never masked)
 *     base   = masked(y, x) ? fill : target
 *     input  = noisy ? base + z * std : base      (mul then add, each rounded; z = the seeded entry's normal of (key0, key1), epoch,
 *                                                  episode, f and OUTPUT element e)
 * A vacated pixel reads nothing.  With sy = sx = bands = 0 the call writes what mtrssm_episode_gather_seeded writes (noisy = 1), bit
 * for bit.  Returns -1 without a launch for: a null aug; sy outside [0, H), sx outside [0, W); bands outside
 * [0, MTRSSM_AUGMENT_MAX_BANDS]; max_rows outside [0, H], max_cols outside [0, W]; per_frame or noisy outside {0, 1}; a fill that is
 * not finite; C, H, W <= 0, W % 4 != 0, C H W >= 2^31 or B T >= 2^31 (one workgroup per frame); and whatever
 * mtrssm_episode_gather_seeded refuses. */
#define MTRSSM_AUGMENT_MAX_BANDS 4
typedef struct MtrssmFeedAugment {
  int32_t sy, sx, bands, max_rows, max_cols, per_frame;
  float fill;
} MtrssmFeedAugment;
int mtrssm_episode_gather_augmented(const MtrssmFeedAugment* aug, const float* store, const int64_t* idx, const int32_t* start,
                                    const int32_t* lengths, int32_t* valid_out, uint32_t key0, uint32_t key1, uint32_t akey0, uint32_t akey1,
                                    uint32_t epoch, int64_t n_episodes, int64_t B, int64_t T, int64_t Tfull, int64_t C, int64_t H, int64_t W,
                                    int32_t noisy, float std_, float* input, float* target, void* stream);

/* ------------------------------------------------------------------------------------------
 * Carried state of truncated BPTT: the initial state of a train step is, per batch row, either the
 * fresh one (core.py:121-135: the chunk's own frame 0 -> init_proj -> prior head) or the posterior the previous chunk ended
 * with.  Both calls are ONE launch over a table of up to MTRSSM_STATE_MAX row-major fp32 tensors [B, width[k]]
 * (MRSSM: deter, stoch; MMTRSSM: deter_l, deter_h, stoch_l, stoch_h, hidden_l, hidden_h), the table passed to the kernel by value.
 *
 * mtrssm_state_select: dst[k][b, :] = reset[b] ? src[k][b * src_stride[k] : + width[k]] : alt[k][b, :]
 *   reset: [B] bytes in {0, 1} in DEVICE memory (read by the kernel: the launch sequence is the same whether a row starts an
 *   episode or continues one, so one captured graph serves every chunk).  src = the fresh state, its rows src_stride[k] >= width[k]
 *   floats apart (a column slice of init_proj's output needs no copy); alt = the carry, contiguous; alt[k] == NULL stands for
 *   zeros: the backward of the select is this call with src = the incoming gradient, g_fresh[b] = reset[b] ? g[b] : 0 (the
 *   carry never receives a gradient).  Replaces nothing upstream: the reference cannot continue a sequence.
 * mtrssm_state_save: dst[k][b, :] = src[k][b, steps - 1, :], src = an output [B, steps, width[k]] of the scan, read in place
 *   (no [:, -1].contiguous() copies); src_stride and alt are ignored.
 * Entries whose width, stride and pointers are multiples of 4 floats / 16 bytes move 16 bytes per lane, the others 4.
 * A null table, reset, src or dst, count outside 1 .. MTRSSM_STATE_MAX, non-positive B / steps / width, a stride below the
 * width or a pointer that is not 4-byte aligned return -1 without a launch.
 * ------------------------------------------------------------------------------------------ */
#define MTRSSM_STATE_MAX 6
typedef struct MtrssmStateTable {
  int32_t count;
  int32_t width[MTRSSM_STATE_MAX];
  int64_t src_stride[MTRSSM_STATE_MAX];
  const float* src[MTRSSM_STATE_MAX];
  const float* alt[MTRSSM_STATE_MAX];
  float* dst[MTRSSM_STATE_MAX];
} MtrssmStateTable;
int mtrssm_state_select(const MtrssmStateTable* table, const uint8_t* reset, int64_t B, void* stream);
int mtrssm_state_save(const MtrssmStateTable* table, int64_t B, int64_t steps, void* stream);
/* mtrssm_state_save at a per-row step (ragged batches): last [B] int32 in DEVICE memory,
 *   dst[k][b, :] = src[k][b, last[b], :] when 0 <= last[b] < steps; otherwise dst[k][b, :] is left as it is (a row with no live
 *   step keeps its carry).  Same lanes and argument rules as mtrssm_state_save; a null or misaligned `last` returns -1. */
int mtrssm_state_save_at(const MtrssmStateTable* table, const int32_t* last, int64_t B, int64_t steps, void* stream);

/* The scalar end of shared_step (core.py:187-221; mmtrssm core.py:563-606) in one launch each way:
 *   recon = nll_a + nll_v;  kl_j = c_j * mean_i kl_j[i], i < n (kl1 may be NULL);  loss = recon + kl_0 + kl_1, written to four scalars (o_k1 may be NULL).
 * bwd: scalar gradients of those four (each may be NULL = 0) -> g_nll_a = g_nll_v = g_recon + g_loss, g_kl_j[i] = (g_kl_j + g_loss) c_j / n. */
int mtrssm_elbo_combine_fwd(const float* nll_a, const float* nll_v, const float* kl0, const float* kl1, int64_t n, float c0, float c1,
                            float* o_recon, float* o_k0, float* o_k1, float* o_loss, void* stream);
int mtrssm_elbo_combine_bwd(const float* g_recon, const float* g_k0, const float* g_k1, const float* g_loss, int64_t n, float c0, float c1,
                            float* g_nll_a, float* g_nll_v, float* g_kl0, float* g_kl1, void* stream);
/* The same epilogue for ragged batches: live [n] in {0, 1}, count a device scalar (float),
 *   kl_j = c_j * sum_i live[i] kl_j[i] / count   (0 when count = 0);   bwd: g_kl_j[i] = live[i] (g_kl_j + g_loss) c_j / count.
 * Same reduction order as mtrssm_elbo_combine_fwd: with every step live and count = n the four scalars are bitwise its. */
int mtrssm_elbo_combine_counted_fwd(const float* nll_a, const float* nll_v, const float* kl0, const float* kl1, const float* live,
                                    const float* count, int64_t n, float c0, float c1, float* o_recon, float* o_k0, float* o_k1,
                                    float* o_loss, void* stream);
int mtrssm_elbo_combine_counted_bwd(const float* g_recon, const float* g_k0, const float* g_k1, const float* g_loss, const float* live,
                                    const float* count, int64_t n, float c0, float c1, float* g_nll_a, float* g_nll_v, float* g_kl0,
                                    float* g_kl1, void* stream);
/* The same epilogue under an ElboSchedule: KL free bits per (b, t), a beta warm-up read from a device
 * scalar, per-modality reconstruction weights.  One pair serves live / count NULL (every step live, N = n) or given (N = *count)
 * and kl1 NULL or given.  Every operation is a separately rounded fp32 operation (no fused multiply-add):
 *   beta   = 1 when warmup = 0, else beta_start + (1 - beta_start) * min(*step / warmup, 1)   (step: device scalar, the optimizer
 *            steps taken so far; it may be NULL only when warmup = 0, otherwise -1)
 *   recon  = w_a nll_a + w_v nll_v;   clip_j[i] = kl_j[i] < free_j ? free_j : kl_j[i]   (a NaN stays a NaN)
 *   k_j    = sum_live clip_j[i] / N * c_j * beta   (0 when N <= 0);   loss = recon + k_0 + k_1
 *   stats  = { raw0, raw1, active0, active1 }: raw_j = sum_live kl_j[i] / N * c_j (the unscheduled term),
 *            active_j = #{live i : not kl_j[i] < free_j} / N;  raw1 = active1 = 0 without kl1.
 * fwd writes recon, k0, k1 (o_k1 may be NULL), loss, beta and the four stats.  bwd reads the STORED beta, never step:
 *   g_nll_a = w_a (g_recon + g_loss), g_nll_v = w_v (g_recon + g_loss),
 *   g_kl_j[i] = (g_k_j + g_loss) c_j beta / N where live[i] and not kl_j[i] < free_j (the tie passes), an explicit 0 elsewhere
 *   and when N <= 0.
 * Same loop and reduction order as mtrssm_elbo_combine_fwd / _counted_fwd: with free = 0 (and no negative KL), w = (1, 1) and
 * warmup = 0 the four scalars and both gradient planes are bitwise theirs. */
typedef struct MtrssmElboSchedule {
  float c0, c1, free0, free1, w_a, w_v, beta_start, warmup;
} MtrssmElboSchedule;
int mtrssm_elbo_schedule_fwd(const float* nll_a, const float* nll_v, const float* kl0, const float* kl1, const float* live,
                             const float* count, const float* step, int64_t n, MtrssmElboSchedule p, float* o_recon, float* o_k0,
                             float* o_k1, float* o_loss, float* o_beta, float* o_stats, void* stream);
int mtrssm_elbo_schedule_bwd(const float* g_recon, const float* g_k0, const float* g_k1, const float* g_loss, const float* kl0,
                             const float* kl1, const float* live, const float* count, const float* beta, int64_t n,
                             MtrssmElboSchedule p, float* g_nll_a, float* g_nll_v, float* g_kl0, float* g_kl1, void* stream);
/* Categorical head of the initial state (core.py:121-135, mmtrssm core.py:321-362): `logits` [rows][K * C] flat (K categoricals
 * of C classes, softmax over classes), `u` [rows][K] uniforms -> logp, probs [rows][K][C] and the inverse-CDF one-hot sample
 * onehot [rows][K * C] (index = #{c <= C - 2 : cumulative probability <= u}, the cumulative sum a left fold).  The straight-through
 * sample of the reference is onehot + probs - probs.detach(): its gradient arrives as g_probs of the backward call,
 *   d_logits[c] = p_c (g_probs[c] - sum_j p_j g_probs[j]) + g_logp[c] - p_c sum_j g_logp[j]   (either gradient may be NULL). */
int mtrssm_categorical_sample_fwd(const float* logits, const float* u, int64_t rows, int32_t K, int32_t C, float* logp, float* probs,
                                  float* onehot, void* stream);
int mtrssm_categorical_sample_bwd(const float* probs, const float* g_probs, const float* g_logp, int64_t rows, int32_t K, int32_t C,
                                  float* d_logits, void* stream);
/* ------------------------------------------------------------------------------------------
 * Gaussian NLL with unit scale, fused reduction.  Replaces objective.likelihood
 * (objective.py:7-23) as used by compute_reconstruction_loss (mrssm/mopoe_mrssm/core.py:279-308):
 *   nll = mean_n sum_e [ 0.5 (target - pred)^2 + 0.5 log(2 pi) ],  n = B*T frames, e = C*H*W.
 * `act` (MTRSSM_ACT_IDENTITY or MTRSSM_ACT_TANH) is the decoder's out_activation (default.yaml: Tanh), applied to `pred`
 * while it is read: pred then holds the decoder's RAW last-layer output and the activated reconstruction is never written.
 * fwd zeroes `out` and accumulates the scalar there; bwd writes d pred = g_out * (act(pred) - target) * act'(pred) / n.
 * ------------------------------------------------------------------------------------------ */
int mtrssm_gaussian_nll_fwd(const float* pred, const float* target, int64_t frames, int64_t event, int32_t act,
                            float* out, void* stream);
int mtrssm_gaussian_nll_bwd(const float* pred, const float* target, const float* g_out,
                            int64_t frames, int64_t event, int32_t act, float* g_pred, void* stream);

/* The same loss over the frames where a modality is present (missing-modality training, DESIGN.md section "Missing
 * modalities"): present[n] per frame (a frame counts when present[n] != 0), count = the divisor,
 *   nll = sum_{n present} sum_e [ 0.5 (target - pred)^2 + 0.5 log(2 pi) ] / count   (0 when count <= 0),
 * d pred = g_out * [n present] * (act(pred) - target) * act'(pred) / count (0 when count <= 0).  `count` is a device scalar
 * (float) the caller forms, so neither call reads anything back to the host.  It is usually the number of present frames, but
 * need not be: a data-parallel rank hands in (present frames of the global batch) / world, so that the mean over ranks is the
 * global batch's loss.  The WHOLE per-frame term is divided by it, the constant included: the forward counts the present frames
 * and adds 0.5 log(2 pi) * event * (present frames) / count, which is exactly the constant when count is their number.
 * The prediction of an absent frame is never used, whatever it holds (NaN and Inf included): its gradient is 0.  With every
 * frame present and count = frames the result is bitwise the unmasked call's.  Null pointers, non-positive sizes or frames * event >= 2^31 return -1 without a launch. */
int mtrssm_gaussian_nll_masked_fwd(const float* pred, const float* target, const float* present, const float* count,
                                   int64_t frames, int64_t event, int32_t act, float* out, void* stream);
int mtrssm_gaussian_nll_masked_bwd(const float* pred, const float* target, const float* present, const float* count,
                                   const float* g_out, int64_t frames, int64_t event, int32_t act, float* g_pred, void* stream);

/* Modality dropout: one call turns uniforms into everything a masked train step reads.
 *   u: [b_global][S][2] fp32 uniforms, S = ceil(steps / span) (a draw is shared by `span` consecutive steps); modality m
 *   (0 audio, 1 vision) is present at (b, t) iff u[b][t / span][m] >= p_m (fp32 compare).  At t = 0 only, a row with neither
 *   present gets the one with the larger u (tie: audio); later steps may have none.
 * Written for the rows row0 .. row0 + b_local - 1 (a data-parallel rank's slice): codes [b_local][steps] (bit 0 audio, bit 1
 * vision, the scans' `modality`), present_audio / present_vision [b_local * steps] in {0, 1} (the masked NLL's `present`),
 * mask0 [b_local][2] bytes in {0, 1} (the t = 0 frame).  counts[2]: the present frames of audio and of vision over ALL b_global
 * rows (zeroed, then one atomic per workgroup; whole numbers below 2^24, so exact).  Nothing is read back to the host.
 * Null pointers, non-positive sizes, a slice outside the batch, p outside [0, 1) or b_global * steps >= 2^24 return -1 without
 * a launch. */
int mtrssm_modality_dropout(const float* u, int64_t b_global, int64_t steps, int64_t span, float p_audio, float p_vision,
                            int64_t row0, int64_t b_local, int32_t* codes, float* present_audio, float* present_vision,
                            uint8_t* mask0, float* counts, void* stream);

/* The masks of a ragged batch: valid [b_global] int32 in DEVICE memory (clamped into [0, steps]), step
 * (b, t) is live iff t < valid[b].  A modality is present iff the step is live AND (u == NULL: no dropout, or the rule of
 * mtrssm_modality_dropout says so, its t = 0 fix-up applied before the AND).  Written for the rank's rows as there, plus
 * live [b_local * steps] in {0, 1} and last [b_local] int32 = valid - 1 (-1: a row with no live step); counts[3]: present audio
 * frames, present vision frames and live steps over ALL b_global rows (zeroed, then one atomic per workgroup and count).
 * Argument rules as mtrssm_modality_dropout (p is only checked when u is given). */
int mtrssm_step_mask_ragged(const int32_t* valid, const float* u, int64_t b_global, int64_t steps, int64_t span, float p_audio,
                            float p_vision, int64_t row0, int64_t b_local, int32_t* codes, float* present_audio, float* present_vision,
                            float* live, uint8_t* mask0, int32_t* last, float* counts, void* stream);

/* The masks of a forecast step: what the model observes and what the loss reconstructs are two planes.
 *   u_context: [b_global] fp32 uniforms in [0, 1); with n = hi - lo + 1 row b observes a context of
 *   c_b = lo + min((int)(u_context[b] * (float)n), n - 1) frames (one fp32 multiply, truncated).  live(b, t) = t < valid[b] (clamped
 *   into [0, steps]; valid == NULL: every row has `steps` live steps), observed = live AND t < c_b.  A modality is SEEN iff the step
 *   is observed AND (u_mask == NULL: no dropout, or the rule of mtrssm_modality_dropout says present, its t = 0 fix-up applied
 *   before the AND); lo >= 1, so frame 0 of a live row is always observed.
 * Written for the rank's rows as there: codes [b_local][steps] (the seen bits; 0 on the open-loop tail and on dead steps),
 * seen_audio / seen_vision [b_local * steps] in {0, 1}, target [b_local * steps] = live (every live frame of both modalities is
 * reconstructed, seen or not), observed [b_local * steps] (the KL's plane: the KL is exactly 0 elsewhere), mask0 [b_local][2] (the
 * seen bits at t = 0), last [b_local] = valid - 1.  counts[2]: live and observed steps over ALL b_global rows (zeroed, then one
 * atomic per workgroup and count).  Argument rules as mtrssm_step_mask_ragged (valid and u_mask may be NULL, u_context may not),
 * plus 1 <= lo <= hi < 2^31. */
int mtrssm_step_mask_forecast(const int32_t* valid, const float* u_mask, const float* u_context, int64_t b_global, int64_t steps,
                              int64_t span, float p_audio, float p_vision, int64_t lo, int64_t hi, int64_t row0, int64_t b_local,
                              int32_t* codes, float* seen_audio, float* seen_vision, float* target, float* observed, uint8_t* mask0,
                              int32_t* last, float* counts, void* stream);

/* Forecast skill: S sampled reconstructions of every frame scored as an ensemble, in one pass.
 *   pred [B][S][T][E] is the decoders' RAW output (`act`: MTRSSM_ACT_IDENTITY or MTRSSM_ACT_TANH, applied while it is read; nothing
 *   activated is written), target [B][T][E], valid [B] int32 in DEVICE memory (NULL: every frame is live; (b, t) is live iff
 *   t < valid[b]).  With y_s = act(pred[b][s][t]) and x = target[b][t], per frame and into the planes [B][T]:
 *     se_s = sum_e 0.5 (x_e - y_s,e)^2;  mean = (se_0 + ... + se_{S-1}) / S;  best = min_s se_s;
 *     ybar_e = (y_0,e + ... + y_{S-1},e) / S;  ens = sum_e 0.5 (x_e - ybar_e)^2;  spread = sum_e 0.5 (sum_s (y_s,e - ybar_e)^2) / S
 *   (the sums over s are left folds; the data term only, without 0.5 E log 2 pi; mean = ens + spread in exact arithmetic; best is
 *   per frame, not per trajectory).  se_samples [B][S][T] (may be NULL) receives se_s, so best == min_s se_samples bitwise.  A
 *   dead frame loads nothing and scores 0 in every plane.
 * One workgroup per frame: the target is read once and every prediction once ((S + 1) * E * 4 bytes), a lane's S quads stay in
 * registers; the reductions run in a fixed order without float atomics, so a frame's result depends on nothing but that frame and
 * two calls agree bitwise.  Null required pointers, B, T, E <= 0, S outside 1 .. 16, E % 4 != 0, an `act` other than the two,
 * pred / target not 16-byte aligned, B * T >= 2^31 or B * S * T * E >= 2^60 return -1 without a launch. */
int mtrssm_ensemble_score(const float* pred, const float* target, const int32_t* valid, int64_t B, int64_t S, int64_t T, int64_t E,
                          int32_t act, float* mean, float* ens, float* best, float* spread, float* se_samples, void* stream);
/* The score planes folded by horizon: planes [P][B][T], context [B] int32 (clamped into [1, T]: c_b frames of row b are observed),
 * valid [B] int32 (may be NULL; clamped into [0, T]).  A live frame has horizon h = 0 when t < c_b, else t - c_b + 1;
 *   sums[p][h] += planes[p][b][t],  counts[h] += 1   (sums [P][T], counts [T], both IN/OUT: batches add up in one buffer).
 * For every bin the live frames are added in ascending b (bin 0: ascending t inside a row) onto the value already there -- a left
 * fold by one thread per (p, h), which an fp32 loop on the host reproduces bit for bit.  Counts are whole numbers in fp32.
 * Null pointers (valid excepted), P outside 1 .. 64, B or T <= 0 or B * T >= 2^24 return -1 without a launch. */
int mtrssm_horizon_table(const float* planes, int64_t P, const int32_t* context, const int32_t* valid, int64_t B, int64_t T,
                         float* sums, float* counts, void* stream);

/* Held-out likelihood: the importance-weighted bound of S sampled posterior trajectories per row.
 * mtrssm_latent_log_ratio: post_logits / prior_logits / stoch [rows][K * C] (a rollout's logits and its one-hot posterior sample);
 *   out[row] = sum_k ( log p_k(c*) - log q_k(c*) ),  p_k / q_k the softmax of categorical k's C prior / posterior logits, c* the
 *   first c with stoch[k][c] > 0.5 (class 0 when there is none).  Any C >= 1.  Each categorical's max, log-sum and differences are
 *   computed in double, the categoricals summed in ascending k, the result rounded to fp32 once; accumulate = 1 adds the double sum
 *   onto out[row] before that one rounding (MMTRSSM's second level), accumulate = 0 overwrites.  Bitwise-equal post and prior
 *   logits (a step that observes nothing) give exactly 0.  Loads are coalesced (consecutive lanes read consecutive floats of a
 *   row; the spans are staged in LDS, C > 512 is walked class by class); a row's result depends on that row only.
 *   Null pointers, rows, K or C <= 0, an accumulate other than 0 / 1 or rows * K * C >= 2^31 return -1 without a launch.
 * mtrssm_iw_bound: se_audio / se_vision [B][S][T] (the data terms mtrssm_ensemble_score writes into se_samples) and log_ratio
 *   [B][S][T] (the sum of the levels' mtrssm_latent_log_ratio); each may be NULL (that term is off), not all three.  valid [B] int32
 *   in DEVICE memory (NULL: every frame is live; (b, t) is live iff t < valid[b]).  On a live frame, per sample s:
 *     a = -se_audio - 0.5 event_audio log 2 pi;  v likewise;  r = log_ratio;  l = (a + v) + r;  cum[s][t] = cum[s][t-1] + l
 *   (a left fold over t; a dead frame adds 0), and into planes [8][B][T], each exactly 0 on a dead frame:
 *     0 iw  = L[t] - L[t-1],  L[t] = max_s cum + log sum_s exp(cum - max_s cum) - log S,  L[-1] = 0
 *     1 elbo = M[t] - M[t-1],  M[t] = (sum_s cum) / S,  M[-1] = 0
 *     2, 3, 4 audio, vision, latent = (sum_s a) / S, (sum_s v) / S, (sum_s r) / S   (0 when the term is off)
 *     5 ess  = (sum_s w)^2 / sum_s w^2,  w = exp(cum - max_s cum)
 *     6, 7 iw_prefix, elbo_prefix = L[t], M[t]
 *   The fold over t, the sums over s (a fixed butterfly inside a 16-lane DPP row, one row of lanes per b) and the ESS run in
 *   double without atomics; each output is rounded to fp32 once.  L[t] >= M[t]; at S = 1 planes 0 / 6 equal planes 1 / 7 bit for
 *   bit.  A row's result depends on that row only and two calls agree bitwise.
 *   Null planes, all three inputs NULL, B or T <= 0, an event size <= 0 of a given data term, S outside 1 .. 16 or B * T >= 2^24
 *   return -1 without a launch. */
int mtrssm_latent_log_ratio(const float* post_logits, const float* prior_logits, const float* stoch, int64_t rows, int64_t K, int64_t C,
                            int32_t accumulate, float* out, void* stream);
int mtrssm_iw_bound(const float* se_audio, const float* se_vision, const float* log_ratio, const int32_t* valid, int64_t B, int64_t S,
                    int64_t T, int64_t event_audio, int64_t event_vision, float* planes, void* stream);

/* Particle-filter likelihood: the bound of mtrssm_iw_bound weighted per frame, with the particles resampled
 * between time segments.  Row b has S particles (1 .. 16); a call folds ONE segment of c frames, the frames t0 .. t0 + c - 1.
 * mtrssm_particle_fold: se_audio / se_vision / log_ratio [B][S][c] as in mtrssm_iw_bound (each may be NULL, not all three); valid [B]
 *   int32 in DEVICE memory (NULL: every frame is live; frame t is live iff t < valid[b]); carry [B][S + 2] double in DEVICE memory,
 *   read and written: lw[0 .. S), base, prev (all zero before a row's first segment).  On a live frame, per particle s:
 *     l = (a + v) + r as in mtrssm_iw_bound;  lw[s] += l;  top = max_s lw;  w_s = exp(lw_s - top);
 *     L = base + (top + log sum_s w_s) - log S
 *   and into planes [8][B][c], each exactly 0 on a dead frame:
 *     0 smc = L - prev (then prev = L);  1 mean = (sum_s l) / S;  2, 3, 4 audio, vision, latent as in mtrssm_iw_bound;
 *     5 ess = (sum_s w)^2 / sum_s w^2;  6 resampled = 1 when the particles were resampled after this frame;  7 smc_prefix = L
 *   Resampling is considered at the segment's last frame t = t0 + c - 1 only, and only with last_segment = 0: it happens iff t is live,
 *   t + 1 < valid[b] and ess <= threshold * S (0 <= threshold <= 1).  It is systematic with ONE uniform u[b * u_stride] (fp32, DEVICE
 *   memory; not read with last_segment = 1): c_s the prefix sums of w in ascending s, target_i = ((u + i) / S) * c_{S-1},
 *   ancestor[b][i] = min(S - 1, #{s : c_s <= target_i}); then base = L and lw[:] = 0.  Otherwise ancestor[b][i] = i.
 *   ancestor [B][S] int32 is written by every call.  The max and the sums over s are the double butterflies of mtrssm_iw_bound, the
 *   prefix sums a walk in lane order (a left fold); every plane is rounded to fp32 once; no atomics; a row's result depends on that
 *   row only and two calls agree bitwise.
 *   Null carry / planes / ancestor, all three inputs NULL, a NULL u or u_stride < 1 with last_segment = 0, B or c <= 0, t0 < 0, an
 *   event size <= 0 of a given data term, S outside 1 .. 16, a threshold outside [0, 1], last_segment outside {0, 1} or
 *   B * c >= 2^24 return -1 without a launch.
 * mtrssm_particle_gather: one launch for all tensors of a state (entries as in mtrssm_state_save: src[k] [B * S][steps][width[k]]
 *   contiguous, dst[k] [B * S][width[k]]; src_stride and alt are ignored):
 *     dst[k][b * S + i, :] = src[k][b * S + ancestor[b][i], steps - 1, :]
 *   (an ancestor outside 0 .. S - 1 is clamped into it).  16 bytes per lane where width[k] % 4 == 0 and both rows are 16-byte
 *   aligned, else 4.  A null table or ancestor, count outside 1 .. MTRSSM_STATE_MAX, B or steps <= 0, S outside 1 .. 16, a null or
 *   misaligned entry, src[k] == dst[k] or B * S * steps * width >= 2^31 return -1 without a launch. */
int mtrssm_particle_fold(const float* se_audio, const float* se_vision, const float* log_ratio, const int32_t* valid, const float* u,
                         int64_t u_stride, int64_t t0, int64_t B, int64_t S, int64_t c, int64_t event_audio, int64_t event_vision,
                         double threshold, int32_t last_segment, double* carry, float* planes, int32_t* ancestor, void* stream);
int mtrssm_particle_gather(const MtrssmStateTable* table, const int32_t* ancestor, int64_t B, int64_t S, int64_t steps, void* stream);

/* Latent overshooting: the KL between the closed-loop posterior at frame t0 + k and the prior rolled k steps
 * open loop from the posterior at t0, k = 1 .. D.  Starts t0_i = o + i * s for i < N = (T - 2 - o) / s + 1; overshoot row
 * r = b * N + i; step j (0-based) of a row is the k = j + 1 step prior for frame t = t0_i + j + 1.  Term (r, k) is live iff
 * t < clamp(valid[b], 0, T) (valid NULL: iff t < T).
 * mtrssm_overshoot_gather: ONE launch for all tensors of a state and the action windows.  Entries as in mtrssm_state_save: src[k]
 *   [B][T][width[k]] contiguous, read in place, dst[k] [B * N][width[k]] (src_stride and alt are ignored):
 *     dst[k][b * N + i, :] = src[k][b, t0_i, :];   windows[b * N + i][j][:] = actions[b, t0_i + 1 + j, :], zeros where that frame >= T
 *   actions [B][T][A], windows [B * N][D][A].  16 bytes per lane where a width is a multiple of 4 and both pointers are 16-byte
 *   aligned, else 4.
 * mtrssm_overshoot_scatter: its backward for the state tensors, one launch.  src[k] = g_dst [B * N][width[k]], dst[k] = g_src
 *   [B][T][width[k]]:  g_src[k][b, t, :] = g_dst[k][b * N + i, :] where t = t0_i, 0 elsewhere; every element of g_src is written
 *   exactly once (no memset beforehand).
 *   Both: a null table / entry / actions / windows, count outside 1 .. MTRSSM_STATE_MAX, B <= 0, T < 2, s < 1, o outside 0 .. T - 2,
 *   D < 2, A <= 0, an N other than (T - 2 - o) / s + 1, src[k] == dst[k], a pointer that is not 4-byte aligned or a tensor of 2^31
 *   elements or more return -1 without a launch.
 * mtrssm_overshoot_kl_fwd: post_logits [b_local][T][K * C] (the rank's closed-loop posterior), os_logits [b_local * N][D][K * C] (the
 *   overshoot rows' prior logits); valid [b_global] int32 in DEVICE memory (ALL rows of the global batch, NULL: every frame is live);
 *   the rank holds the global rows row0 .. row0 + b_local - 1.  Per live term, with lq / lp the log-softmax per categorical of the
 *   posterior / overshoot logits and q = exp(lq):   kl(r, k) = sum_cat sum_c q_c (lq_c - lp_c)   (a class with q_c = 0 adds 0).
 *   Each categorical's max, log-sum and differences in double, categoricals in ascending order, rounded to fp32 once (as
 *   mtrssm_latent_log_ratio).  Outputs: plane [b_local * N][D] fp32, exactly 0 on a dead term; table [2][D] double: per k the sum
 *   and the count of the rank's live terms; count [1] fp32: the live terms with k >= 2 of ALL b_global rows; term [1] fp32: the sum of
 *   the rank's live k >= 2 terms / max(count, 1).  A wave stages both rows in LDS with coalesced loads (any C >= 1; C > 512 reads
 *   in place); the per-term doubles go to `workspace` (mtrssm_overshoot_kl_workspace_bytes(b_local, N, D) bytes, 8-byte aligned, -1
 *   for sizes out of range) and a second one-workgroup launch folds them in a fixed order: no atomics, two calls agree bitwise.
 * mtrssm_overshoot_kl_bwd: g_term [1] (the gradient arriving at `term`) and count [1] in DEVICE memory; scale = g_term / max(count, 1).
 *     g_os_logits [b_local * N][D][K * C] = scale * w_prior * (p - q) on live k >= 2 terms, exactly 0 elsewhere
 *     g_post_logits [b_local][T][K * C] = the sum, over the rows that target (b, t) -- t0 = t - k for k = 2 .. D in ascending k with
 *       t0 >= o, (t0 - o) % s == 0 and (t0 - o) / s < N -- of scale * w_post * q_c ((lq_c - lp_c) - kl_cat); written everywhere
 *   g_post_logits must be NULL exactly when w_post == 0 (then nothing of it is written).  One launch.
 *   Both: null required pointers, rows outside the global batch, K or C <= 0, the size rules above, b_local * N * D * K * C,
 *   b_local * T * K * C or b_global * N >= 2^31, misaligned buffers, a short workspace, negative weights or a gradient buffer that
 *   aliases another buffer return -1 without a launch. */
int mtrssm_overshoot_gather(const MtrssmStateTable* table, const float* actions, float* windows, int64_t B, int64_t T, int64_t N, int64_t s,
                            int64_t o, int64_t D, int64_t A, void* stream);
int mtrssm_overshoot_scatter(const MtrssmStateTable* table, int64_t B, int64_t T, int64_t N, int64_t s, int64_t o, void* stream);
int64_t mtrssm_overshoot_kl_workspace_bytes(int64_t b_local, int64_t N, int64_t D);
int mtrssm_overshoot_kl_fwd(const float* post_logits, const float* os_logits, const int32_t* valid, int64_t b_global, int64_t row0,
                            int64_t b_local, int64_t T, int64_t N, int64_t s, int64_t o, int64_t D, int64_t K, int64_t C, float* plane,
                            double* table, float* count, float* term, void* workspace, int64_t workspace_bytes, void* stream);
int mtrssm_overshoot_kl_bwd(const float* post_logits, const float* os_logits, const int32_t* valid, const float* g_term, const float* count,
                            int64_t b_global, int64_t row0, int64_t b_local, int64_t T, int64_t N, int64_t s, int64_t o, int64_t D, int64_t K,
                            int64_t C, float w_prior, float w_post, float* g_os_logits, float* g_post_logits, void* stream);

/* Latent census: what the categorical latent of a posterior rollout does, per categorical, in one pass.
 * A census step gives row b G copies (1 <= G <= 4) that share the row's uniforms; copy g is scan row r = b * G + g.  Frame t of row b
 * is live iff t < clamp(valid[b], 0, T) (valid [B] int32 in DEVICE memory; NULL: every frame is live).
 * mtrssm_latent_census: post_logits / prior_logits / stoch [B * G][T][K * C] (one level of a rollout: its logits and its one-hot
 *   posterior sample).  Per live frame and categorical k, with lq / lp the log-softmax of the posterior / prior logits (max, log-sum
 *   and differences in double, classes in ascending order, as mtrssm_latent_log_ratio), q = exp(lq), p = exp(lp), c* the first class
 *   with stoch > 0.5 (class 0 when there is none) and lq0 the lq of scan row b * G (the row's first copy):
 *     hq_k = -sum_c q_c lq_c;  hp_k = -sum_c p_c lp_c                         (a class with probability 0 adds 0)
 *     kl_k = sum_c q_c (lq_c - lp_c);  cross_k = sum_c q0_c (lq0_c - lq_c)   (exactly 0 for g = 0 and for bitwise-equal logits)
 *     sw_k = 1 if t >= 1 and c*_k(t) != c*_k(t - 1), else 0
 *   planes [5][B * G][T] fp32 (may be NULL): post_entropy, prior_entropy, kl, cross, switches -- each the sum over k in ascending k of
 *   the quantity above, rounded to fp32 once, exactly 0 on a dead frame; kl and cross are not clamped.
 *   table [G][GS] double, IN/OUT (batches add up in it), GS = 3 K C + 5 K + 2 + 6 T; a group's block holds, in this order:
 *     n [K][C] (live frames with c*_k = c), qsum [K][C] (sum of q_c), psum [K][C] (sum of p_c),
 *     hq, hp, kl, cross, sw [K] each (sums of the per-categorical values), frames (live frames), pairs (live frames with t >= 1),
 *     the position sums [5][T] (the fp32 planes read back as doubles) and the live rows per position [T].
 *   Fold order, fixed by the shapes alone: a row's partial of every cell of n .. sw is a left fold from +0 over its live frames in
 *   ascending t; the step's sum of a cell is a left fold from +0 over the rows' partials in ascending b; that sum is added, in one
 *   add, onto what the table's cell holds.  The position sums likewise: plane[p][b * G + g][t] in ascending b from +0 (dead frames,
 *   exactly 0, included), then one add onto the cell -- a float64 left fold of the returned planes on the host reproduces a step's
 *   sums bit for bit, and a second call of the same step doubles the table exactly.  The counts are whole numbers.  No atomics;
 *   two calls agree bitwise; a row's planes depend on that row and on its first copy only.
 *   Two launches.  The first gives a scan row to one wave: lane j owns categorical k0 + j of a span of at most 64 categoricals; with
 *   C <= 512 the span's 3 (g > 0: 4) x nk x C floats are staged in LDS with coalesced loads, C > 512 is read in place; with K <= 64
 *   and K * C <= 512 the row's partial stays in LDS until the row ends, else the owning lane updates it in `workspace`.  The second
 *   adds the partials and the planes, one thread per cell of the table.  Any C >= 1.
 *   `workspace`: mtrssm_latent_census_workspace_bytes(B, G, T, K, C) bytes, 8-byte aligned (the row partials, the planes of a call
 *   without them, the previous classes); -1 for sizes out of range.  Runs on the caller's stream; nothing is allocated or read back.
 *   Null post_logits / prior_logits / stoch / table / workspace, B, T, K or C <= 0, G outside 1 .. 4, B * G * T >= 2^24,
 *   B * G * T * K * C >= 2^31, a pointer that is not 4-byte (table, workspace: 8-byte) aligned or a short workspace return -1 without
 *   a launch. */
int64_t mtrssm_latent_census_workspace_bytes(int64_t B, int64_t G, int64_t T, int64_t K, int64_t C);
int mtrssm_latent_census(const float* post_logits, const float* prior_logits, const float* stoch, const int32_t* valid, int64_t B, int64_t G,
                         int64_t T, int64_t K, int64_t C, float* planes, double* table, void* workspace, int64_t workspace_bytes,
                         void* stream);

/* Generation coherence: do the two decodes of a sampled rollout read as the same digit, and as the right one.
 * A coherence step gives row b G * S copies (1 <= G <= 4 observed subsets of 1 <= S <= 16 samples); copy (g, s) is scan row
 * (b * G + g) * S + s.  Frame t of row b is live iff t < clamp(valid[b], 0, T) (valid [B] int32 in DEVICE memory; NULL: no row ends
 * early) and 0 <= labels[b][t] <= 9 (labels [B][T] int32 in DEVICE memory; -1 = silence).  With c = min(context, T) frame t has horizon
 * h = 0 for t < c (phase 0) and h = t - c + 1 from c on (phase 1).
 * mtrssm_coherence_fold: logits_v / logits_a [B * G * S][T][10] fp32, the vision / audio reader's logits zv / za of every copy-frame.
 *   Per copy of a live frame, in double:
 *     dv = the lowest index among the largest zv, or 10 (the failure bin) when any of the 10 is not finite; da likewise of za
 *     vision = [dv == label];  audio = [da == label];  agree = [dv == da and dv < 10];  joint = [dv == da == label]
 *     pv_k = exp(zv_k - max zv) / (the left fold over ascending k of exp(zv_k - max zv)); pa_k likewise
 *     soft = the left fold over ascending k of pv_k * pa_k (each product and sum rounded on its own), exactly 0 when a reader failed
 *     pairs[phase][dv][da] += 1
 *   u[p][b * G + g][t] (double) is the left fold from +0 over s = 0 .. S - 1 of plane p's per-copy value, exactly +0 on a dead frame.
 *   planes [5][B * G][T] fp32 (may be NULL): vision, audio, agree, joint, soft -- u / S, rounded to fp32 once.
 *   table [G][GS] double, IN/OUT (steps add up in it), GS = 6 T + 2 * 121; a group's block holds, in this order:
 *     sums [5][T] by horizon (the per-copy values added up, not the means), counts [T] (the live copy-frames per horizon: S per live
 *     frame), pairs [2][11][11].
 *   Fold order, fixed by the shapes alone: cell (g, p, h) of sums is a left fold from +0 over b ascending and, within a row, over t
 *   ascending, of u[p][b * G + g][t] over the frames with h(t) = h (a dead frame's +0 changes nothing); that sum is added, in one add,
 *   onto what the table's cell holds -- a second call of the same step doubles the table exactly.  counts and pairs are whole numbers,
 *   and so are all sums but soft's.  No atomics on floating point and none between workgroups; two calls agree bitwise; a row's planes
 *   depend on that row only.
 *   Two launches.  The first gives (b, g) to one workgroup: spans of 16 frames of its S copies' 2 x 10 logits are staged in LDS with
 *   coalesced loads, a thread scores one copy-frame, then one thread per (plane, frame) adds over s; the (phase, dv, da) counts are
 *   integers in an LDS histogram that the workgroup writes out as its partial set.  The second folds u in the order above, one thread
 *   per cell of the table, and sums the integer partial sets.
 *   `workspace`: mtrssm_coherence_fold_workspace_bytes(B, G, S, T) bytes, 8-byte aligned; its first 5 * B * G * T doubles are u
 *   [5][B * G][T] after the call, the workgroups' pair counts follow; -1 for sizes out of range.  Runs on the caller's stream; nothing is
 *   allocated or read back.
 *   Null logits_v / logits_a / labels / table / workspace, B, T, S or context <= 0, G outside 1 .. 4, S > 16, B * G * S * T >= 2^24, a
 *   pointer that is not 4-byte (table, workspace: 8-byte) aligned or a short workspace return -1 without a launch. */
int64_t mtrssm_coherence_fold_workspace_bytes(int64_t B, int64_t G, int64_t S, int64_t T);
int mtrssm_coherence_fold(const float* logits_v, const float* logits_a, const int32_t* labels, const int32_t* valid, int64_t B, int64_t G,
                          int64_t S, int64_t T, int64_t context, float* planes, double* table, void* workspace, int64_t workspace_bytes,
                          void* stream);

/* Feature moments by bin: the sufficient statistic of a Frechet distance between Gaussian fits.
 * mtrssm_feature_moments: x fp32, row n at x + n * ldx (ldx >= D: a padded buffer is read in place); bin [N] int32 in DEVICE memory:
 *   bin[n] in [0, J) names row n's bin, any other value (-1 by convention) skips the row.
 *   table [J][1 + D + D * D] double, IN/OUT (calls add up in it); bin j's block holds the count of its rows, sum_n x_n [D] and
 *   sum_n x_n x_n^T [D][D] -- a full matrix: both triangles are written and are bit-identical.
 *   Every product x_ni * x_nj is formed in double (exact) on v_mfma_f64_16x16x4_f64 with the contraction over rows; sums in double;
 *   no atomics.  Bins by masking: for bin j the operands of rows in other bins are zeros (and a group of four rows without a row of
 *   bin j is skipped, which adds nothing either way).  Order of addition, fixed by (N, D, J) alone: the rows are cut into
 *   S = min(16, ceil(N / 32)) slices of ceil(N / S) consecutive rows; a slice's partial of a cell starts at +0 and takes its rows four
 *   at a time in ascending order (the four in the MFMA's own fixed order); the call's sum is a left fold from +0 over the slices
 *   in ascending order and is added, in one add, onto what the table's cell holds.  Two calls on the same inputs agree bitwise.
 *   Two launches: one wave per (16 x 16 tile on or above the diagonal, slice) plus one per (16 columns of the sums, slice); then
 *   one thread per cell of the table, which mirrors the tiles below the diagonal.  Nothing is allocated or read back.
 *   `workspace`: mtrssm_feature_moments_workspace_bytes(N, D, J) = 8 * S * J * ((P + DT) * 256 + 1) bytes, 8-byte aligned, with
 *   DT = ceil(D / 16) and P = DT * (DT + 1) / 2 (the slices' tiles, then their counts); -1 for sizes out of range.
 *   Null x / bin / table / workspace, x or bin not 4-byte (table, workspace: 8-byte) aligned, N < 1, D outside 1 .. 256, J outside
 *   1 .. 16, N * ldx >= 2^31 (or a product that overflows), ldx < D or a short workspace return -1 without a launch. */
int64_t mtrssm_feature_moments_workspace_bytes(int64_t N, int D, int J);
int mtrssm_feature_moments(const float* x, int64_t ldx, const int32_t* bin, int64_t N, int D, int J, double* table, void* workspace,
                           int64_t workspace_bytes, void* stream);

/* Linear word probes: one fused step of G multinomial-logistic classifiers over N feature rows.
 *   x [G][N][ld] fp32, of which columns [col0, col0 + F) are read; labels [N] int32 in DEVICE memory, shared by the groups: frame n is
 *   live iff 0 <= labels[n] < C (-1 = silence, a frame past its row's end); weight [G][C][F], bias [G][C].  Per group g and live frame n:
 *     z = W_g x_n + b_g;  nll = logsumexp(z) - z[label];  pred = the lowest index among the largest z;  hit = (pred == label)
 *     stats[g] = (sum nll, sum hit, live count);  g_weight[g] = sum_n (softmax(z) - onehot) x_n^T;  g_bias[g] = sum_n (softmax(z) - onehot)
 *   (normalize = 1: both gradients divided by max(count, 1)).  A dead frame is not read, has nll = hit = 0 and pred = -1 and adds
 *   nothing; with no live frame every sum is exactly 0.  g_weight / g_bias both NULL: evaluation only, the gradient work is skipped.
 *   The planes nll / hit / pred [G][N] may each be NULL.
 * A tile of 16 rows is staged in LDS once and serves both contractions on v_mfma_f32_16x16x4_f32 (fp32 operands and accumulation,
 * classes padded to 16); logits and probabilities never reach memory; exp / log in fp32, the three stats sums in double.  Workgroup
 * partials go to `workspace` (mtrssm_linear_probe_workspace_bytes(G, N, C, F) bytes, 8-byte aligned) and a second small kernel adds
 * them in a fixed order (runs of consecutive partial sets in ascending order, then the runs; the stats by a fixed tree): no float
 * atomics, a grid that depends on the shapes only, two calls agree bitwise.
 * Null required pointers, only one of g_weight / g_bias, G < 1, N outside [1, 2^24), C outside 2 .. 16, F outside 1 .. 2048,
 * col0 < 0, col0 + F > ld, G * N * ld >= 2^31, a normalize other than 0 / 1 or a short workspace return -1 without a launch (the
 * size query returns -1 for sizes out of range). */
int64_t mtrssm_linear_probe_workspace_bytes(int64_t G, int64_t N, int64_t C, int64_t F);
int mtrssm_linear_probe_step(const float* x, int64_t ld, int64_t col0, const int32_t* labels, const float* weight, const float* bias,
                             int64_t G, int64_t N, int64_t C, int64_t F, int32_t normalize, float* g_weight, float* g_bias, float* stats,
                             float* nll, float* hit, int32_t* pred, void* workspace, int64_t workspace_bytes, void* stream);

/* Digit reader: the inference path of the classifier that reads a digit off a predicted vision frame
 * (conv 3x3 1->32, ReLU, pool 2x2, conv 3x3 32->64, ReLU, pool 2x2, Linear 4096->128, ReLU, Linear 128->10; 32 x 32 frames).
 * mtrssm_digit_features: the convolutional trunk of a frame in one launch.  pred [frames][1024] is the decoder's RAW output;
 *   output n reads frame select[n] (int32 [N] in DEVICE memory; NULL: frame n, then N <= frames) as
 *   x = clamp((act(pred) + 1) / 2, 0, 1), `act` MTRSSM_ACT_IDENTITY or MTRSSM_ACT_TANH.  conv1_w [32][1][3][3], conv1_b [32],
 *   conv2_w [64][32][3][3], conv2_b [64] (torch's layouts, fp32); features [N][4096] in the view(-1, 64 * 8 * 8) order.  conv1 is
 *   fp32; conv2 multiplies two bf16 pieces per operand (three products, fp32 sums).  Neither intermediate is written to memory.  A
 *   select[n] outside [0, frames) reads nothing and leaves NaN in row n.  A frame's result depends on that frame only.
 *   Null pointers (select excepted), frames or N outside (0, 2^31), N > frames without select, another `act`, pred / features not
 *   16-byte aligned return -1 without a launch.
 * mtrssm_digit_head: logits[n][k] = b[k] + sum_j w[k][j] hidden[n][j] (hidden [N][128] is fc1's ACTIVATED output, w [10][128]) in
 *   fp32, digit[n] = the lowest index among the largest logits (torch.max's first occurrence).  select / frames (select may be NULL)
 *   are mtrssm_digit_features' own: a frame it could not read (fc1's ReLU has swallowed the NaN features) or whose logits hold a
 *   NaN gets NaN logits and digit 10, the failure bin.  logits [N][10] may be NULL.
 * mtrssm_word_counts: counts[word[n]][digit[n]] += 1 over the frames with word[n] in 0 .. 9 and digit[n] in 0 .. 10 (others are
 *   skipped: word -1 is silence); counts [10][11] fp32 is IN/OUT, column 10 the failure bin.  Integer counting, no float atomics: two
 *   runs agree bitwise.  N outside (0, 2^24) returns -1 (the fp32 counts are exact below 2^24). */
int mtrssm_digit_features(const float* pred, int64_t frames, const int32_t* select, int64_t N, int32_t act, const float* conv1_w,
                          const float* conv1_b, const float* conv2_w, const float* conv2_b, float* features, void* stream);
int mtrssm_digit_head(const float* hidden, const float* w, const float* b, int64_t N, const int32_t* select, int64_t frames, int32_t* digit,
                      float* logits, void* stream);
int mtrssm_word_counts(const int32_t* word, const int32_t* digit, int64_t N, float* counts, void* stream);

/* Training the digit reader.
 * mtrssm_digit_features_train: mtrssm_digit_features (same arguments, bit-identical features) that also writes the TAPE,
 *   uint8 [N][8192 + 4096], 16-byte aligned: one byte per pooled unit of conv1 ([32][16][16]) and of conv2 ([64][8][8], the feature
 *   order) -- the member 2 dy + dx of its 2 x 2 window that holds the maximum (the first in row-major order among equal maxima:
 *   torch's max_pool2d backward), 4 when max + bias <= 0 (a dead unit: relu' = 0).
 * mtrssm_digit_trunk_bwd: the gradients of conv1 / conv2 from g_features [N][4096], with the pool and ReLU choices the tape states
 *   (so the result is a linear function of g_features).  labels int32 [N] in DEVICE memory: row n is live iff 0 <= labels[n] < 10;
 *   a dead row (and one whose select index lies outside [0, frames)) is not read and adds exactly nothing.  pred / frames / select /
 *   N / act as in mtrssm_digit_features.  g_conv1_w [32][1][3][3], g_conv1_b [32], g_conv2_w [64][32][3][3], g_conv2_b [64] are
 *   overwritten, or added to when accumulate = 1.  fp32 arithmetic on exact operands; per frame the kernel reads the frame, its
 *   g_features row and its tape row.  Every workgroup (min(N, CUs) of them) writes one partial set into `workspace`
 *   (mtrssm_digit_trunk_bwd_workspace_bytes(N) bytes, 16-byte aligned; -1 for N outside (0, 2^31)); a second launch adds the sets in
 *   ascending order: no atomics between workgroups, two calls agree bitwise.  No input gradient is produced.
 * mtrssm_digit_head_train: the head with dropout, its loss and its backward, one wave per row.  hidden [N][128] is fc1's ACTIVATED
 *   output h, w [10][128], b [10].  Unit j of row n is kept iff (x >> 8) 2^-24 >= p, x = word j & 3 of
 *   Philox4x32-10(counter = (j >> 2, row0 + rows[n], step, 0), key = (key0, key1)) -- rows int32 [N] in DEVICE memory are the rows' global
 *   numbers (NULL: rows[n] = n), so a row draws the same mask in whatever batch or shard it arrives; p = 0 keeps everything.  With m = keep / (1 - p):
 *   z = w (h m) + b, nll[n] = logsumexp(z) - z[label], pred[n] = the lowest index among the largest z, d = softmax(z) - onehot
 *   (normalize = 1: divided by max(live count, 1)), g_hidden[n] = (w^T d) m [h > 0], g_w (+)= sum_n d (h m)^T, g_b (+)= sum_n d,
 *   stats[3] = (sum nll, sum hit, live count).  A dead row has nll 0, pred -1, a zero g_hidden row and adds nothing.  nll / pred may
 *   be NULL.  Workgroup partial sums go through `workspace` (mtrssm_digit_head_train_workspace_bytes(N) bytes) and are added in a
 *   fixed order.  Null pointers, N outside (0, 2^31), p outside [0, 1), row0 / step that are no 32-bit words, flags other than
 *   0 / 1, misaligned buffers or a short workspace return -1 without a launch. */
int mtrssm_digit_features_train(const float* pred, int64_t frames, const int32_t* select, int64_t N, int32_t act, const float* conv1_w,
                                const float* conv1_b, const float* conv2_w, const float* conv2_b, float* features, uint8_t* tape, void* stream);
int64_t mtrssm_digit_trunk_bwd_workspace_bytes(int64_t N);
int mtrssm_digit_trunk_bwd(const float* pred, int64_t frames, const int32_t* select, int64_t N, int32_t act, const uint8_t* tape,
                           const float* g_features, const int32_t* labels, const float* conv1_w, const float* conv1_b, const float* conv2_w,
                           float* g_conv1_w, float* g_conv1_b, float* g_conv2_w, float* g_conv2_b, int32_t accumulate, void* workspace,
                           int64_t workspace_bytes, void* stream);
int64_t mtrssm_digit_head_train_workspace_bytes(int64_t N);
int mtrssm_digit_head_train(const float* hidden, const float* w, const float* b, const int32_t* labels, const int32_t* rows, int64_t N, int64_t row0,
                            int64_t step, uint32_t key0, uint32_t key1, float p, int32_t normalize, float* nll, int32_t* pred, float* stats, float* g_hidden,
                            float* g_w, float* g_b, int32_t accumulate, void* workspace, int64_t workspace_bytes, void* stream);

/* Episode panels: the finished uint8 video `prior | observation | posterior (| error)` of N episodes, vision on
 * the top row and magma-coloured audio on the bottom row, in one launch.  Replaces the logging callback's host composition
 * (mrssm/callback.py:250-340 create_multimodal_combined_video; 689-905 log_multimodal_video with its per-frame numpy, matplotlib
 * and PIL loops).
 *   Inputs fp32 [N][T][C][H][W] per modality, ACTIVATED values in [-1, 1] (targets or decoder outputs; there is no fused tanh).
 *   Pixel rule, fp32 in this order, no FMA contraction, correctly rounded division:
 *     x = min(max((v + 1) / 2, 0), 1), NaN -> 0
 *     vision byte = trunc(x * 255); Cv = 1 is replicated to RGB, Cv = 3 used as is
 *     audio (channel 0): n = x * 2 - 1; db = (n + 1) / 2 * 80 - 80; s = clamp((clamp(db, -80, 0) - (-80)) / 80, 0, 1);
 *       rgb = MAGMA[min(trunc(s * 256), 255)], MAGMA[k] = trunc(matplotlib magma(k)[:3] * 255)
 *     error column: e = |prior01 - observation01| (Cv = 3: ((e0 + e1) + e2) / 3), rgb = MAGMA[min(trunc(e * 256), 255)]
 *   Canvas: cw = max(Wv, Wa) * scale, Wc = J cw + (J - 1) gap, Hc = bar + Hv scale + gap + Ha scale, J = n_columns.  Cell (vision, j)
 *   starts at (bar, j (cw + gap)), cell (audio, j) at (bar + Hv scale + gap, j (cw + gap)); a frame is drawn left-aligned, nearest
 *   neighbour (canvas[y0 + y][x0 + x] = frame[y / scale][x / scale]), the rest of its cell is 0.  Gap pixels are (64, 64, 64).  The
 *   `bar` top rows are (0, 160, 0) while t < context[n] and (255, 140, 0) from there on.  codes [N][T] int32 (bit 0 audio, bit 1
 *   vision; NULL: both everywhere): with blank_unseen the OBSERVATION cell of a modality that is not seen at (n, t) is black.  valid
 *   [N] int32 (NULL: T everywhere): a frame t >= valid[n] is black altogether.  label = p > 0: the decimal digits of frame0 + t in a
 *   3 x 5 font of p x p pixels (p between digits, a margin of p) white on a black box whose corner is the canvas' (0, 0), drawn last.
 *   out: uint8 [N][T][Hc][Wc][3], 4-byte aligned, mtrssm_episode_panel_bytes(geom, &Hc, &Wc) bytes (Hc / Wc may be NULL).
 * One launch: a lane writes 4 consecutive pixels of the flat video as 3 whole dwords (only the video's final 1 .. 3 bytes, when
 * N T Hc Wc is no multiple of 4, are byte stores); a source element is coloured once for the `scale` pixels of a row it serves.  No
 * atomics; every byte depends on the inputs alone.
 * Bad geometry (sizes < 1, Cv not 1 / 3, scale outside 1 .. 64, gap / bar outside 0 .. 64, label outside 0 .. 16, columns outside
 * 0 .. 3 or repeated, n_columns outside 1 .. 4, a canvas above 32768 either way, frame0 < 0), null context / out, a null input that a
 * column reads or a misaligned buffer return -1 without a launch (the size query returns -1 too). */
#define MTRSSM_PANEL_PRIOR 0
#define MTRSSM_PANEL_OBSERVATION 1
#define MTRSSM_PANEL_POSTERIOR 2
#define MTRSSM_PANEL_ERROR 3
typedef struct MtrssmPanelGeom {
  int32_t N, T, Ca, Ha, Wa, Cv, Hv, Wv, scale, gap, bar, label, frame0, columns[4], n_columns, blank_unseen;
} MtrssmPanelGeom;
int64_t mtrssm_episode_panel_bytes(const MtrssmPanelGeom* geom, int32_t* Hc, int32_t* Wc);
int mtrssm_episode_panel(const MtrssmPanelGeom* geom, const float* obs_a, const float* post_a, const float* prior_a, const float* obs_v,
                         const float* post_v, const float* prior_v, const int32_t* codes, const int32_t* valid, const int32_t* context,
                         uint8_t* out, void* stream);

/* ------------------------------------------------------------------------------------------
 * Fused AdamW over one flat fp32 parameter buffer, with global-norm gradient clipping
 * (yaml: torch.optim.AdamW lr 1e-3; trainer.gradient_clip_val 10 -- default.yaml:103-107,119).
 * sumsq: device scalar holding sum(grad^2) (mtrssm_sumsq writes it); clip <= 0 disables clipping.
 * ------------------------------------------------------------------------------------------ */
int mtrssm_sumsq(const float* x, int64_t n, float* out, void* stream);
int mtrssm_adamw_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n,
                      const float* sumsq, float clip_norm, float grad_scale, float lr, float beta1,
                      float beta2, float eps, float weight_decay, int32_t step, void* stream);
/* The same step with its scalars in device memory, so that it can sit inside a captured hipGraph (FlatAdamW's path):
 *   state[4] (device floats): [0] learning rate (the host writes it when a scheduler changes it), [1] steps taken,
 *   [2] 1 - beta1^step, [3] sqrt(1 - beta2^step).  mtrssm_adamw_prepare = zero `sumsq`, sum(grad^2) into it, step += 1 and the
 *   two bias corrections; mtrssm_adamw_apply = clip + AdamW reading `state`.
 *   active (n bytes, may be NULL = all): 0 marks elements of parameters that never received a gradient; they are left
 *   untouched (no decay, no moments) as torch.optim.AdamW does for `.grad is None` -- MMTRSSM's l_posterior and dummy
 *   transition (mmtrssm/mopoe_mmtrssm/core.py:143-151,188). */
/* Zero `bytes` (multiple of 4, 4-byte aligned) of device memory with a plain kernel: what FlatParameters.zero_grad() uses, so that a
 * captured train step records no memset node (a captured multi-megabyte hipMemsetAsync left foreign bytes at the buffer's head
 * on replay under ROCm 7.2). */
int mtrssm_clear(void* p, int64_t bytes, void* stream);
/* status (device int32, may be NULL): the sticky status word of the step's cooperative scan kernels (first word of the workspace of
 * mtrssm_mrssm_rollout_*_cluster / _wide).  Non-zero = an exchange of the step gave up, its gradients are invalid: prepare then
 * does not count the step and apply leaves parameters and moments untouched (the host raises when it next polls the word). */
int mtrssm_adamw_prepare(const float* grad, int64_t n, float* sumsq, float* state, const int32_t* status, float beta1, float beta2,
                         void* stream);
int mtrssm_adamw_apply(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, const uint8_t* active, int64_t n,
                       const float* sumsq, const float* state, const int32_t* status, float clip_norm, float grad_scale, float beta1,
                       float beta2, float eps, float weight_decay, void* stream);

/* ------------------------------------------------------------------------------------------
 * The fit loop's per-step fold (no reference counterpart: Lightning's on_epoch=True logging and its gradient
 * norm callbacks read scalars back per step).  Called once after every train step, behind the optimizer (which leaves the reduced,
 * unclipped gradient in place), on the caller's stream; two launches, no atomics, nothing allocated.
 *   grad, param: the flat fp32 buffers, numel floats each (numel a multiple of 4), 16-byte aligned.
 *   offsets: G + 1 ascending DEVICE int64 offsets, multiples of 4, offsets[0] = 0, offsets[G] = numel: G <= 32 segments.
 *   group: G DEVICE int32 (NULL: group[s] = s): the first segment of the name segment s belongs to (group[s] <= s,
 *     group[group[s]] = group[s]); the norms of a name are the roots of the summed squares of its segments, kept at its first one.
 *   scalars: K <= 8 DEVICE floats (the all-reduced loss scalars of the gradient buffer's tail), each times scalar_scale (1 / world).
 *   weight: ONE device float, the step's weight (global batch rows).  The step's index is flags[MTRSSM_FIT_FLAG_STEP], which every
 *     call advances by one: the caller writes it when an epoch begins or a run resumes, and no by-value argument changes per step.
 * Per segment: sum(g^2), sum(p^2) -- every product and sum in double -- and the count of non-finite gradient elements.  A
 * workgroup sums one chunk (mtrssm_fit_fold_workspace_bytes reports its floats) of one segment; chunk sums meet in an order fixed by
 * numel and offsets alone: two calls on the same buffers are bitwise equal.  The call leaves them in the workspace's first
 * 3 x 32 doubles: [0][s] sum(g^2), [1][s] sum(p^2), [2][s] the count.
 * A step is FINITE when every scalar and every gradient element is.  acc (doubles) then gains, with norm(x) = sqrt(sum x^2):
 *   [MTRSSM_FIT_ACC_WEIGHT] += w;  [_STEPS] += 1;  [_CLIPPED] += (norm(g) grad_scale > clip_norm > 0);
 *   [_GRAD_SUM] += norm(g) grad_scale;  [_GRAD_MAX] = max(., norm(g) grad_scale);  [_PARAM] = norm(p)          (all segments)
 *   [_SCALARS + k] += w * scalars[k] * scalar_scale                                                            (k < K)
 *   [_SEGMENTS + 3 s + 0 / 1 / 2]: the same sum / max / last norm(p) of the name whose first segment is s       (s < G)
 * Otherwise acc stays as it was, bit for bit, and flags (int32) record the step: [_BAD_STEPS] += 1, [_FIRST_BAD] = the step's index
 * if it is the first, [_BAD_SEGMENTS] |= bit s of every segment with a non-finite gradient element, [_BAD_SCALARS] |= bit k.
 * The caller zeroes both blocks (first bad step: -1) when an epoch begins; MTRSSM_FIT_ACC_DOUBLES / MTRSSM_FIT_FLAG_INTS are their sizes.
 * ------------------------------------------------------------------------------------------ */
#define MTRSSM_FIT_MAX_SEGMENTS 32
#define MTRSSM_FIT_MAX_SCALARS 8
#define MTRSSM_FIT_ACC_WEIGHT 0
#define MTRSSM_FIT_ACC_STEPS 1
#define MTRSSM_FIT_ACC_CLIPPED 2
#define MTRSSM_FIT_ACC_GRAD_SUM 3
#define MTRSSM_FIT_ACC_GRAD_MAX 4
#define MTRSSM_FIT_ACC_PARAM 5
#define MTRSSM_FIT_ACC_SCALARS 6
#define MTRSSM_FIT_ACC_SEGMENTS 14
#define MTRSSM_FIT_ACC_DOUBLES 110
#define MTRSSM_FIT_FLAG_BAD_STEPS 0
#define MTRSSM_FIT_FLAG_FIRST_BAD 1
#define MTRSSM_FIT_FLAG_BAD_SEGMENTS 2
#define MTRSSM_FIT_FLAG_BAD_SCALARS 3
#define MTRSSM_FIT_FLAG_STEP 4
#define MTRSSM_FIT_FLAG_INTS 8
/* Bytes of the caller-owned workspace (-1: numel or G out of range); *chunk_floats (may be NULL) receives the floats of a chunk. */
int64_t mtrssm_fit_fold_workspace_bytes(int64_t numel, int32_t G, int64_t* chunk_floats);
int mtrssm_fit_fold(const float* grad, const float* param, int64_t numel, const int64_t* offsets, const int32_t* group, int32_t G,
                    const float* scalars, int32_t K, float scalar_scale, float grad_scale, float clip_norm, const float* weight,
                    double* acc, int32_t* flags, void* workspace, int64_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Dense fp32 GEMM on the fp32 MFMA with the elementwise neighbours fused in.  Replaces the nn.Linear / MLP calls around
 * the recurrence and their autograd (torchrl MLP at networks.py:57-64,130-145; cnn's Linear layers; init_proj,
 * core.py:132-133) and the weight gradients of the scan:
 *   C[i][j] (+)= act_out( bias[j] + sum_r actA(A'(i, r)) * actB(B'(j, r)) ) * act_z'(zgrad[i][j])
 *   A'(i, r) = a_rmajor ? A[r * lda + i] : A[i * lda + r];   B'(j, r) = b_rmajor ? B[r * ldb + j] : B[j * ldb + r]
 *   forward Y = act(X) W^T + b: A = X, B = W;  data gradient dX = (dY W) * act'(X): A = dY, B = W with b_rmajor;
 *   weight gradient dW += dY^T act(X), db += column sums of dY: A = dY, B = X, both r-major, accumulate, colsum = db.
 * bias, zgrad, colsum may be NULL.  split_r: 0 = choose (splits only when accumulate is set and no output epilogue), else
 * the number of reduction slices (> 1 meets in C by fp32 atomics: accumulate = 1, or a dense C that the call zeroes
 * first).  Numerics: each output element is a k-ordered fp32 fma chain per slice (v_mfma_f32_32x32x2_f32).  Rows may be strided views (lda / ldb / ldc / ldz).
 * ------------------------------------------------------------------------------------------ */
typedef struct MtrssmGemm {
  const float* A;
  const float* B;
  float* C;
  const float* bias;
  const float* zgrad;
  float* colsum;
  int32_t M, N, R, lda, ldb, ldc, ldz;
  int32_t a_rmajor, b_rmajor, act_a, act_b, act_out, act_z, accumulate, split_r;
  int32_t* tickets;   /* optional: >= n_tickets device ints (zeroed by the call).  Lets a reduction be split although the output */
  int32_t n_tickets;  /* has an epilogue (act' of a data gradient): the last slice to arrive at a 64 x 64 tile finishes it */
  int32_t mfma_split; /* 0: fp32 MFMA (above); 2: every operand value as two bf16 pieces (16 significant bits, made while staging),
                         three bf16 MFMA products per k-block, fp32 accumulation -- the conv kernels' default arithmetic, for the
                         large Linear layers inside the conv stacks (cnn.Encoder head, cnn.Decoder stem) */
} MtrssmGemm;
int mtrssm_gemm(const MtrssmGemm* g, void* stream);
/* `count` INDEPENDENT problems (no output of one is an operand or the output of another; mfma_split = 0) in as few launches as
 * their operand layouts allow -- problems with equal (a_rmajor, b_rmajor) share one grid.  The weight gradients of the scan
 * (scan.py: ten to fifteen [out, B*T] x [B*T, in] GEMMs per backward, each a latency-bound launch of its own before) go
 * through this call.  Per problem exactly the arithmetic of mtrssm_gemm. */
int mtrssm_gemm_group(const MtrssmGemm* problems, int32_t count, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MTRSSM_H */
