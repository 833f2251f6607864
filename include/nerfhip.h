/* nerfhip.h — C ABI of libnerfhip.so: the MI355X (gfx950) NeRF volume-rendering hot path.
 *
 * Drop-in boundary for kwea123/nerf_pl's `models/nerf.py` + `models/rendering.py`.
 * The reference has no FFI of its own for this path except the `torchsearchsorted`
 * extension (rendering.py:2,42); every other entry point below replaces a *sequence of
 * ATen launches* inside one reference Python function, cited per function
 * (paths relative to the reference root, line numbers as in SURVEY.md).
 *
 * Conventions
 *   - plain C: pointers + sizes, no torch / C++ types.  All pointers are DEVICE pointers
 *     (HBM) unless the name ends in `_host`.  All tensors are dense row-major fp32 unless noted.
 *   - the caller owns every buffer (inputs, outputs, workspaces); the library allocates
 *     nothing and keeps no mutable global state => every entry point is hipGraph-capturable.
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream).  Nothing synchronises.
 *   - return value: 0 on success, a positive hipError_t, or a negative NERFHIP_E* code.
 *     Nothing throws across the ABI.
 */
#ifndef NERFHIP_H
#define NERFHIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NERFHIP_ABI_VERSION 3     /* 2: nerfhip_mlp_pack_weights_bwd takes the biases (fold block of the W^T image); 3 (additive):
                                   * nerfhip_render_args.regen_enc, nerfhip_mlp_bwd_multi_rays                                   */

#define NERFHIP_E_BADARG (-1)  /* null pointer / non-positive size / unsupported shape */
#define NERFHIP_E_UNSUPPORTED (-2)
#define NERFHIP_E_ALIGN (-3)   /* pointer not aligned as documented */
#define NERFHIP_E_DATA (-4)    /* damaged input data (a JPEG scan that is truncated or holds an invalid code) */

/* MLP arithmetic type (`dtype` arguments). */
#define NERFHIP_F32 0  /* v_mfma_f32_32x32x2_f32, exact fp32 (parity configuration)      */
#define NERFHIP_BF16 1 /* v_mfma_f32_32x32x16_bf16, fp32 accumulate (roofline config)    */
#define NERFHIP_BF16_F8 2 /* as NERFHIP_BF16 (forward, dX chain: bf16 MFMA); the tensors saved for the weight-gradient
                           * GEMM are stored block-scaled in 8 bits — the activations X as OCP e4m3, dY as OCP e5m2, one
                           * e8m0 scale per 32 points x one layer's section — and consumed by
                           * v_mfma_scale_f32_32x32x64_f8f6f4: half the backward's HBM bytes.
                           * Inference entry points treat it as NERFHIP_BF16.                                          */

typedef void* nerfhip_stream_t;

int nerfhip_abi_version(void);
const char* nerfhip_error_string(int code);

/* ---- a2. Embedding.forward  (models/nerf.py:21-38) -------------------------------------
 * out[i, :] = [x, sin(2^0 x), cos(2^0 x), ..., sin(2^(F-1) x), cos(2^(F-1) x)]
 * x (n,C) -> out (n, C*(2F+1)).  1 <= C <= 8, 0 <= F <= 16.                               */
int nerfhip_posenc(const float* x, float* out, int64_t n, int C, int n_freqs, nerfhip_stream_t stream);
/* backward of the above w.r.t. x: gx (n,C) = d<gout,out>/dx.                              */
int nerfhip_posenc_bwd(const float* x, const float* gout, float* gx, int64_t n, int C, int n_freqs,
                       nerfhip_stream_t stream);

/* The same with explicit frequency bands (bands: n_freqs DEVICE floats; NULL = the 2^k above): the reference's
 * `Embedding(..., logscale=False)` = torch.linspace(1, 2^(F-1), F) (nerf.py:16-19), passed as the module built them.   */
int nerfhip_posenc_bands(const float* x, const float* bands, float* out, int64_t n, int C, int n_freqs,
                         nerfhip_stream_t stream);
int nerfhip_posenc_bands_bwd(const float* x, const float* bands, const float* gout, float* gx, int64_t n, int C, int n_freqs,
                             nerfhip_stream_t stream);

/* ---- a5. coarse depth sampling  (models/rendering.py:183-204) --------------------------
 * rays (B,8)=[o d near far]; z (B,S): linear in depth or disparity; when perturb>0,
 * stratified jitter with `perturb_rand` (B,S) ~ U[0,1) (the caller's torch.rand draw).     */
int nerfhip_sample_coarse_z(const float* rays, const float* perturb_rand, float* z, int64_t B, int S,
                            int use_disp, float perturb, nerfhip_stream_t stream);

/* ---- a9. torchsearchsorted.searchsorted(a, v, side='right')  (rendering.py:2,42) --------
 * idx[r,k] = first j in [0,M] with a[r,j] > v[r,k]  (numpy side='right'); a (B,M), v (B,K),
 * idx int64 (B,K).  This is the one native extension the reference depends on.             */
int nerfhip_searchsorted_right(const float* a, const float* v, int64_t* idx, int64_t B, int M, int K,
                               nerfhip_stream_t stream);
/* side='left' (the extension's default; unused by the reference): first j with a[r,j] >= v[r,k]. */
int nerfhip_searchsorted_left(const float* a, const float* v, int64_t* idx, int64_t B, int M, int K,
                              nerfhip_stream_t stream);

/* ---- a8. sample_pdf  (models/rendering.py:14-55) ----------------------------------------
 * bins (B,M+1) with row stride `bins_stride`, weights (B,M) with row stride `w_stride`
 * (so that the reference's `weights_coarse[:, 1:-1]` view needs no copy).
 * u: NULL => deterministic linspace(0,1,K) (`det=True`); else (K) if u_stride==0 or (B,K).
 * samples (B,K).                                                                           */
int nerfhip_sample_pdf(const float* bins, int64_t bins_stride, const float* weights, int64_t w_stride,
                       const float* u, int64_t u_stride, float* samples, int64_t B, int M, int K, float eps,
                       nerfhip_stream_t stream);

/* Rounding of the pdf normaliser `torch.sum(weights, -1)` (rendering.py:30), on whose last bit the searchsorted indices of
 * rendering.py:42 have knife edges (u == 1.0, cdf ties):
 *   NERFHIP_ROW_TOTAL_EXACT  the correctly rounded fp32 sum (host-independent).  What the plain entry points without a row_total
 *                            argument — nerfhip_sample_pdf, nerfhip_fine_z — use.
 *   NERFHIP_ROW_TOTAL_ATEN   the fp32 additions in the order of ATen's CPU sum kernel (torch 2.x, every x86 capability:
 *                            8-float vectors, 4 interleaved accumulators, scalar tail) = the reference's own bits on CPU;
 *                            reproduces the (cdf, u) -> inds triples recorded at the reference's call site on every element.
 *                            What the Python operators (nerf_pl_amd.ops: sample_pdf_u, fine_z, render_rays, the fused training
 *                            step) pass BY DEFAULT through the entry points that take row_total (ops.set_row_total("exact") /
 *                            NERFHIP_ROW_TOTAL=exact selects the other): over the minted reference training runs the HIP fp32
 *                            path then follows the reference's PSNR@step with half the seed-to-seed scatter (oracle and parity). */
#define NERFHIP_ROW_TOTAL_EXACT 0
#define NERFHIP_ROW_TOTAL_ATEN 1

/* Same, additionally exporting what the fused kernel computed on the way (either may be NULL): cdf_out (B,M+1) = the
 * cdf of rendering.py:31-33 and inds_out (B,K) int64 = searchsorted(cdf, u, side='right') of rendering.py:42 — the
 * bit-exact contract of the path, checkable against the indices recorded at the reference's own call site.
 * row_total: NERFHIP_ROW_TOTAL_*.                                                                                   */
int nerfhip_sample_pdf_ex(const float* bins, int64_t bins_stride, const float* weights, int64_t w_stride,
                          const float* u, int64_t u_stride, float* samples, int64_t B, int M, int K, float eps,
                          float* cdf_out, int64_t* inds_out, int row_total, nerfhip_stream_t stream);

/* ---- a10. fine-pass depth assembly  (models/rendering.py:223-229) -----------------------
 * z_mid = midpoints(z_coarse); z_new = sample_pdf(z_mid, w_coarse[:,1:-1], N_i, u);
 * z_fine = sort(cat(z_coarse, z_new)).  One launch, one wave per ray.
 * z_coarse,w_coarse (B,S_c); u as above; z_fine (B,S_c+N_i); z_new (B,N_i) optional (NULL ok). */
int nerfhip_fine_z(const float* z_coarse, const float* w_coarse, const float* u, int64_t u_stride,
                   float* z_fine, float* z_new, int64_t B, int S_c, int N_i, float eps,
                   nerfhip_stream_t stream);

/* Same with the optional exports and the row_total choice of nerfhip_sample_pdf_ex: cdf_out (B,S_c-1), inds_out (B,N_i) int64. */
int nerfhip_fine_z_ex(const float* z_coarse, const float* w_coarse, const float* u, int64_t u_stride, float* z_fine,
                      float* z_new, int64_t B, int S_c, int N_i, float eps, float* cdf_out, int64_t* inds_out,
                      int row_total, nerfhip_stream_t stream);

/* ---- a7. alpha compositing  (models/rendering.py:143-172) -------------------------------
 * raw: (B,S,4)=[r g b sigma] when raw_ch==4, or (B,S) sigma only when raw_ch==1 (weights_only).
 * noise: (B,S) standard-normal draws or NULL; sigma_eff = relu(sigma + noise*noise_std).
 * weights (B,S) always written; opacity (B) always; rgb (B,3) and depth (B) when raw_ch==4.  */
int nerfhip_composite_fwd(const float* raw, int raw_ch, const float* z, const float* rays,
                          const float* noise, float noise_std, int white_back, float* weights, float* rgb,
                          float* depth, float* opacity, int64_t B, int S, nerfhip_stream_t stream);
/* backward: given g_rgb (B,3) [, g_depth (B), g_opacity (B); NULL = 0] produce g_raw (B,S,raw_ch).
 * Recomputes alpha/T from raw,z,noise (nothing else is saved by forward).                   */
int nerfhip_composite_bwd(const float* raw, int raw_ch, const float* z, const float* rays,
                          const float* noise, float noise_std, int white_back, const float* g_rgb,
                          const float* g_depth, const float* g_opacity, const float* g_weights,
                          float* g_raw, int64_t B, int S, nerfhip_stream_t stream);

/* Training fast path (train.py:103-117 with losses.py:9-14): composite_fwd (raw_ch 4) + d MSE / d rgb of every ray against
 * `target` (B,3), i.e. g_rgb = (rgb - target) * grad_scale with grad_scale = 2 / (3 B) for one image's mean-squared error, +
 * composite_bwd for that g_rgb, in ONE launch.  Writes weights (B,S; NULL ok), rgb (B,3), depth (B), opacity (B) and
 * g_raw (B,S,4) = d loss / d raw — bit-identical to composite_fwd -> mse_psnr -> composite_bwd.                          */
int nerfhip_composite_train(const float* raw, const float* z, const float* rays, const float* noise, float noise_std,
                            int white_back, const float* target, float grad_scale, float* weights, float* rgb, float* depth,
                            float* opacity, float* g_raw, int64_t B, int S, nerfhip_stream_t stream);

/* The coarse pass of a training step (rendering.py:143-172 + :223-229): nerfhip_composite_train and, for the same ray in the same
 * wave, nerfhip_fine_z_ex on its weights (u / u_stride / N_i / eps / z_fine / row_total as there) — the weights travel from the quadrature to the
 * inverse-CDF sampling through LDS (`weights` may be NULL).  Bit-identical to the two launches.  3 <= S <= 2048 like the other
 * training entry points: two rays' tables, (7 S + 2 N_i) floats each, share the workgroup's LDS — up to the 160 KB of the CU
 * (S = 2048 with N_i = 128: 114 KB), where nerfhip_fine_z_ex alone holds four rays in 64 KB and stops at 4 S + 2 N_i <= 4092.  */
int nerfhip_composite_train_fine_z(const float* raw, const float* z, const float* rays, const float* noise, float noise_std,
                                   int white_back, const float* target, float grad_scale, float* weights, float* rgb, float* depth,
                                   float* opacity, float* g_raw, int64_t B, int S, const float* u, int64_t u_stride, int N_i,
                                   float eps, float* z_fine, int row_total, nerfhip_stream_t stream);
/* The last pass of a training step: nerfhip_composite_train + the loss values of nerfhip_mse_psnr (losses.py:9-14,
 * metrics.py:4-13) — out3 = [loss, psnr, mse] over this pass's rgb as the fine image and rgb_coarse (B,3; NULL when this pass is
 * the only one) as the coarse image, reduced by the last workgroup to finish in nerfhip_mse_psnr's own order (same bits).
 * ticket: one zero-initialised DEVICE word owned by the caller; the launch leaves it at zero.                              */
int nerfhip_composite_train_loss(const float* raw, const float* z, const float* rays, const float* noise, float noise_std,
                                 int white_back, const float* target, float grad_scale, float* weights, float* rgb, float* depth,
                                 float* opacity, float* g_raw, int64_t B, int S, const float* rgb_coarse, float* out3,
                                 uint32_t* ticket, nerfhip_stream_t stream);

/* ---- a3/a4. NeRF MLP  (models/nerf.py:42-124; D=8 W=256 skips=[4] in 63/27) -------------
 * Parameters are repacked once per weight update into the MFMA A-fragment stream the
 * kernel consumes (layout: DESIGN.md §3).  weights_host[i]/biases_host[i] are HOST arrays of
 * 12 DEVICE pointers in state_dict order: xyz_encoding_1..8, xyz_encoding_final,
 * dir_encoding, sigma, rgb (each weight (out,in) row-major fp32).                           */
size_t nerfhip_mlp_packed_bytes(int dtype);
int nerfhip_mlp_pack_weights(const float* const* weights_host, const float* const* biases_host, void* packed,
                             int dtype, nerfhip_stream_t stream);

/* Training: bytes of the saved-activation buffer the forward fills when `save_acts` != NULL
 * (every B-operand slab of every layer, in register/fragment order; 4.94 KB/point in bf16,
 * 9.9 KB/point in fp32).  The backward entry points consume it.               */
size_t nerfhip_mlp_act_bytes(int64_t n_points, int dtype);

/* NeRF.forward(x, sigma_only) on pre-embedded inputs (nerf.py:83-124):
 * x (n, 90 | 63) with row stride x_stride floats -> out (n,4)=[rgb sigma] | (n,1).
 * save_acts: NULL for inference; else a nerfhip_mlp_act_bytes(n,dtype) buffer (sigma_only must be 0). */
int nerfhip_mlp_fwd_embedded(const float* x, int64_t x_stride, int64_t n, const void* packed, float* out,
                             int sigma_only, int dtype, void* save_acts, nerfhip_stream_t stream);

/* Fused `inference` MLP loop (rendering.py:115-141 + 206-207 + nerf.py:21-38): points are
 * generated in-register as o + d*z, encoded (10 / 4 frequencies) and pushed through the MLP;
 * no (n,63)/(n,90) tensor and no repeat_interleave'd dir embedding ever exists in HBM.
 * rays (B,8), z (B,S) -> out (B,S,4) | (B,S) when sigma_only.                               */
int nerfhip_mlp_fwd_rays(const float* rays, const float* z, int64_t B, int S, const void* packed, float* out,
                         int sigma_only, int dtype, void* save_acts, nerfhip_stream_t stream);

/* The same for the COARSE pass with its depths formed in the kernel's prologue (rendering.py:183-204 = nerfhip_sample_coarse_z,
 * then :206-207): z (B,S) is an OUTPUT here — every point's depth is computed from its ray's bounds (and perturb_rand (B,S), the
 * caller's U[0,1) draw, when perturb > 0), used, and written for the compositing that follows.  Same bits as the two launches. */
int nerfhip_mlp_fwd_rays_coarse(const float* rays, const float* perturb_rand, float* z, int64_t B, int S, int use_disp,
                                float perturb, const void* packed, float* out, int sigma_only, int dtype, void* save_acts,
                                nerfhip_stream_t stream);

/* ---- backward of the MLP (autograd mirror of nerf.py:100-124 under train.py:103-117) -----------
 * Two hand-written phases: the register-resident chain in reverse with W^T streamed
 * (writes dL/d(pre-activation) slabs into `dys`), then dW = dY^T X with points as the MFMA K
 * dimension (split-K partial slabs in `dw_workspace`, reduced and un-permuted into the gradients).
 *   g_out (n,4)  dL/d[rgb sigma];  out (n,4) the forward's output (for sigmoid');
 *   packed_bwd   nerfhip_mlp_pack_weights_bwd() image of the CURRENT parameters: the W^T fragment stream of the chain, then an fp32
 *                snapshot of xyz_encoding_final's weight + bias and of dir_encoding's first 256 weight columns.  xyz_encoding_final
 *                has no activation (nerf.py:70,116): the forward does not save its output, the chain does not store its output
 *                gradient, the dW launch forms G = dY_dir^T h8 and a small fp32 launch (mlp_bwd_fold_kernel) finishes
 *                dW_dir[:, :256] = G W_f^T + db_dir b_f^T, dW_final = W_dir[:, :256]^T G, db_final = W_dir[:, :256]^T db_dir —
 *                the same sums, re-associated (csrc/mlp_layout.h kDwJobs);
 *   acts         buffer the forward filled (save_acts);  dys  nerfhip_mlp_dy_bytes() scratch;
 *   dw_workspace nerfhip_mlp_dw_workspace_bytes() scratch;
 *   grad_w_host / grad_b_host: HOST arrays of 12 DEVICE pointers (state_dict order, (out,in) fp32);
 *   accumulate != 0 adds into them, else overwrites.  No gradient flows to rays / z / x
 *   (the reference's sampled depths are detached, rendering.py:226; rays carry no grad).            */
size_t nerfhip_mlp_packed_bwd_bytes(int dtype);
int nerfhip_mlp_pack_weights_bwd(const float* const* weights_host, const float* const* biases_host, void* packed_bwd, int dtype,
                                 nerfhip_stream_t stream);
/* both images (nerfhip_mlp_pack_weights + nerfhip_mlp_pack_weights_bwd) in ONE launch: what a training step needs
 * of a model whose weights do not change between its forward and its backward                                   */
int nerfhip_mlp_pack_weights_train(const float* const* weights_host, const float* const* biases_host, void* packed,
                                   void* packed_bwd, int dtype, nerfhip_stream_t stream);
/* ... of `n_models` (<= 4) models in ONE launch: weights_host / biases_host hold n_models x 12 DEVICE pointers (model-major),
 * packed_host / packed_bwd_host one DEVICE buffer per model.  A training step packs its coarse and its fine network here. */
int nerfhip_mlp_pack_weights_train_multi(const float* const* weights_host, const float* const* biases_host,
                                         void* const* packed_host, void* const* packed_bwd_host, int n_models, int dtype,
                                         nerfhip_stream_t stream);
size_t nerfhip_mlp_dy_bytes(int64_t n_points, int dtype);
int nerfhip_mlp_dw_splits(int64_t n_points, int dtype);   /* total (job, point-split) workgroups = partial slabs */
/* The workspace size queries and the launches compute the SAME split plan, a function of (points per model, dtype) alone: what a
 * query returns is exactly what the launch with those arguments writes, with or without regenerated encodings.               */
size_t nerfhip_mlp_dw_workspace_bytes(int64_t n_points, int dtype);
int nerfhip_mlp_bwd(const float* g_out, const float* out, int64_t n, const void* packed_bwd, const void* acts,
                    void* dys, void* dw_workspace, float* const* grad_w_host, float* const* grad_b_host,
                    int accumulate, int dtype, nerfhip_stream_t stream);

/* The same with a phase mask (measurement: bench.py times the three kernels of the backward separately with HIP events):
 * bit 0 = backward chain (writes dys), bit 1 = weight-gradient GEMM (reads acts + dys, writes dw_workspace),
 * bit 2 = reduce (dw_workspace -> gradients).  nerfhip_mlp_bwd == phases 7.                                          */
int nerfhip_mlp_bwd_phases(const float* g_out, const float* out, int64_t n, const void* packed_bwd, const void* acts,
                           void* dys, void* dw_workspace, float* const* grad_w_host, float* const* grad_b_host,
                           int accumulate, int dtype, int phases, nerfhip_stream_t stream);

/* The backward of SEVERAL models (<= 2: a training step's fine and coarse network) with ONE weight-gradient launch and ONE
 * reduce launch for all of them: per model its chain kernel, then one dW GEMM whose workgroups are shared out over the 12 jobs
 * of every model in proportion to the models' points (equal ring iterations per workgroup), then one reduce.  All `_host`
 * arguments are HOST arrays with one entry per model (grad_w_host / grad_b_host: n_models x 12 DEVICE pointers, model-major);
 * dw_workspace holds nerfhip_mlp_dw_workspace_bytes_multi() bytes.  `adam` (NULL ok; requires accumulate == 0): apply the Adam
 * update of nerfhip_adam_step to every model's flat parameter buffer inside the reduce kernel — each model's parameters,
 * exp_avg, exp_avg_sq are flat fp32 buffers laid out like its flat gradient buffer grad_flat (the 24 gradient tensors
 * contiguous: w0..w11, b0..b11) — for single-GPU steps, where no all-reduce sits between gradients and update.
 * g_scale (NULL = 1): a DEVICE scalar every g_out is multiplied by inside the chain kernels — the upstream d L / d loss of an
 * autograd backward, applied without a scaling launch.                                                                   */
typedef struct nerfhip_adam_fused {
    int n_models;
    float* param[2];
    float* exp_avg[2];
    float* exp_avg_sq[2];
    const float* grad_flat[2];
    float* state;                 /* {step count, arrival ticket} as for nerfhip_adam_step */
    float lr, beta1, beta2, eps, weight_decay;
} nerfhip_adam_fused;
size_t nerfhip_mlp_dw_workspace_bytes_multi(const int64_t* n_points_host, int n_models, int dtype);
/* The split plan of that launch (host logic only): splits_out[12 m + j] = workgroups of weight-gradient job j (the 12 parameter
 * tensors in state_dict order, reference nerf.py:42-81) of model m; stage_kib_out (NULL ok) = KiB one ring iteration of the job
 * reads.  bf16: workgroups are shared out so that iterations x (fixed cost + cost per KiB) is equal across jobs and models.
 * Returns the number of workgroups (= partial slabs), < 0 on bad arguments.                                                      */
int nerfhip_mlp_dw_plan(const int64_t* n_points_host, int n_models, int dtype, int* splits_out, int* stage_kib_out);
int nerfhip_mlp_bwd_multi(int n_models, const float* const* g_out_host, const float* const* out_host, const int64_t* n_host,
                          const void* const* packed_bwd_host, const void* const* acts_host, void* const* dys_host,
                          void* dw_workspace, float* const* grad_w_host, float* const* grad_b_host, int accumulate, int dtype,
                          int phases, const float* g_scale, const nerfhip_adam_fused* adam, nerfhip_stream_t stream);

/* nerfhip_mlp_bwd_multi for models evaluated ON RAYS (nerfhip_render_train_fwd with regen_enc = 1; NERFHIP_BF16): the
 * weight-gradient launch does not read the positional encodings embedding_xyz(o + d z) / embedding_dir(d) (nerf.py:21-38,
 * rendering.py:186,206-207) from the saved activations — they are the X operand of xyz_encoding_1, of the skip layer and of
 * dir_encoding: 10 of the 282 KiB a 32-point tile is read for — but forms them again from 4 B of depth per point with the forward's
 * own arithmetic (bit-identical operands, so bit-identical gradients).  enc (NULL = nerfhip_mlp_bwd_multi): per model the rays
 * (B,8), the depths z (B,S) the forward evaluated the model at, and S; needs S % 32 == 0 and n = B S a multiple of 256.
 * Measured on MI355X (round 6, same box, alternating): the forward gains 8-10 us of the 1024 x (64+128) step, this launch loses
 * 12-25 — its ring iterations are paced by their instructions, not their bytes — so the Python step leaves it off by default. */
typedef struct nerfhip_enc_source {
    const float* rays[2];
    const float* z[2];
    int S[2];
} nerfhip_enc_source;
int nerfhip_mlp_bwd_multi_rays(int n_models, const float* const* g_out_host, const float* const* out_host, const int64_t* n_host,
                               const void* const* packed_bwd_host, const void* const* acts_host, void* const* dys_host,
                               void* dw_workspace, float* const* grad_w_host, float* const* grad_b_host, int accumulate, int dtype,
                               int phases, const float* g_scale, const nerfhip_adam_fused* adam, const nerfhip_enc_source* enc,
                               nerfhip_stream_t stream);

/* d loss / d x of NeRF.forward on pre-embedded inputs (nerf.py:100-124 is differentiable w.r.t. x): from the dY slabs a
 * nerfhip_mlp_bwd call left in `dys`,  gx[:, 0:63] = W_1^T dY_1 + W_5[:, :63]^T dY_5,  gx[:, 63:90] = W_dir[:, 256:]^T dY_dir.
 * w_xyz1 / w_xyz5 / w_dir: the (out,in) fp32 weights of xyz_encoding_1, xyz_encoding_5, dir_encoding; gx (n, >= 90) with
 * row stride gx_stride floats.  dtype NERFHIP_F32 | NERFHIP_BF16 (NERFHIP_BF16_F8 stores dY too coarsely: unsupported).   */
int nerfhip_mlp_dx_embedded(const void* dys, int64_t n, const float* w_xyz1, const float* w_xyz5, const float* w_dir,
                            float* gx, int64_t gx_stride, int dtype, nerfhip_stream_t stream);

/* ---- a3/a4 for a NON-default NeRF(D, W, in_channels_xyz, in_channels_dir, skips)  (models/nerf.py:42-124) ----
 * The fused kernels above are built for the default shape.  Any other shape runs layer by layer through one MFMA GEMM
 * kernel: activations (n, features) fp32 row-major with a row stride (ld*, in floats; unit column stride), weights (out, in)
 * fp32 row-major with row stride ldw (so a column block of a weight — the two halves of a skip / direction concat,
 * nerf.py:108-109,118 — is addressed by pointer offset + ldw).  dtype: NERFHIP_F32 exact fp32 MFMA; NERFHIP_BF16 and
 * NERFHIP_BF16_F8: operands rounded to bf16, fp32 accumulation.
 *   fwd         y[n, n_out] = act( x[n, n_in] . w[n_out, n_in]^T (+ y when accumulate) (+ bias when non-NULL) )
 *   bwd_input   gx[n, n_in] (+)= (gy * act'(y))[n, n_out] . w[n_out, n_in]        act' from the layer OUTPUT y (ReLU: y > 0;
 *                                                                                 Sigmoid: y (1 - y)); y unused for ACT_NONE
 *   bwd_weight  gw[n_out, n_in] (+)= (gy * act'(y))^T . x;  gb[n_out] (+)= column sums (gb NULL: skipped).  Split over the
 *               points into `workspace` (nerfhip_linear_bwd_weight_workspace_bytes) and reduced in a fixed order.          */
#define NERFHIP_ACT_NONE 0
#define NERFHIP_ACT_RELU 1
#define NERFHIP_ACT_SIGMOID 2
int nerfhip_linear_fwd(const float* x, int64_t ldx, const float* w, int64_t ldw, const float* bias, float* y, int64_t ldy,
                       int64_t n, int n_in, int n_out, int act, int accumulate, int dtype, nerfhip_stream_t stream);
int nerfhip_linear_bwd_input(const float* gy, int64_t ldgy, const float* y, int64_t ldy, int act, const float* w, int64_t ldw,
                             float* gx, int64_t ldgx, int64_t n, int n_in, int n_out, int accumulate, int dtype,
                             nerfhip_stream_t stream);
size_t nerfhip_linear_bwd_weight_workspace_bytes(int64_t n, int n_in, int n_out);
int nerfhip_linear_bwd_weight(const float* gy, int64_t ldgy, const float* y, int64_t ldy, int act, const float* x, int64_t ldx,
                              float* gw, int64_t ldgw, float* gb, void* workspace, int64_t n, int n_in, int n_out,
                              int accumulate, int dtype, nerfhip_stream_t stream);

/* ---- N2. MSELoss.forward + psnr + backward seed  (losses.py:9-14, metrics.py:4-13, train.py:103-117) ----
 * rgb_coarse, rgb_fine (NULL when N_importance == 0), target: n = 3*rays floats each.
 * out3 = [loss, psnr of the fine (else coarse) image, its mse];  g_coarse / g_fine (NULL ok) receive
 * d loss / d rgb = 2 (rgb - target) / n.  One launch, deterministic reduction order.                        */
int nerfhip_mse_psnr(const float* rgb_coarse, const float* rgb_fine, const float* target, int64_t n, float* out3,
                     float* g_coarse, float* g_fine, nerfhip_stream_t stream);

/* ---- N2. Adam on flat parameter storage  (utils/__init__.py:10-30 -> torch.optim.Adam(lr, eps=1e-8, weight_decay)) ----
 * One launch over `n_tensors` (<= 8) flat fp32 tensors: params/grads/exp_avg/exp_avg_sq are HOST arrays of DEVICE
 * pointers, numel_host their element counts.  `state` is a 2-float DEVICE buffer {step count, arrival ticket},
 * zero-initialised by the caller; the kernel uses t = state[0] + 1 for the bias corrections and advances state[0]
 * itself (device-resident step => hipGraph replays keep counting).  Non-amsgrad, L2 weight decay (g += wd * p).      */
int nerfhip_adam_step(float* const* params_host, const float* const* grads_host, float* const* exp_avg_host,
                      float* const* exp_avg_sq_host, const int64_t* numel_host, int n_tensors, float* state, float lr,
                      float beta1, float beta2, float eps, float weight_decay, nerfhip_stream_t stream);

/* ---- N2b. RAdam and Ranger on the same flat storage  (utils/__init__.py:21-26 -> utils/optimizers.py:6-95 RAdam,
 * :266-405 Ranger = RAdam + lookahead) ----
 * Same conventions as nerfhip_adam_step: HOST arrays of `n_tensors` (<= 8) DEVICE pointers, the same 2-float DEVICE `state`
 * {step count, arrival ticket} advanced by the launch itself, one launch for all tensors, nothing allocated or synchronised
 * (capturable).  Hyper-parameters are doubles: the rectification term N_sma(t) and the step size are formed in double on the
 * device, as the reference forms them in Python floats (fp32 cannot resolve N_sma(5) = 4.996 against RAdam's threshold 5).
 * Weight decay is NOT folded into the gradient (p -= wd lr p), eps is added to sqrt(exp_avg_sq) directly; both moments are
 * updated on every step.
 *   RAdam  (optimizers.py:62-93): rectified update when N_sma >= 5; below it the momentum-only form when degenerated_to_sgd,
 *          else the parameters (weight decay included) are left untouched.
 *   Ranger (optimizers.py:369-403): rectified when N_sma > n_sma_threshold, momentum-only form otherwise; weight decay always;
 *          when t % k == 0 the lookahead step slow += alpha (p - slow), p = slow follows.  `slow_host`: flat DEVICE tensors like
 *          params.  The launch with t = 1 fills them from the parameters before it updates those (optimizers.py:353-354); other
 *          launches neither read nor write them unless t % k == 0.
 * NERFHIP_E_BADARG: null pointers, n_tensors outside 1..8, numel < 1, lr / eps / weight_decay < 0, a beta outside [0, 1),
 * k < 1, alpha outside [0, 1].                                                                                          */
int nerfhip_radam_step(float* const* params_host, const float* const* grads_host, float* const* exp_avg_host,
                       float* const* exp_avg_sq_host, const int64_t* numel_host, int n_tensors, float* state, double lr,
                       double beta1, double beta2, double eps, double weight_decay, int degenerated_to_sgd,
                       nerfhip_stream_t stream);
int nerfhip_ranger_step(float* const* params_host, const float* const* grads_host, float* const* exp_avg_host,
                        float* const* exp_avg_sq_host, const int64_t* numel_host, int n_tensors, float* state,
                        float* const* slow_host, double alpha, int k, double n_sma_threshold, double lr, double beta1,
                        double beta2, double eps, double weight_decay, nerfhip_stream_t stream);

/* ---- N1. ray generation  (datasets/ray_utils.py:5-94; consumers blender.py:37-69, llff.py:236-253) --------
 * get_ray_directions: dirs (H,W,3) = ((i-W/2)/focal, -(j-H/2)/focal, -1), i = column, j = row.
 * get_rays: rays_d = normalise(directions @ c2w[:, :3].T), rays_o = c2w[:, 3]; c2w (3,4) row-major DEVICE array.
 * get_ndc_rays: shift to the near plane and project (forward-facing LLFF scenes).  `focal` is a double: the
 * reference forms -1/(W/(2 focal)) in Python double precision before it meets the fp32 tensors.                */
int nerfhip_ray_directions(float* dirs, int H, int W, double focal, nerfhip_stream_t stream);
int nerfhip_get_rays(const float* directions, const float* c2w, float* rays_o, float* rays_d, int64_t n,
                     nerfhip_stream_t stream);
int nerfhip_ndc_rays(int H, int W, double focal, float near, const float* rays_o, const float* rays_d, float* out_o,
                     float* out_d, int64_t n, nerfhip_stream_t stream);
/* All of the above fused, for a batch of pixels: rays (n,8) = [o d near far] of global pixel ids
 * `pixel_ids[r]` = image*H*W + row*W + col (or first_pixel + r when pixel_ids is NULL) under poses
 * c2w (n_images,3,4); use_ndc applies get_ndc_rays with the near plane at ndc_near_plane (llff.py uses 1.0). */
int nerfhip_gen_rays(const float* c2w, const int64_t* pixel_ids, int64_t first_pixel, int64_t n, int H, int W,
                     double focal, float near, float far, int use_ndc, float ndc_near_plane, float* rays,
                     nerfhip_stream_t stream);
/* A training batch in one launch (the reference's Dataset.__getitem__ + DataLoader collate, blender.py:81-84 /
 * train.py:89-94): rays as nerfhip_gen_rays for the n pixel ids, and rgbs (n,3) = rgbs_all[pixel_ids] gathered from the
 * device-resident pixel colours rgbs_all (n_images*H*W, 3).                                                      */
int nerfhip_sample_batch(const float* c2w, const int64_t* pixel_ids, const float* rgbs_all, int64_t n, int H, int W,
                         double focal, float near, float far, int use_ndc, float ndc_near_plane, float* rays, float* rgbs,
                         nerfhip_stream_t stream);

/* ---- the random draws of a training step, as torch's generator would make them  (rendering.py:203,152,39,152; the
 * DataLoader's batch of train.py:89-94) ----
 * ONE launch producing up to 6 tensors from the Philox4x32-10 stream that torch.rand / torch.randn / torch.randint on the GPU
 * consume: draw i is what the i-th of those torch calls would return for a generator at (seed, offset), bit for bit, and
 * *increment_host is what the calls together advance the generator's offset by (the caller then sets the generator to
 * offset + increment: same seed => same training run, whichever path draws).  max_blocks = multiProcessorCount *
 * (maxThreadsPerMultiProcessor / 256) of the device (ATen's launch cap; 2048 on MI355X).
 *   kind UNIFORM: out = numel floats of torch.rand; NORMAL: torch.randn; RANDINT: numel int64 of torch.randint(0, range)
 *   (range <= 2^62).  A draw with out == NULL (and no batch) is one nobody reads — the reference always draws its noise tensors,
 *   also when noise_std == 0 (rendering.py:152): the stream moves past it exactly as the torch call would, nothing is computed.
 * batch_host (NULL ok): draws_host[0] must then be RANDINT over the store's pixel ids; the drawn ids are turned into the
 * training batch in the same launch — rays (numel,8) and rgbs (numel,3) exactly as nerfhip_sample_batch — and draws_host[0].out
 * may be NULL (the ids themselves are then not stored).
 * state (NULL ok): a DEVICE buffer of 4 x uint64 {seed, offset, arrival ticket (0), -}.  When given, seed / offset are read
 * from it instead of the arguments and its offset is advanced by the increment at the end of the launch, so that hipGraph
 * replays of one captured call keep walking the stream.                                                                  */
#define NERFHIP_DRAW_UNIFORM 0
#define NERFHIP_DRAW_NORMAL 1
#define NERFHIP_DRAW_RANDINT 2
typedef struct nerfhip_draw {
    int kind;
    int64_t numel;
    void* out;
    uint64_t range;
} nerfhip_draw;
typedef struct nerfhip_ray_batch {
    const float* c2w;       /* (n_images,3,4) poses */
    const float* rgbs_all;  /* (n_images*H*W,3) pixel colours, or NULL (then rgbs NULL too) */
    float* rays;            /* (numel,8) out, 16-byte aligned */
    float* rgbs;            /* (numel,3) out */
    int H, W;
    double focal;
    float near, far;
    int use_ndc;
    float ndc_near_plane;
} nerfhip_ray_batch;
uint64_t nerfhip_torch_draw_increment(int64_t numel, int max_blocks);
int nerfhip_torch_draws(const nerfhip_draw* draws_host, int n_draws, const nerfhip_ray_batch* batch_host, uint64_t seed,
                        uint64_t offset, uint64_t* state, int max_blocks, uint64_t* increment_host, nerfhip_stream_t stream);

/* The prologue of a training step in ONE launch: nerfhip_torch_draws (same arguments: the batch, its rays, the step's draws) and
 * nerfhip_mlp_pack_weights_train_multi (same arguments: both images of n_models models) — the two jobs of the step that depend
 * only on the generator state and on the parameters.  Same device code as the two launches, same results.                     */
int nerfhip_train_prologue(const nerfhip_draw* draws_host, int n_draws, const nerfhip_ray_batch* batch_host, uint64_t seed,
                           uint64_t offset, uint64_t* state, int max_blocks, uint64_t* increment_host,
                           const float* const* weights_host, const float* const* biases_host, void* const* packed_host,
                           void* const* packed_bwd_host, int n_models, int dtype, nerfhip_stream_t stream);

/* ---- render_rays in ONE launch  (models/rendering.py:58-244; SURVEY 8b "_render_fwd fused: 32 B in + 40 B out per ray") ----
 * The whole pipeline of one `render_rays` call — coarse depths (:183-204), coarse MLP over o + d z (:206-217), compositing
 * (:143-172), sample_pdf + sort (:223-229), fine MLP, compositing — by workgroups that own 4 whole rays each: the MLP runs as
 * sub-passes of nerfhip_mlp_fwd_rays' own network code, the rays' compositing and fine depths by the same workgroup in between
 * (same device code, hence the same bits, as nerfhip_mlp_fwd_rays_coarse -> nerfhip_composite_fwd -> nerfhip_fine_z_ex ->
 * nerfhip_mlp_fwd_rays -> nerfhip_composite_fwd).  The coarse pass always evaluates the full network (`test_time`'s
 * sigma-only shortcut changes no value: pass rgb_coarse = depth_coarse = NULL to drop what the reference does not return).
 * The per-point intermediates z_* / raw_* are caller-owned buffers (outputs for whoever wants them; they stay in L2 between the
 * sub-passes that write and read them).
 * Shapes the kernels take (nerfhip_render_supported): B % 4 == 0, 4 S_c and 4 (S_c + N_i) multiples of the points per
 * sub-pass (256 for bf16, 128 for fp32), S_c >= 3; N_i == 0 renders the coarse pass only.  z_* / raw_* / g_raw_* must be
 * 128-byte aligned (a group's slice of each is then whole cache lines), packed_* 16-byte aligned.                            */
typedef struct nerfhip_render_args {
    const float* rays;          /* (B,8) */
    int64_t B;
    int S_c, N_i;               /* N_samples, N_importance */
    const void* packed_coarse;  /* nerfhip_mlp_pack_weights images of the two models (fine unused when N_i == 0) */
    const void* packed_fine;
    float* z_coarse;            /* (B,S_c)        out */
    float* raw_coarse;          /* (B,S_c,4)      out: [r g b sigma] per coarse point */
    float* z_fine;              /* (B,S_c+N_i)    out */
    float* raw_fine;            /* (B,S_c+N_i,4)  out */
    void* save_coarse;          /* training: nerfhip_mlp_act_bytes(B S_c) / (B (S_c+N_i)) bytes of saved activations */
    void* save_fine;
    const float* perturb_rand;  /* (B,S_c) uniforms when perturb > 0, else NULL                    rendering.py:203 */
    float perturb;
    int use_disp;
    const float* noise_coarse;  /* (B,S_c) / (B,S_c+N_i) standard-normal draws, read when noise_std != 0      :152 */
    const float* noise_fine;
    float noise_std;
    int white_back;
    const float* u;             /* (B,N_i) uniforms (row stride u_stride), or NULL = deterministic linspace    :36-39 */
    int64_t u_stride;
    float eps;                  /* sample_pdf's eps (1e-5) */
    int row_total;              /* NERFHIP_ROW_TOTAL_* */
    float* rgb_coarse;          /* (B,3)  NULL ok */
    float* depth_coarse;        /* (B)    NULL ok */
    float* opacity_coarse;      /* (B) */
    float* rgb_fine;            /* (B,3) (B) (B); unused when N_i == 0 */
    float* depth_fine;
    float* opacity_fine;
    /* training forward only */
    const float* target;        /* (B,3) */
    float grad_scale;           /* 2 / (3 B) */
    float* g_raw_coarse;        /* (B,S_c,4)      out: d loss / d raw */
    float* g_raw_fine;          /* (B,S_c+N_i,4)  out */
    float* out3;                /* [loss, psnr, mse] */
    uint32_t* ticket;           /* one zero-initialised device word owned by the caller; left at zero */
    int regen_enc;              /* nerfhip_render_train_fwd, NERFHIP_BF16 only (ignored otherwise): 1 = the input-encoding slabs (6 of a
                                 * tile block's 151 KiB) are NOT saved; the backward must then be nerfhip_mlp_bwd_multi_rays with
                                 * these rays and z_coarse / z_fine, which forms them again                                     */
} nerfhip_render_args;
/* 1 when the single-launch kernels take this shape and arithmetic (dtype NERFHIP_F32 / NERFHIP_BF16 / NERFHIP_BF16_F8), else 0 */
int nerfhip_render_supported(int64_t B, int S_c, int N_i, int dtype);
/* inference: rgb / depth / opacity of both passes (the training-only fields are ignored) */
int nerfhip_render_fwd(const nerfhip_render_args* args_host, int dtype, nerfhip_stream_t stream);
/* inference under test_time (rendering.py:209-213; what eval.py:69-79 asks for): the coarse network stops at its density head
 * (nerf.py:112-114 sigma_only), so raw_coarse is (B,S_c) — sigma alone — and the coarse pass leaves opacity_coarse only
 * (rgb_coarse / depth_coarse are ignored); N_i > 0.  Bit-identical to nerfhip_mlp_fwd_rays_coarse(sigma_only) ->
 * nerfhip_composite_fwd -> nerfhip_fine_z -> nerfhip_mlp_fwd_rays -> nerfhip_composite_fwd.                                    */
int nerfhip_render_test_fwd(const nerfhip_render_args* args_host, int dtype, nerfhip_stream_t stream);
/* The forward of a training step (train.py:103-117 up to the loss) in ONE launch: the above with the activations saved for
 * nerfhip_mlp_bwd_multi, and per pass what nerfhip_composite_train_fine_z / nerfhip_composite_train_loss append to the
 * quadrature — d MSE / d rgb, the compositing backward (g_raw_*), loss / PSNR / MSE (out3, reduced by the last workgroup to
 * finish in nerfhip_mse_psnr's own order).  Bit-identical to those launches.                                                 */
int nerfhip_render_train_fwd(const nerfhip_render_args* args_host, int dtype, nerfhip_stream_t stream);

/* ---- mesh extraction  (extract_color_mesh.py:144-285; nerf_pl_amd/mesh.py, DESIGN.md "Mesh extraction") -----------------
 * Marching cubes on a dense float32 volume (n0,n1,n2), C order, every dimension >= 2, n0*n1*n2 < 2^31.  Bourke's tables: case
 * bit i set where corner i is below `iso` (compared in fp64).  One vertex per crossed lattice edge (shared by every triangle on
 * it) at a + t, t = (iso - f_a) / (f_b - f_a) in fp64 (0.5 when f_a == f_b), ordered by (owning lattice point in C order, edge
 * axis); triangles ordered by (cell in C order, table order).  Deterministic.  Two calls on one workspace:
 *   count  writes totals[0] = V, totals[1] = T (int64, DEVICE);
 *   emit   the caller reads the totals, refuses V or T >= 2^31 (emit then writes nothing) and passes vertices (V,3) fp64 and
 *          triangles (T,3) int32.                                                                                          */
size_t nerfhip_marching_cubes_workspace_bytes(int64_t n0, int64_t n1, int64_t n2);   /* 0: unsupported shape */
int nerfhip_marching_cubes_count(const float* volume, int64_t n0, int64_t n1, int64_t n2, double iso, void* workspace,
                                 int64_t* totals, nerfhip_stream_t stream);
int nerfhip_marching_cubes_emit(const float* volume, int64_t n0, int64_t n1, int64_t n2, double iso, void* workspace,
                                const int64_t* totals, double* vertices, int32_t* triangles, nerfhip_stream_t stream);

/* Largest edge-connected triangle cluster (open3d cluster_connected_triangles + argmax + remove_unreferenced_vertices).
 * keys (3T) int64: (min << 32 | max) of every triangle's edges (t, 0-1), (t, 1-2), (t, 2-0) at 3t..3t+2.  The caller sorts them
 * (sorted_keys, order = the permutation as int64) and calls largest_cluster, which writes totals[0] = kept triangles,
 * totals[1] = kept vertices, totals[2] = nonzero on failure; then compact writes kept_vertex_ids (totals[1]) int64 (old ids,
 * ascending) and kept_triangles (totals[0],3) int32 (surviving triangles in order, remapped).  Ties between clusters of equal
 * size go to the one holding the lowest triangle id.  Every vertex id must lie in [0, V).                                  */
int nerfhip_mesh_edge_keys(const int32_t* triangles, int64_t T, int64_t* keys, nerfhip_stream_t stream);
size_t nerfhip_mesh_cluster_workspace_bytes(int64_t V, int64_t T);
int nerfhip_mesh_largest_cluster(const int32_t* triangles, int64_t V, int64_t T, const int64_t* sorted_keys, const int64_t* order,
                                 void* workspace, int64_t* totals, nerfhip_stream_t stream);
int nerfhip_mesh_cluster_compact(const int32_t* triangles, int64_t V, int64_t T, void* workspace, int64_t* kept_vertex_ids,
                                 int32_t* kept_triangles, nerfhip_stream_t stream);

/* Vertex normals by open3d's rule: sum of unnormalised face cross products (v1-v0)x(v2-v0) in fp64 (atomic, so the last bits
 * follow the summation order), normalised; zero-length -> (0,0,1).  vertices (V,3) float32 -> normals (V,3) fp64.           */
int nerfhip_mesh_vertex_normals(const float* vertices, int64_t V, const int32_t* triangles, int64_t T, double* normals,
                                nerfhip_stream_t stream);
/* extract_color_mesh.py:190-195: rays (V,8) = [v - d*near*near_t, d, near, far], d = float32(normal).                      */
int nerfhip_mesh_normal_rays(const float* vertices, const double* normals, int64_t V, float near, float far, float near_t,
                             float* rays, nerfhip_stream_t stream);
/* One view of extract_color_mesh.py:223-264.  w2c_host: 12 HOST floats (top rows of the float32 inverse of the 4x4 c2w),
 * origin_host: 3 HOST floats (the pose's last column).  Projection in fp64 with y, z negated, K = [[f,0,W/2],[0,f,H/2],[0,0,1]],
 * depth = z + 1e-5, pixel = float32(xy / depth) clipped to [0,W-1] x [0,H-1]; image (H,W,3) uint8 sampled as cv2.remap
 * INTER_LINEAR does (1/32 px positions, 15-bit weights).  Writes colors (V,4) uint8 (4th byte 0), depth (V) fp64 and the
 * occlusion rays (V,8) = [camera centre, normalised direction, near, float32(depth)].                                    */
int nerfhip_mesh_view_rays(const float* vertices, int64_t V, const float* w2c_host, const float* origin_host, float focal, int W,
                           int H, const uint8_t* image, float near, uint8_t* colors, double* depth, float* rays,
                           nerfhip_stream_t stream);
/* accum (V,4) fp64 += [colour * w, w], w = 0.1 / depth + (opacity < occ_threshold), NaN opacity counted as 0.             */
int nerfhip_mesh_color_accumulate(const uint8_t* colors, const double* depth, const float* opacity, int64_t V,
                                  float occ_threshold, double* accum, nerfhip_stream_t stream);
/* out (V,3) uint8 = trunc(accum[:, :3] / accum[:, 3])                                                                     */
int nerfhip_mesh_color_finish(const double* accum, int64_t V, uint8_t* out, nerfhip_stream_t stream);
/* out (n) uint8 = trunc(float32(rgb * 255)): the vertex-normal mode's colours (extract_color_mesh.py:279)                  */
int nerfhip_mesh_rgb_to_u8(const float* rgb, int64_t n, uint8_t* out, nerfhip_stream_t stream);

/* ---- Unity volume file  (extract_mesh.ipynb, cell "Generate .vol file for volume rendering in Unity"; nerf_pl_amd/volume.py,
 * DESIGN.md "Volume export") ------------------------------------------------------------------------------------------------
 * The notebook's pack, for the points first_index .. first_index+n-1 of a lattice whose full-network output is rgbsigma (n,4)
 * float32 (16-byte aligned), neg_cell = float32(-(xmax - xmin) / N):
 *     sigma = np.maximum(rgbsigma[:, -1], 0);  a = 1 - np.exp(-(xmax-xmin)/N*sigma)      t = neg_cell * sigma (one fp32 multiply),
 *                                                                                        a = 1.0f - (float)exp((double)t)
 *     i = np.where(a > 0)[0]                                                             kept iff a > 0 (NaN, sigma <= 0: dropped)
 *     rgb = (rgbsigma[:, :3].numpy()*255).astype(np.uint32)                              one fp32 multiply, truncated, clamped 0..255
 *     s = rgb.dot([1<<24, 1<<16, 1<<8]) + (a*255).astype(np.uint32)                      R<<24 | G<<16 | B<<8 | A
 *     res = np.stack([i, s], -1).astype(np.uint32)                                       records (index, s), increasing index
 * The kept records are appended at records[2 * (*cursor)] onward (records 8-byte aligned, room for `capacity` records) and the
 * DEVICE int64 *cursor is advanced by the kept count, so a lattice packed in chunks needs no host round trip.  A record that
 * would land at or beyond `capacity` is not written; the cursor still advances by the full count (overflow shows there).
 * Three launches (count, one-workgroup scan, emit) on `stream`; nothing is allocated, nothing synchronises.  n == 0 is success
 * and launches nothing; n < 0, capacity < 0, first_index < 0, first_index + n > 2^32 and null pointers with n > 0 are
 * NERFHIP_E_BADARG.  workspace: nerfhip_vol_workspace_bytes(n) bytes, 8-byte aligned (0 for n < 0 or n > 2^32).               */
size_t nerfhip_vol_workspace_bytes(int64_t n);
int nerfhip_vol_pack(const float* rgbsigma, int64_t n, int64_t first_index, float neg_cell, void* workspace, uint32_t* records,
                     int64_t capacity, int64_t* cursor, nerfhip_stream_t stream);

/* ---- scene loading  (datasets/blender.py:47-58,90-95; nerf_pl_amd/datasets, DESIGN.md "Scene loading") -----------------------
 * What the reference does per image on the host with PIL and torchvision, on byte images in HBM.  All three: n == 0 is success;
 * null pointers with n > 0, sizes < 0 and unsupported channel counts are NERFHIP_E_BADARG before anything is launched.
 *
 * png_unfilter: reverses the PNG scanline filters 0-4 (None, Sub, Up, Average, Paeth; arithmetic modulo 256, Paeth ties a, b, c)
 * of n_images inflated IDAT streams of equal size: 8-bit, non-interlaced, ch = 1 | 3 | 4, each H x (1 + W ch) bytes, back to
 * back.  out (n_images,H,W,ch) uint8 (4-byte aligned when ch == 4).  error_flags (n_images) int32: written by the launch, nonzero
 * where a scanline names a filter above 4 (such a line is copied as if unfiltered; no address depends on the filter byte).     */
int nerfhip_png_unfilter(const uint8_t* streams, uint8_t* out, int32_t* error_flags, int n_images, int H, int W, int ch,
                         nerfhip_stream_t stream);
/* PIL.Image.resize((out_w, out_h), Image.LANCZOS) of n_images 8-bit RGBA images (n,in_h,in_w,4) -> (n,out_h,out_w,4), byte for
 * byte: premultiply by alpha, a horizontal pass (when the width changes) into an 8-bit intermediate, a vertical pass (when the
 * height changes), un-premultiply; equal sizes copy.  Per changed axis the caller supplies Pillow's taps as DEVICE int32 tables:
 * xmin (out), count (out) and taps (out, ksize) in 22-bit fixed point (formed in double on the host:
 * nerf_pl_amd.imageio_min.lanczos_taps).  A window reaching outside the input is clamped to it.  workspace: in_h * out_w * 4
 * bytes per image, needed when both axes change (else NULL ok).  in / out / workspace 4-byte aligned and distinct.            */
int nerfhip_resize_rgba_lanczos(const uint8_t* in, uint8_t* out, uint8_t* workspace, int n_images, int in_h, int in_w, int out_h,
                                int out_w, const int32_t* xmin_h, const int32_t* count_h, const int32_t* taps_h, int ksize_h,
                                const int32_t* xmin_v, const int32_t* count_v, const int32_t* taps_v, int ksize_v,
                                nerfhip_stream_t stream);
/* ToTensor + the blend onto white (blender.py:56-58,93): f = byte / 255 (fp32 division), rgb (n,3) = f_c * f_a + (1 - f_a) with
 * the product, the difference and the sum rounded separately; valid_mask (n) uint8 = alpha > 0 (NULL ok).  rgba (n,4) uint8,
 * 4-byte aligned; rgb may point into a larger (pixels,3) array, so a scene's colours are assembled in place.                  */
int nerfhip_rgba_to_rgb_white(const uint8_t* rgba, float* rgb, uint8_t* valid_mask, int64_t n, nerfhip_stream_t stream);

/* ---- JPEG decoding  (datasets/llff.py:226,312 `Image.open(p).convert('RGB')`; DESIGN.md "Scene loading") ---------------------
 * Baseline sequential DCT, 8 bits, Huffman-coded, one interleaved scan; 1 component, or 3 (YCbCr) with luma sampling hs x vs =
 * 1x1, 2x1 or 2x2 and chroma 1x1.  The results equal the bytes of Pillow's libjpeg-turbo with its defaults (islow inverse DCT,
 * fancy upsampling).  The host parses the markers (nerf_pl_amd.imageio_min.jpeg_parse).
 *
 * jpeg_entropy_decode: HOST function — host pointers only, no GPU, launches nothing.  Huffman-decodes the entropy-coded segment
 * `scan` (scan_bytes bytes, from behind the SOS header up to, not including, the marker that ends it; stuffed zeros and RSTm
 * markers still inside) into coefficient blocks: coef[c] receives component c's blocks in raster order over
 * (mcus_y * v_c) x (mcus_x * h_c) blocks, 64 int16 each in natural (row-major) order, DC prediction resolved, not dequantised.
 * comp (n_comp,4) int32 = h, v, DC table id, AC table id per component.  huffman: 8 tables of 272 bytes (16 code-length counts +
 * 256 symbols), table index = 4 * class + id; bit t of huffman_mask says table t is defined.  coef_blocks[c]: capacity of
 * coef[c] in blocks.  restart_interval in MCUs, 0 = none.  Every read of `scan` and write of `coef` is bounds-checked:
 * NERFHIP_E_DATA for a truncated or invalid stream, a table that is no prefix code or is missing, or a wrong restart marker;
 * NERFHIP_E_BADARG for null / non-positive / too small arguments.                                                              */
int nerfhip_jpeg_entropy_decode(const uint8_t* scan, int64_t scan_bytes, int n_comp, const int32_t* comp, const uint8_t* huffman,
                                int huffman_mask, int mcus_x, int mcus_y, int restart_interval, int16_t* const* coef,
                                const int64_t* coef_blocks);
/* Bytes of the 8-bit component planes of one image (workspace of jpeg_decode); 0 for an unsupported size or sampling.          */
size_t nerfhip_jpeg_planes_bytes(int H, int W, int n_comp, int hs, int vs);
/* Device: n_images images of one size and sampling, two launches.  coef_* (n_images, blocks_c, 64) int16 as the entropy decoder
 * leaves them (coef_cb / coef_cr NULL when n_comp == 1), quant (n_images, n_comp, 64) uint16 in natural order.  Launch 1:
 * dequantise, libjpeg's integer "islow" inverse DCT (13-bit constants, 2 extra bits after the column pass), +128 and range limit
 * -> planes (n_images * jpeg_planes_bytes).  Launch 2: libjpeg-turbo's triangle ("fancy") chroma upsampling for 2x1 and 2x2 —
 * plain replication where the chroma plane is at most 2 samples wide —, its 16-bit fixed-point YCbCr -> RGB, crop -> out
 * (n_images,H,W,4) uint8 with byte 3 = 255.  coef_* and quant 16-byte, planes 8-byte, out 4-byte aligned (NERFHIP_E_ALIGN).     */
int nerfhip_jpeg_decode(const int16_t* coef_y, const int16_t* coef_cb, const int16_t* coef_cr, const uint16_t* quant,
                        uint8_t* planes, uint8_t* out, int n_images, int H, int W, int n_comp, int hs, int vs,
                        nerfhip_stream_t stream);

/* ---- Huffman-decoding the scans on the device  (DESIGN.md "Scene loading": the entropy stage on the GPU) ----------------------
 * A batch of n_images baseline scans of one frame size and sampling goes up as the files' bytes and comes out as the coefficient
 * tensors jpeg_decode takes, bit-equal to jpeg_entropy_decode's.  The stream of every restart interval is cut into subsequences
 * of subseq_bits bits, one thread each; threads carry their exit state (bit position, block inside the MCU, zigzag index) on
 * into the following subsequences until the records agree (self-synchronisation).  The Huffman tables are built on the device
 * from the same 272-byte definitions the host entry takes.
 *
 * All pointers of the batch are device pointers, `comp` excepted, which sits in the struct:
 *   scans              the scans' bytes back to back (total_bytes of them; read byte by byte, no padding needed)
 *   offsets            (n_images + 1) int64, 8-byte aligned: scan i is [offsets[i], offsets[i + 1])
 *   huffman            (n_images, 8, 272) uint8 and huffman_masks (n_images) int32, as jpeg_entropy_decode's
 *   restart_intervals  (n_images) int32, in MCUs, 0 = none: the files of a batch may differ in it
 *   max_scan_bytes     at least the longest scan (1 .. 2^28); max_intervals: at least the most restart intervals of any image,
 *                      ceil(mcus_x * mcus_y / restart_interval), 1 without restarts.  Both size the workspace and the grids; an
 *                      image that exceeds either, or whose offsets are not increasing inside total_bytes, gets status BADARG.
 *   comp               (n_comp, 4) int32 = h, v, DC table id, AC table id, as jpeg_entropy_decode's; at most 6 blocks per MCU
 *   subseq_bits        a multiple of 32 in 32 .. 4096
 *   workspace          jpeg_entropy_workspace_bytes(...) bytes, 256-byte aligned (NERFHIP_E_ALIGN); it carries the state from
 *                      jpeg_entropy_sync over jpeg_entropy_rounds to jpeg_entropy_emit
 *   status             (n_images) int32, written by sync and emit: 0, NERFHIP_E_DATA (a truncated scan, an invalid code, a size or
 *                      index out of range, a wrong or missing RSTm marker, a table that is no prefix code or is missing: whatever
 *                      jpeg_entropy_decode refuses) or NERFHIP_E_BADARG.  The other images of the batch are not affected.
 *   progress           one int32: the number of the last round between workgroups that changed a record (0: none since the
 *                      passes inside the workgroups).  The records are final once a round has run that changed nothing, i.e.
 *                      when progress < the number of the last round enqueued; (workgroups + 1) rounds always suffice.
 * Nothing allocates or synchronises; arguments are validated before anything is launched (NERFHIP_E_BADARG / NERFHIP_E_ALIGN).
 *   jpeg_entropy_workgroups  workgroups (of 256 subsequences) per image for these sizes: the bound of the host's loop; 0 = refused
 *   jpeg_entropy_sync        prepare (classify and compact the bytes, cut at the RSTm markers, build the tables), the passes
 *                            inside every workgroup, then rounds 1 .. `rounds` (0 .. 64) between workgroups
 *   jpeg_entropy_rounds      rounds first_round .. first_round + rounds - 1; a round returns at once when the one before
 *                            changed nothing
 *   jpeg_entropy_emit        block offsets, the second decode from the true entry states into coef_* (n_images, blocks_c, 64)
 *                            int16, which the caller has zeroed (coef_cb / coef_cr NULL when n_comp == 1), DC differences ->
 *                            DC values.  An image whose status is not 0 is left with undefined coefficients.
 * The caller reads status and progress between sync / rounds and emit (one synchronisation per batch), and enqueues more rounds
 * while progress says so.
 *
 * jpeg_entropy_decode_split: HOST function — host pointers only (also workspace, status, progress), no GPU, launches nothing.  The
 * same arguments, the same four steps with the same per-symbol code over the same subsequences, the threads of a workgroup and
 * the workgroups of a round in lockstep.  It exists so that the algorithm, its bounds and its error paths can be tested and run
 * under a sanitizer on a machine without a GPU.  Returns 0 when it ran (the images' results are in status).                      */
typedef struct nerfhip_jpeg_batch {
    const uint8_t* scans;
    const int64_t* offsets;
    const uint8_t* huffman;
    const int32_t* huffman_masks;
    const int32_t* restart_intervals;
    int64_t total_bytes;
    int64_t max_scan_bytes;
    int32_t max_intervals;
    int32_t n_images;
    int32_t n_comp;
    int32_t comp[12];
    int32_t mcus_x, mcus_y;
    int32_t subseq_bits;
    void* workspace;
    int32_t* status;
    int32_t* progress;
} nerfhip_jpeg_batch;
size_t nerfhip_jpeg_entropy_workspace_bytes(int n_images, int64_t max_scan_bytes, int max_intervals, int subseq_bits);
int nerfhip_jpeg_entropy_workgroups(int64_t max_scan_bytes, int max_intervals, int subseq_bits);
int nerfhip_jpeg_entropy_sync(const nerfhip_jpeg_batch* batch, int rounds, nerfhip_stream_t stream);
int nerfhip_jpeg_entropy_rounds(const nerfhip_jpeg_batch* batch, int first_round, int rounds, nerfhip_stream_t stream);
int nerfhip_jpeg_entropy_emit(const nerfhip_jpeg_batch* batch, int16_t* coef_y, int16_t* coef_cb, int16_t* coef_cr,
                              nerfhip_stream_t stream);
int nerfhip_jpeg_entropy_decode_split(const nerfhip_jpeg_batch* batch, int16_t* coef_y, int16_t* coef_cb, int16_t* coef_cr);

/* ---- scoring and logging rendered images  (metrics.py:15-20, utils/visualization.py:6-17; DESIGN.md "Image metrics") ---------
 * ssim: the reference's `metrics.ssim` = 1 - 2 * kornia.losses.ssim(img1, img2, window_size, reduction) as kornia 0.2.0 defines
 * it.  Window: outer product of g[i] = exp(-(i - ws/2)^2 / (2 * 1.5^2)) normalised to sum 1; depth-wise filter with zero padding
 * (ws - 1) / 2 (the padded zeros take part in every mean); per pixel and channel, with mu = filt(x), s11 = filt(x1^2) - mu1^2,
 * s22 = filt(x2^2) - mu2^2, s12 = filt(x1 x2) - mu1 mu2, C1 = 0.01^2, C2 = 0.03^2:
 *     m = (2 mu1 mu2 + C1)(2 s12 + C2) / ((mu1^2 + mu2^2 + C1)(s11 + s22 + C2)),   value = 1 - 2 * (clamp(1 - m, 0, 1) / 2).
 * The second moments are formed on images centred per 32 x 32 tile, so they do not cancel (flat images are exact where the
 * reference's own fp32 arithmetic is off by up to 1.5e-3).  img1, img2: B images of C channels, H x W, `layout` planar (B,C,H,W)
 * or interleaved (B,H,W,C) (a renderer's (H*W,3) colours: B = 1, C = 3).  map: the values in the images' layout, or NULL.
 * mean: one DEVICE float, or NULL; deterministic (per-tile fp64 sums in `workspace`, folded in index order by a second launch).
 * workspace: ssim_workspace_bytes(B,C,H,W) bytes, 8-byte aligned; needed for `mean` only.  window_size odd, 3..11.
 * B*C*H*W == 0 is success; a null image with elements to read, another window_size or layout, or more than 2^31 - 1 tiles is
 * NERFHIP_E_BADARG before anything is launched.                                                                              */
#define NERFHIP_IMAGE_PLANAR 0
#define NERFHIP_IMAGE_INTERLEAVED 1
size_t nerfhip_ssim_workspace_bytes(int B, int C, int H, int W);
int nerfhip_ssim(const float* img1, const float* img2, int B, int C, int H, int W, int window_size, int layout, float* map,
                 float* mean, void* workspace, nerfhip_stream_t stream);
/* visualize_depth: x = nan_to_num(depth) (NaN -> 0, +-inf -> +-FLT_MAX), mi / ma = its minimum / maximum over the n pixels (never
 * read by the host), x = (x - mi) / (ma - mi + 1e-8f) with every operation rounded to fp32 as numpy does, index = trunc(255 x) as
 * uint8 (a NaN quotient -> 0).  table: 256 x 3 DEVICE bytes; out_chw (3,n) float32 = table[index][k] / 255 (fp32 division, as
 * ToTensor), out_hwc (n,3) uint8 = table[index][k]; either may be NULL.  The reference hands cv2's BGR image to PIL as RGB, so
 * its channel 0 is the colour map's blue: a table holds a colour's bytes in OUTPUT channel order.  Two launches.
 * workspace: depth_colormap_workspace_bytes(n) bytes, 4-byte aligned.  n == 0 is success.                                     */
size_t nerfhip_depth_colormap_workspace_bytes(int64_t n);
int nerfhip_depth_colormap(const float* depth, int64_t n, const uint8_t* table, float* out_chw, uint8_t* out_hwc, void* workspace,
                           nerfhip_stream_t stream);

/* ---- animated GIF  (eval.py:145 `imageio.mimsave(f'{scene_name}.gif', imgs, fps=30)`) -------------------------
 * Per frame its own 256-entry palette; all arithmetic is integer and the result is a pure function of the frames (DESIGN.md §13
 * holds the definition, tests/gif_ref.py restates it in numpy).  F frames of H x W, 1 <= H, W <= 65535, H * W <= 2^26,
 * 0 <= F <= 65535; F == 0 is success and touches nothing; null pointers with F > 0 and sizes outside these ranges are
 * NERFHIP_E_BADARG before anything is launched; `workspace` is 8-byte aligned (NERFHIP_E_ALIGN) and holds
 * gif_workspace_bytes(F, H, W) bytes (0 for a refused shape) — about 38.5 KB per strip of NERFHIP_GIF_STRIP pixels plus 168 KB per
 * frame; both calls may share it.  Nothing is allocated, nothing synchronises.
 *
 * gif_quantize: frames (F,H,W,3) uint8 -> indices (F,H*W) uint8, palettes (F,256,3) uint8, box_counts (F) int32.  Histogram over
 * the 32^3 bins (r>>3, g>>3, b>>3); median cut on it (boxes shrunk to their occupied bins; split the most populated box that
 * spans more than one bin, tie to the lowest index, along its longest axis in bins, tie to r, g, b, after the first coordinate
 * whose cumulative count reaches (n + 1) / 2, clamped so the upper part is not empty; the lower part keeps the index, the upper
 * gets the next) until 256 boxes or none can be split; index = the box of the pixel's bin; palette entry = (2 sum + cnt) / (2 cnt)
 * of the entry's true colours, unused entries 0.
 *
 * gif_lzw: indices (F,H*W) -> data (F, gif_data_stride(H,W)) uint8 and lengths (F) int32: per frame the image data as it stands
 * in the file between the minimum-code-size byte (8) and the zero-length terminator: the LZW code stream (clear 256, end 257,
 * first free code 258, 9..12 bits, LSB first) in 255-byte sub-blocks behind their length bytes.  The index stream is cut into
 * strips of NERFHIP_GIF_STRIP consecutive pixels; each starts with a clear code, the end code follows the last.  A strip of K
 * pixels makes its decoder assign codes up to 257 + K - 1 <= 4094, so the 4096-code table never fills and no overflow path
 * exists.  Bytes behind lengths[f] are not written.  lengths[f] == -1: a dictionary probe exceeded its bound (a broken
 * invariant, never input-dependent); that frame's data is not written.                                                          */
#define NERFHIP_GIF_STRIP 3838
size_t nerfhip_gif_workspace_bytes(int F, int H, int W);
size_t nerfhip_gif_data_stride(int H, int W);
int nerfhip_gif_quantize(const uint8_t* frames, int F, int H, int W, uint8_t* indices, uint8_t* palettes, int32_t* box_counts,
                         void* workspace, nerfhip_stream_t stream);
int nerfhip_gif_lzw(const uint8_t* indices, int F, int H, int W, uint8_t* data, int32_t* lengths, void* workspace,
                    nerfhip_stream_t stream);

/* ---- PNG encoder  (eval.py:138 `imageio.imwrite(os.path.join(dir_name, f'{i:03d}.png'), img_pred_)`) -----------
 * The zlib data of an 8-bit grey / RGB / RGBA PNG as a pure function of the pixels (DESIGN.md §15 holds the definition,
 * tests/png_ref.py restates it in numpy); the caller writes the container: signature, IHDR, one IDAT = 78 01 + data + the
 * Adler-32 big-endian, IEND, and the chunk CRC-32s.  0 <= n <= 65535 images or streams; n == 0 is success and touches nothing;
 * null pointers with n > 0 and sizes outside the ranges below are NERFHIP_E_BADARG before anything is launched.  Nothing is
 * allocated, nothing synchronises.
 *
 * png_filter: images (n,H,W,C) uint8, C in {1, 3, 4}, H, W >= 1, H * (1 + W*C) < 2^31 -> streams (n, H * (1 + W*C)) uint8: per
 * scanline the filter type and the filtered bytes.  All five filters (bpp = C, the row above row 0 is zeros) are formed from the
 * raw neighbours; the one with the smallest sum of (v < 128 ? v : 256 - v) over its bytes is kept, a tie goes to the lowest type.
 *
 * png_deflate: streams (n, stream_bytes) uint8, 1 <= stream_bytes < 2^31 -> data (n, png_data_stride(stream_bytes)) uint8,
 * lengths (n) int32, adler (n) uint32.  The stream is cut into strips of NERFHIP_PNG_STRIP bytes; each is one deflate block with
 * dynamic Huffman codes (BFINAL on the last), the blocks follow each other bit by bit.  Tokens: a strip is cut into maximal runs
 * of equal bytes; a run of L bytes is one literal, (L-1) / 258 matches of length 258 and distance 1, and for t = (L-1) % 258 one
 * match of length t if t >= 3, else t literals.  Code lengths: png_code_lengths below.  Bytes behind lengths[i] are not written.
 * lengths[i] == -1: a strip exceeded its derived worst case (a broken invariant, never input-dependent) or the data has 2^31
 * bytes or more; that stream's data is not written.  png_data_stride is that worst case — per strip 17 + 57 + 287 * 14 bits of
 * block header and 15 of end-of-block, 15 bits per byte — and 0 for a refused size.  `workspace` is 8-byte aligned
 * (NERFHIP_E_ALIGN) and holds png_workspace_bytes(n, stream_bytes) bytes (0 for a refused size), about 15.9 KB per strip.
 *
 * png_code_lengths: HOST ONLY, no GPU call.  counts (n_symbols) uint32 -> lengths (n_symbols) uint8 with every length <= limit,
 * 1 <= n_symbols <= 286, 1 <= limit <= 15, n_symbols <= 2^limit: the construction the strip kernel runs for its two alphabets
 * (limit 15 and 7), from the same source (csrc/png_huff.h).  Used symbols in ascending (count, symbol) order; Huffman's merge
 * of the two lightest, of equal weights a merged node before a leaf and the earlier before the later; depths above `limit`
 * count as `limit`; while the Kraft sum exceeds 1, one code of the longest length below `limit` is lengthened by one and takes
 * one code of length `limit` beside it; lengths go back longest first to the ascending order.  One used symbol: length 1.      */
#define NERFHIP_PNG_STRIP 8192
size_t nerfhip_png_workspace_bytes(int n, int64_t stream_bytes);
size_t nerfhip_png_data_stride(int64_t stream_bytes);
int nerfhip_png_filter(const uint8_t* images, int n, int H, int W, int C, uint8_t* streams, nerfhip_stream_t stream);
int nerfhip_png_deflate(const uint8_t* streams, int n, int64_t stream_bytes, uint8_t* data, int32_t* lengths, uint32_t* adler,
                        void* workspace, nerfhip_stream_t stream);
int nerfhip_png_code_lengths(const uint32_t* counts, int n_symbols, int limit, uint8_t* lengths);

/* ---- inflating PNG data  (datasets/blender.py:90 `img = Image.open(...)`, datasets/llff.py `Image.open(image_path)`)
 * n_streams zlib streams (RFC 1950 around RFC 1951 deflate: stored, fixed and dynamic blocks, distances up to 32768, lengths up
 * to 258) -> out (n_streams, out_stride) uint8, stream i's bytes at [i * out_stride, i * out_stride + out_bytes): the layout
 * png_unfilter reads.  Nothing outside these ranges is written, whatever the streams hold.  One workgroup of one wave per stream;
 * no workspace.
 *   data       the streams back to back, total_bytes of them, read byte by byte (no alignment, no padding needed)
 *   offsets    (n_streams + 1) int64, 8-byte aligned (NERFHIP_E_ALIGN): stream i is [offsets[i], offsets[i + 1]), at most 2^27 bytes
 *   status     (n_streams) int32, 4-byte aligned, written by the launch: 0; NERFHIP_E_DATA for a stream that zlib's inflate
 *              refuses (a header other than CM 8 / CINFO <= 7 / valid FCHECK / FDICT clear, block type 3, a stored block whose
 *              lengths disagree, a code set that is over-subscribed or incomplete — the single one-bit code excepted —, no
 *              end-of-block code, a repeat without a previous length or past HLIT + HDIST, HLIT > 286, HDIST > 30, an unassigned
 *              code, symbols 286 / 287 / distance 30 / 31, a distance behind the first byte, missing bits, a wrong Adler-32) or
 *              that produces more or fewer than out_bytes bytes; NERFHIP_E_BADARG for offsets that are not increasing inside
 *              total_bytes.  The header's window size does not limit distances (zlib's default build does not either); bytes
 *              behind the Adler-32 are ignored.  A damaged stream does not affect the others; its output bytes are undefined.
 * n_streams == 0 is success and touches nothing; null pointers with bytes to read or write, negative sizes, out_stride < out_bytes
 * and n_streams > 65535 are NERFHIP_E_BADARG before anything is launched.  Nothing allocates or synchronises.
 *
 * inflate_host: HOST function — host pointers only, no GPU, launches nothing.  The same arguments and verdicts from the same
 * per-symbol code, table builder and copy steps (csrc/inflate_core.h), the 64 lanes of a stream's wave in lockstep.  It exists
 * so that the algorithm, its bounds and its error paths can be tested and run under a sanitizer on a machine without a GPU.
 * Returns 0 when it ran (the streams' results are in status).                                                                    */
int nerfhip_inflate(const uint8_t* data, const int64_t* offsets, int64_t total_bytes, int n_streams, uint8_t* out, int64_t out_bytes,
                    int64_t out_stride, int32_t* status, nerfhip_stream_t stream);
int nerfhip_inflate_host(const uint8_t* data, const int64_t* offsets, int64_t total_bytes, int n_streams, uint8_t* out,
                         int64_t out_bytes, int64_t out_stride, int32_t* status);

/* ---- skipping empty space at eval  (eval.py:58-86 `batched_inference` runs every sample of every ray) -----------
 * Opt-in and beside the render path: an occupancy bitfield of the trained density, a per-ray cull against it that tightens
 * [near, far] (columns 6 and 7 of the ray rows) or drops the ray, the stable compaction of the rays that are left and the
 * scatter of their rendered values into full-size outputs.  No other entry point changes.  Every launch is one thread per cell,
 * word or ray in 256-thread blocks.  Nothing is allocated, nothing synchronises.
 *
 * The bitfield (a public format).  sigma (N,N,N) fp32 as grid.sigma_grid returns it, indexed [iy, ix, iz]; 2 <= N <= 1025.  The
 * grid has M = N - 1 cells per axis.  Cell (iy, ix, iz) is occupied iff one of its 8 corners sigma[iy + a, ix + b, iz + c],
 * a, b, c in {0, 1}, is > threshold or NaN; then the set is dilated by `dilate` >= 0 cells in the Chebyshev metric, clipped at
 * the grid's boundary (dilate >= M fills a grid that has one occupied cell).  words: ceil(M^3 / 32) int32, cell c = (iy M + ix) M
 * + iz is bit c & 31 of word c >> 5, the unused bits of the last word are zero.  workspace: occupancy_workspace_bytes(N) bytes
 * (2 M^3 rounded up to 256 each; 0 for a refused N).  The build is meant for small `dilate`: a dilation pass reads up to
 * 2 dilate + 1 cells per cell (at most M), the pack 32 bytes per word; N = 256 with dilate <= 2 takes 0.07-0.26 ms, a dilate near
 * M at N near 1025 would take on the order of M times longer per pass.
 *
 * cull_rays: rays (n,8) = [o d near far], 16-byte aligned, d of any length; words / M as above, 4-byte aligned
 * (NERFHIP_E_ALIGN); ranges_host: 6 HOST floats x_lo x_hi y_lo y_hi z_lo z_hi, lo < hi; x runs along ix, y along iy, z along iz.
 * Cell i of an axis spans [lo + i h, lo + (i + 1) h], h = (hi - lo) / M.  Per ray: hit (uint8), t0 = max(near, entry parameter
 * of the first occupied cell the ray pierces), t1 = min(far, exit parameter of the last one); hit iff t0 < t1; a miss reports
 * t0 = near, t1 = far.  A ray with a NaN or an infinity in any column is a hit with t0 = near, t1 = far.  Zero direction
 * components of either sign are handled without a division.  0 <= n <= 2^30; n == 0 is success and touches nothing; null
 * pointers with n > 0, M < 1, M > 1024 and ranges that are inverted, empty or not finite are NERFHIP_E_BADARG.
 * cull_rays_host: HOST function — host pointers only, no GPU, launches nothing: the same per-ray routine
 * (csrc/occupancy_core.h) in a loop, the same bits.
 *
 * cull_compact: hit, rays, t0, t1 as above -> slot (n) int32: the exclusive rank of ray i among the hits, -1 for a miss;
 * index (n_hit) int32: the hits' ray numbers, ascending; rays_out (n_hit, 8): their rows with columns 6, 7 replaced by t0, t1
 * (a null t0 or t1 keeps the row's own near or far; index and rays_out are sized for n rows); n_hit: one int32 on the DEVICE.
 * workspace: cull_compact_workspace_bytes(n), 8-byte aligned.  n == 0 writes n_hit = 0 only.
 *
 * cull_scatter: for i < n and each output whose pointer is not null: out[i] = compact[slot[i]] when 0 <= slot[i] < n_compact,
 * else the background: 1.0 (white_back) or 0.0 for rgb (n,3), 0.0 for depth and the two opacities (n) — what compositing gives
 * for all-zero weights.  Any output may be null; an output without its compact source needs n_compact == 0.                     */
size_t nerfhip_occupancy_workspace_bytes(int N);
int nerfhip_occupancy_build(const float* sigma, int N, float threshold, int dilate, int32_t* words, void* workspace,
                            nerfhip_stream_t stream);
int nerfhip_cull_rays(const float* rays, int64_t n, const int32_t* words, int M, const float* ranges_host, uint8_t* hit, float* t0,
                      float* t1, nerfhip_stream_t stream);
int nerfhip_cull_rays_host(const float* rays, int64_t n, const int32_t* words, int M, const float* ranges_host, uint8_t* hit, float* t0,
                           float* t1);
size_t nerfhip_cull_compact_workspace_bytes(int64_t n);
int nerfhip_cull_compact(const uint8_t* hit, const float* rays, const float* t0, const float* t1, int64_t n, int32_t* slot,
                         int32_t* index, float* rays_out, int32_t* n_hit, void* workspace, nerfhip_stream_t stream);
int nerfhip_cull_scatter(const int32_t* slot, int64_t n, int64_t n_compact, int white_back, const float* rgb, float* rgb_out,
                         const float* depth, float* depth_out, const float* opacity_a, float* opacity_a_out, const float* opacity_b,
                         float* opacity_b_out, nerfhip_stream_t stream);

/* ---- epoch sampling  (train.py:89-94 DataLoader(shuffle=True): every ray once per epoch, shuffled) ------------
 * The shuffle is a keyed bijection on [0, n) evaluated per position (a public function: csrc/epoch_core.h states it exactly):
 * a six-round alternating Feistel network over max(2, ceil(log2 n)) bits with murmur3's 32-bit finaliser as the round function,
 * round keys expanded from (seed, epoch) by splitmix64, cycle-walked into [0, n).  1 <= n <= 2^40.
 * Ranks follow torch's DistributedSampler: rank r of `world` owns n_rank = ceil(n / world) positions and its j-th id is
 * perm((j world + r) mod n); all ranks use the same (seed, epoch).
 *
 * epoch_ids_host: HOST function — host pointers only, no GPU: out[i] = the (first + i)-th id of the rank, i < count.
 * epoch_ids: the same into device memory, one thread per id, the same bits.
 * epoch_batch: ONE launch = batch `cursor` of epoch `epoch` of the rank: the ids of positions [cursor B, cursor B + rows),
 * rows = min(B, n_rank - cursor B), their rays (rows,8) and colours (rows,3) exactly as nerfhip_sample_batch makes them for
 * those ids (batch->rays / batch->rgbs hold B rows; the rows past `rows` are left alone), and the ids themselves into
 * ids_or_null.  state: a DEVICE buffer of 4 x uint64 {seed, epoch, cursor, arrival ticket (0)}; the launch reads seed, epoch and
 * cursor from it and its last workgroup writes the next cursor — or cursor 0 and epoch + 1 after the epoch's last batch, which is
 * batch ceil(n_rank / B) - 1, or with drop_last batch floor(n_rank / B) - 1 (the tail of n_rank mod B positions is then never
 * served) — so hipGraph replays of one captured call walk through batches and epochs.  B <= 2^30; drop_last needs B <= n_rank.
 *
 * Every entry returns NERFHIP_E_BADARG for n < 1, n > 2^40, world < 1, rank outside [0, world), B < 1, first < 0, count < 0,
 * first + count > n_rank, null pointers (count > 0) and misaligned ones (int64 / uint64: 8 bytes; rays: 16; floats: 4).         */
int nerfhip_epoch_ids_host(uint64_t seed, uint64_t epoch, int64_t n, int rank, int world, int64_t first, int64_t count,
                           int64_t* out);
int nerfhip_epoch_ids(uint64_t seed, uint64_t epoch, int64_t n, int rank, int world, int64_t first, int64_t count,
                      int64_t* out_dev, nerfhip_stream_t stream);
int nerfhip_epoch_batch(const nerfhip_ray_batch* batch, int64_t n_pixels, int64_t B, int rank, int world, int drop_last,
                        uint64_t* state, int64_t* ids_or_null, nerfhip_stream_t stream);

/* ---- rendering the baked RGBA volume  (README_Unity.md "VolumeRender": the .vol file as a Texture3D) -----------
 * Opt-in and beside everything else: the N^3 RGBA8 lattice of a .vol file kept on the device in bricks, the bitfield of its
 * occupied bricks, and a ray march through both.  The reference's consumer is a Unity shader; the semantics here are this
 * library's own and csrc/baked_core.h states them exactly.  Nothing is allocated, nothing synchronises, no runtime object is
 * created.  2 <= N <= 1625 (N^3 < 2^32, the file's index type).
 *
 * The bricked volume (a public format).  Lattice point (iy, ix, iz) — point i = iy N^2 + ix N + iz of the file, the element
 * [iy, ix, iz] of volume.read_vol's array — lies in brick (by NB + bx) NB + bz, b* = i* >> 3, NB = ceil(N / 8), at local index
 * ((iy & 7) 8 + (ix & 7)) 8 + (iz & 7).  A brick is 512 points of 4 bytes, R G B A in memory order, 2 KiB; points past the lattice
 * are zero; the volume is baked_bytes(N) = NB^3 2048 bytes (0 for a refused N), 16-byte aligned.  A pure permutation, no apron.
 *
 * baked_scatter: clears `data`, then stores the K records (K,2) int32 = [i, R << 24 | G << 16 | B << 8 | A] of a .vol file
 * (volume.vol_records / export_vol / write_vol; 8-byte aligned; the indices distinct).  A record with i >= N^3 is not stored
 * and is counted into *n_bad, one int32 on the DEVICE that the call zeroes first.  baked_from_dense: the same volume from the
 * dense lattice rgba (N,N,N,4) uint8, 4-byte aligned.  One thread per record or point.
 *
 * baked_bricks: the (N-1)^3 cells in bricks of 8^3 cells, MB = ceil((N-1) / 8) per axis.  Cell brick (by, bx, bz) is occupied iff
 * a lattice point with every index in [8 b, 8 b + 8], clipped to [0, N-1], has A > 0: every corner of every cell of the brick.
 * words: ceil(MB^3 / 32) int32, brick c = (by MB + bx) MB + bz is bit c & 31 of word c >> 5, unused bits zero.
 *
 * baked_render: rays (n,8) = [o d near far], 16-byte aligned, d of any length; words_or_null: the bitfield, or null for "every
 * brick occupied" — the outputs do not depend on it bit for bit, it only saves the gathers of empty bricks; ranges_host: 6 HOST
 * floats x_lo x_hi y_lo y_hi z_lo z_hi, x along ix, y along iy, z along iz, the first and last lattice points on the ends.
 * Per ray, in fp32: background (opacity 0, depth 0, rgb = white_back ? 1 : 0) for a non-finite value in any column, a zero
 * direction or a ray that misses the box within [near, far]; else segments of step * cell world units from the box's entry to
 * its exit, the last one cut short; per segment one alpha-weighted trilinear sample at the midpoint (a = sum w A / 255, colour
 * = sum w A rgb / sum w A), alpha = 1 - (1 - a)^(segment length / cell) — the stored A belongs to a thickness of `cell`, as
 * volume.export_vol makes it —, composited front to back: rgb (n,3), depth (n) = sum w t (unnormalised), opacity (n) = sum w;
 * white_back adds 1 - opacity to rgb.  t_stop > 0 ends a ray after the first segment that leaves its transmittance below
 * t_stop.  Any output may be null.  NERFHIP_E_BADARG before anything is launched or dereferenced: N outside [2, 1625], a range
 * with lo >= hi or not finite, cell <= 0 or not finite, step outside [1/16, 8], t_stop outside [0, 1), a box whose diagonal is
 * more than 2^20 segments long, n < 0 or > 2^30, null rays / data / ranges_host with n > 0.  n == 0 is success.
 * baked_render_host: HOST function — host pointers only, no GPU, launches nothing: the same per-ray routine in a loop; its
 * results differ from the device's by the two libraries' exp2f / log2f only.                                                     */
size_t nerfhip_baked_bytes(int N);
int nerfhip_baked_scatter(const int32_t* records, int64_t K, int N, uint8_t* data, int32_t* n_bad, nerfhip_stream_t stream);
int nerfhip_baked_from_dense(const uint8_t* rgba, int N, uint8_t* data, nerfhip_stream_t stream);
int nerfhip_baked_bricks(const uint8_t* data, int N, int32_t* words, nerfhip_stream_t stream);
int nerfhip_baked_render(const float* rays, int64_t n, const uint8_t* data, const int32_t* words_or_null, int N,
                         const float* ranges_host, float cell, float step, float t_stop, int white_back, float* rgb, float* depth,
                         float* opacity, nerfhip_stream_t stream);
int nerfhip_baked_render_host(const float* rays, int64_t n, const uint8_t* data, const int32_t* words_or_null, int N,
                              const float* ranges_host, float cell, float step, float t_stop, int white_back, float* rgb,
                              float* depth, float* opacity);

/* ---- ray casting against a triangle mesh  (README "mixed reality": a virtual object in a NeRF render, z-ordered by NeRF's depth;
 *      the consumer of extract_color_mesh's mesh) ------------------------------------------------------------------
 * Opt-in and beside everything else: a hierarchy of boxes over a triangle mesh, the nearest hit of a ray in it, and two per-ray
 * kernels that turn hits into pixels.  csrc/mesh_core.h states every routine exactly, and every entry point has a _host twin:
 * a HOST function — host pointers only, no GPU, launches nothing — that runs the same routine in a loop and gives the same
 * bits (plain fp32, IEEE division and square root, no libm).  Nothing is allocated, nothing synchronises, launches go to the
 * caller's stream.  0 <= T <= 2^28 triangles, 0 <= V < 2^31 vertices, 0 <= n <= 2^30 rays.
 *
 * The mesh: vertices (V,3) fp32, triangles (T,3) int32.  A triangle with an index outside [0, V) or a non-finite coordinate is
 * BAD: it is counted, gets an empty box and is never hit.
 *
 * The hierarchy (a public format).  The triangles are sorted by the int64 key  morton30 << 32 | t : the centroid
 * ((v0 + v1) + v2) / 3 is quantised per axis to q = min(1023, trunc((c - lo) / (hi - lo) * 1024)) (0 where hi == lo) in the
 * bounds [lo, hi] of the good triangles' vertices, and morton30 interleaves the three q with x in the highest bit of every
 * triple; a bad triangle has morton30 = 2^30.  The keys are distinct, so the order does not depend on the sort.  Leaf j holds
 * the sorted triangles [4j, 4j + 4) ∩ [0, T).  Level 0 has n_0 = ceil(T / 4) nodes, level k + 1 has ceil(n_k / 8), each
 * bounding the 8 consecutive nodes [8i, 8i + 8) ∩ [0, n_k) of level k, up to a level of one node, the root.
 * `boxes` is (mesh_bvh_nodes(T), 6) fp32 = [lo xyz, hi xyz], the levels concatenated from the leaves to the root; every box is
 * the exact min / max of what it bounds (-0 below +0); a node that bounds bad triangles only has lo = +inf, hi = -inf.
 * `tris` is (T, 12) fp32, 16-byte aligned, in sorted order: [v0 xyz, index, v1 xyz, 0, v2 xyz, 0], index the int32 bits of the
 * original triangle number, -1 (and zero coordinates) for a bad triangle.  T = 0 is a valid hierarchy of 0 nodes.
 * mesh_bvh_nodes: the number of nodes (0 for T outside [0, 2^28]).
 *
 * mesh_bvh_keys: `state`, 8 int32 on the DEVICE, is set first — [0] the number of bad triangles, [1] 0, [2..4] / [5..7] the
 * bounds' lo / hi as order-preserving integers (csrc/mesh_core.h mesh_ordered) — then keys (T) int64, 8-byte aligned.
 * mesh_bvh_boxes: sorted_keys (T) = the keys in ascending order (the caller sorts: torch.sort in ops.mesh_bvh_build) -> tris and
 * boxes; one launch for the leaves and one per level above, at most 10, nothing handed between workgroups within a launch.  A
 * sorted key whose low word is not in [0, T) is stored as a bad triangle.
 *
 * mesh_cast: rays (n,8) = [o d near far], 16-byte aligned, d of any length; one ray per lane.  tri (n) int32: the original
 * number of the nearest triangle hit with near <= t <= far, -1 for a miss; t (n): the ray's own parameter (o + t d); b1, b2 (n):
 * the barycentric weights of vertices 1 and 2.  A miss has t = b1 = b2 = 0.  A non-finite value in any column or a zero
 * direction is a miss.  On an equal t the lower original number wins, so the result does not depend on the traversal.  The
 * triangle test is the two-sided watertight one of Woop, Benthin and Wald (JCGT 2013) with the double fallback on a zero edge
 * function.  t, b1, b2 may be null.  mesh_cast_host with brute != 0 ignores `boxes` (may be null) and tests every triangle.
 *
 * mesh_shade: rgb (n,3) = (b0 c0 + b1 c1 + b2 c2) (ambient + (1 - ambient) |n . d| / (|n| |d|)), c the vertex colours
 * colors_or_null (V,3) uint8 / 255 (null: white), n the geometric normal of triangle tri[i]; `background` for tri < 0 (and for a
 * tri >= T or a triangle naming a vertex outside [0, V)).  0 <= ambient <= 1.
 *
 * mixed_compose: a render (rgb_n (n,3), depth_n (n), opacity_n (n)) and a mesh layer (tri, t, rgb_m (n,3)) -> rgb, depth,
 * opacity, mask_or_null (n) uint8.  mode 0 "ztest": s = opacity_n >= tau ? depth_n / opacity_n : +inf; the mesh wins iff
 * tri >= 0 and t < s; the winner's rgb and depth pass through, opacity is 1 and mask 1 where the mesh wins.  mode 1 "clip" (the
 * render was made with far = min(far, t) on hit rays and without a background): rgb = rgb_n + (1 - opacity_n) (hit ? rgb_m :
 * background); on a hit depth = depth_n + (1 - opacity_n) t, opacity = 1, mask = 1; on a miss depth_n, opacity_n, 0.  tau > 0.
 *
 * NERFHIP_E_BADARG before anything is launched or dereferenced: T, V or n out of range, a null pointer that n > 0 (T > 0, V > 0
 * for the mesh's arrays) would read or write, an unknown mode, ambient outside [0, 1], tau <= 0, a non-finite tau or
 * background.  NERFHIP_E_ALIGN for rays (cast) or tris not 16-byte aligned, keys not 8-byte aligned, any other array not 4-byte
 * aligned.  n == 0 (T == 0 for the build) is success.                                                                           */
size_t nerfhip_mesh_bvh_nodes(int64_t T);
int nerfhip_mesh_bvh_keys(const float* vertices, int64_t V, const int32_t* triangles, int64_t T, int64_t* keys, int32_t* state,
                          nerfhip_stream_t stream);
int nerfhip_mesh_bvh_keys_host(const float* vertices, int64_t V, const int32_t* triangles, int64_t T, int64_t* keys, int32_t* state);
int nerfhip_mesh_bvh_boxes(const float* vertices, int64_t V, const int32_t* triangles, int64_t T, const int64_t* sorted_keys,
                           float* tris, float* boxes, nerfhip_stream_t stream);
int nerfhip_mesh_bvh_boxes_host(const float* vertices, int64_t V, const int32_t* triangles, int64_t T, const int64_t* sorted_keys,
                                float* tris, float* boxes);
int nerfhip_mesh_cast(const float* rays, int64_t n, const float* tris, const float* boxes, int64_t T, int32_t* tri, float* t,
                      float* b1, float* b2, nerfhip_stream_t stream);
int nerfhip_mesh_cast_host(const float* rays, int64_t n, const float* tris, const float* boxes, int64_t T, int brute, int32_t* tri,
                           float* t, float* b1, float* b2);
int nerfhip_mesh_shade(const float* rays, int64_t n, const int32_t* tri, const float* b1, const float* b2, const float* vertices,
                       int64_t V, const int32_t* triangles, int64_t T, const uint8_t* colors_or_null, float ambient,
                       float background, float* rgb, nerfhip_stream_t stream);
int nerfhip_mesh_shade_host(const float* rays, int64_t n, const int32_t* tri, const float* b1, const float* b2,
                            const float* vertices, int64_t V, const int32_t* triangles, int64_t T, const uint8_t* colors_or_null,
                            float ambient, float background, float* rgb);
int nerfhip_mixed_compose(int mode, int64_t n, const float* rgb_n, const float* depth_n, const float* opacity_n, const int32_t* tri,
                          const float* t, const float* rgb_m, float tau, float background, float* rgb, float* depth,
                          float* opacity, uint8_t* mask_or_null, nerfhip_stream_t stream);
int nerfhip_mixed_compose_host(int mode, int64_t n, const float* rgb_n, const float* depth_n, const float* opacity_n,
                               const int32_t* tri, const float* t, const float* rgb_m, float tau, float background, float* rgb,
                               float* depth, float* opacity, uint8_t* mask_or_null);

/* ---- shadows for mixed renders: any-hit mesh rays, light samples, lit compose  (the reference README's showpiece: the inserted
 *      object "casts shadow on the scene") -------------------------------------------------------------------------
 * Opt-in and beside everything else.  csrc/shadow_core.h states every routine exactly, and every entry point has a _host twin (a
 * HOST function: host pointers, no GPU, the same routine in a loop, the same bits: plain fp32, IEEE division and square root, no
 * libm).  Nothing is allocated, nothing synchronises, launches go to the caller's stream.  1 <= K <= 64 samples per pixel,
 * n K <= 2^30 rows.
 *
 * mesh_occluded: rays, tris, boxes, T as mesh_cast reads them -> hit (n) uint8: 1 iff some good triangle is accepted by
 * mesh_cast's triangle test with near <= t <= far, that is iff mesh_cast would return tri >= 0.  The same ray set-up, triangle
 * test, box test (limit = far) and bounded pre-order walk, left at the first accepted triangle; no t, no barycentrics, no tie
 * rule.  The answer belongs to the mesh and the row, not to the traversal: the hierarchy, brute force (mesh_occluded_host with
 * brute != 0, which ignores `boxes`) and mesh_cast agree in every bit.
 *
 * shadow_rays: primary rows rays (n,8), 16-byte aligned, and the surface distance s (n) of each -> rows (n K, 8), 16-byte
 * aligned, sample k of pixel i at row i K + k, and cosine_or_null (n).  p = o + s d.  The light: kind 0 directional, (lx, ly, lz)
 * the direction TOWARDS the light (any non-zero length); kind 1 point, (lx, ly, lz) its position.  A row is [p, d_k, bias, far]:
 * d_k the unit vector towards light sample k, far = reach (directional) or |L_k - p| (point).  A pixel has ZERO ROWS (all eight
 * values +0) when s is not finite or <= 0, when its primary row or p holds a non-finite value, or when p lies on a point light;
 * a single sample that coincides with p gives one zero row.  mesh_cast and mesh_occluded miss a zero row, baked_render returns
 * opacity 0 for it.  The light is a square of half-width `radius` facing the pixel, with the frame e1 = normalise(c x axis),
 * e2 = c x e1, c the unit direction to the light's centre and axis the coordinate axis of its smallest |component| (x, y, z on
 * ties).  Sample k is offset by radius (u_k e1 + v_k e2): d_k = normalise(c + offset) (directional), L_k = L + offset (point).
 * (u_k, v_k) in [-1, 1)^2 is the R2 sequence in 32-bit integers, x_k = 2^31 + k 3242174889, y_k = 2^31 + k 2447445414 (mod
 * 2^32), u = (x >> 8) 2^-23 - 1; rotate = 1 adds h = hash(i) to x and hash(h ^ 0x9e3779b9) to y (csrc/shadow_core.h states the
 * hash); rotate = 0 uses one sequence for every pixel.  radius == 0 skips the offset: the K rows of a pixel are its K = 1 row in
 * every bit.  cosine: 1 everywhere when tri_or_null is null, and where tri < 0; elsewhere max(n . c, 0) clamped to 1, n the unit
 * geometric normal of triangle tri[i] of (vertices, V, triangles, T) as mesh_shade forms it, turned to the camera (n . d <= 0);
 * 0 for a pixel with zero rows, a tri >= T, a triangle naming a vertex outside [0, V), a normal of zero or non-finite length.
 *
 * light_compose: rgb (n,3), mask (n) uint8 (mixed_compose's: 1 on a mesh pixel), cosine (n), hit (n K) uint8 of mesh_occluded,
 * trans_or_null (n K): the scene's transmittance along each row (null: 1) -> rgb_out (n,3), visibility_or_null (n): the V
 * applied.  Mesh pixel: V = (sum_k (hit_k ? 0 : 1) trans_k) / K, rgb_out = rgb (ambient + ((1 - ambient) cosine) V).  Scene
 * pixel: V = (sum_k (hit_k ? 0 : 1)) / K (trans is not read), rgb_out = rgb (1 - strength (1 - V)).  Sums in k order.
 * ambient = 1 and strength = 0 make both factors an exact 1.
 *
 * NERFHIP_E_BADARG before anything is launched or dereferenced: n, T, V or K out of range, n K > 2^30, an unknown kind, rotate
 * not 0 or 1, bias or reach not finite and > 0, radius not finite and >= 0, a non-finite light, a directional light of zero
 * length, ambient or strength outside [0, 1], a null pointer that n > 0 would read or write.  NERFHIP_E_ALIGN for rays, rows or
 * tris not 16-byte aligned, any other float or int32 array not 4-byte aligned.  n == 0 is success.                              */
int nerfhip_mesh_occluded(const float* rays, int64_t n, const float* tris, const float* boxes, int64_t T, uint8_t* hit,
                          nerfhip_stream_t stream);
int nerfhip_mesh_occluded_host(const float* rays, int64_t n, const float* tris, const float* boxes, int64_t T, int brute, uint8_t* hit);
int nerfhip_shadow_rays(const float* rays, const float* s, int64_t n, const int32_t* tri_or_null, const float* vertices, int64_t V,
                        const int32_t* triangles, int64_t T, int kind, float lx, float ly, float lz, float bias, float reach, int K,
                        float radius, int rotate, float* rows, float* cosine_or_null, nerfhip_stream_t stream);
int nerfhip_shadow_rays_host(const float* rays, const float* s, int64_t n, const int32_t* tri_or_null, const float* vertices, int64_t V,
                             const int32_t* triangles, int64_t T, int kind, float lx, float ly, float lz, float bias, float reach,
                             int K, float radius, int rotate, float* rows, float* cosine_or_null);
int nerfhip_light_compose(int64_t n, const float* rgb, const uint8_t* mask, const float* cosine, const uint8_t* hit,
                          const float* trans_or_null, int K, float ambient, float strength, float* rgb_out,
                          float* visibility_or_null, nerfhip_stream_t stream);
int nerfhip_light_compose_host(int64_t n, const float* rgb, const uint8_t* mask, const float* cosine, const uint8_t* hit,
                               const float* trans_or_null, int K, float ambient, float strength, float* rgb_out,
                               float* visibility_or_null);

/* ---- mesh decimation: grid vertex clustering with mean or quadric placement  (no counterpart in the reference, whose answer to a
 *      9.4 M triangle mesh is a coarser sigma grid) ----------------------------------------------------------------
 * Opt-in and beside everything else.  csrc/decimate_core.h states every routine exactly, and every entry point has a _host twin
 * (a HOST function: host pointers, no GPU, the same routine in a loop, the same bits).  Nothing is allocated, nothing
 * synchronises, launches go to the caller's stream; the caller sorts between the calls (ops._mesh_decimate: torch.sort).
 *
 * Inputs: vertices (V,3) fp32, triangles (T,3) int32, optional colors (V,3) uint8, cell > 0 finite fp32, optional origin.
 * 0 <= V, T <= 2^28.  The result (a contract, whatever computes it):
 *  1 bad input.  A vertex with a non-finite coordinate belongs to no cluster.  A triangle with an index outside [0, V) or such
 *    a vertex is BAD: dropped and counted (mesh_bvh's rule).
 *  2 cells.  lo = the per-axis minimum over the finite vertices, or the origin (no finite vertex may lie below it).
 *    q_a = floorf((v_a - lo_a) / cell) in fp32, subtraction and IEEE division separately rounded; R_a = max q_a + 1;
 *    cell number c = (q0 R1 + q1) R2 + q2; R0 R1 R2 < 2^31.
 *  3 clusters.  The keys c << 32 | vertex (c = 2^31 - 1 for a vertex of no cluster; distinct, so the sort decides nothing) are
 *    sorted; the non-empty cells, in ascending c, are the clusters 0 .. C - 1; cluster_of[v] is the vertex's cluster or -1.
 *  4 mean.  m = the fp64 sum of the members in ascending vertex number over their count n.  Colours: per channel the integer
 *    sum s, output (2 s + n) / (2 n) in integers.
 *  5 quadric.  Every good triangle t, also one that collapses in 6, has the entries e = 3 t + k, k = 0..2, each in the cluster
 *    of corner k; the keys cluster << 32 | e are sorted.  Per cluster, in ascending e, in fp64 on the fp32 coordinates:
 *    n = (p1 - p0) x (p2 - p0), d = -n . (p0 - m), A += n n^T, b += d n.  lambda = eps (A00 + A11 + A22); x = 0 if that trace
 *    is 0 or not finite, else the solution of (A + lambda I) x = -b (cofactors), 0 if not finite.  position = clamp(m + x,
 *    blo, bhi) per axis, blo_a = (double)lo_a + q_a (double)cell, bhi = blo + (double)cell.  Mean placement is x = 0 without
 *    the clamp.  Either is rounded to fp32 once.
 *  6 triangles.  Good triangles are mapped through cluster_of; one with two equal clusters is COLLAPSED; of those equal after
 *    rotating the smallest cluster to the front (the same orientation) the one with the lowest number stays, the others are
 *    DUPLICATES.  Survivors keep their order and their corner order.
 *  7 vertices.  A cluster no survivor names is UNREFERENCED and removed; the others keep their order; triangles and cluster_of
 *    are renumbered (-1 for a vertex of a removed cluster).
 *
 * The passes (every array on the device, or on the host for a _host twin; 4-byte aligned, int64 and double arrays 8-byte):
 * bounds: state, 8 int32 — [0] the non-finite vertices, [1] 0, [2..4] / [5..7] lo / hi of the finite ones as order-preserving
 *   integers (csrc/mesh_core.h mesh_ordered; +inf / -inf when there is none).
 * keys: lo_host (3 floats), cell and res_host (R, 3 int32) on the HOST -> keys (V) int64.
 * clusters: sorted_keys (V) ascending -> cluster_of (V) int32; seg_start (>= C + 1) int32, cluster i being the sorted positions
 *   [seg_start[i], seg_start[i + 1]); totals[0] = C (int64, on the device).  blk (ceil(V / 256)) int32 and off (the same count)
 *   int64 are scratch.
 * entries: -> keys (3 T) int64, cluster 2^31 - 1 for the corners of a bad triangle.
 * place: placement 0 mean, 1 quadric (reads sorted_entries (3 T), else unused); 0 < eps <= 1 -> mean (C,3) fp64, positions
 *   (C,3) fp32, colors_out (C,3) uint8 (null with colors).
 * tri_keys: -> flags (T) uint8: 0 candidate, 1 bad, 2 collapsed; key_hi = a << 28 | b, key_lo = c << 28 | t of the rotated
 *   clusters (a, b, c); key_hi = 2^63 - 1 and key_lo = t for a triangle that is no candidate.
 * duplicates: the two arrays in ascending (key_hi, key_lo) order -> flags[t] = 3 for every duplicate.
 * mark: -> ref (C) uint8, 1 for a cluster a survivor names; totals (5 int64, on the device) = T', V', bad, collapsed,
 *   duplicate; blk_t / off_t (ceil(T / 256)) and blk_c / off_c (ceil(C / 256)): block totals (int32) and offsets (int64),
 *   which compact reads.
 * compact: -> vnew (C) int32, out_vertices (V',3), out_triangles (T',3), out_colors (V',3) or null, out_cluster_of (V).
 *
 * NERFHIP_E_BADARG before anything is launched or dereferenced: a count out of range, C > V, a null array that a non-zero
 * count would read or write, cell <= 0 or not finite, a non-finite lo, an R < 1 or R0 R1 R2 >= 2^31, an unknown placement,
 * colours in without colours out or the reverse.  NERFHIP_E_ALIGN as stated above.  A zero count is success.                    */
int nerfhip_mesh_decimate_bounds(const float* vertices, int64_t V, int32_t* state, nerfhip_stream_t stream);
int nerfhip_mesh_decimate_bounds_host(const float* vertices, int64_t V, int32_t* state);
int nerfhip_mesh_decimate_keys(const float* vertices, int64_t V, const float* lo_host, float cell, const int32_t* res_host,
                               int64_t* keys, nerfhip_stream_t stream);
int nerfhip_mesh_decimate_keys_host(const float* vertices, int64_t V, const float* lo_host, float cell, const int32_t* res_host,
                                    int64_t* keys);
int nerfhip_mesh_decimate_clusters(const int64_t* sorted_keys, int64_t V, int32_t* blk, int64_t* off, int32_t* cluster_of,
                                   int32_t* seg_start, int64_t* totals, nerfhip_stream_t stream);
int nerfhip_mesh_decimate_clusters_host(const int64_t* sorted_keys, int64_t V, int32_t* blk, int64_t* off, int32_t* cluster_of,
                                        int32_t* seg_start, int64_t* totals);
int nerfhip_mesh_decimate_entries(const int32_t* triangles, int64_t T, int64_t V, const int32_t* cluster_of, int64_t* keys,
                                  nerfhip_stream_t stream);
int nerfhip_mesh_decimate_entries_host(const int32_t* triangles, int64_t T, int64_t V, const int32_t* cluster_of, int64_t* keys);
int nerfhip_mesh_decimate_place(const float* vertices, int64_t V, const uint8_t* colors_or_null, const int32_t* triangles,
                                int64_t T, const int64_t* sorted_keys, const int32_t* seg_start, int64_t C,
                                const int64_t* sorted_entries, const float* lo_host, float cell, const int32_t* res_host,
                                double eps, int placement, double* mean, float* positions, uint8_t* colors_out_or_null,
                                nerfhip_stream_t stream);
int nerfhip_mesh_decimate_place_host(const float* vertices, int64_t V, const uint8_t* colors_or_null, const int32_t* triangles,
                                     int64_t T, const int64_t* sorted_keys, const int32_t* seg_start, int64_t C,
                                     const int64_t* sorted_entries, const float* lo_host, float cell, const int32_t* res_host,
                                     double eps, int placement, double* mean, float* positions, uint8_t* colors_out_or_null);
int nerfhip_mesh_decimate_tri_keys(const int32_t* triangles, int64_t T, int64_t V, const int32_t* cluster_of, uint8_t* flags,
                                   int64_t* key_hi, int64_t* key_lo, nerfhip_stream_t stream);
int nerfhip_mesh_decimate_tri_keys_host(const int32_t* triangles, int64_t T, int64_t V, const int32_t* cluster_of, uint8_t* flags,
                                        int64_t* key_hi, int64_t* key_lo);
int nerfhip_mesh_decimate_duplicates(const int64_t* sorted_hi, const int64_t* sorted_lo, int64_t T, uint8_t* flags,
                                     nerfhip_stream_t stream);
int nerfhip_mesh_decimate_duplicates_host(const int64_t* sorted_hi, const int64_t* sorted_lo, int64_t T, uint8_t* flags);
int nerfhip_mesh_decimate_mark(const int32_t* triangles, int64_t T, int64_t V, const int32_t* cluster_of, const uint8_t* flags,
                               int64_t C, uint8_t* ref, int32_t* blk_t, int64_t* off_t, int32_t* blk_c, int64_t* off_c,
                               int64_t* totals, nerfhip_stream_t stream);
int nerfhip_mesh_decimate_mark_host(const int32_t* triangles, int64_t T, int64_t V, const int32_t* cluster_of,
                                    const uint8_t* flags, int64_t C, uint8_t* ref, int32_t* blk_t, int64_t* off_t, int32_t* blk_c,
                                    int64_t* off_c, int64_t* totals);
int nerfhip_mesh_decimate_compact(const int32_t* triangles, int64_t T, int64_t V, const int32_t* cluster_of, const uint8_t* flags,
                                  int64_t C, const uint8_t* ref, const int64_t* off_t, const int64_t* off_c,
                                  const float* positions, const uint8_t* colors_or_null, int32_t* vnew, float* out_vertices,
                                  int32_t* out_triangles, uint8_t* out_colors_or_null, int32_t* out_cluster_of,
                                  nerfhip_stream_t stream);
int nerfhip_mesh_decimate_compact_host(const int32_t* triangles, int64_t T, int64_t V, const int32_t* cluster_of,
                                       const uint8_t* flags, int64_t C, const uint8_t* ref, const int64_t* off_t,
                                       const int64_t* off_c, const float* positions, const uint8_t* colors_or_null, int32_t* vnew,
                                       float* out_vertices, int32_t* out_triangles, uint8_t* out_colors_or_null,
                                       int32_t* out_cluster_of);

/* ---- texturing a triangle mesh: a per-triangle atlas, its sample points, the lookup  (README_Unity.md wants a small mesh with a
 *      texture; no counterpart in the reference's code) -------------------------------------------------------------
 * Opt-in and beside everything else.  csrc/texture_core.h states every routine exactly, and every entry point has a _host twin (a
 * HOST function: host pointers, no GPU, the same routine in a loop, the same bits).  Nothing is allocated, nothing synchronises,
 * launches go to the caller's stream.  The mesh is mesh_cast's: vertices (V,3) fp32, triangles (T,3) int32, 0 <= V < 2^31.
 *
 * The atlas (a public format).  res = R, 1 <= R <= 64, is the number of texel intervals along a patch leg; the block edge is
 * B = R + 3.  Triangle t has n_tex = (R + 2)(R + 3) / 2 samples at the lattice points (i, j), i, j >= 0, i + j <= R + 1; sample
 * (i, j) lies at the barycentric weights b1 = i / R (vertex 1), b2 = j / R (vertex 2), b0 = 1 - b1 - b2.  The diagonal
 * i + j = R + 1 lies just outside the triangle (b0 = -1 / R): a real sample of the triangle's plane, which a bilinear footprint in
 * a cell on the hypotenuse reads.  Sample number m = j (R + 2) - j (j - 1) / 2 + i; global sample q = t n_tex + m; K = T n_tex,
 * at most 2^30 per call.
 *   Blocks: triangle t lies in block k = t >> 1; nb = Wa / B blocks per row; X0 = (k mod nb) B, Y0 = (k / nb) B.  Wa is a multiple
 * of 4 with B <= Wa <= 16384; Ha = B ceil(ceil(T / 2) / nb) <= 16384 (mesh_tex_height; 0 for T = 0).  An even t puts sample (i, j)
 * at texel (X0 + i, Y0 + j), an odd t at (X0 + B - 1 - i, Y0 + B - 1 - j).  The atlas is (Ha, Wa, 3) uint8, rows from the top,
 * r g b, 4-byte aligned.
 *   Fill: a block texel (lx, ly) with lx + ly = R + 2 belongs to nobody and takes the even triangle's sample (lx - 1, ly) for
 * lx >= 1, else (0, ly - 1).  Zero are: the odd half (lx + ly >= R + 3) of a last block without an odd triangle, blocks with
 * 2 k >= T, and the columns >= nb B.  Every byte of the atlas is written exactly once.
 *
 * mesh_tex_samples: n_tex (0 for R out of range).  mesh_tex_height: Ha (0 for an argument out of range or Ha > 16384).
 *
 * mesh_tex_points: one thread per sample -> points (K,3) fp32: p_a = (v0_a + b1 e1_a) + b2 e2_a in fp32 with b1 = (float)i /
 * (float)R (IEEE division), e = v - v0, every operation separately rounded; normals_or_null (K,3) fp64, 8-byte aligned: the fp64
 * cross product of the fp32 edges, (y1 z2 - z1 y2, z1 x2 - x1 z2, x1 y2 - y1 x2), over its length sqrt((nx nx + ny ny) + nz nz),
 * (0, 0, 1) where that length is zero or not finite.  A BAD triangle (mesh_cast's rule: an index outside [0, V) or a non-finite
 * coordinate) gives the point (0, 0, 0) and the normal (0, 0, 1); mesh_cast never hits it, so its texels are never shown.
 *
 * mesh_tex_atlas: colors (K,3) uint8, one per sample -> atlas.  A gather: one thread per 4 consecutive texels of a row, which
 * writes its 12 bytes as three 32-bit stores.
 *
 * mesh_shade_tex: the hits (tri, b1, b2 of mesh_cast) -> rgb (n,3).  `background` by mesh_shade's rules: tri < 0, tri >= T, or a
 * triangle naming a vertex outside [0, V).  fx = clamp(b1 R, 0, R) (0 for a NaN), fy likewise from b2.  filter 1, bilinear:
 * i = min((int)fx, R), fu = fx - i, j and fv likewise; the texels (i, j), (i + 1, j), (i, j + 1), (i + 1, j + 1) of the triangle
 * as c = byte / 255.0f; rgb = ((1 - fu)(1 - fv) c00 + fu (1 - fv) c10) + ((1 - fu) fv c01 + fu fv c11), times mesh_shade's
 * ambient + (1 - ambient) |n . d| / (|n| |d|).  filter 0, nearest: the texel ((int)(fx + 0.5f), (int)(fy + 0.5f)).  Whatever b1
 * and b2 are, every texel read has 0 <= i, j <= R + 1 and so lies in the triangle's own block; for a point of the triangle all
 * that carry weight are the triangle's own samples.
 *
 * NERFHIP_E_BADARG before anything is launched or dereferenced: R, Wa, Ha, T, V, K or n out of range, Wa no multiple of 4 or
 * below B, Ha not as stated, a null array that would be read or written, an unknown filter, ambient outside [0, 1], a non-finite
 * background.  NERFHIP_E_ALIGN: normals not 8-byte, any other fp32 / int32 array or the atlas not 4-byte aligned.  n == 0 and
 * T == 0 are success.                                                                                                           */
int nerfhip_mesh_tex_samples(int R);
int nerfhip_mesh_tex_height(int64_t T, int R, int Wa);
int nerfhip_mesh_tex_points(const float* vertices, int64_t V, const int32_t* triangles, int64_t T, int R, float* points,
                            double* normals_or_null, nerfhip_stream_t stream);
int nerfhip_mesh_tex_points_host(const float* vertices, int64_t V, const int32_t* triangles, int64_t T, int R, float* points,
                                 double* normals_or_null);
int nerfhip_mesh_tex_atlas(const uint8_t* colors, int64_t T, int R, int Wa, int Ha, uint8_t* atlas, nerfhip_stream_t stream);
int nerfhip_mesh_tex_atlas_host(const uint8_t* colors, int64_t T, int R, int Wa, int Ha, uint8_t* atlas);
int nerfhip_mesh_shade_tex(const float* rays, int64_t n, const int32_t* tri, const float* b1, const float* b2, const float* vertices,
                           int64_t V, const int32_t* triangles, int64_t T, const uint8_t* atlas, int R, int Wa, int Ha, int filter,
                           float ambient, float background, float* rgb, nerfhip_stream_t stream);
int nerfhip_mesh_shade_tex_host(const float* rays, int64_t n, const int32_t* tri, const float* b1, const float* b2,
                                const float* vertices, int64_t V, const int32_t* triangles, int64_t T, const uint8_t* atlas, int R,
                                int Wa, int Ha, int filter, float ambient, float background, float* rgb);

#ifdef __cplusplus
}
#endif
#endif /* NERFHIP_H */
