/*
 * stylerenderer_amd — C ABI of the MI355X-native (gfx950) StyleRenderer generator hot path.
 *
 * One shared library, libstylerenderer_hip.so, built from the .hip sources under stylerenderer_amd/csrc.
 * Every entry point is extern "C", takes plain device pointers + sizes + an explicit HIP
 * stream, allocates nothing, keeps no state and never synchronises the host (all calls are
 * hipGraph-capturable).  Each function states which reference interface it replaces
 * (paths relative to the reference repository WestlyPark/StyleRenderer).
 *
 * Ownership: the caller allocates every buffer (inputs contiguous, fp32 unless noted).
 * Errors: 0 on success; a negative SR_E* code for a rejected argument; a positive value is the
 * hipError_t of a failed launch.  sr_error_string() maps either to text.  (The reference's
 * native functions return `bool` and never check anything, op/upfirdn2d_kernel.cu:205-257.)
 *
 * Threading: any host thread; the kernels are enqueued on `stream` (pass the framework's
 * current stream — the reference uses c10::cuda::getCurrentCUDAStream for two ops,
 * op/fused_bias_act_kernel.cu:78-80, and the legacy default stream for the rasterizer,
 * op/rasterize.cu:89-92, which is deliberately not reproduced).
 */
#ifndef STYLERENDERER_AMD_H_
#define STYLERENDERER_AMD_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* sr_stream_t; /* hipStream_t */

#define SR_OK 0
#define SR_EINVAL (-1)   /* bad size / null pointer / unsupported combination */
#define SR_ERANGE (-2)   /* size exceeds what the kernel indexes */

const char* sr_error_string(int code);
/* ABI version of this header; bumped on any signature change. */
int sr_abi_version(void);

/* ---------------------------------------------------------------------------------------
 * fused bias + activation
 * Replaces  bool fused_bias_act_op(float* y, const float* x, const float* b, const float* ref,
 *             int act, int grad, float alpha, float scale, int size_x, int step_b, int size_b,
 *             int use_bias, int use_ref, int use_cuda)   reference op/fused_bias_act_kernel.cu:71-76
 * (arithmetic: op/fused_bias_act_kernel.cu:15-42).  out[i] = f(x[i] + b[(i / step_b) % size_b]) * scale,
 * f selected by act*10+grad: 30 lrelu(x), 31 lrelu'(ref)*x, 32/12 zero, else identity.
 * Sizes are 64-bit here (the reference's `int` caps tensors at 2^31 elements). */
int sr_fused_bias_act(float* y, const float* x, const float* b, const float* ref, int act, int grad,
                      float alpha, float scale, int64_t size_x, int64_t step_b, int64_t size_b,
                      int use_bias, int use_ref, sr_stream_t stream);

/* Backward of the fused activation with the bias gradient reduced in the same pass.
 * Replaces the pair {fused_bias_act(gy, empty, out, 3, 1, ..) ; grad_input.sum(dims != 1)}
 * of reference op/fused_act.py:29-38.  x layout [n, c, inner]:
 *   gx[i]    = (out[i] > 0 ? gy[i] : alpha * gy[i]) * scale
 *   gb[ch]   = sum over n, inner of gx                      (deterministic two-stage tree)
 * `partial` is caller scratch of sr_fused_act_bwd_scratch_floats(n, c, inner) floats. */
int64_t sr_fused_act_bwd_scratch_floats(int64_t n, int64_t c, int64_t inner);
int sr_fused_act_bwd(float* gx, float* gb, const float* gy, const float* out, float alpha,
                     float scale, int64_t n, int64_t c, int64_t inner, float* partial,
                     sr_stream_t stream);

/* Fused StyledConv tail (reference model.py:26-32: NoiseInjection layers.py:328-332 followed by
 * FusedLeakyReLU op/fused_act.py:52-62) in one pass.  x, y [n, c, inner]; noise [n or 1, 1, inner]
 * with batch stride noise_bstride (0 = shared); noise_w a 1-element DEVICE tensor; bias [c].
 *   t = x + noise_w[0]*noise[b, i] + bias[ch] ;  y = (cond > 0 ? t : alpha*t) * scale
 * cond = t, or ref[...] when ref != NULL (the double-backward form).  noise / bias may be NULL.
 * Requires inner % 4 == 0 and 16-byte aligned pointers (SR_EINVAL otherwise: the caller then uses
 * sr_fused_bias_act). */
int sr_noise_bias_act(float* y, const float* x, const float* noise, const float* noise_w,
                      const float* bias, const float* ref, float alpha, float scale, int64_t n,
                      int64_t c, int64_t inner, int64_t noise_bstride, sr_stream_t stream);
/* Its backward in one pass: gx = (out > 0 ? gy : alpha*gy)*scale, gbias[ch] = sum gx,
 * gnoise_w[0] = sum gx*noise (deterministic two-stage reductions; gbias / gnoise_w may be NULL). */
int64_t sr_noise_bias_act_bwd_scratch_floats(int64_t n, int64_t c, int64_t inner);
int sr_noise_bias_act_bwd(float* gx, float* gbias, float* gnoise_w, const float* gy, const float* out,
                          const float* noise, float alpha, float scale, int64_t n, int64_t c,
                          int64_t inner, int64_t noise_bstride, float* scratch, sr_stream_t stream);
/* The same with one more output: rowdot[b*c + ch] = sum_i gx * y0, where y0 is the forward pass's input
 * rebuilt from its output (out / scale, or out / (alpha*scale) where negative, minus noise_w*noise and bias) —
 * the demodulation gradient of the modulated convolution in front of the activation, without a separate pass
 * over two tensors.  Needs alpha != 0 and scale != 0. */
int64_t sr_noise_bias_act_bwd_dot_scratch_floats(int64_t n, int64_t c, int64_t inner);
int sr_noise_bias_act_bwd_dot(float* gx, float* gbias, float* gnoise_w, float* rowdot, const float* gy,
                              const float* out, const float* noise, const float* noise_w, const float* bias,
                              float alpha, float scale, int64_t n, int64_t c, int64_t inner,
                              int64_t noise_bstride, float* scratch, sr_stream_t stream);
/* StyledMapConv tail (reference model.py:49-54: `out * stylemap[:, :1] + stylemap[:, 1:2]`, then
 * NoiseInjection and FusedLeakyReLU) as one pass and its backward as one pass (+ the fixed-order finish):
 *   y = lrelu((x * a[b,p] + s[b,p]) + noise_w * noise[b,p] + bias[c]) * scale
 *   gx = g * a ; gamap[b,p] = sum_c g * x ; gsmap[b,p] = sum_c g ; gbias[c] = sum_{b,p} g ; gnoise_w = sum g * noise
 * with g = lrelu'(y) * gy * scale.  x / y / gx [n, c, inner]; amap / smap point at [n] planes of `inner` floats
 * `map_bstride` floats apart (two channels of one rasterised-map tensor); gamap / gsmap [n, inner] contiguous.
 * inner % 4 == 0 and 16-byte aligned pointers. */
int sr_noise_bias_act_affine(float* y, const float* x, const float* amap, const float* smap, int64_t map_bstride,
                             const float* noise, const float* noise_w, const float* bias, float alpha,
                             float scale, int64_t n, int64_t c, int64_t inner, int64_t noise_bstride,
                             sr_stream_t stream);
int64_t sr_noise_bias_act_affine_bwd_scratch_floats(int64_t n, int64_t c, int64_t inner);
int sr_noise_bias_act_affine_bwd(float* gx, float* gamap, float* gsmap, float* gbias, float* gnoise_w,
                                 const float* gy, const float* out, const float* x, const float* amap,
                                 int64_t map_bstride, const float* noise, float alpha, float scale, int64_t n,
                                 int64_t c, int64_t inner, int64_t noise_bstride, float* scratch,
                                 sr_stream_t stream);
/* Second-order pass of the same tail (path-length regulariser: the backward above is itself differentiated, reference
 * train.py:118-134).  Cotangents of the first-order outputs: Gx [n, c, inner] | NULL, Gmap = (Ga, Gs) planes at
 * Gmap + b * gmap_bstride (+ inner) | NULL, Gb [c] | NULL, Gnw [1] | NULL.  Writes d_gy, d_x [n, c, inner] and the
 * gradient of the scale plane d_amap[b * d_amap_bstride + p] = sum_c (gy * m) * Gx (nothing flows to the shift
 * plane, the bias or the noise weight: the activation mask is piecewise constant).  scratch:
 * sr_noise_bias_act_affine_bwd2_scratch_floats(n, c, inner) floats. */
int64_t sr_noise_bias_act_affine_bwd2_scratch_floats(int64_t n, int64_t c, int64_t inner);
int sr_noise_bias_act_affine_bwd2(float* d_gy, float* d_x, float* d_amap, int64_t d_amap_bstride, const float* Gx,
                                  const float* Gmap, int64_t gmap_bstride, const float* Gb, const float* Gnw,
                                  const float* gy, const float* out, const float* x, const float* amap,
                                  int64_t map_bstride, const float* noise, float alpha, float scale, int64_t n,
                                  int64_t c, int64_t inner, int64_t noise_bstride, float* scratch, sr_stream_t stream);

/* Adam step over ONE flat fp32 parameter buffer (the optimiser of reference train.py:529-536: torch.optim.Adam with
 * the lazy-regularisation corrected lr / betas, no weight decay) in a single pass over p, g, m, v (28 B/parameter):
 *   m += (g - m)(1 - beta1);  v = beta2 v + (1 - beta2) g^2;  p -= lr / (1 - beta1^t) * m / (sqrt(v) / sqrt(1 - beta2^t) + eps)
 * `step` points at the device scalar t (a float the caller increments before the call), so the launch can be
 * captured in a hipGraph.  All four buffers 16-byte aligned. */
int sr_adam_flat(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2,
                 float eps, const float* step, sr_stream_t stream);
/* Guarded form for data-parallel training: `guard_offs` (host array, <= 16 entries, read at launch time) are positions
 * of `g` — the first element of every all-reduce bucket.  If any of them is NaN the kernel leaves p / m / v untouched
 * stores 1 into `*skipped_host` (pinned host memory, may be NULL) and takes the caller's increment of `*step` back (a
 * refused step does not advance the bias correction).  The guard samples only these positions: NaN elsewhere in `g` is
 * not detected, and a gradient that is legitimately NaN at a guard position refuses the step as well.  Together with sr_signal_wait_poison this
 * turns a lost bucket signal on ONE rank into a refused optimiser step on EVERY rank (the SUM carries the NaN),
 * where torch DDP's reducer (reference distributed.py:98-105) would raise on the rank that lost it. */
int sr_adam_flat_guarded(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2,
                         float eps, float* step, const int64_t* guard_offs, int n_guards,
                         int32_t* skipped_host, sr_stream_t stream);

/* Row-wise dot products of two [rows, inner] tensors, optionally with a scaled copy in the same
 * sweep: dots[r] = sum_i a[r,i]*b[r,i] ; out_scaled[r,i] = b[r,i]*scale[r] (out_scaled may be NULL).
 * These are the style / demodulation gradients of the modulated convolution (sum_p x*dx', sum_p g*y)
 * that autograd would otherwise compute as a multiply pass plus a reduction pass.  Rows of any length
 * (16-byte vector accesses when inner % 4 == 0 and the pointers are aligned, dword accesses otherwise). */
int64_t sr_rowdot_scratch_floats(int64_t rows, int64_t inner);
int sr_rowdot(float* dots, float* out_scaled, const float* a, const float* b, const float* scale,
              int64_t rows, int64_t inner, float* scratch, sr_stream_t stream);
/* dots[r] = (sum_p a[r,p] * b[r,p]) / rdiv[r] — the demodulation gradient sum_p g * y0 / d of a modulated convolution
 * (reference layers.py:298-300 differentiated) without a separate division launch; same sums, same order as sr_rowdot. */
int sr_rowdot_div(float* dots, const float* a, const float* b, const float* rdiv, int64_t rows, int64_t inner,
                  float* scratch, sr_stream_t stream);
/* Backward of sr_rowdot in one pass (second-order sweep of the path-length regulariser): ga = gd[r] * b,
 * gb = gd[r] * a + go * scale[r], gs[r] = sum_p go * b.  ga / gb / gs / gd / go / scale may be NULL (gs needs go and
 * `scratch` of sr_rowdot_scratch_floats(rows, inner) floats). */
int sr_rowdot_bwd(float* ga, float* gb, float* gs, const float* a, const float* b, const float* gd, const float* go,
                  const float* scale, int64_t rows, int64_t inner, float* scratch, sr_stream_t stream);

/* 1x1 modulated convolution with N <= 4 output channels (ToRGB: reference model.py:56-69 via
 * layers.py:293-323 with kernel_size 1, demodulate off), as streaming passes instead of MFMA tiles.
 * ws [B, N, C] = W[j,c] * style[b,c]; x [B, C, hw]; out / g [B, N, hw]; hw % 4 == 0.
 *   fwd: out[b,j,p] = sum_c ws[b,j,c]*x[b,c,p] + bias[j]      dx: dx[b,c,p] = sum_j ws[b,j,c]*g[b,j,p]
 *   dw:  dws[b,j,c] = sum_p g[b,j,p]*x[b,c,p]  (deterministic two-stage reduction) */
int sr_smallconv_fwd(float* out, const float* x, const float* ws, const float* bias, int64_t B, int64_t C,
                     int64_t N, int64_t hw, sr_stream_t stream);
int sr_smallconv_dx(float* dx, const float* g, const float* ws, int64_t B, int64_t C, int64_t N, int64_t hw,
                    sr_stream_t stream);
/* dx = addend + W^T g: the feature map that feeds ToRGB also feeds the next layer (reference model.py:206-219); its two
 * gradients are added in this pass (addend [B, C, hw] or NULL, may alias dx) */
int sr_smallconv_dx_add(float* dx, const float* g, const float* ws, const float* addend, int64_t B, int64_t C, int64_t N,
                        int64_t hw, sr_stream_t stream);
int64_t sr_smallconv_dw_scratch_floats(int64_t B, int64_t C, int64_t N, int64_t hw);
int sr_smallconv_dw(float* dws, const float* g, const float* x, int64_t B, int64_t C, int64_t N, int64_t hw,
                    float* scratch, sr_stream_t stream);
/* the same with the bias gradient gb[j] = sum_{b,p} g[b,j,p] of ToRGB (reference model.py:57-69) summed by the same
 * launch (gb may be NULL); same scratch */
int sr_smallconv_dw_bias(float* dws, float* gb, const float* g, const float* x, int64_t B, int64_t C, int64_t N, int64_t hw,
                         float* scratch, sr_stream_t stream);
/* Backward of a styled layer's tail whose output y [B, C, hw] feeds both the next layer and ToRGB (reference
 * model.py:206-219) in ONE pass: what sr_smallconv_dx_add(gy, g_rgb, ws, g_above), sr_smallconv_dw_bias(dws, gb_rgb, g_rgb, y)
 * and sr_noise_bias_act_bwd_dot(gpre, gbias, gnoise_w, rowdot, gy, y, ...) compute in that order, every output bit for bit
 * (the same partition and expression order; the same finish kernels), without writing gy and reading y once instead of
 * twice.  g_above (the next layer's cotangent, [B, C, hw]) may be NULL (the last layer) and must not be gpre; gbias NULL =
 * frozen bias / noise strength; gb_rgb NULL = no ToRGB bias gradient.  C % 4 == 0, hw % 4 == 0, B * C <= 65535, N <= 4,
 * alpha != 0, scale != 0; gpre, g_above, y, g_rgb, noise on 16-byte boundaries.  scratch: sr_fork_nba_bwd_scratch_floats
 * floats, 8-byte aligned. */
int64_t sr_fork_nba_bwd_scratch_floats(int64_t B, int64_t C, int64_t N, int64_t hw);
int sr_fork_nba_bwd(float* gpre, float* gbias, float* gnoise_w, float* rowdot, float* dws, float* gb_rgb,
                    const float* g_above, const float* y, const float* g_rgb, const float* ws, const float* noise,
                    const float* noise_w, const float* bias, float alpha, float scale, int64_t B, int64_t C, int64_t N,
                    int64_t hw, int64_t noise_bstride, float* scratch, sr_stream_t stream);
/* Modulated weight rows of that convolution and their pull-back (reference layers.py:293-297, demodulate=False):
 *   sr_modrows_fwd: ws[b,j,c] = (scale * w[j,c]) * s[b,c]                       w [N, C], s [B, C], ws [B, N, C]
 *   sr_modrows_bwd: gs[b,c] = sum_j dws[b,j,c] * (scale * w[j,c]);  gw[j,c] = scale * sum_b dws[b,j,c] * s[b,c]
 *                   (gs or gw may be NULL).  Fixed summation order. */
int sr_modrows_fwd(float* ws, const float* w, const float* s, float scale, int64_t B, int64_t N, int64_t C,
                   sr_stream_t stream);
int sr_modrows_bwd(float* gs, float* gw, const float* dws, const float* w, const float* s, float scale, int64_t B,
                   int64_t N, int64_t C, sr_stream_t stream);

/* Vertex normals of a posed mesh (replaces reference utils_3d.py:379-404 mesh_point_normal: three
 * sparse.mm scatters + layers.py:13-34 Normalize).  v [B, nv, 3]; tri [nf, 3] int64 with ids in
 * [0, nv); (adj_off [nv + 1], adj [3 nf]) = CSR list of the corner-major incidences k*nf + f of every
 * vertex, ascending (the caller builds it once per topology).  vn [B, nv, 3] = sum of incident face
 * normals (b-a)x(c-a), divided by max(|.|, eps); norm_out [B, nv] (may be NULL) = the clamped length.
 * Gather in a fixed order: deterministic, no atomics. */
int sr_vertex_normals_f32(float* vn, float* norm_out, const float* v, const int64_t* tri, const int32_t* adj_off,
                          const int32_t* adj, int64_t B, int64_t nv, int64_t nf, float eps, sr_stream_t stream);

/* Posed mesh of the inversion / training loops (reference utils_3d.py random_apply_pose3D: vertices @ R * s + t):
 *   out[b, i, :] = v[b, i, :] @ M[b] + t[b]     v [B or 1, nv, 3] (v_bstride = nv*3, or 0 to share one mesh), M [B,3,3]
 * row-major, t [B,3] or NULL.  sr_affine3_bwd: gm[b] = v[b]^T @ g[b] ([3,3]), gt[b] = sum_i g[b, i, :] — fixed-order
 * sums (run-to-run identical); either may be NULL.  The gradient w.r.t. v is g @ M^T = sr_affine3_fwd(g, M^T). */
int sr_affine3_fwd(float* out, const float* v, const float* m, const float* t, int64_t B, int64_t nv,
                   int64_t v_bstride, sr_stream_t stream);
int sr_affine3_bwd(float* gm, float* gt, const float* v, const float* g, int64_t B, int64_t nv, int64_t v_bstride,
                   sr_stream_t stream);

/* Morphable-mesh node of face reconstruction (csrc/morph.hip; reference face_model.py:71-74, utils_3d.py euler_mat "yxz"
 * and mesh_point_normal).  w = fc.weight [3 nv, d] as stored, bias [3 nv], coeff [B, d], pose [B, 7] = (yaw, pitch, roll,
 * tx, ty, tz, log-scale), lin [B, 3, 3] = exp(log-scale) R (sr_pose_batch_fwd).
 * sr_morph_fwd: vs[b] = (bias + w coeff[b]).view(nv, 3) (the unposed shape) and v[b] = vs[b] @ lin[b] + pose[b, 3:6]; one
 *   pass over w for all B samples (B d <= 8192, else SR_ERANGE).  reg (may be NULL) = lam * sum (coeff / sigma)^2, sigma
 *   [d] (NULL: 1).  The normals are sr_vertex_normals_f32 of vs, rotated by R (sr_affine3_fwd).
 * sr_vertex_normals_bwd_f32: gvs[b, i] = gv[b, i] @ lin[b]^T + (adjoint of the vertex normals at vertex i given gn, the
 *   gradient of the normals ns @ rot[b]); v = the unposed vertices, ns / normc = the outputs of sr_vertex_normals_f32 of
 *   v (normc = the clamped length).  gv may be NULL (then lin may be), rot may be NULL (identity).  The gradient of the
 *   composite normalize() below eps too; a gather over the CSR incidence in the forward's fixed order, no atomics.
 * sr_morph_gcoeff: gcoeff[b, k] = sum_j w[j, k] gvs[b, j] + 2 lam greg[0] coeff[b, k] / sigma[k]^2 (greg: device scalar,
 *   may be NULL), rows = 3 nv; split-K over slabs of rows into scratch [sr_morph_gcoeff_scratch_floats] and a fixed-order
 *   second pass.  sr_morph_pose_bwd: gpose[b] from glin, grot [B, 3, 3] (either may be NULL) and gt [B, 3]. */
int sr_morph_fwd(float* v, float* vs, float* reg, const float* w, const float* bias, const float* coeff, const float* lin,
                 const float* pose, const float* sigma, float lam, int64_t B, int64_t nv, int64_t d, sr_stream_t stream);
int sr_vertex_normals_bwd_f32(float* gvs, const float* gv, const float* gn, const float* lin, const float* rot,
                              const float* v, const float* ns, const float* normc, const int64_t* tri,
                              const int32_t* adj_off, const int32_t* adj, int64_t B, int64_t nv, int64_t nf, float eps,
                              sr_stream_t stream);
int64_t sr_morph_gcoeff_scratch_floats(int64_t rows, int64_t B, int64_t d);
int sr_morph_gcoeff(float* gcoeff, float* scratch, const float* w, const float* gvs, const float* coeff,
                    const float* sigma, float lam, const float* greg, int64_t B, int64_t rows, int64_t d,
                    sr_stream_t stream);
int sr_morph_pose_bwd(float* gpose, const float* glin, const float* grot, const float* gt, const float* pose, int64_t B,
                      sr_stream_t stream);

/* Skinning node of face reconstruction (csrc/skin.hip; reference face_model.py:313-341 LinearBlendSkinningModel, utils_3d.py
 * rodrigues).  nj joints of which the first nroot are roots, np = nj - nroot, parent [np] (parent before child);
 * coeff [B, ds + 3 np] = shape, then one axis-angle per moving joint; pose [B, 7] as above or NULL (no global pose);
 * j0 [nj, 3] = Jreg v_template, js [3 nj, ds] = Jreg S[:ds]; sigma [ds] and pose_inv [np, 3, 3] of the prior (NULL: 1 / I);
 * st [3 nv, D] = the stacked basis transposed, D = ds + 9 np; vt [3 nv] the template; wts [nv, nj] the skinning weights.
 * nj <= 32, else SR_ERANGE.
 * sr_skin_joints_fwd: cx [B, D] = [shape, vec(R_i - I)], chain [B, nj, 15] = (A_i, t_i, J_i) of the kinematic chain,
 *   G [B, nj, 12] = [A_i lin ; (t_i - J_i A_i) lin + t] with the global pose folded in, reg (may be NULL) = lam *
 *   regulation(coeff).  One launch for all B.
 * sr_skin_fwd: vp[b] = (vt + st cx[b]).view(nv, 3) and v[b, k] = vp[b, k] (sum_i wts[k, i] G[b, i, :3]) + sum_i wts[k, i]
 *   G[b, i, 3]; one pass over st per slice of floor(12288 / (D + 12 nj)) samples (D + 12 nj <= 12288, else SR_ERANGE).
 * sr_skin_bwd: with g = gv + gvn (gvn may be NULL), gvp[b, k] = g M_k^T and part [B, ceil(nv / 256), nj, 12] = the
 *   per-workgroup sums of wts[k, i] [vp_k^T g ; g] (sr_skin_bwd_scratch_floats floats), in a fixed order.
 * sr_skin_joints_bwd: sums part over its nblk workgroups in order, then the adjoints of the pose fold, the chain, the
 *   joint regressor and rodrigues: gcoeff [B, ds + 3 np] from gcx [B, D] (sr_morph_gcoeff of st and gvp) plus 2 lam
 *   greg[0] times the prior's gradient (greg: device scalar, may be NULL), and gpose [B, 7] (may be NULL). */
int sr_skin_joints_fwd(float* cx, float* G, float* chain, float* reg, const float* coeff, const float* pose,
                       const float* j0, const float* js, const int32_t* parent, const float* sigma, const float* pose_inv,
                       float lam, int64_t B, int64_t nj, int64_t nroot, int64_t ds, sr_stream_t stream);
int sr_skin_fwd(float* v, float* vp, const float* st, const float* vt, const float* cx, const float* wts, const float* G,
                int64_t B, int64_t nv, int64_t D, int64_t nj, sr_stream_t stream);
int64_t sr_skin_bwd_scratch_floats(int64_t nv, int64_t B, int64_t nj);
int sr_skin_bwd(float* gvp, float* part, const float* gv, const float* gvn, const float* vp, const float* wts,
                const float* G, int64_t B, int64_t nv, int64_t nj, sr_stream_t stream);
int sr_skin_joints_bwd(float* gcoeff, float* gpose, const float* gcx, const float* part, const float* coeff,
                       const float* pose, const float* chain, const float* js, const int32_t* parent, const float* sigma,
                       const float* pose_inv, float lam, const float* greg, int64_t B, int64_t nblk, int64_t nj,
                       int64_t nroot, int64_t ds, sr_stream_t stream);

/* Bilinear blendshape node of face reconstruction (csrc/blend.hip; reference face_model.py:128-146 BlendShapeModel).
 * x [B, ds + de] = identity logits, then expression logits; w = weight [(ds + 1)(de + 1), 3 nv] as stored (the vertex
 * coordinate contiguous; rows need 4-byte alignment only); beta [ds + 1 + 2 de] of the Dirichlet / Beta prior.
 * ds + de + 2 <= 8192 and B <= 65535, else SR_ERANGE.
 * sr_blend_head: xs [B, ds + 1] = softmax(cat(x_s, -sum x_s)), xe [B, de + 1] = cat(1 - sum s, s), s = sigmoid(x_e),
 *   prior [B] = lam * regulation(x[b]) and z [sr_blend_z_floats] = the products xs (x) xe of every sample in blocks of
 *   eight samples, [block][k][8], zero where a block has fewer.  One launch for all B.
 * sr_blend_fwd: vs[b] = (z[b] w).view(nv, 3), v[b] = vs[b] @ lin[b] + pose[b, 3:6] (v NULL: vs alone; then lin and pose
 *   may be NULL), reg (may be NULL) = sum_b prior[b] in sample order.  One pass over w per eight samples.
 * sr_blend_gz: gz[b, k] = sum_c w[k, c] gvs[b, c], gz [B, (ds + 1)(de + 1)]; one pass over w per eight samples, fixed-order
 *   sums, no scratch.
 * sr_blend_tail: gcoeff [B, ds + de] from gz (NULL: zero) through the softmax / sigmoid Jacobians and the couplings of
 *   the last identity and the neutral expression, plus lam greg[0] d regulation / dx (greg: device scalar, may be NULL). */
int64_t sr_blend_z_floats(int64_t B, int64_t ds, int64_t de);
int sr_blend_head(float* xs, float* xe, float* prior, float* z, const float* x, const float* beta, float lam, int64_t B,
                  int64_t ds, int64_t de, sr_stream_t stream);
int sr_blend_fwd(float* v, float* vs, float* reg, const float* w, const float* z, const float* prior, const float* lin,
                 const float* pose, int64_t B, int64_t nv, int64_t ds, int64_t de, sr_stream_t stream);
int sr_blend_gz(float* gz, const float* w, const float* gvs, int64_t B, int64_t nv, int64_t ds, int64_t de,
                sr_stream_t stream);
int sr_blend_tail(float* gcoeff, const float* gz, const float* xs, const float* xe, const float* beta, float lam,
                  const float* greg, int64_t B, int64_t ds, int64_t de, sr_stream_t stream);

/* Pose parameters of the inversion loop, pose = (yaw, pitch, roll, tx, ty, tz, log-scale): rot [3,3] = Rz(roll) Rx(pitch)
 * Ry(yaw) (utils_3d.euler_mat(angles, "yxz"), row-major), lin = exp(log-scale) * rot; sr_pose_bwd: gradient of the seven
 * numbers from the gradients of the two matrices (either may be NULL; entries 3..5 are written as 0: the translation's
 * gradient is sr_affine3_bwd's gt).  One lane each: replaces ~60 one-element tensor-algebra launches per step. */
int sr_pose_fwd(float* lin, float* rot, const float* pose, sr_stream_t stream);
int sr_pose_bwd(float* gpose, const float* glin, const float* grot, const float* pose, sr_stream_t stream);
/* B poses at once, forward only: lin [B, 3, 3], rot [B, 3, 3] or NULL, pose [B, 7].  The random poses of the training
 * loop (reference utils_3d.py:360-376 random_apply_pose3D: euler_mat + scale for a batch of sampled poses). */
int sr_pose_batch_fwd(float* lin, float* rot, const float* pose, int64_t B, sr_stream_t stream);

/* Skinny linear algebra of the style path, B = per-GPU batch rows (csrc/style_linear.hip).
 * EqualLinear (reference layers.py:222-248), optionally with the fused leaky-ReLU of the mapping
 * network (act != 0: op/fused_act.py:86-97 semantics, bias inside the activation):
 *   sr_linear_fwd:   y[b,n] = act(wscale * sum_k x[b,k]*w[n,k] + bscale*bias[n])      (bias may be NULL)
 *   sr_linear_bwd_x: gx[b,k] = wscale * sum_n g'[b,n]*w[n,k],  g' = act'(y) * gy  (y = saved output)
 *   sr_linear_bwd_w: gw[n,k] = wscale * sum_b g'[b,n]*x[b,k];  gbias[n] = bscale * sum_b g'[b,n] (or NULL)
 * Demodulation scale of ModulatedConv2d (layers.py:298-300 as rsqrt(s^2 @ wsq + eps), wsq from
 * sr_weight_prep):
 *   sr_demod_fwd: d[b,co] = rsqrt(sum_ci s[b,ci]^2 * wsq[ci,co] + eps)
 *   sr_demod_bwd: gq = -gd*d^3/2;  gs[b,ci] = gs_add[b,ci] + 2*s[b,ci]*sum_co gq[b,co]*wsq[ci,co]
 *                 (gs_add may be NULL);  gwsq[ci,co] = sum_b s[b,ci]^2 * gq[b,co]   (gs or gwsq may be NULL)
 * x rows have pitch ldx floats (a [B, n_latent, K] latent slice is read in place); everything else is
 * dense.  K, ldx (resp. Co) must be multiples of 4 and the matrices 16-byte aligned (SR_EINVAL otherwise). */
int sr_linear_fwd(float* y, const float* x, const float* w, const float* bias, int64_t B, int64_t K, int64_t N,
                  int64_t ldx, float wscale, float bscale, int act, float alpha, float gain, sr_stream_t stream);
int sr_linear_bwd_x(float* gx, const float* gy, const float* y, const float* w, int64_t B, int64_t K, int64_t N,
                    float wscale, int act, float alpha, float gain, sr_stream_t stream);
int sr_linear_bwd_w(float* gw, float* gbias, const float* gy, const float* y, const float* x, int64_t B,
                    int64_t K, int64_t N, int64_t ldx, float wscale, float bscale, int act, float alpha,
                    float gain, sr_stream_t stream);
int sr_demod_fwd(float* d, const float* s, const float* wsq, int64_t B, int64_t Ci, int64_t Co, float eps,
                 sr_stream_t stream);
int sr_demod_bwd(float* gs, float* gwsq, const float* gd, const float* gs_add, const float* s, const float* d,
                 const float* wsq, int64_t B, int64_t Ci, int64_t Co, sr_stream_t stream);

/* Weight preparation for sr_conv2d_mfma (replaces the per-layer ATen passes of reference
 * layers.py:293-300 / 213-216: scale * weight, pow, sum, views).  w [Co, Ci, k, k], k in {1, 3}.
 *   sr_weight_prep:     wt [k*k, Ci, ld] = scale*w  (ld % 4 == 0, ld >= Co, pad columns zeroed);
 *                       wsq [Ci, Co] = sum_taps (scale*w)^2, or NULL.
 *   sr_weight_prep_bwd: gw [Co,Ci,k,k] = scale*gwt^T + 2*scale^2*w*gwsq  (gwt [k*k,Ci,ldg] or NULL,
 *                       gwsq [Ci,Co] or NULL, not both NULL).
 *   sr_weight_adjoint:  out [taps, N, ldc] = in [taps', C, ldn] transposed in (C, N), taps reversed
 *                       when flip != 0 — the weights of the data-gradient convolution. */
int sr_weight_prep(float* wt, float* wsq, const float* w, float scale, int64_t Co, int64_t Ci, int ksize,
                   int64_t ld, sr_stream_t stream);
int sr_weight_prep_bwd(float* gw, const float* gwt, const float* gwsq, const float* w, float scale,
                       int64_t Co, int64_t Ci, int ksize, int64_t ldg, sr_stream_t stream);
int sr_weight_adjoint(float* out, const float* in, int64_t taps, int64_t C, int64_t N, int64_t ldn,
                      int64_t ldc, int flip, sr_stream_t stream);

/* Batched forms of the two preparations a forward pass needs: n layers per call, per-layer arguments as host arrays
 * (pointers to device tensors, shapes); one launch per 48 layers instead of one per layer — a training iteration at 4
 * images per GPU prepares ~230 weights in its forward passes, each a 5 us launch (stylerenderer_amd/op/weight_bank.py).
 * Same arithmetic per element as the single-layer entry points: results are bit-identical.  wsq[i] may be NULL. */
int sr_weight_prep_batch(int n, float* const* wt, float* const* wsq, const float* const* w, const float* scale,
                         const int64_t* Co, const int64_t* Ci, const int* ksize, const int64_t* ld, sr_stream_t stream);
int sr_weight_adjoint_batch(int n, float* const* out, const float* const* in, const int64_t* taps, const int64_t* C,
                            const int64_t* N, const int64_t* ldn, const int64_t* ldc, const int* flip,
                            sr_stream_t stream);

/* Skinny products of ALL modulated layers of a pass, one launch per call (csrc/bank_mm.hip, op/bankmm.py): the
 * modulation s_l = EqualLinear_l(latent row) of every ModulatedConv2d and the demodulation sums q_l = s_l^2 @ Wsq_l
 * (reference layers.py:222-248, 293-300) and their gradients of any order.  A call takes a TABLE of problems: host
 * arrays of device pointers and extents (<= SR_BANK_MAX per launch; longer tables are cut into several launches).
 *   sr_bank_nt: out_p[b,n] = alpha * sum_k A_p[b,k] * M_p[n,k] + bscale * bias_p[n]      A_p rows of pitch lda[p]
 *               (a latent row of [B, n_latent, K] is read in place), M_p [N_p, K_p] dense, out_p rows of pitch ldo[p];
 *               bias (the array or single entries) may be NULL.
 *   sr_bank_nn: out_o[b,j] = alpha * sum over the n_terms[o] terms t of output o, in table order, of
 *               sum_i A_t[b,i] * M_t[i,j]       (M_t [I_t, J_o] dense; the term arrays A / M / lda / I are the
 *               concatenation of all outputs' terms).  Several layers reading one latent row add their gradients here.
 *   sr_bank_tn: out_p[i,j] = alpha * sum_b A_p[b,i] * C_p[b,j] (dense [I_p, J_p]);  col_p[i] = bscale * sum_b A_p[b,i]
 *               (col, or single entries, may be NULL).
 * K, J, the pitches of A (nt) / C / out (nn) multiples of 4 and those arrays 16-byte aligned (SR_EINVAL otherwise);
 * B <= 65535.  Fixed summation order: deterministic. */
#define SR_BANK_MAX 48
int sr_bank_nt(int n, float* const* out, const float* const* A, const float* const* M, const float* const* bias,
               const int64_t* lda, const int64_t* ldo, const int64_t* K, const int64_t* N, int64_t B, float alpha,
               float bscale, sr_stream_t stream);
int sr_bank_nn(int n_out, float* const* out, const int64_t* ldo, const int64_t* J, const int* n_terms,
               const float* const* A, const float* const* M, const int64_t* lda, const int64_t* I, int64_t B,
               float alpha, sr_stream_t stream);
int sr_bank_tn(int n, float* const* out, float* const* col, const float* const* A, const float* const* C,
               const int64_t* lda, const int64_t* ldc, const int64_t* I, const int64_t* J, int64_t B, float alpha,
               float bscale, sr_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * upfirdn2d: zero-insert upsample -> pad/crop -> 2-D FIR (correlation with the flipped kernel)
 * -> decimate.  Replaces  bool upfirdn2d_op(float* out, const float* x, const float* k,
 *             UpFirDn2DKernelParams& p, int mode, int use_cuda)
 * reference op/upfirdn2d_kernel.cu:205-206 with the struct of op/upfirdn2d.cpp:2-22 flattened into
 * scalars (minor_dim is always 1 in the reference's callers, op/upfirdn2d.py:99,122, and is not
 * carried).  x is [major, in_h, in_w], out is [major, out_h, out_w] with
 * out = (in*up + pad0 + pad1 - k) / down + 1  (op/upfirdn2d.py:103-104); the caller passes the
 * out sizes it allocated and they are checked.  `k` is the [kh, kw] kernel in DEVICE memory. */
int sr_upfirdn2d(float* out, const float* x, const float* k, int64_t major, int in_h, int in_w,
                 int out_h, int out_w, int kh, int kw, int up_x, int up_y, int down_x, int down_y,
                 int pad_x0, int pad_x1, int pad_y0, int pad_y1, sr_stream_t stream);

/* ToRGB skip connection (reference model.py:66-68: `out + self.upsample(skip)`, Upsample = upfirdn2d with up = 2 and the
 * 4x4 kernel, layers.py:170-181) in one pass: out = upfirdn2d(x, k, up = 2, pad = (pad0, pad1)) + addend.
 * x [major, in_h, in_w]; out / addend [major, out_h, out_w], out_h = 2 in_h + pad0 + pad1 - 3.  Same arithmetic
 * as sr_upfirdn2d followed by an addition (IEEE addition commutes), bit for bit. */
int sr_upsample2_add(float* out, const float* x, const float* k, const float* addend, int64_t major, int in_h,
                     int in_w, int out_h, int out_w, int pad0, int pad1, sr_stream_t stream);

/* Blur (4x4 FIR, up = down = 1, pad (pad0, pad1) on both axes: reference layers.py:194-203 after the
 * stride-2 transposed convolution) with the StyledConv tail fused into its store (reference
 * model.py:26-32): y = lrelu((fir(x) + noise_w[0]*noise[b, p]) + bias[ch], alpha) * gain.
 * x [n, c, in_h, in_w] -> y [n, c, out_h, out_w], out = in + pad0 + pad1 - 3; noise [n or 1, 1, out_h, out_w]
 * with batch stride noise_bstride (0 = shared) or NULL; bias [c] or NULL.  One pass instead of two.  This entry and
 * sr_blur_nba_bwd tile maps whose 2^k side is 64 .. 1024 wide (pad 1, 16-byte aligned pointers) by bands of whole rows,
 * everything else by 32 x 64 tiles: same values bit for bit (SR_FIR_BAND=0: tiles everywhere). */
int sr_blur_noise_bias_act(float* y, const float* x, const float* k, const float* noise, const float* noise_w,
                           const float* bias, float alpha, float gain, int64_t n, int64_t c, int in_h, int in_w,
                           int out_h, int out_w, int pad0, int pad1, int64_t noise_bstride, sr_stream_t stream);

/* First-order backward of sr_blur_noise_bias_act in ONE pass (the gradient of reference layers.py:194-203 + model.py:26-32
 * taken together): gx = blur^T(lrelu'(y) * gy * gain) [n, c, out_h, out_w], gbias [c] = sum lrelu'(y) gy gain, gnoise_w [1]
 * = the same sum weighted with the noise (both NULL when bias / noise strength are frozen), rowdot [n * c] = the sum
 * weighted with the pre-activation value rebuilt from y (the demodulation gradient of the convolution in front, see
 * sr_noise_bias_act_bwd_dot).  gy, y [n, c, in_h, in_w] = the forward's OUTPUT extent, out = in + 3 - 2 pad0 its input
 * extent (pad0 = the forward's symmetric padding); k_flipped = the forward taps flipped in both axes (what sr_upfirdn2d
 * takes for the gradient of a blur).  gx is bit-identical to sr_noise_bias_act_bwd followed by sr_upfirdn2d; the three
 * sums are deterministic (per-workgroup partials added in a fixed order) but associate differently from
 * sr_noise_bias_act_bwd_dot, and differently by bands than by tiles.  scratch: sr_blur_nba_bwd_scratch_floats floats. */
int64_t sr_blur_nba_bwd_scratch_floats(int64_t n, int64_t c, int out_h, int out_w);
int sr_blur_nba_bwd(float* gx, float* gbias, float* gnoise_w, float* rowdot, const float* gy, const float* y,
                    const float* k_flipped, const float* noise, const float* noise_w, const float* bias, float alpha,
                    float gain, int64_t n, int64_t c, int in_h, int in_w, int out_h, int out_w, int pad0,
                    int64_t noise_bstride, float* scratch, sr_stream_t stream);


/* ---------------------------------------------------------------------------------------
 * 3DMM triangle rasterizer (z-buffered, deterministic; results equal the reference's
 * SEQUENTIAL CPU loops bit for bit: op/rasterize.cpp:21-67).
 * Replaces  bool rasterize_gpu<scalar,index>(b, nv, nf, h, w, repeat_v, repeat_f, perspective,
 *             const scalar* v, const index* f, index* i, scalar* c, scalar* zB, scalar eps)
 * reference op/rasterize.cu:84-88.
 *   v     [b, nv, 3] (or [nv, 3] when repeat_v)         tri  int64 [nf, 3] (or [b, nf, 3])
 *   index int64 [b, h, w, 3]   coeff [b, h, w, 3]       zbuf [b, h, w] or NULL
 * Unlike the reference the outputs need NOT be pre-initialised: every pixel is written
 * (uncovered: index 0, coeff 0, zbuf -MAX).  `work` is caller scratch of
 * sr_rasterize_scratch_bytes(b, nf, h, w, is_double) bytes.
 * Optional fused attribute interpolation (reference op/rasterize.py:29-37): when `tex` != NULL,
 * attr[b,h,w,c] = sum_k tex[index_k, :] * coeff_k  with tex [b*nv (or nv), c].
 * Optional winner map `win` int32 [b,h,w]: id of the triangle that owns the pixel, -1 where uncovered
 * (what sr_rasterize_grad_* walks; index / coeff may then be NULL: the fused autograd path writes
 * 16 B per pixel instead of 48).  Triangles whose bounding box exceeds 64 pixels are walked by the whole
 * workgroup (LDS queue) instead of one lane; optional `big` int32 [2 + 2*b*nf] is the gradient state of the call for
 * sr_rasterize_grad_*: their count, b*nf slots for the flat ids sample * nf + triangle (any order), b*nf slots
 * for the leader table (smallest row-major pixel each triangle won) and ONE state word: the LDS-tiled forward path
 * builds the table while it resolves its tiles and stores 1, the global-key path fills it with INT_MAX and stores 0 —
 * the gradient pass reads that word on the device and completes the table in place when it is 0 (it never re-derives
 * which path the forward took).
 * `perspective` is a flags word: bit 0 = perspective projection (the reference's bool), bit 1 = SR_RASTER_CHW: the
 * interpolated attributes are written channel-major, attr[b,c,h,w] — what the generator's map heads convolve — instead of
 * the reference's [b,h,w,c] (model.py:262 permutes and every consumer re-lays it out); sr_rasterize_grad_* with the same
 * bit reads grad_out as [b,c,h,w].  Same values either way.  Bit 2 = SR_RASTER_GRAD_ACC (sr_rasterize_grad_* only):
 * grad_v / grad_tex are ADDED to what the buffers hold — one mesh rasterised at several resolutions (GeneratorWithMap,
 * reference model.py:255-262) sums its gradients inside the gather, in call order, instead of in a tensor addition per
 * resolution. */
#define SR_RASTER_CHW 2
#define SR_RASTER_GRAD_ACC 4
int64_t sr_rasterize_scratch_bytes(int64_t b, int64_t nf, int64_t h, int64_t w, int is_double);
/* int32 entries of the gradient state `big` above (2 + 2*b*nf): what the caller of a forward pass allocates. */
int64_t sr_rasterize_grad_state_ints(int64_t b, int64_t nf);
int sr_rasterize_forward_f32(int64_t b, int64_t nv, int64_t nf, int64_t h, int64_t w, int repeat_v,
                             int repeat_f, int perspective, const float* v, const int64_t* tri,
                             int64_t* index, float* coeff, float* zbuf, float eps,
                             const float* tex, int64_t tex_c, float* attr, int32_t* win, int32_t* big,
                             void* work, sr_stream_t stream);
int sr_rasterize_forward_f64(int64_t b, int64_t nv, int64_t nf, int64_t h, int64_t w, int repeat_v,
                             int repeat_f, int perspective, const double* v, const int64_t* tri,
                             int64_t* index, double* coeff, double* zbuf, double eps,
                             const double* tex, int64_t tex_c, double* attr, int32_t* win, int32_t* big,
                             void* work, sr_stream_t stream);

/* The same mesh rasterised at n resolutions (GeneratorWithMap draws one normal map per synthesis resolution, reference
 * model.py:255-262) in THREE launches instead of three per resolution: interpolated attributes only (attr[l]:
 * [b,h_l,w_l,c] or, with SR_RASTER_CHW, [b,c,h_l,w_l]) plus the gradient state win[l] / big[l] of each level (the arrays, or
 * single entries, may be NULL: no gradient state); work[l] >= sr_rasterize_scratch_bytes(b, nf, h_l, w_l, 0) bytes each.
 * Same kernels' bodies as sr_rasterize_forward_f32 on its global-key path: same bits.  Levels the per-call dispatcher would
 * give to the LDS-tiled path are not taken (sr_rasterize_levels_supported returns 0, the call SR_EINVAL): the caller then
 * goes level by level. */
#define SR_RASTER_MAX_LEVELS 12
int sr_rasterize_levels_supported(int n, int64_t b, int64_t nf, const int64_t* h, const int64_t* w);
int sr_rasterize_forward_levels_f32(int n, int64_t b, int64_t nv, int64_t nf, const int64_t* h, const int64_t* w,
                                    int repeat_v, int repeat_f, int perspective, const float* v, const int64_t* tri,
                                    float eps, const float* tex, int64_t tex_c, float* const* attr, int32_t* const* win,
                                    int32_t* const* big, void* const* work, sr_stream_t stream);

/* Gradient of those n levels in FOUR launches: grad_v / grad_tex = the sum over the levels (added in table order — the
 * value n sr_rasterize_grad_f32 calls with SR_RASTER_GRAD_ACC from the second on produce, bit for bit) of the gradient of
 * level l's attribute map w.r.t. the vertices / attribute rows, given grad_out[l] ([b,h_l,w_l,c], or [b,c,h_l,w_l] with
 * SR_RASTER_CHW) and the level's gradient state win[l] / big[l].  work[l] >= sr_rasterize_grad_scratch_bytes(b, nf, c, 0)
 * each.  fp32, c <= 4, nf > 0 and the cached inverse incidence table adj_slot are required (SR_EINVAL otherwise: the
 * caller accumulates level by level). */
int sr_rasterize_grad_levels_f32(int n, int64_t b, int64_t nv, int64_t nf, const int64_t* h, const int64_t* w, int repeat_f,
                                 int perspective, const float* v, const float* tex, int64_t tex_c, const int64_t* tri,
                                 const int32_t* const* win, int32_t* const* big, const float* const* grad_out,
                                 const int32_t* adj_off, const int32_t* adj, int64_t off_bstride, int64_t adj_bstride,
                                 const int32_t* adj_slot, float* grad_v, float* grad_tex, float eps, void* const* work,
                                 sr_stream_t stream);

/* d(coeff)/d(vertex) per pixel.  Replaces  bool rasterize_gpu_backward<scalar,index>(b, n, h, w,
 *   repeat_v, perspective, const scalar* v, const index* i, scalar* dcoeff, scalar eps)
 * reference op/rasterize.cu:124-127 (arithmetic op/rasterize.h:169-228).  dcoeff [b,h,w,3,9];
 * every pixel is written (zeros where the reference leaves its torch::zeros untouched). */
int sr_rasterize_backward_f32(int64_t b, int64_t n, int64_t h, int64_t w, int repeat_v,
                              int perspective, const float* v, const int64_t* index, float* dcoeff,
                              float eps, sr_stream_t stream);
int sr_rasterize_backward_f64(int64_t b, int64_t n, int64_t h, int64_t w, int repeat_v,
                              int perspective, const double* v, const int64_t* index,
                              double* dcoeff, double eps, sr_stream_t stream);

/* Fused backward of `rasterize` (reference op/rasterize.py:39-80: dcoeff, [1x3]@[3x9], and two
 * sparse scatter matmuls) without materialising dcoeff or a COO matrix, and WITHOUT atomics — a
 * deterministic two-phase gather (run-to-run identical results):
 *   phase 1  per (sample, triangle): sums over the pixels the triangle won (`win` of the forward call), in
 *            pixel order, of (grad_out . tex[vertex_i]) * dcoeff[i, :] and grad_out * coeff_k — pixel-parallel
 *            with the triangle's first pixel as its leader; workgroup-cooperative for the triangles in `big`;
 *   phase 2  per (sample, vertex): sum over its incident triangles in the order of the incidence list.
 *   Between the phases the corner values live in VERTEX-MAJOR slots: position e of the (vertex-sorted) incidence list is
 *   the slot of that corner, so phase 1 scatters each corner to adj_slot[k * nf + f] and phase 2 reads ONE contiguous
 *   span per vertex (consecutive vertices: consecutive spans) instead of gathering scattered per-triangle records.
 *   grad_v  [b, nv, 3], grad_tex [b, nv, c]: every row is written (no pre-zeroing); either may be NULL.
 * v [b, nv, 3]; tex [b, nv, c]; tri int64 [nf, 3] (or [b, nf, 3] when !repeat_f); grad_out [b, h, w, c].
 * Incidence list (CSR, built once per topology by the caller): adj_off int32 [nv + 1], adj int32 [3 nf] holding
 * corner-major entries k * nf + f with tri[f][k] == vertex, ascending; per-sample topologies pass batch strides
 * (elements) adj_off_bstride / adj_bstride, shared ones pass 0.  adj_slot int32 [3 nf] (batch stride adj_bstride) is
 * the inverse permutation, adj_slot[adj[e]] = e, built once per topology next to the list; NULL = rebuilt by every
 * call inside `work` (one extra launch).
 * `work`: sr_rasterize_grad_scratch_bytes(b, nf, c, is_double) bytes. */
int64_t sr_rasterize_grad_scratch_bytes(int64_t b, int64_t nf, int64_t tex_c, int is_double);
int sr_rasterize_grad_f32(int64_t b, int64_t nv, int64_t nf, int64_t h, int64_t w, int repeat_f,
                          int perspective, const float* v, const float* tex, int64_t tex_c,
                          const int64_t* tri, const int32_t* win, const int32_t* big, const float* grad_out,
                          const int32_t* adj_off, const int32_t* adj, int64_t adj_off_bstride,
                          int64_t adj_bstride, const int32_t* adj_slot, float* grad_v, float* grad_tex, float eps,
                          void* work, sr_stream_t stream);
int sr_rasterize_grad_f64(int64_t b, int64_t nv, int64_t nf, int64_t h, int64_t w, int repeat_f,
                          int perspective, const double* v, const double* tex, int64_t tex_c,
                          const int64_t* tri, const int32_t* win, const int32_t* big, const double* grad_out,
                          const int32_t* adj_off, const int32_t* adj, int64_t adj_off_bstride,
                          int64_t adj_bstride, const int32_t* adj_slot, double* grad_v, double* grad_tex, double eps,
                          void* work, sr_stream_t stream);

/* Host (CPU) path for HOST pointers: the reference's extension also serves CPU tensors
 * (rasterize_cpu / rasterize_cpu_backward, reference op/rasterize.cpp:21-95, dispatched at :126-150).
 * Sequential loops on the same arithmetic as the kernels (this file's functions are __host__ __device__);
 * outputs are initialised by the callee; zbuf may be NULL.  No stream: runs on the calling thread. */
int sr_rasterize_forward_cpu_f32(int64_t b, int64_t nv, int64_t nf, int64_t h, int64_t w, int repeat_v,
                                 int repeat_f, int perspective, const float* v, const int64_t* tri,
                                 int64_t* index, float* coeff, float* zbuf, float eps);
int sr_rasterize_forward_cpu_f64(int64_t b, int64_t nv, int64_t nf, int64_t h, int64_t w, int repeat_v,
                                 int repeat_f, int perspective, const double* v, const int64_t* tri,
                                 int64_t* index, double* coeff, double* zbuf, double eps);
int sr_rasterize_backward_cpu_f32(int64_t b, int64_t n, int64_t h, int64_t w, int perspective,
                                  const float* v, const int64_t* index, float* dcoeff, float eps);
int sr_rasterize_backward_cpu_f64(int64_t b, int64_t n, int64_t h, int64_t w, int perspective,
                                  const double* v, const int64_t* index, double* dcoeff, double eps);

/* ---------------------------------------------------------------------------------------
 * Dense contraction of the modulated convolution on the matrix cores (exact fp32 MFMA).
 * The reference has no native code here: it calls torch's F.conv2d / F.conv_transpose2d with
 * groups = batch on per-sample weight copies (reference layers.py:293-323).  These entry points
 * are what a host binding calls instead.
 *
 *   out[b,n,oy,ox] = oscale[b,n] * sum_{ky,kx,c} wt[ky*k+kx][c][n] * iscale[b,c] * in[b,c,iy,ix] + obias[n]
 *
 *   in  [B, C, IH, IW]   out [B, N, OH, OW]   wt [k*k, C, wt_ld] (row pitch wt_ld >= N, a multiple
 *   of 4 floats, base 16-byte aligned; columns N..wt_ld-1 are padding and may hold anything)
 *   iscale [B, C] | NULL   oscale [B, N] | NULL   obias [N] | NULL
 *   transposed = 0: correlation, iy = oy*stride + ky - pad   (k in {1,3}, stride in {1,2})
 *   transposed = 1: k = 3, stride = 2, pad = 0: out[2y+ky, 2x+kx] += in[y,x] * wt[ky*3+kx]
 *                   (OH = 2*IH + 1), the stride-2 transposed conv of the upsampling layers.
 *   scratch: sr_conv2d_scratch_floats(...) floats (0 for large maps) for the split-K partial sums
 *   of small feature maps, reduced in fixed order (deterministic); NULL disables the split. */
int64_t sr_conv2d_scratch_floats(int64_t B, int64_t C, int64_t N, int64_t IH, int64_t IW, int64_t OH,
                                 int64_t OW, int ksize, int stride, int pad, int transposed);
int sr_conv2d_mfma(float* out, const float* in, const float* wt, const float* iscale,
                   const float* oscale, const float* obias, int64_t B, int64_t C, int64_t N,
                   int64_t wt_ld, int64_t IH, int64_t IW, int64_t OH, int64_t OW, int ksize, int stride,
                   int pad, int transposed, float* scratch, sr_stream_t stream);
/* The modulated 3x3 stride-1 pad-1 convolution with the StyledConv tail (reference model.py:26-32) fused into
 * its store: out = lrelu((oscale*conv(iscale*in, wt) + noise_w[0]*noise[b, p]) + abias[n], alpha) * gain.
 * Served by the Winograd kernel only: SR_EINVAL when the shape is not eligible (H % 8, W % 32, C % 8, N % 64,
 * C <= 512) — the caller then uses sr_conv2d_mfma + sr_noise_bias_act.  scratch: sr_conv2d_scratch_floats. */
int sr_conv2d_nba(float* out, const float* in, const float* wt, const float* iscale, const float* oscale,
                  const float* noise, const float* noise_w, const float* abias, float alpha, float gain, int64_t B,
                  int64_t C, int64_t N, int64_t wt_ld, int64_t H, int64_t W, int64_t noise_bstride, float* scratch,
                  sr_stream_t stream);

/* The same two entry points with a `flags` word.  SR_CONV_U_READY: `scratch` is the buffer an EARLIER call with the same
 * `wt`, C, N (and the same call geometry) used and nobody has written since — its leading block still holds the
 * Winograd-domain weights, so their preparation (k_wino_weights, one launch per call) is skipped.  For frozen networks
 * (latent inversion, sampling): the caller keeps one scratch per (weight, geometry).  Ignored on the direct path. */
#define SR_CONV_U_READY 1
/* 1 when a stride-1 3x3 call with these sizes and THESE buffers (16-byte alignment of in / out is part of the rule) is
 * served by the Winograd kernel, 0 when by the direct one — what a caller that keeps a scratch for SR_CONV_U_READY
 * must ask before it marks the scratch's weight block as written. */
int sr_conv2d_uses_winograd(int64_t B, int64_t C, int64_t N, int64_t IH, int64_t IW, const float* in, const float* out);
/* Which kernel family serves a sr_conv2d_mfma(_ex) call — the decision the launch itself makes (one dispatch plan,
 * DESIGN.md 4.0), for callers that keep state per path and for tests.  Shape arguments as sr_conv2d_scratch_floats;
 * in / out / wt / wt_ld as the call would pass them (alignment is part of several rules; NULL = assume aligned);
 * have_scratch: 0 when the call passes scratch = NULL (no path that needs scratch is taken then).  Nothing is launched.
 * Returns SR_CONV_PATH_INVALID for a geometry sr_conv2d_mfma rejects, else one of the values below, with
 * SR_CONV_PATH_STRIPS or-ed in when the transposed convolution's border (output row 2*IH, column 2*IW) runs as the
 * two strip launches behind an interior kernel (otherwise as per-phase launches of the direct kernel). */
#define SR_CONV_PATH_INVALID (-1)
#define SR_CONV_PATH_DIRECT 0         /* k_conv_mfma; transposed: its per-phase launches */
#define SR_CONV_PATH_WINO 1           /* 3x3 s1 p1: Winograd F(2x2,3x3), k_conv_wino */
#define SR_CONV_PATH_S2_BF16 2        /* 3x3 s2 p0: split-bf16 (SR_CONV_SPLIT_BF16) */
#define SR_CONV_PATH_S2_WINO 3        /* 3x3 s2 p0: polyphase 25-product form, k_conv_s2_wino */
#define SR_CONV_PATH_GEMM1X1 4        /* 1x1 s1 p0: plain GEMM, k_conv1x1_gemm */
#define SR_CONV_PATH_CONVT_TAPS 5     /* transposed: tap-split, nine shifted 1x1 convolutions + k_convt_tap_reduce */
#define SR_CONV_PATH_CONVT_BF16 6     /* transposed: interior by split-bf16 (SR_CONV_SPLIT_BF16) */
#define SR_CONV_PATH_CONVT_FUSED_KS 7 /* transposed: interior by k_convt_fused in K slices + k_convt_fused_reduce */
#define SR_CONV_PATH_CONVT_FUSED 8    /* transposed: interior by k_convt_fused */
#define SR_CONV_PATH_CONVT_WINO 9     /* transposed: interior by the 25-product form, k_convt_wino */
#define SR_CONV_PATH_STRIPS 0x100
int sr_conv2d_path(int64_t B, int64_t C, int64_t N, int64_t IH, int64_t IW, int64_t OH, int64_t OW, int ksize, int stride,
                   int pad, int transposed, const float* in, const float* out, const float* wt, int64_t wt_ld,
                   int have_scratch);
/* Scratch floats the path sr_conv2d_path returns cannot run without (for SR_CONV_PATH_DIRECT: what its split-K would use;
 * it takes what it is given) — never more than sr_conv2d_scratch_floats of the same shape.  -1 for an invalid geometry. */
int64_t sr_conv2d_path_floats(int64_t B, int64_t C, int64_t N, int64_t IH, int64_t IW, int64_t OH, int64_t OW, int ksize,
                              int stride, int pad, int transposed, const float* in, const float* out, const float* wt,
                              int64_t wt_ld, int have_scratch);

/* Generic-geometry convolution (csrc/conv_generic.hip): any kernel extent kh x kw, stride (sy, sx) and zero padding
 * (py, px), dilation 1, one group, weights in the reference's layout [N, C, kh, kw] — what the reference's EqualConv2d
 * (layers.py:204-221: F.conv2d with any kernel_size / stride / padding) and ModulatedConv2d with kernel_size other than
 * 1 or 3 (layers.py:259-323, F.conv2d / F.conv_transpose2d) reach outside the matrix-core geometries above; replaces the
 * MIOpen call a device tensor would otherwise make.  Direct fp32 kernels, fixed summation order.
 *   sr_conv2d_generic        y [B,N,OH,OW] = conv(x [B,C,IH,IW], w) (+ bias[N] or NULL); OH = (IH + 2 py - kh) / sy + 1
 *   sr_conv2d_generic_dgrad  dx [B,C,IH,IW] = its gradient w.r.t. x for g [B,N,OH,OW]; ALSO F.conv_transpose2d(g, w,
 *                            stride, padding) as a forward operator (w then reads [in = N, out = C, kh, kw])
 *   sr_conv2d_generic_wgrad  dw [N,C,kh,kw] = its gradient w.r.t. w
 * SR_EINVAL when (OH, OW) is not the convolution's extent for (IH, IW); SR_ERANGE past 65535 (sample, channel) planes. */
int sr_conv2d_generic(float* y, const float* x, const float* w, const float* bias, int64_t B, int64_t C, int64_t N,
                      int64_t IH, int64_t IW, int64_t OH, int64_t OW, int kh, int kw, int sy, int sx, int py, int px,
                      sr_stream_t stream);
int sr_conv2d_generic_dgrad(float* dx, const float* g, const float* w, int64_t B, int64_t C, int64_t N, int64_t IH,
                            int64_t IW, int64_t OH, int64_t OW, int kh, int kw, int sy, int sx, int py, int px,
                            sr_stream_t stream);
int sr_conv2d_generic_wgrad(float* dw, const float* x, const float* g, int64_t B, int64_t C, int64_t N, int64_t IH,
                            int64_t IW, int64_t OH, int64_t OW, int kh, int kw, int sy, int sx, int py, int px,
                            sr_stream_t stream);
int sr_conv2d_mfma_ex(float* out, const float* in, const float* wt, const float* iscale,
                      const float* oscale, const float* obias, int64_t B, int64_t C, int64_t N,
                      int64_t wt_ld, int64_t IH, int64_t IW, int64_t OH, int64_t OW, int ksize,
                      int stride, int pad, int transposed, int flags, float* scratch, sr_stream_t stream);
/* out = oscale[b,n] * conv1x1(in, wt)[b,n,p] + addend[b,n,p]  (stride 1, no window; P = pixels per plane): the skip branch of the
 * discriminator's ResBlock with the sum of the two branches in its store (reference model.py: ResBlock.forward
 * `(out + skip) / sqrt(2)`, the factor folded into oscale and the other branch's gain).  _supported: 1 when the GEMM-shaped
 * kernel takes the call (C % 16, N % 128, P % 128, 16-byte aligned operands, enough tiles), else the caller adds separately. */
int sr_conv1x1_add_supported(int64_t B, int64_t C, int64_t N, int64_t wt_ld, int64_t P, const float* in, const float* wt,
                             const float* out, const float* addend);
int sr_conv1x1_add(float* out, const float* in, const float* wt, const float* oscale, const float* addend, int64_t B,
                   int64_t C, int64_t N, int64_t wt_ld, int64_t P, sr_stream_t stream);
int sr_conv2d_nba_ex(float* out, const float* in, const float* wt, const float* iscale, const float* oscale,
                     const float* noise, const float* noise_w, const float* abias, float alpha, float gain,
                     int64_t B, int64_t C, int64_t N, int64_t wt_ld, int64_t H, int64_t W, int64_t noise_bstride,
                     int flags, float* scratch, sr_stream_t stream);

/* Weight gradient of sr_conv2d_mfma (same geometry arguments):
 *   dwt[ky*k+kx][c][n] = sum_{b, pixels} (xscale[b,c] * x[b,c,window]) * (gscale[b,n] * gy[b,n,pixel])
 * x [B,C,IH,IW], gy [B,N,OH,OW], dwt [k*k, C, N]; xscale / gscale may be NULL.  The batch is folded
 * into the reduction (the reference's grouped convolution would give per-sample gradients).
 * `scratch`: sr_conv2d_wgrad_scratch_floats(...) floats of split-K partial sums, reduced in a
 * fixed order (deterministic). */
int64_t sr_conv2d_wgrad_scratch_floats(int64_t B, int64_t C, int64_t N, int64_t IH, int64_t IW,
                                       int64_t OH, int64_t OW, int ksize, int stride, int pad,
                                       int transposed);
int sr_conv2d_wgrad_mfma(float* dwt, const float* x, const float* gy, const float* xscale,
                         const float* gscale, int64_t B, int64_t C, int64_t N, int64_t IH,
                         int64_t IW, int64_t OH, int64_t OW, int ksize, int stride, int pad,
                         int transposed, float* scratch, sr_stream_t stream);
/* Which kernel serves a sr_conv2d_wgrad_mfma call with these sizes and buffers (NULL = assume aligned), mirroring
 * sr_conv2d_path; SR_WGRAD_PATH_INVALID for a geometry the call rejects. */
#define SR_WGRAD_PATH_INVALID (-1)
#define SR_WGRAD_PATH_DIRECT 0   /* k_wgrad_mfma */
#define SR_WGRAD_PATH_SMALL3 1   /* 3x3 s1 p1 with <= 4 x <= 4 channels: streaming k_wgrad_small3 */
#define SR_WGRAD_PATH_WINO 2     /* 3x3 s1 p1: Winograd, k_wgrad_wino */
#define SR_WGRAD_PATH_BF16_1X1 3 /* 1x1 s1 p0: split-bf16 (SR_CONV_SPLIT_BF16) */
#define SR_WGRAD_PATH_BF16_S2 4  /* 3x3 s2 p0, either direction: split-bf16 (SR_CONV_SPLIT_BF16) */
#define SR_WGRAD_PATH_S2_DMA 5   /* 3x3 s2 p0, either direction: k_wgrad_s2_dma */
#define SR_WGRAD_PATH_S2_WINO 6  /* 3x3 s2 p0, either direction: polyphase 25-product k_wgrad_s2p + k_wgrad_s2p_finish */
int sr_conv2d_wgrad_path(int64_t B, int64_t C, int64_t N, int64_t IH, int64_t IW, int64_t OH, int64_t OW, int ksize,
                         int stride, int pad, int transposed, const float* x, const float* gy);
/* Scratch floats the path sr_conv2d_wgrad_path returns writes — never more than sr_conv2d_wgrad_scratch_floats of the
 * same shape.  -1 for an invalid geometry. */
int64_t sr_conv2d_wgrad_path_floats(int64_t B, int64_t C, int64_t N, int64_t IH, int64_t IW, int64_t OH, int64_t OW,
                                    int ksize, int stride, int pad, int transposed, const float* x, const float* gy);
/* Weight gradient AND style gradient of y = gscale * conv(iscale (.) x, wt) from one pass over x and gy:
 *   dwt as sr_conv2d_wgrad_mfma(xscale = iscale);   gis[b][c] = sum_{t,n} wt[t][c][n] * P_b[t][c][n]  (= sum_p x * dx_unscaled),
 * P_b the weight gradient of sample b without the style.  Served where the call's path is SR_WGRAD_PATH_WINO, or
 * SR_WGRAD_PATH_S2_WINO of a transposed convolution, and its K slices do not straddle samples: the finish kernel then
 * forms both from the per-sample partial slabs in a fixed order (deterministic, no atomics).
 * sr_conv2d_wgrad_style_floats: floats of `part` for such a call, -1 for every other call (which keeps
 * sr_conv2d_wgrad_mfma and a row-dot pass; sr_conv2d_wgrad_style returns SR_EINVAL for it).
 * wt [9][C][ldw] is the forward weight (ldw >= N), iscale [B][C] required, gscale [B][N] or NULL;
 * `scratch`: sr_conv2d_wgrad_scratch_floats(...) floats. */
int64_t sr_conv2d_wgrad_style_floats(int64_t B, int64_t C, int64_t N, int64_t IH, int64_t IW, int64_t OH, int64_t OW,
                                     int ksize, int stride, int pad, int transposed, const float* x, const float* gy);
int sr_conv2d_wgrad_style(float* dwt, float* gis, const float* x, const float* gy, const float* iscale,
                          const float* gscale, const float* wt, int64_t ldw, int64_t B, int64_t C, int64_t N, int64_t IH,
                          int64_t IW, int64_t OH, int64_t OW, int ksize, int stride, int pad, int transposed,
                          float* scratch, float* part, sr_stream_t stream);

/* ---- signalling out of a replayed hipGraph (overlapped gradient all-reduce) -----------------------------------
 * The reference overlaps the gradient all-reduce with the backward through torch DDP's bucket hooks
 * (reference distributed.py:98-105, used for the path-length step at train.py:335-352).  This build replays each
 * training phase as ONE hipGraph; a bucket of the flat gradient buffer that is complete in the middle of that graph
 * is announced by a one-lane kernel node.  sr_signal_set stores `*epoch` (a device word the host writes, in stream
 * order, in front of every replay it launches) into `*word` once all work enqueued before it on `stream` has finished;
 * sr_signal_bump is the incrementing form (`*counter += 1`).  sr_signal_wait enqueues a one-lane kernel on another
 * stream that returns when `*counter - at_least >= 0` (signed 32-bit distance): with at_least = the epoch of the replay
 * just launched, everything enqueued behind it starts at that point of the replay.  The producer must already be
 * enqueued when the wait is (the wait spins on the device).  sr_signal_wait_timeout gives up after `timeout_us`
 * (0 = never): it stores `code` into `*status_host` (pinned host memory the caller polls; may be NULL) and returns, so
 * a lost signal becomes a host-side error instead of a silent device-side spin. */
int sr_signal_bump(uint32_t* counter, sr_stream_t stream);
int sr_signal_set(uint32_t* word, const uint32_t* epoch, sr_stream_t stream);
int sr_signal_wait(const uint32_t* counter, uint32_t at_least, sr_stream_t stream);
int sr_signal_wait_timeout(const uint32_t* counter, uint32_t at_least, uint64_t timeout_us, int32_t* status_host,
                           int32_t code, sr_stream_t stream);
/* As sr_signal_wait_timeout; on expiry `*poison` (a float of the data the wait guards, may be NULL) is overwritten
 * with NaN before the kernel returns: what is queued behind the wait then carries a marker that
 * sr_adam_flat_guarded refuses. */
int sr_signal_wait_poison(const uint32_t* counter, uint32_t at_least, uint64_t timeout_us, int32_t* status_host,
                          int32_t code, float* poison, sr_stream_t stream);
/* sr_signal_set for a word in pinned HOST memory (system-scope store): the host-released mode of the bucketed reducer
 * polls it from the CPU and queues the collective itself — no kernel ever spins on the communication stream, so the
 * mode does not depend on the two streams owning separate hardware queues (GPU_MAX_HW_QUEUES). */
int sr_signal_set_host(uint32_t* word_host, const uint32_t* epoch, sr_stream_t stream);

/* Repairs a captured, not yet instantiated hipGraph_t for the HIP 7.0 runtime PyTorch-ROCm 2.10 bundles: memset nodes
 * replay a corrupted value from the second launch on (torch's multi-block reductions zero their semaphores that way),
 * so each memset node is replaced by a fill-kernel node with the same edges.  `replaced` receives the count.  The
 * reference has no counterpart: it never captures its step (train.py enqueues ~4 000 launches per iteration). */
int sr_graph_replace_memset_nodes(void* hip_graph, int* replaced);
/* Number of kernel nodes / of all nodes of a captured hipGraph_t (launch census of a replayed phase: bench.py reports
 * launches per step beside the device time). */
int sr_graph_node_count(void* graph, int* kernel_nodes, int* all_nodes);

/* One layer of the LPIPS distance (reference lpips/networks_basic.py:62-85 + lpips/__init__.py:42-44: normalize_tensor,
 * squared difference, 1x1 `lin` convolution, spatial average) fused — used by the latent-inversion loop:
 *   d[b] = mean_hw sum_c lin[c] * (f0[b,c,p] / (sqrt(sum_c f0^2) + eps) - t[b,c,p])^2
 * f0 [b, c, hw] raw features, t [b | 1, c, hw] NORMALISED target features (t_bstride = c*hw or 0), lin [c].
 * sr_lpips_layer_bwd: gf = d(sum_b gd[b] d[b]) / d f0.  scratch: sr_lpips_layer_scratch_floats(b, hw) floats. */
int64_t sr_lpips_layer_scratch_floats(int64_t b, int64_t hw);
int sr_lpips_layer_fwd(float* d, const float* f0, const float* t, const float* lin, int64_t b, int64_t c, int64_t hw,
                       int64_t t_bstride, float eps, float* scratch, sr_stream_t stream);
int sr_lpips_layer_bwd(float* gf, const float* gd, const float* f0, const float* t, const float* lin, int64_t b,
                       int64_t c, int64_t hw, int64_t t_bstride, float eps, sr_stream_t stream);
/* Perceptual path length (reference ppl.py:93-178), the glue around the mapping network, the generator and the LPIPS
 * trunk.
 * sr_ppl_endpoints: the latents of npairs pairs at t and t + eps, one wave per pair.  Pair i reads a + i * in_stride and
 * b + i * in_stride ([d] each; the sampled [2B, d] tensor read as pairs is a = x, b = x + d, in_stride = 2 d) and t[i];
 * it writes out[(i * n_ends + e) * d ...], e = 0 at t[i] and (n_ends = 2) e = 1 at t[i] + eps, rounded to fp32.
 *   mode 0 (w, ppl.py:14-19 `lerp(t[:, None], a, b)`): out = (0 + a (1 - t)) + b t, bit-identical to torch's fp32 ops;
 *   mode 1 (z, ppl.py:102-112 two-input `slerp`): a^ = a / max(|a|, 1e-8) (layers.py:13-24 'L2'), b^ likewise,
 *     w = acos(a^ . b^) without clamp, out = normalize(sin(w (1 - t)) a^ + sin(w t) b^); a few ulp from libm. */
int sr_ppl_endpoints(float* out, const float* a, const float* b, int64_t in_stride, const float* t, int64_t npairs,
                     int64_t d, int mode, int n_ends, float eps, sr_stream_t stream);
/* sr_ppl_prep: generator images img [n, 3, h, w] -> LPIPS trunk input out [n, 3, oh, ow]: the crop window rows
 * y0 .. y0 + ch, columns x0 .. x0 + cw (ppl.py:159-161 --crop), resized when (oh, ow) != (ch, cw) exactly as
 * F.interpolate(mode='bilinear', align_corners=False) without antialias (ppl.py:162-165), then the ScalingLayer
 * (x - shift[c]) / scale[c] (lpips/networks_basic.py:94-101; shift, scale [3] device arrays). */
int sr_ppl_prep(float* out, const float* img, const float* shift, const float* scale, int64_t n, int64_t h, int64_t w,
                int64_t y0, int64_t x0, int64_t ch, int64_t cw, int64_t oh, int64_t ow, sr_stream_t stream);
/* sr_lpips_pair: the LPIPS distance of every pair of interleaved samples (2i, 2i+1) straight from the raw trunk
 * features (replaces normalize_tensor on full tensors + PNetLin per-layer terms, lpips/__init__.py:42-44,
 * networks_basic.py:66-76):
 *   d[i] = (sum_k mean_hw sum_c lin_k[c] (f0/n0 - f1/n1)^2) / div,   n = sqrt(sum_c f^2) + 1e-10
 * f[k] [2 npairs, c[k], hw[k]] and lin[k] [c[k]] are device pointers held in HOST arrays of n_layers (<= 8) entries;
 * div is eps^2 for PPL.  Two launches (all layers, then a fixed-order finish), no atomics: deterministic.
 * scratch: sr_lpips_pair_scratch_floats(npairs, n_layers, hw) floats. */
int64_t sr_lpips_pair_scratch_floats(int64_t npairs, int64_t n_layers, const int64_t* hw);
int sr_lpips_pair(float* d, const float* const* f, const float* const* lin, const int64_t* c, const int64_t* hw,
                  int64_t n_layers, int64_t npairs, float div, float* scratch, sr_stream_t stream);
/* FID Inception-v3 trunk (reference inception.py InceptionV3([3]) on fid_inception_v3) and FID feature statistics,
 * csrc/inception.hip.  Forward only, float32 NCHW.
 * sr_incep_conv: BasicConv2d with BatchNorm folded in: out = relu(conv(in, wt) + bias), in [B, C, H, W], wt [K, M] with
 * K = C * kh * kw in (c, ky, kx) order (the [M, C, kh, kw] weight transposed), bias [M].  kh, kw in {1, 3, 5, 7},
 * one stride (1 or 2) for both axes, padding ph / pw, OH = (H + 2 ph - kh) / stride + 1 (OW likewise).  GEMM rows
 * seg_m0[s] .. seg_m0[s + 1] (the last to M; seg_m0[0] = 0, nseg <= 3) go to seg_out[s] [B, seg_ctot[s], OH, OW] at
 * channel seg_coff[s]: a branch writes into its slice of the block's concatenated output, and the 1x1 heads of a block
 * run as one GEMM.  seg_out / seg_m0 / seg_coff / seg_ctot are HOST arrays of nseg entries. */
int sr_incep_conv(const float* in, const float* wt, const float* bias, int64_t B, int64_t C, int64_t H, int64_t W,
                  int64_t M, int kh, int kw, int stride, int ph, int pw, int nseg, float* const* seg_out,
                  const int64_t* seg_m0, const int64_t* seg_coff, const int64_t* seg_ctot, sr_stream_t stream);
/* sr_incep_pool: in [B, C, H, W] -> channels coff .. coff + C of out [B, ctot, OH, OW].  mode 0: max 3x3 stride 2 no
 * padding (OH = (H - 3) / 2 + 1); mode 1: average 3x3 stride 1 padding 1 over the in-map taps only
 * (count_include_pad=False); mode 2: max 3x3 stride 1 padding 1. */
int sr_incep_pool(float* out, const float* in, int64_t B, int64_t C, int64_t H, int64_t W, int mode, int64_t coff,
                  int64_t ctot, sr_stream_t stream);
/* sr_incep_gap: out[p] = mean of in[p * hw .. (p + 1) * hw), summed in order (adaptive average pool to 1 x 1). */
int sr_incep_gap(float* out, const float* in, int64_t planes, int64_t hw, sr_stream_t stream);
/* FID feature statistics in fp64 over rows of float32 features f [n, d]: first != 0 sets shift[d] = the mean of this
 * batch; every call adds sum[j] += sum_r (f[r, j] - shift[j]) and, on the upper 64 x 64 tiles of gram [d, d],
 * gram[i, j] += sum_r (f[r, i] - shift[i]) (f[r, j] - shift[j]), rows in order, no atomics (deterministic).
 * sr_fstats_finalize: mean[d] = shift + sum / count, cov[d, d] = (gram - sum sum^T / count) / (count - 1). */
int sr_fstats_update(double* sum, double* gram, double* shift, const float* f, int64_t n, int64_t d, int first,
                     sr_stream_t stream);
int sr_fstats_finalize(double* mean, double* cov, const double* sum, const double* gram, const double* shift,
                       int64_t count, int64_t d, sr_stream_t stream);
/* Pixel term of the inversion loss (BASELINE config[4]): out[0] = mean((a - b)^2) over n elements (one workgroup, fixed
 * order), and ga = gout[0] * 2 / n * (a - b).  a, b 16-byte aligned for the forward. */
int sr_mse_fwd(float* out, const float* a, const float* b, int64_t n, sr_stream_t stream);
int sr_mse_bwd(float* ga, const float* gout, const float* a, const float* b, int64_t n, sr_stream_t stream);
/* Per-sample terms of the batched inversion loss (B targets, objective sum_b L_b), csrc/lpips.hip.
 * sr_mse_rows_fwd: out[b] = mean((a[b] - t[b])^2) over the n elements of row b of [B, n] (B <= 65535); a fixed-order
 *   two-level reduction (chunk partials into scratch [sr_mse_rows_scratch_floats], then one wave per row), no atomics.
 *   a, t 4-byte aligned (float4 loads on the aligned body when both are 16-byte aligned, scalar head and tail).
 * sr_mse_rows_bwd: ga[b, i] = gout[b] * 2 / n * (a[b, i] - t[b, i]).
 * sr_fit_loss_rows: rows[b] = d0[b] + d1[b] + d2[b] + d3[b] + d4[b] + pixel_weight * mse[b]
 *   (+ shape_reg * sum_k (coeff[b, k] / sigma[k])^2 when coeff [B, d] is not NULL; sigma NULL: 1), the five LPIPS layer
 *   distances [B] each; total[0] = sum_b rows[b] in sample order.  One launch.
 * sr_fit_loss_rows_bwd: gd[b] = gtotal[0] (the gradient of every layer distance) and gmse[b] = pixel_weight * gtotal[0]
 *   (gmse may be NULL).  The prior's gradient is not formed here: the morph node's scalar reg carries it. */
int64_t sr_mse_rows_scratch_floats(int64_t B, int64_t n);
int sr_mse_rows_fwd(float* out, const float* a, const float* t, int64_t B, int64_t n, float* scratch,
                    sr_stream_t stream);
int sr_mse_rows_bwd(float* ga, const float* gout, const float* a, const float* t, int64_t B, int64_t n,
                    sr_stream_t stream);
int sr_fit_loss_rows(float* rows, float* total, const float* d0, const float* d1, const float* d2, const float* d3,
                     const float* d4, const float* mse, float pixel_weight, const float* coeff, const float* sigma,
                     float shape_reg, int64_t B, int64_t d, sr_stream_t stream);
int sr_fit_loss_rows_bwd(float* gd, float* gmse, const float* gtotal, float pixel_weight, int64_t B, sr_stream_t stream);
/* 2 x 2 / stride 2 max pooling of the LPIPS trunk (reference lpips/pretrained_networks.py:97-135, torchvision VGG16
 * features 4 / 9 / 16 / 23) over `planes` maps of ih x iw (both even), and its gradient: gx gets gy at the arg-max of
 * every window (first maximum in row-major order, a NaN wins — torch.nn.functional.max_pool2d's rule) and zero elsewhere;
 * every input pixel is written. */
int sr_maxpool2_fwd(float* out, const float* x, int64_t planes, int64_t ih, int64_t iw, sr_stream_t stream);
int sr_maxpool2_bwd(float* gx, const float* gy, const float* x, int64_t planes, int64_t ih, int64_t iw, sr_stream_t stream);

/* Adaptive discriminator augmentation (reference utils_3d.py:155-359 `augment`, train.py:269-280), csrc/augment.hip.
 * Float32 NCHW images with 3 channels, any B <= 65535, H, W.  Every entry point is one or two launches, allocation-free
 * and never reads back to the host: they all run under graph capture.
 * sr_ada_params: draws [B, SR_ADA_NDRAW] standard normals -> rec [B, SR_ADA_REC], one lane per sample, in fp64:
 *   draws 0..4  pose: tx, ty, rotation, log-zoom (sigma pose_p[0..3], mean pose_p[4]), flip (u < pose_p[5])
 *   draws 5..9  colour: brightness, log-contrast (sigma color_p[0..1]), luma flip (u < color_p[2]), hue,
 *               log-saturation (sigma color_p[3..4])
 *   draw 10     select (u < p, p = *p_dev when p_dev is not NULL, else p_host)
 * where u = Phi(draw) for the three uniform slots.  pose_p [6] and color_p [5] are HOST arrays (|.| is taken).
 *   rec[0..11]  six DOUBLES (rec 8-byte aligned): the output-pixel -> source-pixel affine map, ix = a0 x + a1 y + a2,
 *               iy = a3 x + a4 y + a5, i.e. the composite's grid (pad=None: the zoom raised until no border shows)
 *               under grid_sample(align_corners=True); source coordinates are evaluated in fp64
 *   rec[12..23] the 3 x 4 colour matrix, row-major;  rec[24]  1 if the sample is augmented, else 0;  rec[25..27]  0
 * sr_ada_apply: out = C[:, :3] bilinear(img, A (x, y)) + with_bias * C[:, 3] for a selected sample (taps outside the
 *   image contribute 0), out = img otherwise (bit for bit).  out must not alias img.
 * sr_ada_apply_grad: the adjoint in the image (of the with_bias = 0 map): gin = Bilinear^T (C[:, :3]^T gout) for a
 *   selected sample, gin = gout otherwise.  A gather in a fixed order, no atomics: reruns are bit-identical.
 * sr_ada_update: state [4] fp64 = {sum of sign(D(real)), count, p, r_t}; adds stat [2] (this iteration's sign sum and
 *   count, already summed over ranks) and, once the count exceeds 255, sets r_t = sum / count,
 *   p = clamp(p + ((sign(r_t - target) * target) / length) * count, 0, 1) and zeroes the sums (train.Trainer.step). */
#define SR_ADA_NDRAW 11
#define SR_ADA_REC 28
int sr_ada_params(float* rec, const float* draws, int64_t B, const float* pose_p, const float* color_p, const double* p_dev,
                  double p_host, int64_t H, int64_t W, sr_stream_t stream);
int sr_ada_apply(float* out, const float* img, const float* rec, int64_t B, int64_t H, int64_t W, int with_bias,
                 sr_stream_t stream);
int sr_ada_apply_grad(float* gin, const float* gout, const float* rec, int64_t B, int64_t H, int64_t W, sr_stream_t stream);
int sr_ada_update(double* state, const float* stat, double target, double length, sr_stream_t stream);

/* Pillow-exact resampling of uint8 images (Pillow's ImagingResample for 8-bit pixels), csrc/resample.hip.
 * in uint8 [N, H, W, C] contiguous, C in {1, 3, 4}, resized to the virtual image [N, oh, ow, C] of which the window
 * rows oy0 .. oy0 + ohw, columns ox0 .. ox0 + oww is written: out_form 0: uint8 [N, ohw, oww, C]; 1: float32
 * [N, C, ohw, oww] = (v / 255 - 0.5) / 0.5.  Two separable passes, horizontal first into `scratch`
 * (sr_resample_u8_scratch_bytes; 0 when a pass is skipped); each output byte is clip(0, 255, (2^21 + sum_t
 * pixel[first + t] * k[t]) >> 22) in int32.  A pass whose axis keeps its size is skipped and takes NULL tables.
 * Per axis the caller supplies Pillow's 22-bit fixed-point tables (stylerenderer_amd/op/resample.py coefficients()):
 *   coeffs_h_t     DEVICE int32 [ksize_h, ow]: the [ow, ksize_h] table TRANSPOSED;  coeffs_v  DEVICE int32 [oh, ksize_v]
 *   bounds_h / _v  DEVICE int32 [out, 2] = (first source index, tap count); bounds_*_host the same array on the HOST
 *                  (validated against the source size and used to size the passes; first and first + count must not
 *                  decrease along the axis)
 * mul24 != 0 promises |k| < 2^23 for every coefficient (the 24-bit multiply-add is used).  One or two launches on
 * `stream`, no allocation, no host synchronisation; N, ohw <= 65535. */
int64_t sr_resample_u8_scratch_bytes(int64_t N, int64_t H, int64_t W, int64_t C, int64_t oh, int64_t ow,
                                     const int32_t* bounds_v_host, int64_t oy0, int64_t ox0, int64_t ohw, int64_t oww);
int sr_resample_u8(void* out, const uint8_t* in, int64_t N, int64_t H, int64_t W, int64_t C, int64_t oh, int64_t ow,
                   const int32_t* coeffs_h_t, const int32_t* bounds_h, const int32_t* bounds_h_host, int64_t ksize_h,
                   const int32_t* coeffs_v, const int32_t* bounds_v, const int32_t* bounds_v_host, int64_t ksize_v,
                   int64_t oy0, int64_t ox0, int64_t ohw, int64_t oww, int out_form, int mul24, uint8_t* scratch,
                   sr_stream_t stream);

/* Pillow-exact bilinear affine warp of uint8 images (Pillow's Image.transform(AFFINE, BILINEAR)), csrc/warp.hip.
 * in uint8 [N, H, W, C] contiguous, C in {1, 3, 4}; matrix DEVICE float64 [N, 6] (matrix_stride = 6) or [6] shared by
 * the batch (matrix_stride = 0), in Pillow's pixel-centre convention.  For output pixel (x, y), all in float64, left to
 * right, no fused multiply-add: xs = x + .5, ys = y + .5, xin = a0 xs + a1 ys + a2, yin = a3 xs + a4 ys + a5,
 * xf = xin - .5, x0 = floor(xf), dx = xf - x0 (likewise y); x0, y0 are clamped to [-2^30, 2^30]; the taps (x0, x0 + 1) x
 * (y0, y0 + 1) are mapped into the image by `border`; v1 = p00 + (p01 - p00) dx, v2 = p10 + (p11 - p10) dx,
 * v = v1 + (v2 - v1) dy, byte = (uint8) v by truncation.
 * border 0: replicate (clamp); 1: reflect (fedcba|abcdef|fedcba, periodic); 2: constant: `fill` where (xin, yin) is
 * outside [0, W) x [0, H) (or not a number), clamp elsewhere.
 * out_form 0: uint8 [N, oh, ow, C]; 1: float32 [N, C, oh, ow] = (v / 255 - 0.5) / 0.5.  One launch on `stream`, no
 * allocation, no host synchronisation; N <= 65535, oh < 2^20, H, W <= 2^24. */
int sr_warp_affine_u8(void* out, const uint8_t* in, const double* matrix, int64_t matrix_stride, int64_t N, int64_t H,
                      int64_t W, int64_t C, int64_t oh, int64_t ow, int border, int fill, int out_form,
                      sr_stream_t stream);

/* Landmark reprojection term of face reconstruction (stylerenderer_amd/op/landmark.py holds the definition),
 * csrc/landmark.hip.  Landmark l of an embedding idx int32 [L, 3], bary float32 [L, 3] is P_l = sum_k bary[l, k]
 * v[b, idx[l, k], :] of the posed vertices v [B, nv, 3]; its pixel is p_l = ((1 + P_l.x) W / 2 - 1/2,
 * (1 - P_l.y) H / 2 - 1/2), the rasterizer's index coordinates.  With targets target [B, L, 2] in those coordinates,
 * weights conf [B, L] >= 0 (0: missing) and rho = smooth-L1 with `beta` per coordinate:
 *   rows[b] = weight * (2 / max(W, H)) * sum_l conf[b, l] (rho(e_l.x) + rho(e_l.y)) / max(sum_l conf[b, l], 1e-12)
 * sr_landmark_loss_fwd: one launch, one workgroup per sample; writes rows [B], p [B, L, 2] and g [B, L, 2] =
 *   d rows[b] / d p_l.  The sum over l has a fixed order (lane-strided, then an LDS tree): reruns are bit-identical.
 *   Every idx must lie in [0, nv): the caller validates (op/landmark.py does when it builds the CSR list).
 * sr_landmark_loss_bwd: one launch over all B nv vertices; writes (accumulate = 0) or adds to (accumulate != 0) the dense
 *   gv [B, nv, 3] = g_rows[b] * d rows[b] / d v, z = 0, zero on vertices no landmark uses.  csr_off int32 [nv + 1] and
 *   csr_l int32 / csr_w float32 [entries] list for every vertex the landmarks l and weights bary[l, k] that use it, in
 *   ascending 3 l + k; a lane sums its vertex's entries in that order.  g_rows is read at g_rows[b * g_rows_stride]
 *   (stride 0: one value for every sample).  No memset, no scatter, no atomics.
 * No allocation and no host read: both run under graph capture on `stream`.  B <= 65535 for the backward. */
int sr_landmark_loss_fwd(float* rows, float* p, float* g, const float* v, const int32_t* idx, const float* bary,
                         const float* target, const float* conf, int64_t B, int64_t L, int64_t nv, int64_t H, int64_t W,
                         float beta, float weight, sr_stream_t stream);
int sr_landmark_loss_bwd(float* gv, const float* g, const float* g_rows, int64_t g_rows_stride, const int32_t* csr_off,
                         const int32_t* csr_l, const float* csr_w, int64_t B, int64_t L, int64_t nv, int64_t H, int64_t W,
                         int accumulate, sr_stream_t stream);

/* Pose-aware landmarks: contour lines that slide along the silhouette and a visibility gate (definition:
 * stylerenderer_amd/op/landmark.py, landmark_dynamic_composite), csrc/landmark.hip.  Contour line c (C of them) replaces
 * landmark line_lmk[c] by one of its candidate vertices cand[cand_off[c] .. cand_off[c + 1]) (at least one; candidate 0
 * is the static vertex): with a = (v[b, i_up] - v[b, i_down]).xy and u = (a.y, -a.x) / |a| ((1, 0) when |a| < 1e-6),
 *   sel[b, c] = cand[first arg max_j side[c] * dot(v[b, cand_j].xy, u)]        (higher score, then lower position)
 * and P_l = v[b, sel[b, c]] for that landmark; lmk_line int32 [L] holds every landmark's line or -1.  Every other
 * landmark's confidence is multiplied by gate[b, l] = smoothstep(clamp((m - vis_lo) / (vis_hi - vis_lo), 0, 1)),
 * m = N.z / max(|N|, 1e-12) of N = sum_k bary[l, k] normals[b, idx[l, k], :] (vis_hi == vis_lo: 1 where m > vis_lo, else
 * 0); the gate is 1 for contour landmarks and everywhere when use_vis == 0 (normals may then be NULL).  rows, p, g as in
 * sr_landmark_loss_fwd with conf * gate in place of conf.
 * sr_landmark_dyn_fwd: one launch, one workgroup of 256 per sample (a wave per line, lanes over its candidates, wave
 *   arg-max by cross-lane shuffles; then the static forward's fixed-order sums); writes rows [B], p, g [B, L, 2],
 *   sel int32 [B, C], gate [B, L].  C <= 8192.  Every index (idx, cand, i_up, i_down < nv; lmk_line < C) is the caller's
 *   to validate (op/landmark.py does when it builds the lists).
 * sr_landmark_dyn_bwd: sr_landmark_loss_bwd with a second list: csr_* is built from the embedding with the contour
 *   landmarks' weights dropped; line_off int32 [nv + 1], line_c / line_l int32 [entries] list for every vertex the
 *   (line, landmark) pairs in which it is a candidate (first occurrence per line, ascending line); an entry adds
 *   g[b, l] iff sel[b, c] is this vertex.  A lane adds its static entries first, then its line entries, in list order.
 * No atomics, no memset, no allocation, no host read: both run under graph capture on `stream`; reruns are
 * bit-identical.  B <= 65535 for the backward. */
int sr_landmark_dyn_fwd(float* rows, float* p, float* g, int32_t* sel, float* gate, const float* v, const float* normals,
                        const int32_t* idx, const float* bary, const float* target, const float* conf,
                        const int32_t* lmk_line, const int32_t* side, const int32_t* cand_off, const int32_t* cand,
                        int64_t B, int64_t L, int64_t C, int64_t nv, int64_t i_up, int64_t i_down, int use_vis,
                        float vis_lo, float vis_hi, int64_t H, int64_t W, float beta, float weight, sr_stream_t stream);
int sr_landmark_dyn_bwd(float* gv, const float* g, const float* g_rows, int64_t g_rows_stride, const int32_t* sel,
                        const int32_t* csr_off, const int32_t* csr_l, const float* csr_w, const int32_t* line_off,
                        const int32_t* line_c, const int32_t* line_l, int64_t B, int64_t L, int64_t C, int64_t nv,
                        int64_t H, int64_t W, int accumulate, sr_stream_t stream);

/* Region-weighted image loss of face reconstruction (definition: stylerenderer_amd/op/region.py), csrc/region.hip.
 * sr_region_fill: out uint8 [B, 1, H, W] = 1 where pixel (x, y) lies in one of the sample's T closed integer triangles,
 *   else 0.  points int32 [B, P, 2] (x, y; |coordinate| <= 2^20, the caller's to check), tris int32 [T, 3]
 *   (tri_bstride 0: shared) or [B, T, 3] (tri_bstride 3 T) of indices into the sample's points; a triangle with an index
 *   outside [0, P) covers nothing.  In the triangle: inside its bounding box and the three edge functions
 *   cross(b - a, p - a), cross(c - b, p - b), cross(a - c, p - c) (int64) all >= 0 or all <= 0: either winding, a
 *   degenerate triangle is its segment or point.  T = 0 gives zeros.  B <= 65535, H, W <= 2^20.
 * sr_region_grow: out uint8 [N, H, W] (not in place) = in dilated (r > 0: 1 iff a pixel of the picture within Chebyshev
 *   distance r is set) or eroded (r < 0: 1 iff every pixel of the picture within |r| is set; the border does not
 *   erode) by a square window; 1 <= |r| <= 32.
 * sr_region_blend_fwd: m_eff [B, 1, H, W] = mask, times (n.x^2 + n.y^2 + n.z^2 > thresh ? 1 : 0) when normal_map != NULL
 *   (logical [B, 3, H, W], element (b, c, y, x) at normal_map[b nsb + c nsc + y nsh + x nsw]); y [B, C, H, W] = target +
 *   m_eff * (img - target), each operation rounded on its own.  One launch; float4 path when H W % 4 == 0 and y, m_eff,
 *   img, target, mask are 16-byte aligned, one pixel per lane otherwise.
 * sr_region_blend_bwd: g_img [B, C, H, W] = m_eff * g_y.  One launch, same two paths.
 * No atomics, no memset, no allocation, no host read: all four run under graph capture on `stream`. */
int sr_region_fill(uint8_t* out, const int32_t* points, const int32_t* tris, int64_t tri_bstride, int64_t B, int64_t P,
                   int64_t T, int64_t H, int64_t W, sr_stream_t stream);
int sr_region_grow(uint8_t* out, const uint8_t* in, int64_t N, int64_t H, int64_t W, int r, sr_stream_t stream);
int sr_region_blend_fwd(float* y, float* m_eff, const float* img, const float* target, const float* mask,
                        const float* normal_map, int64_t nsb, int64_t nsc, int64_t nsh, int64_t nsw, float thresh,
                        int64_t B, int64_t C, int64_t H, int64_t W, sr_stream_t stream);
int sr_region_blend_bwd(float* g_img, const float* g_y, const float* m_eff, int64_t B, int64_t C, int64_t H, int64_t W,
                        sr_stream_t stream);

/* UV texture baking of face reconstruction (definition: stylerenderer_amd/op/texture.py), csrc/texture.hip.  A texel map
 * face int32 [Th, Tw] (-1: empty), coeff [Th, Tw, 3] names the mesh face under every texel and its barycentric weights
 * (row 0 is the top of the texture); it is shared by the batch.
 * sr_texture_bake: tex [B, C, Th, Tw] and weight [B, 1, Th, Tw] from the posed mesh v, n [B, nv, 3], tri int64 [nf, 3],
 *   the picture image [B, C, Hs, Ws] and the z-buffer zbuf [B, Hz, Wz] of the same posed mesh (the rasterizer's: greater z
 *   is nearer, -FLT_MAX is empty).  For a texel with f = face >= 0, every step one float32 operation in this order:
 *     P = (c0 v[i0] + c1 v[i1]) + c2 v[i2], i_k = tri[f, k]; N likewise from n;  m = N.z / max(|N|, 1e-12)
 *     g = smoothstep(clamp((m - lo) / (hi - lo), 0, 1))  (hi == lo: 1 where m > lo, else 0)
 *     q = ((1 + P.x) Wz / 2 - 1/2, (1 - P.y) Hz / 2 - 1/2); ix = floor(q.x + 1/2), iy = floor(q.y + 1/2)
 *     vis = 0 <= ix < Wz and 0 <= iy < Hz and P.z >= zbuf[b, iy, ix] - z_bias
 *     s = the same projection onto (Hs, Ws); inside = -1/2 <= s.x <= Ws - 1/2 and -1/2 <= s.y <= Hs - 1/2
 *     colour = the bilinear sample of image[b, c] at s, indices clamped to the picture
 *     weight = g if vis and inside, else 0;  tex = colour where weight > 0, else 0
 *   An empty texel, and one whose face or vertices lie outside [0, nf) / [0, nv), writes zeros.  One launch; a lane owns
 *   four consecutive texels of a row, reads their map entries once and walks the B samples; every plane is written with
 *   16-byte stores when Tw % 4 == 0 and tex, weight are 16-byte aligned, with scalar stores otherwise.
 * sr_texture_pad: one pass of texture padding, out of place (tex_out != tex_in, filled_out != filled_in).  filled uint8
 *   [B, 1, Th, Tw].  A filled texel is copied; an unfilled one with at least one filled 8-neighbour becomes filled with the
 *   sum of those neighbours' colours (added in the order rows top to bottom, left to right) divided by their count; any
 *   other texel is copied and stays unfilled.  One launch, one lane per texel.
 * sr_texture_merge: V bakes tex_in [V, C, Th, Tw], weight_in [V, 1, Th, Tw] of one subject in one layout -> tex
 *   [1, C, Th, Tw], weight [1, 1, Th, Tw], best uint8 [Th, Tw], out of place.  Per texel, one float32 operation per step:
 *     wmax = max_v w_v, best = the first v that attains it; wmax <= 0: colour 0, weight 0, best 255
 *     r_v = w_v / wmax, then `sharpness` times r_v = r_v r_v; after the division and after every squaring a value below
 *       2^-63 becomes 0 (no operand or result is subnormal)
 *     den = ((r_0 + r_1) + ...), num_c = ((r_0 t_0c + r_1 t_1c) + ...) from 0, product and sum rounded separately; a view
 *       with r_v = 0 is skipped, not multiplied (what stands in an unweighted texel cannot leak)
 *     tex_c = num_c / den, weight = wmax
 *   1 <= V <= 64, 0 <= sharpness <= 4.  One launch; a lane owns four consecutive texels of a row; 16-byte loads and stores
 *   when Tw % 4 == 0 and all four float planes are 16-byte aligned (best 4-byte aligned), scalar ones otherwise.
 * NULL pointers and non-positive sizes are SR_EINVAL before any launch; B, Th or Tw of 0 returns 0.  No atomics, no
 * scratch, no memset, no allocation, no host read: all three run under graph capture on `stream`; reruns are
 * bit-identical. */
int sr_texture_bake(float* tex, float* weight, const float* v, const float* n, const int64_t* tri, const int32_t* face,
                    const float* coeff, const float* image, const float* zbuf, int64_t B, int64_t C, int64_t nv,
                    int64_t nf, int64_t Th, int64_t Tw, int64_t Hs, int64_t Ws, int64_t Hz, int64_t Wz, float facing_lo,
                    float facing_hi, float z_bias, sr_stream_t stream);
int sr_texture_pad(float* tex_out, uint8_t* filled_out, const float* tex_in, const uint8_t* filled_in, int64_t B,
                   int64_t C, int64_t Th, int64_t Tw, sr_stream_t stream);
int sr_texture_merge(float* tex, float* weight, uint8_t* best, const float* tex_in, const float* weight_in, int64_t V,
                     int64_t C, int64_t Th, int64_t Tw, int sharpness, sr_stream_t stream);

/* The texture look-up node (definition: stylerenderer_amd/op/texture.py, sample_composite), csrc/texture_sample.hip.
 * tex [Bt, C, Th, Tw] with Bt == B or Bt == 1 (one texture shared by all B views), uv [B, H, W, 2], cover uint8 [B, H, W]
 * (op.texture.uv_map), out and gout [B, C, H, W].  Row 0 of the texture is its top: the centre of texel (ty, tx) is at
 * u = (tx + 1/2) / Tw, v = 1 - (ty + 1/2) / Th.  For a pixel with cover != 0 and finite (u, v), every step one float32
 * operation in this order, no contraction:
 *     sx = u Tw - 1/2;  sy = (1 - v) Th - 1/2
 *     inx = -1 <= sx <= Tw, sxc = clamp(sx, -1, Tw);  likewise iny, syc
 *     x0 = floor(sxc), fx = sxc - x0;  xa = clamp(x0, 0, Tw - 1), xb = clamp(x0 + 1, 0, Tw - 1);  likewise y0, fy, ya, yb
 *     top = (1 - fx) T[ya, xa] + fx T[ya, xb];  bot = (1 - fx) T[yb, xa] + fx T[yb, xb]
 *     out_c = top (1 - fy) + bot fy
 *   Any other pixel gets out_c = background and contributes to no gradient.
 * sr_texture_sample_fwd: out.  One launch; a lane owns four consecutive pixels of a row for all channels; 16-byte stores
 *   when W % 4 == 0 and out is 16-byte aligned, scalar stores otherwise.
 * sr_texture_sample_bwd_uv: guv [B, H, W, 2] from gout:
 *     gx = sum over c from 0, in channel order, of g_c ((T[ya, xb] - T[ya, xa]) (1 - fy) + (T[yb, xb] - T[yb, xa]) fy)
 *     gy = sum over c likewise of g_c (bot - top)
 *     grad_u = inx ? gx Tw : 0;  grad_v = iny ? -(gy Th) : 0
 *   One launch, the forward's staging; 16-byte loads and stores when W % 4 == 0 and guv, gout are 16-byte aligned.
 * sr_texture_sample_bwd_tex: gtex [Bt, C, Th, Tw] from gout and the tap list (off int32 [Bt Th Tw + 2], entries int32
 *   [4 B H W]: a CSR over the keys bt Th Tw + ty Tw + tx whose entries ((b H + y) W + x) 4 + k ascend within a key; the
 *   bucket after the last key holds the entries of the pixels without taps; op.texture.tap_plan builds it):
 *     gtex[bt, c, ty, tx] = the sum from 0, in list order, of w_k g_c[b, y, x]
 *     k = 0..3: (ya, xa), (ya, xb), (yb, xa), (yb, xb);  w = (1 - fx)(1 - fy), fx (1 - fy), (1 - fx) fy, fx fy
 *   fx, fy are recomputed from uv; two taps of one pixel that clamp onto one texel are two entries.  With Bt == 1 the list
 *   of a texel runs over all B views.  One launch, a lane per texel for all channels; every texel is written and one
 *   without taps gets exactly 0.  Offsets and entries outside the list or the picture are skipped, never followed.
 * Th, Tw >= 1; B, H or W of 0 writes nothing (bwd_tex: zeros) and returns 0; 4 B H W and Bt Th Tw must be below 2^31.  No
 * atomics, no scratch, no memset, no allocation, no host read: all three run under graph capture on `stream`; reruns are
 * bit-identical. */
int sr_texture_sample_fwd(float* out, const float* tex, const float* uv, const uint8_t* cover, int64_t B, int64_t Bt,
                          int64_t C, int64_t H, int64_t W, int64_t Th, int64_t Tw, float background, sr_stream_t stream);
int sr_texture_sample_bwd_uv(float* guv, const float* gout, const float* tex, const float* uv, const uint8_t* cover,
                             int64_t B, int64_t Bt, int64_t C, int64_t H, int64_t W, int64_t Th, int64_t Tw,
                             sr_stream_t stream);
int sr_texture_sample_bwd_tex(float* gtex, const float* gout, const float* uv, const uint8_t* cover, const int32_t* off,
                              const int32_t* entries, int64_t B, int64_t Bt, int64_t C, int64_t H, int64_t W, int64_t Th,
                              int64_t Tw, sr_stream_t stream);

/* The tap list of sr_texture_sample_bwd_tex built on the device (definition: stylerenderer_amd/op/texture.py, tap_plan),
 * csrc/tap_plan.hip: for a uv map that changes in every step of a captured fit.
 * sr_tap_plan_build: off int32 [Bt Th Tw + 2] and entries int32 [4 B H W] of uv [B, H, W, 2], cover uint8 [B, H, W], the
 *   integers of op.texture.tap_plan.  A pixel's four keys come from sr_texture_sample_fwd's arithmetic (one copy of the
 *   code); a pixel with cover == 0 or a non-finite coordinate files its four taps under the key Bt Th Tw.  A least-
 *   significant-digit radix sort of (key, entry) pairs with d-bit digits in sr_tap_plan_passes passes: 1 + 3 passes + 1
 *   launches, the same sequence for the same shapes whatever the data.  Ties keep their input order, so the entries of a
 *   key ascend; a pair's position is a function of the input alone (no float atomics, no order of retirement), so reruns
 *   are bit-identical.  No workgroup waits for another; every element of off and entries and every element of scratch
 *   that is read is written by each build, nothing needs to start at zero.  No allocation, no memset, no host read: it
 *   runs under graph capture on `stream`.  scratch: sr_tap_plan_scratch_ints int32 elements, 16-byte aligned.  B, H or W
 *   of 0 writes off = 0 only.  Bt == B or 1; 4 B H W and Bt Th Tw must be below 2^31.
 * sr_tap_plan_passes: ceil(bits(Bt Th Tw) / d), -1 for sizes out of range.  sr_tap_plan_digit_bits: d.
 * sr_tap_plan_scratch_ints: a function of the picture's shape alone; -1 for sizes out of range. */
int sr_tap_plan_digit_bits(void);
int sr_tap_plan_passes(int64_t Bt, int64_t Th, int64_t Tw);
int64_t sr_tap_plan_scratch_ints(int64_t B, int64_t H, int64_t W);
int sr_tap_plan_build(int32_t* off, int32_t* entries, int32_t* scratch, int64_t scratch_ints, const float* uv,
                      const uint8_t* cover, int64_t B, int64_t Bt, int64_t H, int64_t W, int64_t Th, int64_t Tw,
                      sr_stream_t stream);

/* The adjoint of the corner explode c[b, 3 f + k] = v[b, tri[f, k]] of op.texture.uv_map (definition:
 * stylerenderer_amd/op/texture.py, explode), csrc/explode.hip.
 * sr_explode_bwd: gv [B, nv, 3] from gc [B, 3 nf, 3] and the topology's incidence list (op.rasterize.incidence: adj_off
 *   int32 [nv + 2], adj int32 [3 nf], the entries k nf + f of a vertex ascending): per coordinate the sum from 0, in list
 *   order, of gc[b, 3 f + k].  One launch, a lane per vertex of a sample; every element of gv is written, a vertex without
 *   a corner gets exactly 0.  Offsets and entries outside the list are skipped, never followed.  No atomics, no scratch, no
 *   allocation, no host read: it runs under graph capture on `stream`; reruns are bit-identical. */
int sr_explode_bwd(float* gv, const float* gc, const int32_t* adj_off, const int32_t* adj, int64_t B, int64_t nv,
                   int64_t nf, sr_stream_t stream);

/* The mip-mapped texture look-up (definition: stylerenderer_amd/op/texture.py, mip_build_composite, mip_lod_composite,
 * mip_sample_composite), csrc/texture_mip.hip.  A (Th, Tw) texture has up to Lmax levels: level 0 is the texture, level
 * l + 1 has half of each side and exists while both sides of level l are even; 1 <= L <= Lmax of them are used.  The
 * pyramid pyr [Bt, C, P] holds level l (sides Th >> l, Tw >> l) at offset_l = sum_{j < l} h_j w_j of every plane, P the sum
 * over all L levels.  Every step is one float32 operation in the stated order, no contraction.
 * sr_mip_build_fwd: pyr from tex [N, Th, Tw], N = Bt C planes: level 0 a copy,
 *     p_{l+1}[y, x] = ((p_l[2y, 2x] + p_l[2y, 2x+1]) + (p_l[2y+1, 2x] + p_l[2y+1, 2x+1])) 0.25
 *   A workgroup reduces a 32 x 32 tile of a source level by up to five levels through LDS; one launch per five levels,
 *   each reading the last level the one before wrote.  Every element of pyr is written.
 * sr_mip_build_bwd: gtex [Bt, C, Th, Tw] from gpyr [Bt, C, P], per level-0 texel (y, x):
 *     t = gpyr_{L-1}[y >> (L-1), x >> (L-1)];  t = gpyr_l[y >> l, x >> l] + 0.25 t for l = L-2 .. 0;  gtex[y, x] = t
 *   One launch, a lane per texel for all channels: a gather, no scatter.
 * sr_mip_lod: lod [B, H, W] of uv [B, H, W, 2], cover uint8 [B, H, W].  A pixel is live with cover != 0 and finite (u, v);
 *   one that is not gets 0.  Along x over the neighbours n = (y, x + 1), (y, x - 1) inside the picture and live:
 *     du = (u_n - u) Tw;  dv = (v_n - v) Th;  d = du du + dv dv;  qx = min d (0 with no such neighbour);  qy along y
 *     rho = sqrt(max(qx, qy)), correctly rounded;  l = the largest integer in [0, L-1] with 2^l <= rho
 *     lambda = rho < 1 ? 0 : l == L-1 ? L-1 : l + (rho 2^-l - 1);  lod = clamp(lambda + bias, 0, L-1)
 *   One launch, a lane per four consecutive pixels of a row; 16-byte stores when W % 4 == 0 and lod is 16-byte aligned.
 * sr_mip_sample_fwd: out [B, C, H, W].  Bt == B or 1.  For a live pixel lod is clamped to [0, L-1] (NaN: 0),
 *     l0 = floor(lod), l1 = min(l0 + 1, L-1), f = lod - l0;  c_l = sr_texture_sample_fwd's blend on level l with
 *     (Th >> l, Tw >> l);  out = f == 0 ? c_l0 : (1 - f) c_l0 + f c_l1   (f == 0: level l1 is not read)
 *   Any other pixel gets `background`.  One launch, sr_texture_sample_fwd's staging.
 * sr_mip_sample_bwd_uv: guv [B, H, W, 2] from gout: guv_l is sr_texture_sample_bwd_uv's formula on level l (its channel
 *   sums in channel order, its inx / iny gating with the level's sides);  guv = f == 0 ? guv_l0 : (1 - f) guv_l0 + f guv_l1.
 * sr_mip_sample_bwd_pyr: gpyr [Bt, C, P] from gout and the tap list (off int32 [Bt P + 2], entries int32 [8 B H W]: a CSR
 *   over the keys bt P + offset_l + ty (Tw >> l) + tx whose entries ((b H + y) W + x) 8 + k ascend within a key; k = 0..3
 *   are the taps of l0 in sr_texture_sample_bwd_tex's order with the weights (1 - f) w_k, k = 4..7 those of l1 with
 *   f w_{k-4}; the bucket after the last key holds the entries without a tap; op.texture.mip_tap_plan builds it):
 *     gpyr[key] = the sum from 0, in list order, of weight g_c[b, y, x]
 *   One launch, a lane per pyramid element for all channels; every element is written and one without taps gets exactly
 *   0.  Offsets and entries outside the list or the picture are skipped, never followed.
 * Th, Tw >= 1 and at most 2^20, Th Tw < 2^31; N, B, H or W of 0 writes nothing (bwd_pyr: zeros) and returns 0; 8 B H W and
 * Bt P must be below 2^31.  No atomics, no scratch, no memset, no allocation, no host read: all run under graph capture on
 * `stream`; reruns are bit-identical. */
int sr_mip_build_fwd(float* pyr, const float* tex, int64_t N, int64_t Th, int64_t Tw, int64_t L, sr_stream_t stream);
int sr_mip_build_bwd(float* gtex, const float* gpyr, int64_t Bt, int64_t C, int64_t Th, int64_t Tw, int64_t L,
                     sr_stream_t stream);
int sr_mip_lod(float* lod, const float* uv, const uint8_t* cover, int64_t B, int64_t H, int64_t W, int64_t Th, int64_t Tw,
               int64_t L, float bias, sr_stream_t stream);
int sr_mip_sample_fwd(float* out, const float* pyr, const float* uv, const uint8_t* cover, const float* lod, int64_t B,
                      int64_t Bt, int64_t C, int64_t H, int64_t W, int64_t Th, int64_t Tw, int64_t L, float background,
                      sr_stream_t stream);
int sr_mip_sample_bwd_uv(float* guv, const float* gout, const float* pyr, const float* uv, const uint8_t* cover,
                         const float* lod, int64_t B, int64_t Bt, int64_t C, int64_t H, int64_t W, int64_t Th, int64_t Tw,
                         int64_t L, sr_stream_t stream);
int sr_mip_sample_bwd_pyr(float* gpyr, const float* gout, const float* uv, const uint8_t* cover, const float* lod,
                          const int32_t* off, const int32_t* entries, int64_t B, int64_t Bt, int64_t C, int64_t H,
                          int64_t W, int64_t Th, int64_t Tw, int64_t L, sr_stream_t stream);

/* The shared identity of a multi-view fit (definition: stylerenderer_amd/op/share.py), csrc/share.hip.
 * sr_share_rows: g [B, d] in place: s[j] = ((g[0, j] + g[1, j]) + g[2, j]) + ... in row order, then g[b, j] = s[j] for
 *   every b, for the columns j < k (1 <= k <= d); the other columns are not touched.  One launch, one lane per column.  No
 *   atomics, no LDS, no scratch, no allocation, no host read: it runs under graph capture on `stream`; reruns on the same
 *   input are bit-identical.  B <= 65535. */
int sr_share_rows(float* g, int64_t B, int64_t d, int64_t k, sr_stream_t stream);

/* The perspective camera of face reconstruction (definition: stylerenderer_amd/op/camera.py), csrc/camera.hip.  v, v', n,
 * n_view, gv, gv' are [B, nv, 3], kappa and gkappa [B]; kappa[b] = 1 / the camera's distance from the plane z = 0 in
 * half-picture-widths.  Per vertex (x, y, z) of row b with k = kappa[b], every step one float32 operation in this order:
 *     q0 = 1 - k z;  clamped = q0 < 1/16;  q = clamped ? 1/16 : q0;  v' = (x / q, y / q, z / q)
 *     a = (k x', k y');  len = sqrt(1 + (a.x a.x + a.y a.y));  d = (-a.x / len, -a.y / len, 1 / len)
 *     c = (N.x d.x + N.y d.y) + N.z d.z;  e = (c + N.z) / (1 + d.z)
 *     n_view = (N.x - e d.x, N.y - e d.y, (N.z - e (d.z + 1)) + 2 c);  k == 0: n_view = N
 * sr_camera_fwd: v' and, when n_view and n are given (both or neither), n_view.  One launch for the batch; a lane owns four
 *   vertices (three 16-byte loads and stores) where the row's offset allows and all tensors are 16-byte aligned, the at most
 *   six other vertices of a row and unaligned tensors go one vertex per lane.
 * sr_camera_bwd: gv and, when gkappa is given, gkappa from gv' (n_view is a constant of the backward pass):
 *     u = (x' gx' + y' gy') + z' gz';  t = u / q;  gv = gv' / q;  gv.z = gv.z + k t unless clamped
 *     gkappa[b] = sum_i z_i t_i, a clamped vertex adding 0
 *   vp is v' of the forward call or NULL (recomputed, the same bits).  One launch; with gkappa one workgroup of 1024 lanes per
 *   row: a lane adds the terms of its items (item j, j + 1024, ... of the row; a group's four vertices in order), then a
 *   fixed-order tree of depth 10 in LDS.
 * B <= 65535.  No atomics, no scratch, no memset, no allocation, no host read: both run under graph capture on `stream`;
 * reruns are bit-identical. */
int sr_camera_fwd(float* vp, float* n_view, const float* v, const float* n, const float* kappa, int64_t B, int64_t nv,
                  sr_stream_t stream);
int sr_camera_bwd(float* gv, float* gkappa, const float* v, const float* vp, const float* gvp, const float* kappa,
                  int64_t B, int64_t nv, sr_stream_t stream);

/* Albedo and lighting: Lambertian shading under second-order spherical harmonics (definition:
 * stylerenderer_amd/op/light.py), csrc/light.hip.  a, out, g, ga are [B, C, H, W], normals and gn [B, 3, H, W], on uint8
 * [B, H, W] (non-zero: the pixel counts), gamma [B, Cl, 9] with Cl = 1 (every channel reads light 0) or Cl = C (channel c
 * reads light c).  Per pixel, every step one float32 operation in this order:
 *     r = sqrt((nx nx + ny ny) + nz nz);  len = r > 1e-12 ? r : 1e-12;  (x, y, z) = n / len
 *     Y = [1, x, y, z, x y, x z, y z, x x - y y, 3 (z z) - 1];   s_l = (((g0 + g1 Y1) + g2 Y2) + ...) + g8 Y8
 * A pixel is live when `on` holds and its normal is finite.
 * sr_light_shade_fwd: divide == 0: out_c = (a_c - black) (s > 0 ? s : 0) + black on live pixels, `background` elsewhere;
 *   divide != 0 (floor > 0): out_c = (a_c - black) / (s > floor ? s : floor) + black on live pixels, a_c elsewhere.  A lane
 *   owns four consecutive pixels of a row; 16-byte accesses where W % 4 == 0 and out, a, normals are 16-byte aligned (on:
 *   4-byte), scalar ones otherwise.
 * sr_light_shade_bwd (Cl <= 4): ga_c = g_c (s > 0 ? s : 0) on live pixels, 0 elsewhere; with e_l the sum from 0 in channel
 *   order of g_c (a_c - black) over the channels that read light l, 0 unless s_l > 0 and the pixel is live:
 *     gn (when given): gY_k = sum_l e_l gamma[l, k];  gx = ((gY1 + gY4 y) + gY5 z) + (2 gY7) x;
 *       gy = ((gY2 + gY4 x) + gY6 z) - (2 gY7) y;  gz = ((gY3 + gY5 x) + gY6 y) + (6 gY8) z;  d = (x gx + y gy) + z gz;
 *       gn = ((gx - x d) / len, (gy - y d) / len, (gz - z d) / len), 0 where r < 1e-12 or the pixel is not live
 *     partial (when given) [B, P, Cl, 9], P = max(1, ceil(H ceil(W / 4) / 1024)): row p holds the sums of e_l Y_k over the
 *       pixels of workgroup p (items 1024 p .. 1024 p + 1023 of four pixels each; a lane adds its up to 16 terms in index
 *       order, then a fixed tree of depth 8).  Every row is written.
 * sr_light_reduce: out [B, n] = the sum of partial [B, P, n] over P in ascending order; f64 != 0: double, else float.
 * sr_light_moments (C <= 4): partial double [B, P, 45 + 9 C], reduced as above: the upper triangle (i <= j, row-major) of
 *   sum w Y Y^T and then sum w Y (a_c - black) for every c, over the pixels with weight [B, 1, H, W] > 0 and a finite
 *   normal.  Y and a_c - black are float32; the products (w Y_i) Y_j, (w Y_k) (a_c - black) and the sums are double.
 * sr_light_texel_attr: out [B, A, Th, Tw] (1 <= A <= 4) from attr [B, nv, A] and the texel map (face int32 [Th, Tw], coeff
 *   [Th, Tw, 3]) of a mesh with the faces tri int64 [nf, 3]: (c0 attr[i0] + c1 attr[i1]) + c2 attr[i2], i_k = tri[face, k];
 *   0 where face < 0; a face or vertex index outside the mesh counts as empty and is not read.
 * B <= 65535.  No atomics, no memset, no allocation, no host read: all run under graph capture on `stream`; reruns are
 * bit-identical. */
int sr_light_shade_fwd(float* out, const float* a, const float* normals, const uint8_t* on, const float* gamma, int64_t B,
                       int64_t C, int64_t Cl, int64_t H, int64_t W, float black, float floor, float background, int divide,
                       sr_stream_t stream);
int sr_light_shade_bwd(float* ga, float* gn, float* partial, const float* g, const float* a, const float* normals,
                       const uint8_t* on, const float* gamma, int64_t B, int64_t C, int64_t Cl, int64_t H, int64_t W,
                       float black, sr_stream_t stream);
int sr_light_reduce(void* out, const void* partial, int64_t B, int64_t P, int64_t n, int f64, sr_stream_t stream);
int sr_light_moments(double* partial, const float* a, const float* normals, const float* weight, int64_t B, int64_t C,
                     int64_t H, int64_t W, float black, sr_stream_t stream);
int sr_light_texel_attr(float* out, const float* attr, const int64_t* tri, const int32_t* face, const float* coeff,
                        int64_t B, int64_t A, int64_t nv, int64_t nf, int64_t Th, int64_t Tw, sr_stream_t stream);

/* Analytic antialiasing at occlusion boundaries (definition: stylerenderer_amd/op/edge.py), csrc/edge.hip.  image, out, g
 * and gimage are [B, C, H, W], v [B, nv, 3], tri int64 [nf, 3], opp int32 [nf, 3] (op.edge.adjacency: the vertex opposite
 * edge k in the other face, -1 boundary, -2 never a silhouette), face int32 [B, H, W] (-1 empty) and zbuf [B, H, W] (greater
 * is nearer).  A pair is a pixel p and its right or lower neighbour q, active iff face[p] != face[q]; the foreground a is q
 * when face[p] < 0, p when face[q] < 0, else q iff z[q] > z[p]; o is the other pixel, F = face[a].  Per corner of F
 *     X = (1 + x) (W / 2) - 0.5;  Y = (1 - y) (H / 2) - 0.5
 * and for the edges k = 0, 1, 2 (corners i = k, j = (k + 1) mod 3), u the coordinate along the pair's axis, s the other one
 * minus a's, every step one float32 operation in this order:
 *     crossing iff (s_i < 0) != (s_j < 0);  den = s_i - s_j;  t = s_i / den;  du = u_j - u_i;  c = u_i + du t
 *     d = c - a_u (a == p) or a_u - c (a == q);  taken iff 0 <= d <= 1
 *     silhouette iff opp == -1, or opp >= 0 and (P_j - P_i) x (P_own - P_i), (P_j - P_i) x (P_opp - P_i) do not have
 *     strictly opposite signs
 * The first k that crosses and is a silhouette is the pair's edge; w = d - 0.5 and o receives when d >= 0.5, else
 * w = 0.5 - d and a receives: the receiver r gets w (image[other] - image[r]).
 * sr_edge_aa_fwd: out[p] = image[p] plus what p receives from its pairs, added in the order left, right, upper, lower.  A
 *   lane per pixel, channels inside; a pixel whose cross shows one face leaves after five loads.
 * sr_edge_aa_bwd_image: gimage[p] = g[p], then per pair in the same order - w g[p] where p receives, + w g[n] where the
 *   neighbour n does.
 * sr_edge_aa_bwd_corner: gc [B, 3 nf, 3], the gradient of the exploded corners (z = 0), all of it written.  Per pair with
 *   receiver r:  gd = the sum from 0 in channel order of g[r] (image[a] - image[o]);  gsd = gd (a == p) or -gd;
 *     gu_i = gsd (1 - t);  gu_j = gsd t;  q = (gsd du) / (den den);  gs_i = -(q s_j);  gs_j = q s_i
 *     gx = gX (W / 2);  gy = gY (-(H / 2))        (X is u in a horizontal pair, s in a vertical one)
 *   A lane per (sample, face) walks the pixels of the face's bounding box (floor of the least and ceil of the greatest
 *   corner coordinate, grown by one pixel, clipped) in row-major order, right pair before lower pair, and adds the terms of
 *   the pairs whose F is its face.  A box of more than sr_edge_big_pixels() pixels is summed by the face's wave: lane l adds
 *   the pixels l, l + 64, ... in that order, then lane l adds lane l + 32, 16, 8, 4, 2, 1.  A face with a non-finite corner
 *   gets 0.
 * Face and vertex numbers outside the mesh switch a pair off and are not followed.  H, W <= 16384.  No atomics, no LDS, no
 * scratch, no memset, no allocation, no host read: all run under graph capture on `stream`; reruns are bit-identical. */
int sr_edge_big_pixels(void);
int sr_edge_aa_fwd(float* out, const float* image, const float* v, const int64_t* tri, const int32_t* opp,
                   const int32_t* face, const float* zbuf, int64_t B, int64_t C, int64_t H, int64_t W, int64_t nv,
                   int64_t nf, sr_stream_t stream);
int sr_edge_aa_bwd_image(float* gimage, const float* g, const float* v, const int64_t* tri, const int32_t* opp,
                         const int32_t* face, const float* zbuf, int64_t B, int64_t C, int64_t H, int64_t W, int64_t nv,
                         int64_t nf, sr_stream_t stream);
int sr_edge_aa_bwd_corner(float* gc, const float* g, const float* image, const float* v, const int64_t* tri,
                          const int32_t* opp, const int32_t* face, const float* zbuf, int64_t B, int64_t C, int64_t H,
                          int64_t W, int64_t nv, int64_t nf, sr_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* STYLERENDERER_AMD_H_ */
