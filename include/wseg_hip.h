/* wseg_hip.h — C ABI of libwseg_hip.so (MI355X / gfx950).
 *
 * The reference (obeychoi0120/wseg) has no FFI: its hot path is PyTorch ATen calls made from
 * network/resnet38d.py, network/resnet38_contrast.py and the loop body of contrast_train.py.
 * Each entry point below replaces one group of those ATen call sites (file:line cited per
 * function, paths relative to the reference root).  The Python host (wseg_amd/) binds them
 * with ctypes; INTEGRATION.md shows the stub a reference maintainer would add.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer owned by the caller (torch allocates); the library never
 *     allocates, frees or synchronises, keeps no mutable global state, and is re-entrant
 *     (contrast_infer.py:69-73 calls forward from 8 threads);
 *   - `stream` is a hipStream_t passed as void*; all work is enqueued on it;
 *   - activations are NHWC ("pixel rows"): element (n,y,x,c) at ((n*H+y)*W+x)*ld + c;
 *   - dtype: 0 = f32 (exact-f32 MFMA, parity mode), 1 = bf16 (bf16 MFMA, f32 accumulate), 2 = f32 storage with split-bf16 products
 *     (conv / wgrad only: every f32 operand x = hi + lo with hi = bf16(x), lo = bf16(x - hi); the product is hi.hi + lo.hi + hi.lo on
 *     the bf16 MFMA with f32 accumulate — 16-17 operand bits at 3 bf16 MFMAs per product instead of the 8x slower f32 MFMA; activations
 *     are split in the kernel, weights arrive pre-split: wseg_pack_x3);
 *   - return 0 on success, negative on error; wseg_last_error() gives the thread-local message.
 */
#ifndef WSEG_HIP_H
#define WSEG_HIP_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define WSEG_F32 0
#define WSEG_BF16 1
#define WSEG_F32X3 2

int wseg_version(void);
/* sizeof(wseg_conv_desc) / sizeof(wseg_wgrad_desc) as this build sees them: a binding checks its mirror of the descriptors against
 * these before the first call (a stale, shorter mirror would hand the kernels uninitialised trailing fields). */
size_t wseg_sizeof_conv_desc(void);
size_t wseg_sizeof_wgrad_desc(void);
const char* wseg_last_error(void);

/* ---- convolution as implicit GEMM ------------------------------------------------------
 * Replaces nn.Conv2d forward / input-gradient for every 3x3 (stride 1|2, dilation 1|2|4) and
 * 1x1 (stride 1|2) conv of the backbone and heads: network/resnet38d.py:17,22,25,61,65,69,72,124;
 * network/resnet38_contrast.py:15-20,36-38,50-51,67.  The frozen BatchNorm(eval)+ReLU
 * (+Dropout2d scale) that follows a conv (resnet38d.py:29-30,40-41,76-77,84-91,187) is the
 * fused epilogue, the residual add (resnet38d.py:44,94) too.
 *
 *   mode 0 (forward):   out[n,oy,ox,:] = sum_{ky,kx} in[n, oy*stride+ky*dil-pad, ox*stride+kx*dil-pad, :] . w[:,ky,kx,:]
 *   mode 1 (data grad): out[n,y,x,:]   = sum_{ky,kx} in[n, (y+pad-ky*dil)/stride, (x+pad-kx*dil)/stride, :] . w[:,ky,kx,:]
 *                       (terms whose division is inexact or out of range are zero)
 *   weights: w[OC][KH*KW][IC], IC contiguous (for mode 1 the caller passes the transposed pack).
 *
 *   epilogue, v = acc:
 *     if r_pre   : v += r_pre
 *     epi 0      : out  = v (+ r_post)                                   raw sum
 *                  out2 = relu(v*scale[c]+shift[c]) * drop[n,c]          (when out2 != NULL)
 *     epi 1      : out  = v*scale[c]*drop[n,c]*(mask>0) + r_post          (BN-ReLU backward)
 *     epi 2      : out  = relu(v)                                         (f8_3/f8_4/fc_proj)
 *     epi 3      : out  = elu(v) = v > 0 ? v : expm1(v)                   (the AffinityNet head f8_3/f8_4/f8_5/f9,
 *                                                                          network/resnet38_aff.py:44-47; 64 / 128-row tiles)
 *   NULL scale/shift/drop/mask/r_post mean 1/0/1/all-pass/0.
 */
typedef struct wseg_conv_desc {
  const void* in;  const void* w;  void* out;  void* out2;
  const void* r_pre;  const void* r_post;  const void* mask;
  const float* scale;  const float* shift;  const float* drop;
  int32_t N, IH, IW, IC, ld_in;
  int32_t OH, OW, OC, ld_out, ld_out2;
  int32_t ld_rpre, ld_rpost, ld_mask;
  int32_t KH, KW, stride, dil, pad;
  int32_t mode, epi, dtype;
  int32_t relu_out2;   /* 1: out2 gets the ReLU (default); 0: affine only */
  int32_t relu_lt;     /* epi 0: ReLU on `out` channels < relu_lt (fused head: f_proj | cam); 0 = none */
  int32_t bm_hint;     /* 0 = library chooses the tile (64 / 128 pixel rows x 128 channels, or the 256 x 256 phase-pipelined
                          bf16 kernel for large layers with OC % 256 == 0, or the 512 x 128 one for OC = 128 layers with many pixels);
                          64 / 128 / 224 / 256 = force; 259 = test hook (512 x 128 tile).  A forced 224 / 256 / 259 whose shape the kernel
                          does not take (see wseg_conv_plan) runs on the 64 / 128-row tiles: wseg_conv_plan tells which */
  /* optional SECOND row segment (the 128x128 view batched behind the 448x448 view in one launch): rows
   * [0, N*OH*OW) use (IH,IW,OH,OW); rows beyond use (IH2,IW2,OH2,OW2), same N, their input pixels follow the
   * first segment's N*IH*IW rows; drop then has 2N rows.  OH2 == 0: single segment. */
  int32_t IH2, IW2, OH2, OW2;
  /* optional SECOND INPUT (K-concatenation): out = conv(in; W[:, :KH*KW*IC]) + in2 . W[:, KH*KW*IC:] with w = [OC][KH*KW*IC + IC2] —
   * a residual block's last conv and its 1x1 skip conv (network/resnet38d.py:35-47, 83-97: branch1 + branch2) as ONE product: the
   * second source is one extra K segment read at the output pixel itself, so the skip output is neither written nor re-read.  With
   * the transposed packs and mode 1 the same form is the sum of the two data gradients into the block's input.  Same-size stride-1
   * convolution (pad = dil*(KH/2)), bf16, OC % 256 == 0, IC2 % 64 == 0 (0: IC2 = IC), epi 0..2 (the form exists on the 256-tile kernel only,
   * which has no ELU: epi 3 is refused), in2 on the OUTPUT pixel grid; NULL: none. */
  const void* in2;
  int32_t ld_in2, IC2;
  int32_t w_rows;      /* rows the weight pack really holds (>= OC; 0 = OC).  A pack zero-padded to a multiple of 256 rows lets a launch whose OC is
                          not one (the fused head: 149 of 192 columns, resnet38_contrast.py:34-38) run on the 256-tile kernel: it reads whole 256-row
                          weight tiles and masks the columns >= OC in its epilogue */
} wseg_conv_desc;
int wseg_conv_igemm(const wseg_conv_desc* d, void* stream);

/* ---- weight gradient -------------------------------------------------------------------
 * Replaces the weight-gradient half of Conv2d backward (autograd of the same call sites).
 *   dw[oc][ky*KW+kx][ic] (+)= sum_{n,oy,ox} dy[n,oy,ox,oc] * x[n, oy*stride+ky*dil-pad, ox*stride+kx*dil-pad, ic]
 * dw is f32, accumulated with atomics (split over pixel ranges); the caller zeroes it once per step
 * so that both views accumulate (contrast_train.py:398 sums both forward graphs).
 */
typedef struct wseg_wgrad_desc {
  const void* x;  const void* dy;  float* dw;
  int32_t N, IH, IW, IC, ld_x;
  int32_t OH, OW, OC, ld_dy;
  int32_t KH, KW, stride, dil, pad;
  int32_t dtype, split_k;      /* split_k <= 0: library heuristic */
  int32_t IC_dw, OC_dw;        /* real extents of dw ([OC_dw][KH*KW][IC_dw]); IC/OC may be padded */
  int32_t tile_hint;           /* 0 = library chooses (256x256 tiles for bf16 with OC,IC >= 256), 128 = force 128x128 */
  int32_t IH2, IW2, OH2, OW2;  /* optional second row segment, as in wseg_conv_desc (OH2 == 0: none) */
  int32_t dw_rot;              /* column rotation of dw: input channel ic accumulates into column (ic + dw_rot) % IC_dw — the PCM feature rows are
                                  [f8_3 | f8_4 | x_s] where f9.weight's columns are [x_s | f8_3 | f8_4] (resnet38_contrast.py:53: torch.cat([x_s, f8_3, f8_4])):
                                  dw_rot = 3 writes f9's gradient in the parameter's own column order (128-tile kernel only; 0 = none) */
} wseg_wgrad_desc;
int wseg_conv_wgrad(const wseg_wgrad_desc* d, void* stream);

/* ---- what a launch would run ---------------------------------------------------------------
 * The plan of wseg_conv_igemm / wseg_conv_wgrad for a descriptor: the same validation (same status, same wseg_last_error text) and the same
 * choice, made by the function the launch itself calls.  Pure host arithmetic: no data pointer is dereferenced and no device is touched, so
 * any non-NULL pointer values do. */
#define WSEG_CONV_64x128 1          /* conv_igemm_kernel, 64-row tiles (any dtype, any epilogue) */
#define WSEG_CONV_128x128 2         /* conv_igemm_kernel, 128-row tiles */
#define WSEG_CONV_224x256 3         /* conv_igemm256_kernel with 224-row tiles (NI = 7); takes what WSEG_CONV_256x256 takes */
#define WSEG_CONV_256x256 4         /* conv_igemm256_kernel with 256-row tiles (NI = 8): bf16 / split-bf16, epi 0..2, OC % 256 == 0 or a pack padded to it (w_rows) */
#define WSEG_CONV_512x128 5         /* conv_igemm512x128_kernel: bf16, epi 0..2, OC % 128 == 0, forward or stride-1 data gradient */
#define WSEG_WGRAD_128x128 6        /* conv_wgrad_kernel (any dtype) */
#define WSEG_WGRAD_256x256 7        /* conv_wgrad_pipe_kernel: bf16, IC and OC >= 256 */
typedef struct wseg_launch_plan {
  int32_t family;                   /* WSEG_CONV_* / WSEG_WGRAD_* */
  int32_t tile_rows, tile_cols;     /* conv: pixel rows x output channels; wgrad: dw rows (oc) x columns (ic) */
  int32_t nwg;                      /* workgroups of the stand-alone launch */
  int32_t perm;                     /* conv: stride-2 data gradient walking its rows in parity-class order */
  int32_t tapf;                     /* conv, 256-tile kernel: the fast tap arithmetic (32-bit offsets, no per-tap division) */
  int32_t nsplit;                   /* wgrad: pixel ranges the reduction is split over */
  int32_t unit;                     /* wgrad, pipe kernel: its UNIT variant (same-size stride-1 layers) */
} wseg_launch_plan;
int wseg_conv_plan(const wseg_conv_desc* d, wseg_launch_plan* out);
int wseg_wgrad_plan(const wseg_wgrad_desc* d, wseg_launch_plan* out);

/* A layer's data gradient (`dg`: mode 1) and a weight gradient (`wg`) as ONE launch: both depend only on dY (autograd runs them back to back:
 * network/resnet38d.py:17-44 backward), and as one grid the weight-gradient tiles back-fill the data gradient's partly filled last round and the two
 * kinds of tile do not end — and store — at the same time.  Qualifies: a bf16 stride-1 data gradient (one or two sources, `out` only, no bm_hint) whose plan is the 256-tile kernel
 * with tapf, + a weight gradient whose plan is the 256 x 256 phase-pipelined kernel; anything else runs as the two ordinary launches, in that order.
 * Same results.  Both descriptors are validated before anything is launched: a bad `wg` launches nothing, also where the pair would have run
 * as two launches.  WSEG_BWD_PAIR=0 in the environment: never one grid (scripts/profile_layers.py, scripts/check_pair_equivalence.py). */
int wseg_conv_bwd_pair(const wseg_conv_desc* dg, const wseg_wgrad_desc* wg, void* stream);
/* the plan of wseg_conv_bwd_pair: 1 = one grid of ((dg_plan.nwg + 7) & ~7) + wg_plan.nwg workgroups, 0 = two launches, < 0 = a bad descriptor
 * (launches nothing); both plans are filled as wseg_conv_plan / wseg_wgrad_plan fill them */
int wseg_conv_bwd_pair_plan(const wseg_conv_desc* dg, const wseg_wgrad_desc* wg, wseg_launch_plan* dg_plan, wseg_launch_plan* wg_plan);

/* ---- weight packing ----------------------------------------------------------------------
 * master f32 [OC][T][IC] -> fwd pack [OCp][T][ICp] and transposed pack [ICp][T][OCp] in `dtype`
 * (zero padded).  Either destination may be NULL.  ic_rot: packed input channel ic is the master's column (ic + ic_rot) % IC
 * (f9.weight's columns [x_s | f8_3 | f8_4] against the feature rows [f8_3 | f8_4 | x_s]: ic_rot = 3, resnet38_contrast.py:53); 0 = none. */
int wseg_pack_weights(const float* master, void* fwd, void* tr, int OC, int T, int IC,
                      int OCp, int ICp, int ic_rot, int dtype, void* stream);
/* the K-concatenated packs of the two-source launches ([W_a[r] | W_b[r]] rows, see wseg_conv_desc.in2) from the per-layer packs, every piece of a
 * step in ONE launch: piece p copies `rows` x `cols16` 16-byte chunks from src + src_off (row stride ld_src) to dst + dst_off (row stride ld_dst), all in
 * 16-byte units; `table` (device, int64) holds per piece {first chunk in the launch, src_off, dst_off, rows, cols16, ld_src, ld_dst}.
 * Replaces torch.cat of the packs (the reference has no counterpart: it runs the skip conv and the last conv of a block as two convolutions,
 * network/resnet38d.py:35-47, 83-97). */
int wseg_copy2d_batch(const void* src, void* dst, const long* table, int npieces, long total_chunks, void* stream);
/* every transposed pack of a training step in ONE launch: layer l is the f32 master [OC][T][IC] at master + off_in[l],
 * written as [IC][T][OC] in `dtype` at out + off_out[l] (element offsets).  `table` (device, int64) holds per layer
 * {index of its first 32x32 tile, off_in, off_out, OC, T, IC}; total_tiles = sum of ceil(OC/32)*ceil(IC/32)*T. */
int wseg_pack_transposed_batch(const float* master, void* out, const long* table, int nlayers, long total_tiles, int dtype, void* stream);
/* the same from the bf16 weight mirror (bf16 -> bf16), `table` counted in 64x64 tiles */
int wseg_pack_transposed_batch_bf16(const void* mirror, void* out, const long* table, int nlayers, long total_tiles, void* stream);
/* Dropout2d scales (resnet38d.py:64,68,86,91; resnet38_contrast.py:14,34) from uniforms u in [0,1):
 * out[i] = u[i] >= p ? 1/(1-p) : 0 with p = p0 for i < split_at, p1 after (one launch for all five masks). */
int wseg_dropout_scale(const float* u, float* out, long total, long split_at, float p0, float p1, void* stream);

/* ---- stem: conv1a (3->64, 3x3, pad 1) + the next block's frozen BN-ReLU -------------------
 * network/resnet38d.py:124,162 (+ :29-30 of b2).  x is the reference's NCHW f32 input;
 * raw = conv1a(x) NHWC, act = relu(raw*scale+shift) NHWC (either may be NULL). */
int wseg_stem_conv(const float* x_nchw, const float* w /*[64][3][3][3] = [oc][ky][kx][ic]*/,
                   const float* scale, const float* shift, void* raw, void* act,
                   int N, int H, int W, int dtype, void* stream);
/* the same with the weights transposed to [27 = (ky*3+kx)*3+ic][64 oc] (f32): the channel pairs become packed FMAs — same products,
 * same order, same results, half the vector instructions (conv1a is frozen: the caller transposes once). */
int wseg_stem_conv_kc(const float* x, const float* w_kc, const float* scale, const float* shift,
                      void* raw, void* act, int N, int H, int W, int dtype, void* stream);

/* ---- CAM head (network/resnet38_contrast.py:34-59) -------------------------------------------
 * Fused head GEMM rows are [f_proj(128) | cam logits(21) | zero pad] (ld = 192).
 * head_split : rows -> planar cam_low [N][21][hw] f32 and cmax[n][c] = max_hw relu(cam)   (:41-43)
 * cam_gate   : the no_grad normalise / bg = 1-max fg / keep-arg-max gate (:44-48) -> G [N*hw][32],
 *              G[:,21] = 1 (PCM column-sum channel), G[:,22:] = 0
 * pcm_xs     : x_s = bilinear(x, (h,w), align_corners=True) (:52) into cols [c_xs, c_xs+3) of the
 *              feature rows `feat` (row stride ld), zeroing the padding cols [c_xs+3, c_end)
 * head_grad_rows : assemble d(head rows) from d_f_proj (planar [N][128][hw], ReLU-masked by the stored
 *              rows) and d_cam_low (planar [N][21][hw]).
 */
int wseg_head_split(const void* head, int ld, int c0, float* cam_low, float* cmax, int N, int hw, int dtype, void* stream);
int wseg_cam_gate(const float* cam_low, const float* cmax, float* G, int N, int hw, void* stream);
int wseg_pcm_xs(const float* x_nchw, void* feat, int ld, int c_xs, int c_end, int N, int H, int W, int h, int w, int dtype, void* stream);
int wseg_head_grad_rows(const float* d_fproj, const float* d_cam_low, const void* head, void* d_head, int ld, int N, int hw, int dtype, void* stream);

/* planar bilinear resize of [planes][ih][iw] f32 (F.interpolate(mode='bilinear'), align_corners
 * 0/1 — resnet38_contrast.py:57-59, contrast_train.py:131-134,145-152,180; contrast_infer.py:62).
 * bwd is the exact adjoint computed by gather (deterministic). plane_mul (nullable) scales plane p;
 * plane_add (nullable, bwd) is a constant added to every d_out element of plane p (the GAP gradient). */
int wseg_resize_planar_fwd(const float* in, float* out, const float* plane_mul, long planes, int ih, int iw, int oh, int ow, int align,
                           int flip_x, int accumulate, void* stream);   /* flip_x: out[..,x] = resized[..,ow-1-x]; accumulate: out += */
int wseg_resize_planar_bwd(const float* d_out, float* d_in, const float* plane_mul, const float* plane_add, long planes, int ih, int iw, int oh, int ow, int align, int accumulate, void* stream);

/* inference post-process, contrast_infer.py:75-98: sum of 8 label-gated CAMs -> clamp, per-class
 * (x-min-1e-5)/(max-min+1e-5) with entries < min+1e-5 zeroed first, argmax against the constant bg score alpha.
 * stats = wseg_plane_stats(sum_cam, 20 planes). */
int wseg_infer_finish(const float* sum_cam, const float* stats, float alpha, float* norm_cam, unsigned char* pred, int npix, void* stream);

/* ---- PCM (network/resnet38_contrast.py:63-75), flash-style: exact-f32 MFMA here, bf16 MFMA in the *_bf16 variants below ----
 * l2norm  : Fh = F/(||F||_2 + 1e-5) over the 192 f9 channels of each pixel row (:70)
 * forward : cam_rv[n][c][j] = sum_i G[i][c] relu(Fh_i.Fh_j) / (sum_i relu(Fh_i.Fh_j) + 1e-5)  (:71-73)
 * backward: gradient w.r.t. Fh only (the CAM input is no_grad in the reference, :41-48). */
int wseg_l2norm_forward(const void* F, int ldf, float* Fh, float* nrm, long rows, int dtype, void* stream);
int wseg_l2norm_backward(const void* F, int ldf, const float* dFh, const float* nrm, void* dF, int lddf, long rows, int dtype, void* stream);
int wseg_pcm_forward(const float* Fh, const float* G, float* cam_rv, float* den, int N, int hw, void* stream);
int wseg_pcm_backward(const float* Fh, const float* G, const float* d_cam_rv, const float* cam_rv, const float* den,
                      float* DN, float* dFh, int N, int hw, void* stream);
/* split-bf16 weight pack for dtype WSEG_F32X3: f32 [.. x K] (K % 32 == 0 per row, numel % 32 == 0) -> per 32-element group
 * [32 hi bf16 | 32 lo bf16] in the same 128 bytes; `src` = a forward pack [OC][T][IC] or a transposed pack [IC][T][OC] in f32. */
int wseg_pack_x3(const float* src, void* dst, long numel, void* stream);
/* f32 [total] -> bf16 planes hi, lo with in = hi + lo to 16-17 bits (16-B aligned, contiguous) */
int wseg_split_bf16(const float* in, void* hi, void* lo, long total, void* stream);
/* bf16-MFMA variants for the bf16 throughput mode (Fb/Gb/DNb = bf16 copies made with wseg_to_bf16) */
int wseg_to_bf16(const float* in, void* out, long total, void* stream);
int wseg_pcm_forward_bf16(const void* Fb, const void* Gb, float* cam_rv, float* den, int N, int hw, void* stream);
/* backward: Gl / DNl = the LOW parts of the split G = Gb + Gl and DN = DNb + DNl (wseg_split_bf16; DNb and DNl are written here).  The gate-channel
 * product of the backward pass is a difference of two nearly cancelling sums and runs in split precision (3 bf16 MFMAs), everything else in bf16. */
int wseg_pcm_backward_bf16(const void* Fb, const void* Gb, const void* Gl, const float* d_cam_rv, const float* cam_rv, const float* den,
                           float* DN, void* DNb, void* DNl, float* dFh, int N, int hw, void* stream);

/* ---- loss step, contrast_train.py:138-395 (forward values + hand-written gradients) -----------
 * All maps planar f32 [N][21][npix]; label20 = float [N][20] multi-hot; loss outputs are device
 * scalars accumulated with atomicAdd (caller zeroes them).
 *  plane_stats        per (n,c): {max relu(U), min relu(U), sum U, argmax, argmin, 0}      (:142, visualization.py:62-66)
 *  cls_loss           mean BCE-with-logits of the GAP logits (:159-160) + its per-pixel gradient as a plane bias
 *  select_kth         k-th order statistic per row by 4-pass radix select + strict sums (torch.topk(...)[0].sum(), :22, :170-171)
 *  er_ecr_prep        ER sum + gradients, bg = 1-max fg, max_onehot, signed ECR differences (:163-169)
 *  ecr_backward       gradient of the top-K mean (:170-171)
 *  rows_resize_forward  f_proj rows -> [N*oh*ow][128] f32, bilinear align_corners=True (:179)
 *  head_grad_fused    d(head rows) = [relu-masked adjoint of rows_resize(dF) | d_cam_low | 0]
 *  pseudo_label       Q6 normalisation, bg threshold, argmax softmax(.*label) (:186-197)
 *  proto_candidates / proto_merge   per-class top-K (K = npix/8) over the batch, weighted mean, L2 norm (:199-209);
 *                     candidates are what ranks all-gather for global-batch prototypes
 *  intra_weights      hard-pixel sampling: random half + similarity rank band per class (:302-331)
 * plane_stats is implemented in csrc/maps.hip beside up_plane_stats, the pixel-to-prototype contrast (intra_weights*, nce_*) in csrc/nce.hip,
 * everything else of this section in csrc/loss.hip.
 */
size_t wseg_plane_stats_workspace_bytes(long planes);
int wseg_plane_stats(const float* U, float* stats, long planes, int npix, void* workspace, void* stream);
/* The same map losses evaluated ON THE FLY from the stride-8 maps `low` [planes][h][w] (csrc/maps.hip): the
 * reference's upsampled [N,21,S,S] tensors (resnet38_contrast.py:57-59, 540 MB per view) and their gradients are
 * never materialised; U(y,x) = bilinear(low, align_corners=True) is recomputed by one pinned expression.
 *  up_plane_stats          = plane_stats(U)                      (contrast_train.py:142,155; visualization.py:62-67)
 *  up_rvmin_values         q = max_{c>=1} U_rv*L and its arg channel per pixel (:16-22)
 *  up_norm_resize_forward  L * bilinear_{S->OS}(max_norm(U))    (:145-158)
 *  resize_adjoint_ones     wvec[y] = sum over the S upsampled rows of their weight on low-res row y (the GAP gradient)
 *  up_maps_backward        d_low[pl] = all gradients of plane pl: max_norm + resize backward of G (NULL: none) with the
 *                          max/min routes, plane_bias[pl]*wvec_y*wvec_x (NULL: none), and the min-pool selection
 *                          (q/argc/res of select_kth, NULL: none; the pixels among the k smallest q of an image with q > 0
 *                          send coef * label to their arg channel). */
int wseg_up_plane_stats(const float* low, float* stats, long planes, int h, int w, int S, const float* label20 /* nullable: all planes; else only bg + labelled classes of [N][20] */, void* workspace, void* stream);
int wseg_up_rvmin_values(const float* low, const float* label20, float* q, unsigned char* argc, int N, int h, int w, int S, void* stream);
int wseg_up_norm_resize_forward(const float* low, const float* stats, const float* label20, float* out, int N, int h, int w, int S, int OS, void* stream);
int wseg_resize_adjoint_ones(float* wvec, int h, int S, void* stream);
int wseg_up_maps_backward(const float* G, const float* low, const float* stats, const float* label20, const float* plane_bias,
                          const float* wvec_y, const float* wvec_x, const float* q, const unsigned char* argc, const float* res,
                          int k, float coef, float* d_low, int N, int h, int w, int S, int OS, void* stream);
int wseg_cls_loss(const float* stats, const float* label20, float* loss_out, float* plane_bias, int N, int npix, float coef, void* stream);
size_t wseg_select_workspace_bytes(int rows);
int wseg_select_kth(const float* vals, int rows, int n, int k, int largest, int use_abs, int relu_vals, float* res, void* workspace, void* stream);
int wseg_select_finish(const float* res, int rows, int k, int relu_vals, float scale, float* loss_out, void* stream);
/* the 8 logged scalars (contrast_train.py:174, 389-395, 401-408) from the step's accumulators acc = [cls1+cls2, (rvmin1+rvmin2)/2, er_sum, ecr, cross,
 * cross2, intra, -]:  out8 = [loss, loss_cls, loss_er, loss_ecr, loss_nce, loss_intra_nce, loss_cross_nce, loss_cross_nce2] */
int wseg_loss_finish(const float* acc, float er_coef, float* out8, void* stream);
int wseg_er_ecr_prep(const float* c1, const float* c2, const float* r1, const float* r2, float* Gc1, float* Gc2, float* dlt1, float* dlt2,
                     float* er_sum, int N, int npix, float er_coef, void* stream);
int wseg_ecr_backward(const float* dlt, const float* res, float* Gr, int N, int per_row, int k, float coef, void* stream);
int wseg_rows_resize_forward(const void* head, int ld, float* F, int N, int ih, int iw, int oh, int ow, int dtype, void* stream);
int wseg_head_grad_fused(const float* dF, const float* d_cam_low, const void* head, void* d_head, int ld, int N, int ih, int iw, int oh, int ow, int dtype, void* stream);
int wseg_pseudo_label(const float* R, const float* label20, float bg_thr, int* y, float* ncam, int N, int npix, void* stream);
int wseg_proto_candidates(const float* ncam, const float* F, const int* tie_idx, float* cand_val, float* cand_feat, int* cand_const, int N, int npix, int K, void* stream);
int wseg_proto_merge(const float* cand_val, const float* cand_feat, const int* cand_const, float* protos, int world, int K,
                     long rank_stride /* 0: contiguous [world][...] arrays; else elements between consecutive ranks' blocks (one gathered buffer) */, void* stream);
/* S_own: ld_s == 21: the [P,21] similarity table (the own-class entry is S_own[p*21 + y[p]]); ld_s == 1: one own-class similarity per pixel
 * (row 1 of the records below) */
int wseg_intra_weights(const int* y, const float* S_own, int ld_s, const float* rkey, const unsigned char* rand_flag, float* w, int P, void* stream);
/* the same sampling over the GLOBAL batch under data parallelism (the reference runs :302-334 on the gathered batch):
 * nce_records (below) writes this rank's records rec[3][P] = {label (int bits), own-class similarity, random key}; after an
 * all-gather rank r's block lies at rec + r*rank_stride and intra_weights_global returns this rank's weights, multiplied by `scale`
 * (= ranks when the gradient all-reduce averages). */
int wseg_intra_weights_global(const float* rec, float* w, int P, int ranks, int own_rank, float scale, long rank_stride, void* stream);

/* ---- fused pixel-to-prototype contrast, contrast_train.py:245-334 (csrc/nce.hip).
 * Two launches per step serve BOTH views; the normalised features and the [P,21] similarity rows
 * never reach HBM: every launch reads the raw features once (P*128*4 B) and writes only records (12 B / pixel) or dF (P*128*4 B).
 *   nce_records : rec[3][P] = {label (int bits), similarity of the pixel to its OWN class's prototype of p_own, rkey (when given)} — what the
 *                 hard-pixel sampling (intra_weights / the all-gather + intra_weights_global) needs; fields used: F, p_own, y_own, rkey, rec
 *   nce_fused   : similarities (exact-f32 MFMA) -> cross-prototype, cross-pseudo-label and intra-view InfoNCE (tau = 0.1) -> dF, and
 *                 sums[0..2] += {cross, cross2, intra} * coef; fields used: F, p_own, p_oth, y_own, y_oth, w_intra, dF
 * Per view v the "other" set is the other view's prototypes / labels (views[0] <-> views[1]); P rows each, D = 128, C = 21. */
typedef struct {
  const float* F;        /* [P][128] un-normalised projected features (f_proj resized to 16x16, rows n,i,j) */
  const float* p_own;    /* [21][128] this view's prototypes */
  const float* p_oth;    /* [21][128] the other view's prototypes */
  const int32_t* y_own;  /* [P] this view's pseudo-labels */
  const int32_t* y_oth;  /* [P] the other view's pseudo-labels */
  const float* w_intra;  /* [P] hard-pixel weights (intra_weights*) */
  const float* rkey;     /* [P] random keys copied into the records (nullable) */
  float* rec;            /* [3][P] out (nce_records) */
  float* dF;             /* [P][128] out (nce_fused) */
} wseg_nce_view;
/* nce_records, split_bf16 = 0: exact-f32 MFMA (the fp32 parity mode: the record's similarity comes from the same nce_sims16 arithmetic as the one nce_fused uses);
 * 1: split-bf16 products (hi.hi + lo.hi + hi.lo on the bf16 MFMA, 16-17 operand bits; the bf16 and bf16x3 modes — the similarity only RANKS pixels) */
int wseg_nce_records(const wseg_nce_view* views, int nviews, int P, int split_bf16, void* stream);
int wseg_nce_fused(const wseg_nce_view* views, int nviews, int P, float coef_cross, float coef_intra, float* sums /* [3], accumulated */, void* stream);

/* ---- training augmentation on the device (contrast_train.py:64-75, tool/imutils.py:6-67, network/resnet38d.py:104-118): a batch of
 * DECODED uint8 HWC images -> RandomResizeLong (Pillow's two-pass 8-bit bicubic, coefficient tables made by the host) -> horizontal flip ->
 * ColorJitter ops in the drawn order (Pillow's ImageEnhance / HSV arithmetic) -> normalise (3 x 256 table) -> RandomCrop placement -> CHW f32.
 * The host draws the random parameters (wseg_amd/augment.py, same draws in the same order as the host pipeline) and fills one
 * descriptor per image; all pointers are device pointers; `tmp` / `img` are scratch of H*rw*3 and rh*rw*3 bytes. */
typedef struct {
  const uint8_t* src; int32_t H, W;                   /* decoded image [H][W][3] */
  int32_t rh, rw;                                     /* size after RandomResizeLong */
  const int32_t* xb; const int32_t* xk; int32_t xks;  /* horizontal pass: bounds [rw][2] = (first source column, count), coefficients [rw][xks] (22 fractional bits) */
  const int32_t* yb; const int32_t* yk; int32_t yks;  /* vertical pass, over rh */
  uint8_t* tmp; uint8_t* img;
  int32_t flip;
  int32_t op[4];                                      /* colour ops in execution order: 0 brightness, 1 contrast, 2 saturation, 3 hue, -1 none */
  float factor[4];                                    /* enhancement factor of ops 0..2 */
  int32_t hue_shift;                                  /* added to the uint8 hue (mod 256) */
  int32_t cont_top, cont_left, img_top, img_left, ch, cw;   /* RandomCrop: [ch][cw] pixels from (img_top, img_left) land at (cont_top, cont_left) */
  float* out;                                         /* [3][crop][crop] */
} wseg_aug_desc;
size_t wseg_sizeof_aug_desc(void);
int wseg_augment_batch(const wseg_aug_desc* descs_dev, int n, int max_pixels /* largest H*rw or rh*rw of the batch */, const float* lut /* [3][256] */,
                       int crop, unsigned long long* lum_sums /* scratch [n][4] */, void* stream);

/* ---- AffinityNet training data on the device (aff_train.py:39-60 in the zip order of voc12/data.py:237-249): ColorJitter -> joint
 * RandomCrop of the image and the 42 CRF score planes into a crop x crop container -> normalise -> joint horizontal flip OF THE CONTAINER
 * (x -> crop-1-x) -> CHW image / 8x8 block means of the scores -> label map (voc12/data.py:251-258).  No resize.
 *
 * Image: the descriptors are wseg_aug_desc with rw = W, rh = H and `img` = the uploaded decoded image itself (the colour ops run on it in
 * place: it is scratch); src, tmp and the coefficient tables are not read.  `lut` is the table of FLOAT32 arithmetic
 * ((float(v) / 255.f - mean) / std, as numpy evaluates normalize on the float32 container); container pixels outside the pasted rectangle
 * get lut[c][0] = normalize(0), not 0. */
int wseg_aff_augment_batch(const wseg_aug_desc* descs_dev, int n, int max_pixels /* largest H*W of the batch */, const float* lut /* [3][256] */,
                           int crop, unsigned long long* lum_sums /* scratch [n][4] */, void* stream);
/* Labels: per stack (0 low alpha, 1 high alpha) only the planes with a non-zero value are shipped, np of them in ascending plane id; an
 * absent plane is a zero plane.  Scores are >= 0.  Plane k of stack s is planes[s] + k * plane_stride, [H][W] f32 (4-byte aligned rows).
 * Per output cell: the mean over the 8x8 container window of every shipped plane (zeros outside the pasted rectangle, always / 64), the
 * arg-max per stack (start: value 0 at plane 0; a later plane wins only when strictly greater = np.argmax over the dense 21 planes), then
 *   label = arg_lo;  arg_lo == 0 -> 255;  arg_hi == 0 -> 0;  max of all means < 1e-5f -> 255.
 * One launch for the batch, no atomics, a fixed summation order: out_u8 [n][crop/8][crop/8] is bit-identical from run to run. */
typedef struct {
  const float* planes[2];
  const int32_t* ids[2];                              /* [np] plane ids, ascending, each in [0, 21) */
  int32_t np[2];                                      /* 0..21 */
  int32_t H, W;
  int64_t plane_stride;                               /* floats between two shipped planes of a stack (>= H*W) */
  int32_t flip;
  int32_t cont_top, cont_left, img_top, img_left, ch, cw;   /* RandomCrop, as in wseg_aug_desc */
} wseg_aff_label_desc;
size_t wseg_sizeof_aff_label_desc(void);
int wseg_aff_labels_batch(const wseg_aff_label_desc* descs_dev, int n, int crop /* % 8 == 0 */, unsigned char* out_u8, void* stream);

/* ---- DeepLab-v1 training data on the device (segmentation/lib/datasets/BaseDataset.py:88-98 __weak_augment__ with the transforms of
 * lib/datasets/transform.py): RandomHSV on the decoded uint8 image -> RandomFlip (image and label, before the rescale) -> RandomScale (image
 * cubic, label nearest) -> ImageNorm (float32 arithmetic: the table of wseg_aff_augment_batch) -> RandomCrop into a container of +0.0 (image)
 * and 255 (label) -> CHW f32 image / uint8 label map.
 *
 * Two descriptor arrays sit side by side, one entry per image: wseg_aug_desc (layout unchanged; the resize passes read it as they do for
 * wseg_augment_batch) and wseg_seg_data_desc.  Launches (blockIdx.y = image), selected by `stages`:
 *   1  hsv      raw -> aug.src, pixelwise and out of place: 8-bit RGB -> HSV (H in [0, 180), integer arithmetic with the two division
 *               tables), h = (h + dh) mod 180 (non-negative), s / v offset and clipped, HSV -> RGB in float32 (every product and difference
 *               rounded on its own), written to column W-1-x where aug.flip is set: the resampler then reads a flipped source
 *   2  resize   the two passes of Pillow's 8-bit bicubic resampler: aug.src -> aug.tmp -> aug.img (rh x rw)
 *   4  finish   ONE launch writes both outputs: aug.out[3][crop][crop] = lut[c][img pixel] inside the pasted rectangle and +0.0 outside;
 *               lab_out[y][x] = lab[yi[img_top + y - cont_top]][xi[img_left + x - cont_left]] inside and 255 outside.  yi [rh] / xi [rw]
 *               are the host's nearest-neighbour source indices (float64 on the host; xi already composed with the flip), clamped to the
 *               label on the device.  aug.flip is NOT applied here: the hsv launch did it.
 * The hue shift, the colour ops and hue_shift of wseg_aug_desc are not read.  No atomics, no float64 on the device: the outputs are
 * bit-identical from run to run.  The entry point reads the HOST copies of the descriptors and refuses, before any launch, n <= 0,
 * crop <= 0, a null pointer a requested stage follows, non-positive sizes, ch / cw outside [1, crop] and a paste rectangle that leaves the
 * container or the rescaled image; also raw / src off a 4-byte boundary and, at crop % 4 == 0 (rows of 16-byte stores), out off a 16-byte or
 * lab_out off a 4-byte boundary.  Any other crop takes the scalar finish kernel. */
typedef struct {
  const uint8_t* raw;                                 /* decoded image [H][W][3] (H, W of the wseg_aug_desc beside it) */
  const uint8_t* lab;                                 /* label map [H][W], unflipped */
  const int32_t* yi; const int32_t* xi;               /* [rh], [rw] */
  uint8_t* lab_out;                                   /* [crop][crop] */
  int32_t dh, ds, dv;                                 /* RandomHSV offsets */
  int32_t reserved;
} wseg_seg_data_desc;
size_t wseg_sizeof_seg_data_desc(void);
#define WSEG_SEG_DATA_HSV 1
#define WSEG_SEG_DATA_RESIZE 2
#define WSEG_SEG_DATA_FINISH 4
int wseg_seg_data_batch(const wseg_aug_desc* aug_host, const wseg_seg_data_desc* seg_host, const wseg_aug_desc* aug_dev,
                        const wseg_seg_data_desc* seg_dev, int n, int crop, const float* lut /* [3][256], device */,
                        const int32_t* hsv_div /* sdiv[256] then hdiv[256], device */, int stages, void* stream);
/* launch geometry of wseg_seg_data_batch: out4 = { workgroups (of 256 threads) per image of the hsv launch for a largest image of
 * max_pixels = H*W (4 pixels per thread), of each resize pass for max_pixels = max(H*rw, rh*rw) (1 per thread), of the finish launch, container
 * pixels per finish thread (4, or 1 when crop % 4 != 0) }.  The hsv and resize launches walk their images in grid-stride loops (at most 1024
 * workgroups per image); the finish launch has one thread per 4 (or 1) container pixels and no loop. */
int wseg_seg_data_geometry(int max_pixels, int crop, int* out4);

/* ---- fused SGD step (tool/torchutils.py:23-33 -> torch.optim.SGD.step) ------------------------
 * One pass over the flat buffers: d = g*grad_scale + wd*p; buf = first ? d : momentum*buf + d;
 * p -= lr*buf.  Segments [begin,end) carry the per-group lr / weight_decay (contrast_train.py:91-96).
 * bf16_mirror (nullable): also receives the updated weights in bf16 (the next step's forward packs). */
int wseg_sgd_step(float* params, const float* grads, float* momentum_buf, long numel,
                  const long* seg_begin, const long* seg_end, const float* seg_lr, const float* seg_wd, int nseg,
                  float momentum, float grad_scale, int first_step, void* bf16_mirror, void* stream);

/* ---- AffinityNet inference: random-walk CAM refinement (network/resnet38_aff.py, aff_infer.py:14-141) -------------------
 * Pair set of radius r (tool/pyutils.py get_indices_of_pairs) on an h x w feature map, pixel p = y*w + x:
 *   offsets (dy, dx), in this order: (0, 1..r-1), then for dy = 1..r-1 every dx in (-r, r) with dx*dx + dy*dy < r*r;  P = their count
 *   (r = 5: 34).  "from" pixels: rows [0, h-r+1) x columns [r-1, w-r+1) (the reference's crop, asymmetric: the first r-1 columns
 *   have no edge to the right), n_from = (h-r+1) * (w-2r+2), f = row-major index inside that rectangle; "to" = from + (dy, dx).
 *   2 <= r <= 6 (r = 1 has no offsets: the reference fails there).  Callers pick r = (min(h,w)-1)/2 below 11, else 5.
 * The affinity matrix A (area = h*w) is symmetric: A[from][to] = A[to][from] = aff, A[i][i] = 1, every other entry 0. */
#define WSEG_AFF_MAX_OFFSETS 64
#define WSEG_RW_MAX_PLANE 8192      /* largest h*w wseg_random_walk accepts (two f32 planes in 64 KiB of LDS); larger maps are refused */
int wseg_aff_num_offsets(int radius);      /* P, or -1 for a radius outside [2, 6] */
/* aff[n][p][f] = exp(-mean_c |feat[to] - feat[from]|) over C channels, f32 accumulation (network/resnet38_aff.py:68-72).
 * feat: pixel rows [N*h*w][ld] in `dtype` (f32 or bf16; C % 8 == 0, ld % 8 == 0, C <= 512). */
int wseg_aff_pairs(const void* feat, int ld, int C, float* aff, int N, int h, int w, int radius, int dtype, void* stream);
/* the dense [area][area] f32 A of ONE image (network/resnet38_aff.py:74-89, forward(x, to_dense=True)): zeroes `dense`, then
 * scatters both orientations of every pair and the unit diagonal. */
int wseg_aff_to_dense(const float* aff, float* dense, int h, int w, int radius, void* stream);
/* random-walk stencil of N images (aff_infer.py:100-102): wgt[n][q][j] = A^beta[i][j] for the neighbour i of column j in slot q
 * (q < P: i = j + offset q, j a "from" pixel; P <= q < 2P: i = j - offset (q-P), i a "from" pixel; 0 where no such edge), and
 * rsum[n][j] = 1 / sum_i A^beta[i][j] (the diagonal counts: every sum is >= 1).  wgt: [N][2P][h*w], rsum: [N][h*w]. */
int wseg_rw_prepare(const float* aff, float* wgt, float* rsum, int N, int h, int w, int radius, int beta, void* stream);
/* 2^logt steps of v[j] <- (v[j] + sum_q v[i_q] wgt[q][j]) * rsum[j] on every plane: v_out = v_in . T^(2^logt) with T = A^beta / colsum
 * (aff_infer.py:103-108 computes the same product by logt dense squarings).  v_in / v_out: [N][planes][h*w] f32 (may alias).
 * One workgroup per plane, the plane ping-ponged in LDS; h*w <= WSEG_RW_MAX_PLANE. */
int wseg_random_walk(const float* wgt, const float* rsum, const float* v_in, float* v_out, int N, int planes, int h, int w, int radius,
                     int logt, void* stream);
/* the walk's input of one image (aff_infer.py:85-98): a 21-plane [21][H][W] map with plane 0 = bg, plane c = cams[src[c]] for
 * src[c] >= 0 (zero when src[c] < 0), zero padded to [8*dh][8*dw], then 8x8 average pooling -> pooled [21][dh][dw].
 * cams: [ncams][H][W] f32 device; src: 21 host ints. */
int wseg_rw_pool(const float* cams, const int* src, float bg, float* pooled, int H, int W, int dh, int dw, void* stream);
/* bilinear upsample (align_corners=False) of cam_rw [planes][dh][dw] to [8*dh][8*dw], arg-max over the planes (the first maximum wins),
 * cropped to [H][W] (aff_infer.py:110-139): pred uint8 [H][W].  planes <= 32. */
int wseg_rw_finish(const float* cam_rw, unsigned char* pred, int planes, int dh, int dw, int H, int W, void* stream);

/* ---- AffinityNet training loss (aff_train.py:111-119 on network/resnet38_aff.py:57-63) and its gradient on the feature rows ----------
 * label: uint8 [N][h][w] device, 0 background, 1..20 a class, 255 ignore.  Per pair (from f, to t) the indicators of voc12/data.py:170-199:
 *   valid = label[f] < 255 && label[t] < 255;  bg = equal && label[f] == 0;  fg = equal && label[f] != 0 && valid;  neg = !equal && valid.
 * feat: pixel rows [N*h*w][ld] in `dtype` (f32 or bf16; C % 8 == 0, C <= 512, ld >= C, ld % 8 == 0).
 * out7 (f32 device): loss, bg_loss, fg_loss, neg_loss, bg_cnt, fg_cnt, neg_cnt with cnt = float(pairs) + 1e-5f, x_loss = sum / cnt over
 *   the terms -log(aff + 1e-5) (bg, fg) / -log(1.00001 - aff) (neg), loss = bg/4 + fg/4 + neg/2.  No atomics: term sums per wave in f32,
 *   per workgroup through LDS, then one workgroup in f64 in a fixed order; the pair counts are integers throughout.  The seven values
 *   are bit-identical from run to run; a label map without a valid pair gives 0, 0, 0, 0, 1e-5, 1e-5, 1e-5.
 * Every argument check runs before the first device call. */
long wseg_aff_loss_workspace_bytes(int N, int h, int w, int radius);      /* -1 (and wseg_last_error) for a bad geometry */
/* aff: [N][P][n_from] f32 as wseg_aff_pairs writes it, or NULL for a loss-only call (the backward needs it). */
int wseg_aff_loss_forward(const void* feat, int ld, int C, const unsigned char* label, float* aff, void* workspace, float* out7, int N,
                          int h, int w, int radius, int dtype, void* stream);
/* d_feat[N*h*w][ld_d] f32 = gscale * d out7[0] / d feat (gscale: one f32 on the device, NULL = 1; out7 is read on the device as well).
 * One wave per pixel gathers the pairs it belongs to in a fixed order: columns < C of EVERY row are written (zeros where a pixel is in
 * no valid pair), columns >= C are untouched; a channel on which the two rows of a pair tie gets no contribution (sign(0) = 0). */
int wseg_aff_loss_backward(const void* feat, int ld, int C, const unsigned char* label, const float* aff, const float* out7,
                           const float* gscale, float* d_feat, int ld_d, int N, int h, int w, int radius, int dtype, void* stream);
/* The backward of wseg_aff_pairs: d_feat[N*h*w][ld_d] f32 = sum over the pairs a pixel belongs to of d_aff[n][p][f] * d aff[n][p][f] / d feat,
 * with aff = exp(-mean_c |f_to - f_from|) as wseg_aff_pairs wrote it (read, not recomputed) and feat the rows it read.  The row walk of
 * wseg_aff_loss_backward with another coefficient (-aff * d_aff / C * sign(f_to - f_from), sign(0) = 0): same write contract, no atomics,
 * bit-identical from run to run; rows of pixels in no pair are zero. */
int wseg_aff_pairs_backward(const void* feat, int ld, int C, const float* aff, const float* d_aff, float* d_feat, int ld_d, int N,
                            int h, int w, int radius, int dtype, void* stream);

/* ---- AffinityNet head, training (network/resnet38_aff.py:39-42: f8_3, f8_4, f8_5, f9 = F.elu(conv(.))): the ELU backward on pixel rows ----
 *   dz[m][c] = gscale * g[m][c] * (y[m][c] > 0 ? 1 : y[m][c] + 1)   for m in [0, M), c in [0, C)
 * y: the saved ELU OUTPUT (elu' = 1 above zero, exp(z) = y + 1 below: no pre-activation is kept); g: the upstream gradient; gscale: one f32
 * on the device, NULL = 1 (nothing synchronises with the host).  g, y, dz: rows of ld_g / ld_y / ld_dz elements in g_dtype / y_dtype /
 * dz_dtype (WSEG_F32 or WSEG_BF16 each, in any combination: the kernel is also the f32 -> bf16 cast of the loss gradient).  Streaming:
 * 16-byte loads and stores, so C % 8 == 0, every ld % 8 == 0 and >= C, 16-byte aligned bases — anything else is refused before any
 * device call.  Columns >= C of dz are never written.  dz may alias g when dtype and ld agree.
 * Exact: y > 0 gives gscale * g rounded once to dz_dtype; y == -1 gives 0; y == 0 takes the y + 1 branch (derivative 1). */
int wseg_elu_backward_rows(const void* g, int ld_g, int g_dtype, const void* y, int ld_y, int y_dtype, const float* gscale, void* dz,
                           int ld_dz, int dz_dtype, long M, int C, void* stream);

/* ---- fully connected CRF, mean field with exact Gaussian kernels (contrast_infer.py:102-134 --out_crf, aff_prepare.py:34-50) ----------
 * The reference calls pydensecrf, whose filters are a permutohedral-lattice approximation; these entry points evaluate every pair
 * (DESIGN.md §3 "crf" states the update).  One image of N = H*W pixels (pixel i = y*W + x), M labels, S label sets sharing the image.
 * Buffers of the all-pairs filter, npad = wseg_crf_padded_pixels(N) (N rounded up to WSEG_CRF_PIX_ALIGN), NC = wseg_crf_columns(S, M):
 *   feat [npad/4][8][4]  f32   pixel quad, feature (x, y, r, g, b, 0, 0, 0) as integers, slot i & 3
 *   Qn   [npad/4][NC][4] f32   pixel quad, column s*M + c, slot i & 3: n_i * Q, zero for i >= N and in the unused columns
 *   out  [npad][NC]      f32   sum_j k(f_i, f_j) * Qn[j][column] (rows i >= N hold finite values nobody reads)
 * All pointers are device pointers the caller allocated; nothing is allocated or synchronised inside. */
#define WSEG_CRF_PIX_ALIGN 128
#define WSEG_CRF_MAX_LABELS 32
#define WSEG_CRF_MAX_COLUMNS 64     /* S * M rounded up to 16 (21 labels: S <= 3) */
#define WSEG_CRF_MAX_RADIUS 128     /* window radius ceil(6.5 * sxy) of the separable Gaussian (sxy <= 19.6) */
#define WSEG_CRF_BG_CONST 0
#define WSEG_CRF_BG_POWER 1
int wseg_crf_padded_pixels(int npix);
int wseg_crf_columns(int S, int n_labels);
/* labels[i] = argmax_c T[c][i], the first maximum winning: T[c] = cams[src[c]] for src[c] >= 0 (else 0), c = 1..n_labels-1;
 * T[0] = param (rule WSEG_CRF_BG_CONST) or (1 - max_c T[c][i])^param with T[0] = 0 inside the max (rule WSEG_CRF_BG_POWER).
 * cams: [ncams][npix] f32 device; src: n_labels host ints (src[0] ignored). */
int wseg_crf_labels(const float* cams, const int* src, int n_labels, int rule, float param, unsigned char* labels, int npix, void* stream);
/* img uint8 [H][W][3] -> feat, the unit column `ones` ([npad/4][16][4]: column 0 = 1 for i < N) the normalisation pass filters, and the
 * Gaussian's ng[i] = 1/sqrt(sum_j k + 1e-20) over its window. */
int wseg_crf_prepare(const unsigned char* img, int H, int W, float gauss_sxy, float* feat, float* ones, float* ng, void* stream);
/* the hot path: out = K . Qn over ALL pairs, K[i][j] = exp(-((dx^2+dy^2)/sxy^2 + (dr^2+dg^2+db^2)/srgb^2)/2); k in f32 on the VALU from
 * exact integer differences, the product on v_mfma_f32_16x16x4_f32 (exact f32 accumulation).  ncols = NC (16, 32, 48 or 64). */
int wseg_crf_bilateral(const float* feat, const float* Qn, float* out, int npix, int ncols, float sxy, float srgb, void* stream);
/* n[i] = 1/sqrt(sums[i*stride] + 1e-20): the bilateral n from column 0 of wseg_crf_bilateral(feat, ones, ...) (stride 16) */
int wseg_crf_rsqrt(const float* sums, int stride, float* n, int npix, void* stream);
/* out[p][y][x] = sum over the window of exp(-(dx^2+dy^2)/(2 sxy^2)) * in[p][y+dy][x+dx], two 1-D passes through tmp (same size) */
int wseg_crf_gaussian(const float* in, float* tmp, float* out, int planes, int H, int W, float sxy, void* stream);
/* one mean-field update for S label sets (labels uint8 [S][npix]): logit[c] = -U[c] + w_gaussian * ng[i]*outg[s*M+c][i] +
 * w_bilateral * nb[i]*outb[i][s*M+c] with U[c] = -ln(gt_prob) at c == label, -ln((1-gt_prob)/(M-1)) elsewhere; Q = softmax(logit).
 * outb == outg == NULL: the initial Q = softmax(-U).  Writes the next filter inputs Qn (= nb*Q, layout above) and Qg (= ng*Q,
 * [S*M][npix]) and, where non-NULL, Qout / logits ([S][M][npix] f32) and amax (uint8 [S][npix], the first maximum). */
int wseg_crf_update(const unsigned char* labels, const float* outb, const float* outg, const float* nb, const float* ng, float* Qn,
                    float* Qg, float* Qout, float* logits, unsigned char* amax, int S, int n_labels, int npix, float gt_prob,
                    float w_bilateral, float w_gaussian, void* stream);
/* the same update for ONE label set whose unary comes from probabilities (pydensecrf's unary_from_softmax, segmentation/lib/utils/DenseCRF.py:17):
 * U[c] = -ln(min(max(prob[c][i], 1e-5), 1)), prob f32 [n_labels][npix]; everything else as wseg_crf_update with S = 1 (one kernel body). */
int wseg_crf_update_prob(const float* prob, const float* outb, const float* outg, const float* nb, const float* ng, float* Qn, float* Qg,
                         float* Qout, float* logits, unsigned char* amax, int n_labels, int npix, float w_bilateral, float w_gaussian,
                         void* stream);

/* ---- DeepLab multi-scale test fusion (segmentation/experiment/SEAM_deeplabv1_resnet38/test.py:71-104) in ONE launch --------------------
 * Per pass (one scale, plain or x-flipped) the reference resamples the net's stride-8 logits bilinearly (align_corners=True) to the scaled
 * input size (ih, iw) (deeplabv1.py:50), resamples that again (align_corners=True) to the original (H, W), un-flips an odd entry with
 * torch.flip, then takes the mean over the passes, the softmax over classes and the arg-max.  Here every output pixel composes the two
 * resamples itself: its 2 x 2 stage-2 taps of the (ih, iw) grid are each evaluated from their own 2 x 2 stage-1 taps of the coarse
 * (fh, fw) grid — ATen's align_corners coordinate rule (scale = (in - 1) / (out - 1), 0 when out == 1, in f32) at both stages, the
 * intermediate value rounded to f32 as the materialised map would be.  A flipped pass is SAMPLED at the mirrored output column W - 1 - x
 * (what the flip after the resize does; the weights are not mirrored).  The passes are summed in array order and the sum divided by n_pass.
 * rows: cls_conv pixel rows [images * fh * fw][ld] (ld % 8 == 0, ld >= n_cls rounded up to 8, 16-byte aligned), dtype WSEG_F32 or WSEG_BF16;
 * img: the image inside the batch the rows belong to.  One thread per output pixel, the class sums in registers; no LDS, no atomics.
 * Outputs (NULL: not written, amax is required): mean_logits / prob (the softmax of the mean) f32 [n_cls][H * W], amax uint8 [H * W] (the
 * first maximum of the mean wins, torch.argmax's rule), margin f32 [H * W] = top-1 minus top-2 of the mean. */
#define WSEG_SEG_MAX_PASSES 16
#define WSEG_SEG_MAX_CLASSES 32
typedef struct wseg_seg_pass {
  const void* rows;
  int32_t ld, dtype, img;
  int32_t fh, fw;      /* coarse (stride-8) dims */
  int32_t ih, iw;      /* intermediate dims: the scaled input's size */
  int32_t flip;
} wseg_seg_pass;
size_t wseg_sizeof_seg_pass(void);
int wseg_seg_fuse(const wseg_seg_pass* passes, int n_pass, int H, int W, int n_cls, float* mean_logits, float* prob, unsigned char* amax,
                  float* margin, void* stream);

/* ---- DeepLab-v1 training loss (deeplabv1.py:50 + train.py:85,97): the cross-entropy (ignore_index 255, mean over the valid pixels of the
 * BATCH) of the stride-8 logits resampled bilinearly (align_corners=True) to the label size, and its gradient on the coarse rows, without the
 * full-size [N][n_cls][H][W] tensor: each label pixel samples its image's coarse rows itself (the source-index arithmetic of wseg_seg_fuse).
 * rows:  cls_conv pixel rows [N*fh*fw][ld] in `dtype` (WSEG_F32 or WSEG_BF16), ld % 8 == 0, ld >= n_cls rounded up to 8, 16-byte aligned;
 *        the classes are columns [0, n_cls), columns >= n_cls are never used.  2 <= n_cls <= WSEG_SEG_MAX_CLASSES.
 * label: uint8 [N][H][W] device; 0 .. n_cls-1 a class, 255 ignore; a value in [n_cls, 255) is ignored as well and counted in out4[3].
 * Any H, W >= 1 and fh, fw >= 1 (H < fh: a downsample); H, W, fh, fw < 2^24 and N*H*W < 2^31.
 * lse:   f32 [N][H][W], the log-sum-exp over the classes of every pixel's sample (what the backward needs), or NULL for a loss-only call.
 * out4 (f32 device): loss = sum / count, count of valid pixels, sum of nll = lse - z[label] over them, count of out-of-range labels.  The
 *   counts are integer sums (out4 holds them converted to f32); the nll sum is reduced per workgroup in a fixed order into the workspace and
 *   then by one workgroup in f64 in a fixed order: no atomics, bit-identical from run to run, nothing synchronises with the host.  A batch
 *   without a valid pixel gives loss = 0 / 0 = NaN (torch's answer) and a zero gradient (torch's as well).
 * Every argument check runs before the first device call. */
long wseg_seg_ce_workspace_bytes(int N, int H, int W);                   /* -1 (and wseg_last_error) for a bad size */
int wseg_seg_ce_forward(const void* rows, int ld, int dtype, const unsigned char* label, float* lse, void* workspace, float* out4, int N,
                        int fh, int fw, int H, int W, int n_cls, void* stream);
/* d_rows[N*fh*fw][ld_d] in d_dtype (WSEG_F32 or WSEG_BF16: the f32 sum rounded once) = gscale * d out4[0] / d rows (gscale: one f32 on the
 * device, NULL = 1; count is read from out4 on the device).  GATHER form, one wave per coarse cell: the lanes walk the fine pixels whose taps
 * include the cell — a conservative range, each pixel tested with the forward's own f32 source index, never an inverted scale — recompute
 * the softmax from the four coarse rows and the saved lse, and add w_y * w_x * (softmax_c - [c == label]) in a fixed order; one fixed
 * butterfly across the lanes, then one multiplication by gscale / count.  No atomics, bit-identical from run to run.  Columns
 * [0, n_cls rounded up to 8) of EVERY row are written (zeros in the columns >= n_cls and in the rows of cells no valid pixel touches), the
 * columns beyond are untouched.  ld_d % 8 == 0, ld_d >= n_cls rounded up to 8, d_rows 16-byte aligned. */
int wseg_seg_ce_backward(const void* rows, int ld, int dtype, const unsigned char* label, const float* lse, const float* out4,
                         const float* gscale, void* d_rows, int ld_d, int d_dtype, int N, int fh, int fw, int H, int W, int n_cls,
                         void* stream);

/* ---- DeepLab-v1 head, training mode (deeplabv1.py:42-49 under train.py:52's plain nn.BatchNorm2d): what lies between the three convolutions,
 * on pixel rows [M][ld] in WSEG_F32 or WSEG_BF16.  Rows are read and written in 8-column (16-byte) chunks: C % 8 == 0, every ld % 8 == 0 and
 * >= C, every base 16-byte aligned (the per-column f32 vectors too, except the outputs of wseg_bn_stats and wseg_col_sums).  Every argument
 * check runs before the first device call; nothing synchronises with the host; no kernel uses atomics and every reduction has a fixed order
 * (per row chunk in f32 registers, the four waves of a workgroup in a fixed order, the chunks in f64, a column's by ONE workgroup), so every output is
 * bit-identical from run to run.
 * The workspace of wseg_bn_stats, wseg_bn_relu_backward and wseg_col_sums (there with C rounded up to 8) is wseg_bn_stats_workspace_bytes(M, C)
 * = (3 * row_chunks + 3) * C floats, 16-byte aligned; -1 (and wseg_last_error) for a bad size.  row_chunks is 1 up to M = 32. */
long wseg_bn_stats_workspace_bytes(long M, int C);
/* The batch statistics of F.batch_norm(x, running_mean, running_var, gamma, beta, training=True, momentum, eps) (ATen batch_norm_stats +
 * batch_norm_gather_stats_with_counts / native_batch_norm's training branch) over the M rows of every column: mean[C], invstd[C] =
 * 1/sqrt(var + eps) with the biased variance, and where scale / shift are non-NULL the fold scale = gamma * invstd, shift = beta - mean * scale
 * (each rounded once from f64).  running_mean / running_var (either may be NULL) become (1 - momentum) * running + momentum * stat, the variance
 * unbiased (var * M / (M - 1)).  M < 2 is refused (torch: "Expected more than 1 value per channel").  The variance is not E[x^2] - mean^2
 * in f32: a chunk's partial is (shift, sum (x - shift), sum (x - shift)^2) about its own first row, re-centred and merged in f64. */
int wseg_bn_stats(const void* x, int ld, int dtype, long M, int C, const float* gamma, const float* beta, double eps, double momentum,
                  float* mean, float* invstd, float* scale, float* shift, float* running_mean, float* running_var, void* workspace,
                  void* stream);
/* y = relu(z * scale[c] + shift[c]) (one fma in f32), times keep / (1 - p) when p > 0 (nn.Dropout(p): ATen native_dropout / bernoulli_), rounded
 * once to y's dtype.  The keep bit comes from a counter hash, no mask tensor exists: with mix32 the two-round xorshift-multiply of
 * wseg_amd/synth.py's hash_uniform, i = row * C + col, u = mix32((mix32(i) + key) mod 2^32) >> 8, keep iff u * 2^-24 >= p
 * (synth.dropout_keep restates it on the host, bit for bit).  M * C < 2^32.  y may be z (same dtype and ld). */
int wseg_bn_relu_drop(const void* z, int ld_z, int z_dtype, const float* scale, const float* shift, void* y, int ld_y, int y_dtype, long M,
                      int C, float p, unsigned key, void* stream);
/* The backward of dropout . relu . batch_norm(training=True) (ATen native_dropout_backward, threshold_backward, native_batch_norm_backward) in
 * three launches (reduce, finish, apply): dy = s * g * [y > 0] on the STORED y (the gate covers ReLU and dropout at once; s = 1 or 1/(1 - p)),
 * xhat = (z - mean) * invstd, s1 = sum dy, s2 = sum dy * xhat per column, dz = gamma * invstd * (dy - s1/M - xhat * s2/M) rounded once to
 * `dtype`, the dtype of y, z and dz; g is f32 or bf16 (g_dtype).  d_beta = s1 and d_gamma = s2 are written where non-NULL.  dz may be g (same
 * dtype and ld), not y or z. */
int wseg_bn_relu_backward(const void* g, int ld_g, int g_dtype, const void* y, int ld_y, const void* z, int ld_z, int dtype, const float* mean,
                          const float* invstd, const float* gamma, float s, void* dz, int ld_dz, float* d_gamma, float* d_beta, long M, int C,
                          void* workspace, void* stream);
/* out[c] = sum over the M rows of rows[r][c] for c < C (f32; at::sum over the pixel dims, cls_conv's bias gradient): C need not be a multiple
 * of 8, whole chunks are read (ld >= C rounded up to 8) and the pad columns' sums are not written. */
int wseg_col_sums(const void* rows, int ld, int dtype, long M, int C, float* out, void* workspace, void* stream);

/* ---- evaluation counters (eval.py:22-52): integer pixel counts, ADDED into a caller-owned device buffer of unsigned 64-bit cells, so one
 * buffer collects a whole dataset and is read back once.  Both run on `stream` and synchronise nothing.  The ground-truth axis has
 * WSEG_EVAL_ROWS = 22 rows: 0..20 the classes, 21 = "a value in 21..254" (the evaluator counts such a pixel towards P of its predicted
 * class and towards no T or TP); a pixel whose gt is 255 is skipped.  All counting is in integers (32-bit per workgroup in LDS, 64-bit
 * in the buffer): the result is exact and does not depend on the order of the adds.  n <= 2^40 pixels per call. */
#define WSEG_EVAL_ROWS 22
#define WSEG_EVAL_CLASSES 20        /* foreground classes: planes of the curve, the winner axis of its histogram */
#define WSEG_EVAL_MAX_THR 64
/* conf[min(gt, 21)][min(pred, 21)] += 1 for every pixel with gt != 255.  pred, gt: uint8 [n] device; conf: u64 [22][22] device. */
int wseg_eval_confusion(const unsigned char* pred, const unsigned char* gt, long n, unsigned long long* conf, void* stream);
/* The background-threshold curve in one pass.  Class c (0..19) scores planes[src[c] * plane_stride + i] at pixel i, or 0.0 where
 * src[c] == -1 (the class is not in the image's dictionary); src: 20 host ints, each in -1..nplanes-1 (planes may be NULL when nplanes
 * is 0).  Per pixel: m = the largest of the 20 scores, c = the lowest class that attains it, k = the number of thresholds strictly below
 * m (float32 comparisons), and hist[min(gt, 21)][c][k] += 1.  np.argmax over [t] ++ scores is c + 1 for the thresholds thr[i] with
 * i < k and 0 for the rest, so suffix sums over k give every threshold's confusion matrix.  All 20 classes absent: m = 0, c = 0.
 * thr: T HOST floats, non-decreasing, 1 <= T <= WSEG_EVAL_MAX_THR (they travel as a launch argument); hist: u64 [22][20][T+1] device.
 * NaN scores are out of contract (no out-of-range access, but the cell such a pixel lands in is unspecified); infinities compare as
 * float32 does.  The workgroup histogram covers only the live winners (the present classes and the first absent one); when that
 * exceeds 64 KiB of LDS (about 12 present classes at T = 60) the pixels add straight into `hist` with 64-bit global atomics. */
int wseg_eval_curve(const float* planes, long plane_stride, int nplanes, const int* src, const unsigned char* gt, long n,
                    const float* thr, int T, unsigned long long* hist, void* stream);

#ifdef __cplusplus
}
#endif
#endif
