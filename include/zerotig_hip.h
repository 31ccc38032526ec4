/* C ABI of libzerotig_hip.so -- the drop-in boundary for the Zero-TIG hot path on MI355X (gfx950).
 *
 * The reference has no FFI: its seam is the Python surface (model.model.Network / loss.LossFunction / utils.utils,
 * SURVEY 8(b)).  The one native hook it anticipates is `alt_cuda_corr.forward` (model/RAFT/corr.py:86).  Each entry
 * point below replaces the ATen call(s) of the cited reference lines.  Conventions:
 *   - plain pointers to DEVICE memory + sizes; no torch types; the caller owns every buffer (inputs, outputs,
 *     workspaces) and keeps it alive until the stream reaches the next op; nothing here allocates or synchronises;
 *   - every function enqueues on `stream` (hipStream_t passed as void*) and returns 0, a hipError_t, or 1001
 *     (invalid argument); the Python host raises RuntimeError on non-zero (zero-tig_amd/lib.py);
 *   - `dt` arguments select the storage type of nhwc activation buffers: 0 = fp32, 1 = bf16 (raw 16-bit, round-to-nearest-even)
 *   - "planar" = [C][H][W] fp32 (the reference's NCHW with N == 1); "nhwc" = [N][H][W][ld] fp32 with an explicit
 *     channel stride `ld` so channel slices of wider buffers can be addressed without copies.
 */
#ifndef ZEROTIG_HIP_H
#define ZEROTIG_HIP_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef void* zt_stream_t;

/* utils/utils.py:203-230 warp_tensor x2 (model.py:249-250), fused.  flow: planar [2][Hf][Wf]; imgA/imgB/outA/outB: planar
 * [C][H][W] (imgB/outB may both be NULL); taps: optional int32 [H][W][2] = floor of the source coordinates (x0,y0). */
int zt_warp2_f32(const float* flow, int Hf, int Wf, const float* imgA, const float* imgB, float* outA, float* outB,
                 int* taps, int C, int H, int W, zt_stream_t stream);


/* ---- stencil primitives on planar tensors (zt_stencil.hip) ------------------------------------------------ */
/* utils/utils.py:15-24 pair_downsampler: o1 = (x[2y,2x+1]+x[2y+1,2x])/2, o2 = (x[2y,2x]+x[2y+1,2x+1])/2; outputs [C][H/2][W/2] */
int zt_pair_down_f32(const float* src, float* o1, float* o2, int C, int H, int W, zt_stream_t stream);
/* adjoint of the above: dst[C][H][W] (+)= pd^T(g1, g2) */
int zt_pair_down_adj_f32(const float* g1, const float* g2, float* dst, int C, int H, int W, int accumulate, zt_stream_t stream);
/* utils/utils.py:52-58 blur: reflect-pad 10 + 21x21 Gaussian, as two 21-tap passes; taps21_host: HOST pointer to the 1-D factor */
int zt_blur21_f32(const float* src, float* tmp, float* dst, const float* taps21_host, int C, int H, int W, zt_stream_t stream);
int zt_blur21_adj_f32(const float* g, float* tmp, float* dst, const float* taps21_host, int C, int H, int W, int accumulate, zt_stream_t stream);
/* utils/utils.py:41-50 LocalMean (reflect-pad 2, 5x5 mean) and its adjoint (dst (+)= scale * LM^T(src)) */
int zt_box5_reflect_f32(const float* src, float* dst, int C, int H, int W, zt_stream_t stream);
int zt_box5_reflect_adj_f32(const float* src, float* dst, int C, int H, int W, float scale, int accumulate, zt_stream_t stream);
/* utils/utils.py:60-79 calculate_local_variance of x = a - b (b may be NULL): D = x - box0(x)/25 (saved for backward, may be NULL), V = box0(D^2)/25 */
int zt_localvar_fwd_f32(const float* a, const float* b, float* D, float* V, int C, int H, int W, zt_stream_t stream);
/* backward: xbar (+)= sign * (E - box0(E)/25), E = 2 D box0(gV)/25 */
int zt_localvar_bwd_f32(const float* D, const float* gV, float* xbar, int C, int H, int W, float sign, int accumulate, zt_stream_t stream);
/* both variance maps of the loss in one launch: (DA, VA) = localvar(a), (DX, VX) = localvar(b - a); same arithmetic as two
   zt_localvar_fwd_f32 calls */
int zt_localvar_fwd_pair_f32(const float* a, const float* b, float* DA, float* VA, float* DX, float* VX, int C, int H, int W, zt_stream_t stream);
/* the variance term's backward in one launch, equal to zt_localvar_bwd_f32(DN, gV, dH3, -1, accumulate) followed by
   zt_localvar_bwd_f32(DH2, gV, dH2x, +1, write) and zt_localvar_bwd_f32(DN, gV, dH2x, +1, accumulate) */
int zt_localvar_bwd_pair_f32(const float* DN, const float* DH2, const float* gV, float* dH3, float* dH2x, int C, int H, int W, zt_stream_t stream);
/* dst[C][H][W] = pd^T(g1 - box5_reflect^T(u1), g2 - box5_reflect^T(u2)) for half-resolution u1, u2, g1, g2 [C][H/2][W/2]: equal to
   zt_box5_reflect_adj_f32(scale -1, accumulate) on g1 and g2 followed by zt_pair_down_adj_f32, without writing g1 / g2 back */
int zt_half_bwd_f32(const float* u1, const float* u2, const float* g1, const float* g2, float* dst, int C, int H, int W, zt_stream_t stream);
/* loss.py:99-136 TextureDifference: a, b planar [3][H][W] -> mask [H][W] in {0,1}; ratio (optional) = 2 s1 s2 / (s1^2+s2^2+1e-5) */
int zt_texture_mask_f32(const float* a, const float* b, float* mask, float* ratio, int H, int W, zt_stream_t stream);
/* loss.py:178-190 SmoothLoss.rgb2yCbCr over the flat memory (nelem = 3*H*W) */
int zt_ycc_flat_f32(const float* src, float* dst, long long nelem, zt_stream_t stream);


/* ---- MFMA implicit-GEMM convolution family (zt_conv*.hip, zt_wgrad.hip) --------------------------------
 * Replaces F.conv2d of model.py:20-27, 36-43, 55-80, every conv of model/RAFT/{extractor,update}.py, and (as a 1x1
 * conv whose "weights" are fmap2) the all-pairs matmul of corr.py:52-60.
 * x: nhwc [N][H][W][ldx] (first Cin channels used; channels >= csplit come from x2 [..][ldx2] when x2 != NULL);
 * w: device layout [KH*KW][Cin][ldw] (zt_repack_conv_weight_f32); y: nhwc [N][Ho][Wo][ldy], or planar
 * [N][Cout] planes of pitch ldy when out_planar; y = act(alpha * (conv + bias)) then epi: 0 none,
 * 1: *= LeakyReLU'(aux) (aux>0 ? 1 : 0.2), 2: *= (aux>0), 3: += aux  (aux nhwc, stride ldaux).
 * act: 0 none, 1 ReLU, 2 LeakyReLU(0.2), 3 sigmoid, 4 tanh, 5 clamp(sigmoid, 1e-4, 1).
 * Supported (KH,KW,stride): (3,3,1|2) (1,1,1|2) (1,5,1) (5,1,1) (7,7,1|2). */
int zt_conv2d_nhwc_f32(const float* x, const float* x2, int csplit, int ldx, int ldx2, int N, int H, int W, int Cin,
                       const float* w, int ldw, const float* bias, float* y, int ldy, int out_planar, int Cout, int KH,
                       int KW, int stride, int padH, int padW, int act, float alpha, const float* aux, int ldaux,
                       int epi, zt_stream_t stream);
/* same with the fused SepConvGRU epilogues of model/RAFT/update.py:42-58 (nhwc output only):
 * epi 4: [z | r] = act(conv): channels < esplit are stored to y; channels >= esplit leave as r * h to y2 [..][ldy2] at channel
 *        co - esplit (aux = h, nhwc ldaux)                                    == `torch.cat`-free `r * h` of update.py:44/52
 * epi 5: q = act(conv): y (= h, read and written in place) <- (1 - z) * h + z * q, aux = z   == update.py:46/54 */
int zt_conv2d_nhwc_f32_ex(const float* x, const float* x2, int csplit, int ldx, int ldx2, int N, int H, int W, int Cin,
                          const float* w, int ldw, const float* bias, float* y, int ldy, int out_planar, int Cout, int KH,
                          int KW, int stride, int padH, int padW, int act, float alpha, const float* aux, int ldaux,
                          int epi, float* y2, int ldy2, int esplit, zt_stream_t stream);
/* weight gradient of a stride-1 "same" conv (autograd of the above): grad_w [Cout][Cin][KH][KW] (torch layout)
 * (+)= sum_p x[p+tap][ci] dz[p][co]; grad_b [Cout] (optional) (+)= sum_p dz[p][co] (bias gradient, folded into the same pass);
 * slab: workspace for per-workgroup partials (deterministic reduction). */
int zt_conv2d_wgrad_nhwc_f32(const float* x, int ldx, const float* dz, int lddz, int H, int W, int Cin, int Cout, int KH,
                             int KW, float* slab, size_t slab_bytes, float* grad_w, float* grad_b, int accumulate, zt_stream_t stream);
/* torch weight [Cout][Cin][KH][KW] -> device layout [tap][Cin][ldw] at column offset co_off (transpose_flip = 0), or the
 * data-gradient operator [tap flipped][Cout][ldw] with in/out channels exchanged (transpose_flip = 1). */
int zt_repack_conv_weight_f32(const float* src, float* dst, int Cout, int Cin, int KH, int KW, int ldw, int co_off,
                              int transpose_flip, zt_stream_t stream);


/* ---- normalisation (zt_norm.hip): nn.BatchNorm2d of model.py:62 (train mode, shared 3x), eval BatchNorm /
 * InstanceNorm of model/RAFT/extractor.py:117-191.  All on nhwc buffers, C % 4 == 0. ------------------------------- */
/* per-(n,c) partial sums over HW pixels: partial[((n*nblk+blk)*2 + {0 sum, 1 sum of squares})*C + c] */
int zt_chan_stats_nhwc(const void* x, int dt, int ldx, int N, int HW, int C, int nblk, float* partial, zt_stream_t stream);
/* mode 0 instance norm (scale = rstd, shift = -mean*rstd); 1 train BN (batch stats, running stats += momentum update with
 * unbiased variance, *num_batches_tracked += 1); 2 eval BN (running stats).  Outputs scale/shift (and mean/rstd) [N][C].
 * Requires N, C, count > 0; modes 0 and 1 read partial and need nblk > 0 (mode 2 ignores both: partial may be NULL);
 * mode 1 needs N == 1 and count > 1 (the unbiased variance of one value per channel is undefined: torch raises). */
int zt_norm_finalize_f32(const float* partial, int nblk, int N, int C, long long count, float eps, int mode,
                         const float* gamma, const float* beta, float* running_mean, float* running_var,
                         long long* num_batches_tracked, float momentum, float* scale, float* shift, float* mean_out,
                         float* rstd_out, zt_stream_t stream);
/* InstanceNorm statistics and scale/shift in one launch (RAFT feature encoder, reference model/RAFT/extractor.py:117-191,
   nn.InstanceNorm2d: biased variance, no affine): partial rows as zt_chan_stats_nhwc; the last workgroup of each sample writes
   scale[n*C+c] = rstd, shift = -mean*rstd.  tickets: N zero-initialised counters, left at zero. */
int zt_instance_norm_stats(const void* x, int dt, int ldx, int N, int HW, int C, int nblk, float* partial, float eps,
                           unsigned* tickets, float* scale, float* shift, zt_stream_t stream);
/* y = [outer_relu]([res +] [inner_relu](x*scale + shift)) */
int zt_norm_apply_nhwc(const void* x, int dt, int ldx, const float* scale, const float* shift, const void* res, int ldres,
                           void* y, int ldy, int N, int HW, int C, int inner_relu, int outer_relu, zt_stream_t stream);
/* backward of y = ReLU(BN_train(z)): stage 1 partial sums of dyh = dy*[bn>0] and dyh*zhat; generic partial reduction;
 * stage 2 dz = gamma*rstd*(dyh - mean(dyh) - zhat*mean(dyh*zhat)) with sums = [sum dyh (C) | sum dyh*zhat (C)];
 * eval_mode = 1: statistics are constants (running stats): dz = gamma*rstd*dyh (reference epochs >= 1, train.py:138).
 * zt_bn_bwd_reduce and zt_bn_bwd_apply require what zt_chan_stats_nhwc does: C % 4 == 0, C >= 4 (reduce: C <= 1024), every
 * ld % 4 == 0, HW > 0, 8-byte aligned dy / z / dz, non-NULL scale / shift / mean / rstd; reduce also nblk > 0. */
int zt_bn_bwd_reduce(const void* dy, int dt, int lddy, const void* z, int ldz, const float* scale, const float* shift,
                         const float* mean, const float* rstd, int HW, int C, int nblk, float* partial, zt_stream_t stream);
int zt_partial_reduce_f32(const float* partial, int nblk, int stride, int n, float* out, int accumulate, float* out2,
                          zt_stream_t stream);
/* terms[0..16] of the loss from the partials of zt_loss_s2_f32 (p1 [nb1][4]), zt_loss_half_f32 (p2 [nb2][10]) and zt_loss_full_f32
   (p3 [nb3][3]) in one launch; every term is summed exactly as zt_partial_reduce_f32 sums a column */
int zt_loss_terms_reduce_f32(const float* p1, int nb1, const float* p2, int nb2, const float* p3, int nb3, float* terms,
                             zt_stream_t stream);
/* one launch for a BatchNorm layer's backward sums: sums[0:2C] = column sums of partial [nblk][2][C]; dbeta += sums[0:C],
   dgamma += sums[C:2C] (torch BatchNorm2d backward, reference model.py:60-67 through autograd) */
int zt_bn_bwd_sums_f32(const float* partial, int nblk, int C, float* dbeta, float* dgamma, float* sums, zt_stream_t stream);
/* same for partials whose second half is sum g (z - mean) (zt_conv3x3_dgrad_bn_sums_bf16): multiplied by rstd on the way */
int zt_bn_bwd_sums_centered_f32(const float* partial, int nblk, int C, const float* rstd, float* dbeta, float* dgamma, float* sums,
                                zt_stream_t stream);
int zt_bn_bwd_apply(const void* dy, int dt, int lddy, const void* z, int ldz, const float* scale, const float* shift,
                        const float* mean, const float* rstd, const float* sums, void* dz, int lddz, int HW, int C,
                        int eval_mode, zt_stream_t stream);


/* ---- element-wise stages of Network.forward (model.py:144-203) and their backward (zt_glue.hip); planar [3][H][W], H,W even */
/* model.py:145-148, loss.py:25,51: x = inp+1e-4; (L11,L12) = pair_downsampler(x); (Lq11,Lq12) = pair_downsampler(inp+1e-9) */
int zt_prep_input_f32(const float* inp, float* x, float* L11, float* L12, float* Lq11, float* Lq12, int H, int W, zt_stream_t stream);
/* torch.cat([...],1) of up to four planar tensors into one nhwc buffer (remaining channels zero) (model.py:168,179,184,189) */
int zt_pack_nhwc(void* dst, int dt, int ld, long long HW, const float* s0, int c0, const float* s1, int c1, const float* s2, int c2,
                     const float* s3, int c3, zt_stream_t stream);
/* model.py:149-152 + loss.py:54: L2 = clamp(x-n,1e-4,1); L_pred1/2 = L11/12 - n11/12; (den1,den2) = pair_downsampler(L2) */
int zt_d1_tail_f32(const float* x, const float* n, const float* L11, const float* n11, const float* L12, const float* n12,
                   float* L2, float* Lp1, float* Lp2, float* den1, float* den2, int H, int W, zt_stream_t stream);
/* model.py:169-177,198-199 */
int zt_post_enh_f32(const float* x, const float* s2, const float* L2, const float* L11, const float* L12, float* s21, float* s22,
                    float* H2, float* H11, float* H12, float* H1, int H, int W, zt_stream_t stream);
/* model.py:179-192: (outA|outB) = clamp(cat[A,B] - r, 1e-4, 1), r planar 6ch */
int zt_clamp_sub6_f32(const float* A, const float* B, const float* r, float* outA, float* outB, long long HW, zt_stream_t stream);
/* Denoise_1 / Denoise_2 forward and its tail in one launch, bf16 throughput mode (zt_denoise.hip; model.py:15-44, 316, 335-337):
 *   out[c] = clamp(ref[c] - conv1x1(lrelu(conv3x3(lrelu(conv3x3(cat(s0..)))))) [c], 1e-4, 1),  c < cout
 * s0..s3: ngroups (1 or 4) planar fp32 [3][H][W] sources, concatenated in order and rounded to bf16 while staged; ref0 (channels
 * 0..2) / ref1 (channels 3..5, cout == 6 only): the planar fp32 tensors subtracted from, used in fp32.  Weights in the layout of
 * zt_repack_conv_weight_bf16: w1 [9][48][ldk1] (ldk1 = 8 or 16), w2 [9][48][48], w3 [1][16][48]; biases fp32.  out: planar fp32
 * [cout][H][W]; res (may be NULL): the residual before the subtraction, same shape.  The 48-channel activations stay on chip. */
int zt_denoise_fused_bf16(const float* s0, const float* s1, const float* s2, const float* s3, int ngroups, const float* ref0,
                          const float* ref1, const void* w1, int ldk1, const float* b1, const void* w2, const float* b2,
                          const void* w3, const float* b3, int cout, float* out, float* res, int H, int W, zt_stream_t stream);
/* its backward into the nhwc gradient of r */
int zt_clamp_sub6_bwd(const float* A, const float* B, const float* r, const float* gA, const float* gB, void* dr, int dt, int ld,
                          long long HW, zt_stream_t stream);
/* all gradient paths into s2 (H2, H11/H12, pair_downsampler, Denoise_2 inputs, direct loss terms) -> Enhancer output-layer gradient (nhwc) */
int zt_post_enh_bwd(const float* x, const float* s2, const float* L11, const float* L12, const float* s21, const float* s22,
                        const float* dIn5, const float* dH2x, const float* dIn3, const float* dIn4, const float* ds2_direct,
                        void* dO, int dt, int ld, float* ds2_total, int H, int W, zt_stream_t stream);
/* gradients entering the three Denoise_1 invocations (nhwc) */
int zt_d1_bwd_prep(const float* x, const float* n, const float* dLp1, const float* dLp2, const float* dden1,
                       const float* dden2, void* dn, void* dn11, void* dn12, int dt, int ld, int H, int W, zt_stream_t stream);
/* ReLU backward on nhwc buffers: out = g * [a > 0] */
int zt_relu_mask_nhwc(const void* g, int dt, int ldg, const void* a, int lda, void* out, int ldo, long long npix, int C, zt_stream_t stream);
/* element-wise helpers of Finetunemodel.forward (model.py:313-316,327-328): mode 0 a+p0; 1 clamp(a-b,p0,p1); 2 clamp(a/b,p0,p1) */
int zt_ew_f32(const float* a, const float* b, float* out, int mode, float p0, float p1, long long n, zt_stream_t stream);
/* utils.py:228 overlap_tensor = 0.5*warped + 0.5*img2: out = alpha*a + beta*b */
int zt_axpby_f32(const float* a, const float* b, float* out, float alpha, float beta, long long n, zt_stream_t stream);
int zt_add3_f32(const float* a, const float* b, const float* c, float* out, long long n, zt_stream_t stream);

/* ---- LossFunction.forward (loss.py:12-78) + gradient w.r.t. its inputs (zt_loss.hip) ------------------------------- */
int zt_plane_sums_f32(const float* x, int C, long long HW, int nblk, float* partial, zt_stream_t stream);
/* loss.py:26-37: scal[0..2] = clamp(enhancement_factor,1,25), scal[3..5] = 0.7^-ef / ef */
int zt_loss_scalars_f32(const float* partial, int nblk, long long HW, int is_WB, float* scal, zt_stream_t stream);
/* the same scalars by one lane straight from global memory (slow; the tests' reference for zt_loss_scalars_f32) */
int zt_loss_scalars_serial_f32(const float* partial, int nblk, long long HW, int is_WB, float* scal, zt_stream_t stream);
/* loss.py:46-49 (700 MSE, 1000 MSE, 5 SmoothLoss, 1600 L_TV): partial[block][4] + direct d/ds2.  fast_exp: 1 = hardware exponential for
 * the bilateral weights (bf16 throughput mode), 0 = libm expf (fp32 parity mode) */
int zt_loss_s2_f32(const float* L2, const float* s2, const float* Y, const float* scal, int H, int W, float* ds2, float* partial,
                   int fast_exp, zt_stream_t stream);
/* loss.py:51-62, 68-73: partial[block][10] = res1_a..d, res2_a..d, inter_a, inter_b; direct gradients; u1/u2 = (1-m)*de (to be LocalMean-adjointed) */
int zt_loss_half_f32(const float* Lq11, const float* Lq12, const float* Lp1, const float* Lp2, const float* den1, const float* den2,
                     const float* H3p, const float* H4p, const float* H11, const float* s21, const float* H12, const float* s22,
                     const float* H3d1, const float* H3d2, const float* mask, const float* LM1, const float* LM2, float* dLp1,
                     float* dLp2, float* dden1, float* dden2, float* dH3p, float* dH4p, float* dH3d1, float* dH3d2, float* u1,
                     float* u2, long long hw, float* partial, zt_stream_t stream);
/* loss.py:64, 66, 75-77: partial[block][3] = color, ill, var; dH3_blur, ds3, gV = d/dV(H2) (= -d/dV(H3-H2)) */
int zt_loss_full_f32(const float* H2b, const float* H3b, const float* s2, const float* s3, const float* VH2, const float* VN,
                     float* dH3b, float* ds3, float* gV, long long n, float* partial, zt_stream_t stream);


/* ---- RAFT / update_cache specific kernels (zt_raft.hip) ------------------------------------------------------------ */
/* F.interpolate(bilinear, align_corners=False) * mul on planar tensors (model.py:226-227,231), ATen CPU rounding sequence */
int zt_resize_bilinear_f32(const float* src, float* dst, int C, int H, int W, int h, int w, float mul, zt_stream_t stream);
/* (x).to(uint8) + per-channel histogram + torchvision==0.18.1 equalize LUT (model.py:234); q: uint8 [C][hw], hist/lut: int32 [C][256] */
int zt_equalize_prepare_u8(const float* src, unsigned char* q, int* hist, int* lut, int C, int hw, zt_stream_t stream);
/* raft.py:80-83,132-138: centred replicate pad to multiples of 8, 2*(x/255)-1; frame 1 float, frame 2 = lut[q2]; dst nhwc [2][Hp][Wp][ld] (dt: 0 fp32, 1 bf16) */
int zt_raft_pack_input(const float* img1, const unsigned char* q2, const int* lut, void* dst, int dt, int ld, int h, int w, int Hp, int Wp, zt_stream_t stream);
/* the same head for two float frames in [0,255] (RAFT.forward called directly, raft.py:77-83) */
int zt_raft_pack_pair(const float* img1, const float* img2, void* dst, int dt, int ld, int h, int w, int Hp, int Wp, zt_stream_t stream);
/* corr.py:25-27 one pyramid level: avg_pool2d(2,2) of [npx][hin][win] (row pitch ldin) -> [npx][hin/2][win/2] */
int zt_corr_pool_f32(const float* src, float* dst, int npx, int hin, int win, int ldin, zt_stream_t stream);
/* corr.py:13-27, 52-60 in one pass, bf16 feature maps: c0[m][y2*w + x2] = alpha * <f1[m], f2[y2*w + x2]> (fp32 [npx][ld0]) and the
 * three avg_pool2d(2,2) levels c1 [npx][h/2 * w/2], c2, c3 (floor sizes), each from the rounded level below.  f1 / f2: nhwc bf16
 * [npx][ld >= 256] (256 channels).  Replaces zt_conv2d_nhwc_bf16 (as a 1x1 GEMM) + 3 x zt_corr_pool_f32. */
int zt_corr_volume_pyramid_bf16(const void* f1, int ld1, const void* f2, int ld2, int h, int w, float alpha, float* c0, int ld0, float* c1,
                                float* c2, float* c3, zt_stream_t stream);
/* corr.py:29-50 (the seam of alt_cuda_corr.forward, corr.py:86): coords [npx][2] -> out nhwc [npx][ldo>=324], channel = lvl*81 + i*9 + j */
int zt_corr_lookup(const float* l0, const float* l1, const float* l2, const float* l3, int h, int w, int ld0, const float* coords,
                   void* out, int dt, int ldo, int npx, zt_stream_t stream);
/* The same lookup with the flow bookkeeping of the PREVIOUS refinement iteration folded in (raft.py:112-126: `coords1 = coords1 +
 * delta_flow` feeds the next iteration's `corr_fn(coords1)`): looks up at coords + delta (delta [npx][ldd] fp32, may be NULL) and
 * records coords_out = coords + delta (a different buffer than coords), flow = coords_out - grid into f4 (fp32 [npx][ldf4]) and the
 * nhwc destinations fhx / fin of storage type dt (each may be NULL) -- one launch less per iteration than lookup + zt_raft_flow_step,
 * bit-identical values. */
int zt_corr_lookup_step(const float* l0, const float* l1, const float* l2, const float* l3, int h, int w, int ld0, const float* coords,
                        void* out, int dt, int ldo, int npx, const float* delta, int ldd, float* coords_out, float* f4, int ldf4,
                        void* fhx, int ldfhx, void* fin, int ldfin, zt_stream_t stream);
/* ---- on-the-fly correlation (zt_corr_alt.hip; corr.py:63-91 AlternateCorrBlock): the same 4 x 81 window without the volume.
 * avg_pool2d of the volume == correlation with the equally pooled fmap2, so level l of query n is alpha * <f1[n], P_l[y][x]>.
 * zt_fmap_pyramid: f2 nhwc [h*w][ld2 >= 256] of storage type dt (256 channels) -> P_1..P_3, fp32 nhwc [hl*wl][256] (floor sizes),
 * P_{l+1} = (((a + b) + c) + d) * 0.25f of the rounded level below, one launch. */
int zt_fmap_pyramid(const void* f2, int dt, int ld2, int h, int w, float* p1, float* p2, float* p3, zt_stream_t stream);
/* zt_corr_lookup / zt_corr_lookup_step with the taps computed from the feature maps: f1 [npx][ld1] and p0 = fmap2 [npx][ld0] of
 * storage type dt_f (pitches >= 256, multiples of 8), p1..p3 from zt_fmap_pyramid.  From the window coordinate to the output the
 * arithmetic is zt_corr_lookup's, so the two differ only by the summation order of the dot products; out / dt / ldo and the flow
 * bookkeeping follow zt_corr_lookup_step (channels >= 324 are never written).  npx == h * w; h, w <= 4096. */
int zt_corr_alt_lookup(const void* f1, int ld1, const void* p0, int ld0, int dt_f, const float* p1, const float* p2, const float* p3,
                       int h, int w, float alpha, const float* coords, void* out, int dt, int ldo, int npx, zt_stream_t stream);
int zt_corr_alt_lookup_step(const void* f1, int ld1, const void* p0, int ld0, int dt_f, const float* p1, const float* p2, const float* p3,
                            int h, int w, float alpha, const float* coords, void* out, int dt, int ldo, int npx, const float* delta,
                            int ldd, float* coords_out, float* f4, int ldf4, void* fhx, int ldfhx, void* fin, int ldfin,
                            zt_stream_t stream);
/* update.py:42-45: rh = r*h with zr = [z|r]; update.py:47: h = (1-z)h + z q */
int zt_gru_rh(const void* zr, int dt, int ldzr, const void* hbuf, int ldh, void* rh, int ldrh, int C, int npx, zt_stream_t stream);
int zt_gru_update(const void* zr, int dt, int ldzr, const void* q, int ldq, void* hbuf, int ldh, int C, int npx, zt_stream_t stream);
/* raft.py:57-62,112-120: coords grid; coords1 += delta (may be NULL), flow = coords1 - coords0 written to f4 (fp32) and to up to two nhwc destinations of storage type dt */
int zt_raft_coords_init_f32(float* coords, int h, int w, zt_stream_t stream);
int zt_raft_flow_step(float* coords1, const float* delta, int ldd, int h, int w, float* f4, int ldf4, void* fhx, int ldfhx, void* fin, int ldfin, int dt, zt_stream_t stream);
/* raft.py:64-75 upsample_flow: flow nhwc (ldf), mask nhwc [npx][576] -> planar [2][8h][8w]; optional planar flow_low [2][h][w] */
int zt_convex_upsample_f32(const float* f4, int ldf, const float* mask, int ldm, float* up, float* flow_low, int h, int w, zt_stream_t stream);


/* ---- optimizer step (zt_optim.hip): nn.utils.clip_grad_norm_(params, max_norm) + torch.optim.Adam.step (train.py:130-131)
 * over one flat bucket.  g is multiplied by gscale first (1/world_size after the data-parallel all-reduce).  partial: nblk floats
 * of workspace.  max_norm <= 0 disables clipping.  gnorm_out (optional): the pre-clip global norm. */
int zt_clip_adam_f32(float* p, const float* g, float* m, float* v, long long n, float* partial, int nblk, float gscale,
                     float max_norm, float lr, float beta1, float beta2, float eps, float weight_decay, long long step,
                     float* gnorm_out, zt_stream_t stream);


/* y[i] += alpha[0] * x[i]: `loss.backward()` (train.py:129) hands the step's parameter gradients (already computed next to the
 * loss by the fused plan) to the optimizer's flat bucket, scaled by the upstream gradient that autograd holds on the device. */
int zt_axpy_dev_f32(float* y, const float* x, const float* alpha, long long n, zt_stream_t stream);


/* ---- RAFT encoder stem in bf16 mode (zt_stem.hip): conv 7x7 / stride 2 / pad 3, 3 -> 64 (extractor.py:120, 168-170).
 * x: nhwc [N][H][W][8] bf16, channels 0..2 valid and 3..7 ZERO (as zt_raft_pack_input / zt_raft_pack_pair write them);
 * w: zt_repack_stem_weight_bf16 of the torch weight [64][3][7][7] -> [7][64][64] bf16; y: nhwc [N][H/2][W/2][ldy >= 64] bf16
 * = conv + bias, then ReLU when relu != 0 (context encoder: the frozen BatchNorm `norm1` folded into w / bias by the caller, so
 * relu(norm1(conv1(x))) of extractor.py:168-170 is this one launch; the feature encoder's InstanceNorm stays a separate pass). */
int zt_repack_stem_weight_bf16(const float* src, void* dst, zt_stream_t stream);
int zt_raft_stem_conv_bf16(const void* x, int N, int H, int W, const void* w, const float* bias, void* y, int ldy, int relu,
                           zt_stream_t stream);


/* ---- output side (zt_io.hip): predict.py:57-61 save_images and evals.py:83-85 PSNR on the device -------------------------
 * zt_quantize_u8_hwc: planar fp32 [3][H][W] in [0,1] -> interleaved uint8 [H][W][3] (what PIL / cv2 write);
 *   mode 0 = clip(x*255, 0, 255) truncated (predict.py / train.py save_images), mode 1 = np.round(x*255) (evals.py:83-84).
 * zt_sqdiff_u8_f32: out[0] = sum_i (round(a_i*255) - round(b_i*255))^2, exact 64-bit integer; PSNR = 10 log10(255^2 n / out).
 *   partial: nblk x 8 bytes of workspace. */
int zt_quantize_u8_hwc(const float* src, unsigned char* dst, int H, int W, int mode, zt_stream_t stream);
int zt_sqdiff_u8_f32(const float* a, const float* b, long long n, unsigned long long* partial, int nblk, unsigned long long* out,
                     zt_stream_t stream);

/* Evaluation metrics of evals.py (zt_metrics.hip).
 * zt_ssim_u8_f32: out[0] = skimage structural_similarity(round(a*255), round(b*255), channel_axis=2, data_range=255) of two planar
 *   fp32 [3][H][W] frames (evals.py:87): 7x7 uniform window, sample covariance, 3-pixel border cropped, mean over the pixels of a
 *   channel, then over the channels.  Window sums are exact integers, the rest is fp64 in a fixed order (same input, same bits).
 *   partial: npartial x 8 bytes of workspace, npartial >= 3 * ceil((H-6)/32) * ceil((W-6)/64).  H < 7 or W < 7: ZT_EINVAL.
 * zt_match_histograms_f32: out = skimage exposure.match_histograms(src, tmpl) with channel_axis=None (evals.py:100-103: the values
 *   of all channels pooled into ONE distribution), bit for bit: out_i = float(interp(cnt_i / n, tq, tv)) in fp64, cnt_i = number of
 *   source values <= src_i (-0.0 == +0.0), tq / tv = cumulative share / value of the occupied levels of round(tmpl*255).
 *   src, out: n finite fp32 values, 16-byte aligned; tmpl: m fp32 values k/255 (a ToTensor image), any m >= 1.
 *   scratch: 16-byte aligned workspace of at least 8 * ((n+3) & ~3) + 1024 * ceil(n/4096) + 8192 bytes (two key buffers of the
 *   radix sort, its digit counts, the template table). */
int zt_ssim_u8_f32(const float* a, const float* b, int H, int W, double* partial, int npartial, double* out, zt_stream_t stream);
int zt_match_histograms_f32(const float* src, long long n, const float* tmpl, long long m, float* out, void* scratch,
                            size_t scratch_bytes, zt_stream_t stream);


/* ---- LPIPS (VGG16, lpips 0.1) of evals.py:73-80, 92-98 (zt_lpips.hip) ------------------------------------------------------
 * zt_conv3x3_wide_bf16: y = [relu](conv3x3(x) + bias), stride 1, pad 1, for wide layers: x bf16 nhwc [N][H][W][ldx], w bf16
 *   [9][CoutP][ldk] (zt_repack_conv_weight_bf16), y bf16 nhwc [N][H][W][ldy], fp32 accumulation.  Cin a multiple of 64, Cout a
 *   multiple of 128 (anything else: 1001), any H, W >= 1; ldx, ldk, ldy multiples of 8, pointers 16-byte aligned (bias too),
 *   N*H*W*ldx < 2^31.  A workgroup owns 8 x 16 pixels x 128 couts (VGG16's conv2_1 .. conv5_3; the 3 -> 64 and 64 -> 64 layers in
 *   front of them are zt_conv2d_nhwc_bf16's).
 * zt_lpips_prep: planar fp32 [3][H][W] in [0,1] -> nhwc [H][W][8] (dt 0 fp32 / 1 bf16), channel c = ((a - 0.5) * 2 - shift_c) /
 *   scale_c with lpips' ScalingLayer constants shift = (-.030, -.088, -.188), scale = (.458, .448, .450); channels 3..7 = 0.
 * zt_maxpool2_nhwc: 2x2 max pool, stride 2, floor (nn.MaxPool2d(2, 2)): [N][H][W][ldx] -> [N][H/2][W/2][ldy], first C channels,
 *   C a multiple of 4 (fp32) / 8 (bf16), as are ldx and ldy.
 * zt_lpips_layer: out[0] = mean over the npix pixels of sum_c w[c] (fa_c / (|fa| + 1e-10) - fb_c / (|fb| + 1e-10))^2, |f| the
 *   channel norm of the pixel (lpips normalize_tensor, the 1x1 `lin` layer, spatial_average), for two nhwc maps of C in {64, 128,
 *   256, 512} channels (strides lda, ldb).  fp32 per pixel, fp64 sums in a fixed order (same input, same bits).
 *   partial: npartial x 8 bytes of workspace (npartial >= 1; 2048 is never exceeded). */
int zt_conv3x3_wide_bf16(const void* x, int ldx, int N, int H, int W, int Cin, const void* w, int CoutP, int ldk, const float* bias,
                         void* y, int ldy, int Cout, int relu, zt_stream_t stream);
int zt_lpips_prep(const float* src, void* dst, int dt, int H, int W, zt_stream_t stream);
int zt_maxpool2_nhwc(const void* x, int dt, int ldx, int N, int H, int W, int C, void* y, int ldy, zt_stream_t stream);
int zt_lpips_layer(const void* fa, int lda, const void* fb, int ldb, int dt, long long npix, int C, const float* w, double* partial,
                   int npartial, double* out, zt_stream_t stream);


/* ---- input side (zt_ingest.hip): dataloader/multi_read_data.py:127-132 on the device -------------------------------------
 * The loader workers decode to interleaved uint8 RGB [H][W][3]; `im.resize((1920, 1080))` (PIL default filter for RGB = BICUBIC,
 * Pillow's 8-bit two-pass resampler) and `transforms.ToTensor()` run here, bit-identical to the host libraries.
 * zt_resample_u8_hwc: ONE pass of the resampler along `axis` (1 = horizontal: [Hi][Wi][3] -> [Hi][Wo][3], Ho == Hi;
 *   0 = vertical: [Hi][Wi][3] -> [Ho][Wi][3], Wo == Wi, 3*Wi % 4 == 0): out = clip8((2^21 + sum_k src[min + k] * coef[o][k]) >> 22);
 *   coef: int32 [out][ksize] = round(w * 2^22), bounds: int32 [out][2] = (first source index, tap count) -- device arrays, computed
 *   by the host exactly as Pillow's precompute_coeffs / normalize_coeffs_8bpc do.  Horizontal first, then vertical (Resample.c).
 * zt_u8hwc_to_planar_f32: uint8 [H][W][3] -> planar fp32 [3][H][W], value lut256[byte] (lut256[k] = float(k) / 255.f: ToTensor). */
int zt_resample_u8_hwc(const unsigned char* src, unsigned char* dst, int Hi, int Wi, int Ho, int Wo, int axis, const int* coef,
                       const int* bounds, int ksize, zt_stream_t stream);
int zt_u8hwc_to_planar_f32(const unsigned char* src, float* dst, int H, int W, const float* lut256, zt_stream_t stream);

/* ---- float resize (zt_resample.hip): train.py / predict.py --y4m_size, DESIGN 8g ----------------------------------------------
 * zt_resample_planar_f32: ONE pass of Pillow's ImagingResample for mode F over planar fp32 along `axis` (1 = rows: src [C][Hi][Wi]
 *   -> dst [C][Hi][No]; 0 = columns: src [C][Hi][Wi] -> dst [C][No][Wi]):
 *   ss = 0.0; for t < count: ss = ss + (double)src[first + t] * coef[o][t]; dst = (float)ss -- the multiply and the add are separate
 *   double operations in tap order.  clamp01 = 1 stores min(max((float)ss, 0), 1) (bicubic overshoots; the model's input is [0, 1]).
 *   coef: double [No][ksize], bounds: int32 [No][2] = (first source index, tap count <= ksize) -- device arrays, the weights of
 *   Pillow's precompute_coeffs before any integer normalisation (zero-tig_amd/ingest.py:pil_bicubic_tables_f64).  Nothing is rounded
 *   to 8 bits between the passes, so it takes the result of zt_yuv16_to_planar_f32 as well.  Rows first, then columns (Resample.c).
 *   Null pointers, sizes <= 0, axis outside {0, 1}, ksize < 1, src == dst: ZT_EINVAL. */
int zt_resample_planar_f32(const float* src, float* dst, int C, int Hi, int Wi, int No, int axis, const double* coef, const int* bounds,
                           int ksize, int clamp01, zt_stream_t stream);


/* ---- raw video frames (zt_yuv.hip): 8-bit planar Y'CbCr <-> RGB with chroma resampling, predict.py --y4m_in / --y4m_out -------
 * A frame is the YUV4MPEG2 payload: plane Y [H][W], then U, then V ([H/2][W/2] for ss 420, [H][W/2] for 422, [H][W] for 444),
 * contiguous uint8.  ss in {420, 422, 444}; siting 0 = chroma centred between the luma columns it covers (C420jpeg; the only value
 * for 444), 1 = horizontally co-sited with the left column (C420, C420mpeg2, C420paldv, C422); vertical siting of 420 is always
 * centred.  W even for 420 / 422, H even for 420; anything else: ZT_EINVAL.  Integer arithmetic, S = 14, bit-exact.
 * coef: HOST arrays of int32 (read during the call), round(c * 2^14) with matrix and range folded in (zero-tig_amd/y4m.py):
 *   decode: 6 values yo, CY, CRV, CGU, CGV, CBU; chroma upsampled to 16x integers U16 / V16 (horizontal weights (3, 1) centre or
 *     4 / (2, 2) left, vertical (3, 1) for 420, clamped at the edges); y = 16 CY (Y - yo), u = U16 - 2048, v = V16 - 2048;
 *     R = clip8((y + CRV v + 2^17) >> 18), G = clip8((y - CGU u - CGV v + 2^17) >> 18), B = clip8((y + CBU u + 2^17) >> 18).
 *   encode: 10 values yo, CYR, CYG, CYB, CUR, CUG, CUB, CVR, CVG, CVB; Y = yo + ((CYR R + CYG G + CYB B + 2^13) >> 14);
 *     U = 128 + ((CUR Rs + CUG Gs + CUB Bs + 2^(13+sh)) >> (14+sh)) over the RGB sums of the footprint (444: the pixel, sh 0; centre:
 *     the two columns, sh 1; left: [1, 2, 1] over 2c-1, 2c, 2c+1 with -1 clamped to 0, sh 2; 420: both rows, sh + 1); clipped.
 * zt_yuv_to_rgb_u8: payload -> uint8 [H][W][3] (what zt_resample_u8_hwc takes).
 * zt_yuv_to_planar_f32: payload -> planar fp32 [3][H][W], value lut256[level] (lut256[k] = float(k) / 255.f); equal to
 *   zt_yuv_to_rgb_u8 followed by zt_u8hwc_to_planar_f32 bit for bit, without the RGB intermediate and for any H * W.
 * zt_rgb_f32_to_yuv: planar fp32 [3][H][W] -> payload; levels as zt_quantize_u8_hwc mode 0 makes them, converted in the same pass.
 * With W % 8 == 0 and 16-byte aligned pointers every access is 4 to 16 bytes wide; otherwise byte accesses, same result. */
int zt_yuv_to_rgb_u8(const unsigned char* src, unsigned char* dst, int H, int W, int ss, int siting, const int* coef,
                     zt_stream_t stream);
int zt_yuv_to_planar_f32(const unsigned char* src, float* dst, int H, int W, int ss, int siting, const int* coef, const float* lut256,
                         zt_stream_t stream);
int zt_rgb_f32_to_yuv(const float* src, unsigned char* dst, int H, int W, int ss, int siting, const int* coef, zt_stream_t stream);

/* ---- high-bit-depth raw video frames (zt_yuv.hip, the grid in zt_scene.hip): planar Y'CbCr of depth B in {9 .. 16} <-> RGB, DESIGN 8f
 * The payload has the plane shapes above as little-endian uint16, the value in the low B bits; a sample above m = 2^B - 1 is read
 * as m.  ss, siting, the tap tables and the footprints are those of the 8-bit entry points.  coef: HOST pointer to 64-bit integers,
 * round(c * 2^20) with matrix, range and depth folded in (zero-tig_amd/y4m.py); every entry must fit 32 bits.  mid = 2^(B-1).
 *   decode: 6 values yo, CY, CRV, CGU, CGV, CBU; y = 16 CY (min(Y, m) - yo), u = U16 - 16 mid, v = V16 - 16 mid (chroma 16x as above),
 *     R16 = clip16((y + CRV v + 2^23) >> 24), G16 = clip16((y - CGU u - CGV v + 2^23) >> 24), B16 = clip16((y + CBU u + 2^23) >> 24);
 *     the value written is float(L16) / 65535.f.
 *   encode: 10 values yo, CYR, CYG, CYB, CUR, CUG, CUB, CVR, CVG, CVB; L16 = x > 0 ? (x < 1 ? (int)(x * 65535.f + 0.5f) : 65535) : 0
 *     (NaN -> 0); Y = yo + ((CYR R + CYG G + CYB B + 2^19) >> 20); U = mid + ((CUR Rs + CUG Gs + CUB Bs + 2^(19+sh)) >> (20+sh)), V
 *     alike, over the footprint sums of the 16-bit levels; every plane clipped to 0..m.
 * zt_luma_grid_u16: zt_luma_grid_u8 (below) of the plane min(y, m) >> (B - 8), bit for bit; yo8 is the 8-bit offset (16 or 0).
 * With W % 8 == 0 (the grid: W % 16 == 0) and 16-byte aligned pointers every access is 8 or 16 bytes wide; otherwise 2-byte
 * accesses, same result.  Any other depth, and the size / siting combinations the 8-bit entry points reject: ZT_EINVAL. */
int zt_yuv16_to_planar_f32(const uint16_t* src, float* dst, int H, int W, int ss, int siting, int depth, const long long* coef,
                           zt_stream_t stream);
int zt_rgb_f32_to_yuv16(const float* src, uint16_t* dst, int H, int W, int ss, int siting, int depth, const long long* coef,
                        zt_stream_t stream);
int zt_luma_grid_u16(const uint16_t* y, int H, int W, int depth, int yo8, unsigned int* grid /* [gh*gw] */, zt_stream_t stream);

/* ---- scene cuts in a raw video stream (zt_scene.hip): predict.py --y4m_scene_cut, zero-tig_amd/scenecut.py, DESIGN 8e ------------
 * zt_luma_grid_u8: the luma plane y [H][W] (the first H * W bytes of a payload) in 16 x 16 cells, gh = ceil(H / 16) rows of
 *   gw = ceil(W / 16), edge cells holding the pixels that exist: grid[i * gw + j] = sum over the cell of max(y - yo, 0), at most
 *   256 * 255.  yo in 0..255 (16 for limited range, 0 for full range).  16-byte loads when W % 16 == 0 and y is 16-byte aligned,
 *   byte loads otherwise, same result.
 * zt_grid_sad_u32: out2[0] = sum |a[k] - b[k]|, out2[1] = sum (a[k] + b[k]) over k < n, 64-bit sums; out2 is overwritten, the
 *   caller zeroes nothing.
 * Integer and deterministic (no atomics).  H, W or n <= 0, yo outside 0..255: ZT_EINVAL. */
int zt_luma_grid_u8(const unsigned char* y, int H, int W, int yo, unsigned int* grid /* [gh*gw] */, zt_stream_t stream);
int zt_grid_sad_u32(const unsigned int* a, const unsigned int* b, int n, unsigned long long* out2 /* sad, tot */, zt_stream_t stream);

/* ---- plane metrics of a raw video stream (zt_planes.hip): evals.py --y4m_in / --y4m_gt, DESIGN 8h ----------------------------------
 * Samples as in the zt_yuv blocks: depth 8 = uint8; depth B in {9, 10, 12, 14, 16} = little-endian uint16 (2-byte aligned), a
 * sample above m = 2^B - 1 is read as m.  Any other depth: ZT_EINVAL.  Results go to device memory; nothing synchronises.
 * zt_yuv_sse: a, b = two payloads of ONE layout (planes Y, U, V with the shapes above for ss in {420, 422, 444}; W even for 420 /
 *   422, H even for 420, anything else ZT_EINVAL); out3[p] = sum over plane p of (a - b)^2 as exact 64-bit integers, in one pass
 *   over both payloads.  A squared difference is below 2^32, so a plane of fewer than 2^31 samples cannot wrap 64 bits: a frame of
 *   H * W >= 2^31 is ZT_EINVAL.  PSNR_p = 10 log10(m^2 n_p / out3[p]).  16-byte loads when W % 8 == 0 (W % 16 == 0 at 8 bits) and
 *   both pointers are 16-byte aligned, sample-wide loads otherwise, same result.  partial: 3 * nblk x 8 bytes of workspace,
 *   1 <= nblk <= 4096 workgroups share the samples.
 * zt_ssim_plane: out[0] = skimage structural_similarity(a, b, data_range=m) of two contiguous planes [H][W] (a plane pointer inside
 *   a payload is fine): the definition of zt_ssim_u8_f32 for one channel -- 7x7 uniform window, sample covariance (49/48),
 *   C1 = (0.01 m)^2, C2 = (0.03 m)^2, 3-sample border cropped, mean over the windows inside the plane.  The five window sums are
 *   exact integers (32-bit up to 12 bits, 49 * 4095^2 < 2^30; 64-bit for 14 and 16 bits), the rest is fp64 in a fixed order.
 *   16-byte loads when W % 8 == 0 (W % 16 == 0 at 8 bits) and both pointers are 16-byte aligned, sample-wide loads otherwise, same
 *   result.  partial: npartial x 8 bytes of workspace, npartial >= ceil((H-6)/TH) * ceil((W-6)/64), TH = 32 rows up to 12 bits and 16
 *   rows for 14 and 16 bits (ceil((H-6)/16) * ceil((W-6)/64) is enough at every depth).  H < 7 or W < 7: ZT_EINVAL.
 * Integer where stated and deterministic (no atomics, fixed reduction order): same input, same bits. */
int zt_yuv_sse(const void* a, const void* b, int H, int W, int ss, int depth, unsigned long long* partial, int nblk,
               unsigned long long* out3 /* Y, U, V */, zt_stream_t stream);
int zt_ssim_plane(const void* a, const void* b, int H, int W, int depth, double* partial, int npartial, double* out,
                  zt_stream_t stream);

/* ---- temporal consistency of a video (zt_temporal.hip): evals.py --tc 1, zero-tig_amd/temporal.py, DESIGN 8i -------------------------
 * zt_warp_error_f32: one pass over a frame pair.  cur, prev: planar [3][H][W]; fb, ff: planar [2][Hf][Wf], the backward flow
 *   (cur -> prev) and the forward flow (prev -> cur) in pixels, the flow of pixel (y, x) at [(y + oy) * Wf + (x + ox)] (RAFT's
 *   centred padding: oy = (Hf - H) / 2, ox = (Wf - W) / 2).  Per pixel, in IEEE fp32 with one rounding per operation (no fused
 *   multiply-add), (u, v) = fb at the pixel:
 *     px = (float)x + u, py = (float)y + v; inside = 0 <= px <= W - 1 && 0 <= py <= H - 1 (false for NaN); outside: px = py = 0
 *     x0 = floor(px), ax = px - x0, x1 = min(x0 + 1, W - 1), the same in y
 *     bil(p) = (1 - ay) * ((1 - ax) * p[y0][x0] + ax * p[y0][x1]) + ay * ((1 - ax) * p[y1][x0] + ax * p[y1][x1])
 *     fu, fv = bil(ff) (through the same offset); su = u + fu, sv = v + fv
 *     valid = inside && su * su + sv * sv <= 0.01f * ((u * u + v * v) + (fu * fu + fv * fv)) + 0.5f
 *     d_c = cur_c - bil(prev_c), e = (d_0^2 + d_1^2) + d_2^2;  s_c = cur_c - prev_c, e0 = (s_0^2 + s_1^2) + s_2^2
 *     b = | ((cur_0 + cur_1) + cur_2) - ((prev_0 + prev_1) + prev_2) |
 *   out_n[0] = number of valid pixels (exact); out3 = { sum over valid pixels of e, sum over all pixels of e0, sum over all pixels
 *   of b }, each term converted to double before it is added.  ws: 32 * nblk bytes of workspace (8-byte aligned), 1 <= nblk <= 4096
 *   workgroups share the 256 x 4 pixel tiles; one workgroup then adds the per-block partials in index order.  No atomics: the same
 *   input with the same nblk gives the same bits.  16-byte loads of the coalesced part where W % 4 == 0 and the pointers are
 *   16-byte aligned (the flows also need Wf % 4 == 0 and ox % 4 == 0), value-wide loads otherwise, same result.
 *   H, W < 1, oy, ox < 0, Hf < H + oy, Wf < W + ox, Hf * Wf >= 2^31, nblk outside 1..4096, a NULL or misaligned pointer: ZT_EINVAL. */
int zt_warp_error_f32(const float* cur, const float* prev, const float* fb, const float* ff, int H, int W, int Hf, int Wf, int oy,
                      int ox, void* ws, int nblk, long long* out_n, double* out3, zt_stream_t stream);

/* ---- looking at the flows of --tc 1 (zt_flowviz.hip): evals.py --tc_viz / --tc_flo_dir, utils/flow_viz.py, DESIGN 8k ------------------
 * Flows: planar [2][Hf][Wf] fp32, the window (oy, ox, H, W) as in zt_warp_error_f32.  IEEE fp32, one rounding per operation, no fused
 * multiply-add, no library transcendental (sqrtf and / are correctly rounded): a numpy float32 restatement gives the same bits.
 * zt_flow_radmax_f32: out1[0] = the largest sqrtf(u * u + v * v) over the window of fa and, when not NULL, fb, over the pixels whose
 *   u * u + v * v is finite (so both components are finite, and the result always is); 0 when there is none.  ws: 4 * nblk bytes,
 *   1 <= nblk <= 4096.  A maximum does not depend on the order: no atomics, same input, same bits.
 * zt_flow_to_rgb: the colour wheel of Baker et al. 2007 at the scale R = rad_dev[0] (a float on the device):
 *     den = R + 1e-5f; un = u / den, vn = v / den; r2 = un * un + vn * vn; rad = sqrtf(r2); r2 not finite (NaN included): black
 *     a = atan2(-vn, -un) by a fixed sequence of fp32 operations (zt_flowviz.hip; the sign of a zero counts)
 *     fk = (a / pi + 1) * 27 (pi in float32, so that +-pi give exactly 0 and 54); k0 = min(max((int)floorf(fk), 0), 54); f = fk - floorf(fk); k1 = k0 + 1, 55 -> 0
 *     col = (1 - f) * (wheel[k0] / 255) + f * (wheel[k1] / 255); rad <= 1: col = 1 - rad * (1 - col), otherwise col = col * 0.75f
 *     level = (int)floorf(255 * col) clamped to 0..255
 *   out_u8: uint8 [H][W][3] (NULL: not written); out_f32: planar fp32 [3][H][W] of level / 255.f (NULL: not written); at least one.
 *   bgr = 1: the channels in the order blue, green, red.
 * zt_flow_wheel: pure host query, the 55 x 3 levels of the wheel.
 * zt_tc_viz_f32: out = planar fp32 [3][2H][2W], one picture of four panels of the frame pair of zt_warp_error_f32, whose per-pixel
 *   u, v, inside, ax, ay, fu, fv, valid, e it computes with the same operations: top left / top right the wheel colour of fb / ff at
 *   the pixel (both at rad_dev[0]); bottom left cur where valid, (1, 0, 1) where the pixel lands outside the frame, (0, 1, 1) where it
 *   fails the forward-backward test; bottom right min(1, sqrtf(e / 3) * gain) where valid, 0 elsewhere.  prev = NULL (no partner;
 *   fb, ff, rad_dev are not read and may be NULL): white, white, cur, black.  gain: finite, >= 0.
 * zt_flow_pack_hwc_f32: the window as interleaved [H][W][2], the payload of a Middlebury .flo file.
 * 16-byte loads / stores where W % 4 == 0 and the pointer is 16-byte aligned (flows: also Wf % 4 == 0 and ox % 4 == 0; the uint8
 * output: 32-bit stores, 4-byte aligned), value by value otherwise, same result.  H, W < 1, oy, ox < 0, Hf < H + oy, Wf < W + ox,
 * Hf * Wf >= 2^31, H > 262140, a NULL or misaligned pointer: ZT_EINVAL. */
int zt_flow_radmax_f32(const float* fa, const float* fb /* or NULL */, int H, int W, int Hf, int Wf, int oy, int ox, float* ws,
                       int nblk, float* out1, zt_stream_t stream);
int zt_flow_to_rgb(const float* flow, int H, int W, int Hf, int Wf, int oy, int ox, const float* rad_dev, unsigned char* out_u8,
                   float* out_f32, int bgr, zt_stream_t stream);
int zt_flow_wheel(unsigned char* out165);
int zt_tc_viz_f32(const float* cur, const float* prev /* or NULL */, const float* fb, const float* ff, int H, int W, int Hf, int Wf,
                  int oy, int ox, const float* rad_dev, float gain, float* out, zt_stream_t stream);
int zt_flow_pack_hwc_f32(const float* flow, int H, int W, int Hf, int Wf, int oy, int ox, float* out, zt_stream_t stream);

/* ---- no-reference grading of a video (zt_noref.hip): evals.py --noref 1, DESIGN 8j --------------------------------------------------
 * a, b: planar fp32 [3][H][W], the decoded input and the enhanced frame.  Level = zt_quant_u8(v, 1) = rint(v * 255) & 255 (one fp32
 * multiply), lightness L = max of the three levels; La from a, Lb from b.  Sample (i, j) of the Hs x Ws grid is the pixel at row
 * ((2i + 1) H) / (2 Hs), column ((2j + 1) W) / (2 Ws) in integers: (Hs, Ws) = (H, W) is every pixel once, a larger grid repeats pixels.
 * zt_lightness_joint_hist_f32: hist[x * 256 + y] = number of samples with (La, Lb) = (x, y), uint32 [256][256]; hist is zeroed in
 *   stream order first.  Each workgroup counts at most 65532 samples in a private table of 16-bit counters in LDS (128 KB) and adds
 *   its non-zero counters to hist with integer atomics: any order of the additions gives the same table.  16-byte loads on the full
 *   grid when W % 4 == 0 and both frames are 16-byte aligned, value-wide loads otherwise, same result.  H, W outside 1..2^20,
 *   Hs, Ws < 1, Hs * Ws >= 2^32, a NULL or misaligned pointer: ZT_EINVAL.
 * zt_noref_from_hist: with C the 2-D inclusive cumulative sum of hist, R[x] = C[x][255], K[y] = C[255][y], ha / hb the marginals:
 *   out_i = { Ns = C[255][255], S_loe = sum hist[x][y] (R[x] + K[y] - 2 C[x][y]), S_a = sum x ha[x], S_b = sum y hb[y], hb[255],
 *   hb[0] } as exact 64-bit integers (S_loe < Ns^2: exact for Ns up to 2^31), out_f = { E_a, E_b }, the entropies in bits of the two
 *   marginals, -sum p log2 p with p = h / Ns in fp64, added in level order.  R[x] + K[y] - 2 C[x][y] is the number of samples q for
 *   which (La_p >= La_q) xor (Lb_p >= Lb_q) for a sample p at (x, y), so S_loe is the lightness order error summed over all ordered
 *   pairs.  hist: 16-byte aligned, read only; one workgroup, no workspace.  Deterministic; nothing synchronises. */
int zt_lightness_joint_hist_f32(const float* a, const float* b, int H, int W, int Hs, int Ws, unsigned int* hist, zt_stream_t stream);
int zt_noref_from_hist(const unsigned int* hist, long long* out_i /* [6] */, double* out_f /* [2] */, zt_stream_t stream);

/* ---- no-reference colour grading of a frame (zt_color.hip): evals.py --color 1, DESIGN 8m --------------------------------------------
 * x: planar fp32 [3][H][W].  Levels R, G, B = zt_quant_u8(v, 1) = rint(v * 255) & 255; N = H * W; block = B, 4..64; k1 = W / B,
 * k2 = H / B, nblk = k1 * k2; block (i, j) is rows iB .. iB + B - 1, columns jB .. jB + B - 1, the rows and columns left over are in
 * no block.  lin16: uint32 [256], the sRGB decoding of a level times 65535, rounded; flut: fp32 [65536], the CIELAB f(i / 65535); both
 * are made by the caller in fp64 (zero-tig_amd/ops.py).  Per pixel, in unsigned 32-bit and then in fp32 with one rounding an operation:
 *     r, g, b = lin16[R], lin16[G], lin16[B]
 *     X16 = (28440 r + 24655 g + 12441 b + 32768) >> 16, Y16 = (13938 r + 46868 g + 4730 b + 32768) >> 16,
 *     Z16 = (1164 r + 7174 g + 57198 b + 32768) >> 16;  fx, fy, fz = flut[X16], flut[Y16], flut[Z16]
 *     L = 116 fy - 16; a = 500 (fx - fy); b = 200 (fy - fz); C = sqrtf(a a + b b); D = sqrtf(C C + L L); S = D > 0 ? C / D : 0
 *     kL = (int)floorf(L * 10) clamped to 0..1000
 * Per channel c and pixel of a block, e2 = (gx gx + gy gy) c c with the 3 x 3 Sobel pair on the levels, frame borders replicated
 * (a block's rim reads the real pixels beyond it); per block and channel emax2 / emin2 = the largest / smallest e2, and cmax / cmin
 * = the largest / smallest of the block's 3 B B levels.
 * out_i = { N, nblk, sum R, sum G, sum B, S1 S2 T of R - G, S1 S2 T of R + G - 2B, n_kept, k01, k99, the number of blocks with
 *   emin2 == 0 for R, G, B, the number of blocks with cmax == cmin }: S1 / S2 the sum / the sum of squares; T the sum of the values
 *   that are left when, in ascending order, the first TL = (N + 9) / 10 and the last TR = N / 10 are dropped, n_kept = N - TL - TR;
 *   k01 / k99 the smallest kL whose cumulative count reaches (N + 99) / 100 / (99 N + 99) / 100.  Exact 64-bit integers.
 * out_f = { sum C, sum (double)C (double)C, sum S, E_R, E_G, E_B, A }: E_c = sum over the blocks with emin2 > 0 of
 *   log(emax2 / emin2), A = sum over the blocks with cmax > cmin of r log(r), r = (cmax - cmin) / (cmax + cmin), in fp64.
 * One pass over the frame by at most max_workgroups workgroups (0: the default, 256; at most 1024), each with a private table of the
 * six histograms in LDS that it adds to the table in ws with integer atomics, and its own fp64 sums; then one workgroup finishes.  The order of every fp64
 * sum follows from H, W, block and max_workgroups alone: the same call gives the same bits.  ws: 8-byte aligned, at least the size
 * zt_color_ws_bytes reports (a pure host query); nothing in it is kept between calls.  H, W < 1, H * W >= 2^31, block outside
 * 4..64, max_workgroups < 0, a NULL or misaligned pointer, a workspace too small: ZT_EINVAL.  Nothing synchronises. */
int zt_color_ws_bytes(int H, int W, int block, size_t* bytes);
int zt_color_stats_f32(const float* x, int H, int W, int block, const unsigned int* lin16, const float* flut, int max_workgroups,
                       void* ws, size_t ws_bytes, long long* out_i /* [18] */, double* out_f /* [7] */, zt_stream_t stream);

/* ---- NIQE of a frame (zt_niqe.hip): evals.py --niqe MODEL, DESIGN 8n --------------------------------------------------------------
 * Mittal, Soundararajan and Bovik 2013, as the MATLAB release's computefeature / computequality and its Python ports state it.
 * Per-pixel work in unsigned integers or in fp32 with one rounding an operation, sums in fp64.
 * x: planar fp32 [3][H][W].  Levels R, G, B = zt_quant_u8(v, 1); grey g = (19591 R + 38472 G + 7473 B + 32768) >> 16, 0..255.
 * Crop: Hc = H / 96 * 96, Wc = W / 96 * 96 from the top left; everything below is about the cropped image.  k2 = Hc / 96,
 * k1 = Wc / 96, nblk = k1 * k2, block b = i k1 + j is rows 96 i .., columns 96 j .. .
 * Scale 1: x = (float)g, block side P = 96.  Scale 2: the half-size image (Hc / 2 x Wc / 2, P = 48) of MATLAB's imresize(., 0.5):
 *   S[i][j] = sum_a sum_b t[a] t[b] g[rf(2i - 3 + a)][rf(2j - 3 + b)], t = (-3, -9, 29, 111, 111, 29, -9, -3), a, b = 0..7, in
 *   integers (|S| < 2^25); rf reflects with the edge repeated (-1 -> 0, -2 -> 1, n -> n - 1); x2 = (float)S * (1.0f / 65536).
 * MSCN field of either scale over its whole image: win = fp32 [7], the normalised Gaussian of sigma 7 / 6 rounded from fp64 by the
 *   caller; rows then columns, indices clamped to the image; acc = win[0] p[0], then acc = acc + win[k] p[k], k = 1..6; mu from x, m2
 *   from x * x (the product rounded once); sigma = sqrtf(fabsf(m2 - mu * mu)); m = (x - mu) / (sigma + 1.0f).  A sample of the
 *   half-size image beyond its edge is the clamped sample of x2 (clamp first, then that sample's eight taps).
 * Per block and scale five fields: f = 0: m; f = 1..4: m[y][x] * m[(y - dy) mod P][(x - dx) mod P], (dy, dx) = (0, 1), (1, 0), (1, 1),
 *   (1, -1), the shift circular within the block.  Of field f: n_neg / n_pos = the samples v < 0 / v > 0, S2_neg / S2_pos = the sums of
 *   v * v (rounded to fp32) over them, S_abs = the sum of |v|; S_sigma = the sum of sigma over the block (scale 1; 0 at scale 2).
 * zt_niqe_block_sums_f32: out_i = int64 [2][nblk][10] = { n_neg, n_pos } of f = 0..4; out_f = fp64 [2][nblk][16] = { S2_neg, S2_pos,
 *   S_abs } of f = 0..4, then S_sigma; scale 1 first.  One pass over x writes the grey levels of the cropped image into ws; then a
 *   workgroup per tile (one block of one scale, at most max_workgroups of them, 0: no cap).  The order of every sum follows from P
 *   alone: the same frame gives the same bits whatever max_workgroups is.  ws: 4-byte aligned, at least what zt_niqe_ws_bytes
 *   reports (a pure host query); nothing in it is kept between calls.
 * zt_niqe_frame_f32: sums_i / sums_f as above; r_gam, c1, c2: fp64 [9801] made by the caller over alpha_i = 0.2 + 0.001 i:
 *   r_gam = Gamma(2/a)^2 / (Gamma(1/a) Gamma(3/a)) (strictly increasing), c1 = sqrt(Gamma(1/a) / Gamma(3/a)), c2 = Gamma(2/a) / Gamma(1/a).
 *   The fit of a field, n = P * P, in fp64: l = sqrt(S2_neg / n_neg), r = sqrt(S2_pos / n_pos), gh = l / r,
 *   rhat = (S_abs / n)^2 / ((S2_neg + S2_pos) / n), rn = rhat (gh^3 + 1)(gh + 1) / (gh^2 + 1)^2, pos = the first index that minimises
 *   (r_gam[i] - rn)^2 (by bisection and a comparison of the two neighbours), alpha = 0.2 + 0.001 pos, bl = l c1[pos], br = r c1[pos],
 *   mean = (br - bl) c2[pos].  n_neg = 0, n_pos = 0 or an rn that is not finite: every number of the fit is NaN.
 *   Features of a scale: (alpha, (bl + br) / 2) of f = 0, then (alpha, mean, bl, br) of f = 1..4: 18; a block's row is scale 1 then
 *   scale 2: 36.  A row is valid when all 36 are finite.
 *   out_i = int64 [38] = { nblk, nv = the valid rows, count[36] = the finite values of each column };
 *   out_f = fp64 [738] = { the sum of the finite values of each column [36], the mean of the valid rows [36], the scatter of the valid
 *   rows about that mean, sum (f_i - mean_i)(f_j - mean_j), upper triangle row-major [666] }; mean and scatter are 0 when nv = 0.
 *   One workgroup, rows in block order.  Deterministic.
 * H or W < 96, H * W >= 2^31, nblk < 1, max_workgroups < 0, a NULL or misaligned pointer, a workspace too small: ZT_EINVAL.
 * Nothing synchronises. */
int zt_niqe_ws_bytes(int H, int W, size_t* bytes);
int zt_niqe_block_sums_f32(const float* x, int H, int W, const float* win, int max_workgroups, void* ws, size_t ws_bytes,
                           long long* out_i, double* out_f, zt_stream_t stream);
int zt_niqe_frame_f32(const long long* sums_i, const double* sums_f, int nblk, const double* r_gam, const double* c1, const double* c2,
                      long long* out_i /* [38] */, double* out_f /* [738] */, zt_stream_t stream);

/* ---- result PNGs encoded on the device (zt_png.hip) ------------------------------------------------------------------
 * predict.py:57-61, 101-104 (and evals.py's --save_images files): `Image.fromarray(u8).save(path, "PNG")`.  src: uint8 [H][W][3] (what
 * zt_quantize_u8_hwc writes) -> out: a complete zlib stream (78 01, deflate blocks, big-endian Adler-32) of the Paeth-filtered
 * scanlines, *nbytes (device scalar) = its length; the host frames it as IHDR / IDAT / IEND with CRC-32s.  Blocks of 8 rows, each
 * one dynamic-Huffman block of literals with its own length-limited canonical code (no LZ77 matching), byte-aligned by an empty
 * stored block.  Deterministic.  ws (16-byte aligned) / out (4-byte aligned): at least the sizes zt_png_sizes reports.
 * zt_png_encode_u8_mode: mode 1 = that stream (zt_png_encode_u8 means mode 1); mode 2 = the same scanlines, blocks and framing, but a
 * block whose bytes have runs is written with run-length matches (length 3..258, distance 1, never reaching across the block; 286
 * literal/length codes, one distance code) where that is strictly shorter, and exactly as in mode 1 otherwise: never longer than
 * mode 1, and the mode-1 bytes where no block has a run worth a match.  Any other mode is ZT_EINVAL.  Same sizes for both modes.
 * zt_png_sizes: pure host query (no device work, no stream): workspace and worst-case stream size in bytes for an H x W frame.
 * zt_png_code_lengths: the code construction alone: hist257 = counts of the 256 byte values + end-of-block -> len257 = code
 * lengths (0 = symbol unused, at most 15, Kraft sum exactly 1; a lone symbol gets an unused one-bit sibling). */
int zt_png_sizes(int H, int W, size_t* ws_bytes, size_t* out_bytes);
int zt_png_encode_u8(const unsigned char* src, int H, int W, void* ws, size_t ws_bytes, unsigned char* out, size_t out_bytes,
                     unsigned* nbytes, zt_stream_t stream);
int zt_png_encode_u8_mode(const unsigned char* src, int H, int W, int mode, void* ws, size_t ws_bytes, unsigned char* out,
                          size_t out_bytes, unsigned* nbytes, zt_stream_t stream);
int zt_png_code_lengths(const unsigned* hist257, unsigned char* len257, zt_stream_t stream);


/* ---- hardware self-test probes (zt_probe.hip): pin the test emulator's model of gfx950 instructions to the chip ----- */
/* ds_read_b64_tr_b16 on a [16][64] image of 16-bit codes: out[lane*4+q]; bf16 MFMA 16x16x32: D[16][16] = A[16][32] B[32][16] */
int zt_probe_tr16(const unsigned short* img, unsigned short* out, int col0, zt_stream_t stream);
int zt_probe_mfma_bf16(const unsigned short* A, const unsigned short* B, float* D, zt_stream_t stream);


/* ---- bf16 throughput mode of the convolution family: x / x2 / aux / dz are bf16 nhwc (channel strides multiples of 8), w is
 * bf16 [tap][CoutP][ldk] (input channel fastest; the all-pairs correlation passes fmap2 itself, nhwc, as w), accumulation fp32.
 * out_mode: 0 = bf16 nhwc, 1 = fp32 planar (plane pitch ldy), 2 = fp32 nhwc.  Same geometries / act / alpha / epi as the fp32 entry. */
int zt_conv2d_nhwc_bf16(const void* x, const void* x2, int csplit, int ldx, int ldx2, int N, int H, int W, int Cin, const void* w,
                        int CoutP, int ldk, const float* bias, void* y, int ldy, int out_mode, int Cout, int KH, int KW, int stride,
                        int padH, int padW, int act, float alpha, const void* aux, int ldaux, int epi, zt_stream_t stream);
/* TWO independent stride-1 convolutions over the same map (square kernels KA / KB in {1, 3, 7}, pad K / 2; bf16 nhwc in and out,
 * y = act(conv + bias)) in ONE launch: RAFT's motion encoder runs convc1 (1x1, 324 -> 256) next to convf1 (7x7, 2 -> 128) and convc2
 * (3x3, 256 -> 192) next to convf2 (3x3, 128 -> 64) (update.py:89-94).  Same results as two zt_conv2d_nhwc_bf16 calls (which is what
 * it falls back to when the two problems do not share a launch shape). */
int zt_conv2d_pair_nhwc_bf16(const void* xA, int ldxA, int CinA, const void* wA, int CoutPA, int ldkA, const float* biasA, void* yA, int ldyA,
                             int CoutA, int KA, const void* xB, int ldxB, int CinB, const void* wB, int CoutPB, int ldkB, const float* biasB,
                             void* yB, int ldyB, int CoutB, int KB, int N, int H, int W, int act, zt_stream_t stream);
/* same, with the kernel variant pinned (tests / tuning): 0 auto, 1 persistent weight-stationary (stride 1, K in {1,3}, Cin <= 64, N == 1),
 * 2 tiled, 3 register-stationary persistent (3x3, bf16 nhwc output, act in {none, ReLU, LeakyReLU}, exactly 48 or 64 couts) */
int zt_conv2d_nhwc_bf16_variant(const void* x, const void* x2, int csplit, int ldx, int ldx2, int N, int H, int W, int Cin, const void* w,
                                int CoutP, int ldk, const float* bias, void* y, int ldy, int out_mode, int Cout, int KH, int KW, int stride,
                                int padH, int padW, int act, float alpha, const void* aux, int ldaux, int epi, int variant, zt_stream_t stream);
/* bf16 twin of zt_conv2d_nhwc_f32_ex (epi 4 / 5: bf16 nhwc outputs, tiled kernel), plus
 * epi 6: y = relu(act(conv + bias) + aux) -- the tail of a RAFT ResidualBlock whose eval-mode BatchNorm is folded into the
 *        conv's weights and bias (model/RAFT/extractor.py:45-56: `y = relu(norm2(conv2(y))); return relu(x + y)`) */
int zt_conv2d_nhwc_bf16_ex(const void* x, const void* x2, int csplit, int ldx, int ldx2, int N, int H, int W, int Cin, const void* w,
                           int CoutP, int ldk, const float* bias, void* y, int ldy, int out_mode, int Cout, int KH, int KW, int stride,
                           int padH, int padW, int act, float alpha, const void* aux, int ldaux, int epi, void* y2, int ldy2, int esplit,
                           zt_stream_t stream);
/* Enhancer block head (model.py:60-62): y = conv3x3(x) + bias (stride 1, pad 1, N == 1, bf16 nhwc) AND the train-mode
 * BatchNorm statistics of y in the same pass: stats [stats_blocks = 512][2][Cout] per-workgroup partial (sum, sum of squares) of
 * the stored values, zero-filled beyond the launch's workgroups -- feed to zt_norm_finalize_f32(partial = stats, nblk = 512).
 * The 64 -> 64 full-resolution layer accumulates them in the register-stationary kernel's store phase; any other geometry runs
 * the convolution followed by the statistics kernel (same output contract). */
int zt_conv3x3_bn_stats_bf16(const void* x, int ldx, int H, int W, int Cin, const void* w, int CoutP, int ldk, const float* bias,
                             void* y, int ldy, int Cout, float* stats, int stats_blocks, zt_stream_t stream);
/* Enhancer block backward (autograd of model.py:60-67): df = conv3x3^T(dz) + res (the data gradient with the residual add, wT = the
 * flipped / transposed weights, all bf16 nhwc with 64 channels, N == 1) AND, in the same pass, the BatchNorm-backward sums of the
 * block BELOW, whose output gradient df is: g = df * [bn_scale * zprev + bn_shift > 0] (its ReLU), stats [512][2][64] = per-workgroup
 * (sum g, sum g (zprev - bn_mean)), zero beyond the launch's workgroups -- feed to zt_bn_bwd_sums_centered_f32(nblk = 512).
 * Replaces zt_conv2d_nhwc_bf16 (epi 3) + zt_bn_bwd_reduce. */
int zt_conv3x3_dgrad_bn_sums_bf16(const void* dz, int lddz, int H, int W, const void* wT, int CoutP, int ldk, void* df, int lddf,
                                  const void* res, int ldres, const void* zprev, int ldz, const float* bn_scale, const float* bn_shift,
                                  const float* bn_mean, float* stats, int stats_blocks, zt_stream_t stream);
/* relu_mask (optional, thin-input 3x3 layer with 64 couts): dz is taken as dz * [relu_mask > 0], i.e. the backward of the ReLU
 * that follows the layer (model.py:55-56) is folded into the staging of dz instead of a separate masking pass */
int zt_conv2d_wgrad_nhwc_bf16(const void* x, int ldx, const void* dz, int lddz, int H, int W, int Cin, int Cout, int KH, int KW,
                              float* slab, size_t slab_bytes, float* grad_w, float* grad_b, int accumulate, const void* relu_mask,
                              int ldmask, zt_stream_t stream);
/* Deferred, batched form of the weight gradient for a whole backward pass (bf16 mode): every call of a layer APPENDS its
 * per-workgroup slabs (KH*KW*Cin16*Cout16 + Cout16 floats each, Cin16 / Cout16 = channel counts rounded up to 16) to that layer's slab region and reports how many it wrote
 * (*nslab_out, host int); zt_wgrad_reduce_multi_f32 then reduces up to 16 layers in ONE launch: layer i sums nslab[i] slabs at
 * slab[i] into grad_w[i] ([Cout][Cin][K][K]) and grad_b[i] (may be NULL), (+)= when accumulate.  All array arguments are host arrays. */
int zt_conv2d_wgrad_partial_bf16(const void* x, int ldx, const void* dz, int lddz, int H, int W, int Cin, int Cout, int KH, int KW,
                                 float* slab, size_t slab_bytes, const void* relu_mask, int ldmask, int* nslab_out, zt_stream_t stream);
/* Backward of Denoise_1/2's 1x1 output layer (model.py:27, 43) in one pass over its operands: dz[p][48] = (W^T dr[p]) * LeakyReLU'(a2[p])
 * (what zt_conv2d_nhwc_bf16 with the transposed weights wT [48][8] and epi 1 computes) AND the layer's weight / bias gradient slabs
 * ([48][16] + [16] floats each, *nslab_out of them appended at `slab`: feed to zt_wgrad_reduce_multi_f32 with Cin 48, Cout Cdr, K 1).
 * dr: nhwc bf16 [HW][8] with Cdr = 3 or 6 valid channels; a2 / dz: nhwc bf16, channel strides lda / lddz >= 48. */
int zt_thin1x1_bwd_bf16(const void* dr, int Cdr, const void* wT, const void* a2, int lda, void* dz, int lddz, int HW, float* slab,
                        size_t slab_bytes, int* nslab_out, zt_stream_t stream);
int zt_wgrad_reduce_multi_f32(int nseg, const void* const* slab, const int* nslab, const int* Cin, const int* Cout, const int* K,
                              void* const* grad_w, void* const* grad_b, int accumulate, zt_stream_t stream);
/* all weight repacks of a step in one launch (up to 24 entries; host arrays; square kernels K x K; same layouts as the single form) */
int zt_repack_conv_weights_bf16_multi(int n, const void* const* src, void* const* dst, const int* Cout, const int* Cin, const int* K,
                                      const int* CoutP, const int* ldk, const int* transpose_flip, zt_stream_t stream);
int zt_repack_conv_weight_bf16(const float* src, void* dst, int Cout, int Cin, int KH, int KW, int CoutP, int ldk, int co_off,
                               int transpose_flip, zt_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
