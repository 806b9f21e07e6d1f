/*
 * libshgan_hip.so -- C ABI of the MI355X-native SH-GAN generator-forward kernels.
 *
 * Drop-in boundary: everything the reference reaches through its native plugin
 * (`upfirdn2d_plugin.upfirdn2d`, lib/model_zoo/stylegan_utils/upfirdn2d.cpp:16,98-101) or through
 * ATen/cuDNN from the Python ops of lib/model_zoo/{stylegan,shgan}.py is exported here with plain
 * pointers and sizes.  Conventions:
 *   - all tensors are dense NCHW fp32 device buffers owned by the caller (outputs and workspaces
 *     included); no hidden allocation, no synchronisation; work is enqueued on `stream`
 *     (a hipStream_t passed as void*), like at::cuda::getCurrentCUDAStream() in upfirdn2d.cpp:91;
 *   - return value 0 = ok, <0 = error (SHG_ERR_*); shg_last_error() gives the message
 *     (the reference raises RuntimeError from TORCH_CHECK / AT_CUDA_CHECK, upfirdn2d.cpp:19-36,92);
 *   - thread-safe for distinct streams; the error string is thread-local.
 *
 * Extents.  No entry point reads or writes a byte outside the extents stated for its arguments: a tensor
 * argument is exactly the elements of the shape and strides given for it, a packed operand exactly what its
 * `*_elems` / `*_bytes` function returns, and a workspace `ws` is touched only within
 * [ws, ws + *_workspace_bytes(...)).  This holds for buffers without any allocator slack before or behind
 * them: ragged last tiles, vector accesses, plane pitches, channel padding and split-K slices stay inside.
 * tests/test_gpu_alloc_guard.py runs every entry point on buffers housed between poisoned guard bands.
 */
#ifndef SHGAN_HIP_H
#define SHGAN_HIP_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define SHG_OK 0
#define SHG_ERR_ARG (-1)
#define SHG_ERR_LAUNCH (-2)
#define SHG_ERR_UNSUPPORTED (-3)

int shg_abi_version(void);
const char* shg_last_error(void);
/* gcnArchName of device `dev` into buf; returns the CU count (256 on MI355X) or <0. */
int shg_device_info(int dev, char* buf, int buflen);

/* ---- A10: upfirdn2d -- replaces upfirdn2d.cpp:16 `upfirdn2d(x,f,upx,upy,downx,downy,padx0,padx1,pady0,pady1,flip,gain)`.
 * x [N,C,H,W], f [fh,fw], y [N,C,OH,OW] with OH/OW from shg_upfirdn2d_out_size (rule of upfirdn2d.cpp:32-33). */
int shg_upfirdn2d_out_size(int H, int W, int fh, int fw, int upx, int upy, int downx, int downy, int padx0, int padx1,
                           int pady0, int pady1, int* OH, int* OW);
int shg_upfirdn2d_f32(const float* x, const float* f, float* y, int N, int C, int H, int W, int fh, int fw, int upx, int upy,
                      int downx, int downy, int padx0, int padx1, int pady0, int pady1, int flip, float gain, void* stream);
/* the same operator over the plugin's whole operand range (upfirdn2d.cpp:38-59: any strides, AT_DISPATCH_FLOATING_TYPES_AND_HALF):
 * dtype 0 float32 / 1 float16 / 2 float64 (accumulation float, float64: double); x_strides / y_strides = element strides (n, c, h, w);
 * f float32 [fh,fw] with element strides f_stride_y / f_stride_x.  Serves float64, float32 channels_last, float16 NCHW and views
 * without a conversion pass; the two dense network layouts keep their streaming kernels (shg_upfirdn2d_f32 / _f16). */
int shg_upfirdn2d_strided(const void* x, const float* f, void* y, int dtype, int N, int C, int H, int W, const long* x_strides,
                          const long* y_strides, int fh, int fw, long f_stride_y, long f_stride_x, int upx, int upy, int downx, int downy,
                          int padx0, int padx1, int pady0, int pady1, int flip, float gain, void* stream);
/* upfirdn2d fused with the tail of an up-sampling synthesis layer (stylegan.py:295-304, comodgan.py:326-327):
 * y = lrelu_agc(FIR(x)*gain*scale[n,c] + noise*noise_strength + bias[c]) + residual.
 * noise_mode 0 none, 1 noise [OH,OW], 2 noise [N,OH,OW]; act 0 none / 1 lrelu_agc; clamp < 0 = no clamp. */
int shg_upfirdn2d_epilogue_f32(const float* x, const float* f, float* y, int N, int C, int H, int W, int fh, int fw, int upx,
                               int upy, int downx, int downy, int padx0, int padx1, int pady0, int pady1, int flip, float gain,
                               const float* scale, const float* bias, const float* noise, int noise_mode, float noise_strength,
                               int act, float alpha, float act_gain, float clamp, const float* residual, void* stream);

/* ---- A11: bias + activation -- the `x + bias -> lrelu_agc(gain)` of stylegan.py:232-238 / common/utils.py:135-143,
 * with the optional demodulation scale [N*C], noise and residual of the non-fused modconv path (stylegan.py:175-180). */
int shg_bias_act_f32(const float* x, float* y, const float* scale, const float* bias, const float* noise, int noise_mode,
                     float noise_strength, const float* residual, int N, int C, int HW, int act, float alpha, float gain,
                     float clamp, void* stream);
/* Backward of shg_bias_act_f32 without scale / noise / residual (the training path's bias + lrelu_agc): dx = g * slope(y), with
 * the forward OUTPUT y.  The bias gradient is the per-channel sum of dx. */
int shg_bias_act_backward_f32(const float* g, const float* y, float* dx, long total, int act, float alpha, float gain, float clamp,
                              void* stream);
/* stylegan_utils/fma.py:15 -- y = a*b + c, elementwise on `total` floats. */
int shg_fma_f32(const float* a, const float* b, const float* c, float* y, long total, void* stream);
/* stylegan_utils/fma.py:15-58 with NumPy broadcasting and without materialising it: y (contiguous, `shape`) = a*b + c, each operand
 * addressed through element strides (0 on a broadcast dimension); c may be NULL (y = a*b, the product of fma.py:41,44).  nd <= 6
 * (collapse neighbouring dimensions first); f64 != 0: operands are doubles. */
int shg_fma_bcast(const void* a, const void* b, const void* c, void* y, int nd, const long* shape, const long* sa, const long* sb,
                  const long* sc, int f64, void* stream);
/* `_unbroadcast(g * b, shape)` (fma.py:48-58) in one pass: dimensions ordered kept-first (nk of them), reduced-last; out (contiguous,
 * the kept sizes) = sum over the reduced index of g*b (b NULL: of g).  inner_kept != 0 when g's fastest-varying dimension is a kept
 * one (one thread per output), 0 for one workgroup per output along the reduced index.  Fixed summation order: deterministic. */
int shg_mul_reduce(const void* g, const void* b, void* out, int nd, int nk, const long* shape, const long* sg, const long* sb,
                   int inner_kept, int f64, void* stream);
/* stylegan.py:173 -- y[nc,:] = x[nc,:] * s[nc]. */
int shg_scale_channels_f32(const float* x, const float* s, float* y, int NC, int HW, void* stream);
/* out [N,K] = sum over b of part [N,B,K] in block order (the per-workgroup partial sums of shg_modtail_backward_*: deterministic). */
int shg_sum_partials_f32(const float* part, float* out, int N, int B, int K, void* stream);
/* `(weight * gain).to(float16)` of the fp16 layers and its gradient in one launch each: to_half != 0: dst (halves) = half(src (floats) * gain);
 * else dst (floats) = float(src (halves)) * gain. */
int shg_scale_cast_f32_f16(const void* src, void* dst, long n, float gain, int to_half, void* stream);
/* Phase planes of a stride-2 transposed convolution (shg_conv2d_f32 mode 2 / out_mode 1, shg_conv2d_up_poly_f32) -> image with the
 * crop / zero-extension conv2d_gradfix.py:96-128 applies: y[n,c,Y,X] = full[Y+lo][X+lo] (+ bias[c]), zero outside the
 * (2H+1) x (2W+1) result.  N*C <= 65535. */
int shg_planes_to_image_f32(const float* mid, const float* bias, float* y, int N, int C, int H, int W, int lo, int OH, int OW,
                            void* stream);

/* ---- A9/A8: convolution on the fp32 MFMA units -- replaces F.conv2d / F.conv_transpose2d reached through
 * conv2d_gradfix.py:35-43,109-116 from conv2d_resample.py:26-51.
 * Weight preparation: w [O,I,KH,KW] -> wt [OP/64][IP*KH*KW][64] (GEMM layout in 64-column blocks; OP = O rounded up to a
 *   multiple of 64, IP = I rounded up to a multiple of 32, padding zero filled),
 *   wscale [O] scratch, wsq [I*OP] (sum over taps of wt^2, for demodulation) or NULL.
 *   demod=1: w * rsqrt(mean_{I,k,k} w^2) (stylegan.py:146) * gain; demod=0: w * gain (stylegan.py:227).
 *   flip=1 gives a true convolution (w.flip([2,3]), conv2d_resample.py:32-33); one layout serves all modes. */
int shg_conv_weight_prep_f32(const float* w, float* wt, float* wscale, float* wsq, int O, int I, int KH, int KW, int OP,
                             int demod, float gain, int flip, void* stream);
/* y = act(out_scale[n,o] * conv(x * in_scale[n,i], wt) + noise*noise_strength + bias[o]) + residual.
 * mode 0: stride 1, symmetric `pad` -> [NB,O,H+2pad-kh+1,..]; mode 1: stride 2 -> [(H+2pad-kh)/2+1];
 * mode 2: transposed stride 2, pad 0 -> [2H+1, 2W+1] (conv2d_resample.py:130-137); all four sub-pixel phases in one pass.
 * Slot b uses the weight set wt + (b % wgroups)*wstride (wgroups > 1 = grouped conv, stylegan.py:187-190).
 * Any of in_scale [NB,I], out_scale [NB,O], bias [O], noise, residual [NB,O,OH,OW] may be NULL. */
int shg_conv2d_f32(const float* x, const float* wt, float* y, int NB, int I, int O, int OP, int H, int W, int kh, int kw,
                   int mode, int pad, int wgroups, long wstride, const float* in_scale, const float* out_scale,
                   const float* bias, const float* noise, int noise_mode, float noise_strength, int act, float alpha, float gain,
                   float clamp, const float* residual, int out_mode, void* workspace, size_t ws_bytes, void* stream);
/* Split-K workspace (bytes) shg_conv2d_f32 can use for this problem; 0 = no split.  Small grids (4x4..16x16 layers)
 * are split along the input channels so that they still fill 256 CUs. */
size_t shg_conv2d_workspace_bytes(int NB, int I, int O, int H, int W, int kh, int kw, int mode, int pad, int wgroups);
/* Winograd F(2x2,3x3) form of the stride-1 3x3 'same' convolution (mode 0, pad 1 of shg_conv2d_f32; same fused operands and
 * result up to fp32 round-off, 2.25x fewer MFMA flops).  Weights: w [O,I,3,3] with the per-output-channel factor wscale [O]
 * (the `wscale` output of shg_conv_weight_prep_f32) -> wu [OP/64][ceil(I/c)][16][64][c] = G (w*wscale) G^T in the
 * register layout of the kernel, c = shg_conv_wino_chunk() input channels per K-chunk. */
int shg_conv_wino_chunk(void);
int shg_conv_weight_prep_wino_f32(const float* w, const float* wscale, float* wu, int O, int I, int OP, int flip, void* stream);
int shg_conv2d_wino_f32(const float* x, const float* wu, float* y, int NB, int I, int O, int OP, int H, int W,
                        const float* in_scale, const float* out_scale, const float* bias, const float* noise, int noise_mode,
                        float noise_strength, int act, float alpha, float gain, float clamp, const float* residual, void* stream);
/* the same with scratch for a split along the input channels: a workgroup owns one (tile, 64 output channels) pair, so 512-channel layers
 * at 16^2 (32^2 for the F(4x4) form below) are 32-128 workgroups for batches 4-16 and take the same time at every batch; with
 * `workspace` of shg_conv2d_wino_workspace_bytes (0: the problem fills the chip, nothing is split) the channel chunks are cut into
 * slices, partial outputs summed and the layer tail applied by a second small launch.  Same result up to the order of the fp32 sums. */
size_t shg_conv2d_wino_workspace_bytes(int NB, int I, int O, int OP, int H, int W);
int shg_conv2d_wino_ws_f32(const float* x, const float* wu, float* y, int NB, int I, int O, int OP, int H, int W,
                           const float* in_scale, const float* out_scale, const float* bias, const float* noise, int noise_mode,
                           float noise_strength, int act, float alpha, float gain, float clamp, const float* residual, void* workspace,
                           size_t ws_bytes, void* stream);
/* Winograd F(4x4,3x3) form of the same convolution (conv_wino4.hip; 4x fewer MFMA flops than the direct form, about 1e-5
 * relative round-off per layer): wu has shg_conv_wino4_weight_elems(OP, I) floats, [OP/64][ceil(I/8)][4][72][64] in the
 * register layout of the kernel.  shg_conv2d_wino4_supported tells whether the geometry is served (H >= 16, W >= 32,
 * W % 4 == 0, I <= 1024); otherwise call shg_conv2d_wino_f32 / shg_conv2d_f32. */
long shg_conv_wino4_weight_elems(int OP, int I);
int shg_conv_weight_prep_wino4_f32(const float* w, const float* wscale, float* wu, int O, int I, int OP, int flip, void* stream);
int shg_conv2d_wino4_supported(int NB, int I, int O, int H, int W);
int shg_conv2d_wino4_f32(const float* x, const float* wu, float* y, int NB, int I, int O, int OP, int H, int W,
                         const float* in_scale, const float* out_scale, const float* bias, const float* noise, int noise_mode,
                         float noise_strength, int act, float alpha, float gain, float clamp, const float* residual, void* stream);
/* ... and with scratch for the split along the input channels (see shg_conv2d_wino_ws_f32): the 512-channel layers at 32^2 */
size_t shg_conv2d_wino4_workspace_bytes(int NB, int I, int O, int OP, int H, int W);
int shg_conv2d_wino4_ws_f32(const float* x, const float* wu, float* y, int NB, int I, int O, int OP, int H, int W,
                            const float* in_scale, const float* out_scale, const float* bias, const float* noise, int noise_mode,
                            float noise_strength, int act, float alpha, float gain, float clamp, const float* residual, void* workspace,
                            size_t ws_bytes, void* stream);
/* the same launch with the route of the weight operands chosen by the caller (A/B measurements, route-agreement test): 0 as
 * shg_conv2d_wino4_ws_f32 takes it (LDS ring; W >= 256 on 8 x 64 pixel tiles from 64 input channels on), 1 register ring, 2
 * wave-private LDS ring on the tile shapes that hold one, both with W >= 256 on the 4 x 128 pixel tiles, 3 like 2 with W >= 256 on
 * the 8 x 64 pixel tiles.  Same bits on every route. */
int shg_conv2d_wino4_route_f32(const float* x, const float* wu, float* y, int NB, int I, int O, int OP, int H, int W,
                               const float* in_scale, const float* out_scale, const float* bias, const float* noise, int noise_mode,
                               float noise_strength, int act, float alpha, float gain, float clamp, const float* residual, int route,
                               void* workspace, size_t ws_bytes, void* stream);
/* mode 2 with out_mode 1 writes the four sub-pixel phases as planes [4][NB,O,H+1,W+1] (coalesced); this kernel applies the
 * 4x4 FIR of conv2d_resample.py:138 (pad 1) straight from the planes and fuses the synthesis-layer tail:
 * y [N,C,2H,2W] = lrelu_agc(FIR(mid)*gain*scale[n,c] + noise*noise_strength + bias[c]) + residual.  H, W = low-res extents. */
int shg_upfir_planar_f32(const float* mid, const float* f, float* y, int N, int C, int H, int W, int flip, float gain,
                         const float* scale, const float* bias, const float* noise, int noise_mode, float noise_strength,
                         int act, float alpha, float act_gain, float clamp, const float* residual, void* stream);
/* The same for a SEPARABLE filter (row-marching kernel): taps_host = {fx[0..3], fy[0..3]} in HOST memory; W even, W/2 a divisor of
 * 64 or W in {128, 256}; y / noise / residual 16-byte aligned. */
int shg_upfir_planar_sep_supported(int H, int W);
int shg_upfir_planar_sep_f32(const float* mid, const float* taps_host, float* y, int N, int C, int H, int W, int flip, float gain,
                             const float* scale, const float* bias, const float* noise, int noise_mode, float noise_strength,
                             int act, float alpha, float act_gain, float clamp, const float* residual, void* stream);
/* Polyphase-Winograd form of mode 2 / out_mode 1 (conv_wino_poly.hip): the `ee` phase as F(3x3,2x2), `eo`/`oe`/`oo` of
 * every 2x2 block of low-resolution pixels with 16 multiplies, one-pixel strips by single-tap contractions -- 5.8 instead of
 * 9 multiplies per low-resolution pixel, same result up to fp32 round-off.  y [4][NB,O,H+1,W+1] raw phase planes (no
 * epilogue operands: the consumer is shg_upfir_planar_f32).  wt / wscale from shg_conv_weight_prep_f32; wu_a, wu_b:
 * [OP/64][ceil(I/8)][16][64][8] floats each.  shg_conv2d_up_poly_supported tells whether the geometry is served
 * (H, W >= 16, H even, W % 4 == 0); otherwise call shg_conv2d_f32. */
int shg_conv_weight_prep_up_poly_f32(const float* w, const float* wscale, float* wu_a, float* wu_b, int O, int I, int OP, int flip,
                                     void* stream);
int shg_conv2d_up_poly_supported(int NB, int I, int O, int H, int W);
int shg_conv2d_up_poly_f32(const float* x, const float* wt, const float* wu_a, const float* wu_b, float* y, int NB, int I, int O,
                           int OP, int H, int W, const float* in_scale, void* stream);
/* ... with scratch for the split along the input channels on small grids (see shg_conv2d_wino_ws_f32): 16^2 / 32^2 inputs */
size_t shg_conv2d_up_poly_workspace_bytes(int NB, int I, int O, int OP, int H, int W);
int shg_conv2d_up_poly_ws_f32(const float* x, const float* wt, const float* wu_a, const float* wu_b, float* y, int NB, int I, int O,
                              int OP, int H, int W, const float* in_scale, void* workspace, size_t ws_bytes, void* stream);
/* Polyphase-Winograd form of the FIR-filtered stride-2 3x3 convolution (conv2d_resample.py:116-120), same reduction of the
 * multiply count.  shg_fir_down_planar_f32 applies the 4x4 pre-filter (padding 2) to x [N,C,H,W] and writes the (H+1)x(W+1)
 * result as its four polyphase planes xp [4][N*C][H/2+1][PP] (PP = a multiple of 4 >= W/2+1); shg_conv2d_down_poly_f32 then
 * computes y [NB,O,OH,OW] = act(conv3x3_stride2 + bias)*gain + residual (OH = H/2, OW = W/2; OH, OW >= 16, OW % 4 == 0). */
int shg_fir_down_planar_f32(const float* x, const float* f, float* y, int N, int C, int H, int W, int PP, int flip, float gain,
                            void* stream);
/* Row-marching form of the same pre-filter for a SEPARABLE filter f[ky][kx] = fy[ky]*fx[kx] (every filter upfirdn2d.setup_filter
 * builds from a 1-D kernel, upfirdn2d.py:61-95): taps_host = {fx[0..3], fy[0..3]} in HOST memory.  PP == 0: y [N,C,H+1,W+1]
 * (= upfirdn2d(x, f, padding=2)); PP > 0: the polyphase planes above with pitch PP.  W in {8,16,32,64,128,256,512}. */
int shg_fir_pad2_sep_supported(int H, int W, int PP);
int shg_fir_pad2_sep_f32(const float* x, const float* taps_host, float* y, int N, int C, int H, int W, int PP, int flip, float gain,
                         void* stream);
/* The x2 resampling FIRs of the training rows, separable filter (taps_host as above), row-marching kernels:
 * up == 1: y [N,C,H/2,W/2] = upfirdn2d(x, f, down=2, padding=1); up == 2: y [N,C,2H,2W] = upfirdn2d(x, f, up=2, padding=[2,1,2,1]). */
int shg_fir_resample2_sep_supported(int H, int W, int up);
int shg_fir_resample2_sep_f32(const float* x, const float* taps_host, float* y, int N, int C, int H, int W, int up, int flip, float gain,
                              void* stream);
int shg_conv_weight_prep_down_poly_f32(const float* w, const float* wscale, float* wu_a, float* wu_b, int O, int I, int OP, int flip,
                                       void* stream);
int shg_conv2d_down_poly_supported(int NB, int I, int O, int OH, int OW);
int shg_conv2d_down_poly_f32(const float* xp, const float* wu_a, const float* wu_b, float* y, int NB, int I, int O, int OP, int OH,
                             int OW, int PP, const float* in_scale, const float* bias, int act, float alpha, float gain,
                             float clamp, const float* residual, void* stream);
/* 1x1 convolution with I <= 8 input channels (encoder fromrgb, stylegan.py:640-642): y = act(W*wgain @ x + bias). */
int shg_conv1x1_thin_in_f32(const float* x, const float* w, const float* bias, float* y, int N, int I, int O, int HW, float wgain,
                            int act, float alpha, float gain, float clamp, void* stream);
/* torgb (stylegan.py:325-337) fused with the RGB skip up-sampling (comodgan.py:331-338, upfirdn2d.py:305-314):
 * y[n,o] = sum_i w[o,i]*styles[n,i]*x[n,i] + bias[o] + upsample2d(base_up[n,o], f)   (O <= 4; base_up may be NULL). */
int shg_torgb_f32(const float* x, const float* w, const float* styles, const float* bias, const float* base_up, const float* f,
                  float* y, int N, int I, int O, int H, int W, void* stream);

/* ---- A3/A2: dense (stylegan.py:87-98), normalize_2nd_moment (stylegan.py:343-344). */
int shg_dense_f32(const float* x, const float* w, const float* b, float* y, int N, int K, int O, int ldx, int ldy, float wgain,
                  float bgain, int act, float alpha, float gain, float clamp, void* stream);
/* The other two products of a dense layer under autograd (the gradients of stylegan.py:87-98; the reference reaches them through
 * torch.addmm's backward): out[N,K] = scale * a[N,M] @ b[M,K]  and  out[M,K] = scale * a[N,M]^T @ b[N,K] with, optionally,
 * colsum[m] = csum_scale * sum_n a[n,m] (weight and bias gradient in one pass). */
int shg_matmul_nn_f32(const float* a, const float* b, float* out, int N, int M, int K, int lda, int ldo, float scale, void* stream);
int shg_matmul_tn_f32(const float* a, const float* b, float* out, float* colsum, int N, int M, int K, int lda, int ldb, float scale,
                      float csum_scale, void* stream);
/* Weight side of modulated_conv2d under autograd (stylegan.py:136-138,146,150-155): wn = w * rsqrt(mean_{i,k} w^2) per output channel (with
 * the fp16 pre-normalisation by the max-norm first when `prenorm`), wsq[o,i] = sum_k wn^2, sfac[o] = wn / w; and its transpose
 * g_w = sfac * (G - wn * mean(G wn)), G = g_wn + 2 g_wsq wn.  w, wn, gwn, gw: [O,I,K]; wsq, gwsq: [O,I]; sfac: [O]. */
int shg_demod_weight_f32(const float* w, float* wn, float* wsq, float* sfac, int O, int I, int K, int prenorm, void* stream);
int shg_demod_weight_backward_f32(const float* wn, const float* sfac, const float* gwn, const float* gwsq, float* gw, int O, int I, int K,
                                  void* stream);
/* Style side of modulated_conv2d under autograd (stylegan.py:138,147,155): sn = s1 * rsqrt(mean_{n,i} s1^2), s1 = s / max_i |s| per row when
 * `prenorm` else s; d[n,o] = rsqrt(sum_i sn^2 wsq[o,i] + 1e-8) (d may be NULL); aux [N+1] = {row maxima (1 without prenorm), rsqrt(mean)}.
 * Backward: gs [N,I], gwsq [O,I] (may be NULL) from gsn [N,I] / gd [N,O] (either may be NULL); partq = scratch of ceil(O/64)*N*I floats.
 * N <= 32, N*I <= 8192 (64 KB of LDS in the backward pass). */
int shg_style_factors_f32(const float* s, const float* wsq, float* sn, float* d, float* aux, int N, int I, int O, int prenorm, void* stream);
int shg_style_factors_backward_f32(const float* sn, const float* d, const float* wsq, const float* aux, const float* gsn, const float* gd,
                                   float* gs, float* gwsq, float* partq, int N, int I, int O, int prenorm, void* stream);
int shg_normalize_2nd_moment_f32(const float* x, float* y, int N, int K, float eps, void* stream);
/* ---- A4: per-forward style side of modulated_conv2d (stylegan.py:147-155):
 * s_out = styles*pre_gain*rsqrt(mean(.^2)) when demod (else styles*pre_gain); dcoef[n,o] = rsqrt(sum_i s^2*wsq[i,o] + 1e-8). */
int shg_modconv_style_prep_f32(const float* styles, int ld, const float* wsq, float* s_out, float* dcoef, int N, int I, int O,
                               int OP, int demod, float pre_gain, void* stream);

/* Grouped forms (at most 32 groups per call): every style affine of a synthesis pass in one launch, and every
 * normalisation / demodulation-coefficient computation in a second one.  Group g of shg_dense_grouped_f32 computes
 * y = [x1 | x2] @ (w*wgain)^T + b*bgain with w [O, K1+K2] -- the concatenated input cat([w_i, x_global]) of
 * comodgan.py:245-262,316-338 is read from its two sources; K2 = 0 -> plain dense.  The descriptor arrays are host
 * memory (copied into the kernel arguments); the pointers inside are device pointers. */
typedef struct {
    const float* x1; const float* x2; const float* w; const float* b; float* y;
    int ld1, ld2, K1, K2, O, ldy;
    float wgain, bgain;
} shg_dense_group;
int shg_dense_grouped_f32(const shg_dense_group* groups, int G, int N, void* stream);
typedef struct {
    const float* styles; const float* wsq; float* s_out; float* dcoef;
    int ld, I, O, OP, demod;
    float pre_gain;
} shg_style_group;
int shg_modconv_style_prep_grouped_f32(const shg_style_group* groups, int G, int N, void* stream);

/* ---- A16-A19: Spectral Hint Unit (shgan.py:312-336).
 * rfft2(norm='forward') + row shift of [C] planes of 64x64 per sample (x + n*x_batch_stride) -> T [N,2C,64,33]. */
int shg_shu_rfft2_shift_f32(const float* x, long x_batch_stride, float* T, int N, int C, void* stream);
/* Weight gradient of y = conv2d(x, w, stride, pad) (conv2d_gradfix.py:140-146, the cuDNN backward-weight call):
 * dw[o,i,ky,kx] = sum_{n,oy,ox} g[n,o,oy,ox] * x[n,i,oy*stride-pad+ky, ox*stride-pad+kx]; 3x3 or 1x1, stride 1 or 2; deterministic
 * (K slices summed in order).  For conv_transpose2d pass dL/dy as `x` and the layer input as `g`: dw comes out as [Cin,Cout,kh,kw].
 * Input gradients are compositions of the forward entry points (conv <-> transposed conv, conv2d_gradfix.py:118-135). */
size_t shg_conv2d_wgrad_workspace_bytes(int NB, int I, int O, int OH, int OW, int kh, int kw);
int shg_conv2d_wgrad_f32(const float* x, const float* g, float* dw, int NB, int I, int O, int H, int W, int OH, int OW,
                         int kh, int kw, int stride, int pad, void* workspace, size_t ws_bytes, void* stream);
/* The same weight gradient for the stride-1 3x3 'same' layers (pad 1, OH = H, OW = W, W % 4 == 0, W >= 4) in the Winograd domain -- the
 * transpose of F(4x4,3x3): dw = G^T [ sum_tiles (A dY A^T) .* (B^T d B) ] G, a quarter of the multiplications, both operands transformed
 * in the kernel, fp32 MFMA; deterministic; ~5e-6 relative against float64 (the direct form: ~2e-6).  shg_conv2d_wgrad_wino_supported
 * tells whether a geometry is served (1 / 0); x and g 16-byte aligned. */
int shg_conv2d_wgrad_wino_supported(int H, int W, int OH, int OW, int kh, int kw, int stride, int pad);
size_t shg_conv2d_wgrad_wino_workspace_bytes(int NB, int I, int O, int H, int W);
int shg_conv2d_wgrad_wino_f32(const float* x, const float* g, float* dw, int NB, int I, int O, int H, int W, void* workspace,
                              size_t ws_bytes, void* stream);
/* SHU spectral stage in one launch (shgan.py:320-321 conv0 + ReLU, :143-160 heterogeneous filter incl. the band sum):
 * S[n,o,p] = sum_k cw[k,p] * sum_i W1[o*bands+k, i] * relu(sum_j W0[i,j] T[n,j,p] + b0[i]);  T, S: [N,64,P], P % 64 == 0;
 * w0p [32][2][64] / w1p [bands*32][2][64]: weights in MFMA operand order, element [ks][mo][l] = W[mo*32 + (l & 31)][2*ks + (l >> 5)]
 * (for w1p the rows of band k are W1[o*bands+k, :]); cw [bands,P].  Then shg_shu_split_irfft2_f32 with bands = 1. */
int shg_shu_spectral_f32(const float* T, const float* w0p, const float* b0, const float* w1p, const float* cw, float* S,
                         int N, int C2, int P, int bands, void* stream);
/* band-weighted sum (bands > 1: Y [N,2C*bands,64,33], cw [bands,64,33]) -> Gaussian split -> unshift -> irfft2 at
 * r = 4,8,16,32,64: out[l] planes [C][r][r] per sample at out[l] + n*out_batch_stride[l]; accumulate=1 adds in place
 * (shgan.py:378-382).  gauss[l] = [r, r/2+1] table (shgan.py:281-310). */
int shg_shu_split_irfft2_f32(const float* Y, const float* cw, const float* const* gauss, float* const* out,
                             const long* out_batch_stride, int N, int C, int bands, int accumulate, void* stream);
/* Transpose of shg_shu_split_irfft2_f32 with bands == 1 (training rows: the gradient of shgan.py:326-336 w.r.t. the filtered
 * spectrum): g[l] = dL/d(out[l]) planes [N,C,r,r] (null = none) -> GS [N,2C,64,33].  The transpose of shg_shu_rfft2_shift_f32 is
 * shg_shu_split_irfft2_f32 itself, restricted to the 64 x 64 level with the table (1/c_k)/4096 (c_0 = c_32 = 1, else 2). */
int shg_shu_split_adjoint_f32(const float* const* g, const long* g_batch_stride, const float* const* gauss, float* GS, int N, int C,
                              void* stream);
/* Size-general forms of the four SHU entry points above (which stay fixed at 64 x 64 with 5 levels): `size` = the transform size
 * (shu_input_res) = 16, 32, 64 or 128 -- from 256 a plane and its half spectrum no longer fit the LDS of one workgroup -- and
 * `res` = the `levels` (1..6) level sizes, consecutive powers of two from shu_lowest_res >= 4 up to `size`; gauss / out / g and the
 * stride arrays have `levels` entries in that order.  Spectra are [N,2C,size,size/2+1], DC on row size/2 - 1, scale 1/size^2.
 * shg_shu_spectral_n_f32 takes any P % 4 == 0 (a last partial tile of 64 positions is guarded).  The transpose of
 * shg_shu_rfft2_shift_n_f32 is shg_shu_split_irfft2_n_f32 with one level and the table (1/c_k)/size^2 (c_0 = c_{size/2} = 1, else 2). */
int shg_shu_rfft2_shift_n_f32(const float* x, long x_batch_stride, float* T, int N, int C, int size, void* stream);
int shg_shu_spectral_n_f32(const float* T, const float* w0p, const float* b0, const float* w1p, const float* cw, float* S,
                           int N, int C2, int P, int bands, void* stream);
int shg_shu_split_irfft2_n_f32(const float* Y, const float* cw, const float* const* gauss, float* const* out,
                               const long* out_batch_stride, int N, int C, int bands, int accumulate, int size, const int* res,
                               int levels, void* stream);
int shg_shu_split_adjoint_n_f32(const float* const* g, const long* g_batch_stride, const float* const* gauss, float* GS, int N, int C,
                                int size, const int* res, int levels, void* stream);

/* ---- A24: eval composite (lib/experiments/shgan_default.py:257-262): x4 [N,4,H,W], img [N,3,H,W] -> u8 [N,3,H,W]. */
int shg_composite_u8(const float* x4, const float* img, uint8_t* out, int N, int H, int W, void* stream);

/* ---- Pluralistic sampling: K completions per masked input (model_zoo/comodgan.py Generator.sample_many; csrc/plural.hip).
 * Expansion: one launch writes dst[n*K + k] = src[n] (n < N, k < K) for every level of a table in DEVICE memory -- x_global and the
 *   encoder's skip features, so that synthesis row n*K + k reads input n.  src holds N images of `bytes` bytes each, dst N*K of them;
 *   any element type: a level moves in the widest unit of 16 / 8 / 4 / 2 / 1 bytes that divides `bytes` and both addresses.  A level
 *   with a null pointer or bytes <= 0 is skipped.  max_bytes_per_image (>= the largest level) sizes the grid only.  K = 1 is a copy.
 * Composite: x4 [N,4,H,W], img [N*K,3,H,W] -> u8 [N*K,3,H,W], shg_composite_u8's arithmetic and shape domain; row r takes the mask and
 *   the known pixels of input r / K. */
typedef struct {
    const void* src;
    void* dst;
    long bytes; /* per image */
} shg_expand_level;
int shg_plural_expand(const shg_expand_level* levels, int n_levels, int N, int K, long max_bytes_per_image, void* stream);
int shg_plural_composite_u8(const float* x4, const float* img, uint8_t* out, int N, int K, int H, int W, void* stream);

/* ---- input hand-off of the eval loop (lib/experiments/shgan_default.py:267-274): x = cat([mask-0.5, real*mask]).
 * real [N,3,H,W] in [-1,1], mask [N,H,W] in {0,1} -> x [N,4,H,W]. */
int shg_assemble_input_f32(const float* real, const float* mask, float* x, int N, int H, int W, void* stream);
/* The same from decoded uint8 pixels (ds_ffhq.py:307-347 + shgan_default.py:267-274): real [N,3,H,W] uint8, lut [256] = the float value of
 * every code as the host formatter computes it (torch: u8.float().div(255)*2-1), so the result equals the host route bit for bit. */
int shg_assemble_input_u8(const uint8_t* real, const float* mask, const float* lut, float* x, int N, int H, int W, void* stream);

/* ---- next row N2: freeform-mask rasteriser (lib/data_factory/ds_ffhq.py:145-217).  The host makes the random draws in the
 * reference's order and emits 8-word int32 records per mask (RECT / DISC / QUAD + 4 EDGE / POINT, see csrc/mask_raster.hip);
 * the device draws them exactly as Pillow's ImageDraw.line(width) / ellipse would.  records [total][8], offsets [B+1],
 * flips [B][2], disc_table [max_half+1][2*max_half+1][2]; mask [B,1,s,s] (1 keep / 0 hole), holes [B] += hole pixel counts
 * (zero it first).  s: multiple of 32 in [32, 1024]. */
int shg_mask_raster_f32(const int* records, const int* offsets, const int* flips, const int* disc_table, int max_half, float* mask,
                        int* holes, int B, int s, void* stream);
/* The same with content boxes (OpenImages' FreeFormMaskFormatter, ds_openimages.py:148-166): boxes [B][2] = (h', w') int32 (device);
 * keep (1.0) is written at every x >= w' or y >= h'.  holes counts the mask BEFORE this fill (RandomMask's rejection loop). */
int shg_mask_raster_box_f32(const int* records, const int* offsets, const int* flips, const int* disc_table, int max_half, const int* boxes,
                            float* mask, int* holes, int B, int s, void* stream);

/* ---- LaMa thin / medium / thick masks (lib/data_factory/lama_mask_utils.py behind LamaMaskFormatter, ds_ffhq.py:352-381): the
 * rasteriser of cv2.line(thickness > 1) -- OpenCV's ThickLine in 16.16 fixed point -- and of the box generator's rectangles, one
 * workgroup per mask (csrc/mask_lama.hip).  Records of 8 int32 words: RECT (0, x0, x1, y0, y1) = columns [x0, x1) of rows [y0, y1);
 * LINE (1, x0, y0, x1, y1, t, dpx, dpy) with dp = the 16.16 quad offset (cvRound(dy r), cvRound(dx r)) computed by the host.
 * records_host / offsets_host are the HOST copies of records [total][8] / offsets [B+1] (device): every record is checked from them
 * before the launch (type, |coordinate| <= 2048, t in [2, 1023], (t + 1) >> 1 <= rmax).  circle_table [rmax+1][rmax+1] (device): half
 * width of row |j| of the filled circle of radius r, -1 = none.  mask [B,1,s,s] (1 keep / 0 hole, 16-byte aligned), holes [B] = hole
 * pixel counts, WRITTEN (no zeroing needed).  s: multiple of 32 in [32, 512].  Not checked against cv2 itself. */
int shg_mask_lama_f32(const int* records_host, const int* offsets_host, const int* records, const int* offsets, const int* circle_table,
                      int rmax, float* mask, int* holes, int B, int total, int s, void* stream);

/* ---- next row N1: FID statistics (lib/evaluator/eva_fid.py:251-263).  S [DP,DP] float64 += sum_b w_b [x_b,1][x_b,1]^T on the
 * fp64 matrix cores: S[:D,:D] = sum x x^T, S[:D,D] = sum x, S[D,D] = count (tiles on / above the diagonal only).
 * feats [B,D] float32 (float64 when is_f64), weights [B] or NULL, DP >= D+1 a multiple of 32. */
int shg_fid_accumulate_f64(const void* feats, int is_f64, const float* weights, double* S, int B, int D, int DP, void* stream);

/* ---- FID detector: the feature extractor of Inception-v3 `inception-2015-12-05` (eva_fid.py:30,145-158), float32 NCHW
 * (sh-gan_amd/inception.py drives it; csrc/inception.hip).
 * shg_inception_frontend_f32: x [B,3,H,W] -> y [B,3,299,299] = (resize(v) - 128) / 128, v = lut[x] when lut [256] is given (x uint8),
 *   else x*scale + bias (x float32, two roundings); resize = TF1 legacy bilinear, source = i * size / 299, no half-pixel offset, border
 *   clamp; none when H = W = 299.
 * shg_inception_weight_prep_f32: BN-folded w [O,I,kh,kw], bias [O] -> wp [Kp][Np] (shg_inception_packed_weight_elems floats, Kp = I*kh*kw
 *   rounded up to 16, Np = O rounded up to 64, k = (ky*kw + kx)*I + c, zero outside), bp [Np]; once per detector.
 * shg_inception_conv_f32: G <= SHG_INC_MAX_GROUPS independent convolutions in one launch, each y[:, y_coff:y_coff+O] =
 *   relu(conv2d(x[:, x_coff:x_coff+I], w, stride (sh,sw), pad (ph,pw)) + bias) on exact-fp32 MFMA; x [B][x_ctot][H][W],
 *   y [B][y_ctot][OH][OW], kernel <= 7 x 7, stride 1 or 2, pad < kernel, w 16-byte aligned.  splitk > 1 splits K over that many
 *   workgroups, partial sums in `workspace` (shg_inception_conv_workspace_bytes; 0 when no group splits) added in split order.
 * shg_inception_pool_f32: 3 x 3 pool of x [B,C,H,W] into y[:, y_coff:y_coff+C] of [B,y_ctot,OH,OW]; mode 0 max, 1 average over the
 *   in-bounds taps (count_include_pad=False); stride 1 or 2, pad 0 or 1.
 * shg_inception_mean_f32: y [B,C] = mean of x [B,C,HW] over HW (fixed summation order: independent of B). */
#define SHG_INC_MAX_GROUPS 8
typedef struct {
    const float* x; const float* w; const float* bias; float* y;
    int I, H, W, x_ctot, x_coff;
    int O, kh, kw, sh, sw, ph, pw, OH, OW, y_ctot, y_coff;
    int splitk;
} shg_inc_conv_desc;
int shg_inception_frontend_f32(const void* x, const float* lut, float scale, float bias, float* y, int B, int H, int W, void* stream);
long shg_inception_packed_weight_elems(int O, int I, int kh, int kw);
int shg_inception_weight_prep_f32(const float* w, const float* bias, float* wp, float* bp, int O, int I, int kh, int kw, void* stream);
size_t shg_inception_conv_workspace_bytes(const shg_inc_conv_desc* groups, int G, int B);
int shg_inception_conv_f32(const shg_inc_conv_desc* groups, int G, int B, void* workspace, size_t ws_bytes, void* stream);
int shg_inception_pool_f32(const float* x, float* y, int B, int C, int H, int W, int mode, int stride, int pad, int y_ctot, int y_coff, void* stream);
int shg_inception_mean_f32(const float* x, float* y, int B, int C, int HW, void* stream);
/* shg_inception_head_f32: the detector's classifier output (return_features=False): probs [B,C] = softmax(feats [B,D] . w [C,D]^T
 *   (+ bias [C]; NULL = no_output_bias)) in one launch, one workgroup per image, fp32 FMA; D a multiple of 4, 4 (C + D) + 32 bytes of LDS <= 64 KiB,
 *   feats and w 16-byte aligned. */
int shg_inception_head_f32(const float* feats, const float* w, const float* bias, float* probs, int B, int C, int D, void* stream);

/* ---- KID and Inception Score (lib/evaluator/stylegan_metrics/kernel_inception_distance.py:34-44, inception_score.py:30-36;
 * sh-gan_amd/kid.py and inception_score.py drive them; csrc/kid.hip).
 * shg_kid_sums_f64: fake [n_f,D], real [n_r,D] (float32, float64 when is_f64; 16-byte aligned; D >= 64, a multiple of 4), idx_f / idx_r
 *   [S,m] int32 = the rows of subset s on each side (m >= 2, S <= 65535) -> out [S,3] float64 = { sum_{i!=j} k(x_i,x_j),
 *   sum_{i!=j} k(y_i,y_j), sum_{i,j} k(x_i,y_j) }, k(u,v) = (u.v / D + 1)^3, x / y the gathered fake / real rows.  fp64 MFMA on 64 x 64
 *   tiles, rows gathered through the index table while staged, the symmetric terms on the upper triangle only; one partial sum per tile
 *   in `workspace` (shg_kid_workspace_bytes; 0 for invalid arguments), added per subset in a fixed order by a second launch: no atomics,
 *   the same bits run to run and whichever subsets share the launch.  An index outside [0, n) makes its subset's sums NaN.
 * shg_is_accumulate_f64: acc [num_splits, C+2] float64 += a batch of probs [B,C] float32; split [B] int32 names each image's split
 *   (negative = skip).  Columns 0..C-1 = sum_i p_ic, column C = sum_i sum_c p_ic log p_ic (p == 0 contributes 0), column C+1 = the image
 *   count.  Fixed order over the batch, no atomics. */
size_t shg_kid_workspace_bytes(int S, int m);
int shg_kid_sums_f64(const void* fake, const void* real, int is_f64, int n_f, int n_r, int D, const int* idx_f, const int* idx_r, int S, int m,
                     void* workspace, size_t ws_bytes, double* out, void* stream);
int shg_is_accumulate_f64(const float* probs, const int* split, double* acc, int B, int C, int num_splits, void* stream);

/* ---- The streaming pass of the linear SVM behind U-IDS / P-IDS (CoModGAN's inception discriminative scores; sh-gan_amd/ids_score.py
 * drives it; csrc/svm.hip).  q = X~^T phi(X~ v) with X~ = [X, 1] over the rows of x0 [n0,D] (label y0) and, optionally, x1 [n1,D]
 * (label y1; null with n1 = 0): float32 rows at a pitch of ld0 / ld1 >= D floats, 1 <= D <= 4096, fewer than 2^31 rows, read ONCE, every
 * product and sum in float64.  v [D+1] float64 (the intercept's entry last).  Per row t_i = x~_i . v, then
 *   mode 0 (grad): z [n0+n1] float64 = t_i and a [n0+n1] bytes = [1 - y_i t_i > 0] are written; s_i = -2 C y_i a_i (1 - y_i t_i);
 *   mode 1 (hv):   a is read; s_i = 2 C a_i t_i; z = t_i is written unless z is null.
 * q [D+2] float64 = sum_i s_i x~_i (D+1 entries), then the loss sum_i a_i (1 - y_i t_i)^2 (mode 0; 0 in mode 1).  One partial of D+2
 *   doubles per workgroup in `workspace` (shg_svm_pass_workspace_bytes; 0 for invalid sizes), added in a fixed order by a second launch:
 *   no atomics, and the partition of the rows depends on (n0+n1, D) only -- the same bits on every run.  16-byte loads when D and both
 *   pitches are multiples of 4 and both bases 16-byte aligned, dword loads otherwise; no load reaches past column D of a row.  Rows
 *   4-byte, float64 operands 8-byte aligned.  C must be positive and finite, y0 and y1 finite (any values: +1 / -1 for the SVM). */
size_t shg_svm_pass_workspace_bytes(long n0, long n1, int D);
int shg_svm_pass_f64(const float* x0, long n0, long ld0, double y0, const float* x1, long n1, long ld1, double y1, int D, int mode, double C,
                     const double* v, double* z, unsigned char* a, double* q, void* workspace, size_t ws_bytes, void* stream);

/* ---- Square float64 GEMM on the fp64 MFMA, the device tail of FID (sh-gan_amd/fid_stats.py drives it; csrc/gemm_f64.hip).
 * shg_gemm_f64: C[b] = alpha A[b] B[b] + beta_diag I for b < batch (1..65535): n x n float64 (1 <= n <= 46336), row-major at pitches
 *   lda, ldb, ldc >= n doubles; entry b of an operand starts stride_x * b doubles after entry 0 (any sign, 0 shares an input; stride_c
 *   != 0 when batch > 1).  C must not overlap A or B.  128 x 128 tiles of C, K staged through LDS in chunks of 16; any n: loads outside
 *   the matrices read as 0, nothing beside C[:n,:n] is written.  16-byte loads when A, B are 16-byte aligned and lda, ldb and (batch > 1)
 *   stride_a, stride_b are even, 8-byte loads otherwise: the same bits either way.  Operands 8-byte aligned.
 *   partials: NULL, or [batch][2][shg_gemm_f64_tiles(n)] doubles: per tile (row-major over the tile grid) the sum of the diagonal
 *   entries and the sum of the squared entries of C as stored; adding a row in a fixed order gives tr C[b] and |C[b]|_F^2.  No atomics:
 *   the same bits on every run.
 * shg_gemm_f64_tiles(n): ceil(n / 128)^2; 0 for an n that is not served. */
int shg_gemm_f64_tiles(int n);
int shg_gemm_f64(const double* A, const double* B, double* C, int n, long lda, long ldb, long ldc, double alpha, double beta_diag, int batch,
                 long stride_a, long stride_b, long stride_c, double* partials, void* stream);

/* ---- Improved precision / recall, `pr50k3_full` (lib/evaluator/stylegan_metrics/precision_recall.py:19-60; sh-gan_amd/
 * precision_recall.py drives them; csrc/pr.hip).  Rows are fp16 [n,D], 16-byte aligned, D >= 64 a multiple of 8.  d16(i,j) = the
 *   Euclidean distance as sqrt(max(0, |a|^2 + |b|^2 - 2 a.b)) -- a.b on the fp16 MFMA (exact products, fp32 sums), fp32 row norms --
 *   rounded ONCE to fp16.
 * shg_pr_radii_f16: radii_out [n] fp16 = the (k + 1)-th smallest d16(j, .) over all n rows, j itself included (line 53);
 *   1 <= k <= 15, n >= k + 1; workspace of shg_pr_workspace_bytes(n, n, k).
 * shg_pr_inside_f16: inside_out [m] uint8 = 1 when some manifold row j has d16(p, j) <= radii[j], compared as fp16 values (line 58);
 *   m >= 1, n >= 2; workspace of shg_pr_workspace_bytes(m, n, 0).
 *   A workgroup owns 128 points and sweeps a slice of the other side on 128 x 128 MFMA tiles; a point's k + 1 smallest distances (its
 *   flag) stay in registers, no distance reaches memory; one partial result per slice in `workspace`, merged in slice order by a
 *   last launch.  The slice count follows the swept side's row count alone.  No atomics: the same bits run to run.
 * shg_pr_workspace_bytes(m, n, k): k >= 1 the radii call on n rows (m is not read), k == 0 the inside call; 0 for invalid arguments. */
size_t shg_pr_workspace_bytes(int m, int n, int k);
int shg_pr_radii_f16(const void* feats, int n, int D, int k, void* workspace, size_t ws_bytes, void* radii_out, void* stream);
int shg_pr_inside_f16(const void* probes, int m, const void* manifold, int n, int D, const void* radii, void* workspace, size_t ws_bytes,
                      unsigned char* inside_out, void* stream);

/* ---- VGG16 up to fc2, the detector of `pr50k3_full` (precision_recall.py:64-76; sh-gan_amd/vgg16.py drives it; csrc/vgg16.hip).  The
 * 13 convolutions run on shg_inception_conv_f32 after shg_inception_weight_prep_f32, fc1 / fc2 on shg_dense_f32.
 * shg_vgg16_frontend_f32: x [B,3,H,W] -> y [B,3,224,224] = (area(v) - mean[c]) / std[c]; v as shg_inception_frontend_f32 (lut [256]
 *   for uint8 x, else x*scale + bias); area = F.interpolate(mode='area'): the mean over the bin [floor(i*H/224), ceil((i+1)*H/224)) on
 *   each axis, exact bins for any ratio; mean / std [3] host floats, std > 0.
 * shg_vgg16_maxpool2_f32: y [B,C,H/2,W/2] = 2 x 2 max pool, stride 2, of x [B,C,H,W] (floor: an odd last row / column is dropped). */
int shg_vgg16_frontend_f32(const void* x, const float* lut, float scale, float bias, const float* mean, const float* stdv, float* y, int B,
                           int H, int W, void* stream);
int shg_vgg16_maxpool2_f32(const float* x, float* y, int B, int C, int H, int W, void* stream);

/* ---- LPIPS, AlexNet backbone: `lpips.LPIPS(net='alex')` as lib/evaluator/eva_lpips.py:39-52 calls it (sh-gan_amd/lpips.py drives it;
 * csrc/lpips.hip).  conv2..conv5 and the max pools run on the detector's convolution and pool entry points above.
 * Conv1 weight prep: w [64,3,11,11], bias [64] -> wp [SHG_LPIPS_CONV1_WP_ELEMS] floats, bp [64] in the layout of
 *   shg_inception_weight_prep_f32 for (O, I, kh, kw) = (64, 3, 11, 11), a kernel size that entry point itself refuses: [368][64],
 *   k = (ky*11 + kx)*3 + c, zero rows beyond K = 363; once per network.
 * Conv1: x [B,3,H,W] -> y [B,64,OH,OW] = relu(conv2d(s(v), w, stride 4, pad 2) + bias), OH = (H + 4 - 11) / 4 + 1, H and W >= 7, on
 *   exact-fp32 MFMA.  v = lut[x] when lut [256] is given (x uint8), else ((x*scale + bias) - 0.5) * 2 with every step rounded to float32
 *   (x float32; x*scale + bias is the evaluator batch's [0, 1] form, the rest eva_lpips.py:39-40); s(v) = (v - shift[c]) * float32(1 /
 *   scaling[c]), the LPIPS scaling layer, on in-bounds taps only (the zero padding is of the scaled image).  shift, scaling: HOST
 *   arrays of 3 floats; wp 16-byte aligned.
 * Head, for one tap: fp, fg [B,C,h,w] (features of the B preds and the B gts), w [C] -> out[b] += mean over pixels of
 *   sum_c w[c] (fp/(sqrt(sum_c fp^2) + 1e-10) - fg/(sqrt(sum_c fg^2) + 1e-10))^2, out float64 [B].  scratch: the number of bytes the
 *   scratch query returns (0 for invalid arguments): per-tile float64 partial sums, added per image in a fixed order -- no atomics,
 *   the same bits run to run and in any batch. */
#define SHG_LPIPS_CONV1_WP_ELEMS (368 * 64)
int shg_lpips_conv1_weight_prep_f32(const float* w, const float* bias, float* wp, float* bp, void* stream);
int shg_lpips_conv1_f32(const void* x, const float* lut, float scale, float bias, const float* shift, const float* scaling, const float* wp,
                        const float* bp, float* y, int B, int H, int W, void* stream);
size_t shg_lpips_head_scratch_bytes(int B, int h, int w);
int shg_lpips_head_f32(const float* fp, const float* fg, const float* w, int B, int C, int h, int wd, void* scratch, size_t scratch_bytes,
                       double* out, void* stream);
/* Pair form of the head (sh-gan_amd/diversity.py): f [M,C,h,w], device tables ia, ib int32 [P], w [C] -> out[p] += the head's value for
 *   the pair (f[ia[p]], f[ib[p]]), out float64 [P]; P <= 65535.  The arithmetic, the fixed summation order and the scratch layout are
 *   shg_lpips_head_f32's: a pair's bits equal that entry point's on the two rows and depend neither on P nor on the pair's place in the
 *   table; ia[p] == ib[p] adds exactly 0.  ia_host / ib_host: optional HOST copies of the tables (both or neither); with them an index
 *   outside [0, M) is SHG_ERR_ARG and nothing is launched.  Without them (tables that exist on the device only) the kernel clamps such
 *   an index into [0, M) and stores 1 into *err (device int, may be null; the caller zeroes it): no read leaves f in either case. */
size_t shg_lpips_head_pairs_scratch_bytes(int P, int h, int w);
int shg_lpips_head_pairs_f32(const float* f, const int* ia, const int* ib, const int* ia_host, const int* ib_host, const float* w, int M, int P,
                             int C, int h, int wd, void* scratch, size_t scratch_bytes, double* out, int* err, void* stream);

/* The scaling layer as a pass of its own, for a backbone whose first convolution is not conv1 above (net = 'vgg', sh-gan_amd/lpips.py):
 * x [B,3,H,W] uint8 (lut [256]) or float32 -> y [B,3,H,W] float32 = s(v), v and s as in conv1 (same float32 steps, same host arrays). */
int shg_lpips_scaling_f32(const void* x, const float* lut, float scale, float bias, const float* shift, const float* scaling, float* y, int B,
                          int H, int W, void* stream);

/* ---- LPIPS as a training loss (sh-gan_amd/lpips.py: Lpips.loss; csrc/lpips_bwd.hip): the backward pass of the frozen network with
 * respect to the pred image.  Current stream, no atomics, no host synchronisation, fixed summation orders.  ONE masking rule: whoever
 * writes a gradient into the buffer of a post-ReLU activation y selects it by y > 0 itself (a select, never a multiply).
 * shg_lpips_dgrad_f32: input gradient of a stride-1 k x k convolution at pad = k / 2 (odd k <= 7) on the detector's exact-fp32 MFMA tile:
 *   dx [B,O,H,W] = conv2d(g [B,I,H,W], wt, pad) with wt [O,I,k,k] = w.transpose(0,1).flip(2,3) packed by shg_inception_weight_prep_f32
 *   (16-byte aligned); no bias, no ReLU; ymask [B,O,H,W] given: dx = ymask > 0 ? dx : 0; NULL: stored as it is.  K is never split.
 * shg_lpips_maxpool_bwd_f32: k x k (k = 2 or 3), stride 2, floor max pool of x [B,C,H,W] (a post-ReLU activation), gy [B,C,OH,OW],
 *   OH = (H - k) / 2 + 1: dx = x > 0 ? sum of gy over the windows whose first maximum in row-major order the element is : 0.
 * shg_lpips_head_bwd_f32: one tap's distance head.  f, fr [B,C,h,w] (pred / real tap), w [C], g [B] -> df [B,C,h,w]: per position
 *   s = sqrt(sum f^2), a = 1 / (s + 1e-10), q_c = 2 w_c (a f_c - fr_c / (|fr| + 1e-10)) g_b / (h w),
 *   v_c = f_c > 0 ? a q_c - f_c a^2 (sum_j q_j f_j) / s : 0 (an all-zero tap vector gives exact zeros); df = v or, accumulate != 0, df + v.
 * shg_lpips_conv1_pm1_f32 / shg_lpips_scale_pm1_f32: shg_lpips_conv1_f32 / shg_lpips_scaling_f32 for a float32 image v in [-1, 1] that
 *   enters the scaling layer as it is, s(v) = (v - shift[c]) * float32(1 / scaling[c]) (HOST arrays of 3 floats).
 * shg_lpips_conv1_dgrad_f32: g [B,64,OH,OW], w [64,3,11,11] (the caller folds 1 / scaling[c] in) -> dx [B,3,H,W], the transposed 11 x 11
 *   stride 4 pad 2 convolution; pixels that no window reaches get 0.
 * shg_l1_mean_f32: out [B] float32 = mean |a - b| over the n elements of image b (float64, fixed order, rounded once; one launch).
 * shg_l1_mean_bwd_f32: dx [B,n] = sign(a - b) g[b] / n (sign(0) = 0). */
int shg_lpips_dgrad_f32(const float* g, const float* wp, const float* ymask, float* dx, int B, int I, int O, int H, int W, int k, int pad,
                        void* stream);
int shg_lpips_maxpool_bwd_f32(const float* x, const float* gy, float* dx, int B, int C, int H, int W, int k, void* stream);
int shg_lpips_head_bwd_f32(const float* f, const float* fr, const float* w, const float* g, float* df, int B, int C, int h, int wd, int accumulate,
                           void* stream);
int shg_lpips_conv1_pm1_f32(const float* x, const float* shift, const float* scaling, const float* wp, const float* bp, float* y, int B, int H, int W,
                            void* stream);
int shg_lpips_scale_pm1_f32(const float* x, const float* shift, const float* scaling, float* y, int B, int H, int W, void* stream);
int shg_lpips_conv1_dgrad_f32(const float* g, const float* w, float* dx, int B, int H, int W, void* stream);
int shg_l1_mean_f32(const float* a, const float* b, float* out, int B, long n, void* stream);
int shg_l1_mean_bwd_f32(const float* a, const float* b, const float* g, float* dx, int B, long n, void* stream);

/* ---- Perceptual path length (`ppl2_wend`, lib/evaluator/stylegan_metrics/perceptual_path_length.py; sh-gan_amd/ppl.py drives it;
 * csrc/ppl.hip): the sampler's image front end (:71-85) in one pass over the synthesis output.  x [N,C,H,W] float32 in [-1, 1], C = 1
 * or 3, H == W -> y [N,3,S,S] float32:
 *   crop (0 / 1): the window rows [3c, 7c), columns [2c, 6c), c = H / 8 (:72-75), else the whole image;
 *   factor = img_resolution / 256 (:78): the mean over factor x factor boxes, S = side / factor; 0 and 1 copy; the side must be
 *     divisible by the factor (the reference's reshape throws otherwise);
 *   m = that mean rounded to float32 (the box is summed in float64: the correctly rounded mean up to a double rounding), then in
 *     float32 u = (m + 1) * 127.5 (:83) and y = (u - mean[c]) / std[c], each step rounded once; a single-channel image is repeated to
 *     three (:84-85) with each channel's own mean / std.  mean, std: HOST arrays of 3 floats, std > 0 (as shg_vgg16_frontend_f32).
 * One thread per group of 4 / factor output pixels of a row reading float4 rows when factor is 1, 2 or 4, H % 4 == 0, the window's first
 * column % 4 == 0, S divisible by the group and x, y 16-byte aligned; one output pixel per thread with scalar loads otherwise -- the
 * same bits either way.  Every element of y is written exactly once; nothing outside the window is read.  C not in {1, 3}, H != W, an
 * empty window, factor outside 0..256 or a side the factor does not divide: SHG_ERR_ARG, nothing launched. */
int shg_ppl_frontend_f32(const float* x, float* y, int N, int C, int H, int W, int factor, int crop, const float* mean, const float* stdv,
                         void* stream);

/* ---- training tail on the gradient buckets (sh-gan_amd/optim.py drives it; csrc/optim.hip): gradient average + sanitisation + Adam
 * (lib/experiments/stylegan_default.py:159-166 with torch.optim.Adam, weight_decay 0, amsgrad off) and the G_ema update (:383-390).
 * Tables are int64 arrays ON THE DEVICE, one row per segment (= one parameter) plus a sentinel row; the last column of a row is the
 * segment's first chunk (a chunk = SHG_OPT_CHUNK consecutive elements of one segment, a segment of n elements has ceil(n / chunk)),
 * the sentinel's is the total, which is also passed as `chunks`.  The tables hold raw device addresses: the caller guarantees that
 * every range lies inside its allocation (optim.py checks that on the host before a launch).
 * Adam row, SHG_ADAM_ROW int64: {param, grad, exp_avg, exp_avg_sq addresses (4-byte aligned; grad, exp_avg and exp_avg_sq congruent
 *   mod 16), numel, touched flag, scalar slot, hyper-parameter group, 0, first chunk}.
 * Tick: for every touched row steps[slot] += 1 (float32 counter, as torch's capturable Adam keeps it) and scalars[slot *
 *   SHG_ADAM_SCALARS ..] = {lr / (1 - beta1^t), 1 / sqrt(1 - beta2^t), 1 - beta1, beta2, 1 - beta2, eps} computed in float64 from
 *   hyper [ngroups][4] = {lr, beta1, beta2, eps} (float64) and rounded to float32.  One small workgroup, no host read.
 * Stream: per element g = grad averaged over `world` ranks (div_mode 0: left as it is, 1: times float32(1 / world) -- what torch's
 *   div_ by a host scalar computes on the device --, 2: divided by world), then if `sanitize` NaN -> 0, +inf -> 1e5, -inf -> -1e5, written
 *   back to grad; for touched rows m = lerp(m, g, 1 - beta1) (torch's two-form lerp), v = beta2 v + (1 - beta2) g^2,
 *   p -= step_size * m / (sqrt(v) * bc2 + eps).  Rows that are not touched keep param, exp_avg, exp_avg_sq and their step bit for bit.
 * EMA row, SHG_EMA_ROW int64: {dst, src addresses (4-byte aligned), 32-bit words, kind (0: dst = lerp(src, dst, beta[0]) in float32,
 *   1: dst = src, words copied as they are), 0, first chunk}; beta: one float32 on the device. */
#define SHG_OPT_CHUNK 4096
#define SHG_ADAM_ROW 10
#define SHG_ADAM_SCALARS 8
#define SHG_EMA_ROW 6
int shg_adam_tick(const long* table, int nseg, const double* hyper, int ngroups, float* steps, float* scalars, void* stream);
int shg_adam_buckets_f32(const long* table, int nseg, long chunks, const float* scalars, float world, int div_mode, int sanitize, void* stream);
int shg_ema_lerp_f32(const long* table, int nseg, long chunks, const float* beta, void* stream);

/* ---- what a training run keeps beside the step (sh-gan_amd/training_stats.py, optim.py, train_stage.py; csrc/train_stats.hip and the
 * health form of the Adam pass in csrc/optim.hip).  No atomics, no host read; every reduction has a shape fixed by its data (lane-strided
 * partial sums, a tree over the wave, a tree over the four waves), so equal inputs give equal bits.
 * Moments: table int64 [rows + 1][SHG_STATS_ROW] on the device, row = {address of a contiguous float32 tensor (4-byte aligned), numel >= 1,
 *   slot in [0, slots), 0}, the last row a sentinel; acc float64 [slots][4] += {count, sum, sum of squares} of the finite elements (each
 *   widened to float64 before it is squared) and {non-finite count}.  One workgroup per slot walks that slot's rows in table order.
 *   rows = 0 launches nothing.  The table is checked on the host (training_stats.validate_stats_table) and trusted here.
 * Adam with health: shg_adam_buckets_f32's pass (same table, same bits in param, exp_avg, exp_avg_sq and grad), which also writes
 *   workspace float64 [chunks][SHG_HEALTH_COLS] for the chunks of touched segments: {sum g^2 of the averaged, sanitised gradient, elements the
 *   sanitisation replaced (0 with sanitize off), max |g|, sum p_old^2, sum (p_old - p_new)^2 with the difference taken in float32}.
 * Reduce: one workgroup per segment folds its chunk rows into health float64 [nseg + 1][SHG_HEALTH_COLS] (sums added, the maximum kept), one
 *   more folds every touched chunk into row nseg and adds 1 to steps[0]; untouched segments are left alone.
 * Grid: x [gw * gh, C, H, W] float32, C 1 or 3 -> out uint8 [gh * H, gw * W, C], image n at row n / gw, column n % gw;
 *   value = (uint8) clip(rint((x - lo) * scale), 0, 255), subtract and multiply rounded one by one in float32, rint to even, NaN -> 0; with
 *   real [like x] and mask [gw * gh, 1, H, W] (both or neither) x is first replaced by real * mask + x * (1 - mask), each operation rounded. */
#define SHG_STATS_ROW 4
#define SHG_HEALTH_COLS 5
int shg_stats_moments_f64(const long* table, int rows, double* acc, int slots, void* stream);
int shg_adam_buckets_health_f32(const long* table, int nseg, long chunks, const float* scalars, float world, int div_mode, int sanitize,
                                double* workspace, void* stream);
int shg_health_reduce_f64(const long* table, int nseg, long chunks, const double* workspace, double* health, double* steps, void* stream);
int shg_image_grid_u8(const float* x, const float* real, const float* mask, uint8_t* out, int C, int H, int W, int gw, int gh, float lo,
                      float scale, void* stream);

/* ---- evaluation image metrics (lib/evaluator/eva_psnr.py, for_dataset=None, rgb_range=1; eva_ssim._ssim, size_average=False).
 * pred, gt [B,C,H,W] contiguous; each operand is uint8 when its lut [256] (value of every code: float64 for pred, float32 for gt) is
 * given, float32 otherwise; the element value is then v*scale + bias (the evaluator's fake/255 and (real+1)/2).  As in the reference's
 * evaluator batch, PSNR takes pred in float64 and gt in float32; SSIM takes both in float32.  psnr [B] = -10 log10(mean (pred-gt)^2), +inf
 * when the mean is 0; ssim [B] = mean of the SSIM map (window_size-tap Gaussian, sigma 1.5, zero padding window_size/2, C1 = 0.01^2,
 * C2 = 0.03^2).  window_size odd in [1, 31]; psnr_only skips SSIM (ssim may be NULL).  scratch: shg_image_metrics_scratch_bytes
 * bytes (per-tile fp64 partial sums, reduced per image in a fixed order: results are bitwise reproducible and independent of the
 * batch an image sits in).  shg_image_metrics_scratch_bytes returns 0 for invalid arguments. */
size_t shg_image_metrics_scratch_bytes(int B, int H, int W, int window_size);
int shg_image_metrics(const void* pred, const double* pred_lut, float pred_scale, float pred_bias, const void* gt, const float* gt_lut,
                      float gt_scale, float gt_bias, int B, int C, int H, int W, int window_size, int psnr_only, void* scratch,
                      size_t scratch_bytes, double* psnr, double* ssim, void* stream);

/* ---- Places2 evaluation input: FixResolutionLoader's PIL Image.resize([R, R], BICUBIC) (ds_places2.py:90-103) of a ragged batch, 8 bits
 * per channel, bit-exact to Pillow, + the formatter's horizontal flip of the resized image (FreeFormMaskFormatter, :214-229).
 * src: src_bytes bytes holding B HWC RGB uint8 images back to back; dst: uint8 [B,3,R,R].  table: device int32 [table_elems] = B
 * descriptors of 12 ints {h, w, byte offset in src, flip, h-bounds, h-coefs, KH, v-bounds, v-coefs, KV, band rows, column chunk} followed
 * by the per-axis fixed-point tables they point at (bounds [R][2] = first tap, taps; coefficients [R][K], 22 fractional bits; layout and
 * builder: sh-gan_amd/resize.py).  Grid chunks x bands x B: every image's R / column chunk and R / band rows must not exceed them;
 * lds_bytes (<= 49152) >= 3 x (source rows of a band) x (column chunk rounded up to 4) for every band.  A
 * descriptor or tap range outside src / table leaves that image's bytes unwritten (never an out-of-bounds access). */
int shg_resize_bicubic_u8(const void* src, long src_bytes, const int* table, long table_elems, void* dst, int B, int R, int chunks, int bands,
                          int lds_bytes, void* stream);
/* OpenImages evaluation input: FixResolutionLoader of ds_openimages.py:63-81 -- each image resized (same 8-bit bicubic) to its own box
 * (h', w') <= R that keeps its aspect ratio (its own size when it fits), pasted at the top-left of a zero R x R canvas; flip mirrors the
 * whole canvas (FreeFormMaskFormatter, :148-166).  Same arguments, but descriptors of 14 ints {the 12 above, h', w'} with per-axis
 * tables of w' / h' entries (builder: resize.build_fit_table).  Every byte of dst [B,3,R,R], padding included, is written by the launch. */
int shg_resize_fit_pad_u8(const void* src, long src_bytes, const int* table, long table_elems, void* dst, int B, int R, int chunks, int bands,
                          int lds_bytes, void* stream);

/* ---- Inpainting photographs of any size (sh-gan_amd/inpaint.py drives both; csrc/inpaint.hip).  src: src_bytes bytes holding B HWC RGB
 * uint8 images back to back; mask: mask_bytes bytes holding their HW uint8 masks back to back (non-zero = known, 0 = hole).  table:
 * device int32 [table_elems] = B descriptors of 16 ints {h, w, image byte offset, mask byte offset, window y0, x0, ch, cw, h-bounds,
 * h-coefs, KH, v-bounds, v-coefs, KV, band rows, column chunk} followed by the per-axis tables they point at: bounds [n][2] = (first tap,
 * taps) and coefficients [n][K] (builders: inpaint.build_gather_table / build_paste_table).  A descriptor, window or tap range outside
 * src / mask / table / fake leaves that image's bytes unwritten (never an out-of-bounds access).
 * shg_inpaint_gather_u8: dst uint8 [B,3,R,R] = Pillow's crop(window).resize((R, R), BICUBIC) of every image, bit-exact (fixed-point
 *   tables of (cw -> R) / (ch -> R), 22 fractional bits, n = R; the source is read in place at the image's row pitch); mask_dst float32
 *   [B,1,R,R]: pixel (i, j) is 1 iff every native pixel of rows [i ch / R, max(ceil((i + 1) ch / R), lo + 1)) x the same columns is known.
 *   Grid chunks x bands x B over the R x R output; lds_bytes (<= 49152) >= 3 x (window rows of a band) x (column chunk rounded up to 4).
 * shg_inpaint_paste_u8: out uint8 [K][img_bytes], every row a copy of src on entry; fake float32 [B*K,3,R,R], row n K + k = sample k of
 *   image n.  Per window pixel p, F = feather + 1 (feather in 0..32): A = max(0, F - Chebyshev distance to the nearest hole pixel inside
 *   the window); v = fake resampled R x R -> ch x cw at p with the float32 tap tables (bit patterns in the int32 table, n = cw / ch;
 *   horizontal pass, then vertical, fused multiply-adds in tap order from 0); g = clamp(v * 127.5 + 127.5, 0, 255);
 *   out = (uint8)(int)((A g + (F - A) out) / F), every operation rounded on its own; A = 0 stores nothing.  alpha: NULL, or uint8
 *   [mask_bytes], zeroed by the caller, that receives A.  Grid chunks x bands x B over the largest window; lds_bytes (<= 49152) >=
 *   16 + align16(TB CW) + max(align16((TB + 2 feather) roundup4(CW + 2 feather)) + align16((TB + 2 feather) CW), 12 (rows of fake under a
 *   band) CW).  No atomics: an image's bytes are the same alone, in any batch and on every run. */
int shg_inpaint_gather_u8(const void* src, long src_bytes, const void* mask, long mask_bytes, const int* table, long table_elems, void* dst,
                          float* mask_dst, int B, int R, int chunks, int bands, int lds_bytes, void* stream);
int shg_inpaint_paste_u8(void* out, long img_bytes, const void* mask, long mask_bytes, const int* table, long table_elems, const float* fake,
                         void* alpha, int B, int K, int R, int feather, int chunks, int bands, int lds_bytes, void* stream);

/* ---- Gradient-domain (Poisson) paste-back (sh-gan_amd/inpaint.py paste_back_membrane; csrc/membrane.hip).  With A, g and orig of
 * shg_inpaint_paste_u8: Omega = {A > 0}; the membrane c solves 4 c(p) - sum_{q in N4(p)} c(q) = 0 in Omega with c = d = orig - g on the
 * window pixels with A = 0 and c = 0 outside the window; out = (uint8)(int)((A clamp(g + c, 0, 255) + (F - A) out) / F).
 * grids: device int32 [B][6] = {gy0, gx0, gh, gw, float offset, byte offset}: per image the solve grid (a box of the window, in window
 *   coordinates, that holds Omega's bounding box and one more ring where the window allows), the offset of its K planes [K][gh][gw][3]
 *   in g / field, and the offset of its Omega bytes [gh][gw].  A grid outside its window or its buffers leaves the image alone.
 * shg_inpaint_membrane_setup_f32: src = the packed originals; writes, inside the grids, g (the bits shg_inpaint_paste_u8 computes),
 *   field (d where A = 0, 0 in Omega) and omega (A > 0; the K samples of an image share it).  table, fake, chunks, bands, lds_bytes as
 *   shg_inpaint_paste_u8.
 * shg_membrane_solve_f32: P problems, table device int32 [P][4] = {h, w, float offset into field, byte offset into omega}, h <= max_h,
 *   w <= max_w, slices of field disjoint: field float32 [h][w][3], omega uint8 [h][w], neighbours outside the h x w grid count as 0.  On
 *   return the field holds c in Omega and is untouched elsewhere.  Multigrid V-cycles (csrc/membrane.hip) until the residual's max norm
 *   over Omega and the three channels is <= res_tol[p] (device float32 [P]): info (device int32 [P][3]) = {cycles run, bits of the last
 *   norm, state}, state 1 = certified, 2 = stalled (a cycle did not lower the norm: the float32 floor), 0 = out of max_cycles (0..1024).
 *   A fixed sequence of launches, no host synchronisation; no atomics: a problem's bits do not depend on the batch or the run.
 *   ws: ws_bytes >= shg_membrane_workspace_bytes(P, max_h, max_w) (16-byte aligned, as field); its old contents are irrelevant.
 *   A problem whose descriptor breaks a rule above is left alone with info = {0, +inf, 0}.
 * shg_inpaint_membrane_paste_u8: out, alpha, table, chunks, bands, lds_bytes as shg_inpaint_paste_u8; g and field (= c) as above.
 * shg_membrane_tile / shg_membrane_coarsest: the smoother's tile side and the largest side of a coarsest level. */
int shg_membrane_tile(void);
int shg_membrane_coarsest(void);
size_t shg_membrane_workspace_bytes(int P, int max_h, int max_w);
int shg_inpaint_membrane_setup_f32(const void* src, long img_bytes, const void* mask, long mask_bytes, const int* table, long table_elems,
                                   const int* grids, const float* fake, float* g, float* field, long g_elems, void* omega, long omega_bytes,
                                   int B, int K, int R, int feather, int chunks, int bands, int lds_bytes, void* stream);
int shg_membrane_solve_f32(float* field, long field_elems, const void* omega, long omega_bytes, const int* table, int P, const float* res_tol,
                           int max_cycles, int max_h, int max_w, void* ws, size_t ws_bytes, int* info, void* stream);
int shg_inpaint_membrane_paste_u8(void* out, long img_bytes, const void* mask, long mask_bytes, const int* table, long table_elems,
                                  const int* grids, const float* g, const float* field, long g_elems, void* alpha, int B, int K, int R,
                                  int feather, int chunks, int bands, int lds_bytes, void* stream);

/* ---- Hole groups: one window per group of holes (sh-gan_amd/inpaint.py label_holes / owner_plane / plan_windows; csrc/hole_label.hip;
 * INTEGRATION section T).  mask as above; shapes: device int32 [B][4] = {h, w, image byte offset, mask byte offset}, every h <= max_h and
 * w <= max_w.  With r = feather + 1 in 1..33: D = the pixels within Chebyshev distance r of a hole pixel of the same image; a group is an
 * 8-connected component of D and its root the smallest y w + x over its pixels.
 * shg_hole_label_i32: labels int32 [mask_bytes] = the root where the pixel lies in D, -1 elsewhere; comps int32 [max_components][8] =
 *   {image, root, ya, yb, xa, xb, hole pixels, 0} (the half-open box of the group's hole pixels), one row per group in no particular
 *   order, unused rows zero; counter int32 [2] = {groups found, flags}: bit 0 = more groups than max_components (those beyond it are
 *   missing from comps; labels is complete), bit 1 = a find / union loop ran into its cap (every loop carries one: no kernel can spin).
 *   scratch: int32 [mask_bytes], contents irrelevant.  A memset and at most four launches; integer atomics only: the same bits on every
 *   run.  An image whose descriptor points outside mask is left unwritten.
 * shg_hole_owner_u8: owner uint8 [mask_bytes] = 0 at a known pixel, at a hole pixel the key its group has in table (device int32
 *   [n_table][3] = {image, root, key in 1..255}; 0 when the table does not name the group).  labels: what shg_hole_label_i32 wrote.
 * shg_hole_label_tile: the side of the tile one workgroup labels in LDS.
 * The keyed paste-backs take `owner` where the mask went and keys (device int [B], 1..255): window b blends the holes whose owner byte is
 *   keys[b]; the rows of table / grids are per window and the windows of an image may overlap; alpha receives A only where A > 0.  With
 *   r = feather + 1 no aligned 4-byte word of out or alpha is touched by two windows.  Everything else as the forms above. */
int shg_hole_label_tile(void);
int shg_hole_label_i32(const void* mask, long mask_bytes, const int* shapes, int B, int max_h, int max_w, int r, int max_components, int* labels,
                       int* scratch, int* comps, int* counter, void* stream);
int shg_hole_owner_u8(const void* mask, long mask_bytes, const int* shapes, int B, int max_h, int max_w, const int* labels, const int* table,
                      int n_table, int* scratch, void* owner, void* stream);
int shg_inpaint_paste_keyed_u8(void* out, long img_bytes, const void* owner, long mask_bytes, const int* keys, const int* table, long table_elems,
                               const float* fake, void* alpha, int B, int K, int R, int feather, int chunks, int bands, int lds_bytes, void* stream);
int shg_inpaint_membrane_setup_keyed_f32(const void* src, long img_bytes, const void* owner, long mask_bytes, const int* keys, const int* table,
                                         long table_elems, const int* grids, const float* fake, float* g, float* field, long g_elems, void* omega,
                                         long omega_bytes, int B, int K, int R, int feather, int chunks, int bands, int lds_bytes, void* stream);
int shg_inpaint_membrane_paste_keyed_u8(void* out, long img_bytes, const void* owner, long mask_bytes, const int* keys, const int* table,
                                        long table_elems, const int* grids, const float* g, const float* field, long g_elems, void* alpha, int B,
                                        int K, int R, int feather, int chunks, int bands, int lds_bytes, void* stream);

/* ---- Training input of Places2, OpenImages and DTD: the "random scale, random crop" formatter (AdvInpaintingFormatter,
 * ds_places2.py:183-207, ds_openimages.py:117-141; InpaintingFormatter, ds_texture.py:121-149).  dst float32 [B,3,s,s]: per image the
 * window [ch:ch+s, cw:cw+s] of torch's bicubic resample (upsample_bicubic2d, align_corners = false, A = -0.75, 4 x 4 clamped taps,
 * float32 coordinates) of the image to nh x nw, flipped vertically / horizontally when the flags say so; only the window is computed.
 * A sample's value is lut[byte] (device float32 [256]).  desc / desc_dev: the same B rows of 9 ints {h, w, byte offset in src, nh, nw, ch,
 * cw, flip_v, flip_h} in host and in device memory: the host copy is checked before the launch (h, w >= 1; the image inside src;
 * nh, nw >= s; the window inside nh x nw; flags 0 / 1), the device copy is what the kernel reads.  ragged: src holds HWC RGB images of
 * their own sizes (no alignment assumed); planar: three h x w planes per image at its offset (a uint8 [B,3,H,W] tensor).  One launch;
 * no atomics: an image's window has the same bits alone and inside any batch. */
int shg_randcrop_bicubic_ragged_f32(const void* src, long src_bytes, const int* desc, const int* desc_dev, const float* lut, float* dst, int B,
                                    int s, void* stream);
int shg_randcrop_bicubic_planar_f32(const void* src, long src_bytes, const int* desc, const int* desc_dev, const float* lut, float* dst, int B,
                                    int s, void* stream);

/* ---- the ADA augmentation pipe for the critic's input (sh-gan_amd/ada.py drives it; csrc/ada.hip): StyleGAN2-ADA's AugmentPipe, blit +
 * geometry + colour categories.  shg_ada_params_f32: draws u [N,24] (uniform in [0,1)) and g [N,8] (standard normal), column layout in
 * ada.py, and the probability p (ONE float in device memory, read on the device) -> G_inv [N,3,3], the colour matrix [N,3,4] (rows 0..2 of
 * ADA's 4x4) and margins int32 [4] = {mx0, my0, mx1, my1}, the batch-wide reflect-pad extents.  One workgroup, float64 arithmetic, no host
 * synchronisation.  cfg is HOST memory (copied into the kernel arguments).
 * shg_ada_apply_f32: y = pipe(x), x and y [N,C,H,W], x != y.  geom = 1: reflect-pad by the margins -> x2 upsampling with the 12-tap sym6
 * low-pass -> bilinear resampling by G_inv (zeros outside) -> x2 decimation, fused into one launch; geom = 0: G_inv and margins are not read.
 * color_count = 3: channels [color_first, color_first + 3) become M x + t (bias = 0: M x only, the operator's linear part);
 * color_count = 1: channel color_first becomes x * mean_r(sum_c M[r][c]) + mean_r(t[r]); 0: no colour stage, Cm is not read.  Every other
 * channel passes the geometry alone.  geom = 0 and color_count = 0 together: SHG_ERR_ARG (the caller passes the tensor through).
 * shg_ada_apply_adjoint_f32: gx = A^T gy, A the linear part of the same call.  With geom = 1 gx must be ZERO on entry (float atomics
 * accumulate into it, staged through LDS); their order is not fixed, so gx is not bit-reproducible from run to run.  N * C <= 65535.
 * shg_ada_apply_adjoint_gather_f32: the same gx in gather form, the same bits on every run.  Two launches without atomics: gs = D^T C^T gy
 * on the sample grid [N,C,2H+10,2W+10] into the caller's workspace (shg_ada_adjoint_gather_workspace_bytes; device memory, contents
 * irrelevant on entry), then every source pixel sums, in a fixed order and in float64, the samples whose bilinear footprint reaches the
 * upsampled pixels it feeds (csrc/ada_geom.h: the window of a pixel is the bounding box of the inverse affine map).  gx need NOT be
 * cleared: every element is written.  Decided per sample on the device: a sample whose window half extents |M00| + |M01|, |M10| + |M11|
 * (M the inverse of the 2 x 2 part) are at most 24 and whose entries are finite and of sane size (|k| + |L| (2 (W + H) + 20) <= 2^24,
 * csrc/ada_geom.h) takes the gather; any other sample (a singular, more than ~16-fold magnifying, huge or non-finite matrix) is handled
 * by the scatter kernel launched behind it -- correct, but that sample's gradient is not bit-reproducible.  geom = 0: the colour kernel alone, workspace not read.  geom = 1 with a null or too small
 * workspace: SHG_ERR_ARG.  shg_ada_adjoint_gather_workspace_bytes: 0 for sizes the entry point rejects. */
typedef struct {
    float xflip, rotate90, xint, scale, rotate, aniso, xfrac;          /* probability multipliers, geometry */
    float brightness, contrast, lumaflip, hue, saturation;             /* probability multipliers, colour */
    float xint_max, scale_std, rotate_max, aniso_std, xfrac_std;
    float brightness_std, contrast_std, hue_max, saturation_std;
    int color_count;                                                   /* 1 or 3 (hue and saturation exist for 3 only) */
} shg_ada_config;
int shg_ada_params_f32(const float* u, const float* g, const float* p, const shg_ada_config* cfg, float* G_inv, float* Cm, int* margins,
                       int N, int H, int W, void* stream);
int shg_ada_apply_f32(const float* x, const float* G_inv, const float* Cm, const int* margins, float* y, int N, int C, int H, int W, int geom,
                      int color_first, int color_count, int bias, void* stream);
int shg_ada_apply_adjoint_f32(const float* gy, const float* G_inv, const float* Cm, const int* margins, float* gx, int N, int C, int H, int W,
                              int geom, int color_first, int color_count, void* stream);
long shg_ada_adjoint_gather_workspace_bytes(int N, int C, int H, int W);
int shg_ada_apply_adjoint_gather_f32(const float* gy, const float* G_inv, const float* Cm, const int* margins, float* gx, void* workspace,
                                     long workspace_bytes, int N, int C, int H, int W, int geom, int color_first, int color_count,
                                     void* stream);

/* ---- the tail of the ADA pipe (sh-gan_amd/ada.py: FullAugmentPipe; csrc/ada_tail.hip): ADA's image-space filter, additive noise and cutout,
 * in ADA's order, after the colour stage.  shg_ada_tail_params_f32: draws ut [N,8] (uniform in [0,1)) and gt [N,5] (standard normal), column
 * layout in ada.py, and the probability p (ONE float in device memory) -> Hz [N,43], the per-sample taps g @ Hz_fbank (the 4 x 43 sym2 bank
 * lives with the kernel); sigma [N]; cut [N,4] = {cx, cy, half_w, half_h} in units of the image size.  One workgroup, float64 arithmetic,
 * no host synchronisation; cfg is HOST memory.  A sample none of whose band gates fired gets the exact unit impulse (tap 21 = 1, the rest 0);
 * closed gates give sigma = 0 and half sizes 0.
 * shg_ada_tail_apply_f32: x, y [N,C,H,W], x != y, z [N,color_count,H,W].  On channels [color_first, color_first + color_count):
 * y = mask * (fir(x) + sigma z), fir = reflect-pad by 21, the 43 taps along x, then along y (correlations), fused in one launch through
 * LDS; on the other channels y = mask * x.  mask = |(x + 0.5) / W - cx| >= half_w or |(y + 0.5) / H - cy| >= half_h, in float32.  A null Hz,
 * z (with sigma) or cut skips that stage; all three null: SHG_ERR_ARG.  bias = 0 drops the noise term (the operator's linear part).  A
 * sample whose taps are the exact impulse is not filtered: its bits pass.  With Hz: H, W >= 22 (reflect: pad < size), else SHG_ERR_ARG.
 * shg_ada_tail_adjoint_f32: gx = A^T gy, A the linear part of the same call (not self-adjoint: the reflected pad folds back).  A gather,
 * no atomics: gx is the same bits on every run and need not be cleared. */
typedef struct {
    float imgfilter;                 /* probability multiplier of every band gate */
    float bands[4];                  /* ADA's imgfilter_bands: per-band factor of that probability */
    float imgfilter_std;
    float noise, noise_std;
    float cutout, cutout_size;
} shg_ada_tail_config;
int shg_ada_tail_params_f32(const float* ut, const float* gt, const float* p, const shg_ada_tail_config* cfg, float* Hz, float* sigma,
                            float* cut, int N, void* stream);
int shg_ada_tail_apply_f32(const float* x, const float* Hz, const float* sigma, const float* z, const float* cut, float* y, int N, int C, int H,
                           int W, int color_first, int color_count, int bias, void* stream);
int shg_ada_tail_adjoint_f32(const float* gy, const float* Hz, const float* cut, float* gx, int N, int C, int H, int W, int color_first,
                             int color_count, void* stream);

/* ---- next row N3 (training-side critic, forward only): minibatch_std_layer (stylegan.py:686-704).
 * x [N,C,H,W] -> y [N,C+F,H,W]; N % G == 0, C % F == 0; stat [N/G * F] is caller-owned scratch. */
int shg_minibatch_std_f32(const float* x, float* y, float* stat, int N, int C, int H, int W, int G, int F, void* stream);

/* ---- next row N3, fp16 route (the reference's `use_fp16` branches: stylegan.py:136-138,486,660-667, comodgan.py:40-47,305; its native
 * op is instantiated for half as well, upfirdn2d.cpp:59 AT_DISPATCH_FLOATING_TYPES_AND_HALF).  Layout of every fp16 activation:
 * channels-LAST, [N,H,W,C] IEEE halves (torch.channels_last on a [N,C,H,W] tensor) -- 8 consecutive channels are one 16-byte MFMA
 * operand.  Arithmetic: v_mfma_f32_32x32x16_f16, fp32 accumulation, one rounding to fp16.  Every tensor pointer of this section and the
 * per-channel fp32 operands (bias, out_scale / d) must be 16-byte aligned (vector loads; SHG_ERR_ARG otherwise).
 * shg_conv2d_f16_pack_weight: w [T][O][I] halves (T = k*k correlation taps, row-major (ky,kx)) -> wp in MFMA operand order
 *   [ceil(O/32) rounded up to 4][T][I/16][64][8] (shg_conv2d_f16_packed_weight_elems halves, zero beyond O): every operand of the
 *   kernel is one coalesced, unconditional 1 KiB load.
 * shg_conv2d_f16: w = that packed tensor, bias fp32 [O] or NULL, I % 32 == 0.
 *   mode 0: y [N,OH,OW,O] = conv2d(x, w, stride, pad);  mode 1: rows / columns [crop, crop+OH) x [crop, crop+OW) of
 *   conv_transpose2d(x, w, stride 2), 3x3, w[t][o][i] = torch weight[i][o][ky][kx] (conv2d_gradfix.py:109-116); entries beyond the
 *   (2H+1) x (2W+1) result are NOT written (shg_conv2d_f16_needs_clear: zero y first). */
long shg_conv2d_f16_packed_weight_elems(int T, int O, int I);
int shg_conv2d_f16_pack_weight(const void* w, void* wp, int T, int O, int I, void* stream);
/* the same operand order straight from a torch-layout weight: src [O][I][T] halves, or [I][O][T] when `transposed` (conv_transpose2d layout /
 * the channel-transposed weight of an input gradient); `flip` reverses the taps (180-degree rotation); input channels are zero-padded to a
 * multiple of 32 (wp holds shg_conv2d_f16_packed_weight_elems(T, O, roundup(I, 32)) halves). */
int shg_conv2d_f16_pack_weight_oihw(const void* src, void* wp, int T, int O, int I, int transposed, int flip, void* stream);
int shg_conv2d_f16(const void* x, const void* w, const float* bias, void* y, int N, int I, int O, int H, int W, int k, int stride, int pad,
                   int mode, int crop, int OH, int OW, void* stream);
int shg_conv2d_f16_needs_clear(int H, int W, int crop, int OH, int OW);
/* the same with the layer tail of the inference route fused: x*in_scale[n,i] at staging (both modes); mode 0 additionally
 * y = A(conv*out_scale[n,o] + noise*noise_strength + bias[o]) + residual on the half-rounded result (stylegan.py:173-181,298-304). */
int shg_conv2d_f16_fused(const void* x, const void* w, void* y, int N, int I, int O, int H, int W, int k, int stride, int pad, int mode, int crop,
                         int OH, int OW, const float* in_scale, const float* out_scale, const float* noise, int noise_mode, float noise_strength,
                         const float* bias, int act, float alpha, float gain, float clamp, const void* residual, void* stream);
/* weight gradient (replaces the cuDNN backward-weight call of conv2d_gradfix.py:140-146 for halves): dw [k*k][O][I] FP32 =
 * sum_{n,oy,ox} g[n,oy,ox,o] * x[n, oy*stride-pad+ky, ox*stride-pad+kx, i]; x [N,H,W,I], g [N,OH,OW,O] halves; I, O % 8 == 0;
 * deterministic (fp32 partial sums per pixel slice in `workspace`, reduced in a fixed order). */
size_t shg_conv2d_wgrad_f16_workspace_bytes(int N, int I, int O, int OH, int OW, int k);
int shg_conv2d_wgrad_f16(const void* x, const void* g, float* dw, int N, int I, int O, int H, int W, int OH, int OW, int k, int stride, int pad,
                         void* workspace, size_t ws_bytes, void* stream);
/* upfirdn2d on halves (same argument meaning as shg_upfirdn2d_f32; f stays fp32 [fh,fw], fp32 accumulation; C % 8 == 0). */
int shg_upfirdn2d_f16(const void* x, const float* f, void* y, int N, int C, int H, int W, int fh, int fw, int upx, int upy, int downx, int downy,
                      int padx0, int padx1, int pady0, int pady1, int flip, float gain, void* stream);
/* y = lrelu_agc(x + bias[c]) (act = 0: (x + bias) * gain) over `pixels` x C halves, and dL/dx from dL/dy and the saved OUTPUT y. */
/* Block-boundary casts `x.to(dtype)` (stylegan.py:486-495,659-663; comodgan.py:39-43,305-312) between the two activation layouts of this
 * library: float32 [N,C,H*W] (NCHW) -> float16 [N,H*W,C] (NHWC, torch.channels_last) when to_half, the reverse otherwise.  C % 8 == 0, or C <= 16
 * (thin tensors: the 4-channel network inputs). */
int shg_relayout_f32_f16(const void* src, void* dst, int N, int C, long HW, int to_half, void* stream);
int shg_bias_act_f16(const void* x, const float* bias, void* y, long pixels, int C, int act, float alpha, float gain, float clamp, void* stream);
int shg_bias_act_backward_f16(const void* g, const void* y, void* dx, long total, int act, float alpha, float gain, float clamp, void* stream);
/* modulation tail of a half layer in one pass each way (stylegan.py:173,176-181 + :298-304): y = A(t*d[n,c] + noise + bias[c]); backward from the
 * saved output: gt = gy*A'(y)*d, part [N][blocks][2][C] = per-workgroup pixel sums of gz*t and gz (caller sums over blocks: deterministic),
 * gnoise [N,HW] = channel sums of gz.  d fp32 [N,C] / noise fp32 [HW] (mode 1) or [N,HW] (mode 2) / bias fp32 [C], each optional. */
/* the same backward for float32 NCHW layers (forward = shg_bias_act_f32 with scale / noise / bias): gt = gy*A'(y)*d, part [N][blocks][2][C],
 * gnoise [cslices][N,HW] (per channel slice: the caller adds them); HW % 4 == 0, C <= 512.
 * Both take an optional second product u (a tensor like gy) / e fp32 [N,C]: gt = A'(y) * (gy*d + u*e) -- the tail's double backward
 * (R1 / path length, stylegan_default_loss.py:72-88,118-124): d/dgy = A'(y) (ggt d + t ggd) in one pass. */
int shg_modtail_backward_f32_blocks(long HW);
int shg_modtail_backward_f32_cslices(int N, int C, long HW);
int shg_modtail_backward_f32(const float* gy, const float* y, const float* t, const float* d, const float* u, const float* e, float* gt, float* part,
                             float* gnoise, int N, int C, long HW, int act, float alpha, float gain, float clamp, void* stream);
/* Kernel routes of the fp16 convolutions: bit 0 = the persistent LDS-DMA ring kernel for 3x3 stride-1 launches (csrc/conv_f16_ring.hip), bit 1 = the
 * merged-phase kernel for the stride-2 transposed form (csrc/conv_f16_upring.hip), bit 2 = the persistent kernel for 3x3 stride-2 launches
 * (csrc/conv_f16_down.hip); default 7; 0 = the gather kernel for everything.  Bits 0 / 1 give the gather kernel's bits, bit 2 the same
 * products summed k-step-major; returns the previous mask. */
int shg_conv2d_f16_set_routes(int mask);
int shg_modtail_f16(const void* t, const float* d, const float* noise, int noise_mode, const float* bias, void* y, int N, long HW, int C, int act,
                    float alpha, float gain, float clamp, void* stream);
int shg_modtail_backward_f16_blocks(long HW, int C);
int shg_modtail_backward_f16(const void* gy, const void* y, const void* t, const float* d, const void* u, const float* e, void* gt, float* part,
                             float* gnoise, int N, long HW, int C, int act, float alpha, float gain, float clamp, void* stream);

#ifdef __cplusplus
}
#endif
#endif
