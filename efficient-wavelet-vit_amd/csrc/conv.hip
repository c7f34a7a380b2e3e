// Dense 2-D convolution (kernel 1x1 or 3x3, pad k/2, stride 1|2) as an MFMA
// implicit GEMM, channels-last bf16 (gfx950).
//
// Callers: the MWT conv stack of network/mwt.py:23-72 — hf_conv['fusion'] (all 3
// levels batched), multiscale_fusion (384 -> 128, 112^2, reading the three
// level-major fusion outputs in place), freq_conv / freq_pool (stride 2) — 74 % of
// the model's FLOPs (SURVEY §8 note 3), and the EfficientNetV2-S backbone's dense
// convs (FusedMBConv 3x3, MBConv expand/project 1x1, head 1x1).  Three kernels:
//
//   fwd    y[m, co]  = sum_{tap, ci} x[pix(m, tap), ci] * W[co, ci, tap]   (+ bias)
//   dgrad  dx[m, ci] = sum_{tap, co} dy[pix^T(m, tap), co] * W[co, ci, tap]
//          (same kernel: A gathers dy through the transposed pixel map, B = W packed
//           [ci][tap][co]; stride 2 handled by the parity test of pix^T)
//   wgrad  dW[co, tap, ci] = sum_m dy[m, co] * x[pix(m, tap), ci]   (split over m)
//
// GEMM tile 128xBNx32, 256 threads = 4 waves (2x2), each wave 64x(BN/2) =
// 4x(BN/32) v_mfma_f32_16x16x32_bf16 tiles, fp32 accumulate.  Operands are staged
// global -> registers -> LDS with the next K-tile's loads in flight during the
// current tile's MFMAs.  When the per-tap channel count is a multiple of 32 every
// K-tile lies inside one tap, so the tap (and the pixel offset it implies) is a
// wave-uniform scalar and the gather costs a handful of VALU ops per vector.
// fwd/dgrad images are [row][k] (k contiguous, padded 80-B rows) read with
// ds_read_b128; wgrad's operands both have the reduction (pixel) index outermost
// in HBM, so they are staged as natural [k][row] images (256-B rows, XOR-swizzled
// 16-B chunks) and read as MFMA fragments with ds_read_b64_tr_b16.
//
// Grouped channels-last layout (gc, gs): channel c of pixel p lives at
// (c / gc) * gs + p * gc + c % gc.  gc = C is plain NHWC; gc = 128, gs = B*H*W*128
// is the MWT's level-major fusion output [L][B][H][W][128] read as the
// [B][H][W][3*128] concatenation (mwt.py:112) without materialising it.
// (This file: packs, validation, fwd / dgrad entry points; the kernel families: conv_common.h.)
#include "conv_common.h"

namespace ewvit {

// pack fp32 W (element (co, ci, tap) at co*s_co + ci*s_ci + tap*s_tap: any of the
// parameter's memory formats) -> bf16 [Cout][taps][Cin_pad] (fwd, wp) and/or
// [Cin_pad][taps][Cout] (dgrad, wp_t) in one pass; ci >= Cin packs zeros
__global__ __launch_bounds__(256) void conv_pack_kernel(const float *__restrict__ w, int64_t s_co, int64_t s_ci,
                                                        int64_t s_tap, bf16_t *__restrict__ wp,
                                                        bf16_t *__restrict__ wp_t, int Cout, int Cin, int Cin_pad,
                                                        int taps) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;   // index in the fwd layout
  const int64_t total = (int64_t)Cout * Cin_pad * taps;
  if (i >= total) return;
  const int ci = (int)(i % Cin_pad);
  const int tap = (int)((i / Cin_pad) % taps);
  const int co = (int)(i / ((int64_t)Cin_pad * taps));
  const bf16_t v = f2bf(ci < Cin ? w[co * s_co + ci * s_ci + tap * s_tap] : 0.f);
  if (wp) wp[i] = v;
  if (wp_t) wp_t[((int64_t)ci * taps + tap) * Cout + co] = v;
}

// multi-tensor pack: up to EWVIT_PACK_MAX weights per launch.  A workgroup packs one
// (weight, tap, 64-co x 64-ci) tile: read once, written row-contiguous to the fwd
// layout [co][tap][ci] and, through an LDS transpose, to the bwd_data layout
// [ci][tap][co] (tensor found by a uniform prefix-sum search over tile counts)
struct PackArgs {
  int n;
  int chunk0[EWVIT_PACK_MAX + 1];
  const float *w[EWVIT_PACK_MAX];
  bf16_t *wp[EWVIT_PACK_MAX];
  bf16_t *wpt[EWVIT_PACK_MAX];
  int64_t s_co[EWVIT_PACK_MAX], s_ci[EWVIT_PACK_MAX], s_tap[EWVIT_PACK_MAX];
  int cout[EWVIT_PACK_MAX], cin[EWVIT_PACK_MAX], cin_pad[EWVIT_PACK_MAX], taps[EWVIT_PACK_MAX];
};

__global__ __launch_bounds__(256) void conv_pack_multi_kernel(PackArgs a) {
  __shared__ bf16_t tile[64][66];
  const int blk = blockIdx.x, tid = threadIdx.x;
  int t = 0;
  while (t + 1 < a.n && a.chunk0[t + 1] <= blk) ++t;
  const int Cout = a.cout[t], Cin = a.cin[t], Cin_pad = a.cin_pad[t], taps = a.taps[t];
  const int nco = (Cout + 63) >> 6, nci = (Cin_pad + 63) >> 6;
  const int local = blk - a.chunk0[t];
  const int tap = local / (nco * nci), rem = local - tap * nco * nci;
  const int co0 = (rem / nci) * 64, ci0 = (rem % nci) * 64;
  const float *w = a.w[t];
  bf16_t *wp = a.wp[t], *wpt = a.wpt[t];
  const int64_t sco = a.s_co[t], sci = a.s_ci[t], stap = a.s_tap[t];
  if (sci == 1 && (Cin & 3) == 0 && (Cin_pad & 3) == 0 && (Cout & 3) == 0 && (sco & 3) == 0 && (stap & 3) == 0) {
    // ci-contiguous weights (the 1x1 convs, channels-last 3x3): 4 channels a thread, float4
    // loads, 8-byte stores in both layouts — all 4 loads of a thread in flight
    float4 v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int e4 = tid + 256 * u, r = e4 >> 4, c4 = (e4 & 15) * 4;
      const int co = co0 + r, ci = ci0 + c4;
      v[u] = co < Cout && ci < Cin ? *reinterpret_cast<const float4 *>(w + co * sco + ci + tap * stap)
                                   : make_float4(0.f, 0.f, 0.f, 0.f);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int e4 = tid + 256 * u, r = e4 >> 4, c4 = (e4 & 15) * 4;
      const int co = co0 + r, ci = ci0 + c4;
      const bf16_t b0 = f2bf(v[u].x), b1 = f2bf(v[u].y), b2 = f2bf(v[u].z), b3 = f2bf(v[u].w);
      tile[r][c4] = b0; tile[r][c4 + 1] = b1; tile[r][c4 + 2] = b2; tile[r][c4 + 3] = b3;
      if (wp && co < Cout && ci < Cin_pad) {
        uint2 pk;
        pk.x = (unsigned)b0 | ((unsigned)b1 << 16);
        pk.y = (unsigned)b2 | ((unsigned)b3 << 16);
        *reinterpret_cast<uint2 *>(wp + ((int64_t)co * taps + tap) * Cin_pad + ci) = pk;
      }
    }
    if (!wpt) return;
    __syncthreads();
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int e4 = tid + 256 * u, r = e4 >> 4, c4 = (e4 & 15) * 4;
      const int ci = ci0 + r, co = co0 + c4;
      if (ci < Cin_pad && co < Cout) {
        uint2 pk;
        pk.x = (unsigned)tile[c4][r] | ((unsigned)tile[c4 + 1][r] << 16);
        pk.y = (unsigned)tile[c4 + 2][r] | ((unsigned)tile[c4 + 3][r] << 16);
        *reinterpret_cast<uint2 *>(wpt + ((int64_t)ci * taps + tap) * Cout + co) = pk;
      }
    }
    return;
  }
#pragma unroll 4
  for (int e = tid; e < 4096; e += 256) {
    const int r = e >> 6, c = e & 63;
    const int co = co0 + r, ci = ci0 + c;
    const bf16_t v = f2bf(co < Cout && ci < Cin ? w[co * sco + ci * sci + tap * stap] : 0.f);
    tile[r][c] = v;
    if (wp && co < Cout && ci < Cin_pad) wp[((int64_t)co * taps + tap) * Cin_pad + ci] = v;
  }
  if (!wpt) return;
  __syncthreads();
#pragma unroll 4
  for (int e = tid; e < 4096; e += 256) {
    const int r = e >> 6, c = e & 63;
    const int ci = ci0 + r, co = co0 + c;
    if (ci < Cin_pad && co < Cout) wpt[((int64_t)ci * taps + tap) * Cout + co] = tile[c][r];
  }
}

int check_geom(const ConvGeom &g, const char *nm) {
  EWVIT_CHECK_ARG(g.N > 0 && g.H > 0 && g.W > 0 && g.Cin > 0 && g.Cout > 0, "%s: empty shape", nm);
  EWVIT_CHECK_ARG(g.Cin % 8 == 0 && g.Cout % 8 == 0, "%s: Cin=%d Cout=%d must be multiples of 8", nm, g.Cin, g.Cout);
  EWVIT_CHECK_ARG(g.stride == 1 || g.stride == 2, "%s: stride %d", nm, g.stride);
  EWVIT_CHECK_ARG(g.ks == 1 || g.ks == 3, "%s: kernel size %d (1 or 3)", nm, g.ks);
  return 0;
}

// grouped layout (gc, gs) for a tensor of C channels: gc == 0 means plain NHWC
int check_group(int64_t &gc, int64_t &gs, int64_t C, int64_t pixels, const char *nm, const char *which) {
  if (gc == 0 || gc == C) { gc = C; gs = 0; return 0; }
  EWVIT_CHECK_ARG(gc > 0 && gc % CBK == 0 && C % gc == 0, "%s: %s group width %lld must divide %lld and be a multiple of %d",
                  nm, which, (long long)gc, (long long)C, CBK);
  EWVIT_CHECK_ARG(gs >= pixels * gc, "%s: %s group stride %lld < %lld", nm, which, (long long)gs, (long long)(pixels * gc));
  return 0;
}

}  // namespace ewvit

using namespace ewvit;

extern "C" int ewvit_set_grid_cap(int max_workgroups);
extern "C" int ewvit_conv2d_set_grid_cap(int max_workgroups) { return ewvit_set_grid_cap(max_workgroups); }

extern "C" int ewvit_conv2d_pack_weight(const float *w, int64_t s_co, int64_t s_ci, int64_t s_tap, void *wp,
                                        void *wp_t, int64_t Cout, int64_t Cin, int64_t Cin_pad, int ksize,
                                        void *stream) {
  EWVIT_CHECK_ARG(w && (wp || wp_t) && Cout > 0 && Cin > 0 && Cin_pad >= Cin, "conv2d_pack_weight: bad args");
  EWVIT_CHECK_ARG(ksize == 1 || ksize == 3, "conv2d_pack_weight: kernel size %d", ksize);
  const int taps = ksize * ksize;
  const int64_t total = Cout * Cin_pad * taps;
  hipLaunchKernelGGL(conv_pack_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, as_stream(stream), w,
                     s_co, s_ci, s_tap, (bf16_t *)wp, (bf16_t *)wp_t, (int)Cout, (int)Cin, (int)Cin_pad, taps);
  return launch_status("conv2d_pack_weight");
}

extern "C" int ewvit_conv2d_pack_weights(int n, const float *const *w, const int64_t *s_co, const int64_t *s_ci,
                                         const int64_t *s_tap, void *const *wp, void *const *wp_t,
                                         const int64_t *Cout, const int64_t *Cin, const int64_t *Cin_pad,
                                         const int *ksize, void *stream) {
  EWVIT_CHECK_ARG(n >= 0 && n <= EWVIT_PACK_MAX, "conv2d_pack_weights: %d weights (max %d per launch)", n,
                  EWVIT_PACK_MAX);
  if (n == 0) return 0;
  PackArgs a;
  a.n = n;
  int64_t chunks = 0;
  for (int i = 0; i < n; ++i) {
    EWVIT_CHECK_ARG(w[i] && (wp[i] || wp_t[i]) && Cout[i] > 0 && Cin[i] > 0 && Cin_pad[i] >= Cin[i] &&
                        (ksize[i] == 1 || ksize[i] == 3),
                    "conv2d_pack_weights: weight %d", i);
    const int taps = ksize[i] * ksize[i];
    a.chunk0[i] = (int)chunks;
    chunks += (int64_t)taps * ((Cout[i] + 63) / 64) * ((Cin_pad[i] + 63) / 64);
    EWVIT_CHECK_ARG(chunks < ((int64_t)1 << 30), "conv2d_pack_weights: too many elements");
    a.w[i] = w[i]; a.wp[i] = (bf16_t *)wp[i]; a.wpt[i] = (bf16_t *)wp_t[i];
    a.s_co[i] = s_co[i]; a.s_ci[i] = s_ci[i]; a.s_tap[i] = s_tap[i];
    a.cout[i] = (int)Cout[i]; a.cin[i] = (int)Cin[i]; a.cin_pad[i] = (int)Cin_pad[i]; a.taps[i] = taps;
  }
  a.chunk0[n] = (int)chunks;
  hipLaunchKernelGGL(conv_pack_multi_kernel, dim3((unsigned)chunks), dim3(256), 0, as_stream(stream), a);
  return launch_status("conv2d_pack_weights");
}

// rows per BatchNorm partial that ewvit_conv2d_fwd_bn leaves for this shape (the
// LDS-DMA kernel's m-tile), or 0 when the shape takes the register-staged kernel
// (the windowed kernel, convwin.hip, leaves one partial row per 16 x 16 output block)
extern "C" int64_t ewvit_conv2d_fwd_bn_rows(int64_t N, int64_t H, int64_t W, int64_t Cin, int64_t Cout, int ksize,
                                           int stride) {
  if (!use_glds() || Cin % 64 || Cout % 8 || Cout > 65536) return 0;
  const int64_t Ho = (H - 1) / stride + 1, Wo = (W - 1) / stride + 1;
  const int64_t K = (int64_t)ksize * ksize * Cin;
  if (2 * N * H * W * Cin >= (int64_t)OOB || Cout * K * 2 >= (int64_t)OOB || N * Ho * Wo * Cout >= (int64_t)1 << 40)
    return 0;
  FwdArgs a = fwd_args(mkg(N, H, W, Cin, Cout, ksize, stride), Cin, 0);
  a.bn_part = reinterpret_cast<float *>(1);    // (a statistics epilogue)
  if (win_ok(a, false)) return 256;
  int bm, bn;
  glds_tile(a, false, bm, bn);
  return bm;
}

extern "C" int ewvit_conv2d_fwd_bn(const void *x, const void *wp, const float *bias, void *y, int64_t N, int64_t H,
                                   int64_t W, int64_t Cin, int64_t Cout, int ksize, int stride, int64_t x_group_c,
                                   int64_t x_group_stride, const float *bn_shift, float *bn_part,
                                   float *bn_shift_out, void *stream) {
  EWVIT_CHECK_ARG(x && wp && y && bn_part && bn_shift_out, "conv2d_fwd_bn: null pointer");
  ConvGeom g = mkg(N, H, W, Cin, Cout, ksize, stride);
  if (int rc = check_geom(g, "conv2d_fwd_bn")) return rc;
  if (int rc = check_group(x_group_c, x_group_stride, Cin, N * H * W, "conv2d_fwd_bn", "x")) return rc;
  const int64_t rows = ewvit_conv2d_fwd_bn_rows(N, H, W, Cin, Cout, ksize, stride);
  EWVIT_CHECK_ARG(rows > 0 && x_group_c % 64 == 0,
                  "conv2d_fwd_bn: shape takes the register-staged kernel (query ewvit_conv2d_fwd_bn_rows)");
  FwdArgs a = fwd_args(g, x_group_c, x_group_stride);
  a.src = (const bf16_t *)x; a.wp = (const bf16_t *)wp; a.bias = bias; a.out = (bf16_t *)y;
  a.bn_shift = bn_shift; a.bn_part = bn_part; a.bn_shift_out = bn_shift_out;
  const int64_t xb = grouped_bytes(N * H * W, Cin, x_group_c, x_group_stride);
  if (rows == 256)
    EWVIT_CHECK_ARG(launch_win(a, xb, false, as_stream(stream)), "conv2d_fwd_bn: windowed kernel refused the shape");
  else
    EWVIT_CHECK_ARG(launch_glds(a, xb, false, as_stream(stream)), "conv2d_fwd_bn: LDS-DMA kernel refused the shape");
  return launch_status("conv2d_fwd_bn");
}

// ---- convs reading relu(x * scale + shift): the training BatchNorm + ReLU of x's producer
// applied in the windowed kernels' operand staging (XF; coefficients from ewvit_bn_coef, one
// [2][group channels] block per channel group of x), so the normalised tensor is never written.
// The forward (with the next BatchNorm's statistics) and the weight gradient (conv_wgrad.hip);
// the input gradient is the plain conv's (it does not read x).  3x3 stride 1 over maps the
// windowed kernels take.
bool ewvit::xf_args(FwdArgs &a, WgradArgs &w, const ConvGeom &g, int64_t x_group_c, int64_t x_group_stride) {
  if (g.ks != 3 || g.stride != 1 || x_group_c <= 0 || g.Cin % x_group_c || g.Cin > 512 || !use_glds()) return false;
  a = fwd_args(g, x_group_c, x_group_stride);
  a.bn_part = reinterpret_cast<float *>(1);
  a.xf = reinterpret_cast<const float *>(1);
  w = wgrad_args(g, x_group_c, x_group_stride);
  const int64_t xb = grouped_bytes((int64_t)g.N * g.H * g.W, g.Cin, x_group_c, x_group_stride);
  return win_ok(a, false) && xb < (int64_t)OOB && wgrad_win_splits(w, xb) > 0;
}
extern "C" int ewvit_conv2d_xf_ok(int64_t N, int64_t H, int64_t W, int64_t Cin, int64_t Cout, int ksize, int stride,
                                  int64_t x_group_c, int64_t x_group_stride) {
  FwdArgs a;
  WgradArgs w;
  return xf_args(a, w, mkg(N, H, W, Cin, Cout, ksize, stride), x_group_c, x_group_stride) ? 1 : 0;
}
extern "C" int ewvit_conv2d_fwd_bn_xf(const void *x, const void *wp, const float *bias, void *y, int64_t N, int64_t H,
                                      int64_t W, int64_t Cin, int64_t Cout, int64_t x_group_c, int64_t x_group_stride,
                                      const float *xf, const float *bn_shift, float *bn_part, float *bn_shift_out,
                                      void *stream) {
  EWVIT_CHECK_ARG(x && wp && y && xf && bn_part && bn_shift_out, "conv2d_fwd_bn_xf: null pointer");
  ConvGeom g = mkg(N, H, W, Cin, Cout, 3, 1);
  if (int rc = check_geom(g, "conv2d_fwd_bn_xf")) return rc;
  if (int rc = check_group(x_group_c, x_group_stride, Cin, N * H * W, "conv2d_fwd_bn_xf", "x")) return rc;
  FwdArgs a;
  WgradArgs w;
  EWVIT_CHECK_ARG(xf_args(a, w, g, x_group_c, x_group_stride),
                  "conv2d_fwd_bn_xf: shape not taken by the windowed kernels (query ewvit_conv2d_xf_ok)");
  a.src = (const bf16_t *)x; a.wp = (const bf16_t *)wp; a.bias = bias; a.out = (bf16_t *)y;
  a.bn_shift = bn_shift; a.bn_part = bn_part; a.bn_shift_out = bn_shift_out; a.xf = xf;
  const int64_t xb = grouped_bytes(N * H * W, Cin, x_group_c, x_group_stride);
  EWVIT_CHECK_ARG(launch_win(a, xb, false, as_stream(stream)), "conv2d_fwd_bn_xf: windowed kernel refused the shape");
  return launch_status("conv2d_fwd_bn_xf");
}

// input channels per tap the fwd expects its weight pack to have: Cin rounded up to 64
// when Cin % 64 != 0 (Cin % 16 == 0) and the padded LDS-DMA kernel takes the shape
extern "C" int64_t ewvit_conv2d_fwd_pack_cin(int64_t N, int64_t H, int64_t W, int64_t Cin, int64_t Cout, int ksize,
                                            int stride) {
  if (Cin % 64 == 0 || Cin % 16 || !use_glds()) return Cin;
  const int64_t Cp = (Cin + 63) / 64 * 64;
  if (4 * Cp > 5 * Cin) return Cin;      // > 25 % zero K (48 -> 64 measured slower): exact-K kernel
  const int64_t Ho = (H - 1) / stride + 1, Wo = (W - 1) / stride + 1;
  if (2 * N * H * W * Cin >= (int64_t)OOB || Cout * ksize * ksize * Cp * 2 >= (int64_t)OOB ||
      N * Ho * Wo * Cout >= (int64_t)1 << 40)
    return Cin;
  return Cp;
}

extern "C" int ewvit_conv2d_fwd(const void *x, const void *wp, const float *bias, void *y, int64_t N, int64_t H,
                                int64_t W, int64_t Cin, int64_t Cout, int ksize, int stride, int64_t x_group_c,
                                int64_t x_group_stride, void *stream) {
  EWVIT_CHECK_ARG(x && wp && y, "conv2d_fwd: null pointer");
  ConvGeom g = mkg(N, H, W, Cin, Cout, ksize, stride);
  if (int rc = check_geom(g, "conv2d_fwd")) return rc;
  if (int rc = check_group(x_group_c, x_group_stride, Cin, N * H * W, "conv2d_fwd", "x")) return rc;
  FwdArgs a = fwd_args(g, x_group_c, x_group_stride);
  a.src = (const bf16_t *)x; a.wp = (const bf16_t *)wp; a.bias = bias; a.out = (bf16_t *)y;
  hipStream_t s = as_stream(stream);
  const int64_t xb = grouped_bytes(N * H * W, Cin, x_group_c, x_group_stride);
  const int64_t cp = x_group_stride ? Cin : ewvit_conv2d_fwd_pack_cin(N, H, W, Cin, Cout, ksize, stride);
  if (cp != Cin) {
    // the weights were packed with cp input channels (ewvit_conv2d_fwd_pack_cin)
    a.KC = (int)cp; a.KCr = (int)Cin;
    EWVIT_CHECK_ARG(launch_glds(a, xb, false, s), "conv2d_fwd: padded LDS-DMA kernel refused");
  } else if (!launch_win(a, xb, false, s) && !launch_small(a, false, s) && !launch_glds(a, xb, false, s)) {
    launch_fwd(a, false, s);
  }
  return launch_status("conv2d_fwd");
}

// 1 when ewvit_conv2d_bwd_data_add can run this shape (the LDS-DMA dgrad kernel)
extern "C" int64_t ewvit_conv2d_bwd_data_add_ok(int64_t N, int64_t H, int64_t W, int64_t Cin, int64_t Cout, int ksize,
                                               int stride) {
  if (!use_glds() || (Cout % 64 && (Cout % 8 || 5 * ((Cout + 63) / 64 * 64) > 6 * Cout)) ||
      Cin % 8 || 2 * N * H * W * Cout >= (int64_t)OOB ||
      Cin * ksize * ksize * Cout * 2 >= (int64_t)OOB)
    return 0;
  (void)stride;
  return 1;
}

// dx = dgrad(dy) + addend (plain NHWC, bf16): the skip connection's gradient of a
// residual block added in the dgrad epilogue of the block's first conv
extern "C" int ewvit_conv2d_bwd_data_add(const void *dy, const void *wp_t, void *dx, const void *addend, int64_t N,
                                         int64_t H, int64_t W, int64_t Cin, int64_t Cout, int ksize, int stride,
                                         void *stream) {
  EWVIT_CHECK_ARG(dy && wp_t && dx && addend, "conv2d_bwd_data_add: null pointer");
  ConvGeom g = mkg(N, H, W, Cin, Cout, ksize, stride);
  if (int rc = check_geom(g, "conv2d_bwd_data_add")) return rc;
  EWVIT_CHECK_ARG(ewvit_conv2d_bwd_data_add_ok(N, H, W, Cin, Cout, ksize, stride),
                  "conv2d_bwd_data_add: shape not supported (query ewvit_conv2d_bwd_data_add_ok)");
  FwdArgs a = dgrad_args(g, Cin, 0);
  a.src = (const bf16_t *)dy; a.wp = (const bf16_t *)wp_t; a.out = (bf16_t *)dx;
  a.addend = (const bf16_t *)addend;
  const int64_t sb = 2 * N * (int64_t)g.Ho * g.Wo * Cout;
  EWVIT_CHECK_ARG(dgrad_by_parity(a, sb, as_stream(stream)) || launch_glds(a, sb, true, as_stream(stream)),
                  "conv2d_bwd_data_add: LDS-DMA kernel refused the shape");
  return launch_status("conv2d_bwd_data_add");
}

// partial rows per channel group ewvit_conv2d_bwd_data_bn leaves for this shape (one per 128
// dx rows), or 0 when the shape does not take it: stride 1, the LDS-DMA dgrad
// (ewvit_conv2d_bwd_data_add_ok)
extern "C" int64_t ewvit_conv2d_bwd_bn_rows(int64_t N, int64_t H, int64_t W, int64_t Cin, int64_t Cout, int ksize,
                                           int stride) {
  if (stride != 1 || !ewvit_conv2d_bwd_data_add_ok(N, H, W, Cin, Cout, ksize, stride) ||
      Cin > 65536)
    return 0;
  FwdArgs a = dgrad_args(mkg(N, H, W, Cin, Cout, ksize, stride), Cin, 0);
  a.bwd.part = reinterpret_cast<float *>(1);
  int bm, bn;
  glds_tile(a, true, bm, bn);
  return (N * H * W + bm - 1) / bm;
}

// dx = dgrad(dy) (+ addend, when not null; plain dx only) and the backward statistics of the
// BatchNorm whose output was this conv's input (bx: that BN's input, dx's layout, bf16; mean /
// invstd its saved statistics; gamma / beta or null; act 0/1/2; rscale [N] with act 0: the
// drop-path factor per frame of the MBConv tail, or null).  BatchNorm groups: a grouped dx
// (dx_group_c, dx_group_stride: the multiscale conv's level-major input) has one per channel
// group, mean / invstd [groups][group_c]; a plain dx with bn_group_rows > 0 (a multiple of 128
// dividing N*H*W) one per slice of that many rows, mean / invstd [groups][Cin].  part
// [groups][ewvit_conv2d_bwd_bn_rows per channel group or ... / groups per row group][2 C]
// gets per 128-row m-tile (sum g, sum g * xhat) of the bf16-rounded dx; *nrc_out = the partial
// rows per BatchNorm group (what ewvit_bn_bwd_partials is given)
extern "C" int ewvit_conv2d_bwd_data_bn(const void *dy, const void *wp_t, void *dx, const void *addend, int64_t N,
                                        int64_t H, int64_t W, int64_t Cin, int64_t Cout, int ksize, int stride,
                                        int64_t dx_group_c, int64_t dx_group_stride, const void *bx,
                                        const float *mean, const float *invstd, const float *gamma, const float *beta,
                                        int act, const float *rscale, int64_t bn_group_rows, float *part,
                                        int *nrc_out, void *stream) {
  EWVIT_CHECK_ARG(dy && wp_t && dx && bx && mean && invstd && part && nrc_out && act >= 0 && act <= 2 &&
                      !(rscale && act),
                  "conv2d_bwd_data_bn: bad args");
  ConvGeom g = mkg(N, H, W, Cin, Cout, ksize, stride);
  if (int rc = check_geom(g, "conv2d_bwd_data_bn")) return rc;
  if (int rc = check_group(dx_group_c, dx_group_stride, Cin, N * H * W, "conv2d_bwd_data_bn", "dx")) return rc;
  EWVIT_CHECK_ARG(ewvit_conv2d_bwd_bn_rows(N, H, W, Cin, Cout, ksize, stride) > 0,
                  "conv2d_bwd_data_bn: shape not supported (query ewvit_conv2d_bwd_bn_rows)");
  EWVIT_CHECK_ARG(!(addend && dx_group_stride), "conv2d_bwd_data_bn: an addend needs a plain dx");
  EWVIT_CHECK_ARG(bn_group_rows == 0 || (!dx_group_stride && bn_group_rows % 128 == 0 &&
                                         (N * H * W) % bn_group_rows == 0),
                  "conv2d_bwd_data_bn: BatchNorm row groups of %lld rows", (long long)bn_group_rows);
  FwdArgs a = dgrad_args(g, dx_group_c, dx_group_stride);
  a.src = (const bf16_t *)dy; a.wp = (const bf16_t *)wp_t; a.out = (bf16_t *)dx;
  a.addend = (const bf16_t *)addend;
  a.bwd.part = part; a.bwd.x = (const bf16_t *)bx; a.bwd.mean = mean; a.bwd.invstd = invstd; a.bwd.gamma = gamma;
  a.bwd.beta = beta; a.bwd.rscale = rscale; a.bwd.act = act; a.bwd.hw = (int)(H * W); a.bwd.grows = bn_group_rows;
  const int64_t sb = 2 * N * (int64_t)g.Ho * g.Wo * Cout;
  int bm = 0;
  EWVIT_CHECK_ARG(launch_glds(a, sb, true, as_stream(stream), &bm) && bm > 0,
                  "conv2d_bwd_data_bn: LDS-DMA kernel refused the shape");
  const int64_t ntm = (a.M + bm - 1) / bm;
  *nrc_out = (int)(bn_group_rows ? bn_group_rows / bm : ntm);
  return launch_status("conv2d_bwd_data_bn");
}

// the windowed input gradient with the backward statistics of the BatchNorm(+act) whose output
// the conv read (convwin.hip BST): one partial row per 16 x 16 block per channel group, part
// [groups][N*H*W / 256][2 group_c]; BatchNorm groups = dx's channel groups (mean / invstd
// [groups][group_c], gamma / beta [group_c] or null), or — a plain dx (group_c = Cin,
// group_stride 0) with bn_group_rows > 0 — slices of that many rows (whole images; mean / invstd
// [N*H*W / bn_group_rows][Cin]), part [slices][bn_group_rows / 256][2 Cin].
// ewvit_conv2d_bwd_bn_win_rows: N*H*W / 256 (the partial rows per channel group; with row groups
// the total over the slices), 0 when the windowed kernel does not take the shape.
static bool bst_args(FwdArgs &a, const ConvGeom &g, int64_t dx_group_c, int64_t dx_group_stride,
                     int64_t bn_group_rows) {
  if (g.ks != 3 || g.stride != 1 || dx_group_c <= 0 || g.Cin % dx_group_c) return false;
  a = dgrad_args(g, dx_group_c, dx_group_stride);
  a.bwd.part = reinterpret_cast<float *>(1);
  a.bwd.x = reinterpret_cast<const bf16_t *>(2);
  a.bwd.mean = a.bwd.invstd = reinterpret_cast<const float *>(4);
  if (bn_group_rows < 0 || (bn_group_rows && (dx_group_stride || dx_group_c != g.Cin))) return false;
  a.bwd.grows = bn_group_rows;
  const int64_t sb = 2 * (int64_t)g.N * g.H * g.W * g.Cout;
  return sb < (int64_t)OOB && win_ok(a, true);
}
extern "C" int64_t ewvit_conv2d_bwd_bn_win_rows(int64_t N, int64_t H, int64_t W, int64_t Cin, int64_t Cout, int ksize,
                                               int stride, int64_t dx_group_c, int64_t dx_group_stride,
                                               int64_t bn_group_rows) {
  FwdArgs a;
  return bst_args(a, mkg(N, H, W, Cin, Cout, ksize, stride), dx_group_c, dx_group_stride, bn_group_rows)
             ? N * H * W / 256
             : 0;
}
extern "C" int ewvit_conv2d_bwd_data_bn_win(const void *dy, const void *wp_t, void *dx, int64_t N, int64_t H,
                                            int64_t W, int64_t Cin, int64_t Cout, int64_t dx_group_c,
                                            int64_t dx_group_stride, const void *bx, const float *mean,
                                            const float *invstd, const float *gamma, const float *beta, int act,
                                            int64_t bn_group_rows, float *part, void *stream) {
  EWVIT_CHECK_ARG(dy && wp_t && dx && bx && mean && invstd && part && act >= 0 && act <= 2,
                  "conv2d_bwd_data_bn_win: bad args");
  ConvGeom g = mkg(N, H, W, Cin, Cout, 3, 1);
  if (int rc = check_geom(g, "conv2d_bwd_data_bn_win")) return rc;
  if (int rc = check_group(dx_group_c, dx_group_stride, Cin, N * H * W, "conv2d_bwd_data_bn_win", "dx")) return rc;
  FwdArgs a;
  EWVIT_CHECK_ARG(bst_args(a, g, dx_group_c, dx_group_stride, bn_group_rows),
                  "conv2d_bwd_data_bn_win: shape not taken (query ewvit_conv2d_bwd_bn_win_rows)");
  a.src = (const bf16_t *)dy; a.wp = (const bf16_t *)wp_t; a.out = (bf16_t *)dx;
  a.bwd.part = part; a.bwd.x = (const bf16_t *)bx; a.bwd.mean = mean; a.bwd.invstd = invstd; a.bwd.gamma = gamma;
  a.bwd.beta = beta; a.bwd.rscale = nullptr; a.bwd.act = act; a.bwd.hw = (int)(H * W); a.bwd.grows = bn_group_rows;
  const int64_t sb = 2 * N * H * W * Cout;
  EWVIT_CHECK_ARG(launch_win(a, sb, true, as_stream(stream)), "conv2d_bwd_data_bn_win: windowed kernel refused");
  return launch_status("conv2d_bwd_data_bn_win");
}

extern "C" int ewvit_conv2d_bwd_data(const void *dy, const void *wp_t, void *dx, int64_t N, int64_t H, int64_t W,
                                     int64_t Cin, int64_t Cout, int ksize, int stride, int64_t dx_group_c,
                                     int64_t dx_group_stride, void *stream) {
  EWVIT_CHECK_ARG(dy && wp_t && dx, "conv2d_bwd_data: null pointer");
  ConvGeom g = mkg(N, H, W, Cin, Cout, ksize, stride);
  if (int rc = check_geom(g, "conv2d_bwd_data")) return rc;
  if (int rc = check_group(dx_group_c, dx_group_stride, Cin, N * H * W, "conv2d_bwd_data", "dx")) return rc;
  FwdArgs a = dgrad_args(g, dx_group_c, dx_group_stride);
  a.src = (const bf16_t *)dy; a.wp = (const bf16_t *)wp_t; a.out = (bf16_t *)dx;
  hipStream_t s = as_stream(stream);
  const int64_t sb = 2 * N * (int64_t)g.Ho * g.Wo * Cout;
  if (!launch_win(a, sb, true, s) && !launch_small(a, true, s) && !dgrad_by_parity(a, sb, s) &&
      !launch_glds(a, sb, true, s))
    launch_fwd(a, true, s);
  return launch_status("conv2d_bwd_data");
}
