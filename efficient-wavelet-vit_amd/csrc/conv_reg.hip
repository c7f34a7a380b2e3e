// The register-staged fwd / dgrad (conv.hip's header; every shape's fallback), the small-channel 3x3.
#include "conv_common.h"

namespace ewvit {

template <bool DGRAD, int BN_, int KS, int BK, int PF>
__global__ __launch_bounds__(256) void conv_fwd_kernel(FwdArgs a) {
  // BK: K-tile depth (32 | 64); PF: K-tiles of register prefetch (1 | 2)
  constexpr int WN = BN_ / 2, J = WN / 16;  // per-wave columns, 16-wide MFMA tiles
  constexpr int LD = BK + 8;                 // padded [row][k] image row (bf16)
  constexpr int CPR = BK / 8;                // 16-B chunks per image row
  constexpr int VA = CBM * CPR / 256;        // A vectors staged per thread per K-tile
  constexpr int VB = BN_ * CPR / 256;        // B vectors
  constexpr int A_EL = 2 * CBM * LD, B_EL = 2 * BN_ * LD;
  constexpr int CST = BN_ + 8;               // epilogue image row (bf16)
  static_assert(CBM * CST <= A_EL + B_EL, "epilogue tile must fit the staging LDS");
  static_assert(VB >= 1, "tile too narrow for the staging map");
  // one LDS array: double-buffered A / B images, reused as the output tile image
  __shared__ __attribute__((aligned(16))) bf16_t smem[A_EL + B_EL];
  auto As = reinterpret_cast<bf16_t (*)[CBM][LD]>(smem);
  auto Bs = reinterpret_cast<bf16_t (*)[BN_][LD]>(smem + A_EL);
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int wm = w >> 1, wn = w & 1;
  const int64_t ntm = (a.M + CBM - 1) / CBM;
  // one M-tile per workgroup, or a grid-stride walk when the grid is capped (g_grid_cap)
  for (int64_t mt = blockIdx.x; mt < ntm; mt += gridDim.x) {
  const int64_t m0 = mt * CBM;
  const int n0 = blockIdx.y * BN_;
  const int K = KS * KS * a.KC;
  const int nk = (K + BK - 1) / BK;
  const bool fastk = (a.KC % BK) == 0;    // every K-tile inside one tap / one src group
  const int cbn = a.KC / BK;              // channel blocks per tap (fastk)
  const int ls = a.g.stride >> 1;         // log2(stride)
  const int smask = a.g.stride - 1;

  // staged vector v = tid + 256*u covers image row v / CPR, chunk v % CPR
  int arow[VA], ach[VA];
  int py[VA], px[VA];    // fwd: oh*s - pad, ow*s - pad;  dgrad: oh + pad, ow + pad
  int64_t pbase[VA];     // n * srcH * srcW
  bool avalid[VA];
#pragma unroll
  for (int u = 0; u < VA; ++u) {
    const int v = tid + 256 * u;
    arow[u] = v / CPR;
    ach[u] = (v % CPR) * 8;
    const int64_t m = m0 + arow[u];
    avalid[u] = m < a.M;
    const int64_t mm = avalid[u] ? m : 0;
    const int ow = (int)(mm % a.outW);
    const int64_t t = mm / a.outW;
    const int oh = (int)(t % a.outH);
    const int n = (int)(t / a.outH);
    if (!DGRAD) { py[u] = oh * a.g.stride - a.g.pad; px[u] = ow * a.g.stride - a.g.pad; }
    else        { py[u] = oh + a.g.pad;               px[u] = ow + a.g.pad; }
    pbase[u] = (int64_t)n * a.srcH * a.srcW;
  }
  // pixel index of tap (kh, kw) for staged row u, or -1 when it falls outside src
  auto src_pix = [&](int u, int kh, int kw) -> int64_t {
    int sh, sw;
    if (!DGRAD) {
      sh = py[u] + kh; sw = px[u] + kw;
    } else {
      const int th = py[u] - kh, tw = px[u] - kw;
      if (th < 0 || tw < 0 || ((th | tw) & smask)) return -1;
      sh = th >> ls; sw = tw >> ls;
    }
    if ((unsigned)sh >= (unsigned)a.srcH || (unsigned)sw >= (unsigned)a.srcW) return -1;
    return pbase[u] + (int64_t)sh * a.srcW + sw;
  };
  int ltap = 0, lcb = 0;   // fastk: tap / channel block of the next K-tile to load
  auto load_tile = [&](int kt, uint4 (&ra)[VA], uint4 (&rb)[VB]) {
    int kh = 0, kw = 0;
    int64_t goff = 0;      // group offset (elements) of this tile's channel block
    int cin0 = 0;          // channel within the group for ach == 0
    if (fastk) {
      kh = ltap / KS; kw = ltap - kh * KS;
      const int c0 = lcb * BK;
      const int gi = c0 / a.sgc;
      goff = (int64_t)gi * a.sgs;
      cin0 = c0 - gi * a.sgc;
      if (++lcb == cbn) { lcb = 0; ++ltap; }
    }
#pragma unroll
    for (int u = 0; u < VA; ++u) {
      const int k = kt * BK + ach[u];
      int64_t off, p;
      if (fastk) {
        p = src_pix(u, kh, kw);
        off = goff + p * a.sgc + cin0 + ach[u];
      } else {   // KC % BK != 0 (ungrouped src): per-thread tap
        const int tap = KS == 1 ? 0 : k / a.KC;
        const int c = k - tap * a.KC;
        const int th = tap / KS;
        p = src_pix(u, th, tap - th * KS);
        off = p * a.KC + c;
      }
      uint4 va = make_uint4(0u, 0u, 0u, 0u);
      if (avalid[u] && k < K && p >= 0) va = *reinterpret_cast<const uint4 *>(a.src + off);
      ra[u] = va;
    }
#pragma unroll
    for (int u = 0; u < VB; ++u) {
      const int v = tid + 256 * u;
      const int n = n0 + v / CPR, k = kt * BK + (v % CPR) * 8;
      uint4 vb = make_uint4(0u, 0u, 0u, 0u);
      if (n < a.Ncol && k < K) vb = *reinterpret_cast<const uint4 *>(a.wp + (int64_t)n * K + k);
      rb[u] = vb;
    }
  };
  auto store_tile = [&](int buf, const uint4 (&ra)[VA], const uint4 (&rb)[VB]) {
#pragma unroll
    for (int u = 0; u < VA; ++u) *reinterpret_cast<uint4 *>(&As[buf][arow[u]][ach[u]]) = ra[u];
#pragma unroll
    for (int u = 0; u < VB; ++u) {
      const int v = tid + 256 * u;
      *reinterpret_cast<uint4 *>(&Bs[buf][v / CPR][(v % CPR) * 8]) = rb[u];
    }
  };

  cf32x4 acc[4][J];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < J; ++j) acc[i][j] = cf32x4{0.f, 0.f, 0.f, 0.f};

  const int fr = lane & 15, fk = (lane >> 4) * 8;
  auto compute = [&](int cur) {
#pragma unroll
    for (int ks = 0; ks < BK / 32; ++ks) {
      cbf16x8 af[4], bfr[J];
#pragma unroll
      for (int i = 0; i < 4; ++i)
        af[i] = *reinterpret_cast<const cbf16x8 *>(&As[cur][wm * 64 + i * 16 + fr][ks * 32 + fk]);
#pragma unroll
      for (int j = 0; j < J; ++j)
        bfr[j] = *reinterpret_cast<const cbf16x8 *>(&Bs[cur][wn * WN + j * 16 + fr][ks * 32 + fk]);
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < J; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i], bfr[j], acc[i][j], 0, 0, 0);
    }
  };
  if constexpr (PF == 1) {
    // K-tile kt+1 is loaded into registers while kt is computed from LDS
    uint4 ra[VA], rb[VB];
    load_tile(0, ra, rb);
    store_tile(0, ra, rb);
    __syncthreads();
    for (int kt = 0; kt < nk; ++kt) {
      const int cur = kt & 1;
      const bool more = kt + 1 < nk;
      if (more) load_tile(kt + 1, ra, rb);
      compute(cur);
      if (more) store_tile(cur ^ 1, ra, rb);
      __syncthreads();
    }
  } else {
    // K-tile kt+2 is loaded into registers while kt is computed from LDS and kt+1
    // (loaded one step earlier) is written to the other LDS buffer
    auto step = [&](int kt, uint4 (&na)[VA], uint4 (&nb)[VB], const uint4 (&ra)[VA], const uint4 (&rb)[VB]) {
      const int cur = kt & 1;
      if (kt + 2 < nk) load_tile(kt + 2, na, nb);
      compute(cur);
      if (kt + 1 < nk) store_tile(cur ^ 1, ra, rb);
      __syncthreads();
    };
    uint4 pa[VA], pb[VB], qa[VA], qb[VB];
    load_tile(0, pa, pb);
    if (nk > 1) load_tile(1, qa, qb);
    store_tile(0, pa, pb);
    __syncthreads();
    int kt = 0;
    for (; kt + 1 < nk; kt += 2) {
      step(kt, pa, pb, qa, qb);
      step(kt + 1, qa, qb, pa, pb);
    }
    if (kt < nk) step(kt, pa, pb, qa, qb);
  }
  // epilogue: accumulators (+ bias) -> bf16 tile image in LDS (C/D map col = lane&15,
  // row = (lane>>4)*4 + r), then 16-B row-contiguous stores of 8 output channels
  // (the loop above ended with a barrier, so the staging images are free)
#pragma unroll
  for (int j = 0; j < J; ++j) {
    const int cl = wn * WN + j * 16 + (lane & 15);
    const float b = (a.bias && n0 + cl < a.Ncol) ? a.bias[n0 + cl] : 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) smem[(wm * 64 + i * 16 + (lane >> 4) * 4 + r) * CST + cl] = f2bf(acc[i][j][r] + b);
  }
  __syncthreads();
  constexpr int VPR = BN_ / 8;               // 16-B vectors per tile row
#pragma unroll
  for (int k = 0; k < CBM * VPR / 256; ++k) {
    const int v = tid + 256 * k;
    const int rl = v / VPR, cv = v % VPR;
    const int64_t row = m0 + rl;
    const int col = n0 + cv * 8;
    if (row < a.M && col < a.Ncol) {
      const int gi = col / a.ogc;
      *reinterpret_cast<uint4 *>(a.out + (int64_t)gi * a.ogs + row * a.ogc + (col - gi * a.ogc)) =
          *reinterpret_cast<const uint4 *>(&smem[rl * CST + cv * 8]);
    }
  }
  __syncthreads();         // the output image is read before the next tile stages into smem
  }
}

// M-tiles of the register-staged grid: all, or (g_grid_cap) at most cap / N-tiles of them
static unsigned capped_mtiles(int64_t M, int ntn) {
  int64_t gx = (M + CBM - 1) / CBM;
  if (g_grid_cap > 0 && gx * ntn > g_grid_cap) gx = g_grid_cap / ntn > 0 ? g_grid_cap / ntn : 1;
  return (unsigned)gx;
}

// ---------------------------------------------------------------- small-channel 3x3
// 3x3 stride-1 convs over few channels (KC = 16 / 24 per tap, <= 64 outputs): stage 1 of the
// backbone (24 -> 24 at 112^2, forward and input gradient) and the MWT seperate conv
// (16 -> 64).  A GEMM tile of 128 pixels re-gathers its 9 taps from L2 per K-tile; here a
// workgroup stages the input rows its TH output rows need ONCE in LDS ([TH+2][W+2][KC] bf16,
// zero halo — no bounds tests in the loop), keeps the packed weights of all taps in
// registers (they are the MFMA A operand: K = 9*KC padded to k-steps of 32, N = Ncol padded
// to 16-wide tiles), and walks 16-pixel groups: per group, KSTEPS ds_read_b128 of the pixel
// operand and NT*KSTEPS v_mfma_f32_16x16x32_bf16.  Operands weights-first, so a lane ends
// with 4 consecutive output channels of one pixel (8-byte stores).  FLIP: the input gradient
// (taps mirrored; weights packed [Cin][taps][Cout]).  Grid: (N * ceil(H/TH)) workgroups,
// walked persistently when the launch is capped.
template <int KC, int NT, bool FLIP>
__global__ __launch_bounds__(256) void conv3x3_small_kernel(FwdArgs a, int TH, int nblk) {
  constexpr int CC = KC / 8, NCH = 9 * CC, KSTEPS = (NCH + 3) / 4, K = 9 * KC;
  extern __shared__ __attribute__((aligned(16))) unsigned char cs_smem[];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int H = a.outH, W = a.outW, Wp = W + 2;
  const int rowb = Wp * KC * 2;                  // bytes per staged row
  // weights (MFMA A operand): lane -> output channel (lane & 15) of each 16-wide tile,
  // k chunk 4*s + (lane >> 4)
  cbf16x8 wf[NT][KSTEPS];
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int s = 0; s < KSTEPS; ++s) {
      const int n = t * 16 + (lane & 15), kc = 4 * s + (lane >> 4);
      uint4 v = make_uint4(0u, 0u, 0u, 0u);
      if (n < a.Ncol && kc < NCH) v = *reinterpret_cast<const uint4 *>(a.wp + (int64_t)n * K + kc * 8);
      wf[t][s] = __builtin_bit_cast(cbf16x8, v);
    }
  float bias[NT][4];
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int n = t * 16 + 4 * (lane >> 4) + i;
      bias[t][i] = (a.bias && n < a.Ncol) ? a.bias[n] : 0.f;
    }
  const int nbh = (H + TH - 1) / TH;
  for (int blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
    const int img = blk / nbh, r0 = (blk - img * nbh) * TH;
    const int rows = H - r0 < TH ? H - r0 : TH;
    // stage input rows r0-1 .. r0+TH, cols -1 .. W, 16 B (8 channels) per item
    const int items = (TH + 2) * Wp * CC;
    __syncthreads();                             // the previous tile's readers are done
    for (int i = tid; i < items; i += 256) {
      const int c8 = i % CC, px = i / CC;
      const int tr = px / Wp, tc = px - tr * Wp;
      const int ir = r0 - 1 + tr, ic = tc - 1;
      uint4 v = make_uint4(0u, 0u, 0u, 0u);
      if ((unsigned)ir < (unsigned)H && (unsigned)ic < (unsigned)W)
        v = *reinterpret_cast<const uint4 *>(a.src + (((int64_t)img * H + ir) * W + ic) * KC + c8 * 8);
      *reinterpret_cast<uint4 *>(cs_smem + (size_t)tr * rowb + (tc * KC + c8 * 8) * 2) = v;
    }
    __syncthreads();
    const int npx = rows * W, ngr = (npx + 15) / 16;
    for (int gi = w; gi < ngr; gi += 4) {
      const int q = gi * 16 + (lane & 15);
      const int qq = q < npx ? q : npx - 1;
      const int r = qq / W, c = qq - r * W;
      cf32x4 acc[NT];
#pragma unroll
      for (int t = 0; t < NT; ++t) acc[t] = cf32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int s = 0; s < KSTEPS; ++s) {
        const int kc = 4 * s + (lane >> 4);
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if (kc < NCH) {
          const int tap = kc / CC, c8 = kc - tap * CC;
          const int kh = tap / 3, kw = tap - kh * 3;
          const int tr = FLIP ? r + 2 - kh : r + kh, tc = FLIP ? c + 2 - kw : c + kw;
          v = *reinterpret_cast<const uint4 *>(cs_smem + (size_t)tr * rowb + (tc * KC + c8 * 8) * 2);
        }
        const cbf16x8 xf = __builtin_bit_cast(cbf16x8, v);
#pragma unroll
        for (int t = 0; t < NT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[t][s], xf, acc[t], 0, 0, 0);
      }
      if (q < npx) {
        bf16_t *o = a.out + (((int64_t)img * H + r0 + r) * W + c) * a.Ncol;
#pragma unroll
        for (int t = 0; t < NT; ++t) {
          const int n = t * 16 + 4 * (lane >> 4);
          if (n < a.Ncol) {
            const uint32_t lo = (uint32_t)f2bf(acc[t][0] + bias[t][0]) | ((uint32_t)f2bf(acc[t][1] + bias[t][1]) << 16);
            const uint32_t hi = (uint32_t)f2bf(acc[t][2] + bias[t][2]) | ((uint32_t)f2bf(acc[t][3] + bias[t][3]) << 16);
            *reinterpret_cast<uint2 *>(o + n) = make_uint2(lo, hi);
          }
        }
      }
    }
  }
}

bool launch_small(const FwdArgs &a, bool dgrad, hipStream_t s) {
  if (a.g.ks != 3 || a.g.stride != 1 || a.sgs != 0 || a.ogs != 0 || a.sgc != a.KC || a.ogc != a.Ncol ||
      a.KCr || a.addend || a.bn_part || a.pc >= 0 || a.outH != a.srcH || a.outW != a.srcW || a.outW > 256 ||
      a.Ncol % 8)
    return false;
  const int KC = a.KC, NT = (a.Ncol + 15) / 16;
  if (!((KC == 24 && NT <= 2) || (KC == 16 && NT <= 4))) return false;
  const int H = a.outH, W = a.outW;
  // rows per workgroup, LDS <= 64 KB: 4 rows for 24 channels (stage 1: 29 us; 2 / 6 / 8 rows
  // 34 / 31 / 33 us), 8 for 16 (the seperate conv: 119 us; 4 / 6 / 12 rows 129 / 123 / 133 us),
  // tools/small_ab.sh
  const int ldsmax = 64 * 1024;
  const int thmax = KC == 16 ? 8 : 4;
  int TH = thmax;
  while (TH > 1 && (TH + 2) * (W + 2) * KC * 2 > ldsmax) --TH;
  const size_t lds = (size_t)(TH + 2) * (W + 2) * KC * 2;
  const int64_t nblk64 = (int64_t)a.g.N * ((H + TH - 1) / TH);
  if (nblk64 >= (1ll << 31)) return false;
  const int nblk = (int)nblk64;
  const dim3 grid((unsigned)(g_grid_cap > 0 && nblk > g_grid_cap ? g_grid_cap : nblk));
#define EWVIT_SMALL(KC_, NT_)                                                                                     \
  do {                                                                                                          \
    if (dgrad)                                                                                                  \
      hipLaunchKernelGGL((conv3x3_small_kernel<KC_, NT_, true>), grid, dim3(256), lds, s, a, TH, nblk);        \
    else                                                                                                        \
      hipLaunchKernelGGL((conv3x3_small_kernel<KC_, NT_, false>), grid, dim3(256), lds, s, a, TH, nblk);       \
  } while (0)
  if (KC == 24) {
    if (NT == 1) EWVIT_SMALL(24, 1);
    else EWVIT_SMALL(24, 2);
  } else {
    if (NT <= 2) EWVIT_SMALL(16, 2);
    else EWVIT_SMALL(16, 4);
  }
#undef EWVIT_SMALL
  return true;
}

template <bool DGRAD, int KS, int BK, int PF>
static void launch_fwd_v(const FwdArgs &a, hipStream_t s) {
  if (a.Ncol <= 64) {
    dim3 grid(capped_mtiles(a.M, 1), 1);
    hipLaunchKernelGGL((conv_fwd_kernel<DGRAD, 64, KS, BK, PF>), grid, dim3(256), 0, s, a);
  } else {
    const int ntn = (a.Ncol + CBN - 1) / CBN;
    dim3 grid(capped_mtiles(a.M, ntn), (unsigned)ntn);
    hipLaunchKernelGGL((conv_fwd_kernel<DGRAD, 128, KS, BK, PF>), grid, dim3(256), 0, s, a);
  }
}

template <bool DGRAD, int KS>
static void launch_fwd_ks(const FwdArgs &a, hipStream_t s) {
  if (a.KC % 64 == 0 && a.sgc % 64 == 0) launch_fwd_v<DGRAD, KS, 64, 1>(a, s);
  else launch_fwd_v<DGRAD, KS, 32, 1>(a, s);
}

void launch_fwd(const FwdArgs &a, bool dgrad, hipStream_t s) {
  if (a.g.ks == 1) dgrad ? launch_fwd_ks<true, 1>(a, s) : launch_fwd_ks<false, 1>(a, s);
  else dgrad ? launch_fwd_ks<true, 3>(a, s) : launch_fwd_ks<false, 3>(a, s);
}

}  // namespace ewvit
