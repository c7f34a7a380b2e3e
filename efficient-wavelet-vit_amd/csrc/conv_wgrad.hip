// The weight gradients (conv.hip's header: the GEMM and layouts): the register-staged, LDS-DMA and
// 1x1 kernels, their split reduce, the split rules, the entry points (windowed kernel: convwin.hip).
#include "conv_common.h"
#include "reduce_jobs.h"

namespace ewvit {

// ---------------------------------------------------------------- wgrad
// C[co][n'] with n' = tap*Cin + ci, reduction over output pixels m.
template <int KS>
__global__ __launch_bounds__(256) void conv_wgrad_kernel(WgradArgs a) {
  __shared__ __attribute__((aligned(16))) unsigned char smem[2][2][CBK * 256];  // [buf][A/B][32 rows x 256 B]
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int wm = w >> 1, wn = w & 1;
  const int co0 = blockIdx.y * CBM;
  const int np0 = blockIdx.x * CBN;
  const int NP = KS * KS * a.g.Cin;
  const int64_t mbeg = (int64_t)blockIdx.z * a.mper;
  const int64_t mend = mbeg + a.mper < a.M ? mbeg + a.mper : a.M;
  const int nk = (int)((mend - mbeg + CBK - 1) / CBK);

  // staging: 32 rows x 16 chunks per operand = 512 vectors -> 2 per thread
  // vector v: row = v >> 4, chunk = v & 15
  int vrow[2], vch[2];
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int v = tid + 256 * u;
    vrow[u] = v >> 4;
    vch[u] = v & 15;
  }
  // the B chunk's (tap, ci) is fixed per thread
  int tkh[2], tkw[2];
  int64_t bgoff[2];      // grouped-layout offset of this chunk's channel
  bool bok[2];
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int np = np0 + vch[u] * 8;
    bok[u] = np < NP;
    const int btap = bok[u] ? np / a.g.Cin : 0;
    const int bci = bok[u] ? np - btap * a.g.Cin : 0;
    tkh[u] = btap / KS - a.g.pad;
    tkw[u] = btap % KS - a.g.pad;
    const int gi = bci / a.xgc;
    bgoff[u] = (int64_t)gi * a.xgs + (bci - gi * a.xgc);
  }
  // pixel coordinates of each staged row, advanced by CBK pixels per K-tile
  // (no 64-bit div/mod in the loop)
  int pn[2], poh[2], pow_[2];
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int64_t m = mbeg + vrow[u];
    pow_[u] = (int)(m % a.g.Wo);
    const int64_t t = m / a.g.Wo;
    poh[u] = (int)(t % a.g.Ho);
    pn[u] = (int)(t / a.g.Ho);
  }
  const bool do_bias = a.dbias_part != nullptr && blockIdx.x == 0;
  float bsum[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  auto load_tile = [&](int kt, uint4 (&ra)[2], uint4 (&rb)[2]) {
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int64_t m = mbeg + (int64_t)kt * CBK + vrow[u];
      const int co = co0 + vch[u] * 8;
      uint4 va = make_uint4(0u, 0u, 0u, 0u), vb = va;
      if (m < mend && co < a.g.Cout) va = *reinterpret_cast<const uint4 *>(a.dy + m * a.g.Cout + co);
      const int ih = poh[u] * a.g.stride + tkh[u], iw = pow_[u] * a.g.stride + tkw[u];
      if (m < mend && bok[u] && (unsigned)ih < (unsigned)a.g.H && (unsigned)iw < (unsigned)a.g.W)
        vb = *reinterpret_cast<const uint4 *>(a.x + bgoff[u] + (((int64_t)pn[u] * a.g.H + ih) * a.g.W + iw) * a.xgc);
      ra[u] = va;
      rb[u] = vb;
      pow_[u] += CBK;
      while (pow_[u] >= a.g.Wo) {
        pow_[u] -= a.g.Wo;
        if (++poh[u] == a.g.Ho) { poh[u] = 0; ++pn[u]; }
      }
    }
  };
  auto bias_acc = [&](const uint4 (&ra)[2]) {
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const unsigned wv[4] = {ra[u].x, ra[u].y, ra[u].z, ra[u].w};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        bsum[2 * j] += __uint_as_float(wv[j] << 16);
        bsum[2 * j + 1] += __uint_as_float(wv[j] & 0xffff0000u);
      }
    }
  };
  auto store_tile = [&](int buf, const uint4 (&ra)[2], const uint4 (&rb)[2]) {
    if (do_bias) bias_acc(ra);
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      *reinterpret_cast<uint4 *>(&smem[buf][0][swz_off(vrow[u], vch[u])]) = ra[u];
      *reinterpret_cast<uint4 *>(&smem[buf][1][swz_off(vrow[u], vch[u])]) = rb[u];
    }
  };
  // transposed fragment read: rows k0..k0+3 of an image, columns c0..c0+15 (16-lane group);
  // lane 4q+p supplies row k0+q, columns c0+4p..c0+4p+3
  auto tr_read = [&](const unsigned char *img, int k0, int c0) -> cs4 {
    const int i = lane & 15, q = i >> 2, p = i & 3;
    const int col = c0 + 4 * p;
    const int off = swz_off(k0 + q, col >> 3) + 2 * (col & 7);
    return __builtin_amdgcn_ds_read_tr16_b64_v4i16(
        (__attribute__((address_space(3))) cs4 *)(img + off));
  };

  cf32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = cf32x4{0.f, 0.f, 0.f, 0.f};

  const int g = lane >> 4;  // k rows 8g .. 8g+7 of the 32-row tile
  // same two-deep register prefetch as the fwd kernel
  auto step = [&](int kt, uint4 (&na)[2], uint4 (&nb)[2], const uint4 (&ra)[2], const uint4 (&rb)[2]) {
    const int cur = kt & 1;
    if (kt + 2 < nk) load_tile(kt + 2, na, nb);
    cbf16x8 af[4], bfr[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const cs4 lo = tr_read(smem[cur][0], 8 * g, wm * 64 + i * 16);
      const cs4 hi = tr_read(smem[cur][0], 8 * g + 4, wm * 64 + i * 16);
      af[i] = __builtin_bit_cast(cbf16x8, (__attribute__((ext_vector_type(8))) short){
                                              lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]});
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const cs4 lo = tr_read(smem[cur][1], 8 * g, wn * 64 + j * 16);
      const cs4 hi = tr_read(smem[cur][1], 8 * g + 4, wn * 64 + j * 16);
      bfr[j] = __builtin_bit_cast(cbf16x8, (__attribute__((ext_vector_type(8))) short){
                                               lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]});
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i], bfr[j], acc[i][j], 0, 0, 0);
    if (kt + 1 < nk) store_tile(cur ^ 1, ra, rb);
    __syncthreads();
  };
  uint4 pa[2], pb[2], qa[2], qb[2];
  if (nk > 0) {
    load_tile(0, pa, pb);
    if (nk > 1) load_tile(1, qa, qb);
    store_tile(0, pa, pb);
  }
  __syncthreads();
  int kt = 0;
  for (; kt + 1 < nk; kt += 2) {
    step(kt, pa, pb, qa, qb);
    step(kt + 1, qa, qb, pa, pb);
  }
  if (kt < nk) step(kt, pa, pb, qa, qb);
  if (do_bias) {
    // threads with equal (tid & 15) hold the same 8 channels: lanes l, l^16, l^32, l^48
    // in a wave, then the 4 waves through LDS (the staging buffers are free now)
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      bsum[j] = rows_sum4(bsum[j]);
    }
    float *red = reinterpret_cast<float *>(&smem[0][0][0]);  // [4 waves][16 chunks][8]
    if (lane < 16)
#pragma unroll
      for (int j = 0; j < 8; ++j) red[(w * 16 + lane) * 8 + j] = bsum[j];
    __syncthreads();
    if (tid < 128) {
      const int ch = tid >> 3, j = tid & 7;
      const int co = co0 + ch * 8 + j;
      const float s = (red[(0 * 16 + ch) * 8 + j] + red[(1 * 16 + ch) * 8 + j]) +
                      (red[(2 * 16 + ch) * 8 + j] + red[(3 * 16 + ch) * 8 + j]);
      if (co < a.g.Cout) a.dbias_part[(int64_t)blockIdx.z * a.g.Cout + co] = s;
    }
  }
  float *dst = a.part + (int64_t)blockIdx.z * a.g.Cout * NP;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int col = np0 + wn * 64 + j * 16 + (lane & 15);
    if (col >= NP) continue;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = co0 + wm * 64 + i * 16 + (lane >> 4) * 4 + r;
        if (row < a.g.Cout) dst[(int64_t)row * NP + col] = acc[i][j][r];
      }
  }
}

// dW[co][ci][tap] (= or +=) sum over splits of part[s][co][tap*Cin + ci] (wgrad_reduce_block,
// reduce_jobs.h; T chosen so ~64K threads run) — fixed order, deterministic.  Blocks >= nmain reduce
// the bias partials: 64 channels per block, 4 waves over the partial rows, fixed-order combine.
__global__ __launch_bounds__(256) void conv_wgrad_reduce_kernel(const float *__restrict__ part, float *__restrict__ dw,
                                                                int Cout, int Cin, int taps, int splits, int bparts,
                                                                int accumulate, const float *__restrict__ dbias_part,
                                                                float *__restrict__ dbias, WOut wo, int T, int nmain) {
  __shared__ float red[4][64];
  const int tid = threadIdx.x;
  if ((int)blockIdx.x >= nmain) {
    const int c = ((int)blockIdx.x - nmain) * 64 + (tid & 63), q = tid >> 6;
    float sb = 0.f;
    if (c < Cout) {
      int k = q;
      for (; k + 12 < bparts; k += 16) {
        float v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = dbias_part[(int64_t)(k + 4 * u) * Cout + c];
#pragma unroll
        for (int u = 0; u < 4; ++u) sb += v[u];
      }
      for (; k < bparts; k += 4) sb += dbias_part[(int64_t)k * Cout + c];
    }
    red[q][tid & 63] = sb;
    __syncthreads();
    if (tid < 64 && c < Cout) {
      const float r = (red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid]);
      dbias[c] = accumulate ? dbias[c] + r : r;
    }
    return;
  }
  // (the split sums: reduce_jobs.h, shared with the deferred form)
  wgrad_reduce_block(part, dw, Cin, taps, splits, accumulate, wo, T, (int64_t)Cout * taps * Cin, (int)blockIdx.x);
}

// wgrad: C[co][n'] over pixel K-tiles of BK; NS-deep ring of [pixel][128] images of
// 256-B rows, chunk c of row r at c ^ (((r&3)<<2) | ((r>>2)&3)) (read transposed,
// ds_read_b64_tr_b16).  Bias gradient (sum of dy over pixels): the blocks of n'-tile
// t sum the dy image of the K-tiles kt = t (mod n'-tiles), spreading the extra reads.
template <int KS, int BK, int NS, int WJ = 4>
__global__ __launch_bounds__(256) void conv_wgrad_glds_kernel(WgradArgs a, int64_t x_bytes, int ntx, int nty,
                                                              RedJobs rj) {
  constexpr int NB = WJ / 4;         // 128-column x images per stage (n'-tile of 128 * NB)
  constexpr int IMG = BK * 256, STG = (1 + NB) * IMG;
  constexpr int P = BK / 16;        // pieces (4 rows x 256 B) per wave per image
  __shared__ __attribute__((aligned(16))) unsigned char smem[NS * STG];
  // the first rj.nblk workgroups run deferred reductions of earlier weight gradients
  if ((int)blockIdx.x < rj.nblk) {
    run_red_jobs(rj, (int)blockIdx.x, reinterpret_cast<float *>(smem));
    return;
  }
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int tile = xcd_remap((int)blockIdx.x - rj.nblk, (int)gridDim.x - rj.nblk);
  const int split = tile / (ntx * nty);
  const int tx = tile % ntx, ty = (tile / ntx) % nty;
  const int co0 = ty * 128, np0 = tx * 128 * NB;
  const int NP = KS * KS * a.g.Cin;
  const int64_t mbeg = (int64_t)split * a.mper;
  const int64_t mend = mbeg + a.mper < a.M ? mbeg + a.mper : a.M;
  const int nk = (int)((mend - mbeg + BK - 1) / BK);
  const __amdgpu_buffer_rsrc_t rx = mk_rsrc(a.x, x_bytes);
  const __amdgpu_buffer_rsrc_t rd = mk_rsrc(a.dy, a.M * a.g.Cout * 2);

  // piece p = ws*P + j: rows 4p .. 4p+3; lane -> row 4p + lane/16, stored chunk lane%16.
  // A K-tile's first pixel (n0, oh0, ow0) is tracked in scalars; a row's pixel is that
  // plus r, carried through (ow, oh) with exact multiply-high divisions (r < 64).
  const int ws = __builtin_amdgcn_readfirstlane(w);
  const int wm = ws >> 1, wn = ws & 1;
  int rr[P], aoff[P], tkh[NB * P], tkw[NB * P], bgo[NB * P];
  bool aok[P], bok[NB * P];
#pragma unroll
  for (int j = 0; j < P; ++j) {
    const int p = ws * P + j, r = p * 4 + (lane >> 4);
    const int lc = (lane & 15) ^ (((r & 3) << 2) | ((r >> 2) & 3));
    rr[j] = r;
    aok[j] = co0 + lc * 8 < a.g.Cout;
    aoff[j] = (int)(((mbeg + r) * a.g.Cout + co0 + lc * 8) * 2);
#pragma unroll
    for (int b = 0; b < NB; ++b) {
      const int e = b * P + j;
      const int np = np0 + b * 128 + lc * 8;
      bok[e] = np < NP;
      const int btap = bok[e] ? np / a.g.Cin : 0;
      const int bci = bok[e] ? np - btap * a.g.Cin : 0;
      tkh[e] = btap / KS - a.g.pad;
      tkw[e] = btap % KS - a.g.pad;
      const int gi = bci / a.xgc;
      bgo[e] = (int)(((int64_t)gi * a.xgs + (bci - gi * a.xgc)) * 2);
    }
  }
  // exact floor(x / d) = umulhi(x, ceil(2^32 / d)) for x < 2^32 / d
  const uint32_t magW = (uint32_t)((0x100000000ull + a.g.Wo - 1) / a.g.Wo);
  const uint32_t magH = (uint32_t)((0x100000000ull + a.g.Ho - 1) / a.g.Ho);
  int sn = (int)(mbeg / ((int64_t)a.g.Ho * a.g.Wo));
  int soh = (int)((mbeg / a.g.Wo) % a.g.Ho);
  int sow = (int)(mbeg % a.g.Wo);
  const int xrow = a.xgc * 2;                       // bytes per pixel step
  auto stage = [&](int kt, int buf) {               // kt: the split's K-tile index
    unsigned char *base = smem + buf * STG + ws * P * 1024;
    const int lim = (int)(mend - mbeg) - kt * BK;   // rows r < lim are inside the split
    const int adel = kt * BK * a.g.Cout * 2;
#pragma unroll
    for (int j = 0; j < P; ++j) {
      glds16(rd, base + j * 1024, rr[j] < lim && aok[j] ? (uint32_t)(aoff[j] + adel) : OOB);
      const uint32_t owt = (uint32_t)(sow + rr[j]);
      const uint32_t q = __umulhi(owt, magW);
      const int ow = (int)(owt - q * a.g.Wo);
      const uint32_t oht = (uint32_t)soh + q;
      const uint32_t q2 = __umulhi(oht, magH);
      const int oh = (int)(oht - q2 * a.g.Ho);
      const int n = sn + (int)q2;
#pragma unroll
      for (int b = 0; b < NB; ++b) {
        const int e = b * P + j;
        const int ih = oh * a.g.stride + tkh[e], iw = ow * a.g.stride + tkw[e];
        const bool ok = rr[j] < lim && bok[e] && (unsigned)ih < (unsigned)a.g.H && (unsigned)iw < (unsigned)a.g.W;
        glds16(rx, base + (1 + b) * IMG + j * 1024,
               ok ? (uint32_t)(((n * a.g.H + ih) * a.g.W + iw) * xrow + bgo[e]) : OOB);
      }
    }
    sow += BK;                                      // the next K-tile (scalar)
    while (sow >= a.g.Wo) {
      sow -= a.g.Wo;
      if (++soh == a.g.Ho) { soh = 0; ++sn; }
    }
  };
  auto tr_read = [&](const unsigned char *img, int k0, int c0) -> cs4 {
    const int i = lane & 15, q = i >> 2, p = i & 3;
    const int col = c0 + 4 * p;
    const int off = swz_off(k0 + q, col >> 3) + 2 * (col & 7);
    return __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) cs4 *)(img + off));
  };
  const bool do_bias = a.dbias_part != nullptr;
  float bsum[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  cf32x4 acc[4][WJ];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < WJ; ++j) acc[i][j] = cf32x4{0.f, 0.f, 0.f, 0.f};
  const int g = lane >> 4;
  auto compute = [&](int kt, int buf) {
    const unsigned char *As = smem + buf * STG;
    // wave column wn: 64 columns of the one x image (WJ 4), or a whole image (WJ 8)
    const unsigned char *Bs = As + IMG + (NB > 1 ? wn * IMG : 0);
    const int bc0 = NB > 1 ? 0 : wn * 64;
#pragma unroll
    for (int ks = 0; ks < BK / 32; ++ks) {
      cbf16x8 af[4], bfr[WJ];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const cs4 lo = tr_read(As, ks * 32 + 8 * g, wm * 64 + i * 16);
        const cs4 hi = tr_read(As, ks * 32 + 8 * g + 4, wm * 64 + i * 16);
        af[i] = __builtin_bit_cast(cbf16x8, (__attribute__((ext_vector_type(8))) short){
                                                lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]});
      }
#pragma unroll
      for (int j = 0; j < WJ; ++j) {
        const cs4 lo = tr_read(Bs, ks * 32 + 8 * g, bc0 + j * 16);
        const cs4 hi = tr_read(Bs, ks * 32 + 8 * g + 4, bc0 + j * 16);
        bfr[j] = __builtin_bit_cast(cbf16x8, (__attribute__((ext_vector_type(8))) short){
                                                 lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]});
      }
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < WJ; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i], bfr[j], acc[i][j], 0, 0, 0);
    }
    if (do_bias && kt % ntx == tx) {
      // thread t of a K-group: rows (t>>4)*(BK/16) .. of its dy image, chunk t & 15 (8 channels)
#pragma unroll
      for (int q = 0; q < BK / 16; ++q) {
        const int r = (tid >> 4) * (BK / 16) + q;
        const uint4 v = *reinterpret_cast<const uint4 *>(As + swz_off(r, tid & 15));
        const unsigned wv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          bsum[2 * e] += __uint_as_float(wv[e] << 16);
          bsum[2 * e + 1] += __uint_as_float(wv[e] & 0xffff0000u);
        }
      }
    }
  };
  int ld = 0, lbuf = 0;
  for (; ld < NS - 1 && ld < nk; ++ld) {
    stage(ld, lbuf);
    lbuf = lbuf + 1 == NS ? 0 : lbuf + 1;
  }
  int cur = 0;
  for (int kt = 0; kt < nk; ++kt) {
    wait_tile<(1 + NB) * P, NS>(nk - 1 - kt);
    if (ld < nk) {
      stage(ld, lbuf);
      ++ld;
      lbuf = lbuf + 1 == NS ? 0 : lbuf + 1;
    }
    compute(kt, cur);
    cur = cur + 1 == NS ? 0 : cur + 1;
  }
  __syncthreads();
  if (do_bias) {
    // threads t, t^16, t^32, t^48 of a wave hold the same 8 channels; then the 4 waves
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      bsum[j] = rows_sum4(bsum[j]);
    }
    float *red = reinterpret_cast<float *>(smem);
    if (lane < 16)
#pragma unroll
      for (int j = 0; j < 8; ++j) red[(w * 16 + lane) * 8 + j] = bsum[j];
    __syncthreads();
    if (tid < 128) {
      const int ch = tid >> 3, j = tid & 7;
      const int co = co0 + ch * 8 + j;
      float s = (red[(0 * 16 + ch) * 8 + j] + red[(1 * 16 + ch) * 8 + j]) +
                (red[(2 * 16 + ch) * 8 + j] + red[(3 * 16 + ch) * 8 + j]);
      if (co < a.g.Cout) a.dbias_part[((int64_t)split * ntx + tx) * a.g.Cout + co] = s;
    }
  }
  float *dst = a.part + (int64_t)split * a.g.Cout * NP;
#pragma unroll
  for (int j = 0; j < WJ; ++j) {
    const int col = np0 + wn * 16 * WJ + j * 16 + (lane & 15);
    if (col >= NP) continue;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = co0 + wm * 64 + i * 16 + (lane >> 4) * 4 + r;
        if (row < a.g.Cout) dst[(int64_t)row * NP + col] = acc[i][j][r];
      }
  }
}

// 1x1 stride-1 weight gradient over a plain NHWC x (the backbone's MBConv expand / project and
// head convs, sfe.py:111-113): dW[co][ci] = sum_m dy[m][co] * x[m][ci] with no pixel map, so a
// staging lane's global offset is one register advanced by a scalar stride per K-tile (lanes
// past Cout / Cin start at OOB and stay there; rows >= M fall past the buffer's end and read
// zeros) — none of the generic kernel's per-piece address math; the DMAs are asm (glds16_asm),
// so hipcc does not drain them before the fragment reads.  128 x 128 output tile, 4 waves
// of 64 x 64, 64-pixel K-tiles in an NS-deep LDS-DMA ring; a K-tile's fragments for both
// 32-pixel steps are read before its MFMAs, so the second step's reads overlap the first
// step's MFMAs.  Leaves [splits][Cout][Cin] slabs (conv_wgrad_reduce_kernel), or dW itself for
// one split.
template <int NS>
__global__ __launch_bounds__(256) void conv_wgrad_1x1_kernel(WgradArgs a, int ntx, int nty, RedJobs rj) {
  constexpr int BK = 64, IMG = BK * 256, STG = 2 * IMG, P = BK / 16;
  __shared__ __attribute__((aligned(16))) unsigned char smem[NS * STG];
  // the first rj.nblk workgroups run deferred reductions of earlier weight gradients
  if ((int)blockIdx.x < rj.nblk) {
    run_red_jobs(rj, (int)blockIdx.x, reinterpret_cast<float *>(smem));
    return;
  }
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int tile = xcd_remap((int)blockIdx.x - rj.nblk, (int)gridDim.x - rj.nblk);
  const int split = tile / (ntx * nty);
  const int tx = tile % ntx, ty = (tile / ntx) % nty;
  const int co0 = ty * 128, ci0 = tx * 128;
  const int Cout = a.g.Cout, Cin = a.g.Cin;
  const int64_t mbeg = (int64_t)split * a.mper;
  const int64_t mend = mbeg + a.mper < a.M ? mbeg + a.mper : a.M;
  const int nk = (int)((mend - mbeg + BK - 1) / BK);
  const __amdgpu_buffer_rsrc_t rx = mk_rsrc(a.x, a.M * Cin * 2);
  const __amdgpu_buffer_rsrc_t rd = mk_rsrc(a.dy, a.M * Cout * 2);
  const int ws = __builtin_amdgcn_readfirstlane(w);
  const int wm = ws >> 1, wn = ws & 1;
  // piece j of wave ws: rows 16 ws + 4 j + lane / 16, source chunk (lane % 16) ^ swz(row)
  uint32_t aoff[P], boff[P];
#pragma unroll
  for (int j = 0; j < P; ++j) {
    const int r = ws * 16 + 4 * j + (lane >> 4);
    const int lc = (lane & 15) ^ (((r & 3) << 2) | ((r >> 2) & 3));
    aoff[j] = co0 + lc * 8 < Cout ? (uint32_t)(((mbeg + r) * Cout + co0 + lc * 8) * 2) : OOB;
    boff[j] = ci0 + lc * 8 < Cin ? (uint32_t)(((mbeg + r) * Cin + ci0 + lc * 8) * 2) : OOB;
  }
  const uint32_t adel = (uint32_t)(BK * Cout * 2), bdel = (uint32_t)(BK * Cin * 2);
  const uint32_t lds0 = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) unsigned char *)smem + ws * P * 1024;
  auto stage = [&](int buf) __attribute__((always_inline)) {
    const uint32_t base = lds0 + buf * STG;
#pragma unroll
    for (int j = 0; j < P; ++j) {
      glds16_asm(rd, base + j * 1024, aoff[j]);
      glds16_asm(rx, base + IMG + j * 1024, boff[j]);
      aoff[j] += adel;
      boff[j] += bdel;
    }
  };
  auto tr_read = [&](const unsigned char *img, int k0, int c0) __attribute__((always_inline)) -> cs4 {
    const int i = lane & 15, q = i >> 2, p = i & 3;
    const int col = c0 + 4 * p;
    const int off = swz_off(k0 + q, col >> 3) + 2 * (col & 7);
    return __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) cs4 *)(img + off));
  };
  cf32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = cf32x4{0.f, 0.f, 0.f, 0.f};
  const int g = lane >> 4;
  auto compute = [&](int buf) __attribute__((always_inline)) {
    const unsigned char *As = smem + buf * STG, *Bs = As + IMG;
    cbf16x8 af[2][4], bfr[2][4];
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const cs4 alo = tr_read(As, ks * 32 + 8 * g, wm * 64 + i * 16);
        const cs4 ahi = tr_read(As, ks * 32 + 8 * g + 4, wm * 64 + i * 16);
        af[ks][i] = __builtin_bit_cast(cbf16x8, (__attribute__((ext_vector_type(8))) short){
                                                     alo[0], alo[1], alo[2], alo[3], ahi[0], ahi[1], ahi[2], ahi[3]});
        const cs4 blo = tr_read(Bs, ks * 32 + 8 * g, wn * 64 + i * 16);
        const cs4 bhi = tr_read(Bs, ks * 32 + 8 * g + 4, wn * 64 + i * 16);
        bfr[ks][i] = __builtin_bit_cast(cbf16x8, (__attribute__((ext_vector_type(8))) short){
                                                      blo[0], blo[1], blo[2], blo[3], bhi[0], bhi[1], bhi[2], bhi[3]});
      }
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[ks][i], bfr[ks][j], acc[i][j], 0, 0, 0);
  };
  int ld = 0, lbuf = 0;
  for (; ld < NS - 1 && ld < nk; ++ld) {
    stage(lbuf);
    lbuf = lbuf + 1 == NS ? 0 : lbuf + 1;
  }
  int cur = 0;
  for (int kt = 0; kt < nk; ++kt) {
    wait_tile<2 * P, NS>(nk - 1 - kt);
    if (ld < nk) {
      stage(lbuf);
      ++ld;
      lbuf = lbuf + 1 == NS ? 0 : lbuf + 1;
    }
    compute(cur);
    cur = cur + 1 == NS ? 0 : cur + 1;
  }
  float *dst = a.part + (int64_t)split * Cout * Cin;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int col = ci0 + wn * 64 + j * 16 + (lane & 15);
    if (col >= Cin) continue;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = co0 + wm * 64 + i * 16 + (lane >> 4) * 4 + r;
        if (row < Cout) dst[(int64_t)row * Cin + col] = acc[i][j][r];
      }
  }
}

}  // namespace ewvit

using namespace ewvit;

// split of the pixel reduction: at most 512 workgroups — the 2 per CU that registers
// and LDS allow, so every split runs in the first (only) round — >= 4 K-tiles of 64
// pixels per split, and f32 partial slabs no larger than 4x the bf16 operands.
// Wide n'-tiles (128 x 256 per block, each wave 64 x 128: a quarter fewer LDS and L2 bytes
// per MFMA; 32 pixels per K-tile, 2-deep ring, 48 KB) for n' >= 2048 over >= 64K pixels
// (multiscale_fusion 384 -> 128, 3x3, 64 x 112^2: 951 -> 850 us; measured slower on
// freq_conv's n' = 1152 and on every backbone 1x1, which keep the 128-column tiles; the
// 64-pixel / 96 KB form ran 1233 us).  ewvit_conv2d_set_wgrad_wide: 4 auto (default), 2 wide
// whenever the shape allows it, 0 never (test switches).
static int g_wgw = 4;
static int wgrad_wide(const ConvGeom &g) {
  const int64_t NP = (int64_t)g.ks * g.ks * g.Cin;
  int v = g_wgw;
  if (v == 4) v = (NP >= 2048 && (int64_t)g.N * g.Ho * g.Wo >= 65536) ? 2 : 0;
  if (!v || NP < 256 || ((NP + 255) / 256 * 256 - NP) * 8 > NP) return 0;
  return 2;
}
static int64_t wgrad_splits(const ConvGeom &g, int wide = 0) {
  const int64_t M = (int64_t)g.N * g.Ho * g.Wo;
  const int64_t NP = (int64_t)g.ks * g.ks * g.Cin;
  const int64_t tn = wide ? 2 * CBN : CBN;
  const int64_t tiles = ((NP + tn - 1) / tn) * ((g.Cout + CBM - 1) / CBM);
  // (fewer, longer splits measured slower: 256 / 128 target workgroups for the backbone's
  // <= 28^2 maps 3231-3233 / 3148 frames/s against 3214-3231 at 512, round 4)
  int64_t s = 512 / tiles;
  if (g_grid_cap > 0 && s * tiles > g_grid_cap) s = g_grid_cap / tiles;
  const int64_t maxs = M / 256;
  if (s > maxs) s = maxs;
  const int64_t cap = 2 * M * ((int64_t)g.Cin + g.Cout) / ((int64_t)g.Cout * NP);
  if (s > cap) s = cap;
  if (s < 1) s = 1;
  return s;
}

// the 1x1 kernel (conv_wgrad_1x1_kernel): plain NHWC x, stride 1, no bias gradient; splits for
// ~g_w1_wg workgroups with >= g_w1_minkt K-tiles of 64 pixels each, slabs <= 4x the operands
// (256 / 8 / 2-deep ring: stage-6 expand 22.2 -> 18.4 us, stage-5 23.7 -> 19.2 us, stage-4
// 26.6 -> 22.7 us against the generic kernel, profiles/r05/ab/wgrad1x1_kernel.log).
// ewvit_conv2d_set_wgrad_1x1 (test / tuning): workgroup target (0 = never), min K-tiles, ring.
static int g_w1_wg = 256, g_w1_minkt = 8, g_w1_ring = 2;
static bool w1x1_ok(const ConvGeom &g, int64_t x_group_stride, bool has_bias, int64_t M) {
  return g_w1_wg > 0 && g.ks == 1 && g.stride == 1 && x_group_stride == 0 && !has_bias &&
         M * g.Cin * 2 < (int64_t)OOB / 2 && M * g.Cout * 2 < (int64_t)OOB / 2;
}
static int64_t w1x1_splits(const ConvGeom &g) {
  const int64_t M = (int64_t)g.N * g.Ho * g.Wo;
  const int64_t tiles = ((g.Cin + CBN - 1) / CBN) * ((g.Cout + CBM - 1) / CBM);
  int64_t s = g_w1_wg / tiles;
  const int64_t maxs = ((M + 63) / 64) / g_w1_minkt;
  if (s > maxs) s = maxs;
  const int64_t cap = 2 * M * ((int64_t)g.Cin + g.Cout) / ((int64_t)g.Cout * g.Cin);
  if (s > cap) s = cap;
  return s < 1 ? 1 : s;
}
// min_ktiles < 1 / ring not 2 or 3 keep the current value (so a caller can move the workgroup
// target alone and restore it without knowing the other two knobs)
extern "C" int ewvit_conv2d_set_wgrad_1x1(int target_wg, int min_ktiles, int ring) {
  const int prev = g_w1_wg;
  g_w1_wg = target_wg;
  if (min_ktiles >= 1) g_w1_minkt = min_ktiles;
  if (ring == 2 || ring == 3) g_w1_ring = ring;
  return prev;
}
// the three knobs: 0 workgroup target, 1 min K-tiles, 2 ring slots
extern "C" int ewvit_conv2d_wgrad_1x1_config(int which) {
  return which == 0 ? g_w1_wg : which == 1 ? g_w1_minkt : g_w1_ring;
}

extern "C" int ewvit_conv2d_set_wgrad_wide(int variant) {
  const int prev = g_wgw;
  g_wgw = variant == 0 || variant == 2 ? variant : 4;
  return prev;
}

extern "C" int64_t ewvit_conv2d_bwd_weight_workspace(int64_t N, int64_t H, int64_t W, int64_t Cin, int64_t Cout,
                                                     int ksize, int stride) {
  ConvGeom g = mkg(N, H, W, Cin, Cout, ksize, stride);
  // the windowed kernel (convwin.hip): [splits][Cout][9 Cin] slabs + [splits][Cout] bias partials
  const int wsp = wgrad_win_splits(wgrad_args(g, Cin, 0), 2 * N * H * W * Cin);
  const int64_t winb = (int64_t)wsp * Cout * (9 * Cin + 1) * (int64_t)sizeof(float);
  const int64_t ntx = (ksize * ksize * Cin + CBN - 1) / CBN;
  const int64_t narrow = wgrad_splits(g) * Cout * (ksize * ksize * Cin + ntx) * (int64_t)sizeof(float);
  const int wide = wgrad_wide(g);
  int64_t need = narrow > winb ? narrow : winb;
  if (w1x1_ok(g, 0, false, (int64_t)N * H * W)) {
    const int64_t w1 = w1x1_splits(g) * Cout * Cin * (int64_t)sizeof(float);
    if (w1 > need) need = w1;
  }
  if (!wide) return need;
  const int64_t ntw = (ksize * ksize * Cin + 2 * CBN - 1) / (2 * CBN);
  const int64_t wb = wgrad_splits(g, wide) * Cout * (ksize * ksize * Cin + ntw) * (int64_t)sizeof(float);
  return wb > need ? wb : need;
}

// The tail of every weight gradient: dW (= or +=) the sum of the `splits` slabs of `ws`, dbias
// that of the `bparts` rows of `dbias_part`.  T = split lanes per output: ~64K threads, <= splits,
// <= 64.  `defer` (the caller's mark, on the paths whose next launch can carry the job): queued
// for the stream's next weight-gradient launch instead of launched (reduce_jobs.h).
static int wgrad_finish(const char *what, const ConvGeom &g, float *ws, float *dw, float *dbias,
                        const float *dbias_part, int splits, int bparts, const WOut &wo, int accumulate, bool defer,
                        hipStream_t s) {
  const int taps = g.ks * g.ks;
  const int64_t n4 = (int64_t)g.Cout * taps * g.Cin / 4;
  int T = 1;
  while (T < 64 && T * 2 <= splits && n4 * T * 2 <= 65536) T *= 2;
  if (defer) {
    RedJob j;
    j.kind = 1; j.part = ws; j.dw = dw; j.n = n4 * 4; j.Cin = g.Cin; j.taps = taps; j.splits = splits;
    j.accumulate = accumulate; j.T = T; j.wo = wo;
    reduce_defer(s, j);
    return 0;
  }
  const int64_t nmain = (n4 * T + 255) / 256;
  const int64_t nbias = dbias ? (g.Cout + 63) / 64 : 0;
  hipLaunchKernelGGL(conv_wgrad_reduce_kernel, dim3((unsigned)(nmain + nbias)), dim3(256), 0, s, ws, dw, g.Cout,
                     g.Cin, taps, splits, bparts, accumulate, dbias_part, dbias, wo, T, (int)nmain);
  return launch_status(what);
}

extern "C" int ewvit_conv2d_bwd_weight(const void *x, const void *dy, float *dw, float *dbias, int accumulate,
                                       int64_t N, int64_t H, int64_t W, int64_t Cin, int64_t Cout, int ksize,
                                       int stride, int64_t x_group_c, int64_t x_group_stride, int64_t dw_cin,
                                       int64_t dw_s_co, int64_t dw_s_ci, int64_t dw_s_tap, float *workspace,
                                       void *stream) {
  // (the caller's "defer this reduce" mark is consumed by every call, whatever path it takes)
  const bool defer_mark = reduce_take_defer();
  EWVIT_CHECK_ARG(x && dy && dw && workspace, "conv2d_bwd_weight: null pointer");
  ConvGeom g = mkg(N, H, W, Cin, Cout, ksize, stride);
  if (int rc = check_geom(g, "conv2d_bwd_weight")) return rc;
  if (int rc = check_group(x_group_c, x_group_stride, Cin, N * H * W, "conv2d_bwd_weight", "x")) return rc;
  EWVIT_CHECK_ARG(dw_cin > 0 && dw_cin <= Cin, "conv2d_bwd_weight: dw_cin %lld not in (0, %lld]", (long long)dw_cin,
                  (long long)Cin);
  const int taps = ksize * ksize;
  WgradArgs a = wgrad_args(g, x_group_c, x_group_stride);
  a.x = (const bf16_t *)x; a.dy = (const bf16_t *)dy; a.part = workspace;
  const WOut wo{dw_s_co, dw_s_ci, dw_s_tap, (int)dw_cin};
  hipStream_t s = as_stream(stream);
  const int64_t xb = grouped_bytes(N * H * W, Cin, x_group_c, x_group_stride);
  const bool glds = use_glds() && xb < (int64_t)OOB && a.M * g.Cout * 2 < (int64_t)OOB;
  // the windowed kernel (convwin.hip): 3x3 stride 1 over maps of whole 8 x 16 tiles
  const int wsp = glds ? wgrad_win_splits(a, xb) : 0;
  if (wsp > 0) {
    a.dbias_part = dbias ? workspace + (int64_t)wsp * g.Cout * taps * g.Cin : nullptr;
    launch_wgrad_win(a, xb, wsp, s);
    if (int rc = launch_status("conv2d_bwd_weight (windowed)")) return rc;
    return wgrad_finish("conv2d_bwd_weight reduce", g, workspace, dw, dbias, a.dbias_part, wsp, wsp, wo, accumulate,
                        false, s);
  }
  if (glds && w1x1_ok(g, x_group_stride, dbias != nullptr, a.M)) {
    // the 1x1 kernel: K-tile-aligned splits, slabs + the reduce pass (or dW itself, one split)
    const int ntx = (g.Cin + CBN - 1) / CBN, nty = (g.Cout + CBM - 1) / CBM;
    const int64_t sp0 = w1x1_splits(g);
    int64_t mper = (a.M + sp0 - 1) / sp0;
    a.mper = (mper + 63) / 64 * 64;
    const int sp = (int)((a.M + a.mper - 1) / a.mper);
    a.dbias_part = nullptr;
    const bool direct = sp == 1 && !accumulate && dw_cin == Cin && dw_s_ci == 1 && dw_s_co == Cin;
    a.part = direct ? dw : workspace;
    // deferred reductions of earlier weight gradients on this stream ride in front of the tiles
    const RedJobs rj = reduce_take_jobs(s);
    const unsigned nwg = (unsigned)((int64_t)ntx * nty * sp + rj.nblk);
    if (g_w1_ring == 2) hipLaunchKernelGGL(conv_wgrad_1x1_kernel<2>, dim3(nwg), dim3(256), 0, s, a, ntx, nty, rj);
    else hipLaunchKernelGGL(conv_wgrad_1x1_kernel<3>, dim3(nwg), dim3(256), 0, s, a, ntx, nty, rj);
    if (int rc = launch_status("conv2d_bwd_weight (1x1)")) return rc;
    if (direct) return 0;
    return wgrad_finish("conv2d_bwd_weight reduce", g, workspace, dw, nullptr, nullptr, sp, 0, wo, accumulate,
                        defer_mark, s);
  }
  const int wide = glds ? wgrad_wide(g) : 0;
  const int64_t splits = wgrad_splits(g, wide);
  a.dbias_part = dbias ? workspace + splits * g.Cout * taps * (int64_t)g.Cin : nullptr;
  const int tnw = wide ? 2 * CBN : CBN;
  const int ntx = (taps * g.Cin + tnw - 1) / tnw, nty = (g.Cout + CBM - 1) / CBM;
  const int64_t kq = !glds ? CBK : wide ? 32 : 64;  // K-tile depth (pixels)
  int64_t mper = (a.M + splits - 1) / splits;
  mper = (mper + kq - 1) / kq * kq;
  a.mper = mper;
  const int sp = (int)((a.M + mper - 1) / mper);
  // the glds kernel leaves bias partials per (split, n'-tile); the old one per split
  const int bparts = glds ? sp * ntx : sp;
  // one split of a 1x1 conv whose dW is [Cout][Cin] row-major: the slab IS dW (and
  // dbias) — no reduce pass
  const bool direct = sp == 1 && taps == 1 && !accumulate && (!dbias || bparts == 1) && dw_cin == Cin &&
                      dw_s_ci == 1 && dw_s_co == Cin;
  if (direct) { a.part = dw; a.dbias_part = dbias; }
  if (glds) {
    const RedJobs rj = reduce_take_jobs(s);
    const unsigned nwg = (unsigned)((int64_t)ntx * nty * sp + rj.nblk);
#define EWVIT_GLDS_WG(BK_, NS_, WJ_)                                                                        \
  do {                                                                                                    \
    if (ksize == 1) hipLaunchKernelGGL((conv_wgrad_glds_kernel<1, BK_, NS_, WJ_>), dim3(nwg), dim3(256), 0, s, a, xb, ntx, nty, rj); \
    else hipLaunchKernelGGL((conv_wgrad_glds_kernel<3, BK_, NS_, WJ_>), dim3(nwg), dim3(256), 0, s, a, xb, ntx, nty, rj);            \
  } while (0)
    if (wide) EWVIT_GLDS_WG(32, 2, 8);
    else EWVIT_GLDS_WG(64, 2, 4);
#undef EWVIT_GLDS_WG
  } else {
    dim3 grid((unsigned)ntx, (unsigned)nty, (unsigned)sp);
    if (ksize == 1) hipLaunchKernelGGL(conv_wgrad_kernel<1>, grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL(conv_wgrad_kernel<3>, grid, dim3(256), 0, s, a);
  }
  if (int rc = launch_status("conv2d_bwd_weight")) return rc;
  if (direct) return 0;
  return wgrad_finish("conv2d_bwd_weight reduce", g, workspace, dw, dbias, a.dbias_part, sp, bparts, wo, accumulate,
                      defer_mark && glds && !dbias, s);
}

// dW (+ db) of the conv over relu(x * scale + shift) (see ewvit_conv2d_fwd_bn_xf): the windowed
// kernel with the transform in its x staging, then the split reduction; same workspace as
// ewvit_conv2d_bwd_weight
extern "C" int ewvit_conv2d_bwd_weight_xf(const void *x, const void *dy, float *dw, float *dbias, int accumulate,
                                          int64_t N, int64_t H, int64_t W, int64_t Cin, int64_t Cout,
                                          int64_t x_group_c, int64_t x_group_stride, const float *xf, int64_t dw_cin,
                                          int64_t dw_s_co, int64_t dw_s_ci, int64_t dw_s_tap, float *workspace,
                                          void *stream) {
  EWVIT_CHECK_ARG(x && dy && dw && xf && workspace, "conv2d_bwd_weight_xf: null pointer");
  ConvGeom g = mkg(N, H, W, Cin, Cout, 3, 1);
  if (int rc = check_geom(g, "conv2d_bwd_weight_xf")) return rc;
  if (int rc = check_group(x_group_c, x_group_stride, Cin, N * H * W, "conv2d_bwd_weight_xf", "x")) return rc;
  FwdArgs fa;
  WgradArgs a;
  EWVIT_CHECK_ARG(xf_args(fa, a, g, x_group_c, x_group_stride),
                  "conv2d_bwd_weight_xf: shape not taken by the windowed kernels (query ewvit_conv2d_xf_ok)");
  EWVIT_CHECK_ARG(dw_cin > 0 && dw_cin <= Cin, "conv2d_bwd_weight_xf: dw_cin %lld not in (0, %lld]", (long long)dw_cin,
                  (long long)Cin);
  a.x = (const bf16_t *)x; a.dy = (const bf16_t *)dy; a.xf = xf;
  const int64_t xb = grouped_bytes(N * H * W, Cin, x_group_c, x_group_stride);
  const int wsp = wgrad_win_splits(a, xb);
  a.part = workspace;
  a.dbias_part = dbias ? workspace + (int64_t)wsp * g.Cout * 9 * g.Cin : nullptr;
  hipStream_t s = as_stream(stream);
  launch_wgrad_win(a, xb, wsp, s);
  if (int rc = launch_status("conv2d_bwd_weight_xf (windowed)")) return rc;
  const WOut wo{dw_s_co, dw_s_ci, dw_s_tap, (int)dw_cin};
  return wgrad_finish("conv2d_bwd_weight_xf reduce", g, workspace, dw, dbias, a.dbias_part, wsp, wsp, wo, accumulate,
                      false, s);
}
