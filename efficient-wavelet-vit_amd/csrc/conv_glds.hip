// The LDS-DMA implicit-GEMM fwd / dgrad (conv.hip's header: the GEMMs and layouts), its split-K
// epilogue and per-stream scratch, and the tile rules.
#include "conv_common.h"

#include <map>
#include <mutex>

namespace ewvit {

// The same three GEMMs with the operands moved HBM/L2 -> LDS by buffer_load ... lds
// (16 B per lane, no register round trip, no ds_write), for the shapes whose K-tiles
// stay inside one tap and one channel group (fwd/dgrad: KC % 64 == 0; wgrad: Cin %
// 128 == 0 or 1x1).  Out-of-image taps and ragged tile edges are zero-filled by the
// buffer descriptor's range check (the lane's offset is pushed past num_records),
// so there is no per-lane branch around a load.  The DMA writes each wave's 1 KiB
// piece lane-linearly; the XOR swizzle that keeps the fragment reads conflict-free
// is applied to the lane's SOURCE address and undone on the read (the swizzle is an
// involution).  One K-tile is in flight while the previous one is multiplied; grid
// order is remapped so that consecutive tiles (which share input halo rows and, for
// wgrad, the same pixels) run on one XCD and meet in its L2.
// fwd / dgrad: BM x BN_ x 64 tiles, BM/32 waves (BM/64 x 2), NS-deep LDS ring of
// [row][64 k] images (128-B rows); 16-B chunk c of row r is stored at chunk
// c ^ ((r >> 1) & 7): conflict-free ds_read_b128 fragment reads
// DENSE (forward, plain NHWC x, Cin % 8 == 0 and not a multiple of 64: the backbone's 24 /
// 48 / 96-channel inputs, the MWT seperate conv's 16): the K axis is taps x Cin flattened
// ([Cout][taps][Cin] packs are exactly that), so a 64-wide K-tile spans several taps —
// each 16-B chunk of a row is (tap, 8 channels), with its own tap offset and in-image test.
// A lane's chunk index is fixed per row, so it advances by 8 chunks per K-tile: tap +=
// 8 / CC, cc += 8 % CC (CC = Cin / 8).  Zero waste but the last K-tile's tail (A past the
// last tap reads through the OOB offset, B's tail meets only those zeros).
// BST (dgrad): the backward statistics of the BatchNorm before the conv (FwdArgs::bwd) in
// the epilogue — its own instantiation, so the plain dgrad keeps its register budget
template <bool DGRAD, int BM, int BN_, int KS, int NS, int WC = 2, bool DENSE = false, bool BST = false>
__global__ __launch_bounds__(BM / 64 * WC * 64) void conv_glds_kernel(FwdArgs a, int64_t src_bytes, int ntn,
                                                                      int tap_inner, int ntiles) {
  static_assert(!(DENSE && DGRAD), "dense K: forward only");
  static_assert(!BST || DGRAD, "backward statistics: dgrad only");
  constexpr int NW = BM / 64 * WC, BK = 64;      // waves: BM/64 rows x WC columns
  constexpr int WN = BN_ / WC, J = WN / 16;
  constexpr int A_B = BM * BK * 2, B_B = BN_ * BK * 2, STG = A_B + B_B;
  constexpr int PA = BM / 8 / NW, PB = BN_ / 8 / NW;   // 1 KiB pieces per wave per K-tile
  static_assert(PB >= 1, "tile shape");
  // BatchNorm statistics image (fwd, or dgrad with BST), after the ring
  constexpr int RED_B = (DGRAD && !BST) ? 0 : BM / 64 * BN_ * 2 * 4;
  __shared__ __attribute__((aligned(16))) unsigned char smem[NS * STG + RED_B];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int ws = __builtin_amdgcn_readfirstlane(w);   // wave id, provably uniform
  const int wm = ws / WC, wn = ws % WC;
  if ((int)blockIdx.x >= ntiles) return;
  const int K = KS * KS * a.KC;
  const int cbn = (a.KC + BK - 1) / BK;   // ragged KC: the last block's lanes >= KC read zeros
  const bool cls = DGRAD && KS == 3 && a.pc >= 0;
  const int py = a.pc >> 1, px = a.pc & 1;
  const int ntaps = cls ? a.ntap : KS * KS;
  const int CC = a.KC >> 3;                // DENSE: 8-channel chunks per tap
  const int KSP = a.ksplit;                // split K: K-tiles per work item nk / KSP
  const int nk = (DENSE ? (K + BK - 1) / BK : ntaps * cbn) / KSP;
  const int tq = DENSE ? 8 / CC : 0, tr = DENSE ? 8 % CC : 0;   // DENSE: per-K-tile tap / chunk advance
  const int ls = a.g.stride >> 1, smask = a.g.stride - 1;
  const __amdgpu_buffer_rsrc_t rs = mk_rsrc(a.src, src_bytes);
  const __amdgpu_buffer_rsrc_t rw = mk_rsrc(a.wp, (int64_t)a.Ncol * K * 2);
  // (builtin DMAs: hipcc then waits vmcnt(4) ahead of each K-tile's fragment reads, so one
  // K-tile stays in flight whatever NS.  The asm DMAs of the windowed kernels, which leave
  // NS-1 in flight, measured slower here — the step 18.29 -> 18.56 ms on one box,
  // profiles/r05/ab/glds_asm_vs_builtin_ab.log: the backbone's small grids share the CUs with
  // the MWT stream, and deeper DMA queues cost that stream more than they gain)

  // A rows staged by this lane: piece p = w*PA + j covers rows 8p..8p+7.  Every tap's
  // source pixel is the row's base pixel plus a tap offset that is the same for all
  // rows (fwd: +(kh*W + kw); dgrad: -(kh*W + kw), or -((kh/2)*W + kw/2) at stride 2),
  // so a row keeps one byte offset and a mask of the taps that land inside the image
  // (and, for stride-2 dgrad, on the stride lattice); a K-tile adds one scalar.
  //
  // Tile loop: one tile per workgroup, or — with a capped grid (ewvit_set_grid_cap: a
  // branch sharing the GPU with another stream) — a persistent walk over the tiles.  The
  // staging cursor runs ahead of the compute cursor across tile boundaries: the next
  // tile's first K-tiles are in flight while this tile's last ones are multiplied and its
  // epilogue stores, so a walk pays the ring's fill latency once, not once per tile.
  int rb[PA], lc8[PA];
  unsigned vmask[PA];
  int dtap[PA], dcc[PA];  // DENSE: the (tap, chunk) each piece stages next
  uint32_t boff[PB];      // B (packed weights) byte offset of K-tile 0, or OOB
  const int kcr = a.KCr ? a.KCr : a.KC;
  // K-tile cursor: tap, channel block, group index / offset of the block.  With
  // tap_inner the 9 taps of one 64-channel block are consecutive K-tiles, so a block's
  // live input window (its pixels + halo, 64 channels) stays small enough for the
  // XCD's L2 to serve the tap re-reads; otherwise taps are outer.
  int ltap = 0, lcb = 0, lgi = 0, lcin = 0;
  auto setup = [&](int item) {          // the staged tile's row / column offsets
  const int tile = item / KSP;
  const int64_t m0 = (int64_t)(tile / ntn) * BM;
  const int n0 = (tile % ntn) * BN_;
  ltap = 0; lcb = 0; lgi = 0; lcin = 0;
  if (KSP > 1) { lcb = (item % KSP) * nk; lcin = lcb * BK; }   // (1x1, one channel group)
#pragma unroll
  for (int j = 0; j < PA; ++j) {
    const int p = ws * PA + j, r = p * 8 + (lane >> 3);
    const int lc = (lane & 7) ^ ((r >> 1) & 7);
    const int64_t m = m0 + r;
    const int64_t mm = m < a.M ? m : 0;
    const int ow = (int)(mm % a.outW);
    const int64_t t = mm / a.outW;
    const int oh = (int)(t % a.outH);
    const int n = (int)(t / a.outH);
    int by, bx;            // base pixel (may lie outside the image)
    unsigned msk = 0;
    if (cls) {
      // class taps: dy pixel (oh + dh, ow + dw), dh = (py + 1 - kh) / 2 in {0, 1} (unrolled:
      // a runtime index into the kernel argument's tapl[] puts the argument on the stack)
#pragma unroll
      for (int lt = 0; lt < 4; ++lt) {
        if (lt >= a.ntap) break;
        const int tp = a.tapl[lt], kh = tp / 3, kw = tp - kh * 3;
        const int sh = oh + ((py + 1 - kh) >> 1), sw = ow + ((px + 1 - kw) >> 1);
        if (m < a.M && sh < a.srcH && sw < a.srcW) msk |= 1u << lt;
      }
    } else
#pragma unroll
    for (int kh = 0; kh < KS; ++kh)
#pragma unroll
      for (int kw = 0; kw < KS; ++kw) {
        int sh, sw;
        bool ok = m < a.M;
        if (!DGRAD) {
          sh = oh * a.g.stride - a.g.pad + kh; sw = ow * a.g.stride - a.g.pad + kw;
        } else {
          const int th = oh + a.g.pad - kh, tw = ow + a.g.pad - kw;
          ok = ok && th >= 0 && tw >= 0 && !((th | tw) & smask);
          sh = th >> ls; sw = tw >> ls;
        }
        ok = ok && (unsigned)sh < (unsigned)a.srcH && (unsigned)sw < (unsigned)a.srcW;
        if (ok) msk |= 1u << (kh * KS + kw);
      }
    if (!DGRAD) { by = oh * a.g.stride - a.g.pad; bx = ow * a.g.stride - a.g.pad; }
    else if (cls) { by = oh; bx = ow; }
    else        { by = (oh + a.g.pad) >> ls;       bx = (ow + a.g.pad) >> ls; }
    const int64_t pix = (int64_t)n * a.srcH * a.srcW + (int64_t)by * a.srcW + bx;
    rb[j] = (int)((pix * a.sgc + (DENSE ? 0 : lc * 8)) * 2);
    vmask[j] = msk;
    lc8[j] = lc * 8;
    if (DENSE) { dtap[j] = lc / CC; dcc[j] = lc - dtap[j] * CC; }
  }
#pragma unroll
  for (int j = 0; j < PB; ++j) {
    const int p = ws * PB + j, r = p * 8 + (lane >> 3);
    const int lc = (lane & 7) ^ ((r >> 1) & 7);
    const int n = n0 + r;
    boff[j] = n < a.Ncol ? (uint32_t)(((int64_t)n * K + lc * 8) * 2) : OOB;
  }
  };
  int ld = 0;             // K-tiles of the staged tile issued so far
  auto stage = [&](int buf) {
    if constexpr (DENSE) {
      unsigned char *base = smem + buf * STG + ws * PA * 1024;
#pragma unroll
      for (int j = 0; j < PA; ++j) {
        const int tp = dtap[j];
        const int kh = (tp * 11) >> 5, kw = tp - kh * 3;     // tp / 3 for tp < 32 (KS == 3)
        const int dpix = KS == 3 ? kh * a.srcW + kw : 0;
        const bool ok = (tp < KS * KS) & (((vmask[j] >> tp) & 1u) != 0);
        glds16(rs, base + j * 1024, ok ? (uint32_t)(rb[j] + (dpix * a.sgc + dcc[j] * 8) * 2) : OOB);
        dtap[j] += tq;
        dcc[j] += tr;
        if (dcc[j] >= CC) { dcc[j] -= CC; ++dtap[j]; }
      }
      unsigned char *bb = smem + buf * STG + A_B + ws * PB * 1024;
      const uint32_t kb = (uint32_t)(ld * BK * 2);
#pragma unroll
      for (int j = 0; j < PB; ++j) glds16(rw, bb + j * 1024, boff[j] == OOB ? OOB : boff[j] + kb);
      return;
    }
    const int rt = cls ? (ltap == 0 ? a.tapl[0] : ltap == 1 ? a.tapl[1] : ltap == 2 ? a.tapl[2] : a.tapl[3])
                       : ltap;                     // the weight tap
    const int kh = rt / KS, kw = rt - kh * KS;
    int dpix;
    if (!DGRAD) dpix = kh * a.srcW + kw;
    else if (cls) dpix = ((py + 1 - kh) >> 1) * a.srcW + ((px + 1 - kw) >> 1);
    else dpix = -((kh >> ls) * a.srcW + (kw >> ls));
    const int sdelta = (int)(((int64_t)dpix * a.sgc + (int64_t)lgi * a.sgs + lcin) * 2);
    const int tap = ltap, c0 = lcin;
    const uint32_t kb = (uint32_t)((rt * a.KC + lcb * BK) * 2);
    if (tap_inner) {
      if (++ltap == ntaps) {
        ltap = 0; ++lcb;
        lcin += BK;
        if (lcin == a.sgc) { lcin = 0; ++lgi; }
      }
    } else {
      lcin += BK;
      if (lcin == a.sgc) { lcin = 0; ++lgi; }
      if (++lcb == cbn) { lcb = 0; ++ltap; lgi = 0; lcin = 0; }
    }
    unsigned char *base = smem + buf * STG + ws * PA * 1024;
#pragma unroll
    for (int j = 0; j < PA; ++j)
      glds16(rs, base + j * 1024,
                 ((((vmask[j] >> tap) & 1u) != 0) & (c0 + lc8[j] < kcr)) ? (uint32_t)(rb[j] + sdelta) : OOB);
    unsigned char *bb = smem + buf * STG + A_B + ws * PB * 1024;
#pragma unroll
    for (int j = 0; j < PB; ++j) glds16(rw, bb + j * 1024, boff[j] == OOB ? OOB : boff[j] + kb);
  };

  cf32x4 acc[4][J];
  const int fr = lane & 15, fq = lane >> 4;
  auto frag = [&](const unsigned char *img, int r, int ch) -> cbf16x8 {
    return *reinterpret_cast<const cbf16x8 *>(img + r * 128 + 16 * (ch ^ ((r >> 1) & 7)));
  };
  // both 32-deep steps' fragments are read before the MFMAs, so the second step's reads run
  // under the first step's MFMAs
  auto compute = [&](int buf) {
    const unsigned char *As = smem + buf * STG, *Bs = As + A_B;
    cbf16x8 af[BK / 32][4], bfr[BK / 32][J];
#pragma unroll
    for (int ks = 0; ks < BK / 32; ++ks) {
#pragma unroll
      for (int i = 0; i < 4; ++i) af[ks][i] = frag(As, wm * 64 + i * 16 + fr, ks * 4 + fq);
#pragma unroll
      for (int j = 0; j < J; ++j) bfr[ks][j] = frag(Bs, wn * WN + j * 16 + fr, ks * 4 + fq);
    }
#pragma unroll
    for (int ks = 0; ks < BK / 32; ++ks)
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < J; ++j)
          // operands swapped (B first): the lane holds 4 consecutive output COLUMNS of
          // one row, acc[i][j][r] = C[i*16 + (lane&15)][j*16 + 4*(lane>>4) + r], so the
          // epilogue stores 8 B per lane straight from registers (no LDS image)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bfr[ks][j], af[ks][i], acc[i][j], 0, 0, 0);
  };
  // `inflight` counts issued K-tiles not yet multiplied (<= NS-1); the buffer refilled is
  // always the one every wave finished reading before the last barrier
  int ts = blockIdx.x, lbuf = 0, inflight = 0, cur = 0;
  ld = 0;
  setup(xcd_remap(ts, ntiles));
  for (; ld < NS - 1 && ld < nk; ++ld, ++inflight) {
    stage(lbuf);
    lbuf = lbuf + 1 == NS ? 0 : lbuf + 1;
  }
  for (int ti = blockIdx.x; ti < ntiles; ti += gridDim.x) {
  const int item = xcd_remap(ti, ntiles), tile = item / KSP;
  const int64_t m0 = (int64_t)(tile / ntn) * BM;
  const int n0 = (tile % ntn) * BN_;
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < J; ++j) acc[i][j] = cf32x4{0.f, 0.f, 0.f, 0.f};
  int kt = 0;
  for (; ld < nk; ++kt) {     // steady state: refill with this tile's K-tiles
    // K-tile kt landed; the inflight-1 younger ones may stay in flight (the previous
    // tile's epilogue stores, issued after them, only make this wait conservative)
    wait_tile<PA + PB, NS>(inflight - 1);
    stage(lbuf);
    ++ld;
    lbuf = lbuf + 1 == NS ? 0 : lbuf + 1;
    compute(cur);
    cur = cur + 1 == NS ? 0 : cur + 1;
  }
  // this tile is fully issued: the remaining (<= NS-1) iterations refill with the next
  // tile's first K-tiles, so they are in flight during this tile's tail and epilogue
  const bool nxt = ts + (int)gridDim.x < ntiles;
  if (nxt) {
    ts += gridDim.x;
    setup(xcd_remap(ts, ntiles));
  }
  ld = 0;
  for (; kt < nk; ++kt) {
    wait_tile<PA + PB, NS>(inflight - 1);
    if (nxt) {
      stage(lbuf);
      ++ld;
      lbuf = lbuf + 1 == NS ? 0 : lbuf + 1;
    } else {
      --inflight;
    }
    compute(cur);
    cur = cur + 1 == NS ? 0 : cur + 1;
  }
  if (KSP > 1) {
    // split K: the fp32 partial tile, 16 B (4 columns of one row) per lane and row
    float *kp = a.kpart + (int64_t)(item % KSP) * a.M * a.Ncol;
#pragma unroll
    for (int j = 0; j < J; ++j) {
      const int col = n0 + wn * WN + j * 16 + fq * 4;
      if (col >= a.Ncol) continue;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int64_t row = m0 + wm * 64 + i * 16 + fr;
        if (row < a.M)
          *reinterpret_cast<float4 *>(kp + row * a.Ncol + col) =
              make_float4(acc[i][j][0], acc[i][j][1], acc[i][j][2], acc[i][j][3]);
      }
    }
    continue;
  }
  // epilogue: (+ bias) -> bf16, 8-B stores of 4 consecutive channels per lane
  // (Ncol % 8 == 0 and group widths % 32 == 0: a 4-channel run never straddles)
  const bool stats = !DGRAD && a.bn_part != nullptr;
  constexpr bool bstats = BST;
  int64_t opx[4];               // parity-class dgrad: the dx pixel of each of this lane's rows
  if (cls) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int64_t row = m0 + wm * 64 + i * 16 + fr;
      const int64_t rr = row < a.M ? row : 0;
      const int ow = (int)(rr % a.outW);
      const int64_t t = rr / a.outW;
      const int oh = (int)(t % a.outH);
      const int64_t n = t / a.outH;
      opx[i] = (n * a.dstH + 2 * oh + py) * a.dstW + 2 * ow + px;
    }
  }
  float cs[J][4], cq[J][4];     // this lane's column sums over its 4 rows (BN statistics)
  // BST: the stored bf16 values, kept for the statistics pass after the stores
  uint2 hpk[BST ? J : 1][4];
#pragma unroll
  for (int j = 0; j < J; ++j) {
    const int col = n0 + wn * WN + j * 16 + fq * 4;
#pragma unroll
    for (int r = 0; r < 4; ++r) { cs[j][r] = 0.f; cq[j][r] = 0.f; }
    if (col >= a.Ncol) continue;
    float4 bv = make_float4(0.f, 0.f, 0.f, 0.f);
    if (a.bias) bv = *reinterpret_cast<const float4 *>(a.bias + col);
    float4 kv = make_float4(0.f, 0.f, 0.f, 0.f);
    if (stats && a.bn_shift) kv = *reinterpret_cast<const float4 *>(a.bn_shift + col);
    const int gi = col / a.ogc;
    bf16_t *ob = a.out + (int64_t)gi * a.ogs + (col - gi * a.ogc);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int64_t row = m0 + wm * 64 + i * 16 + fr;
      if (row < a.M) {
        const int64_t opix = cls ? opx[i] : row;
        float4 av = bv;
        if (a.addend) {
          const uint2 q = *reinterpret_cast<const uint2 *>(a.addend + (ob - a.out) + opix * a.ogc);
          av.x += __uint_as_float(q.x << 16); av.y += __uint_as_float(q.x & 0xffff0000u);
          av.z += __uint_as_float(q.y << 16); av.w += __uint_as_float(q.y & 0xffff0000u);
        }
        const bf16_t h0 = f2bf(acc[i][j][0] + av.x), h1 = f2bf(acc[i][j][1] + av.y);
        const bf16_t h2 = f2bf(acc[i][j][2] + av.z), h3 = f2bf(acc[i][j][3] + av.w);
        uint2 pk;
        pk.x = (uint32_t)h0 | ((uint32_t)h1 << 16);
        pk.y = (uint32_t)h2 | ((uint32_t)h3 << 16);
        *reinterpret_cast<uint2 *>(ob + opix * a.ogc) = pk;
        if constexpr (BST) hpk[j][i] = pk;
        if (stats) {
          const float d0 = bf2f(h0) - kv.x, d1 = bf2f(h1) - kv.y, d2 = bf2f(h2) - kv.z, d3 = bf2f(h3) - kv.w;
          cs[j][0] += d0; cs[j][1] += d1; cs[j][2] += d2; cs[j][3] += d3;
          cq[j][0] = fmaf(d0, d0, cq[j][0]); cq[j][1] = fmaf(d1, d1, cq[j][1]);
          cq[j][2] = fmaf(d2, d2, cq[j][2]); cq[j][3] = fmaf(d3, d3, cq[j][3]);
        }
      }
    }
  }
  if constexpr (BST) {
    // g = dx * act'(xhat * gamma + beta) (act) or dx * rscale[frame]; sums of g and g * xhat
    // over the stored values, one column block at a time: its 4 BN-input loads and the BN
    // parameters are issued together, so their latencies overlap
    float brs[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int64_t row = m0 + wm * 64 + i * 16 + fr;
      brs[i] = a.bwd.rscale && row < a.M ? a.bwd.rscale[row / a.bwd.hw] : 1.f;
    }
#pragma unroll
    for (int j = 0; j < J; ++j) {
      const int col = n0 + wn * WN + j * 16 + fq * 4;
      if (col >= a.Ncol) continue;
      const int gi = col / a.ogc;
      const bf16_t *xg = a.bwd.x + (int64_t)gi * a.ogs + (col - gi * a.ogc);   // the BN input, dx's layout
      uint2 xq[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int64_t row = m0 + wm * 64 + i * 16 + fr;
        xq[i] = row < a.M ? *reinterpret_cast<const uint2 *>(xg + row * a.ogc) : make_uint2(0u, 0u);
      }
      // statistics: [row group][C] of a row-grouped BN, [channel group][C] = col of a grouped dx;
      // the affine parameters are shared by the groups
      const int64_t sidx = (a.bwd.grows ? m0 / a.bwd.grows * a.ogc : 0) + col;
      const int pidx = col - gi * a.ogc;
      const float4 mu4 = *reinterpret_cast<const float4 *>(a.bwd.mean + sidx);
      const float4 iv4 = *reinterpret_cast<const float4 *>(a.bwd.invstd + sidx);
      const float4 ga4 = a.bwd.gamma ? *reinterpret_cast<const float4 *>(a.bwd.gamma + pidx) : make_float4(1.f, 1.f, 1.f, 1.f);
      const float4 be4 = a.bwd.beta ? *reinterpret_cast<const float4 *>(a.bwd.beta + pidx) : make_float4(0.f, 0.f, 0.f, 0.f);
      const float mu[4] = {mu4.x, mu4.y, mu4.z, mu4.w}, iv[4] = {iv4.x, iv4.y, iv4.z, iv4.w};
      const float ga[4] = {ga4.x, ga4.y, ga4.z, ga4.w}, be[4] = {be4.x, be4.y, be4.z, be4.w};
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int64_t row = m0 + wm * 64 + i * 16 + fr;
        if (row >= a.M) continue;
        const float xv[4] = {__uint_as_float(xq[i].x << 16), __uint_as_float(xq[i].x & 0xffff0000u),
                             __uint_as_float(xq[i].y << 16), __uint_as_float(xq[i].y & 0xffff0000u)};
        const float hv[4] = {__uint_as_float(hpk[j][i].x << 16), __uint_as_float(hpk[j][i].x & 0xffff0000u),
                             __uint_as_float(hpk[j][i].y << 16), __uint_as_float(hpk[j][i].y & 0xffff0000u)};
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float xh = (xv[r] - mu[r]) * iv[r];
          const float g = a.bwd.act ? hv[r] * bn_act_grad(a.bwd.act, fmaf(xh, ga[r], be[r])) : hv[r] * brs[i];
          cs[j][r] += g;
          cq[j][r] = fmaf(g, xh, cq[j][r]);
        }
      }
    }
  }
  if (stats || bstats) {
  // BatchNorm partial statistics of this m-tile: the 16 row lanes of each column
  // (DPP row sums), then the BM/64 waves that share a column block through LDS, in order
#pragma unroll
  for (int j = 0; j < J; ++j)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      cs[j][r] = row_sum16(cs[j][r]);
      cq[j][r] = row_sum16(cq[j][r]);
    }
  // [BM/64][BN_][2] after the ring (the next tile's K-tiles are landing in it); its
  // previous tile's readers finished before this tile's K-loop barriers
  // (dgrad: no image after the ring — its partials go into ring slot 0 once every wave has
  // finished reading it; an uncapped grid, so no next tile's K-tiles are landing there)
  float *red = reinterpret_cast<float *>(smem + NS * STG);
  if (fr == 0)
#pragma unroll
    for (int j = 0; j < J; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int cl = wn * WN + j * 16 + fq * 4 + r;
        red[(wm * BN_ + cl) * 2] = cs[j][r];
        red[(wm * BN_ + cl) * 2 + 1] = cq[j][r];
      }
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");   // no vmcnt drain
  if (tid < BN_) {
    const int col = n0 + tid;
    if (col < a.Ncol) {
      float S = 0.f, Q = 0.f;
#pragma unroll
      for (int q = 0; q < BM / 64; ++q) { S += red[(q * BN_ + tid) * 2]; Q += red[(q * BN_ + tid) * 2 + 1]; }
      const int64_t t = m0 / BM;
      if (DGRAD) {
        // channel group gi of a grouped dx is its own BatchNorm group: rows [gi][m-tile][2 ogc]
        const int gi = col / a.ogc, cl = col - gi * a.ogc;
        float *pr = a.bwd.part + ((int64_t)gi * ((a.M + BM - 1) / BM) + t) * 2 * a.ogc;
        pr[cl] = S;
        pr[a.ogc + cl] = Q;
      } else {
        a.bn_part[t * 2 * a.Ncol + col] = S;
        a.bn_part[t * 2 * a.Ncol + a.Ncol + col] = Q;
      }
      if (!DGRAD && t == 0 && a.bn_shift_out) a.bn_shift_out[col] = a.bn_shift ? a.bn_shift[col] : 0.f;
    }
  }
  }
  }
}

// ---- split-K epilogue (conv_glds_kernel with FwdArgs::ksplit > 1; 1x1, plain layouts): block
// = one bm-row m-tile (the tile the BatchNorm partial rows follow) x 64 columns; thread = 4
// columns x rows r, r + 16, .. of the tile.  It adds the splits' fp32 partials in split order,
// then runs conv_glds_kernel's epilogue once: (+ bias, + addend) -> bf16, and MODE 1 the
// forward statistics sum (y - K), sum (y - K)^2 / MODE 2 the backward statistics (BST: sum g,
// sum g * xhat) of the tile, its 16 row lanes added in order through LDS.
template <int MODE>
__global__ __launch_bounds__(256) void conv_splitk_epi_kernel(FwdArgs a, int bm) {
  __shared__ float red[16][64][2];
  const int tid = threadIdx.x, cq = tid & 15, rl = tid >> 4;
  const int64_t m0 = (int64_t)blockIdx.x * bm;
  const int col = blockIdx.y * 64 + cq * 4;
  const bool cok = col < a.Ncol;
  const int64_t plane = a.M * a.Ncol;
  const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
  const float4 bv = (cok && a.bias) ? *reinterpret_cast<const float4 *>(a.bias + col) : zero;
  const float4 kv = (MODE == 1 && cok && a.bn_shift) ? *reinterpret_cast<const float4 *>(a.bn_shift + col) : zero;
  float mu[4] = {0.f, 0.f, 0.f, 0.f}, iv[4] = {0.f, 0.f, 0.f, 0.f};
  float ga[4] = {1.f, 1.f, 1.f, 1.f}, be[4] = {0.f, 0.f, 0.f, 0.f};
  if (MODE == 2 && cok) {
    const int64_t sidx = (a.bwd.grows ? m0 / a.bwd.grows * a.ogc : 0) + col;
    const float4 mu4 = *reinterpret_cast<const float4 *>(a.bwd.mean + sidx);
    const float4 iv4 = *reinterpret_cast<const float4 *>(a.bwd.invstd + sidx);
    mu[0] = mu4.x; mu[1] = mu4.y; mu[2] = mu4.z; mu[3] = mu4.w;
    iv[0] = iv4.x; iv[1] = iv4.y; iv[2] = iv4.z; iv[3] = iv4.w;
    if (a.bwd.gamma) {
      const float4 g4 = *reinterpret_cast<const float4 *>(a.bwd.gamma + col);
      ga[0] = g4.x; ga[1] = g4.y; ga[2] = g4.z; ga[3] = g4.w;
    }
    if (a.bwd.beta) {
      const float4 b4 = *reinterpret_cast<const float4 *>(a.bwd.beta + col);
      be[0] = b4.x; be[1] = b4.y; be[2] = b4.z; be[3] = b4.w;
    }
  }
  float cs[4] = {0.f, 0.f, 0.f, 0.f}, cqq[4] = {0.f, 0.f, 0.f, 0.f};
  if (cok) {
    for (int r = rl; r < bm; r += 16) {
      const int64_t row = m0 + r;
      if (row >= a.M) break;
      const float *kp = a.kpart + row * a.Ncol + col;
      float4 t = *reinterpret_cast<const float4 *>(kp);
      for (int sp = 1; sp < a.ksplit; ++sp) {
        const float4 u = *reinterpret_cast<const float4 *>(kp + sp * plane);
        t.x += u.x; t.y += u.y; t.z += u.z; t.w += u.w;
      }
      float4 av = bv;
      if (a.addend) {
        const uint2 q = *reinterpret_cast<const uint2 *>(a.addend + row * a.ogc + col);
        av.x += __uint_as_float(q.x << 16); av.y += __uint_as_float(q.x & 0xffff0000u);
        av.z += __uint_as_float(q.y << 16); av.w += __uint_as_float(q.y & 0xffff0000u);
      }
      const bf16_t h0 = f2bf(t.x + av.x), h1 = f2bf(t.y + av.y), h2 = f2bf(t.z + av.z), h3 = f2bf(t.w + av.w);
      uint2 pk;
      pk.x = (uint32_t)h0 | ((uint32_t)h1 << 16);
      pk.y = (uint32_t)h2 | ((uint32_t)h3 << 16);
      *reinterpret_cast<uint2 *>(a.out + row * a.ogc + col) = pk;
      const float hv[4] = {bf2f(h0), bf2f(h1), bf2f(h2), bf2f(h3)};
      if (MODE == 1) {
        const float kk[4] = {kv.x, kv.y, kv.z, kv.w};
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const float d = hv[q] - kk[q];
          cs[q] += d;
          cqq[q] = fmaf(d, d, cqq[q]);
        }
      } else if (MODE == 2) {
        const uint2 xq = *reinterpret_cast<const uint2 *>(a.bwd.x + row * a.ogc + col);
        const float xv[4] = {__uint_as_float(xq.x << 16), __uint_as_float(xq.x & 0xffff0000u),
                             __uint_as_float(xq.y << 16), __uint_as_float(xq.y & 0xffff0000u)};
        const float brs = a.bwd.rscale ? a.bwd.rscale[row / a.bwd.hw] : 1.f;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const float xh = (xv[q] - mu[q]) * iv[q];
          const float g = a.bwd.act ? hv[q] * bn_act_grad(a.bwd.act, fmaf(xh, ga[q], be[q])) : hv[q] * brs;
          cs[q] += g;
          cqq[q] = fmaf(g, xh, cqq[q]);
        }
      }
    }
  }
  if (MODE == 0) return;
#pragma unroll
  for (int q = 0; q < 4; ++q) { red[rl][cq * 4 + q][0] = cs[q]; red[rl][cq * 4 + q][1] = cqq[q]; }
  __syncthreads();
  if (tid < 64) {
    const int c = blockIdx.y * 64 + tid;
    if (c < a.Ncol) {
      float S = 0.f, Q = 0.f;
      for (int q = 0; q < 16; ++q) { S += red[q][tid][0]; Q += red[q][tid][1]; }
      const int64_t t = blockIdx.x;
      if (MODE == 2) {
        float *pr = a.bwd.part + t * 2 * a.ogc;
        pr[c] = S;
        pr[a.ogc + c] = Q;
      } else {
        a.bn_part[t * 2 * a.Ncol + c] = S;
        a.bn_part[t * 2 * a.Ncol + a.Ncol + c] = Q;
        if (t == 0 && a.bn_shift_out) a.bn_shift_out[c] = a.bn_shift ? a.bn_shift[c] : 0.f;
      }
    }
  }
}

int g_glds = 1;   // (conv_common.h)
extern "C" int ewvit_conv2d_set_glds(int variant) {
  const int prev = g_glds;
  g_glds = variant ? 1 : 0;
  return prev;
}

// one launch of conv_glds_kernel (a, grid, ntn, ntiles, src_bytes, s of the caller): the kernel-size switch
#define EWVIT_GLDS_K(DG_, BM_, BN__, NS_, WC_, DENSE_, BST_, TI_)                                                   \
  do {                                                                                                            \
    if (a.g.ks == 1)                                                                                              \
      hipLaunchKernelGGL((conv_glds_kernel<DG_, BM_, BN__, 1, NS_, WC_, DENSE_, BST_>), grid,                      \
                         dim3(BM_ / 64 * WC_ * 64), 0, s, a, src_bytes, ntn, TI_, ntiles);                        \
    else                                                                                                          \
      hipLaunchKernelGGL((conv_glds_kernel<DG_, BM_, BN__, 3, NS_, WC_, DENSE_, BST_>), grid,                      \
                         dim3(BM_ / 64 * WC_ * 64), 0, s, a, src_bytes, ntn, TI_, ntiles);                        \
  } while (0)

// the dense-K forward (conv_glds_kernel<false, ..., DENSE>): 128-row tiles, 8 waves with a
// 2-deep ring for grids of <= 2048 blocks, 4 waves beyond, the 4-deep ring for <= 256
static void launch_glds_dense(const FwdArgs &a, int64_t src_bytes, hipStream_t s) {
  const int bn = 128;
  const int ntn = (a.Ncol + bn - 1) / bn;
  const int64_t nwg = (a.M + 127) / 128 * ntn;
  const int ntiles = (int)nwg;
  const dim3 grid((unsigned)(g_grid_cap > 0 && nwg > g_grid_cap ? g_grid_cap : nwg));
  // (Ncol > 64: 128-wide column tiles)
  // grids up to 4096 blocks take 8 waves (stage 2's 48 -> 192 expands, 3136 blocks: 81 -> 75
  // us); a 3-deep ring for the big grids measured 30-60 % slower
  if (nwg <= 256) EWVIT_GLDS_K(false, 128, 128, 4, 4, true, false, 0);
  else if (nwg <= 4096) EWVIT_GLDS_K(false, 128, 128, 2, 4, true, false, 0);
  else EWVIT_GLDS_K(false, 128, 128, 2, 2, true, false, 0);
}

// Tile of the LDS-DMA fwd / dgrad: 128 rows (256 for a <= 64-column dgrad over > 4096 row tiles:
// the MWT fusion conv's input gradient); grids of < 128 such tiles — the backbone's long-K
// 1x1 convs at 7^2 (stage 6 project forward / expand input gradient: 3136 x 256 x 1536, 50
// tiles, 24 K-tiles each) — take 64-row tiles, and 64-column tiles if still < 128 (4x the
// workgroups).  Any BatchNorm partial rows the kernel leaves follow its row tile.
static int g_small_tiles = 1;
extern "C" int ewvit_conv2d_set_small_tiles(int on) {
  const int prev = g_small_tiles;
  g_small_tiles = on ? 1 : 0;
  return prev;
}
void glds_tile(const FwdArgs &a, bool dgrad, int &bm, int &bn) {
  bn = a.Ncol <= 32 ? 32 : a.Ncol <= 64 ? 64 : 128;
  const int64_t ntn = (a.Ncol + bn - 1) / bn, mt = (a.M + 127) / 128;
  bm = 128;
  if (dgrad && bn == 64 && mt * ntn > 4096 && !a.bwd.part) { bm = 256; return; }
  if (g_small_tiles && bn >= 64 && mt * ntn < 128) {
    bm = 64;
    if (bn == 128 && (a.M + 63) / 64 * ntn < 128) bn = 64;
  }
}

// split K for the LDS-DMA 1x1 fwd / dgrad (FwdArgs::ksplit): the backbone's long-K 1x1 convs
// over few tiles — stage 6's project forward / expand input gradient (3136 x 256 x 1536: 196
// workgroups of 24 K-tiles), the head conv (K = 1280) — run their K loop serially per workgroup
// on < 256 workgroups.  Split into S ranges (S | K-tiles, >= g_ksplit_min_kt K-tiles each, <= 1024
// work items), fp32 partials in a per-stream scratch buffer, conv_splitk_epi_kernel for the
// epilogue.  OFF by default: measured slower in the step at every setting — S <= 2 / >= 8 K-tiles
// 3725-3729, S <= 2 / >= 4 3710, S <= 4 / >= 8 3708-3713, S <= 8 / >= 4 3665-3679 against
// 3755-3766 frames/s unsplit (same box, profiles/r06/ab/ksplit.log): beside the MWT the step is
// bound by CU-time and memory traffic, which the partials and the epilogue pass add to, not by
// these kernels' latency.  ewvit_conv2d_set_ksplit(1) / EWVIT_CONV_KSPLIT=1: on (tests, A/B).
static int g_ksplit = 0, g_ksplit_max = 2, g_ksplit_min_kt = 8;
extern "C" int ewvit_conv2d_set_ksplit(int on) {
  const int prev = g_ksplit;
  g_ksplit = on ? 1 : 0;
  if (on > 1) { g_ksplit_max = on & 15; g_ksplit_min_kt = on >> 4; }   // tuning: max S | min K-tiles << 4
  return prev;
}
// the split partials' scratch, one buffer per (device, stream) (the branches run convs
// concurrently), grown outside stream capture only (nullptr -> the caller runs unsplit); a
// replaced buffer is kept, since kernels queued on the stream may still read it
static float *ksplit_scratch(hipStream_t s, size_t bytes) {
  static std::mutex mu;
  static std::map<StreamKey, std::pair<void *, size_t>> bufs;
  std::lock_guard<std::mutex> lk(mu);
  auto &e = bufs[stream_key(s)];
  if (e.second >= bytes) return static_cast<float *>(e.first);
  hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(s, &st) != hipSuccess || st != hipStreamCaptureStatusNone) return nullptr;
  void *p = nullptr;
  if (hipMalloc(&p, bytes) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
  e = {p, bytes};
  return static_cast<float *>(p);
}

template <bool DGRAD>
static bool launch_glds_t(FwdArgs a, int64_t src_bytes, hipStream_t s, int *bm_out) {
  const int64_t K = (int64_t)a.g.ks * a.g.ks * a.KC;
  const bool padded = a.KCr && a.KCr != a.KC;     // plain x, channels padded to 64 per tap
  // ragged: plain (ungrouped) x whose per-tap K is not a multiple of 64 — the last
  // 64-channel block of each tap zero-fills its A lanes >= KC and reads finite weights
  // of the next tap / row (or zeros past the end) for B, which meet only zeros
  // (only while the zero lanes stay <= 20 % of K: K = 48 per tap measured slower than
  // the register-staged kernel, K = 160 -> 3 blocks 17 % faster)
  const bool ragged = !padded && a.KC % 64 != 0;
  // (only with 128-wide column tiles: for Cout <= 64 — stage 1's 24 -> 24 at 112^2, the MWT
  // seperate conv's 16 -> 64, the 96 -> 48 projects — the register-staged kernel measured
  // as fast or faster: 62 vs 64, 166 vs 199, 15 vs 16 us; Cout 96 / 192: 39 -> 32, 106 -> 81,
  // 34 -> 27 us, tools/conv_bench.py)
  if (!DGRAD && ragged && use_glds() && a.Ncol > 64 && a.sgs == 0 && a.sgc == a.KC && a.KC % 8 == 0 &&
      src_bytes < (int64_t)OOB && a.Ncol * K * 2 < (int64_t)OOB && a.M * a.ogc < ((int64_t)1 << 40) &&
      (a.g.ks == 1 || a.g.ks == 3)) {
    launch_glds_dense(a, src_bytes, s);
    return true;
  }
  // a parity-class dgrad, which already skips 3/4 of the taps, takes up to 1/3 zero lanes
  const int kpad = (a.KC + 63) / 64 * 64;
  const bool ragged_ok = a.pc >= 0 ? 2 * kpad <= 3 * a.KC : 5 * kpad <= 6 * a.KC;
  if (ragged && (a.sgs != 0 || a.sgc != a.KC || a.KC % 8 || !ragged_ok))
    return false;
  if (!use_glds() || (!ragged && a.KC % 64) || (padded ? a.sgc != a.KCr : (!ragged && a.sgc % 64)) ||
      src_bytes >= (int64_t)OOB ||
      a.Ncol * K * 2 >= (int64_t)OOB ||
      a.M * a.ogc >= (int64_t)1 << 40)
    return false;
  const int tap_inner = 1;           // the 9 taps of a 64-channel block are consecutive K-tiles
  // <= 32 columns (stage 2's entry-conv input gradient, 24 channels): 32-wide column tiles.
  // A <= 64-column dgrad over > 4096 row tiles (the MWT fusion conv's 56-channel input
  // gradient, 2.4 M pixels): 256-row blocks, 535 -> 505 us.  Stage 2's 48-channel 3x3 dgrad
  // (1568 row tiles) runs faster on 8-wave 128-row blocks (96 -> 75 us, tools/dgrad_ab.sh)
  int BM, bn;
  glds_tile(a, DGRAD, BM, bn);
  const int ntn = (a.Ncol + bn - 1) / bn;
  const bool big = BM == 256;
  if (bm_out) *bm_out = BM;
  const int64_t mt = (a.M + BM - 1) / BM;
  int64_t nwg = mt * ntn;
  if (nwg >= (int64_t)1 << 31) return false;
  int S = 1;
  if (g_ksplit && a.g.ks == 1 && a.pc < 0 && !padded && !ragged && a.sgs == 0 && a.sgc == a.KC && a.ogs == 0 &&
      a.ogc == a.Ncol && !big && nwg < 256) {
    const int nkt = a.KC / 64;
    for (int c = g_ksplit_max; c >= 2; --c)
      if (nkt % c == 0 && nkt / c >= g_ksplit_min_kt && nwg * c <= 1024) { S = c; break; }
    if (S > 1) {
      float *ws = ksplit_scratch(s, (size_t)S * a.M * a.Ncol * sizeof(float));
      if (ws) { a.ksplit = S; a.kpart = ws; nwg *= S; }
      else S = 1;
    }
  }
  const int ntiles = (int)nwg;
  const dim3 grid((unsigned)(g_grid_cap > 0 && nwg > g_grid_cap ? g_grid_cap : nwg));
  // (the statistics epilogue is a separate instantiation of each tile but the 256-row one)
#define EWVIT_GLDS_FWDW(BM_, BN__, NS_, WC_)                                                                        \
  do {                                                                                                            \
    if (bst) EWVIT_GLDS_K(DGRAD, BM_, BN__, NS_, WC_, false, DGRAD, tap_inner);                                    \
    else EWVIT_GLDS_K(DGRAD, BM_, BN__, NS_, WC_, false, false, tap_inner);                                        \
  } while (0)
  // Blocks: grids of <= 2048 workgroups (the backbone's 7^2 - 28^2 convs) and every dgrad with
  // 128-wide column tiles (freq_conv's parity-class dgrad 185 -> 162 us, multiscale 834 -> 820)
  // take 8 waves (64 x BN/4 each) — twice the waves per CU to hide the latency of short K
  // loops; big grids keep 4 waves (64 x BN/2 each: fewer LDS reads per MFMA).  Grids of <= 256
  // workgroups (the backbone's long-K 1x1 convs at 7^2 / 14^2: at most one block per CU, so
  // occupancy hides nothing) take 8 waves with a 4-deep ring (3 K-tiles in flight).
  const bool w8 = nwg <= 2048 || (DGRAD && bn == 128);
  const bool sg = nwg <= 256;
  // the backward-statistics epilogue: 64- / 128-row tiles (glds_tile: the partial rows
  // ewvit_conv2d_bwd_bn_rows promised); split K: the epilogue kernel sums them
  const bool bst = DGRAD && a.bwd.part && S == 1;
  if (big) EWVIT_GLDS_K(DGRAD, 256, 64, 2, 2, false, false, tap_inner);
  else if (BM == 64) {
    if (bn == 64) EWVIT_GLDS_FWDW(64, 64, 4, 4);
    else EWVIT_GLDS_FWDW(64, 128, 4, 4);
  } else if (bn == 32) EWVIT_GLDS_FWDW(128, 32, 2, 2);
  else if (bn == 64) {
    if (sg) EWVIT_GLDS_FWDW(128, 64, 4, 4);
    else if (w8) EWVIT_GLDS_FWDW(128, 64, 2, 4);
    else EWVIT_GLDS_FWDW(128, 64, 2, 2);
  } else {
    if (sg) EWVIT_GLDS_FWDW(128, 128, 4, 4);
    else if (w8) EWVIT_GLDS_FWDW(128, 128, 2, 4);
    else EWVIT_GLDS_FWDW(128, 128, 2, 2);
  }
#undef EWVIT_GLDS_FWDW
  if (S > 1) {
    const dim3 eg((unsigned)mt, (unsigned)((a.Ncol + 63) / 64));
    if (DGRAD && a.bwd.part) hipLaunchKernelGGL(conv_splitk_epi_kernel<2>, eg, dim3(256), 0, s, a, BM);
    else if (!DGRAD && a.bn_part) hipLaunchKernelGGL(conv_splitk_epi_kernel<1>, eg, dim3(256), 0, s, a, BM);
    else hipLaunchKernelGGL(conv_splitk_epi_kernel<0>, eg, dim3(256), 0, s, a, BM);
  }
  return true;
}
bool launch_glds(const FwdArgs &a, int64_t src_bytes, bool dgrad, hipStream_t s, int *bm_out) {
  return dgrad ? launch_glds_t<true>(a, src_bytes, s, bm_out) : launch_glds_t<false>(a, src_bytes, s, bm_out);
}

// stride-2 3x3 dgrad as 4 launches, one per output parity class (py, px), each over
// only its live taps (1, 2, 2 and 4 of the 9); false when the LDS-DMA kernel cannot
// take the class launches (nothing launched)
bool dgrad_by_parity(FwdArgs a, int64_t src_bytes, hipStream_t s) {
  if (a.g.ks != 3 || a.g.stride != 2 || a.g.pad != 1 || a.ogs != 0 || a.sgs != 0 || !use_glds())
    return false;
  const int H = a.outH, W = a.outW;
  FwdArgs c[4];
  for (int pc = 0; pc < 4; ++pc) {
    const int py = pc >> 1, px = pc & 1;
    c[pc] = a;
    c[pc].pc = pc;
    c[pc].dstH = H; c[pc].dstW = W;
    c[pc].outH = (H - py + 1) / 2; c[pc].outW = (W - px + 1) / 2;
    c[pc].M = (int64_t)a.g.N * c[pc].outH * c[pc].outW;
    int nt = 0;
    for (int kh = 0; kh < 3; ++kh)
      for (int kw = 0; kw < 3; ++kw)
        if (((py + 1 - kh) & 1) == 0 && ((px + 1 - kw) & 1) == 0) c[pc].tapl[nt++] = kh * 3 + kw;
    c[pc].ntap = nt;
  }
  // the KC / layout checks of launch_glds do not depend on the class: probe class 3's
  // shape first so a refusal launches nothing
  int order[4] = {3, 0, 1, 2};
  for (int q = 0; q < 4; ++q) {
    const int pc = order[q];
    if (c[pc].M == 0) continue;
    if (!launch_glds(c[pc], src_bytes, true, s)) {
      if (q == 0) return false;
      set_error("conv2d_bwd_data: parity class %d refused after class 3 ran", pc);
      return false;
    }
  }
  return true;
}

}  // namespace ewvit
