// Shared declarations of the conv kernels.  One translation unit per kernel family, each owning
// its kernels and their launchers and exposing plain host functions here:
//   conv_reg.hip    register-staged fwd / dgrad, the small-channel 3x3
//   conv_glds.hip   LDS-DMA fwd / dgrad, its split-K epilogue and scratch
//   conv_wgrad.hip  the weight gradients, their reduce and entry points
//   convwin.hip     the windowed 3x3 stride-1 kernels of the MWT's big maps
//   conv.hip        weight packs, argument validation, the fwd / dgrad entry points
#pragma once
#include "common.h"

namespace ewvit {

typedef __attribute__((ext_vector_type(8))) __bf16 cbf16x8;
typedef __attribute__((ext_vector_type(4))) float cf32x4;
typedef __attribute__((ext_vector_type(4))) short cs4;

constexpr int CBM = 128, CBN = 128, CBK = 32;

struct ConvGeom {
  int N, H, W, Cin;      // x (fwd) / dx (dgrad) grid
  int Ho, Wo, Cout;      // y / dy grid
  int stride, ks, pad;   // ks 1|3, pad = ks/2
};

// ---------------------------------------------------------------- fwd / dgrad
// A(m, k): m = pixel of the OUTPUT grid of this GEMM (y for fwd, dx for dgrad),
// k = tap * KC + c (KC = Cin for fwd, Cout for dgrad).  B(k, n) = Wp[n][k].
struct FwdArgs {
  const bf16_t *src = nullptr;   // gathered operand: x (fwd) or dy (dgrad), grouped NHWC
  const bf16_t *wp = nullptr;    // packed weights [Ncol][taps][KC]
  const float *bias = nullptr;   // [Ncol] or null
  bf16_t *out = nullptr;         // [M][Ncol], grouped NHWC
  ConvGeom g;
  int64_t M;
  int Ncol, KC;          // GEMM N and per-tap K
  int srcH, srcW;        // spatial size of `src`
  int outH, outW;        // spatial size of the GEMM's output grid
  int sgc, ogc;          // channel group widths of src / out
  int64_t sgs, ogs;      // group strides (elements)
  // optional BatchNorm statistics of the (bf16-rounded) output, LDS-DMA fwd only:
  // per m-tile t and column c, bn_part[t][c] = sum (y - K[c]), bn_part[t][Ncol + c] =
  // sum (y - K[c])^2 with K = bn_shift (or 0); tile 0 copies K to bn_shift_out
  const float *bn_shift = nullptr;
  float *bn_part = nullptr;
  float *bn_shift_out = nullptr;
  // LDS-DMA fwd over a plain NHWC x whose channel count is not a multiple of 64: KC is
  // the per-tap K padded up to 64 (the weights packed with that many input channels)
  // and the staging lanes of channels >= KCr (the real count) read zeros
  int KCr = 0;
  int nt = 0;            // windowed fwd / dgrad: non-temporal hint on the window DMAs
  // optional addend of the output (same layout as out, bf16), added before rounding —
  // the skip connection's gradient folded into the block input's dgrad
  const bf16_t *addend = nullptr;
  // stride-2 3x3 dgrad by output parity class (LDS-DMA kernel): the GEMM rows are the
  // dx pixels (2i + py, 2j + px) of class pc = 2*py + px on an outH x outW grid, and
  // only the class's ntap live taps tapl[] run (dy pixel (i + dh, j + dw)); the
  // epilogue scatters row (n, i, j) to dx pixel (n, 2i + py, 2j + px) of dstH x dstW
  int pc = -1, ntap = 0;
  int tapl[4] = {0, 0, 0, 0};
  int dstH = 0, dstW = 0;
  // optional (LDS-DMA dgrad, plain NHWC dx, uncapped grid): the backward statistics of the
  // BatchNorm(+act) whose output this conv read, summed over the bf16-rounded dx per m-tile
  // (common.h BnBwdStats; bwd.part [m-tiles][2 Ncol])
  BnBwdStats bwd;
  // optional input transform of the windowed fwd (convwin.hip, XF): the conv reads
  // relu(x * xf[g][0][c] + xf[g][1][c]) — a training BatchNorm + ReLU applied by its producer's
  // coefficients (ewvit_bn_coef) — instead of x; channel group g = c / sgc, zero padding after
  // the transform
  const float *xf = nullptr;
  // split K (LDS-DMA 1x1 fwd / dgrad over few tiles, conv_glds.hip launch_glds): work item i is
  // (tile i / ksplit, K-range i % ksplit of nk / ksplit K-tiles), which stores its fp32 partial
  // tile at kpart[split][M][Ncol]; conv_splitk_epi_kernel sums the splits and runs the epilogue
  int ksplit = 1;
  float *kpart = nullptr;
};

typedef __attribute__((address_space(3))) void lds_t;
constexpr uint32_t OOB = 0x80000000u;   // any offset >= num_records reads as zero

__device__ __forceinline__ __amdgpu_buffer_rsrc_t mk_rsrc(const void *p, int64_t bytes) {
  const uint32_t n = bytes >= (int64_t)OOB ? OOB : (uint32_t)bytes;
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(p), (short)0, (int)n, 0x00020000);
}
__device__ __forceinline__ void glds16(__amdgpu_buffer_rsrc_t r, unsigned char *lds, uint32_t voff) {
  __builtin_amdgcn_raw_ptr_buffer_load_lds(r, (lds_t *)lds, 16, voff, 0, 0, 0);
}
// bijective XCD remap: blocks b, b+8, b+16 ... (one XCD) get consecutive tile ids
__device__ __forceinline__ int xcd_remap(int bid, int nwg) {
  const int xcd = bid & 7, q = nwg >> 3, r = nwg & 7;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (bid >> 3);
}

// wait until at most the N youngest vector-memory ops (LDS-DMA pieces) are pending,
// then the workgroup barrier; one asm statement, so hipcc neither drains the DMA
// queue at the barrier nor moves LDS reads across it
template <int N> __device__ __forceinline__ void wait_vm_barrier() {
  asm volatile("s_waitcnt vmcnt(%0)\n\ts_barrier" ::"n"(N) : "memory");
}
// tile kt's pieces landed (L per tile per thread); `rem` younger tiles already issued
// (at most NS-2 of them) may stay in flight across the barrier
template <int L, int NS> __device__ __forceinline__ void wait_tile(int rem) {
  if constexpr (NS >= 4) { if (rem >= 2) { wait_vm_barrier<2 * L>(); return; } }
  if constexpr (NS >= 3) { if (rem >= 1) { wait_vm_barrier<L>(); return; } }
  wait_vm_barrier<0>();
}

// LDS-DMA issued from inline asm: hipcc cannot see these, so it neither waits on them before
// LDS reads (it drains the whole vmcnt queue ahead of any LDS access that may alias a builtin
// DMA) nor counts them; every kernel using them waits with explicit vmcnt counts (wait_tile,
// win_sync).  M0 (the DMA's LDS base) is reserved to hipcc, which sets it before each of its
// own uses; no other M0 user runs in these kernels.
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Winline-asm"
// a buffer resource as four dwords (gfx9 layout: base, base_hi | stride << 16, num_records,
// flags), so the asm operand can be pinned to SGPRs with readfirstlane (hipcc's divergence
// analysis sometimes leaves uniform values in VGPRs, which an "s" operand then rejects)
typedef __attribute__((ext_vector_type(4))) int ci32x4;
__device__ __forceinline__ ci32x4 mk_rsrc4(const void *p, int64_t bytes) {
  const uint32_t n = bytes >= (int64_t)OOB ? OOB : (uint32_t)bytes;
  const uint64_t a = (uint64_t)(uintptr_t)p;
  return ci32x4{(int)(uint32_t)a, (int)((uint32_t)(a >> 32) & 0xffff), (int)n, 0x00020000};
}
__device__ __forceinline__ void glds16_asm(__amdgpu_buffer_rsrc_t r, uint32_t lds, uint32_t voff) {
  asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, 0 offen lds" ::"s"(lds), "v"(voff), "s"(r)
               : "memory", "m0");
}
__device__ __forceinline__ void glds16_asm(ci32x4 r, uint32_t lds, uint32_t voff) {
  const ci32x4 rr = {__builtin_amdgcn_readfirstlane(r[0]), __builtin_amdgcn_readfirstlane(r[1]),
                     __builtin_amdgcn_readfirstlane(r[2]), __builtin_amdgcn_readfirstlane(r[3])};
  const uint32_t l = __builtin_amdgcn_readfirstlane(lds);
  asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, 0 offen lds" ::"s"(l), "v"(voff), "s"(rr)
               : "memory", "m0");
}
// ... with the non-temporal hint when `nt` (a uniform kernel argument: a scalar branch): the
// windowed MWT convs' activation windows (A/B, ewvit_conv2d_set_win_nt) — streamed once per
// tile, so they need not keep their L2 lines against the concurrent backbone's working set
__device__ __forceinline__ void glds16_asm(__amdgpu_buffer_rsrc_t r, uint32_t lds, uint32_t voff, bool nt) {
  if (nt)
    asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, 0 offen nt lds" ::"s"(lds), "v"(voff),
                 "s"(r) : "memory", "m0");
  else
    glds16_asm(r, lds, voff);
}
__device__ __forceinline__ void glds16_asm(ci32x4 r, uint32_t lds, uint32_t voff, bool nt) {
  if (nt) {
    const ci32x4 rr = {__builtin_amdgcn_readfirstlane(r[0]), __builtin_amdgcn_readfirstlane(r[1]),
                       __builtin_amdgcn_readfirstlane(r[2]), __builtin_amdgcn_readfirstlane(r[3])};
    const uint32_t l = __builtin_amdgcn_readfirstlane(lds);
    asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, 0 offen nt lds" ::"s"(l), "v"(voff),
                 "s"(rr) : "memory", "m0");
  } else {
    glds16_asm(r, lds, voff);
  }
}
#pragma clang diagnostic pop

// ---------------------------------------------------------------- wgrad
// A(co, m) = dy[m][co]   -> image Ast[m][co]  (rows of 128 co = 256 B)
// B(m, n') = x[pix(m,tap)][ci] -> image Bst[m][n'] (rows of 128 n' = 256 B)
// 16-B chunk ch of row r lives at 256*r + 16*(ch ^ swz(r)),
// swz(r) = ((r&3)<<2) | ((r>>2)&3)  (T10 image (b): conflict-free tr reads).
struct WgradArgs {
  const bf16_t *x;       // [N, H, W, Cin], grouped (xgc, xgs)
  const bf16_t *dy;      // [N, Ho, Wo, Cout]
  float *part;           // [splits][Cout][taps*Cin]
  float *dbias_part;     // [splits][Cout] partial bias gradients (sum of dy), or null
  ConvGeom g;
  int64_t M;             // N*Ho*Wo
  int64_t mper;          // pixels per split (multiple of 32)
  int xgc;
  int64_t xgs;
  const float *xf = nullptr;  // input transform of the windowed wgrad (FwdArgs::xf; groups of xgc)
  int nt = 0;                 // windowed wgrad: non-temporal hint, 1 the dy tile DMAs, 2 the x windows'
};

__device__ __forceinline__ int swz_off(int r, int ch) {
  return 256 * r + 16 * (ch ^ (((r & 3) << 2) | ((r >> 2) & 3)));
}

// ---------------------------------------------------------------- host
inline ConvGeom mkg(int64_t N, int64_t H, int64_t W, int64_t Cin, int64_t Cout, int ks, int stride) {
  ConvGeom g;
  g.N = (int)N; g.H = (int)H; g.W = (int)W; g.Cin = (int)Cin; g.Cout = (int)Cout; g.stride = stride;
  g.ks = ks; g.pad = ks / 2;
  g.Ho = (int)((H - 1) / stride + 1);
  g.Wo = (int)((W - 1) / stride + 1);
  return g;
}
// bytes a grouped channels-last bf16 tensor spans (gs == 0: plain NHWC)
inline int64_t grouped_bytes(int64_t pixels, int64_t C, int64_t gc, int64_t gs) {
  return 2 * (gs ? (C / gc - 1) * gs + pixels * gc : pixels * C);
}
// the forward GEMM of g: rows = y pixels, columns = Cout, per-tap K = Cin, x grouped (gc, gs) ...
inline FwdArgs fwd_args(const ConvGeom &g, int64_t x_gc, int64_t x_gs) {
  FwdArgs a;
  a.g = g;
  a.M = (int64_t)g.N * g.Ho * g.Wo; a.Ncol = g.Cout; a.KC = g.Cin;
  a.srcH = g.H; a.srcW = g.W; a.outH = g.Ho; a.outW = g.Wo;
  a.sgc = (int)x_gc; a.sgs = x_gs; a.ogc = g.Cout; a.ogs = 0;
  return a;
}
// ... and the input-gradient GEMM, the transposed roles: rows = dx pixels, columns = Cin,
// per-tap K = Cout, dx grouped (gc, gs).  Callers set only pointers and options.
inline FwdArgs dgrad_args(const ConvGeom &g, int64_t dx_gc, int64_t dx_gs) {
  FwdArgs a;
  a.g = g;
  a.M = (int64_t)g.N * g.H * g.W; a.Ncol = g.Cin; a.KC = g.Cout;
  a.srcH = g.Ho; a.srcW = g.Wo; a.outH = g.H; a.outW = g.W;
  a.sgc = g.Cout; a.sgs = 0; a.ogc = (int)dx_gc; a.ogs = dx_gs;
  return a;
}
inline WgradArgs wgrad_args(const ConvGeom &g, int64_t x_gc, int64_t x_gs) {
  WgradArgs a;
  a.g = g;
  a.M = (int64_t)g.N * g.Ho * g.Wo;
  a.xgc = (int)x_gc; a.xgs = x_gs;
  return a;
}
// argument validation (conv.hip); check_group normalises gc == 0 (plain NHWC) to (C, 0)
int check_geom(const ConvGeom &g, const char *nm);
int check_group(int64_t &gc, int64_t &gs, int64_t C, int64_t pixels, const char *nm, const char *which);
// the problems of a conv reading relu(x * scale + shift) in the windowed kernels (conv.hip):
// false when they do not take the shape
bool xf_args(FwdArgs &a, WgradArgs &w, const ConvGeom &g, int64_t x_group_c, int64_t x_group_stride);

// Kernel family: 1 (default) the LDS-DMA kernels wherever the shape allows them, the
// register-staged kernels elsewhere; 0 the register-staged kernels everywhere — a test
// switch (ewvit_conv2d_set_glds): they are the fallback of the shapes the LDS-DMA kernels
// refuse, so the tests run every case through both.
extern int g_glds;   // (conv_glds.hip)
inline bool use_glds() { return g_glds != 0; }
// the register-staged fwd / dgrad (conv_reg.hip): takes every shape; the small-channel 3x3:
// true when it ran the shape
void launch_fwd(const FwdArgs &a, bool dgrad, hipStream_t s);
bool launch_small(const FwdArgs &a, bool dgrad, hipStream_t s);
// the LDS-DMA fwd / dgrad (conv_glds.hip): true when it ran the shape (*bm_out: its row tile);
// its tile for a shape; the stride-2 3x3 dgrad as one launch per output parity class
bool launch_glds(const FwdArgs &a, int64_t src_bytes, bool dgrad, hipStream_t s, int *bm_out = nullptr);
void glds_tile(const FwdArgs &a, bool dgrad, int &bm, int &bn);
bool dgrad_by_parity(FwdArgs a, int64_t src_bytes, hipStream_t s);
// the windowed 3x3 stride-1 fwd / dgrad (convwin.hip): true when it ran the shape
bool launch_win(const FwdArgs &a, int64_t src_bytes, bool dgrad, hipStream_t s);
bool win_ok(const FwdArgs &a, bool dgrad);
extern int g_win;   // 1: the windowed kernels take the shapes they accept (default), 0: never
// the windowed 3x3 stride-1 weight gradient (convwin.hip): pixel splits it would use for this
// shape (0 = it does not take the shape), and the launch (slabs [splits][Cout][9*Cin] +
// bias partials [splits][Cout] for conv_wgrad_reduce_kernel)
int wgrad_win_splits(const WgradArgs &a, int64_t x_bytes);
bool launch_wgrad_win(const WgradArgs &a, int64_t x_bytes, int splits, hipStream_t s);

}  // namespace ewvit
