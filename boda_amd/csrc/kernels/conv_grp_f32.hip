// conv_grp_f32.hip -- a convolution with group = g > 1 and its data and filter gradients (hip_conv_grp, hip_bconv_in_grp, hip_bconv_filts_grp), fp32, NCHW / OIHW,
// for gfx950; specialised by hiprtc.  The reference has no grouped convolution; the definition is in terms of the ungrouped functions:
//
//   for every group j < g the ungrouped function on the op sliced to that group -- in[:, j*CG .. (j+1)*CG), filts[j*OCG .. (j+1)*OCG) (rows of CG x KH x KW),
//   biases[j*OCG ..), out / out_grad_loss[:, j*OCG .. (j+1)*OCG) -- the results side by side along the channel or filter-row axis.
//
// The image strides are those of the WHOLE tensors (p.C, p.OC); a group's share is the compile-time CG / OCG.  A thread never reads an operand of another group: an Inf or
// NaN in group j's operands changes no bit outside group j's outputs (containment).
//
// Two forms of each function, chosen by the planner from the op alone (plan_conv_grp) or forced by a seven-field tile; both are correct for every grouped geometry.
//
// FORM 1, the MATRIX form: per group the implicit GEMM of the ungrouped kernels, D[i][j] = sum_k A(k, i) * B(k, j) on v_mfma_f32_32x32x2_f32 (MT 32) or
// v_mfma_f32_16x16x4_f32 (MT 16; a group's row extent below 32), both exact ascending-k fma chains.  The group is one more coordinate of the workgroup walk
// (blockIdx -> group, row tile, column tile): a tile never straddles two groups, rows past the group's OCG (resp. CG) and terms past its K are OOB-zero buffer loads --
// never a neighbouring group's channel --, base offsets are g*CG planes / g*OCG rows, the image stride that of the whole C / OC.  A workgroup is WI x WJ waves, each
// with its own (BI / WI) x (BJ / WJ) tile of MT x MT blocks; the operands go from memory straight into the MFMA's registers (the caches serve the reuse; no LDS staging).
//   FUNC 1  i = out_chan of the group, j = (img, oy, ox), k = (c, ky, kx) ascending; a padded term is a product with +0; bias and ReLU on the finished chain.
//   FUNC 2  per phase (ry, rx) = ((y + PY) % SY, (x + PX) % SX), as kernels/bconv_in_f32.hip: i = in_chan of the group, j = the phase's pels (img, y, x),
//           k = (out_chan of the group, tx, ty) ascending = out_x, out_y ascending with the taps (ry + SY*(TY-1-ty), rx + SX*(TX-1-tx)) descending; a tap or an out
//           position that does not exist is a +0 operand (oracle/bck_chain.in_grad_chain).  Every pel belongs to one phase: every element is written.
//   FUNC 3  i = out_chan of the group, j = (c, fy, fx), k = (img, oy, ox) in KSL slices of whole BK steps; the tile BI x BJ is ONE wave's, the workgroup's KSL (1..16)
//           waves are the slices of that tile: each runs its chain from +0 (whole BK steps: the K tail's fma(+0, +0, acc) where a slice ends in a partial step), the
//           slabs meet in LDS and are added in slice order.  Deterministic; no atomics, no workspace.
//
// FORM 0, the DIRECT form: no MFMA, no LDS staging, one explicit fmaf chain per output in the written order: the form for small per-group reductions (depthwise
// layers, channel multipliers, CG x KH x KW or OCG too small to fill a matrix block).  There is no tile that could straddle two groups.
//
//   FUNC 1  out[img][oc][oy][ox] = act( chain + biases[oc] ), chain = fmaf(filts[oc][c][ky][kx], in[img][j*CG + c][oy*SY - PY + ky][ox*SX - PX + kx] or +0, chain)
//           from +0 over k = (c, ky, kx) ascending -- be=cpu's hip_conv chain (csrc/cpu_compute.cc: a padded term is a product with +0), the bias added after the
//           chain, then v > 0 ? v : +0 where RELU.  A thread owns VX adjacent outputs of one output row; a row segment of the input is read once per (c, ky) and serves
//           all KW taps from registers; the taps are plain per-lane loads of one filter row (lanes of one out_chan share the address; served by the caches).  At stride 1 with rows of
//           whole quads (W % 4 == 0) the span is read as aligned 16-byte loads; 16-byte stores where OW % 4 == 0.
//   FUNC 2  in_grad_loss[img][j*CG + c][y][x]: the reference template's chain (test/rtc/BckConv_in_grad_loss.cucl; be=cpu's bconv_in) -- out_chan of the group
//           ascending, out_x ascending, out_y ascending, the filter taps descending with them, only the terms that exist, from +0.  A position no term reaches is +0.
//           VX = 4 (a forced tile; stride 1 in x): a thread owns four adjacent x of a row -- one read of an out_grad_loss element serves all of them, 16-byte stores
//           where W % 4 == 0.  Measured level to slower than VX = 1, which the planner keeps.
//   FUNC 3  filts_grad_loss[oc][c][fy][fx] = slab[0] + slab[1] + ... + slab[KSL-1], slab s = one chain fmaf(out_grad_loss[k], in-patch[k] or +0, .) from +0 over the
//           K steps [s*kt_per, (s+1)*kt_per) of BK terms, k = (img, oy, ox) ascending, clipped to K = B*OH*OW; a slice that ends in a partial K step takes the K tail's
//           fma(+0, +0, acc) (a -0 becomes +0), an empty slice is +0: hip_bconv_filts' rule (kernels/bconv_filts_f32.hip; oracle/bck_chain.filts_sliced_chain).  A
//           thread owns all KH x KW taps of one (oc, c) pair for one slice and walks k in row segments (16-byte loads of out_grad_loss where OW % 4 == 0, the
//           input columns of a segment read once per filter row).  KSL = 1 writes the outputs; with K slices (2..1024) a thread writes its slab to the call's
//           workspace and a second launch in the same stream (-DSLAB_SUM=1) adds the slabs in slice order: deterministic, no atomics, no tickets.  KH x KW <= 49.
//
// -D parameters: KNAME FUNC FORM CG OCG KH KW SY SX PY PX | FORM 0: FUNC 1: RELU VX; FUNC 2: VX; FUNC 3: BK KSL [SLAB_SUM] | FORM 1: MT BI BJ BK WI WJ KSL, FUNC 1: RELU.  Host side: plan_conv_grp (native_plan.cc), native_kernels_t::conv_grp.

#ifndef __HIPCC_RTC__
#include <hip/hip_runtime.h>
#endif
#include "kernel_args.h"      // conv_grp_args_t
#include "device_prelude.h"

constexpr int kOOB = (int)0x80000000;   // byte offset beyond any num_records (tensors are < 2^31 bytes): the hardware returns 0
constexpr int kKHW = KH * KW;

#if FORM == 1
// ---------------------------------------------------------------- the matrix form
#if MT == 32
typedef f32x16 acc_t;
constexpr int kKS = 2, kNR = 16;   // k terms of one MFMA; accumulator registers of a block
__device__ __forceinline__ acc_t mma(float a, float b, acc_t c) { return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0); }
__device__ __forceinline__ int acc_row(int r, int lane) { return 8 * (r >> 2) + 4 * (lane >> 5) + (r & 3); }   // column = lane & 31
#else
typedef f32x4 acc_t;
constexpr int kKS = 4, kNR = 4;
__device__ __forceinline__ acc_t mma(float a, float b, acc_t c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }
__device__ __forceinline__ int acc_row(int r, int lane) { return 4 * (lane >> 4) + r; }                       // column = lane & 15
#endif
static_assert(MT == 32 || MT == 16, "MFMA block: 32 x 32 x 2 or 16 x 16 x 4");
#if FUNC == 3
constexpr int kWTI = BI, kWTJ = BJ, kNT = 64 * KSL;     // the tile is one wave's; the waves are the K slices
static_assert(KSL >= 1 && KSL <= 16 && BK % kKS == 0 && KSL * BI * BJ * 4 <= 65536, "K slices: 1..16 waves, slabs within the LDS");
#else
constexpr int kWTI = BI / WI, kWTJ = BJ / WJ, kNT = 64 * WI * WJ;
#endif
constexpr int kTI = kWTI / MT, kTJ = kWTJ / MT;
static_assert(kTI >= 1 && kTJ >= 1 && kWTI % MT == 0 && kWTJ % MT == 0 && kTI * kTJ * kNR <= 128, "a wave's tile: whole MFMA blocks, at most 128 accumulator registers");
constexpr int kM = (FUNC == 2) ? CG : OCG;              // a group's row extent
constexpr int kTilesI = (kM + BI - 1) / BI;

extern "C" __global__ __launch_bounds__(kNT) void KNAME(conv_grp_args_t const p) {
  int const tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  int const li = lane & (MT - 1), ko = lane / MT;       // operand index within a block; k offset within an MFMA
  int const OHW = p.OH * p.OW, HW = p.H * p.W;
  rsrc_t const rA = make_rsrc(p.a, p.a_bytes), rB = make_rsrc(p.b, p.b_bytes);
  acc_t acc[kTI][kTJ];
#pragma unroll
  for (int a = 0; a < kTI; ++a)
#pragma unroll
    for (int b = 0; b < kTJ; ++b)
#pragma unroll
      for (int r = 0; r < kNR; ++r) acc[a][b][r] = 0.f;
  float av[kTI], bv[kTJ];
  int bid = (int)blockIdx.x;
#if FUNC == 1
  constexpr int kK = CG * kKHW;
  int const N = p.B * OHW, tiles_j = (N + BJ - 1) / BJ;
  int const tj = bid % tiles_j; bid /= tiles_j;
  int const ti = bid % kTilesI, grp = bid / kTilesI;
  int const i0 = ti * BI + (wave / WJ) * kWTI, j0 = tj * BJ + (wave % WJ) * kWTJ;
  int offA[kTI], baseB[kTJ], iy0[kTJ], ix0[kTJ]; bool jok[kTJ];
#pragma unroll
  for (int a = 0; a < kTI; ++a) { int const i = i0 + a * MT + li; offA[a] = (i < OCG) ? (grp * OCG + i) * kK : -1; }
#pragma unroll
  for (int b = 0; b < kTJ; ++b) {
    int const j = j0 + b * MT + li, img = j / OHW, pel = j - img * OHW, oy = pel / p.OW, ox = pel - oy * p.OW;
    jok[b] = j < N; baseB[b] = (img * p.C + grp * CG) * HW; iy0[b] = oy * SY - PY; ix0[b] = ox * SX - PX;
  }
  for (int k0 = 0; k0 < kK; k0 += kKS) {
    int const k = k0 + ko, c = k / kKHW, r = k - c * kKHW, ky = r / KW, kx = r - ky * KW;
    bool const kok = k < kK;
#pragma unroll
    for (int a = 0; a < kTI; ++a) av[a] = bload1(rA, (kok && offA[a] >= 0) ? ((offA[a] + k) * 4) : kOOB);
#pragma unroll
    for (int b = 0; b < kTJ; ++b) {
      int const iy = iy0[b] + ky, ix = ix0[b] + kx;
      bool const ok = kok && jok[b] && (unsigned)iy < (unsigned)p.H && (unsigned)ix < (unsigned)p.W;
      bv[b] = bload1(rB, ok ? ((baseB[b] + c * HW + iy * p.W + ix) * 4) : kOOB);
    }
#pragma unroll
    for (int a = 0; a < kTI; ++a)
#pragma unroll
      for (int b = 0; b < kTJ; ++b) acc[a][b] = mma(av[a], bv[b], acc[a][b]);
  }
#pragma unroll
  for (int b = 0; b < kTJ; ++b) {
    int const j = j0 + b * MT + li;
    if (j >= N) continue;
    int const img = j / OHW, pel = j - img * OHW;
#pragma unroll
    for (int a = 0; a < kTI; ++a)
#pragma unroll
      for (int r = 0; r < kNR; ++r) {
        int const i = i0 + a * MT + acc_row(r, lane);
        if (i >= OCG) continue;
        int const oc = grp * OCG + i;
        float v = acc[a][b][r] + p.bias[oc];
        if (RELU) v = (v > 0.f) ? v : 0.f;
        p.d[((long)img * p.OC + oc) * OHW + pel] = v;
      }
  }
#elif FUNC == 2
  constexpr int TY = (KH + SY - 1) / SY, TX = (KW + SX - 1) / SX, kK = OCG * TX * TY;
  int const ti = bid % kTilesI; bid /= kTilesI;
  int const tiles_j = (int)p.n;                        // pel tiles over all phases (the host's walk: conv_grp_threads)
  int const grp = bid / tiles_j; int rem = bid - grp * tiles_j;
  int ry = 0, rx = 0, y0 = 0, x0 = 0, ny = 0, nx = 0;
  {   // workgroup -> (phase, pel tile of the phase): workgroup-uniform
    bool found = false;
    for (int py = 0; py < SY && !found; ++py)
      for (int px = 0; px < SX && !found; ++px) {
        int const yy = ((py - PY) % SY + SY) % SY, xx = ((px - PX) % SX + SX) % SX;
        int const my = (yy < p.H) ? (p.H - yy + SY - 1) / SY : 0, mx = (xx < p.W) ? (p.W - xx + SX - 1) / SX : 0;
        int const t = (p.B * my * mx + BJ - 1) / BJ;
        if (rem < t) { ry = py; rx = px; y0 = yy; x0 = xx; ny = my; nx = mx; found = true; } else rem -= t;
      }
    if (!found) return;
  }
  int const NP = p.B * ny * nx;
  int const i0 = ti * BI + (wave / WJ) * kWTI, j0 = rem * BJ + (wave % WJ) * kWTJ;
  int pimg[kTJ], py_[kTJ], px_[kTJ], qy[kTJ], qx[kTJ]; bool jok[kTJ];
#pragma unroll
  for (int b = 0; b < kTJ; ++b) {
    int const j = j0 + b * MT + li; jok[b] = j < NP;
    int const jj = jok[b] ? j : 0, img = jj / (ny * nx), q = jj - img * (ny * nx), my = q / nx, mx = q - my * nx;
    pimg[b] = img; py_[b] = y0 + my * SY; px_[b] = x0 + mx * SX; qy[b] = (py_[b] + PY) / SY; qx[b] = (px_[b] + PX) / SX;
  }
  for (int k0 = 0; k0 < kK; k0 += kKS) {
    int const k = k0 + ko, ocl = k / (TX * TY), r = k - ocl * (TX * TY), tx = r / TY, ty = r - tx * TY;
    int const fy = ry + SY * (TY - 1 - ty), fx = rx + SX * (TX - 1 - tx);
    bool const tap = k < kK && fy < KH && fx < KW;
#pragma unroll
    for (int a = 0; a < kTI; ++a) { int const i = i0 + a * MT + li; av[a] = bload1(rA, (tap && i < CG) ? ((((grp * OCG + ocl) * CG + i) * kKHW + fy * KW + fx) * 4) : kOOB); }
#pragma unroll
    for (int b = 0; b < kTJ; ++b) {
      int const oy = qy[b] - (TY - 1) + ty, ox = qx[b] - (TX - 1) + tx;
      bool const ok = tap && jok[b] && (unsigned)oy < (unsigned)p.OH && (unsigned)ox < (unsigned)p.OW;
      bv[b] = bload1(rB, ok ? ((((pimg[b] * p.OC + grp * OCG + ocl) * p.OH + oy) * p.OW + ox) * 4) : kOOB);
    }
#pragma unroll
    for (int a = 0; a < kTI; ++a)
#pragma unroll
      for (int b = 0; b < kTJ; ++b) acc[a][b] = mma(av[a], bv[b], acc[a][b]);
  }
#pragma unroll
  for (int b = 0; b < kTJ; ++b) {
    if (!jok[b]) continue;
#pragma unroll
    for (int a = 0; a < kTI; ++a)
#pragma unroll
      for (int r = 0; r < kNR; ++r) {
        int const i = i0 + a * MT + acc_row(r, lane);
        if (i < CG) p.d[(((long)pimg[b] * p.C + grp * CG + i) * p.H + py_[b]) * p.W + px_[b]] = acc[a][b][r];
      }
  }
#else
  constexpr int kN = CG * kKHW, kTilesJ = (kN + BJ - 1) / BJ;
  int const tj = bid % kTilesJ; bid /= kTilesJ;
  int const ti = bid % kTilesI, grp = bid / kTilesI;
  int const i0 = ti * BI, j0 = tj * BJ, slice = wave;
  int const K = p.B * OHW, nkt = (K + BK - 1) / BK;
  int const kt0 = min(slice * p.kt_per, nkt), kt1 = min(kt0 + p.kt_per, nkt);
  int offB[kTJ], jfy[kTJ], jfx[kTJ]; bool jok[kTJ];
#pragma unroll
  for (int b = 0; b < kTJ; ++b) {
    int const j = j0 + b * MT + li; jok[b] = j < kN;
    int const jj = jok[b] ? j : 0, c = jj / kKHW, f = jj - c * kKHW;
    jfy[b] = f / KW - PY; jfx[b] = f - (f / KW) * KW - PX; offB[b] = (grp * CG + c) * HW;
  }
  for (int kt = kt0; kt < kt1; ++kt)
    for (int kk = 0; kk < BK; kk += kKS) {
      int const k = kt * BK + kk + ko, img = k / OHW, pel = k - img * OHW, oy = pel / p.OW, ox = pel - oy * p.OW;
      bool const kok = k < K;
#pragma unroll
      for (int a = 0; a < kTI; ++a) { int const i = i0 + a * MT + li; av[a] = bload1(rA, (kok && i < OCG) ? (((img * p.OC + grp * OCG + i) * OHW + pel) * 4) : kOOB); }
#pragma unroll
      for (int b = 0; b < kTJ; ++b) {
        int const iy = oy * SY + jfy[b], ix = ox * SX + jfx[b];
        bool const ok = kok && jok[b] && (unsigned)iy < (unsigned)p.H && (unsigned)ix < (unsigned)p.W;
        bv[b] = bload1(rB, ok ? ((img * p.C * HW + offB[b] + iy * p.W + ix) * 4) : kOOB);
      }
#pragma unroll
      for (int a = 0; a < kTI; ++a)
#pragma unroll
        for (int b = 0; b < kTJ; ++b) acc[a][b] = mma(av[a], bv[b], acc[a][b]);
    }
#if KSL > 1
  {   // the slabs meet in LDS and are added in slice order; element e = ((a * kTJ + b) * kNR + r) * 64 + lane
    constexpr int kE = kTI * kTJ * kNR * 64;
    __shared__ float slab[KSL * kE];
#pragma unroll
    for (int a = 0; a < kTI; ++a)
#pragma unroll
      for (int b = 0; b < kTJ; ++b)
#pragma unroll
        for (int r = 0; r < kNR; ++r) slab[slice * kE + ((a * kTJ + b) * kNR + r) * 64 + lane] = acc[a][b][r];
    __syncthreads();
    for (int e = tid; e < kE; e += kNT) {
      float sum = slab[e];
      for (int s = 1; s < KSL; ++s) sum = sum + slab[s * kE + e];
      int const ln = e & 63, r = (e >> 6) % kNR, ab = (e >> 6) / kNR, a = ab / kTJ, b = ab - a * kTJ;
      int const i = i0 + a * MT + acc_row(r, ln), j = j0 + b * MT + (ln & (MT - 1));
      if (i < OCG && j < kN) p.d[(long)(grp * OCG + i) * kN + j] = sum;
    }
  }
#else
#pragma unroll
  for (int b = 0; b < kTJ; ++b) {
    int const j = j0 + b * MT + li;
    if (j >= kN) continue;
#pragma unroll
    for (int a = 0; a < kTI; ++a)
#pragma unroll
      for (int r = 0; r < kNR; ++r) { int const i = i0 + a * MT + acc_row(r, lane); if (i < OCG) p.d[(long)(grp * OCG + i) * kN + j] = acc[a][b][r]; }
  }
#endif
#endif
}

// ---------------------------------------------------------------- the direct form
#elif FUNC == 1
constexpr int kSpan = (VX - 1) * SX + KW;   // input columns the VX outputs of a thread meet in one filter row
constexpr bool kVecSpan = SX == 1 && VX == 4;           // (ox0 is then a multiple of 4)
constexpr int kA0 = (4 - PX % 4) % 4;                   // the span's first column ox0 - PX within its aligned quad
constexpr int kChunks = (kA0 + kSpan + 3) / 4;
extern "C" __global__ __launch_bounds__(256) void KNAME(conv_grp_args_t const p) {
  long const t = (long)blockIdx.x * 256 + threadIdx.x;
  if (t >= p.n) return;
  int const nxq = (p.OW + VX - 1) / VX;
  int const xq = (int)(t % nxq); long r = t / nxq;
  int const oy = (int)(r % p.OH); r /= p.OH;
  int const oc = (int)(r % p.OC), img = (int)(r / p.OC);
  int const grp = oc / OCG, ox0 = xq * VX;
  rsrc_t const rIn = make_rsrc(p.b, p.b_bytes);
  float const *const f = p.a + (long)oc * (CG * kKHW);
  int const HW = p.H * p.W;
  int const in0 = (img * p.C + grp * CG) * HW;
  int const ix0 = ox0 * SX - PX;
  float acc[VX];
#pragma unroll
  for (int i = 0; i < VX; ++i) acc[i] = 0.f;
  for (int c = 0; c < CG; ++c) {
#pragma unroll
    for (int ky = 0; ky < KH; ++ky) {
      int const iy = oy * SY - PY + ky;
      bool const row_ok = (unsigned)iy < (unsigned)p.H;
      int const rbase = in0 + c * HW + iy * p.W;
      float x[kSpan];
      if (kVecSpan && (p.W & 3) == 0) {   // stride 1, four outputs, rows of whole quads: the span as aligned 16-byte loads (a quad lies wholly inside the row or wholly outside it)
        f32x4 q[kChunks];
#pragma unroll
        for (int j = 0; j < kChunks; ++j) { int const cx = ix0 - kA0 + 4 * j; q[j] = bload4(rIn, (row_ok && (unsigned)cx < (unsigned)p.W) ? ((rbase + cx) * 4) : kOOB); }
#pragma unroll
        for (int s = 0; s < kSpan; ++s) x[s] = q[(kA0 + s) / 4][(kA0 + s) % 4];
      } else {
#pragma unroll
        for (int s = 0; s < kSpan; ++s) { int const ix = ix0 + s; x[s] = bload1(rIn, (row_ok && (unsigned)ix < (unsigned)p.W) ? ((rbase + ix) * 4) : kOOB); }
      }
#pragma unroll
      for (int kx = 0; kx < KW; ++kx) {
        float const w = f[c * kKHW + ky * KW + kx];
#pragma unroll
        for (int i = 0; i < VX; ++i) acc[i] = __builtin_fmaf(w, x[i * SX + kx], acc[i]);   // (outputs past the row's end: dropped by the store)
      }
    }
  }
  float const bias = p.bias[oc];
  long const o = (((long)img * p.OC + oc) * p.OH + oy) * p.OW + ox0;
  float v[VX];
#pragma unroll
  for (int i = 0; i < VX; ++i) { v[i] = acc[i] + bias; if (RELU) v[i] = (v[i] > 0.f) ? v[i] : 0.f; }
  if (VX == 4 && (p.OW & 3) == 0) { f32x4 q; q[0] = v[0]; q[1] = v[1 % VX]; q[2] = v[2 % VX]; q[3] = v[3 % VX]; *reinterpret_cast<f32x4 *>(p.d + o) = q; }
  else {
#pragma unroll
    for (int i = 0; i < VX; ++i) if (ox0 + i < p.OW) p.d[o + i] = v[i];
  }
}

#elif FUNC == 2
static_assert(VX == 1 || SX == 1, "adjacent outputs of one thread share their out_x terms at stride 1 only");
extern "C" __global__ __launch_bounds__(256) void KNAME(conv_grp_args_t const p) {
  long const t = (long)blockIdx.x * 256 + threadIdx.x;
  if (t >= p.n) return;
  int const nxq = (p.W + VX - 1) / VX;
  int const x0 = (int)(t % nxq) * VX; long r = t / nxq;
  int const y = (int)(r % p.H); r /= p.H;
  int const cf = (int)(r % p.C), img = (int)(r / p.C);
  int const grp = cf / CG, c = cf - grp * CG;
  int const OHW = p.OH * p.OW;
  int const oyb = max(0, y + PY - KH + SY) / SY, oye = min((y + PY) / SY + 1, p.OH);
  float const *const g = p.b + ((long)img * p.OC + grp * OCG) * OHW;
  float const *const f = p.a + ((long)grp * OCG * CG + c) * kKHW;
  float v[VX];
#pragma unroll
  for (int i = 0; i < VX; ++i) v[i] = 0.f;
#if VX == 1
  int const oxb = max(0, x0 + PX - KW + SX) / SX, oxe = min((x0 + PX) / SX + 1, p.OW);
  for (int ocl = 0; ocl < OCG; ++ocl) {
    int fx = x0 + PX - oxb * SX;   // out_x ascending (outer), the filter taps descending
    for (int ox = oxb; ox < oxe; ++ox, fx -= SX) {
      int fy = y + PY - oyb * SY;
      for (int oy = oyb; oy < oye; ++oy, fy -= SY)
        v[0] = __builtin_fmaf(g[ocl * OHW + oy * p.OW + ox], f[ocl * (CG * kKHW) + fy * KW + fx], v[0]);
    }
  }
#else
  // VX adjacent x at stride 1: one walk over the union of their out_x ranges; an out_grad_loss element is read once and serves every output it is a term of.  Each
  // output still meets exactly its own terms, out_x ascending (outer), out_y ascending: the chains are the single-output ones
  int const oxlo = max(0, x0 + PX - KW + 1), oxhi = min(x0 + VX + PX, p.OW);
  for (int ocl = 0; ocl < OCG; ++ocl)
    for (int ox = oxlo; ox < oxhi; ++ox) {
      int fy = y + PY - oyb * SY;
      for (int oy = oyb; oy < oye; ++oy, fy -= SY) {
        float const gv = g[ocl * OHW + oy * p.OW + ox];
#pragma unroll
        for (int i = 0; i < VX; ++i) {
          int const fx = x0 + i + PX - ox;
          if ((unsigned)fx < (unsigned)KW) v[i] = __builtin_fmaf(gv, f[ocl * (CG * kKHW) + fy * KW + fx], v[i]);
        }
      }
    }
#endif
  long const o = (((long)img * p.C + cf) * p.H + y) * p.W + x0;
  if (VX == 4 && (p.W & 3) == 0) { f32x4 q; q[0] = v[0]; q[1] = v[1 % VX]; q[2] = v[2 % VX]; q[3] = v[3 % VX]; *reinterpret_cast<f32x4 *>(p.d + o) = q; }
  else {
#pragma unroll
    for (int i = 0; i < VX; ++i) if (x0 + i < p.W) p.d[o + i] = v[i];
  }
}

#else
// A thread owns ALL KH x KW taps of one (out_chan, in_chan) pair for one K slice: it walks k = (img, oy, ox) ascending in row segments -- four consecutive ox where the
// row allows (OW % 4 == 0: one 16-byte load of out_grad_loss), else one -- reads the segment's input columns once per filter row and feeds every tap's chain from
// registers, the segment's terms in ascending k.  Each tap's chain is the written one: fma(g[k], in-patch[k] or +0, acc) from +0 over the slice, then the K tail's +0.
static_assert(KSL >= 1 && KSL <= 1024 && BK >= 1 && kKHW <= 49, "K slices: 1..1024; a kernel's taps in registers");
template <int N> __device__ __forceinline__ void filts_seg(float (&acc)[KH][KW], float const (&gv)[4], rsrc_t rIn, int plane, int oy, int ox, int H, int W) {
  constexpr int kSp = (N - 1) * SX + KW;
#pragma unroll
  for (int fy = 0; fy < KH; ++fy) {
    int const iy = oy * SY - PY + fy;
    bool const row_ok = (unsigned)iy < (unsigned)H;
    float x[kSp];
#pragma unroll
    for (int s = 0; s < kSp; ++s) { int const ix = ox * SX - PX + s; x[s] = bload1(rIn, (row_ok && (unsigned)ix < (unsigned)W) ? ((plane + iy * W + ix) * 4) : kOOB); }
#pragma unroll
    for (int fx = 0; fx < KW; ++fx)
#pragma unroll
      for (int i = 0; i < N; ++i) acc[fy][fx] = __builtin_fmaf(gv[i], x[i * SX + fx], acc[fy][fx]);   // ascending k within the segment
  }
}
#if SLAB_SUM
// the second launch of a sliced call: one thread per element of filts_grad_loss, slab[0] + slab[1] + ... + slab[ksl-1] in slice order, plain fp32 adds
extern "C" __global__ __launch_bounds__(256) void KNAME(conv_grp_args_t const p) {
  long const e = (long)blockIdx.x * 256 + threadIdx.x, n = p.n * kKHW;
  if (e >= n) return;
  float const *const s = p.ws + e;
  float sum = s[0];
  for (int q = 1; q < (int)p.ksl; ++q) sum = sum + s[(long)q * n];
  p.d[e] = sum;
}
#else
extern "C" __global__ __launch_bounds__(256) void KNAME(conv_grp_args_t const p) {
  long const t = (long)blockIdx.x * 256 + threadIdx.x;
  long const pair = t / KSL;                        // (oc, c): kKHW consecutive elements of filts_grad_loss
  int const s = (int)(t - pair * KSL);              // the slice; the lanes of a wave are neighbouring slices of one pair
  if (pair >= p.n) return;
  float acc[KH][KW];
#pragma unroll
  for (int fy = 0; fy < KH; ++fy)
#pragma unroll
    for (int fx = 0; fx < KW; ++fx) acc[fy][fx] = 0.f;
  {
    int const c = (int)(pair % CG), oc = (int)(pair / CG), grp = oc / OCG;
    int const OHW = p.OH * p.OW, HW = p.H * p.W, K = p.B * OHW;
    int const nkt = (K + BK - 1) / BK;
    int const kt0 = min(s * p.kt_per, nkt), kt1 = min(kt0 + p.kt_per, nkt);
    int const k0 = min(kt0 * BK, K), k1 = min(kt1 * BK, K);
    rsrc_t const rIn = make_rsrc(p.b, p.b_bytes);
    bool const quads = (p.OW & 3) == 0;
    int img = k0 / OHW, pel = k0 - img * OHW, oy = pel / p.OW, ox = pel - oy * p.OW;
    for (int k = k0; k < k1;) {
      float const *const gp = p.a + ((long)img * p.OC + oc) * OHW + oy * p.OW + ox;
      int const plane = (img * p.C + grp * CG + c) * HW;
      float gv[4];
      int n = 1;
      if (quads && (ox & 3) == 0 && k + 4 <= k1) {   // four consecutive ox of one row, 16-byte aligned
        f32x4 const q = *reinterpret_cast<f32x4 const *>(gp);
        gv[0] = q[0]; gv[1] = q[1]; gv[2] = q[2]; gv[3] = q[3];
        filts_seg<4>(acc, gv, rIn, plane, oy, ox, p.H, p.W); n = 4;
      } else { gv[0] = gp[0]; gv[1] = gv[2] = gv[3] = 0.f; filts_seg<1>(acc, gv, rIn, plane, oy, ox, p.H, p.W); }
      k += n; ox += n;
      if (ox == p.OW) { ox = 0; if (++oy == p.OH) { oy = 0; ++img; } }
    }
    if ((k1 - k0) % BK) {   // the slice ends in the K tail: fma(+0, +0, acc)
#pragma unroll
      for (int fy = 0; fy < KH; ++fy)
#pragma unroll
        for (int fx = 0; fx < KW; ++fx) acc[fy][fx] = acc[fy][fx] + 0.f;
    }
  }
  // KSL = 1: the outputs; else slab s of the call's workspace, in the outputs' layout
  float *const o = (KSL == 1 ? p.d : p.ws + (long)s * (p.n * kKHW)) + pair * kKHW;
#pragma unroll
  for (int fy = 0; fy < KH; ++fy)
#pragma unroll
    for (int fx = 0; fx < KW; ++fx) o[fy * KW + fx] = acc[fy][fx];
}
#endif
#endif
