// bconv_in_bf16.hip -- data gradient of a convolution (BckConv in_grad_loss) with bf16 OPERANDS and fp32 sums, for gfx950; specialised at run time by hiprtc.
// The function op's hip_operands=bf16 on hip_bconv_in selects it; tensors stay fp32 in the reference layouts.  With r(v) = fp32 -> bf16 round-to-nearest-even
// (v_cvt_pk_bf16_f32; inf stays inf, NaN stays NaN):
//
//   in_grad_loss[img][c][iy][ix] = sum_{oc, ox, oy} r(out_grad_loss[img][oc][oy][ox]) * r(filts[oc][c][iy + PY - oy*SY][ix + PX - ox*SX])     (fp32 accumulation)
//
// The sub-pixel phase decomposition, the tile walk, the OOB-zero buffer loads and the -DZINP epilogue are bconv_in_f32.hip's: per phase
//   D[i = c][j = pel of the phase] = sum_k I(k, c) * J(k, pel),   k = (oc, ixt, iyt),   I = the phase's flipped sub-filter, J = out_grad_loss (0 outside the plane).
// What changes is the matrix instruction, v_mfma_f32_32x32x16_bf16 (16 k per instruction, 16 times the fp32 MFMA rate), and so the on-chip data path.
//
// Data path (the form of gemm_conv_bf16.hip).  Both operands are K-OUTER in memory: out_grad_loss has its pels contiguous at one (oc, tap), a 1x1 layer's filts its
// in_chan contiguous at one oc.  The MFMA fragment wants 8 consecutive k per lane.  So a thread owns ONE column (a channel of I, a pel of J) and 8 consecutive k: it
// issues 8 dword buffer loads -- each of them wave-coalesced, the lanes of a wave being consecutive columns at one k -- converts with v_cvt_pk_bf16_f32 and writes one
// 16-byte chunk (ds_write_b128) into a [column][BK + 8] bf16 image; the fragments are ds_read_b128.  The K tail (k >= K), taps outside the kernel, pels outside the plane
// and columns past the tensor all read byte offset kOOB, which the buffer hardware answers with 0: a select on the offset, no branch per load.
//
// LDS banks.  The row pitch is (BK + 8) * 2 bytes = (BK/8 + 1) 16-byte slots, an ODD number of slots for every BK that is a multiple of 16 (48 B at BK 16, 80 B at 32,
// 144 B at 64).  ds_read_b128 is served in four groups of 16 lanes over 64 banks (16 slots of a 256-byte bank row); the 16 lanes of a group read 16 rows whose numbers
// cover every residue mod 16 ({0-3, 12-15, 20-27} and {4-11, 16-19, 28-31}, likewise for the upper half wave), at one k offset: slot = (row * odd + const) mod 16 takes 16
// different values -- conflict-free.  ds_write_b128 is served in eight groups of 8 consecutive lanes over 32 banks (8 slots): 8 consecutive columns at one k chunk,
// slot = (column * odd + const) mod 8, 8 different values -- conflict-free as well.
//
// Numerics.  Products of bf16 values are exact in fp32; the 16 terms inside one MFMA are not a sequential fma chain, so the ORDER of the fp32 additions is the
// instruction's and the result is held to a bound, not to bits.  It is the same bits from run to run and from graph replay to eager: one
// workgroup owns an output, K is not sliced, nothing is atomic.  The finite-data caveat of the fp32 kernel applies: padded terms are 0 * x, so an inf / NaN in filts or
// out_grad_loss poisons terms the formula never forms.  What the bf16 MFMA does with subnormal operands is not stated in the hardware guides and is not tested.
//
// -DZINP=1: in_grad_loss[e] = in[e] > 0 ? g[e] : +0 on the finished value, the condition `in` read UNROUNDED (bconv_in_f32.hip's select).  Positions no term reaches
// (1x1 at stride 2) are +0 either way.
//
// -D parameters: KNAME BI BJ BK WI WJ MINW KH KW SY SX PY PX [ZINP].  Host side: plan_bconv_in_bf16 (native_plan.cc), native_kernels_t::bconv_in (native_kernels.cc).

#ifndef __HIPCC_RTC__
#include <hip/hip_runtime.h>
#endif
#ifndef ZINP
#define ZINP 0
#endif

#include "kernel_args.h"      // bconv_args_t
#include "device_prelude.h"

constexpr int kOOB = (int)0x80000000;   // byte offset beyond any num_records (tensors are < 2^31 bytes): the hardware returns 0

constexpr int kTY = (KH + SY - 1) / SY, kTX = (KW + SX - 1) / SX, kTT = kTY * kTX;
constexpr int kNT = WI * WJ * 64;
constexpr int kTI = BI / (WI * 32), kTJ = BJ / (WJ * 32);
constexpr int kP = BK + 8;                                    // LDS row pitch (bf16 elements)
constexpr int kKC = BK / 8;                                   // 8-k chunks of a column per K step
constexpr int kCI = (BI * kKC + kNT - 1) / kNT, kCJ = (BJ * kKC + kNT - 1) / kNT;   // chunks per thread
static_assert(BI % (WI * 32) == 0 && BJ % (WJ * 32) == 0 && BK % 16 == 0, "tile: whole 32 x 32 MFMA blocks, K steps of 16");
static_assert(kNT % BI == 0 && kNT % BJ == 0, "staging: every thread owns one column of each operand");
static_assert(((BI * kKC) % kNT == 0 || BI * kKC < kNT) && ((BJ * kKC) % kNT == 0 || BJ * kKC < kNT), "staging: whole chunks per thread, or fewer chunks than threads");

extern "C" __global__ __launch_bounds__(WI * WJ * 64, MINW) void KNAME(bconv_args_t const p) {
  __shared__ __attribute__((aligned(16))) __bf16 smem[2 * (BI + BJ) * kP];
  int const tid = threadIdx.x, lane = tid & 63;
  int const wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  int const wi = wave / WJ, wj = wave % WJ;

  // ---- workgroup -> (phase, pel tile, channel tile); the host sizes the grid with the same walk (bconv_in_tiles)
  int const tile_i = (int)blockIdx.x % p.tiles_i;
  int jt = (int)blockIdx.x / p.tiles_i;
  int ry = 0, rx = 0, ny = 0, nx = 0;
  for (int ph = 0; ph < SY * SX; ++ph) {
    ry = ph / SX; rx = ph % SX;
    ny = (ry < p.H) ? (p.H - ry + SY - 1) / SY : 0; nx = (rx < p.W) ? (p.W - rx + SX - 1) / SX : 0;
    int const nt = (p.B * ny * nx + BJ - 1) / BJ;
    if (jt < nt) break;
    jt -= nt;
  }
  int const P = p.B * ny * nx, nyx = ny * nx;
  int const py = (ry + PY) % SY, px = (rx + PX) % SX, qy0 = (ry + PY) / SY, qx0 = (rx + PX) / SX;
  int const i0 = tile_i * BI, j0 = jt * BJ;
  int const K = p.OC * kTT, OHW = p.OH * p.OW, KHW = KH * KW;
  rsrc_t const rA = make_rsrc(p.a, p.a_bytes), rB = make_rsrc(p.b, p.b_bytes);

  // ---- staging roles: chunk q of a thread is column tid % BX, k chunk tid / BX + q * (kNT / BX) (8 consecutive k)
  int const icol = tid % BI, ikc0 = tid / BI, jcol = tid % BJ, jkc0 = tid / BJ;
  int const ic = i0 + icol, jl = j0 + jcol;
  bool const c_ok = ic < p.C, j_ok = jl < P;
  int oyb = 0, oxb = 0, jbase = 0;
  {
    int const img = jl / max(nyx, 1), rem = jl - img * nyx, ty = rem / max(nx, 1), tx = rem - ty * nx;
    oyb = qy0 + ty - (kTY - 1); oxb = qx0 + tx - (kTX - 1);   // (oy, ox) of k-taps iyt = ixt = 0
    jbase = (img * p.OC * p.OH + oyb) * p.OW + oxb;
  }
  float ra[kCI * 8], rb[kCJ * 8];
  auto load = [&](int k0) {
#pragma unroll
    for (int q = 0; q < kCI; ++q) {
      int const kc = ikc0 + q * (kNT / BI);
      if (kc >= kKC) continue;   // (only where there are fewer chunks than threads)
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        int const k = k0 + 8 * kc + e;
        int const oc = k / kTT, t = k - oc * kTT, ixt = t / kTY, iyt = t - ixt * kTY;
        int const fy = py + SY * (kTY - 1 - iyt), fx = px + SX * (kTX - 1 - ixt);
        bool const ok = c_ok && k < K && fy < KH && fx < KW;
        ra[q * 8 + e] = bload1(rA, ok ? (((oc * p.C + ic) * KHW + fy * KW + fx) * 4) : kOOB);
      }
    }
#pragma unroll
    for (int q = 0; q < kCJ; ++q) {
      int const kc = jkc0 + q * (kNT / BJ);
      if (kc >= kKC) continue;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        int const k = k0 + 8 * kc + e;
        int const oc = k / kTT, t = k - oc * kTT, ixt = t / kTY, iyt = t - ixt * kTY;
        bool const ok = j_ok && k < K && (unsigned)(oyb + iyt) < (unsigned)p.OH && (unsigned)(oxb + ixt) < (unsigned)p.OW;
        rb[q * 8 + e] = bload1(rB, ok ? ((jbase + oc * OHW + iyt * p.OW + ixt) * 4) : kOOB);
      }
    }
  };
  auto store = [&](int buf) {   // 8 fp32 -> one 16-byte bf16 chunk (round-to-nearest-even)
    __bf16 *const Is = smem + buf * (BI + BJ) * kP, *const Js = Is + BI * kP;
#pragma unroll
    for (int q = 0; q < kCI; ++q) {
      int const kc = ikc0 + q * (kNT / BI);
      if (kc >= kKC) continue;
      bf16x8 v;
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = (__bf16)ra[q * 8 + e];
      *reinterpret_cast<bf16x8 *>(Is + icol * kP + 8 * kc) = v;
    }
#pragma unroll
    for (int q = 0; q < kCJ; ++q) {
      int const kc = jkc0 + q * (kNT / BJ);
      if (kc >= kKC) continue;
      bf16x8 v;
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = (__bf16)rb[q * 8 + e];
      *reinterpret_cast<bf16x8 *>(Js + jcol * kP + 8 * kc) = v;
    }
  };

  f32x16 acc[kTI][kTJ];
#pragma unroll
  for (int a = 0; a < kTI; ++a)
#pragma unroll
    for (int b = 0; b < kTJ; ++b) acc[a][b] = f32x16{0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};

  // fragment fetch: lane l holds A[i = l & 31][k = 8 * (l >> 5) .. + 7] (and B alike) of each 16-deep MFMA step
  int const a_off = (wi * (kTI * 32) + (lane & 31)) * kP + 8 * (lane >> 5);
  int const b_off = (BI + wj * (kTJ * 32) + (lane & 31)) * kP + 8 * (lane >> 5);
  int const nkt = (K + BK - 1) / BK;
  load(0); store(0);
  __syncthreads();
  for (int t = 0; t < nkt; ++t) {
    if (t + 1 < nkt) load((t + 1) * BK);   // in flight during the MFMAs of step t
    __bf16 const *const S = smem + (t & 1) * (BI + BJ) * kP;
#pragma unroll
    for (int kk = 0; kk < BK / 16; ++kk) {
      bf16x8 av[kTI], bv[kTJ];
#pragma unroll
      for (int a = 0; a < kTI; ++a) av[a] = *reinterpret_cast<bf16x8 const *>(S + a_off + a * 32 * kP + kk * 16);
#pragma unroll
      for (int b = 0; b < kTJ; ++b) bv[b] = *reinterpret_cast<bf16x8 const *>(S + b_off + b * 32 * kP + kk * 16);
#pragma unroll
      for (int a = 0; a < kTI; ++a)
#pragma unroll
        for (int b = 0; b < kTJ; ++b) acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av[a], bv[b], acc[a][b], 0, 0, 0);
    }
    if (t + 1 < nkt) store((t + 1) & 1);   // the other buffer: every wave finished reading it before the previous barrier
    __syncthreads();
  }

  // ---- epilogue (bconv_in_f32.hip's): C/D layout of the 32x32 MFMA family -- column j = lane & 31, row i = 8*(r>>2) + 4*(lane>>5) + (r&3) for register r
#pragma unroll
  for (int b = 0; b < kTJ; ++b) {
    int const j = j0 + wj * (kTJ * 32) + b * 32 + (lane & 31);
    if (j >= P) continue;
    int const img = j / nyx, rem = j - img * nyx, ty = rem / nx, tx = rem - ty * nx;
    long const obase = ((long)img * p.C * p.H + (ry + SY * ty)) * p.W + (rx + SX * tx);
#if ZINP
    // the condition values of this column of blocks, all loaded before its first store; a channel past the tensor reads the last channel instead (never stored)
    float zc[kTI][16];
#pragma unroll
    for (int a = 0; a < kTI; ++a)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        int const c = i0 + wi * (kTI * 32) + a * 32 + 8 * (r >> 2) + 4 * (lane >> 5) + (r & 3);
        zc[a][r] = p.zin[obase + (long)(c < p.C ? c : p.C - 1) * p.H * p.W];
      }
    __builtin_amdgcn_s_waitcnt(0x0F70);   // vmcnt(0): every condition value has arrived before the first store
#endif
#pragma unroll
    for (int a = 0; a < kTI; ++a)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        int const c = i0 + wi * (kTI * 32) + a * 32 + 8 * (r >> 2) + 4 * (lane >> 5) + (r & 3);
#if ZINP
        if (c < p.C) p.d[obase + (long)c * p.H * p.W] = zc[a][r] > 0.0f ? acc[a][b][r] : 0.0f;
#else
        if (c < p.C) p.d[obase + (long)c * p.H * p.W] = acc[a][b][r];
#endif
      }
  }
}
