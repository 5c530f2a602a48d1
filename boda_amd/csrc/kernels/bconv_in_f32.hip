// bconv_in_f32.hip -- data gradient of a convolution (BckConv in_grad_loss), fp32 MFMA, for gfx950; specialised at run time by hiprtc.
//
//   in_grad_loss[img][c][iy][ix] = sum_{oc, ox, oy} out_grad_loss[img][oc][oy][ox] * filts[oc][c][iy + PY - oy*SY][ix + PX - ox*SX]
//
// Sub-pixel (phase) decomposition (as the reference's bconv, src/cnn_op.cc:80-113): the input pels with iy = ry + SY*ty, ix = rx + SX*tx (residues ry < SY,
// rx < SX) form one phase; inside it the gradient is a stride-1 correlation of out_grad_loss with a flipped sub-filter of TY x TX taps (TY = ceil(KH/SY),
// taps fy = py + SY*(TY-1-jy), py = (ry+PY) % SY; taps beyond the kernel are zero).  One launch covers all SY*SX phases: each workgroup tile lies inside ONE
// phase, so the filter operand of the tile is that phase's sub-filter.  Per phase an implicit GEMM
//   D[i = c][j = pel of the phase] = sum_k I(k, c) * J(k, pel),   k = (oc, ixt, iyt): oc ascending, then ox ascending, then oy ascending
// with I(k, c) = filts[oc][c][fy][fx] (0 for taps outside the kernel), J(k, pel) = out_grad_loss[img][oc][oy][ox] (0 outside the plane: OOB-zero buffer loads).
//
// Numerics: v_mfma_f32_32x32x2_f32 is an exact fp32 fma chain in ascending k, so every output is ONE fma chain in exactly the order of the reference's
// template (test/rtc/BckConv_in_grad_loss.cucl: out_chan, then out_x, then out_y; the filter taps run descending) -- bit-identical to it.  The extra terms
// (borders, taps outside the kernel, the K tail past OC * TY * TX) are fma(0, w, acc), fma(g, 0, acc) or fma(0, 0, acc), which equal acc for FINITE data up to the
// sign of a zero.  The accumulator starts at +0 but does become -0: a negative product that underflows gives fma(g, w, +0) = -0, and it stays -0 through further
// such terms.  A padded term fma(+0, w, -0) with w > 0, or any K-tail term, then gives +0 where the reference, which skips the term, keeps -0 -- equal by value,
// not by bits (oracle/bck_chain.in_grad_chain forms the same terms; the directed case of tests/test_gpu_bck_special.py shows both signs).
// An inf / nan in out_grad_loss poisons the padded terms the reference never forms: every pel of the element's PHASE WINDOW y + PY - oy*SY in [0, SY*TY) (likewise x)
// comes back as a NaN, not only the pels of its kernel window [0, KH) -- measured: all of them, on every strided form whose stride does not divide the kernel size;
// outside the phase window nothing changes.  An inf / nan in filts is contained in its in_chan.
//
// -DZINP=1 (the function op's zero_if_in_non_pos): the ReLU gradient that follows this launch in a gradient pipe, folded into the store --
//   in_grad_loss[e] = in[e] > 0 ? g[e] : +0,   g[e] the value above, `in` (p.zin) the convolution's forward input, which has in_grad_loss's dims:
// hip_zero_if_non_pos's rule (kernels/bck_ops_f32.hip OP 5) with cond = in.  A select on the finished chain, never a product: a +0, -0 or NaN condition gives +0
// whatever g is.  The MFMA chains are the same; positions no term reaches (1x1 at stride 2) are written +0 either way.
//
// -D parameters: KNAME BI BJ BK WI WJ MINW KH KW SY SX PY PX [ZINP].  Host side: plan_bconv_in (native_plan.cc), native_kernels_t::bconv_in (native_kernels.cc).

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
constexpr int kIR = BK * BI / kNT, kJR = BK * BJ / kNT;   // staged elements per thread
constexpr int kIP = BI + 4, kJP = BJ + 4;                 // LDS row pitches (floats)
static_assert(BI % (WI * 32) == 0 && BJ % (WJ * 32) == 0 && BK % 2 == 0, "tile: whole 32 x 32 MFMA blocks, K steps of 2");
static_assert(kNT % BI == 0 && kNT % BJ == 0 && (BK * BI) % kNT == 0 && (BK * BJ) % kNT == 0, "staging: every thread owns one column and whole rows");

extern "C" __global__ __launch_bounds__(WI * WJ * 64, MINW) void KNAME(bconv_args_t const p) {
  __shared__ __attribute__((aligned(16))) float smem[2 * BK * (kIP + kJP)];
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

  // ---- staging roles: filter operand column c = i0 + tid % BI, rows tid / BI + r * (kNT / BI); gradient operand column = pel j0 + tid % BJ, rows likewise
  int const ic = i0 + tid % BI, ir0 = tid / BI;
  int const jl = j0 + tid % BJ, jr0 = tid / BJ;
  bool const c_ok = ic < p.C;
  int oyb = 0, oxb = 0, jbase = 0; bool const j_ok = jl < P;
  {
    int const img = jl / max(nyx, 1), rem = jl - img * nyx, ty = rem / max(nx, 1), tx = rem - ty * nx;
    oyb = qy0 + ty - (kTY - 1); oxb = qx0 + tx - (kTX - 1);   // (oy, ox) of k-taps iyt = ixt = 0
    jbase = (img * p.OC * p.OH + oyb) * p.OW + oxb;
  }
  float ra[kIR], rb[kJR];
  auto load = [&](int k0) {
#pragma unroll
    for (int r = 0; r < kIR; ++r) {
      int const k = k0 + ir0 + r * (kNT / BI);
      int const oc = k / kTT, t = k - oc * kTT, ixt = t / kTY, iyt = t - ixt * kTY;
      int const fy = py + SY * (kTY - 1 - iyt), fx = px + SX * (kTX - 1 - ixt);
      bool const ok = c_ok && k < K && fy < KH && fx < KW;
      ra[r] = bload1(rA, ok ? (((oc * p.C + ic) * KHW + fy * KW + fx) * 4) : kOOB);
    }
#pragma unroll
    for (int r = 0; r < kJR; ++r) {
      int const k = k0 + jr0 + r * (kNT / BJ);
      int const oc = k / kTT, t = k - oc * kTT, ixt = t / kTY, iyt = t - ixt * kTY;
      bool const ok = j_ok && k < K && (unsigned)(oyb + iyt) < (unsigned)p.OH && (unsigned)(oxb + ixt) < (unsigned)p.OW;
      rb[r] = bload1(rB, ok ? ((jbase + oc * OHW + iyt * p.OW + ixt) * 4) : kOOB);
    }
  };
  auto store = [&](int buf) {
    float *const Is = smem + buf * BK * (kIP + kJP), *const Js = Is + BK * kIP;
#pragma unroll
    for (int r = 0; r < kIR; ++r) Is[(ir0 + r * (kNT / BI)) * kIP + tid % BI] = ra[r];
#pragma unroll
    for (int r = 0; r < kJR; ++r) Js[(jr0 + r * (kNT / BJ)) * kJP + tid % BJ] = rb[r];
  };

  f32x16 acc[kTI][kTJ];
#pragma unroll
  for (int a = 0; a < kTI; ++a)
#pragma unroll
    for (int b = 0; b < kTJ; ++b) acc[a][b] = f32x16{0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};

  int const nkt = (K + BK - 1) / BK;
  load(0); store(0);
  __syncthreads();
  for (int t = 0; t < nkt; ++t) {
    if (t + 1 < nkt) load((t + 1) * BK);   // in flight during the MFMAs of step t
    float const *const Is = smem + (t & 1) * BK * (kIP + kJP), *const Js = Is + BK * kIP;
#pragma unroll
    for (int kk = 0; kk < BK / 2; ++kk) {
      int const row = 2 * kk + (lane >> 5);
      float av[kTI], bv[kTJ];
#pragma unroll
      for (int a = 0; a < kTI; ++a) av[a] = Is[row * kIP + wi * (kTI * 32) + a * 32 + (lane & 31)];
#pragma unroll
      for (int b = 0; b < kTJ; ++b) bv[b] = Js[row * kJP + wj * (kTJ * 32) + b * 32 + (lane & 31)];
#pragma unroll
      for (int a = 0; a < kTI; ++a)
#pragma unroll
        for (int b = 0; b < kTJ; ++b) acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[a], bv[b], acc[a][b], 0, 0, 0);
    }
    if (t + 1 < nkt) store((t + 1) & 1);   // the other buffer: every wave finished reading it before the previous barrier
    __syncthreads();
  }

  // ---- epilogue: C/D layout of the 32x32 MFMA family -- column j = lane & 31, row i = 8*(r>>2) + 4*(lane>>5) + (r&3) for register r
#pragma unroll
  for (int b = 0; b < kTJ; ++b) {
    int const j = j0 + wj * (kTJ * 32) + b * 32 + (lane & 31);
    if (j >= P) continue;
    int const img = j / nyx, rem = j - img * nyx, ty = rem / nx, tx = rem - ty * nx;
    long const obase = ((long)img * p.C * p.H + (ry + SY * ty)) * p.W + (rx + SX * tx);
#if ZINP
    // the condition values of this column of blocks, all loaded before its first store (a load issued between stores waits for every earlier store): the same
    // elements the stores below write, so the same bounds and the same coalescing.  A channel past the tensor reads the last channel instead (never stored): an
    // unconditional load, so the loads issue back to back -- a load under its own branch is waited for before the next one is issued
    float zc[kTI][16];
#pragma unroll
    for (int a = 0; a < kTI; ++a)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        int const c = i0 + wi * (kTI * 32) + a * 32 + 8 * (r >> 2) + 4 * (lane >> 5) + (r & 3);
        zc[a][r] = p.zin[obase + (long)(c < p.C ? c : p.C - 1) * p.H * p.W];
      }
    // vmcnt(0) (gfx9 encoding; expcnt / lgkmcnt left at their maxima): every condition value has arrived before the first store.  Left to the compiler, the wait for each
    // value sits in front of its own store, and a vmcnt wait between stores waits for the earlier stores as well
    __builtin_amdgcn_s_waitcnt(0x0F70);
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
