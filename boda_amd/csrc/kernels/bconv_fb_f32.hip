// bconv_fb_f32.hip -- filter AND bias gradient of a convolution in one function call (hip_bconv_filts_biases), fp32 MFMA, both operands staged k-major, for gfx950;
// specialised by hiprtc.
//
//   filts_grad_loss[oc][c][fy][fx] = sum_{img, oy, ox} out_grad_loss[img][oc][oy][ox] * in[img][c][oy*SY - PY + fy][ox*SX - PX + fx]
//   biases_grad_loss[oc]           = sum_{img, oy, ox} out_grad_loss[img][oc][oy][ox]
//
// The GEMM of bconv_filts_f32.hip: D[i = oc][j = (c, fy, fx)] = sum_k I(k, oc) * J(k, j), k = (img, oy, ox) ascending, I = out_grad_loss, J = the input patch, zero
// outside the plane and past K (OOB-zero buffer loads), v_mfma_f32_32x32x2_f32 on WI x WJ waves of 32 x 32 blocks, double-buffered LDS.
//
// Staging.  BOTH operands are loaded with the lanes consecutive along k: thread t owns k offset t % BK and the rows / columns t / BK + r * (threads / BK).  It
// splits its k into (img, oy, ox) ONCE per K step; a column adds its constant (c, fy, fx) offset and, where the layer pads, the border test.  A 1x1 / stride-1 layer
// reads one contiguous run of a channel plane per column, a stride-2 one every other element of a row.  The LDS images are TRANSPOSED, [row or column][k] with the odd
// pitch BK + 1: the k-major stores of a half wave fall on consecutive banks, and the MFMA operand reads (32 rows at one k per half wave) on 32 different banks.
//
// K slices (SLICED=1, p.ksl = 2..1024).  Workgroup (tile, s) accumulates K steps [s*kt_per, (s+1)*kt_per) as one chain from +0 and writes its raw accumulators to slab s
// of the call's workspace, in the layout of the outputs ([OC][C*KH*KW] floats, then OC bias partials).  The second kernel of this file, bodahip_bconv_slab_sum
// (-DSLAB_SUM=1), runs behind it in the same function call: one thread per output element, slab[0] + slab[1] + ... + slab[ksl-1] in slice order, plain fp32 adds.  No
// tickets, no atomics, no workgroup waits on another.  SLICED=0 (p.ksl = 1) writes the outputs directly; there is no second launch.
//
// Filter numerics: oracle/bck_chain.filts_sliced_chain(I, J, BK, KSL) -- nkt = ceil(K / BK), kt_per = ceil(nkt / KSL); slab s = ONE ascending-k fma chain from +0 over
// slice s (an empty slice: +0), result = slab[0] + ... + slab[KSL-1].  Fixed by (BK, KSL); BI, BJ, the waves and who loads what never matter.  The zero terms (borders,
// K tail) are fma(a, 0, acc) = acc on finite data.  KSL = 1 is the reference template's single chain, be=cpu's bits.
//
// Bias numerics (tests/bconv_fb_ref.py is the numpy twin): the workgroups of the first j tile (tile_j == 0) sum the I values they stage anyway, on the VALU.  Per slice
// and out_chan there are BK chains, one per residue a = k % BK:  c_a = sum_t I(t*BK + a, oc)  over the slice's K steps t ascending, from +0, plain adds, terms past K
// being +0.  The slice's partial is ((c_0 + c_1) + c_2) + ... + c_{BK-1}; the partials of the slices are added in slice order by bodahip_bconv_slab_sum like the
// filter slabs (an empty slice: +0).  KSL = 1: the one partial is the result.  Fixed by (BK, KSL) as well.
//
// -D parameters: KNAME BI BJ BK WI WJ MINW KH KW SY SX PY PX SLICED | KNAME SLAB_SUM.  Host side: plan_bconv_filts_biases (native_plan.cc), native_kernels.cc.

#ifndef __HIPCC_RTC__
#include <hip/hip_runtime.h>
#endif
#include "kernel_args.h"      // bconv_fb_args_t
#include "device_prelude.h"

#if SLAB_SUM
extern "C" __global__ __launch_bounds__(256) void KNAME(bconv_fb_args_t const p) {
  long const n = p.slab_elems, nf = n - p.OC;   // a slab: the filter gradient's elements, then the OC bias partials
  long const e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= n) return;
  float const *s = p.ws + e;
  float sum = s[0];
  int i = 1;
  for (; i + 16 <= p.ksl; i += 16) {
    float v[16];
#pragma unroll
    for (int u = 0; u < 16; ++u) v[u] = s[(long)(i + u) * p.slab_elems];
#pragma unroll
    for (int u = 0; u < 16; ++u) sum = sum + v[u];
  }
  for (; i < p.ksl; ++i) sum = sum + s[(long)i * p.slab_elems];
  if (e < nf) p.df[e] = sum; else p.db[e - nf] = sum;
}
#else

constexpr int kOOB = (int)0x80000000;   // byte offset beyond any num_records (tensors are < 2^31 bytes): the hardware returns 0

constexpr int kNT = WI * WJ * 64;
constexpr int kTI = BI / (WI * 32), kTJ = BJ / (WJ * 32);
constexpr int kG = kNT / BK;                  // rows / columns staged side by side
constexpr int kIR = BI / kG, kJR = BJ / kG;   // staged elements per thread
constexpr int kP = BK + 1;                    // LDS pitch of the transposed images (floats): odd
constexpr bool kPad = PY != 0 || PX != 0;     // without padding no tap of a valid k leaves the plane: (OH-1)*SY + KH-1 <= H-1
static_assert(BI % (WI * 32) == 0 && BJ % (WJ * 32) == 0 && BK % 2 == 0, "tile: whole 32 x 32 MFMA blocks, K steps of 2");
static_assert(kNT % BK == 0 && BI % kG == 0 && BJ % kG == 0 && BI <= kNT, "staging: every thread owns one k offset and whole rows / columns");

extern "C" __global__ __launch_bounds__(WI * WJ * 64, MINW) void KNAME(bconv_fb_args_t const p) {
  __shared__ float smem[2 * (BI + BJ) * kP];
  int const tid = threadIdx.x, lane = tid & 63;
  int const wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  int const wi = wave / WJ, wj = wave % WJ;
  int const tile_id = (int)blockIdx.x / p.ksl, slice = (int)blockIdx.x % p.ksl;
  int const tile_i = tile_id % p.tiles_i, tile_j = tile_id / p.tiles_i;
  int const i0 = tile_i * BI, j0 = tile_j * BJ;
  int const OHW = p.OH * p.OW, HW = p.H * p.W, KHW = KH * KW, NJ = p.C * KHW;
  int const K = p.B * OHW;
  bool const do_bias = tile_j == 0;   // (workgroup-uniform)
  rsrc_t const rG = make_rsrc(p.g, p.g_bytes), rX = make_rsrc(p.x, p.x_bytes);

  // ---- staging roles: k offset ak, rows i0 + rg + r * kG of I, columns j0 + rg + r * kG of J
  int const ak = tid % BK, rg = tid / BK;
  int jo[kJR], jf[kPad ? kJR : 1];   // per column: element offset of (c, fy, fx) in an image, -1 past the last column; (fy, fx) packed for the border test
#pragma unroll
  for (int r = 0; r < kJR; ++r) {
    int const j = j0 + rg + r * kG;
    int const c = j / KHW, f = j - c * KHW, fy = f / KW, fx = f - fy * KW;
    jo[r] = (j < NJ) ? (c * HW + fy * p.W + fx) : -1;
    if (kPad) jf[r] = (fy << 16) | fx;
  }
  float ra[kIR], rb[kJR], cb[kIR];
#pragma unroll
  for (int r = 0; r < kIR; ++r) cb[r] = 0.f;
  auto load = [&](int k0) {
    int const k = k0 + ak, img = k / OHW, pel = k - img * OHW, oy = pel / p.OW, ox = pel - oy * p.OW;
    int const kmask = (k < K) ? 0 : kOOB;   // OR-ed into every offset of the step: past K everything reads as 0 (no branch per load)
    int const gbase = img * p.OC * OHW + pel;
#pragma unroll
    for (int r = 0; r < kIR; ++r) {
      int const oc = i0 + rg + r * kG;
      ra[r] = bload1(rG, ((oc < p.OC) ? ((gbase + oc * OHW) * 4) : kOOB) | kmask);
    }
    int const iy0 = oy * SY - PY, ix0 = ox * SX - PX;
    int const xbase = img * p.C * HW + iy0 * p.W + ix0;
#pragma unroll
    for (int r = 0; r < kJR; ++r) {
      bool ok = jo[r] >= 0;
      if (kPad) ok = ok && (unsigned)(iy0 + (jf[r] >> 16)) < (unsigned)p.H && (unsigned)(ix0 + (jf[r] & 0xffff)) < (unsigned)p.W;
      rb[r] = bload1(rX, (ok ? ((xbase + jo[r]) * 4) : kOOB) | kmask);
    }
  };
  auto store = [&](int buf) {
    float *const Is = smem + buf * (BI + BJ) * kP, *const Js = Is + BI * kP;
#pragma unroll
    for (int r = 0; r < kIR; ++r) Is[(rg + r * kG) * kP + ak] = ra[r];
#pragma unroll
    for (int r = 0; r < kJR; ++r) Js[(rg + r * kG) * kP + ak] = rb[r];
    if (do_bias) {   // the bias chains: residue ak of every out_chan this thread stages, K steps ascending
#pragma unroll
      for (int r = 0; r < kIR; ++r) cb[r] = cb[r] + ra[r];
    }
  };

  f32x16 acc[kTI][kTJ];
#pragma unroll
  for (int a = 0; a < kTI; ++a)
#pragma unroll
    for (int b = 0; b < kTJ; ++b) acc[a][b] = f32x16{0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};

  int const nkt_all = (K + BK - 1) / BK;
  int const kt0 = min(slice * p.kt_per, nkt_all), kt1 = min(kt0 + p.kt_per, nkt_all);
  if (kt0 < kt1) {   // (workgroup-uniform; an empty slice contributes its zero accumulators)
    load(kt0 * BK); store(0);
    __syncthreads();
    for (int t = kt0; t < kt1; ++t) {
      int const cur = (t - kt0) & 1;
      if (t + 1 < kt1) load((t + 1) * BK);
      float const *const Is = smem + cur * (BI + BJ) * kP + (wi * (kTI * 32) + (lane & 31)) * kP + (lane >> 5);
      float const *const Js = smem + cur * (BI + BJ) * kP + (BI + wj * (kTJ * 32) + (lane & 31)) * kP + (lane >> 5);
#pragma unroll
      for (int kk = 0; kk < BK / 2; ++kk) {
        float av[kTI], bv[kTJ];
#pragma unroll
        for (int a = 0; a < kTI; ++a) av[a] = Is[a * 32 * kP + 2 * kk];
#pragma unroll
        for (int b = 0; b < kTJ; ++b) bv[b] = Js[b * 32 * kP + 2 * kk];
#pragma unroll
        for (int a = 0; a < kTI; ++a)
#pragma unroll
          for (int b = 0; b < kTJ; ++b) acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[a], bv[b], acc[a][b], 0, 0, 0);
      }
      if (t + 1 < kt1) store(cur ^ 1);
      __syncthreads();
    }
  }

  // ---- where this workgroup writes: the outputs (one slice) or slab `slice`
#if SLICED
  float *const df = p.ws + (long)slice * p.slab_elems, *const db = df + (long)p.OC * NJ;
#else
  float *const df = p.df, *const db = p.db;
#endif

  // ---- the bias partial of the slice: the BK chains of an out_chan side by side in LDS ([out_chan][residue], the I image's layout), one thread per out_chan adds them
  // in residue order.  (Every wave is past the K loop's last barrier: the operand images are dead.)
  if (do_bias) {
#pragma unroll
    for (int r = 0; r < kIR; ++r) smem[(rg + r * kG) * kP + ak] = cb[r];
    __syncthreads();
    if (tid < BI && i0 + tid < p.OC) {
      float s = smem[tid * kP];
#pragma unroll
      for (int a = 1; a < BK; ++a) s = s + smem[tid * kP + a];
      db[i0 + tid] = s;
    }
  }

  // ---- epilogue: column j = lane & 31 (contiguous in filts_grad_loss), row i = 8*(r>>2) + 4*(lane>>5) + (r&3) for register r
#pragma unroll
  for (int b = 0; b < kTJ; ++b) {
    int const j = j0 + wj * (kTJ * 32) + b * 32 + (lane & 31);
    if (j >= NJ) continue;
#pragma unroll
    for (int a = 0; a < kTI; ++a)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        int const oc = i0 + wi * (kTI * 32) + a * 32 + 8 * (r >> 2) + 4 * (lane >> 5) + (r & 3);
        if (oc < p.OC) df[(long)oc * NJ + j] = acc[a][b][r];
      }
  }
}
#endif
