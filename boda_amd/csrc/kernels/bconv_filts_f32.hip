// bconv_filts_f32.hip -- filter and bias gradients of a convolution (BckConv filts_grad_loss / biases_grad_loss), fp32 MFMA, for gfx950; specialised by hiprtc.
//
//   filts_grad_loss[oc][c][fy][fx] = sum_{img, oy, ox} out_grad_loss[img][oc][oy][ox] * in[img][c][oy*SY - PY + fy][ox*SX - PX + fx]
//
// A GEMM D[i = oc][j = (c, fy, fx)] = sum_k I(k, oc) * J(k, j) with k = (img, oy, ox) ascending -- the reference template's order (img, in_y, in_x:
// test/rtc/BckConv_filts_grad_loss.cucl) --, I(k, oc) = out_grad_loss (contiguous along k), J(k, j) = the input patch gathered at stride (SY, SX), zero
// outside the plane (OOB-zero buffer loads).  D is small (out_chan x in_chan*KH*KW) and K long (img*OH*OW), so the K range is cut into KSL slices
// reduced INSIDE the launch, the pattern of conv_nhwc_bf16.hip -DKSL: workgroup (tile, s) accumulates K steps [s*kt_per, (s+1)*kt_per) as one exact MFMA
// chain, writes its raw accumulators write-through to slab s of the tile, drains, and takes ONE relaxed agent-scope ticket; the workgroup that draws the
// tile's last ticket resets it and sums the KSL slabs in slice order.  No float atomics, no workgroup waits on another: run-to-run deterministic, and the
// same bits for every tile shape that cuts K at the same places -- the same slice count AND the same slice length kt_per * BK, with nkt = ceil(K / BK) and
// kt_per = ceil(nkt / KSL) (K = 300, KSL = 3: slices of 128 at BK = 32, of 112 at BK = 16 -- different bits; BI, BJ and the waves never matter).  KSL = 1 is the
// reference template's single sequential chain bit for bit (the skipped border terms are fma(g, 0, acc) on finite data; a NaN / Inf in out_grad_loss makes them
// NaNs inside that out_chan's filter row, and a -0 accumulator becomes +0 under them and under the K tail's fma(0, 0, acc): DESIGN.md section 3.11a); KSL > 1 is a different association:
// result = slab[0] + slab[1] + ... + slab[KSL-1], slab s = the chain from +0 over slice s, an empty slice (kt0 == kt1) a slab of +0.  Both are held to the CPU
// emulation of exactly this (oracle/bck_chain.py) by tests/test_gpu_bck_chain.py.
//
// -DBIAS_ONLY=1: biases_grad_loss[oc] = sum over img, y, x of out_grad_loss -- one workgroup per out_chan, a fixed-order chain per thread (ascending flat
// index, stride 256) and a fixed LDS tree: deterministic.
//
// -D parameters: KNAME BI BJ BK WI WJ MINW KH KW SY SX PY PX KSL | KNAME BIAS_ONLY.  Host side: plan_bconv_filts (native_plan.cc), native_kernels.cc.

#ifndef __HIPCC_RTC__
#include <hip/hip_runtime.h>
#endif
#include "kernel_args.h"      // bconv_args_t
#include "device_prelude.h"

constexpr int kOOB = (int)0x80000000;   // byte offset beyond any num_records (tensors are < 2^31 bytes): the hardware returns 0

#if BIAS_ONLY
extern "C" __global__ __launch_bounds__(256) void KNAME(bconv_args_t const p) {
  __shared__ float red[256];
  int const oc = blockIdx.x, tid = threadIdx.x, OHW = p.OH * p.OW, n = p.B * OHW;
  float s = 0.f;
  for (int e = tid; e < n; e += 256) { int const img = e / OHW; s += p.a[((long)img * p.OC + oc) * OHW + (e - img * OHW)]; }
  red[tid] = s;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) { if (tid < h) red[tid] = red[tid] + red[tid + h]; __syncthreads(); }
  if (tid == 0) p.d[oc] = red[0];
}
#else

constexpr int kNT = WI * WJ * 64;
constexpr int kTI = BI / (WI * 32), kTJ = BJ / (WJ * 32);
constexpr int kIR = BK * BI / kNT, kJR = BK * BJ / kNT;   // staged elements per thread
constexpr int kIP = BI + 4, kJP = BJ + 4;                 // LDS row pitches (floats)
static_assert(BI % (WI * 32) == 0 && BJ % (WJ * 32) == 0 && BK % 2 == 0, "tile: whole 32 x 32 MFMA blocks, K steps of 2");
static_assert(kNT % BK == 0 && kNT % BJ == 0 && (BK * BI) % kNT == 0 && (BK * BJ) % kNT == 0, "staging: every thread owns whole rows / columns");
static_assert(KSL >= 1 && KSL <= 32, "K slices: 1..32");

extern "C" __global__ __launch_bounds__(WI * WJ * 64, MINW) void KNAME(bconv_args_t const p) {
  __shared__ __attribute__((aligned(16))) float smem[2 * BK * (kIP + kJP)];
  int const tid = threadIdx.x, lane = tid & 63;
  int const wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  int const wi = wave / WJ, wj = wave % WJ;
  int const tile_id = (int)blockIdx.x / KSL, slice = (int)blockIdx.x % KSL;
  int const tile_i = tile_id % p.tiles_i, tile_j = tile_id / p.tiles_i;
  int const i0 = tile_i * BI, j0 = tile_j * BJ;
  int const OHW = p.OH * p.OW, HW = p.H * p.W, KHW = KH * KW, NJ = p.C * KHW;
  int const K = p.B * OHW;
  rsrc_t const rA = make_rsrc(p.a, p.a_bytes), rB = make_rsrc(p.b, p.b_bytes);

  // ---- staging roles.  Gradient operand: lane-consecutive along k (contiguous pels), k-offset tid % BK, out_chans tid / BK + r * (kNT / BK).
  //      Input operand: column j = j0 + tid % BJ (fixed (c, fy, fx)), rows tid / BJ + r * (kNT / BJ).
  int const ak = tid % BK, ai0 = i0 + tid / BK;
  int const jl = j0 + tid % BJ, jr0 = tid / BJ;
  bool const j_ok = jl < NJ;
  int jc = 0, jfy = 0, jfx = 0;
  if (j_ok) { jc = jl / KHW; int const f = jl - jc * KHW; jfy = f / KW; jfx = f - jfy * KW; }
  int const jbase = jc * HW + (jfy - PY) * p.W + (jfx - PX);
  float ra[kIR], rb[kJR];
  auto load = [&](int k0) {
    {
      int const k = k0 + ak, img = k / OHW, pel = k - img * OHW;
      int const base = img * p.OC * OHW + pel;
#pragma unroll
      for (int r = 0; r < kIR; ++r) {
        int const oc = ai0 + r * (kNT / BK);
        ra[r] = bload1(rA, (k < K && oc < p.OC) ? ((base + oc * OHW) * 4) : kOOB);
      }
    }
#pragma unroll
    for (int r = 0; r < kJR; ++r) {
      int const k = k0 + jr0 + r * (kNT / BJ), img = k / OHW, pel = k - img * OHW, oy = pel / p.OW, ox = pel - oy * p.OW;
      int const iy = oy * SY - PY + jfy, ix = ox * SX - PX + jfx;
      bool const ok = j_ok && k < K && (unsigned)iy < (unsigned)p.H && (unsigned)ix < (unsigned)p.W;
      rb[r] = bload1(rB, ok ? ((img * p.C * HW + jbase + oy * SY * p.W + ox * SX) * 4) : kOOB);
    }
  };
  auto store = [&](int buf) {
    float *const Is = smem + buf * BK * (kIP + kJP), *const Js = Is + BK * kIP;
#pragma unroll
    for (int r = 0; r < kIR; ++r) Is[ak * kIP + tid / BK + r * (kNT / BK)] = ra[r];
#pragma unroll
    for (int r = 0; r < kJR; ++r) Js[(jr0 + r * (kNT / BJ)) * kJP + tid % BJ] = rb[r];
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
      float const *const Is = smem + cur * BK * (kIP + kJP), *const Js = Is + BK * kIP;
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
      if (t + 1 < kt1) store(cur ^ 1);
      __syncthreads();
    }
  }

#if KSL > 1
  {   // ---- in-launch reduction of the K slices (see the top of this file and conv_nhwc_bf16.hip -DKSL): write-through 16-byte slab stores, every wave drains,
      // barrier, one relaxed agent-scope ticket per workgroup; the last arriver reads the slabs with L1-bypassing loads and sums them in slice order
    constexpr int kQ = kTI * kTJ * 4;            // accumulator quads per thread
    constexpr int kSlabB = kQ * kNT * 16;        // bytes per slab
    rsrc_t const rW = make_rsrc(p.ws + p.ws_slab + (long)tile_id * (long)(KSL * (kSlabB / 4)), (unsigned)(KSL * kSlabB));
    unsigned *const ticket = reinterpret_cast<unsigned *>(p.ws) + tile_id;
#pragma unroll
    for (int a = 0; a < kTI; ++a)
#pragma unroll
      for (int b = 0; b < kTJ; ++b)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          f32x4 v; v[0] = acc[a][b][4 * g]; v[1] = acc[a][b][4 * g + 1]; v[2] = acc[a][b][4 * g + 2]; v[3] = acc[a][b][4 * g + 3];
          __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), rW, slice * kSlabB + (((a * kTJ + b) * 4 + g) * kNT + tid) * 16, 0, 16);
        }
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n s_barrier" ::: "memory");
    unsigned *const flag = reinterpret_cast<unsigned *>(smem);   // (the operand images are dead: every wave is past the K loop's last barrier)
    if (tid == 0) *flag = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n s_barrier" ::: "memory");
    bool const last = (*flag == (unsigned)(KSL - 1));
    if (!last) return;
    if (tid == 0) __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // ready for the next launch / graph replay
#pragma unroll
    for (int a = 0; a < kTI; ++a)
#pragma unroll
      for (int b = 0; b < kTJ; ++b)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          int const o = (((a * kTJ + b) * 4 + g) * kNT + tid) * 16;
          f32x4 sum = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rW, o, 0, 16));
#pragma unroll
          for (int s = 1; s < KSL; ++s) sum += __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rW, s * kSlabB + o, 0, 16));
          acc[a][b][4 * g] = sum[0]; acc[a][b][4 * g + 1] = sum[1]; acc[a][b][4 * g + 2] = sum[2]; acc[a][b][4 * g + 3] = sum[3];
        }
  }
#endif

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
        if (oc < p.OC) p.d[(long)oc * NJ + j] = acc[a][b][r];
      }
  }
}
#endif
