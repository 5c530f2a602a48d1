// bconv_fb_bf16.hip -- filter AND bias gradient of a convolution in one function call (hip_bconv_filts_biases with hip_operands=bf16): bf16 OPERANDS and fp32 sums for the
// filter gradient, the bias gradient from the unrounded fp32 values, for gfx950; specialised by hiprtc.  Tensors stay fp32 in the reference layouts.  With r(v) = fp32 ->
// bf16 round-to-nearest-even (v_cvt_pk_bf16_f32; inf stays inf, NaN stays NaN):
//
//   filts_grad_loss[oc][c][fy][fx] = sum_{img, oy, ox} r(out_grad_loss[img][oc][oy][ox]) * r(in[img][c][oy*SY - PY + fy][ox*SX - PX + fx])      (fp32 accumulation)
//   biases_grad_loss[oc]           = sum_{img, oy, ox} out_grad_loss[img][oc][oy][ox]                                                         (no rounding)
//
// The GEMM of bconv_fb_f32.hip: D[i = oc][j = (c, fy, fx)] = sum_k I(k, oc) * J(k, j), k = (img, oy, ox) ascending, I = out_grad_loss, J = the input patch, zero outside
// the plane and past K (OOB-zero buffer loads: a select or an OR on the offset, no branch per load), on v_mfma_f32_32x32x16_bf16, WI x WJ waves of 32 x 32 blocks,
// double-buffered LDS.
//
// Staging.  k is the contiguous direction of both operands in memory, and both are loaded with the lanes consecutive along k, as in bconv_fb_f32.hip.  A thread owns TWO
// consecutive k (k pair t % (BK/2)) and the rows / columns t / (BK/2) + r * (threads / (BK/2)): it splits its two k into (img, oy, ox) once per K step, loads two dwords
// per row / column, converts the pair with v_cvt_pk_bf16_f32 and writes it as ONE ds_write_b32 into a [row or column][BK + 8] bf16 image.  The fragments (8 consecutive k
// of one row per lane) are ds_read_b128.
//
// LDS banks.  Pitch (BK + 8) * 2 bytes = (BK/8 + 1) 16-byte slots, odd for BK % 16 == 0.  ds_read_b128: four groups of 16 lanes over 64 banks; a group's 16 rows cover
// every residue mod 16, slot = (row * odd + const) mod 16: conflict-free.  ds_write_b32: two groups of 32 lanes over 32 banks; the lanes of a group are BK/2 consecutive
// dwords of each of 64/BK rows, a row pitch of BK/2 + 4 dwords: BK 64 one row, conflict-free; BK 32 two rows 20 dwords apart, 4 of 32 banks taken twice; BK 16 four rows
// 12 dwords apart, 8 of 32 banks taken twice.  A K step has (BI + BJ) / kG such stores per thread beside its loads and MFMAs; the 2-way part is left as it is.
//
// K slices (SLICED=1, p.ksl = 2..1024): exactly bconv_fb_f32.hip's -- workgroup (tile, s) accumulates K steps [s*kt_per, (s+1)*kt_per) from +0 and writes its raw
// accumulators to slab s of the call's workspace ([OC][C*KH*KW] floats, then OC bias partials); bodahip_bconv_slab_sum (bconv_fb_f32.hip -DSLAB_SUM=1) runs behind it in the
// same call and adds the slabs in slice order, plain fp32 adds.  No tickets, no atomics, no workgroup waits on another.  SLICED=0 (p.ksl = 1) writes the outputs directly.
//
// Filter numerics: products of bf16 values are exact in fp32; the 16 terms inside one MFMA are not a sequential chain, so the order of the fp32 additions inside a slice is
// the instruction's: the result is held to a bound, not to bits, and is the same bits from run to run and from graph replay to eager (fixed by
// (BK, KSL) and the instruction).  The zero terms (borders, K tail) are a * 0 on finite data: the finite-data caveat of the fp32 kernels applies (an inf / NaN operand
// poisons padded terms).  What the bf16 MFMA does with subnormal operands is not stated in the hardware guides and is not tested.
//
// Bias numerics: bit for bit the written chain of the fp32 fused call (tests/bconv_fb_ref.biases_chain(out_grad_loss, BK, KSL)).  The workgroups of the first j tile add
// the fp32 values they loaded, BEFORE rounding, on the VALU: per slice and out_chan BK chains, one per residue a = k % BK, c_a = sum_t I(t*BK + a, oc) over the slice's K
// steps ascending from +0; the slice's partial is ((c_0 + c_1) + c_2) + ... + c_{BK-1}; the partials are added in slice order by the slab sum.
//
// -D parameters: KNAME BI BJ BK WI WJ MINW KH KW SY SX PY PX SLICED.  Host side: plan_bconv_fb_bf16 (native_plan.cc), native_kernels_t::bconv_filts_biases.

#ifndef __HIPCC_RTC__
#include <hip/hip_runtime.h>
#endif
#include "kernel_args.h"      // bconv_fb_args_t
#include "device_prelude.h"

constexpr int kOOB = (int)0x80000000;   // byte offset beyond any num_records (tensors are < 2^31 bytes): the hardware returns 0

constexpr int kNT = WI * WJ * 64;
constexpr int kTI = BI / (WI * 32), kTJ = BJ / (WJ * 32);
constexpr int kH = BK / 2;                    // k pairs of a K step
constexpr int kG = kNT / kH;                  // rows / columns staged side by side
constexpr int kIR = BI / kG, kJR = BJ / kG;   // staged rows / columns per thread (two k each)
constexpr int kP = BK + 8;                    // LDS pitch of the [row][k] images (bf16 elements)
constexpr int kBP = BK + 1;                   // pitch of the bias chains' image (floats), bconv_fb_f32.hip's
constexpr bool kPad = PY != 0 || PX != 0;     // without padding no tap of a valid k leaves the plane: (OH-1)*SY + KH-1 <= H-1
static_assert(BI % (WI * 32) == 0 && BJ % (WJ * 32) == 0 && BK % 16 == 0, "tile: whole 32 x 32 MFMA blocks, K steps of 16");
static_assert(kNT % kH == 0 && BI % kG == 0 && BJ % kG == 0 && BI <= kNT, "staging: every thread owns one k pair and whole rows / columns");
static_assert(BI * kBP * 4 <= 2 * (BI + BJ) * kP * 2, "the bias chains fit the operand images");

extern "C" __global__ __launch_bounds__(WI * WJ * 64, MINW) void KNAME(bconv_fb_args_t const p) {
  __shared__ __attribute__((aligned(16))) __bf16 smem[2 * (BI + BJ) * kP];
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

  // ---- staging roles: k offsets ak, ak + 1; rows i0 + rg + r * kG of I, columns j0 + rg + r * kG of J
  int const ak = 2 * (tid % kH), rg = tid / kH;
  int jo[kJR], jf[kPad ? kJR : 1];   // per column: element offset of (c, fy, fx) in an image, -1 past the last column; (fy, fx) packed for the border test
#pragma unroll
  for (int r = 0; r < kJR; ++r) {
    int const j = j0 + rg + r * kG;
    int const c = j / KHW, f = j - c * KHW, fy = f / KW, fx = f - fy * KW;
    jo[r] = (j < NJ) ? (c * HW + fy * p.W + fx) : -1;
    if (kPad) jf[r] = (fy << 16) | fx;
  }
  float ra[kIR][2], rb[kJR][2], cb[kIR][2];
#pragma unroll
  for (int r = 0; r < kIR; ++r) cb[r][0] = cb[r][1] = 0.f;
  auto load = [&](int k0) {
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      int const k = k0 + ak + u, img = k / OHW, pel = k - img * OHW, oy = pel / p.OW, ox = pel - oy * p.OW;
      int const kmask = (k < K) ? 0 : kOOB;   // OR-ed into every offset of the step: past K everything reads as 0 (no branch per load)
      int const gbase = img * p.OC * OHW + pel;
#pragma unroll
      for (int r = 0; r < kIR; ++r) {
        int const oc = i0 + rg + r * kG;
        ra[r][u] = bload1(rG, ((oc < p.OC) ? ((gbase + oc * OHW) * 4) : kOOB) | kmask);
      }
      int const iy0 = oy * SY - PY, ix0 = ox * SX - PX;
      int const xbase = img * p.C * HW + iy0 * p.W + ix0;
#pragma unroll
      for (int r = 0; r < kJR; ++r) {
        bool ok = jo[r] >= 0;
        if (kPad) ok = ok && (unsigned)(iy0 + (jf[r] >> 16)) < (unsigned)p.H && (unsigned)(ix0 + (jf[r] & 0xffff)) < (unsigned)p.W;
        rb[r][u] = bload1(rX, (ok ? ((xbase + jo[r]) * 4) : kOOB) | kmask);
      }
    }
  };
  auto store = [&](int buf) {
    __bf16 *const Is = smem + buf * (BI + BJ) * kP, *const Js = Is + BI * kP;
#pragma unroll
    for (int r = 0; r < kIR; ++r) { bf16x2 v; v[0] = (__bf16)ra[r][0]; v[1] = (__bf16)ra[r][1]; *reinterpret_cast<bf16x2 *>(Is + (rg + r * kG) * kP + ak) = v; }
#pragma unroll
    for (int r = 0; r < kJR; ++r) { bf16x2 v; v[0] = (__bf16)rb[r][0]; v[1] = (__bf16)rb[r][1]; *reinterpret_cast<bf16x2 *>(Js + (rg + r * kG) * kP + ak) = v; }
    if (do_bias) {   // the bias chains: residues ak, ak + 1 of every out_chan this thread stages, K steps ascending, the UNROUNDED values
#pragma unroll
      for (int r = 0; r < kIR; ++r) { cb[r][0] = cb[r][0] + ra[r][0]; cb[r][1] = cb[r][1] + ra[r][1]; }
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
  int const nkt_all = (K + BK - 1) / BK;
  int const kt0 = min(slice * p.kt_per, nkt_all), kt1 = min(kt0 + p.kt_per, nkt_all);
  if (kt0 < kt1) {   // (workgroup-uniform; an empty slice contributes its zero accumulators)
    load(kt0 * BK); store(0);
    __syncthreads();
    for (int t = kt0; t < kt1; ++t) {
      int const cur = (t - kt0) & 1;
      if (t + 1 < kt1) load((t + 1) * BK);
      __bf16 const *const S = smem + cur * (BI + BJ) * kP;
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

  // ---- the bias partial of the slice: the BK chains of an out_chan side by side in LDS ([out_chan][residue] floats), one thread per out_chan adds them in residue
  // order.  (Every wave is past the K loop's last barrier: the operand images are dead.)
  if (do_bias) {
    float *const fb = reinterpret_cast<float *>(smem);
#pragma unroll
    for (int r = 0; r < kIR; ++r) { fb[(rg + r * kG) * kBP + ak] = cb[r][0]; fb[(rg + r * kG) * kBP + ak + 1] = cb[r][1]; }
    __syncthreads();
    if (tid < BI && i0 + tid < p.OC) {
      float s = fb[tid * kBP];
#pragma unroll
      for (int a = 1; a < BK; ++a) s = s + fb[tid * kBP + a];
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
