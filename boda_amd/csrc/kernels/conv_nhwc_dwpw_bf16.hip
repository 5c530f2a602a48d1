// conv_nhwc_dwpw_bf16.hip -- a depthwise convolution and the 1x1 convolution that alone reads it, as ONE launch on channels-last bf16 tensors (hip_conv_nhwc_dw_pw),
// for gfx950; specialised by hiprtc.  in img:y:x:chan bf16; filts y:x:chan bf16 (tap-major, as conv_nhwc_dw_bf16.hip), biases float; filts2 out_chan:1:1:in_chan
// bf16, biases2 float; out img:y:x:chan (NOC channels) bf16 or float.  The depthwise layer's output never reaches memory.
//
// The definition, per output pel:
//   t[c]    = the chain of conv_nhwc_dw_bf16.hip bit for bit: fp32 acc = +0; for ky, then kx ascending acc = fmaf(in, F[ky][kx][c], acc), a padded tap a product with
//             +0; + biases[c]; RELU: acc > 0 ? acc : +0; ONE round-to-nearest-even to bf16 (the intermediate is bf16, as it is between the two calls)
//   out[oc] = sum_c t[c] * F2[oc][c] accumulated in fp32 by v_mfma_f32_32x32x16_bf16 from +0, + biases2[oc]; RELU2; one rounding to bf16, or none (OUT_F32)
//
// The work split.  A workgroup owns one image, TY output rows x TX output columns -- P = TY * TX pels, kPP = P rounded up to 32 -- and ALL out_chans, so the depthwise
// work is done once per pel.  Its LDS holds the depthwise ring and the tile T[kPP][C] of t in bf16, pel-major, at a pitch of an ODD number of 16-byte chunks
// (C/8 rounded up to even, + 1): the 16-byte fragment reads of phase B, 32 consecutive pels at one chunk index, fall into different bank groups.
//   Phase A (every thread tid < TX * CB; lane = (column x, chunk cb), chunk fastest): the depthwise layer exactly as conv_nhwc_dw_bf16.hip walks it -- the
//     (TY-1)*SY + KH input rows of the tile pass once through a two-row ring, loaded through a buffer resource so that the padding arrives as zeros, each row feeding
//     every output row it reaches from rolling fp32 accumulators -- once per block of CB chunks, the blocks visited in turn.  A finished output row is rounded and
//     written to T instead of to memory.  With C % 16 == 8 the last K step reads one chunk past the channels: that chunk of every pel is zeroed up front (garbage
//     there times a zero filter would be a NaN).  The rows of the pels P .. kPP-1 stay as they are: an MFMA column depends on its own pel only and those are not stored
//   Phase B (every wave): the units (32-out_chan block, group of kPG pel tiles of 32) are dealt round-robin to the waves.  For a unit the wave loops K over C in steps
//     of 16: the filter fragment -- 8 consecutive in_chans of out_chan 32 ob + (lane & 31), chunk 2 ks + (lane >> 5) -- is one 16-byte global load through a buffer
//     resource (past NOC or C: zeros), prefetched kFR steps ahead through a register ring; the pel fragments are 16-byte LDS reads of T.  out_chan is the MFMA row
//     axis, so a lane ends with four consecutive out_chans of one pel per accumulator quad: + biases2, RELU2, one 8-byte (bf16) or 16-byte (float) store through a
//     buffer resource; ragged out_chan blocks, ragged pels and pels past the plane are masked there.
// One launch, no workspace, no atomics.
//
// -D parameters: KNAME C8 NOC CH CW COH COW KH KW SY SX PY PX RELU RELU2 OUT_F32 TY TX CB.  Host side: plan_conv_nhwc_dwpw (native_plan.cc),
// native_kernels_t::conv_nhwc_dwpw.

#ifndef __HIPCC_RTC__
#include <hip/hip_runtime.h>
#endif
#include "kernel_args.h"      // conv_dwpw_args_t
#include "device_prelude.h"

constexpr int kOOB = (int)0x80000000;           // byte offset beyond any num_records (tensors are < 2^31 bytes): the hardware returns 0 / drops the store
constexpr int kNA_T = TX * CB;                  // threads of phase A
constexpr int kNT = (kNA_T + 63) / 64 * 64;     // threads of the workgroup: whole waves
constexpr int kNW = kNT / 64;
constexpr int kIW = (TX - 1) * SX + KW;         // input columns of a segment
constexpr int kRowCh = kIW * CB;                // chunks of one ring row
constexpr int kNL = (kRowCh + kNT - 1) / kNT;   // chunks a thread loads per row
constexpr int kNA = (KH + SY - 1) / SY;         // output rows in flight
constexpr int kPer = SY * kNA;                  // the period of (tap, slot) along the tile's input rows
constexpr int kNR = (TY - 1) * SY + KH;         // input rows of a tile
constexpr int kNCB = (C8 + CB - 1) / CB;        // chunk blocks
constexpr int kP = TY * TX, kPT = (kP + 31) / 32, kPP = kPT * 32;   // pels, pel tiles of 32, padded pels
constexpr int kKS = (C8 + 1) / 2;               // K steps of 16 channels
constexpr int kPitch = 2 * kKS + 1;             // chunks per pel of T: odd
constexpr int kOCB = (NOC + 31) / 32;            // out_chan blocks
constexpr int kPG0 = kPT * kOCB / kNW, kPG = kPG0 < 1 ? 1 : (kPG0 > 4 ? 4 : (kPG0 > kPT ? kPT : kPG0));   // pel tiles of a unit: as many as keep every wave busy, at most 4
constexpr int kNPG = (kPT + kPG - 1) / kPG;     // pel-tile groups
constexpr int kFR = 4;                          // filter fragments in flight
static_assert(KH >= 1 && KH <= 5 && KW >= 1 && KW <= 5 && (SY == 1 || SY == 2) && (SX == 1 || SX == 2) && PY >= 0 && PY < KH && PX >= 0 && PX < KW, "kernels 1..5, strides 1 | 2, padding below the kernel");
static_assert(kNA_T >= 1 && kNT <= 1024 && CB >= 1 && CB <= C8 && TY >= 1 && C8 <= 128 && NOC % 8 == 0 && kPT <= 8, "workgroup, channel and tile sizes");
static_assert((2 * kRowCh + kPP * kPitch) * 16 <= 160 * 1024, "ring + T within the LDS");

struct chk_t { static constexpr bool value = true; };
struct nochk_t { static constexpr bool value = false; };
__device__ __forceinline__ f32x2 wide2(unsigned w) { return f32x2{__builtin_bit_cast(float, w << 16), __builtin_bit_cast(float, w & 0xffff0000u)}; }   // two bf16 of one word

extern "C" __global__ __launch_bounds__(kNT) void KNAME(conv_dwpw_args_t const p) {
  __shared__ u32x4 ring[2][kRowCh];
  __shared__ u32x4 T[kPP * kPitch];
  int const tid = threadIdx.x;
  bool const act = tid < kNA_T;                                // (the tail of the last wave only loads ring rows in phase A)
  int const cb = act ? tid % CB : 0, x = act ? tid / CB : 0;
  int bid = blockIdx.x;
  int const xs = bid % p.n_xs; bid /= p.n_xs;
  int const ys = bid % p.n_ys, img = bid / p.n_ys;
  int const ox0 = xs * TX, oy0 = ys * TY;
  int const iy0 = oy0 * SY - PY, ix0 = ox0 * SX - PX;          // the tile's first input row / column (negative: padding)
  rsrc_t const rI = make_rsrc(p.in, p.in_bytes), rF = make_rsrc(p.filts, p.f_bytes), rB = make_rsrc(p.bias, (unsigned)(C8 * 32));
  rsrc_t const rF2 = make_rsrc(p.filts2, p.f2_bytes), rB2 = make_rsrc(p.bias2, (unsigned)(NOC * 4)), rO = make_rsrc(p.out, p.out_bytes);

  if (C8 & 1)                                                  // the K tail: chunk C8 of every pel is read by the last K step
    for (int s = tid; s < kPP; s += kNT) T[s * kPitch + C8] = u32x4{0u, 0u, 0u, 0u};

  // ---- phase A: the depthwise layer, chunk block by chunk block, into T
  for (int cs = 0; cs < kNCB; ++cs) {
    int const c = cs * CB + cb;
    bool const has_c = c < C8;
    u32x4 f[KH * KW];                                          // the lane's 8 channels of every tap, packed bf16
#pragma unroll
    for (int t = 0; t < KH * KW; ++t) f[t] = bload4u(rF, has_c ? (t * C8 + c) * 16 : kOOB);
    f32x4 const b_lo = bload4(rB, has_c ? c * 32 : kOOB), b_hi = bload4(rB, has_c ? c * 32 + 16 : kOOB);

    // ring row j: the chunks (xi, cbl) of input row iy0 + j, this thread's being tid, tid + kNT, ...
    auto load_row = [&](int j, u32x4 (&dst)[kNL]) {
      int const iy = iy0 + j;
      bool const row_ok = iy >= 0 && iy < CH;
      int const row_off = ((img * CH + iy) * CW + ix0) * C8 + cs * CB;   // in chunks
#pragma unroll
      for (int l = 0; l < kNL; ++l) {
        int const s = tid + l * kNT, xi = s / CB, cbl = s % CB, ix = ix0 + xi;
        bool const ok = row_ok && s < kRowCh && ix >= 0 && ix < CW && cs * CB + cbl < C8;
        dst[l] = bload4u(rI, ok ? (row_off + xi * C8 + cbl) * 16 : kOOB);
      }
    };
    auto store_row = [&](int slot, u32x4 const (&src)[kNL]) {
#pragma unroll
      for (int l = 0; l < kNL; ++l) { int const s = tid + l * kNT; if (kRowCh % kNT == 0 || s < kRowCh) ring[slot][s] = src[l]; }
    };

    u32x4 nxt[kNL];
    load_row(0, nxt); store_row(0, nxt);
    __syncthreads();

    f32x2 acc[kNA][4];
#pragma unroll
    for (int a = 0; a < kNA; ++a)
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[a][e] = f32x2{0.f, 0.f};

    // one period of input rows, j = jb .. jb + kPer - 1.  chk: test which rows (j < kNR) and output rows (0 <= q < TY) exist -- uniform tests
    auto period = [&](int jb, auto chk) {
      constexpr bool kChk = decltype(chk)::value;
#pragma unroll
      for (int r = 0; r < kPer; ++r) {
        int const j = jb + r;
        if (kChk && j >= kNR) break;
        if (!kChk || j + 1 < kNR) load_row(j + 1, nxt);           // in flight during this row's arithmetic
        u32x4 v[KW];
#pragma unroll
        for (int kx = 0; kx < KW; ++kx) v[kx] = ring[j & 1][(x * SX + kx) * CB + cb];
#pragma unroll
        for (int ky = 0; ky < KH; ++ky) {
          if ((r - ky) % SY != 0) continue;                       // (constant after unrolling: this input row is no tap ky of any output row)
          int const dq = (r - ky) / SY;                           // exact; q = jb / SY + dq, and jb / SY is a multiple of kNA
          int const slot = ((dq % kNA) + kNA) % kNA;
          int const q = jb / SY + dq;
          if (kChk && !(q >= 0 && q < TY)) continue;
#pragma unroll
          for (int kx = 0; kx < KW; ++kx) {
            u32x4 const w = f[ky * KW + kx];
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[slot][e] = __builtin_elementwise_fma(wide2(v[kx][e]), wide2(w[e]), acc[slot][e]);
          }
          if (ky == KH - 1) {                                     // the output row's last tap: finish it into T
            bf16x8 h;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
              float s = acc[slot][e >> 1][e & 1] + (e < 4 ? b_lo[e] : b_hi[e - 4]);
              if (RELU) s = (s > 0.f) ? s : 0.f;
              h[e] = (__bf16)s;
            }
            if (act && has_c) T[(q * TX + x) * kPitch + c] = __builtin_bit_cast(u32x4, h);
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[slot][e] = f32x2{0.f, 0.f};
          }
        }
        if (!kChk || j + 1 < kNR) store_row((j + 1) & 1, nxt);
        __syncthreads();
      }
    };
    // steady: every q of the period exists (jb / SY - (kNA - 1) >= 0 and jb / SY + kNA <= TY) and so does every row and its successor (jb + kPer < kNR)
    constexpr int kSteady0 = kPer, kSteadyEnd = (TY - kNA) * SY < kNR - kPer ? (TY - kNA) * SY : kNR - kPer - 1;   // steady periods start at jb in [kSteady0, kSteadyEnd]
    period(0, chk_t{});
    int jb = kPer;
    for (; jb >= kSteady0 && jb <= kSteadyEnd; jb += kPer) period(jb, nochk_t{});
    for (; jb < kNR; jb += kPer) period(jb, chk_t{});
  }
  __syncthreads();                                             // T is whole

  // ---- phase B: out[pel][oc] = T[pel][:] . F2[oc][:] on the matrix cores
  int const lane = tid & 63, wave = tid >> 6, l31 = lane & 31, lhi = lane >> 5;
  for (int u = wave; u < kOCB * kNPG; u += kNW) {
    int const ob = u / kNPG, pt0 = (u % kNPG) * kPG;
    int const oc_f = ob * 32 + l31;                            // the out_chan whose filter row this lane fetches
    auto load_f = [&](int ks) { int const ch = 2 * ks + lhi; return bload4u(rF2, (ks < kKS && oc_f < NOC && ch < C8) ? (oc_f * C8 + ch) * 16 : kOOB); };
    u32x4 fr[kFR];
#pragma unroll
    for (int i = 0; i < kFR; ++i) fr[i] = load_f(i);
    f32x16 acc[kPG];
#pragma unroll
    for (int g = 0; g < kPG; ++g)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[g][r] = 0.f;
    for (int ks0 = 0; ks0 < kKS; ks0 += kFR) {
#pragma unroll
      for (int i = 0; i < kFR; ++i) {
        int const ks = ks0 + i;
        bf16x8 const a = __builtin_bit_cast(bf16x8, fr[i]);
        fr[i] = load_f(ks + kFR);
        if (ks < kKS) {
#pragma unroll
          for (int g = 0; g < kPG; ++g)
            if (kPT % kPG == 0 || pt0 + g < kPT)
              acc[g] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, __builtin_bit_cast(bf16x8, T[((pt0 + g) * 32 + l31) * kPitch + 2 * ks + lhi]), acc[g], 0, 0, 0);
        }
      }
    }
    // accumulator r of a lane: out_chan 32 ob + 8 (r / 4) + 4 lhi + r % 4, pel 32 (pt0 + g) + l31
#pragma unroll
    for (int g = 0; g < kPG; ++g) {
      if (!(kPT % kPG == 0 || pt0 + g < kPT)) continue;
      int const pel = (pt0 + g) * 32 + l31, q = pel / TX, oy = oy0 + q, ox = ox0 + pel % TX;
      bool const pel_ok = pel < kP && oy < COH && ox < COW;
      int const o_pel = ((img * COH + oy) * COW + ox) * NOC;    // in elements
#pragma unroll
      for (int rq = 0; rq < 4; ++rq) {
        int const oc = ob * 32 + 8 * rq + 4 * lhi;
        bool const ok = pel_ok && oc < NOC;                      // (NOC % 8 == 0: a quad is whole or absent)
        f32x4 const b2 = bload4(rB2, oc < NOC ? oc * 4 : kOOB);
        f32x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) { float s = acc[g][rq * 4 + e] + b2[e]; if (RELU2) s = (s > 0.f) ? s : 0.f; o[e] = s; }
        if (OUT_F32) __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, o), rO, ok ? (o_pel + oc) * 4 : kOOB, 0, 0);
        else {
          bf16x4 h;
#pragma unroll
          for (int e = 0; e < 4; ++e) h[e] = (__bf16)o[e];
          __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, h), rO, ok ? (o_pel + oc) * 2 : kOOB, 0, 0);
        }
      }
    }
  }
}
