// conv_nhwc_dw_bf16.hip -- a depthwise convolution (group == C == OC, channel multiplier 1) on channels-last bf16 tensors (hip_conv_nhwc_dw), for gfx950; specialised
// by hiprtc.  in img:y:x:chan bf16, filts y:x:chan bf16 (tap-major: F[ky][kx][c] = filts_ref[c][0][ky][kx]), biases float, out img:y:x:chan bf16 or float.
//
// The definition, held to bits.  Per output element, in fp32:
//   acc = +0;  for ky ascending, for kx ascending: acc = fmaf(float(in[img][oy*SY - PY + ky][ox*SX - PX + kx][c]), float(F[ky][kx][c]), acc), a tap in the padding
//   being a product with +0 (for finite filters: the term skipped);  acc = acc + biases[c];  RELU: acc > 0 ? acc : +0;  one round-to-nearest-even to bf16, or none
//   (OUT_F32).  A product of two bf16 values is exact in fp32, so the chain is plain float32 multiplies and adds in the written order.  v_pk_fma_f32 is two such fmas.
//
// There is no reduction over channels: nothing for the matrix cores, two flops per input byte at 3 x 3.  The layer is a stream through HBM, and the work split is made
// for that stream:
//   * a lane owns one 8-channel chunk (16 bytes) of a pel; chunks are the fastest-varying thread index, then x: tid = x * CB + cb.  A wave's global loads and stores
//     are contiguous 16-byte accesses along the tensor's chan-then-x order (whole pels where CB == C8, runs of CB chunks otherwise) -- also at C = 32, four chunks a pel
//   * a workgroup owns one image, a strip of TY output rows, a segment of TX output columns and a block of CB chunks: TX * CB threads
//   * input rows go through an LDS ring of two rows of kIW = (TX-1)*SX + KW columns x CB chunks, each row loaded ONCE, in ascending iy.  Row j+1's global loads are
//     issued (into registers) before row j's arithmetic and stored to the other ring row after it; one barrier a row.  The loads go through a buffer resource: a chunk
//     left of, right of, above or below the plane (or past C8) is read at an offset beyond the resource and comes back as zeros, so the padding IS zeros in the ring
//     and the inner loop has no bounds test per lane
//   * a lane reads its KW chunks of the row from LDS (16-byte reads, columns x*SX + kx: stride 2 in x reads every second column) and feeds EVERY output row the input
//     row reaches: input row j of the strip is tap ky = j - q*SY of the strip's output row q, so ceil(KH / SY) output rows are in flight, each with its own
//     accumulator set (8 floats), slot q mod ceil(KH/SY).  Rows arrive in ascending j, so an output's taps arrive in ascending ky, and kx ascends inside a row: the
//     written order.  The row loop is unrolled over one period SY * ceil(KH/SY) of (tap, slot), so every register index is a constant; which output rows exist
//     (0 <= q < TY) is a wave-uniform test.  Stride 2 in y: two input rows per output row, the same walk
//   * the filters stay in registers as packed bf16, four registers a tap, widened on use (<< 16, & 0xffff0000): a 7 x 7 window is 196 registers, not 392
//   * with the last tap an output row is finished: bias, ReLU, one rounding, one 16-byte store (two for float) per lane, through a buffer resource as well
//
// -D parameters: KNAME C8 CH CW COH COW KH KW SY SX PY PX RELU OUT_F32 TY TX CB.  Host side: plan_conv_nhwc_dw (native_plan.cc), native_kernels_t::conv_nhwc_dw.

#ifndef __HIPCC_RTC__
#include <hip/hip_runtime.h>
#endif
#include "kernel_args.h"      // conv_dw_args_t
#include "device_prelude.h"

constexpr int kOOB = (int)0x80000000;           // byte offset beyond any num_records (tensors are < 2^31 bytes): the hardware returns 0 / drops the store
constexpr int kNT = TX * CB;                    // threads of a workgroup
constexpr int kIW = (TX - 1) * SX + KW;         // input columns of a segment
constexpr int kRowCh = kIW * CB;                // chunks of one ring row
constexpr int kNL = (kRowCh + kNT - 1) / kNT;   // chunks a thread loads per row
constexpr int kNA = (KH + SY - 1) / SY;         // output rows in flight
constexpr int kPer = SY * kNA;                  // the period of (tap, slot) along the strip's input rows
constexpr int kNR = (TY - 1) * SY + KH;         // input rows of a strip
static_assert(KH >= 1 && KH <= 7 && KW >= 1 && KW <= 7 && (SY == 1 || SY == 2) && (SX == 1 || SX == 2) && PY >= 0 && PY < KH && PX >= 0 && PX < KW, "kernels 1..7, strides 1 | 2, padding below the kernel");
static_assert(kNT >= 1 && kNT <= 1024 && CB >= 1 && TY >= 1 && 2 * kRowCh * 16 <= 65536, "workgroup and ring sizes");
constexpr int kWaves = KH * KW <= 9 ? 3 : (KH * KW <= 25 ? 2 : 1);   // waves per SIMD the register budget is held to: what hides the latency of the one-row prefetch

struct chk_t { static constexpr bool value = true; };
struct nochk_t { static constexpr bool value = false; };
__device__ __forceinline__ f32x2 wide2(unsigned w) { return f32x2{__builtin_bit_cast(float, w << 16), __builtin_bit_cast(float, w & 0xffff0000u)}; }   // two bf16 of one word

extern "C" __global__ __launch_bounds__(kNT) __attribute__((amdgpu_waves_per_eu(kWaves))) void KNAME(conv_dw_args_t const p) {
  __shared__ u32x4 ring[2][kRowCh];
  int const tid = threadIdx.x, cb = tid % CB, x = tid / CB;
  int bid = blockIdx.x;
  int const cs = bid % p.n_cs; bid /= p.n_cs;
  int const xs = bid % p.n_xs; bid /= p.n_xs;
  int const ys = bid % p.n_ys, img = bid / p.n_ys;
  int const c = cs * CB + cb, ox = xs * TX + x, oy0 = ys * TY;
  int const iy0 = oy0 * SY - PY, ix0 = xs * TX * SX - PX;     // the strip's first input row / the segment's first input column (negative: padding)
  rsrc_t const rI = make_rsrc(p.in, p.in_bytes), rF = make_rsrc(p.filts, p.f_bytes), rB = make_rsrc(p.bias, (unsigned)(C8 * 32)), rO = make_rsrc(p.out, p.out_bytes);
  bool const has_c = c < C8;

  u32x4 f[KH * KW];                                            // the lane's 8 channels of every tap, packed bf16
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

  // one period of input rows, j = jb .. jb + kPer - 1.  chk: test which rows (j < kNR) and output rows (0 <= q < TY) exist -- wave-uniform tests; the steady periods
  // in the middle of a strip need none and are straight-line code
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
      for (int t = 0; t < KH * KW; ++t) asm volatile("" : "+v"(f[t]));   // (no instruction: the packed filters count as new values here, so their widened forms are not kept across rows)
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
        if (ky == KH - 1) {                                     // the output row's last tap: finish it
          int const oy = oy0 + q;
          float o[8];
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            float s = acc[slot][e >> 1][e & 1] + (e < 4 ? b_lo[e] : b_hi[e - 4]);
            if (RELU) s = (s > 0.f) ? s : 0.f;
            o[e] = s;
          }
          bool const ok = has_c && ox < COW && oy < COH;
          int const pel = ((img * COH + oy) * COW + ox) * C8 + c;   // in chunks
          if (OUT_F32) {
            __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, f32x4{o[0], o[1], o[2], o[3]}), rO, ok ? pel * 32 : kOOB, 0, 0);
            __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, f32x4{o[4], o[5], o[6], o[7]}), rO, ok ? pel * 32 + 16 : kOOB, 0, 0);
          } else {
            bf16x8 h;
#pragma unroll
            for (int e = 0; e < 8; ++e) h[e] = (__bf16)o[e];
            __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, h), rO, ok ? pel * 16 : kOOB, 0, 0);
          }
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

