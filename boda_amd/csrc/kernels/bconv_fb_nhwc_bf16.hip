// bconv_fb_nhwc_bf16.hip -- filter AND bias gradient of a convolution from channels-last bf16 tensors (hip_bconv_fb_nhwc), for gfx950; specialised by hiprtc.
// in img:y:x:chan (C) and out_grad_loss img:y:x:chan (OC) are bfloat16 as the forward pass leaves them; the outputs are float:
//
//   filts_grad_loss[oc][ky][kx][c] = sum_{b, oy, ox} out_grad_loss[b][oy][ox][oc] * in[b][oy*SY + ky - PY][ox*SX + kx - PX][c]      (fp32 accumulation, exact products)
//   biases_grad_loss[oc]           = sum_{b, oy, ox} float(out_grad_loss[b][oy][ox][oc])
//
// A GEMM per tap: D[i = oc][j = c] = sum_k G(k, i) * X_tap(k, j), k = an output pel, on v_mfma_f32_32x32x16_bf16, WI x WJ waves of kTI x kTJ blocks of 32 x 32.
// Both operands are K-OUTER in memory (a pel's channels are contiguous), so nothing is converted or transposed on the way in:
//
// Staging.  A stage is BK output pels.  1 x 1 kernels (kFlat): BK consecutive pels of the flat (b, oy, ox) order; only the input pels that are used are loaded (stride 2
// skips the others).  Larger kernels: a block of kYB x XB output pels of one image (kYB * XB == BK), and the input goes in as ONE patch of kPH x kPW pels -- the rows and
// columns the block reaches under the TR kernel rows of this workgroup's tap group -- loaded once and read by every tap, padding as zeros.  Rows of both operands go
// into LDS as they lie in memory: 16-byte chunks (8 channels) through registers (OOB-zero buffer loads; a select on the offset, no branch per load), images
// G[k][BI channels] and X[slot][BJ channels], double-buffered.  Ragged OC / C, pels past the plane or past K and the padding are zero ROWS or chunks of these images.
//
// Fragments.  ds_read_b64_tr_b16 (tools/ds_read_tr_probe.py): in a block of 16 lanes, lane t gives the address of 4 consecutive channels -- row t / 4, channels
// 4 * (t % 4) .. + 3 of the block's 16 -- and RECEIVES channel t at the four rows.  Two reads (rows +0 and +4) are the eight k of a lane's MFMA operand: lane l holds
// channel l % 32 at k = 8 * (l / 32) .. + 7, so lanes 0..31 address rows k..k+3 and 32..63 rows k+8..k+11, 64 contiguous bytes of each.  EXEC is all ones at every read
// and every MFMA (no divergent branch around either); what the read does under a partial EXEC was not probed.
//
// LDS banks.  Pitch of an image row: 2 * width bytes, + 64 unless that is 64 mod 128 already (64 | 192 | 320 bytes for 32 | 64 | 128 channels).  A half wave reads 4 rows
// x 64 bytes; with a pitch of 64 mod 128 the four rows start at the four different multiples of 64 mod 256: all 64 banks once.  That holds where consecutive k are
// consecutive slots (G always; X for 1 x 1 kernels and for SX == 1 inside a row of the block); with SX == 2 the rows are two slots apart and pairs of them share banks
// (2-way), as they do where four k cross a row of the block.  The staging writes are 16 bytes per lane, consecutive lanes consecutive chunks of a row.
//
// Accumulators.  A wave keeps one fp32 tile per tap of its group (kTaps = TR * KW tiles of kTI * kTJ * 16 registers) and multiplies ONE G fragment against each tap's
// shifted X fragment: G is read from LDS once per K step.  Taps beyond the kernel's last row (a ragged last group) are computed and not stored.
//
// K slices (SLICED=1, ksl = 2..1024): workgroup (tile, tap group, s) accumulates stages [s * st_per, (s+1) * st_per) from +0 and writes its raw accumulators to slab s
// of the call's workspace (filts_grad_loss's elements in its own layout, then OC bias partials); bodahip_bconv_slab_sum (bconv_fb_f32.hip -DSLAB_SUM=1) adds the slabs in
// slice order behind it.  No tickets, no atomics.  SLICED=0 writes the outputs directly.  Every element of both outputs is written by every call.
//
// Filter numerics: the products are exact in fp32; the order of the additions inside a slice is the instruction's and the stage order, fixed by (BK, XB, KSL): the same
// bits from run to run and from graph replay to eager, held to the bound of DESIGN.md section 3.16.  The zero terms (padding, tails) are a * 0 on finite data: an inf /
// NaN operand poisons the padded terms it meets (the finite-data caveat of section 3.11a).
//
// Bias numerics.  The workgroups of the first j tile and the first tap group add the values they stage, in fp32 on the VALU: thread t owns the 8 channels of chunk
// t % kCI and the image rows t / kCI + n * (kNT / kCI); it adds them stage by stage, n ascending, from +0.  The kNT / kCI chains of a channel are added in ascending
// t / kCI by one thread; the slices' partials in slice order by the slab sum.
//
// -D parameters: KNAME BI BJ BK WI WJ XB TR KH KW SY SX PY PX SLICED.  Host side: plan_bconv_fb_nhwc (native_plan.cc), native_kernels_t::bconv_fb_nhwc.

#ifndef __HIPCC_RTC__
#include <hip/hip_runtime.h>
#endif
#include "kernel_args.h"      // bconv_nhwc_args_t
#include "device_prelude.h"

typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) s16x4 *lds_s16x4_t;

constexpr int kOOB = (int)0x80000000;   // byte offset beyond any num_records (tensors are < 2^31 bytes): the hardware returns 0

constexpr bool kFlat = KH == 1 && KW == 1;
constexpr int kNT = WI * WJ * 64;
constexpr int kTI = BI / (WI * 32), kTJ = BJ / (WJ * 32);
constexpr int kYB = BK / XB;                                  // rows of a stage's block of output pels (kFlat: XB == BK, one row of consecutive pels)
constexpr int kTaps = TR * KW;
constexpr int kSXe = kFlat ? 1 : SX;                          // slots between consecutive k of a block row (kFlat: only the used pels are staged)
constexpr int kPH = kFlat ? 1 : (kYB - 1) * SY + TR, kPW = kFlat ? BK : (XB - 1) * SX + KW;   // the patch, in input pels
constexpr int kSlots = kPH * kPW;
constexpr int kCI = BI / 8, kCJ = BJ / 8;                     // 16-byte chunks of an image row
constexpr int pitch_of(int w) { return 2 * w + ((2 * w) % 128 == 64 ? 0 : 64); }
constexpr int kPI = pitch_of(BI), kPJ = pitch_of(BJ);         // bytes
constexpr int kGBytes = BK * kPI, kBuf = kGBytes + kSlots * kPJ;
constexpr int kNG = (BK * kCI + kNT - 1) / kNT, kNX = (kSlots * kCJ + kNT - 1) / kNT;   // chunks a thread stages per stage
constexpr int kBG = kNT / kCI;                                // bias chains per channel
static_assert(BI % (WI * 32) == 0 && BJ % (WJ * 32) == 0 && BK % 16 == 0 && BK % XB == 0 && (!kFlat || XB == BK), "tile: whole 32 x 32 MFMA blocks, K steps of 16, whole block rows");
static_assert(kNT % kCI == 0 && kBG * BI * 4 <= 2 * kBuf, "bias: a thread owns one chunk column; the chains fit the operand images");
static_assert(TR >= 1 && TR <= KH && kTaps * kTI * kTJ <= 16, "accumulators: at most 256 registers");

extern "C" __global__ __launch_bounds__(WI * WJ * 64) void KNAME(bconv_nhwc_args_t const p) {
  __shared__ __attribute__((aligned(16))) char smem[2 * kBuf];
  int const tid = threadIdx.x, lane = tid & 63;
  int const wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  int const wi = wave / WJ, wj = wave % WJ;
  int bid = (int)blockIdx.x;
  int const slice = bid % p.ksl; bid /= p.ksl;
  int const tg = bid % p.n_tg; bid /= p.n_tg;
  int const tile_i = bid % p.tiles_i, tile_j = bid / p.tiles_i;
  int const i0 = tile_i * BI, j0 = tile_j * BJ, ky0 = tg * TR;
  int const OHW = p.OH * p.OW, K = p.B * OHW;
  int const nxb = (p.OW + XB - 1) / XB, nyb = (p.OH + kYB - 1) / kYB;
  int const n_st = kFlat ? (K + BK - 1) / BK : p.B * nyb * nxb;
  bool const do_bias = tile_j == 0 && tg == 0;   // (workgroup-uniform)
  rsrc_t const rG = make_rsrc(p.g, p.g_bytes), rX = make_rsrc(p.x, p.x_bytes);

  // ---- staging roles: chunk q = tid + n * kNT of an image is chunk q % kC of row / slot q / kC
  int const ci = tid % kCI, cj = tid % kCJ;
  bool const ci_ok = i0 + ci * 8 < p.OC, cj_ok = j0 + cj * 8 < p.C;
  u32x4 rg[kNG], rx[kNX];
  float cb[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) cb[e] = 0.f;
  auto load = [&](int st) {
    int b = 0, oy0 = 0, ox0 = 0;
    if (!kFlat) { b = st / (nyb * nxb); int const r = st - b * nyb * nxb, oyb = r / nxb; oy0 = oyb * kYB; ox0 = (r - oyb * nxb) * XB; }
#pragma unroll
    for (int n = 0; n < kNG; ++n) {
      int const q = tid + n * kNT, row = q / kCI;
      int pel; bool ok = ci_ok && q < BK * kCI;
      if (kFlat) { pel = st * BK + row; ok = ok && pel < K; }
      else { int const oy = oy0 + row / XB, ox = ox0 + row % XB; pel = (b * p.OH + oy) * p.OW + ox; ok = ok && oy < p.OH && ox < p.OW; }
      rg[n] = bload4u(rG, ok ? (pel * p.OC + i0 + ci * 8) * 2 : kOOB);
    }
#pragma unroll
    for (int n = 0; n < kNX; ++n) {
      int const q = tid + n * kNT, slot = q / kCJ;
      int pel; bool ok = cj_ok && q < kSlots * kCJ;
      if (kFlat) {
        int const k = st * BK + slot; ok = ok && k < K;
        if (SY == 1 && SX == 1) pel = k;
        else { int const bb = k / OHW, r = k - bb * OHW, oy = r / p.OW, ox = r - oy * p.OW; pel = (bb * p.H + oy * SY) * p.W + ox * SX; }
      } else {
        int const iy = oy0 * SY - PY + ky0 + slot / kPW, ix = ox0 * SX - PX + slot % kPW;
        pel = (b * p.H + iy) * p.W + ix; ok = ok && (unsigned)iy < (unsigned)p.H && (unsigned)ix < (unsigned)p.W;
      }
      rx[n] = bload4u(rX, ok ? (pel * p.C + j0 + cj * 8) * 2 : kOOB);
    }
  };
  auto store = [&](int buf) {
    char *const Gs = smem + buf * kBuf, *const Xs = Gs + kGBytes;
#pragma unroll
    for (int n = 0; n < kNG; ++n) { int const q = tid + n * kNT; if (q < BK * kCI) *reinterpret_cast<u32x4 *>(Gs + (q / kCI) * kPI + ci * 16) = rg[n]; }
#pragma unroll
    for (int n = 0; n < kNX; ++n) { int const q = tid + n * kNT; if (q < kSlots * kCJ) *reinterpret_cast<u32x4 *>(Xs + (q / kCJ) * kPJ + cj * 16) = rx[n]; }
    if (do_bias) {   // the bias chains: this thread's 8 channels, its rows of the stage in ascending n (rows that were not loaded are +0)
#pragma unroll
      for (int n = 0; n < kNG; ++n)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          cb[2 * e] = cb[2 * e] + __builtin_bit_cast(float, rg[n][e] << 16);
          cb[2 * e + 1] = cb[2 * e + 1] + __builtin_bit_cast(float, rg[n][e] & 0xffff0000u);
        }
    }
  };

  f32x16 acc[kTaps][kTI][kTJ];
#pragma unroll
  for (int t = 0; t < kTaps; ++t)
#pragma unroll
    for (int a = 0; a < kTI; ++a)
#pragma unroll
      for (int b = 0; b < kTJ; ++b)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][a][b][r] = 0.f;

  // ---- fragment addresses (bytes inside a buffer).  The lane's row of a read: 8 * (l / 32) + (l % 16) / 4, + 4 for the second read, + 16 per K step; its channels:
  // 16 * ((l / 16) % 2) + 4 * (l % 4) .. + 3 of a 32-channel block.  G's row k is k itself; X's row is the slot of output pel k of the block (tap 0, 0)
  int const lrow = 8 * (lane >> 5) + ((lane & 15) >> 2), lch = 16 * ((lane >> 4) & 1) + 4 * (lane & 3);
  int const a_off = lrow * kPI + (wi * (kTI * 32) + lch) * 2;
  int x_off[BK / 16][2];
#pragma unroll
  for (int kk = 0; kk < BK / 16; ++kk)
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      int const k = kk * 16 + h * 4 + lrow;
      x_off[kk][h] = kGBytes + ((k / XB) * SY * kPW + (k % XB) * kSXe) * kPJ + (wj * (kTJ * 32) + lch) * 2;
    }
  auto frag = [&](char const *S, int off0, int off1) -> bf16x8 {
    s16x4 const lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_t)(S + off0)), hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_t)(S + off1));
    return __builtin_bit_cast(bf16x8, __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
  };

  int const st0 = min(slice * p.st_per, n_st), st1 = min(st0 + p.st_per, n_st);
  if (st0 < st1) {   // (workgroup-uniform; an empty slice contributes its zero accumulators)
    load(st0); store(0);
    __syncthreads();
    for (int st = st0; st < st1; ++st) {
      int const cur = (st - st0) & 1;
      if (st + 1 < st1) load(st + 1);
      char const *const S = smem + cur * kBuf;
#pragma unroll
      for (int kk = 0; kk < BK / 16; ++kk) {
        bf16x8 av[kTI];
#pragma unroll
        for (int a = 0; a < kTI; ++a) av[a] = frag(S, a_off + (kk * 16) * kPI + a * 64, a_off + (kk * 16 + 4) * kPI + a * 64);
#pragma unroll
        for (int t = 0; t < kTaps; ++t) {
          int const toff = ((t / KW) * kPW + t % KW) * kPJ;   // (compile-time: the tap's shift inside the patch)
          bf16x8 bv[kTJ];
#pragma unroll
          for (int b = 0; b < kTJ; ++b) bv[b] = frag(S, x_off[kk][0] + toff + b * 64, x_off[kk][1] + toff + b * 64);
#pragma unroll
          for (int a = 0; a < kTI; ++a)
#pragma unroll
            for (int b = 0; b < kTJ; ++b) acc[t][a][b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av[a], bv[b], acc[t][a][b], 0, 0, 0);
        }
      }
      if (st + 1 < st1) store(cur ^ 1);
      __syncthreads();
    }
  }

  // ---- where this workgroup writes: the outputs (one slice) or slab `slice`
  long const NF = (long)p.OC * (KH * KW) * p.C;
#if SLICED
  float *const df = p.ws + (long)slice * p.slab_elems, *const db = df + NF;
#else
  float *const df = p.df, *const db = p.db;
#endif

  // ---- the bias partial of the slice: the kBG chains of a channel side by side in LDS ([chain][channel] floats), one thread per channel adds them in chain order.
  // (Every wave is past the K loop's last barrier: the operand images are dead.)
  if (do_bias) {
    float *const fb = reinterpret_cast<float *>(smem);
#pragma unroll
    for (int e = 0; e < 8; ++e) fb[(tid / kCI) * BI + ci * 8 + e] = cb[e];
    __syncthreads();
    if (tid < BI && i0 + tid < p.OC) {
      float s = fb[tid];
#pragma unroll
      for (int r = 1; r < kBG; ++r) s = s + fb[r * BI + tid];
      db[i0 + tid] = s;
    }
  }

  // ---- epilogue: column c = lane & 31 (contiguous in filts_grad_loss), row oc = 8*(r>>2) + 4*(lane>>5) + (r&3) for register r
#pragma unroll
  for (int t = 0; t < kTaps; ++t) {
    int const ky = ky0 + t / KW, kx = t % KW;
    if (ky >= KH) continue;   // (workgroup-uniform: a ragged last tap group)
#pragma unroll
    for (int b = 0; b < kTJ; ++b) {
      int const c = j0 + wj * (kTJ * 32) + b * 32 + (lane & 31);
      if (c >= p.C) continue;
#pragma unroll
      for (int a = 0; a < kTI; ++a)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          int const oc = i0 + wi * (kTI * 32) + a * 32 + 8 * (r >> 2) + 4 * (lane >> 5) + (r & 3);
          if (oc < p.OC) df[((long)(oc * KH + ky) * KW + kx) * p.C + c] = acc[t][a][b][r];
        }
    }
  }
}
