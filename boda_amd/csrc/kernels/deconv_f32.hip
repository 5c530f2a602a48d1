// deconv_f32.hip -- a Deconvolution (transposed convolution) and its data and filter gradients (hip_deconv, hip_deconv_bck_in, hip_deconv_bck_filts), fp32, NCHW,
// for gfx950; specialised by hiprtc.  The reference knows the op type and its shapes but has no function for it; the definition is in terms of the BckConv / Convolution
// functions with the operands' roles exchanged.  in is B x C x H x W (the SMALL map), filts C x OC x KH x KW (Caffe's blob: in_chan:out_chan:y:x), out B x OC x OH x OW
// with OH = (H-1)*SY + KH - 2*PY, OW likewise:
//
//   out[img][oc][y][x] = biases[oc] + sum_{c,iy,ix} in[img][c][iy][ix] * filts[c][oc][y + PY - iy*SY][x + PX - ix*SX]     (taps outside the kernel do not exist)
//
// These are the DIRECT forms: no MFMA, one explicit fmaf chain per output in be=cpu's order, only the terms that exist.  They are the forms for the shape family of
// FCN heads -- few channels, large kernels at large strides, outputs of tens of megabytes -- which fills no matrix block and is bound by the output stream.
//
//   FUNC 1  forward = hip_bconv_in on (filts := filts, out_grad_loss := in), then + biases[oc]: per output the reference template's chain
//           (test/rtc/BckConv_in_grad_loss.cucl; be=cpu's bconv_in) from +0 -- c ascending, ix ascending, iy ascending, the filter taps (fy, fx) = (y + PY - iy*SY,
//           x + PX - ix*SX) descending with them, fmaf(in, filt, acc), only the terms that exist -- and ONE fp32 add of the bias as the last operation.  An output no
//           term reaches (a kernel smaller than the stride) is +0 + bias, and it is written.
//           Phase-decomposed as kernels/bconv_in_f32.hip: an output's phase ((y + PY) % SY, (x + PX) % SX) fixes its ceil(KH/SY) x ceil(KW/SX) taps.  A workgroup owns
//           one out_chan, one ROW phase ry and one of ZS chunks of that phase's work; it stages the phase's filter rows fy = ry + SY*t of every in_chan, CC x TY x KW
//           floats, in LDS (21 x 2 x 64 floats = 10.5 KB for FCN's 64/32 head; in_chans in chunks of CC where they do not fit 32 KB -- the chunks are then restaged for every pass of
//           the workgroup over 256 items, correct but a filter fetch that grows with the items: the planner sends wide layers to the matrix path, so only a wide layer
//           at a stride above 16 or a forced direct form gets here), then walks the phase's output rows
//           over all images.  A thread owns four adjacent x of one row: 16-byte stores where OW % 4 == 0.  `in` is read through the caches with buffer loads (a position
//           outside the plane reads as an offset past the buffer and is never used: its term is skipped by a select).  Where the four x share their in column
//           (SX >= 4 and the quad inside one stride step) one read of `in` serves all four.
//   FUNC 2  data gradient = hip_conv on (filts := filts read as out_chan=C:in_chan=OC, biases := +0, in := out_grad_loss), no ReLU: per output (img, c, iy, ix)
//           be=cpu's hip_conv chain from +0 over k = (oc, ky, kx) ascending, OC*KH*KW terms, fmaf(filts[c][oc][ky][kx], out_grad_loss[img][oc][iy*SY - PY + ky]
//           [ix*SX - PX + kx] or +0, acc) -- a padded term is a product with +0 --, then + (+0), the zero bias.  One output per thread; a filter row's loads (a row
//           segment of at most 16 taps) are issued ahead of its part of the chain.
//   FUNC 3  filter gradient = hip_bconv_filts on (in := out_grad_loss, out_grad_loss := in): filts_grad_loss[c][oc][ky][kx] = slab[0] + ... + slab[KSL-1],
//           slab s = one chain fmaf(out_grad_loss[img][oc][iy*SY - PY + ky][ix*SX - PX + kx], in[img][c][iy][ix], acc) from +0 over the terms that exist among the K
//           steps [s*kt_per, (s+1)*kt_per) of BK terms, k = (img, iy, ix) ascending over the SMALL map, clipped to K = B*H*W; a slice that ends in a partial K step takes
//           the K tail's + (+0) (hip_bconv_filts' rule; oracle/bck_chain.filts_sliced_chain); an empty slice is +0.  One (c, oc, ky, kx) per thread and slice, kx
//           fastest: adjacent threads read adjacent out_grad_loss columns and the same `in` element.  KSL = 1 writes the outputs (be=cpu's single chain); with K slices
//           a thread writes its slab to the call's workspace and a second launch in the same stream (FUNC 5) adds the slabs in slice order: no atomics, no tickets.
//   FUNC 5  the slab sum.
//
// -D parameters: KNAME FUNC NIC NOC (in_chans, out_chans) KH KW SY SX PY PX | FUNC 3: BK KSL.  Host side: plan_deconv (native_plan.cc), native_kernels_t::deconv.

#ifndef __HIPCC_RTC__
#include <hip/hip_runtime.h>
#endif
#include "kernel_args.h"      // deconv_args_t
#include "device_prelude.h"

#pragma clang fp contract(off) reassociate(off)

constexpr int kOOB = (int)0x80000000;   // byte offset beyond any num_records (tensors are < 2^31 bytes): the hardware returns 0
constexpr int C = NIC, OC = NOC;        // (the -D names differ from the argument structs' fields C / OC, which kernel_args.h does not shield)
constexpr int kKHW = KH * KW;
constexpr int TY = (KH + SY - 1) / SY, TX = (KW + SX - 1) / SX;   // taps of one phase, per axis

#if FUNC == 1
constexpr int kLdsFloats = 8192;                                  // 32 KB of filter rows
constexpr int kRow = TY * KW;                                     // one in_chan's staged floats
constexpr int CC = (C * kRow <= kLdsFloats) ? C : (kLdsFloats / kRow);
static_assert(CC >= 1, "one in_chan's rows of a phase fit the LDS");
constexpr int kNC = (C + CC - 1) / CC;                            // in_chan chunks

// the terms of one in_chan for the four outputs of a thread.  j / s ascending = iy / ix ascending, the taps descending: iy = qy - (TY-1) + j meets filter row
// ry + SY*(TY-1-j), which is staged row TY-1-j; ix = qx - (TX-1) + s meets column rx + SX*(TX-1-s).  SHARE: the four x have one qx
template <bool SHARE> __device__ __forceinline__ void chan_terms(float (&acc)[4], float const *w, rsrc_t rIn, int plane, int qy, int const (&qx)[4], int const (&rx)[4], int ry, int H, int W) {
  if (SHARE) {
#pragma unroll
    for (int s = 0; s < TX; ++s) {
      int const ix = qx[0] - (TX - 1) + s, fx0 = rx[0] + SX * (TX - 1 - s);
      bool const xok = (unsigned)ix < (unsigned)W;
#pragma unroll
      for (int j = 0; j < TY; ++j) {
        int const iy = qy - (TY - 1) + j;
        bool const ok = xok && (unsigned)iy < (unsigned)H && ry + SY * (TY - 1 - j) < KH;
        float const v = bload1(rIn, ok ? (plane + iy * W + ix) * 4 : kOOB);
        float const *const wr = w + (TY - 1 - j) * KW + fx0;
#pragma unroll
        for (int i = 0; i < 4; ++i) if (ok && fx0 + i < KW) acc[i] = __builtin_fmaf(v, wr[i], acc[i]);
      }
    }
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int s = 0; s < TX; ++s) {
        int const ix = qx[i] - (TX - 1) + s, fx = rx[i] + SX * (TX - 1 - s);
        bool const xok = (unsigned)ix < (unsigned)W && fx < KW;
#pragma unroll
        for (int j = 0; j < TY; ++j) {
          int const iy = qy - (TY - 1) + j;
          bool const ok = xok && (unsigned)iy < (unsigned)H && ry + SY * (TY - 1 - j) < KH;
          float const v = bload1(rIn, ok ? (plane + iy * W + ix) * 4 : kOOB);
          float const wv = w[(TY - 1 - j) * KW + (ok ? fx : 0)];
          if (ok) acc[i] = __builtin_fmaf(v, wv, acc[i]);
        }
      }
  }
}

extern "C" __global__ __launch_bounds__(256) void KNAME(deconv_args_t const p) {
  __shared__ float lw[CC * kRow];
  int bid = (int)blockIdx.x;
  int const zs = bid % p.zs; bid /= p.zs;
  int const ry = bid % SY, oc = bid / SY;
  int const y0 = ((ry - PY) % SY + SY) % SY;                       // the phase's first row
  int const ny = y0 < p.OH ? (p.OH - y0 + SY - 1) / SY : 0, nxq = (p.OW + 3) / 4;
  int const items = p.B * ny * nxq;                                // (img, row of the phase, quad of x)
  int const it0 = min(zs * p.per, items), it1 = min(it0 + p.per, items);
  if (it0 >= it1) return;                                          // (workgroup-uniform)
  rsrc_t const rIn = make_rsrc(p.b, p.b_bytes);
  int const HW = p.H * p.W;
  float const bias = p.bias[oc];
  auto stage = [&](int c0) {   // rows fy = ry + SY*t of in_chans [c0, c0 + CC): lw[cl][t][fx]; a row past the kernel is +0 and never used
    for (int e = (int)threadIdx.x; e < CC * kRow; e += 256) {
      int const cl = e / kRow, r = e - cl * kRow, t = r / KW, fx = r - t * KW, fy = ry + SY * t, c = c0 + cl;
      lw[e] = (c < C && fy < KH) ? p.a[((long)(c * OC + oc) * KH + fy) * KW + fx] : 0.f;
    }
  };
  if (kNC == 1) { stage(0); __syncthreads(); }
  for (int base = it0; base < it1; base += 256) {                  // (workgroup-uniform trip count: the barriers below are met by every thread)
    int const it = base + (int)threadIdx.x;
    bool const live = it < it1;
    int const itc = live ? it : it0;
    int const xq = itc % nxq, r = itc / nxq, q = r % ny, img = r / ny;
    int const y = y0 + q * SY, x0 = xq * 4, qy = (y + PY) / SY;
    int qx[4], rx[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) { qx[i] = (x0 + i + PX) / SX; rx[i] = (x0 + i + PX) - qx[i] * SX; }
    bool const share = qx[0] == qx[3];
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int ch = 0; ch < kNC; ++ch) {
      if (kNC > 1) { __syncthreads(); stage(ch * CC); __syncthreads(); }
      int const cn = min(CC, C - ch * CC);
      int plane = (img * C + ch * CC) * HW;
      if (share) for (int cl = 0; cl < cn; ++cl, plane += HW) chan_terms<true>(acc, lw + cl * kRow, rIn, plane, qy, qx, rx, ry, p.H, p.W);
      else for (int cl = 0; cl < cn; ++cl, plane += HW) chan_terms<false>(acc, lw + cl * kRow, rIn, plane, qy, qx, rx, ry, p.H, p.W);
    }
    if (!live) continue;
    long const o = (((long)img * OC + oc) * p.OH + y) * p.OW + x0;
    float v[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = acc[i] + bias;
    if ((p.OW & 3) == 0) { f32x4 qv; qv[0] = v[0]; qv[1] = v[1]; qv[2] = v[2]; qv[3] = v[3]; *reinterpret_cast<f32x4 *>(p.d + o) = qv; }
    else {
#pragma unroll
      for (int i = 0; i < 4; ++i) if (x0 + i < p.OW) p.d[o + i] = v[i];
    }
  }
}

#elif FUNC == 2
constexpr int kSeg = KW < 16 ? KW : 16;   // taps of a filter row whose loads run ahead of their terms
extern "C" __global__ __launch_bounds__(256) void KNAME(deconv_args_t const p) {
  long const t = (long)blockIdx.x * 256 + threadIdx.x;
  if (t >= p.n) return;
  int const ix = (int)(t % p.W); long r = t / p.W;
  int const iy = (int)(r % p.H); r /= p.H;
  int const c = (int)(r % C), img = (int)(r / C);
  rsrc_t const rG = make_rsrc(p.b, p.b_bytes);
  int const OHW = p.OH * p.OW, Y0 = iy * SY - PY, X0 = ix * SX - PX;
  float const *f = p.a + (long)c * OC * kKHW;
  int gplane = img * OC * OHW;
  float acc = 0.f;
  for (int oc = 0; oc < OC; ++oc, f += kKHW, gplane += OHW) {
#pragma unroll 1
    for (int ky = 0; ky < KH; ++ky) {
      int const Y = Y0 + ky;
      bool const row_ok = (unsigned)Y < (unsigned)p.OH;
      int const rbase = gplane + Y * p.OW + X0;
#pragma unroll
      for (int k0 = 0; k0 < KW; k0 += kSeg) {
        float g[kSeg], w[kSeg];
#pragma unroll
        for (int s = 0; s < kSeg; ++s) {
          int const kx = k0 + s;
          bool const ok = kx < KW && row_ok && (unsigned)(X0 + kx) < (unsigned)p.OW;
          g[s] = bload1(rG, ok ? (rbase + kx) * 4 : kOOB);
          w[s] = kx < KW ? f[ky * KW + kx] : 0.f;
        }
#pragma unroll
        for (int s = 0; s < kSeg; ++s) if (k0 + s < KW) acc = __builtin_fmaf(w[s], g[s], acc);
      }
    }
  }
  p.d[t] = acc + 0.f;   // the zero bias of hip_conv: a -0 becomes +0
}

#elif FUNC == 3
static_assert(KSL >= 1 && KSL <= 1024 && BK >= 1, "K slices: 1..1024");
extern "C" __global__ __launch_bounds__(256) void KNAME(deconv_args_t const p) {
  long const t = (long)blockIdx.x * 256 + threadIdx.x;
  long const s = t / p.n, e = t - s * p.n;                 // the slice; the element of filts_grad_loss (kx fastest)
  if (s >= KSL) return;
  int const kx = (int)(e % KW); long r = e / KW;
  int const ky = (int)(r % KH); r /= KH;
  int const oc = (int)(r % OC), c = (int)(r / OC);
  int const HW = p.H * p.W, OHW = p.OH * p.OW, K = p.B * HW;
  int const nkt = (K + BK - 1) / BK;
  int const kt0 = min((int)s * p.kt_per, nkt), kt1 = min(kt0 + p.kt_per, nkt);
  int const k0 = min(kt0 * BK, K), k1 = min(kt1 * BK, K);
  int img = k0 / HW, pel = k0 - img * HW, iy = pel / p.W, ix = pel - iy * p.W;
  float acc = 0.f;
  for (int k = k0; k < k1; ++k) {
    int const Y = iy * SY - PY + ky, X = ix * SX - PX + kx;
    if ((unsigned)Y < (unsigned)p.OH && (unsigned)X < (unsigned)p.OW)
      acc = __builtin_fmaf(p.a[((long)img * OC + oc) * OHW + Y * p.OW + X], p.b[((long)img * C + c) * HW + iy * p.W + ix], acc);
    if (++ix == p.W) { ix = 0; if (++iy == p.H) { iy = 0; ++img; } }
  }
  if ((k1 - k0) % BK) acc = acc + 0.f;                     // the slice ends in the K tail
  (KSL == 1 ? p.d : p.ws + s * p.n)[e] = acc;
}

#elif FUNC == 5
// the second launch of a sliced filter gradient: one thread per element of filts_grad_loss, slab[0] + slab[1] + ... + slab[ksl-1] in slice order, plain fp32 adds
extern "C" __global__ __launch_bounds__(256) void KNAME(deconv_args_t const p) {
  long const e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= p.n) return;
  float const *const sl = p.ws + e;
  float sum = sl[0];
  for (int q = 1; q < (int)p.ksl; ++q) sum = sum + sl[(long)q * p.n];
  p.d[e] = sum;
}

#else
#error "deconv_f32.hip: -DFUNC=1 | 2 | 3 | 5"
#endif
