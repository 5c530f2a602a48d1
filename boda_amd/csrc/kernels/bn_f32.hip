// bn_f32.hip -- the training BatchNorm of the gradient pipe and the Eltwise-SUM gradient, fp32, reference layout (img:chan:y:x), for gfx950; specialised by hiprtc
// (-DOP=<n> picks the kernel).  This backend's own arithmetic: the reference names the op types BatchNorm / Scale / Eltwise but never ran them and has no training
// BatchNorm.  It is pinned by the formulas below and held bit for bit between be=hip, be=cpu (csrc/cpu_compute.cc) and a numpy twin (tests/bn_ref.py).
//
// Every operation below is ONE fp32 rounding, in the order written; the file is compiled with contraction and reassociation off, the divide and the square root are
// the correctly rounded ones.  Per channel c, N = img * y * x, fN = (float)N.
//
//   hip_bn_stats     in -> mean, inv_std; run_mean, run_var rewritten in place.  eps, maf ride in the op
//       mean = S1 / fN,  S1 = SUM x
//       var  = S2 / fN,  S2 = SUM (x - mean) * (x - mean)          (two passes, the biased variance)
//       inv_std = 1 / sqrtf(var + eps)
//       run_mean' = maf * run_mean + omm * mean                     omm = 1 - maf, formed once on the host in fp32
//       run_var'  = maf * run_var  + omm * (var * unb)              unb = fN / (float)(N - 1), formed once on the host in fp32; N == 1: var itself, no multiply
//   hip_bn_fwd       in, mean, inv_std, scale, bias -> out (may be in's buffer).  relu rides in the op
//       xh = (x - mean[c]) * inv_std[c];  y = xh * scale[c] + bias[c]   (a multiply, then an add);  relu=1: y > 0 ? y : +0
//   hip_bn_bck_sums  in, mean, inv_std, out_grad_loss -> scale_grad_loss, bias_grad_loss
//       scale_grad_loss = SUM dy * xh,  bias_grad_loss = SUM dy,  xh recomputed exactly as above
//   hip_bn_bck_in    in, mean, inv_std, scale, scale_grad_loss, bias_grad_loss, out_grad_loss -> in_grad_loss (may be out_grad_loss's buffer)
//       k = scale[c] * inv_std[c];  mb = bias_grad_loss[c] / fN;  mg = scale_grad_loss[c] / fN;  dx = k * ((dy - mb) - xh * mg)
//   hip_fan_out      in -> outs_0 .. outs_{n-1}, 2 <= n <= 8: every outs_i = in bit for bit, in read once
// BatchNorm ON THE RUNNING PAIR (fine-tuning with frozen statistics): the statistics are constants of the step, so the data gradient loses its
// two mean terms and the running pair is only read.  hip_bn_fwd is the forward pass as it is, on hip_bnf_prep's outputs
//   hip_bnf_prep     run_mean, run_var -> mean, inv_std.  eps rides in the op
//       mean = run_mean (the bits);  ve = run_var + eps;  sd = sqrtf(ve);  inv_std = 1 / sd          (the arithmetic of the finalising step of hip_bn_stats)
//   hip_bnf_bck      in, mean, inv_std, scale, out_grad_loss -> in_grad_loss (may be out_grad_loss's buffer), scale_grad_loss, bias_grad_loss
//       scale_grad_loss = SUM dy * xh,  bias_grad_loss = SUM dy: the chain of hip_bn_bck_sums, term for term -- the same bits on the same mean / inv_std
//       k = scale[c] * inv_std[c];  dx = k * dy, stored by the thread that owns the element in that chain: ONE pass over in and out_grad_loss
//   hip_bnf_bck_in   inv_std, scale, out_grad_loss -> in_grad_loss (may be out_grad_loss's buffer):  k = scale[c] * inv_std[c];  dx = k * dy.  Reads no `in`
//
// THE ORDER OF THE THREE SUMS (S1, S2, and the pair of hip_bn_bck_sums) is this chain, the same on every backend, run to run, whatever the dispatch order:
//   * a channel's elements are numbered e = img * HW + pel, 0 <= e < N.  Slab s holds e in [s * slab, min(N, (s + 1) * slab)); slab (a multiple of 4) and the slab
//     count come from bn_slab_plan (csrc/rtc_types.h), a function of the op alone -- dims and a forced slab length --, never of the device
//   * inside a slab the elements are numbered r = e - s * slab.  Chain t (0 <= t < 256) owns the elements with (r / 4) mod 256 == t and adds their terms to +0 one by one
//     in ascending r:  a = +0;  a = a + term(r0);  a = a + term(r1); ...   A chain without elements stays +0
//   * the 256 chains meet in a fixed tree: for h = 128, 64, .. 1:  a[t] = a[t] + a[t + h] for t < h.  a[0] is the slab's partial P_s
//   * the channel's sum is ((P_0 + P_1) + P_2) + ..., in slab order STARTING FROM P_0
//   One workgroup owns one (channel, slab); thread t is chain t.  P_s goes to a per-call workspace ([2][chan][slab] floats); the NEXT launch of the same call reads
//   it -- the launch boundary is the hand-off: no tickets, no flags, no atomics.  hip_bn_stats is three launches (S1 partials; S2 partials, every workgroup re-adding
//   the channel's S1 partials in slab order to get mean; the finalising step, one thread per channel), hip_bn_bck_sums two.
//
// Loads: QUADS (set by the host where HW is a multiple of 4 and every tensor pointer is 16-byte aligned; uniform over the launch): a chain's four elements are one
// 16-byte load, up to four such loads per tensor are issued before the first use.  Otherwise the element path: the same ownership, scalar loads, four in flight.
// The element-wise kernels follow bodahip_chan_affine: a thread owns one quad of a plane or one element, loads everything before it stores, writes nothing else.
//
// THE CHUNKED CHAIN (hip_bnc_stats, hip_bnc_bck_sums): the batch is cut into img chunks, chunk i = images [T * i / n, T * (i + 1) / n).  Inside a
// chunk the elements are numbered from the chunk's first image, the slab plan is the plan of the chunk's own dims, and the rules above give the chunk total D_i; the
// channel's sum is ((D_a + D_b) + D_c) + ... over the non-empty chunks in ascending order STARTING FROM the first.  fN, unb, the N == 1 case and the mean of S2's terms
// are the whole batch's.  One chunk is the chain above.  Its forms: MODE=3, the S2 partials with mean[c] read from memory (the mean of the WHOLE batch, which the cross-
// chunk step of S1 wrote); FIN=4, a chunk total (one sum's slab partials in slab order -> one value per channel); XCH=1, the cross-chunk step: the totals [chunk][2][C]
// added in chunk order, then FIN=3 (mean = S1 / fN alone), FIN=1 (the finalising arithmetic below, verbatim) or FIN=2 (the raw pair).  On several devices chunk i is
// device i's shard; the totals are copied between the launches, no kernel reads another device's memory.
//
// -D parameters: KNAME OP, then  1: MODE (0 S1, 1 S2, 2 the bck_sums pair, 3 S2 with mean from memory), DX (MODE 2 only: 1 = hip_bnf_bck, the owner also stores dx) | 2: FIN (1 stats, 2 bck_sums, 3 mean alone, 4 one raw sum), XCH | 3: RELU | 5: NOUT.
// Host side: bn_slab_plan / bn_op_of_op (rtc_types.h), plan_bn (native_plan.cc), native_kernels_t::bn_call (native_kernels.cc), the argument checks in native_run.cc.

#ifndef __HIPCC_RTC__
#include <hip/hip_runtime.h>
#endif

#pragma clang fp contract(off) reassociate(off)

#include "kernel_args.h"      // bn_args_t
#include "device_prelude.h"

#if OP == 1
#ifndef DX
#define DX 0
#endif
#if DX && MODE != 2
#error "bn_f32.hip: DX=1 is a form of MODE=2"
#endif
#if MODE == 2
#define NSUM 2
#else
#define NSUM 1
#endif
#if MODE == 0
#define TERM(x, d) { a0 = a0 + (x); }
#elif MODE == 1 || MODE == 3
#define TERM(x, d) { float const df = (x) - mean; float const sq = df * df; a0 = a0 + sq; }
#else
#define TERM(x, d) { float const df = (x) - mean; float const xh = df * istd; float const tm = (d) * xh; a0 = a0 + tm; a1 = a1 + (d); }
#endif
extern "C" __global__ __launch_bounds__(256) void KNAME(bn_args_t const p) {
  __shared__ float red[NSUM][256];
  int const tid = threadIdx.x;
  int const c = (int)(blockIdx.x / (unsigned)p.nslabs), s = (int)(blockIdx.x - (unsigned)c * (unsigned)p.nslabs);
  if (c >= p.C) return;   // (never: the grid is C * nslabs)
  int const e0 = s * p.slab;
  int const len = (p.N - e0 < p.slab) ? p.N - e0 : p.slab;
  int const nq = (len + 3) >> 2;   // quads of the slab, the last one ragged on the element path only
#if MODE == 1
  float const *const w1p = p.ws + (long)c * p.nslabs;
  float S1 = w1p[0];
  for (int i = 1; i < p.nslabs; ++i) S1 = S1 + w1p[i];
  float const mean = S1 / p.fN;
#elif MODE == 2
  float const mean = p.c0[c], istd = p.c1[c];
#if DX
  float const kk = p.c2[c] * istd;
#endif
#elif MODE == 3
  float const mean = p.c0[c];
#endif
  int img, pel;
  { int const e = e0 + 4 * tid; img = e / p.HW; pel = e - img * p.HW; }   // (this chain's first element; may lie behind the slab: then q < nq fails below)
  float a0 = 0.0f;
#if NSUM == 2
  float a1 = 0.0f;
#endif
  if (p.quads) {
    for (int q = tid; q < nq; q += 1024) {
      f32x4 X[4];
#if MODE == 2
      f32x4 D[4];
#endif
#if DX
      long O[4];
#endif
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (q + 256 * k < nq) {
          long const off = ((long)img * p.C + c) * p.HW + pel;
          X[k] = *(f32x4 const *)(p.in + off);
#if MODE == 2
          D[k] = *(f32x4 const *)(p.dy + off);
#endif
#if DX
          O[k] = off;
#endif
        }
        pel += p.step_pel; img += p.step_img;
        if (pel >= p.HW) { pel -= p.HW; ++img; }
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (q + 256 * k < nq) {
#if MODE == 2
          TERM(X[k].x, D[k].x) TERM(X[k].y, D[k].y) TERM(X[k].z, D[k].z) TERM(X[k].w, D[k].w)
#if DX
          // THE IN-PLACE STORE (out may be dy's buffer).  Element e of channel c belongs to exactly one (channel, slab) workgroup and there to exactly one chain, this
          // thread: nobody else loads or stores it, in this launch or in the FIN launch behind it.  All of this round's loads of this thread (the loop above) are issued
          // before this store, and a later round touches other elements: the store can neither race with a load of dy[e] nor be read back
          f32x4 v; v.x = kk * D[k].x; v.y = kk * D[k].y; v.z = kk * D[k].z; v.w = kk * D[k].w;
          *(f32x4 *)(p.out + O[k]) = v;
#endif
#else
          TERM(X[k].x, 0) TERM(X[k].y, 0) TERM(X[k].z, 0) TERM(X[k].w, 0)
#endif
        }
      }
    }
  } else {
    for (int q = tid; q < nq; q += 256) {
      float X[4];
#if MODE == 2
      float D[4];
#endif
#if DX
      long O[4];
#endif
      int const r = 4 * q;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (r + j < len) {
          int pj = pel + j, ij = img;
          while (pj >= p.HW) { pj -= p.HW; ++ij; }
          long const off = ((long)ij * p.C + c) * p.HW + pj;
          X[j] = p.in[off];
#if MODE == 2
          D[j] = p.dy[off];
#endif
#if DX
          O[j] = off;
#endif
        }
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (r + j < len) {
#if MODE == 2
          TERM(X[j], D[j])
#if DX
          p.out[O[j]] = kk * D[j];   // (the same ownership: element r + j of the slab is this chain's alone, and its four loads of the round came first)
#endif
#else
          TERM(X[j], 0)
#endif
        }
      }
      pel += p.step_pel; img += p.step_img;
      if (pel >= p.HW) { pel -= p.HW; ++img; }
    }
  }
  red[0][tid] = a0;
#if NSUM == 2
  red[1][tid] = a1;
#endif
  __syncthreads();
#pragma unroll
  for (int h = 128; h > 0; h >>= 1) {
    if (tid < h) {
      red[0][tid] = red[0][tid] + red[0][tid + h];
#if NSUM == 2
      red[1][tid] = red[1][tid] + red[1][tid + h];
#endif
    }
    __syncthreads();
  }
  if (tid == 0) {
    long const slot = (long)c * p.nslabs + s;
#if MODE == 1
    p.ws[(long)p.C * p.nslabs + slot] = red[0][0];
#else
    p.ws[slot] = red[0][0];
#endif
#if NSUM == 2
    p.ws[(long)p.C * p.nslabs + slot] = red[1][0];
#endif
  }
}

#elif OP == 2
#ifndef XCH
#define XCH 0
#endif
extern "C" __global__ __launch_bounds__(256) void KNAME(bn_args_t const p) {
  int const c = (int)(blockIdx.x * 256 + threadIdx.x);   // one owner per channel
  if (c >= p.C) return;
#if XCH   // the cross-chunk step: p.ws holds the totals [chunk][2][C] of the nslabs non-empty chunks, in chunk order
  float const *const pa = p.ws + c;
  long const st = 2L * p.C;
#if FIN == 3
  float A = pa[0];
  for (int i = 1; i < p.nslabs; ++i) A = A + pa[i * st];
#else
  float const *const pb = pa + p.C;
  float A = pa[0], Bv = pb[0];
  for (int i = 1; i < p.nslabs; ++i) { A = A + pa[i * st]; Bv = Bv + pb[i * st]; }
#endif
#elif FIN == 4   // a chunk total: one sum's slab partials
  float const *const pa = p.ws + (long)c * p.nslabs;
  float A = pa[0];
  for (int i = 1; i < p.nslabs; ++i) A = A + pa[i];
#else
  float const *const pa = p.ws + (long)c * p.nslabs;
  float const *const pb = pa + (long)p.C * p.nslabs;
  float A = pa[0], Bv = pb[0];
  for (int i = 1; i < p.nslabs; ++i) { A = A + pa[i]; Bv = Bv + pb[i]; }
#endif
#if FIN == 1
  float const mean = A / p.fN;
  float const var = Bv / p.fN;
  float const ve = var + p.eps;
  float const sd = sqrtf(ve);
  float const istd = 1.0f / sd;
  float const rm = p.w2[c], rv = p.w3[c];   // (read before anything of this channel is written)
  float const m1 = p.maf * rm;
  float const m2 = p.omm * mean;
  float const uv = (p.N == 1) ? var : var * p.unb;
  float const v1 = p.maf * rv;
  float const v2 = p.omm * uv;
  p.w0[c] = mean; p.w1[c] = istd;
  p.w2[c] = m1 + m2; p.w3[c] = v1 + v2;
#elif FIN == 3
  p.w0[c] = A / p.fN;
#elif FIN == 4
  p.w0[c] = A;
#else
  p.w0[c] = A; p.w1[c] = Bv;
#endif
}

#elif OP == 3 || OP == 4
#if OP == 3
struct chan_t { float mean, istd, sc, bi; };
__device__ __forceinline__ float bn1(float x, float, chan_t const &k) {
  float const df = x - k.mean;
  float const xh = df * k.istd;
  float v = xh * k.sc;
  v = v + k.bi;
#if RELU
  v = v > 0.0f ? v : 0.0f;
#endif
  return v;
}
#else
struct chan_t { float mean, istd, k, mb, mg; };
__device__ __forceinline__ float bn1(float x, float dy, chan_t const &k) {
  float const df = x - k.mean;
  float const xh = df * k.istd;
  float const t1 = dy - k.mb;
  float const t2 = xh * k.mg;
  float const t3 = t1 - t2;
  return k.k * t3;
}
#endif
extern "C" __global__ __launch_bounds__(256) void KNAME(bn_args_t const p) {
  long const id = (long)blockIdx.x * 256 + threadIdx.x;   // (plane, unit of the plane): `quads` quads, then HW - 4 quads single elements
  if (id >= p.n) return;
  int const units = p.quads + (p.HW - 4 * p.quads);
  long const plane = id / units;
  int const u = (int)(id - plane * units);
  int const c = (int)(plane % p.C);
  chan_t k;
  k.mean = p.c0[c]; k.istd = p.c1[c];
#if OP == 3
  k.sc = p.c2[c]; k.bi = p.c3[c];
#else
  k.k = p.c2[c] * k.istd;
  k.mg = p.c3[c] / p.fN;
  k.mb = p.c4[c] / p.fN;
#endif
  long const base = plane * p.HW;
  if (u < p.quads) {
    f32x4 const x = ((f32x4 const *)(p.in + base))[u];
#if OP == 4
    f32x4 const d = ((f32x4 const *)(p.dy + base))[u];
#else
    f32x4 const d = x;
#endif
    f32x4 v;
    v.x = bn1(x.x, d.x, k); v.y = bn1(x.y, d.y, k); v.z = bn1(x.z, d.z, k); v.w = bn1(x.w, d.w, k);
    ((f32x4 *)(p.out + base))[u] = v;
  } else {
    long const e = base + 4L * p.quads + (u - p.quads);
    float const x = p.in[e];
#if OP == 4
    float const d = p.dy[e];
#else
    float const d = x;
#endif
    p.out[e] = bn1(x, d, k);
  }
}

#elif OP == 5
extern "C" __global__ __launch_bounds__(256) void KNAME(bn_args_t const p) {
  long const id = (long)blockIdx.x * 256 + threadIdx.x;   // `quads` quads of the flat tensor, then the tail's single elements
  if (id >= p.n) return;
  if (id < p.quads) {
    f32x4 const v = ((f32x4 const *)p.in)[id];
#pragma unroll
    for (int i = 0; i < NOUT; ++i) ((f32x4 *)p.outs[i])[id] = v;
  } else {
    long const e = 4L * p.quads + (id - p.quads);
    float const v = p.in[e];
#pragma unroll
    for (int i = 0; i < NOUT; ++i) p.outs[i][e] = v;
  }
}

#elif OP == 6
extern "C" __global__ __launch_bounds__(256) void KNAME(bn_args_t const p) {
  int const c = (int)(blockIdx.x * 256 + threadIdx.x);   // one owner per channel; c0 / c1 = the running pair, only read
  if (c >= p.C) return;
  float const rm = p.c0[c], rv = p.c1[c];
  float const ve = rv + p.eps;
  float const sd = sqrtf(ve);
  p.w0[c] = rm; p.w1[c] = 1.0f / sd;
}

#elif OP == 7
extern "C" __global__ __launch_bounds__(256) void KNAME(bn_args_t const p) {
  long const id = (long)blockIdx.x * 256 + threadIdx.x;   // (plane, unit of the plane) as for OP 3 / 4; c0 = inv_std, c1 = scale
  if (id >= p.n) return;
  int const units = p.quads + (p.HW - 4 * p.quads);
  long const plane = id / units;
  int const u = (int)(id - plane * units);
  int const c = (int)(plane % p.C);
  float const kk = p.c1[c] * p.c0[c];
  long const base = plane * p.HW;
  if (u < p.quads) {   // (out may be dy's buffer: this thread alone loads and stores this quad, the load first)
    f32x4 const d = ((f32x4 const *)(p.dy + base))[u];
    f32x4 v;
    v.x = kk * d.x; v.y = kk * d.y; v.z = kk * d.z; v.w = kk * d.w;
    ((f32x4 *)(p.out + base))[u] = v;
  } else {
    long const e = base + 4L * p.quads + (u - p.quads);
    float const d = p.dy[e];
    p.out[e] = kk * d;
  }
}

#else
#error "bn_f32.hip: -DOP=1..7"
#endif
