// bck_ops_f32.hip -- the non-conv ops of the gradient pipe, fp32, reference layouts (img:chan:y:x), for gfx950; specialised by hiprtc (-DOP=<n> picks the kernel).
// All of them are bandwidth kernels: one thread per written element (x fastest, so a wave stores whole lines), gathers from a handful of neighbouring lines,
// no atomics -- every output element has one owner, which is what makes the results the same bits run to run.
//
// The semantics are the reference templates', quirks included (parity is the contract); every kernel keeps the WRITTEN order of its fp32 operations: the
// file is compiled with contraction and reassociation off, so a*b + c stays two roundings, and it calls the real powf / expf / logf.
//
// OP 1  bodahip_pool_yx  (test/rtc/pool.cucl with emit_out_in_yx=1)   in -> out, out_in_yx
//   * AVG=1 (an average pooling of the gradient pipe): the taps inside the plane are summed from +0 in the same order and divided by their NUMBER (the window
//     clipped by the border); out_in_yx is -1 everywhere, what the template leaves for an average.  The rest describes AVG=0
//   * padding pels never take part; taps are visited kx OUTER, ky inner
//   * the maximum starts at -FLT_MAX and is replaced on strict `>`: the FIRST maximal tap in that order wins a tie (and a NaN never wins)
//   * out_in_yx is a FLOAT holding in_y*W + in_x of the winning tap, or -1 when no tap won (a window of -FLT_MAX / NaN only, or one wholly in the padding)
// OP 2  bodahip_spreading  (test/rtc/spreading.cucl)   out_grad_loss, out_in_yx -> in_grad_loss   (the template's `out` arg is never read)
//   * one value per in_grad_loss pel: the outputs whose window holds it are out_x in [max(0, x+pad-k+s)/s, min((x+pad)/s + 1, OW)), likewise y
//   * out_x OUTER, out_y inner, a sequential fp32 sum from +0 (a pel no window holds is exactly +0)
//   * max (AVG=0): add out_grad_loss where out_in_yx == y*W + x (compared as floats);  average (AVG=1): add out_grad_loss / (KH*KW) -- the FULL window area
//     even where the window is clipped by a border, as the reference does (its own FIXME says so); a division per term, not a multiplication by 1/area
//   * ZINP=1 (the function op's zero_if_in_non_pos): the ReLU gradient that follows this call in a gradient pipe, folded into the store -- in_grad_loss = in > 0 ? v : +0
//     with `in` (p3) the pooling's forward input at the written pel: OP 5's rule with cond = in, a select on the finished sum (a +0, -0 or NaN condition gives +0)
// OP 3  bodahip_lrn_sb  (test/rtc/lrn.cucl, the caffe-matching path, emit_out_scale_base=1)   in -> out, out_scale_base
//   * scale_base = k + ls_sum * (alpha / local_size), the quotient formed once in fp32 on the host
//   * ls_sum is CARRIED along the channels of a pel as (ls_sum + new*new) - old*old, in that order; its bits depend on the whole history from channel 0, so a
//     thread that owns channels [c0, c0 + CB) first walks channels 0 .. c0 - 1 updating only the sum (loads that its neighbours' walks keep in the caches)
//   * out = in * powf(scale_base, -beta)
// OP 4  bodahip_bck_lrn  (test/rtc/bck_lrn.cucl, the #else branch)   in, out, out_grad_loss, out_scale_base -> in_grad_loss
//   * t[c] = out_grad_loss[c] * out[c] / scale_base[c], zero outside the tensor, kept in a ring of local_size slots, slot = channel mod local_size
//   * ls_sum is RECOMPUTED for every channel from +0 over the ring in SLOT order i = 0 .. local_size-1 (not in channel order, and not carried)
//   * in_grad_loss = out_grad_loss * powf(scale_base, -beta) + in * ls_sum * coef,  coef = ((2 * -beta) * alpha) / local_size formed once in fp32 on the host
//   * a thread owns CB channels of a pel; its walk starts at a multiple of local_size at or below c0 - local_size/2, so every ring slot is a compile-time index
//   * ZINP=1: in_grad_loss = in > 0 ? (the value above) : +0 -- the same fold as OP 2's, on the `in` value the formula has loaded already
// OP 5  bodahip_zero_if_non_pos  (test/rtc/ZeroIfNonPos.cucl)   out = cond > 0 ? in : 0.0f -- the code's `>` (the reference's comment says >=); +0, -0 and NaN
//   conditions give +0.  float4 over the first n4 quads, scalars over the tail.
// OP 6  bodahip_softmax  (test/rtc/softmax.cucl, 1 x 1 planes)   in -> prob
//   * pel_max starts at 0.0f, not at the first value: the shift is max(0, max in), so an all-negative row is NOT shifted to its maximum
//   * prob = expf(in - pel_max) / sum.  One WAVE per image: lane l takes channels l, l + 64, ...; its part of the sum is a sequential chain in that order, the 64
//     parts meet in a fixed xor butterfly (32, 16, .. 1), so every lane holds the same bits and two runs give the same bits.  This is a different summation
//     order than the reference's single chain (be=cpu keeps that one); the test bound allows any order.
// OP 7  bodahip_sm_grad_and_loss  (test/rtc/sm_grad_and_loss.cucl)   prob, label -> in_grad_loss, loss_per_pel
//   * label is a FLOAT holding the class index, read by image; in_grad_loss = (prob - [chan == label]) / img_count: an fp32 subtract, then an fp32 divide
//   * loss_per_pel = -logf(max(prob[label], FLT_MIN)); a label outside [0, chan) matches no channel and reads no memory: its loss is -logf(FLT_MIN)
//   * B is read only as that divisor, the threads are counted by n: on an img shard of a batch (the function op's img_shards=1 on a multi-device backend) the host
//     passes the WHOLE batch's image count as B and the shard's elements as n -- the same kernel, the one-device bits
// OP 8  bodahip_sum_loss_over_imgs  (test/rtc/sum_loss_over_imgs.cucl)   loss = (sequential fp32 sum of loss_per_pel over the images from +0) / img_count: one thread
// OP 9  bodahip_reduce  (test/rtc/reduce.cucl, the sum of a fan-out's partial gradients)   ins_0 .. ins_{NIN-1} -> out
//   * out[i] = (((+0 + ins_0[i]) + ins_1[i]) + ...): a sequential fp32 chain from +0 in the op's input order, so two -0 inputs give +0
// OP 10 bodahip_dropout  (test/rtc/dropout.cucl; the gradient of dropout is the same dropout)   inout, in place
//   * h = (uint32)flat index + seed (wraps), then h ^= h >> 16; h *= 0x85ebca6b; h ^= h >> 13; h *= 0xc2b2ae35; h ^= h >> 16
//   * inout = h > thresh ? inout * scale : +0;  thresh = (uint32)((float)0xffffffff * ratio) and scale = (float)(1 / (1 - (double)ratio)) come from the host;
//     the seed is a run-time argument: a new seed is no new specialisation
//   * SEEDVAR=1 (the function op's seed_from_var): seed = *p4 + p.seed (a uint32 wrap-around add), p4 one uint32 word in device memory that every thread
//     loads from the same address -- a captured launch (hipGraph) freezes p.seed but not the word, so every replay can drop other elements.  With word w and
//     by-value o the bits are those of the plain kernel under the seed (w + o) mod 2^32; without the define the kernel is the plain one
// OP 11 bodahip_concat / OP 12 bodahip_split  (the reference's copy calls, src/rtc_fwd.cc:267-294)   in -> out: an img:chan:y:x tensor copied into (11) / out of (12)
//   the channel range [cix, cix + chan) of a wider one.  Per image that range is one run of `run` = chan * y * x consecutive floats, `wide` = the wider tensor's
//   floats per image, `off` = cix * y * x
// OP 13 bodahip_chan_affine  (this backend's own: an inference BatchNorm / Scale run of the forward pipe, conv_pipe.fold_affine)   in, a, b -> out
//   * out[i,c,y,x] = in[i,c,y,x] * a[c] + b[c]: an fp32 multiply, then an fp32 add, two roundings; RELU=1 (the op's relu): x > 0 ? x : +0 on that sum, so -0 and a NaN give +0
//   * a thread owns one quad or one tail element of one plane, loads before it stores and touches nothing else: in and out may be the same buffer
//   * n4 counts the float4 quads of ONE plane here (0 unless both pointers are 16-byte aligned and HW is a multiple of 4), the elements behind them are scalars
// OP 14 bodahip_shard_sum  (this backend's own: the sum of the per-shard partial gradients of a multi-device backend, csrc/hip_multi.cc)   B slabs -> out
//   * slab d holds n floats at p0 + d * wide (wide: the slab stride in floats); out[e] = ((slab_0[e] + slab_1[e]) + slab_2[e]) + ...: plain fp32 adds in slab order that
//     START FROM slab 0's value -- no +0 in front, so one slab is a copy and keeps a -0
//   * the slab count is a loop bound: one specialisation for every device count.  A thread owns one quad or one tail element, reads it from every slab and then
//     stores: out may be slab 0.  n4 = 0 unless p0, out and the stride are all 16-byte aligned
// OP 15 bodahip_crop / OP 16 bodahip_crop_bck  (this backend's own: Caffe's Crop at axis 2 and its gradient)   in -> out  /  out_grad_loss -> in_grad_loss
//   * out[i,c,y,x] = in[i,c,y + PY,x + PX]: the OH x OW window at offset (PY, PX) of the H x W plane; one thread per window element
//   * in_grad_loss[i,c,y,x] = out_grad_loss[i,c,y - PY,x - PX] inside the window and +0 outside it: one thread per plane element, every element written
// OP 9 .. 12 take float4 over the first n4 quads and scalars over the tail, like OP 5; the host sets n4 = 0 unless every pointer (11, 12: every per-image run) is
// 16-byte aligned.  Quads never straddle a run: 11 / 12 use them only when run, wide and off are multiples of 4.
//
// -D parameters: KNAME OP, then  1, 2: H W OH OW KH KW SY SX PY PX AVG | 3, 4: LS CB | 9: NIN | 2, 4: [ZINP] | 10: [SEEDVAR] | 13: RELU | 14: none | 15, 16: H W OH OW PY PX.  Host side: plan_bck_op / plan_shard_sum (native_plan.cc), native_kernels.cc.

#ifndef __HIPCC_RTC__
#include <hip/hip_runtime.h>
#endif

#pragma clang fp contract(off) reassociate(off)
#ifndef ZINP
#define ZINP 0
#endif
#ifndef SEEDVAR
#define SEEDVAR 0
#endif

#include "kernel_args.h"      // bck_ops_args_t
#include "device_prelude.h"

constexpr float kFltMax = 3.402823466e+38f, kFltMin = 1.175494351e-38f;

#if OP == 1
extern "C" __global__ __launch_bounds__(256) void KNAME(bck_ops_args_t const p) {
  long const id = (long)blockIdx.x * 256 + threadIdx.x;
  if (id >= p.n) return;
  int const ox = (int)(id % OW), oy = (int)((id / OW) % OH);
  long const plane = id / (OW * OH);
  float const *const in = p.p0 + plane * (H * W);
#if AVG
  float best = 0.0f, cnt = 0.0f; int const oyx = -1;
#else
  float best = -kFltMax; int oyx = -1;
#endif
#pragma unroll
  for (int kx = 0; kx < KW; ++kx) {
#pragma unroll
    for (int ky = 0; ky < KH; ++ky) {
      int const iy = oy * SY + ky - PY, ix = ox * SX + kx - PX;
      if (iy >= 0 && ix >= 0 && ix < W && iy < H) {
        float const v = in[iy * W + ix];
#if AVG
        best = best + v; cnt = cnt + 1.0f;
#else
        if (v > best) { best = v; oyx = iy * W + ix; }
#endif
      }
    }
  }
#if AVG
  best = best / cnt;
#endif
  p.o0[id] = best;
  p.o1[id] = (float)oyx;
}

#elif OP == 2
constexpr int kMaxX = (KW + SX - 1) / SX, kMaxY = (KH + SY - 1) / SY;   // the most windows that hold one pel, per axis
extern "C" __global__ __launch_bounds__(256) void KNAME(bck_ops_args_t const p) {
  long const id = (long)blockIdx.x * 256 + threadIdx.x;
  if (id >= p.n) return;
  int const x = (int)(id % W), y = (int)((id / W) % H);
  long const plane = id / (W * H);
  float const *const ogl = p.p1 + plane * (OH * OW);
  float const *const oiyx = p.p2 + plane * (OH * OW);
  int const xt = x + PX - KW + SX, yt = y + PY - KH + SY;
  int const oxb = (xt > 0 ? xt : 0) / SX, oyb = (yt > 0 ? yt : 0) / SY;
  int const oxe = ((x + PX) / SX + 1 < OW) ? (x + PX) / SX + 1 : OW, oye = ((y + PY) / SY + 1 < OH) ? (y + PY) / SY + 1 : OH;
  float const spread_sz = (float)(KW * KH);
  float const in_yx = (float)(y * W + x);
#if ZINP
  float const zc = p.p3[id];   // (loaded ahead of the gather; this thread owns the pel)
#endif
  float v = 0.0f;
#pragma unroll
  for (int i = 0; i < kMaxX; ++i) {
    int const ox = oxb + i;
#pragma unroll
    for (int j = 0; j < kMaxY; ++j) {
      int const oy = oyb + j;
      if (ox < oxe && oy < oye) {
        int const oix = oy * OW + ox;
#if AVG
        v = v + ogl[oix] / spread_sz;
#else
        if (in_yx == oiyx[oix]) v = v + ogl[oix];
#endif
      }
    }
  }
#if ZINP
  v = zc > 0.0f ? v : 0.0f;
#endif
  p.o0[id] = v;
}

#elif OP == 3
constexpr int kHalf = LS / 2;
extern "C" __global__ __launch_bounds__(256) void KNAME(bck_ops_args_t const p) {
  long const id = (long)blockIdx.x * 256 + threadIdx.x;   // (img, channel block, pel), pel fastest
  if (id >= p.n) return;
  int const ncb = (p.C + CB - 1) / CB;
  int const pel = (int)(id % p.HW), cb = (int)((id / p.HW) % ncb);
  long const img = id / ((long)p.HW * ncb);
  long const base = img * p.C * p.HW + pel;
  int const c0 = cb * CB, c1 = (c0 + CB < p.C) ? c0 + CB : p.C;   // this thread writes channels [c0, c1)
  float line[LS];   // the last LS inputs, newest last
#pragma unroll
  for (int i = 0; i < LS; ++i) line[i] = 0.0f;
  float ls_sum = 0.0f;
  for (int c_in = 0; c_in < c1 + kHalf; ++c_in) {
    float const entering = (c_in < p.C) ? p.p0[base + (long)c_in * p.HW] : 0.0f;
    float const leaving = line[0];
#pragma unroll
    for (int i = 0; i < LS - 1; ++i) line[i] = line[i + 1];
    line[LS - 1] = entering;
    ls_sum = ls_sum + entering * entering;
    ls_sum = ls_sum - leaving * leaving;
    int const c_out = c_in - kHalf;
    if (c_out >= c0) {
      float const scale_base = p.f2 + ls_sum * p.f0;
      p.o1[base + (long)c_out * p.HW] = scale_base;
      p.o0[base + (long)c_out * p.HW] = line[LS - 1 - kHalf] * powf(scale_base, -p.f1);
    }
  }
}

#elif OP == 4
constexpr int kHalf = LS / 2;
constexpr int kSteps = CB + 2 * kHalf + LS - 1;   // from the ring-aligned start to the last channel entering
extern "C" __global__ __launch_bounds__(256) void KNAME(bck_ops_args_t const p) {
  long const id = (long)blockIdx.x * 256 + threadIdx.x;   // (img, channel block, pel), pel fastest
  if (id >= p.n) return;
  int const ncb = (p.C + CB - 1) / CB;
  int const pel = (int)(id % p.HW), cb = (int)((id / p.HW) % ncb);
  long const img = id / ((long)p.HW * ncb);
  long const base = img * p.C * p.HW + pel;
  int const c0 = cb * CB, c1 = (c0 + CB < p.C) ? c0 + CB : p.C;
  int const lo = c0 - kHalf;
  int const cs = lo - (((lo % LS) + LS) % LS);   // first channel walked: the multiple of LS at or below c0 - kHalf (so slot = step % LS is a constant per step)
  float ring[LS];
#pragma unroll
  for (int i = 0; i < LS; ++i) ring[i] = 0.0f;
#pragma unroll
  for (int s = 0; s < kSteps; ++s) {
    int const c_in = cs + s;
    float t = 0.0f;
    if (c_in >= 0 && c_in < p.C && c_in < c1 + kHalf) {
      long const ix = base + (long)c_in * p.HW;
      t = p.p2[ix] * p.p1[ix] / p.p3[ix];
    }
    ring[s % LS] = t;
    int const c_out = c_in - kHalf;
    if (c_out >= c0 && c_out < c1) {
      float ls_sum = 0.0f;
#pragma unroll
      for (int i = 0; i < LS; ++i) ls_sum = ls_sum + ring[i];
      long const ox = base + (long)c_out * p.HW;
      float const in_v = p.p0[ox];
      float const a = p.p2[ox] * powf(p.p3[ox], -p.f1);
      float const b = in_v * ls_sum * p.f3;
#if ZINP
      p.o0[ox] = in_v > 0.0f ? a + b : 0.0f;
#else
      p.o0[ox] = a + b;
#endif
    }
  }
}

#elif OP == 5
extern "C" __global__ __launch_bounds__(256) void KNAME(bck_ops_args_t const p) {
  long const id = (long)blockIdx.x * 256 + threadIdx.x;
  if (id >= p.n) return;
  if (id < p.n4) {
    f32x4 const v = ((f32x4 const *)p.p0)[id], c = ((f32x4 const *)p.p1)[id];
    f32x4 o;
    o.x = c.x > 0.0f ? v.x : 0.0f; o.y = c.y > 0.0f ? v.y : 0.0f; o.z = c.z > 0.0f ? v.z : 0.0f; o.w = c.w > 0.0f ? v.w : 0.0f;
    ((f32x4 *)p.o0)[id] = o;
  } else {
    long const e = 4L * p.n4 + (id - p.n4);
    p.o0[e] = p.p1[e] > 0.0f ? p.p0[e] : 0.0f;
  }
}

#elif OP == 6
extern "C" __global__ __launch_bounds__(256) void KNAME(bck_ops_args_t const p) {
  int const lane = threadIdx.x & 63;
  long const img = (long)blockIdx.x * 4 + (threadIdx.x >> 6);   // one wave per image (a 1 x 1 plane: one pel)
  if (img >= p.B) return;                                       // (whole waves leave together: the shuffles below see full waves)
  float const *const in = p.p0 + img * p.C;
  float *const prob = p.o0 + img * p.C;
  float pel_max = 0.0f;
  for (int c = lane; c < p.C; c += 64) { float const v = in[c]; pel_max = (v > pel_max) ? v : pel_max; }
#pragma unroll
  for (int m = 32; m > 0; m >>= 1) { float const o = __shfl_xor(pel_max, m, 64); pel_max = (o > pel_max) ? o : pel_max; }
  float pel_sum = 0.0f;
  for (int c = lane; c < p.C; c += 64) { float const v = expf(in[c] - pel_max); prob[c] = v; pel_sum = pel_sum + v; }
#pragma unroll
  for (int m = 32; m > 0; m >>= 1) pel_sum = pel_sum + __shfl_xor(pel_sum, m, 64);
  for (int c = lane; c < p.C; c += 64) prob[c] = prob[c] / pel_sum;   // (each lane reads back what it wrote itself)
}

#elif OP == 7
extern "C" __global__ __launch_bounds__(256) void KNAME(bck_ops_args_t const p) {
  long const id = (long)blockIdx.x * 256 + threadIdx.x;   // (img, chan)
  if (id >= p.n) return;
  int const chan = (int)(id % p.C);
  long const img = id / p.C;
  float const lf = p.p1[img];
  bool const valid = lf >= 0.0f && lf < (float)p.C;
  int const label = valid ? (int)lf : -1;
  float v = p.p0[id];
  if (chan == label) v = v - 1.0f;
  v = v / (float)p.B;
  p.o0[id] = v;
  if (chan == 0) {
    float const pl = valid ? p.p0[img * p.C + label] : 0.0f;
    p.o1[img] = -logf(pl > kFltMin ? pl : kFltMin);
  }
}

#elif OP == 8
extern "C" __global__ __launch_bounds__(64) void KNAME(bck_ops_args_t const p) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  float v = 0.0f;
  for (int i = 0; i < p.B; ++i) v = v + p.p0[i];
  p.o0[0] = v / (float)p.B;
}

#elif OP == 9
#define RED_INS(T, ix) \
  T v = (T)0.0f + ((T const *)p.p0)[ix]; v = v + ((T const *)p.p1)[ix]; \
  if (NIN > 2) v = v + ((T const *)p.p2)[ix]; if (NIN > 3) v = v + ((T const *)p.p3)[ix]; if (NIN > 4) v = v + ((T const *)p.p4)[ix]; \
  if (NIN > 5) v = v + ((T const *)p.p5)[ix]; if (NIN > 6) v = v + ((T const *)p.p6)[ix]; if (NIN > 7) v = v + ((T const *)p.p7)[ix];
extern "C" __global__ __launch_bounds__(256) void KNAME(bck_ops_args_t const p) {
  long const id = (long)blockIdx.x * 256 + threadIdx.x;
  if (id >= p.n) return;
  if (id < p.n4) {
    RED_INS(f32x4, id)
    ((f32x4 *)p.o0)[id] = v;
  } else {
    long const e = 4L * p.n4 + (id - p.n4);
    RED_INS(float, e)
    p.o0[e] = v;
  }
}

#elif OP == 10
__device__ __forceinline__ float drop1(float x, unsigned ix, unsigned seed, bck_ops_args_t const &p) {
  unsigned h = ix + seed;
  h ^= h >> 16; h *= 0x85ebca6bu; h ^= h >> 13; h *= 0xc2b2ae35u; h ^= h >> 16;
  return h > p.thresh ? x * p.f0 : 0.0f;
}
extern "C" __global__ __launch_bounds__(256) void KNAME(bck_ops_args_t const p) {
  long const id = (long)blockIdx.x * 256 + threadIdx.x;
  if (id >= p.n) return;
#if SEEDVAR
  unsigned const seed = *(unsigned const *)p.p4 + p.seed;   // (one address for the whole launch)
#else
  unsigned const seed = p.seed;
#endif
  if (id < p.n4) {
    f32x4 v = ((f32x4 const *)p.o0)[id];
    unsigned const e = 4u * (unsigned)id;
    v.x = drop1(v.x, e, seed, p); v.y = drop1(v.y, e + 1u, seed, p); v.z = drop1(v.z, e + 2u, seed, p); v.w = drop1(v.w, e + 3u, seed, p);
    ((f32x4 *)p.o0)[id] = v;
  } else {
    long const e = 4L * p.n4 + (id - p.n4);
    p.o0[e] = drop1(p.o0[e], (unsigned)e, seed, p);
  }
}

#elif OP == 11 || OP == 12
extern "C" __global__ __launch_bounds__(256) void KNAME(bck_ops_args_t const p) {
  long const id = (long)blockIdx.x * 256 + threadIdx.x;
  if (id >= p.n) return;
  long const e = (id < p.n4) ? 4L * id : 4L * p.n4 + (id - p.n4);   // first element, counted in the narrow tensor
  long const img = e / p.run;
  long const w = img * p.wide + p.off + (e - img * p.run);          // the same element in the wide tensor
#if OP == 11
  if (id < p.n4) *(f32x4 *)(p.o0 + w) = *(f32x4 const *)(p.p0 + e); else p.o0[w] = p.p0[e];
#else
  if (id < p.n4) *(f32x4 *)(p.o0 + e) = *(f32x4 const *)(p.p0 + w); else p.o0[e] = p.p0[w];
#endif
}

#elif OP == 13
__device__ __forceinline__ float affine1(float x, float a, float b) {
  float v = x * a;
  v = v + b;
#if RELU
  v = v > 0.0f ? v : 0.0f;
#endif
  return v;
}
extern "C" __global__ __launch_bounds__(256) void KNAME(bck_ops_args_t const p) {
  long const id = (long)blockIdx.x * 256 + threadIdx.x;   // (plane, unit of the plane): n4 quads, then HW - 4 n4 single elements
  if (id >= p.n) return;
  int const units = p.n4 + (p.HW - 4 * p.n4);
  long const plane = id / units;
  int const u = (int)(id - plane * units);
  int const c = (int)(plane % p.C);
  float const a = p.p1[c], b = p.p2[c];
  long const base = plane * p.HW;
  if (u < p.n4) {
    f32x4 v = ((f32x4 const *)(p.p0 + base))[u];
    v.x = affine1(v.x, a, b); v.y = affine1(v.y, a, b); v.z = affine1(v.z, a, b); v.w = affine1(v.w, a, b);
    ((f32x4 *)(p.o0 + base))[u] = v;
  } else {
    long const e = base + 4L * p.n4 + (u - p.n4);
    p.o0[e] = affine1(p.p0[e], a, b);
  }
}

#elif OP == 14
#define SUM_SLABS(T, ix) \
  T v = ((T const *)p.p0)[ix]; \
  for (int d = 1; d < p.B; ++d) v = v + ((T const *)(p.p0 + (long)d * p.wide))[ix];
extern "C" __global__ __launch_bounds__(256) void KNAME(bck_ops_args_t const p) {
  long const id = (long)blockIdx.x * 256 + threadIdx.x;
  if (id >= p.n) return;
  if (id < p.n4) {
    SUM_SLABS(f32x4, id)
    ((f32x4 *)p.o0)[id] = v;
  } else {
    long const e = 4L * p.n4 + (id - p.n4);
    SUM_SLABS(float, e)
    p.o0[e] = v;
  }
}

#elif OP == 15
extern "C" __global__ __launch_bounds__(256) void KNAME(bck_ops_args_t const p) {
  long const id = (long)blockIdx.x * 256 + threadIdx.x;   // one element of the window
  if (id >= p.n) return;
  int const x = (int)(id % OW), y = (int)((id / OW) % OH);
  long const plane = id / (OW * OH);
  p.o0[id] = p.p0[(plane * H + (y + PY)) * W + (x + PX)];
}

#elif OP == 16
extern "C" __global__ __launch_bounds__(256) void KNAME(bck_ops_args_t const p) {
  long const id = (long)blockIdx.x * 256 + threadIdx.x;   // one element of the plane
  if (id >= p.n) return;
  int const x = (int)(id % W) - PX, y = (int)((id / W) % H) - PY;
  long const plane = id / (W * H);
  bool const inside = (unsigned)x < (unsigned)OW && (unsigned)y < (unsigned)OH;
  float v = 0.0f;
  if (inside) v = p.p0[(plane * OH + y) * OW + x];
  p.o0[id] = v;
}

#else
#error "bck_ops_f32.hip: -DOP=1..16"
#endif
