// bck_ops_f32.hip -- the non-conv ops of the gradient pipe, fp32, reference layouts (img:chan:y:x), for gfx950; specialised by hiprtc (-DOP=<n> picks the kernel).
// All of them are bandwidth kernels: one thread per written element (x fastest, so a wave stores whole lines), gathers from a handful of neighbouring lines,
// no atomics -- every output element has one owner, which is what makes the results the same bits run to run.
//
// The semantics are the reference templates', quirks included (parity is the contract); every kernel keeps the WRITTEN order of its fp32 operations: the
// file is compiled with contraction and reassociation off, so a*b + c stays two roundings, and it calls the real powf / expf / logf.
//
// OP 1  bodahip_pool_yx  (test/rtc/pool.cucl with emit_out_in_yx=1, max pooling)   in -> out, out_in_yx
//   * padding pels never take part; taps are visited kx OUTER, ky inner
//   * the maximum starts at -FLT_MAX and is replaced on strict `>`: the FIRST maximal tap in that order wins a tie (and a NaN never wins)
//   * out_in_yx is a FLOAT holding in_y*W + in_x of the winning tap, or -1 when no tap won (a window of -FLT_MAX / NaN only, or one wholly in the padding)
// OP 2  bodahip_spreading  (test/rtc/spreading.cucl)   out_grad_loss, out_in_yx -> in_grad_loss   (the template's `out` arg is never read)
//   * one value per in_grad_loss pel: the outputs whose window holds it are out_x in [max(0, x+pad-k+s)/s, min((x+pad)/s + 1, OW)), likewise y
//   * out_x OUTER, out_y inner, a sequential fp32 sum from +0 (a pel no window holds is exactly +0)
//   * max (AVG=0): add out_grad_loss where out_in_yx == y*W + x (compared as floats);  average (AVG=1): add out_grad_loss / (KH*KW) -- the FULL window area
//     even where the window is clipped by a border, as the reference does (its own FIXME says so); a division per term, not a multiplication by 1/area
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
// OP 8  bodahip_sum_loss_over_imgs  (test/rtc/sum_loss_over_imgs.cucl)   loss = (sequential fp32 sum of loss_per_pel over the images from +0) / img_count: one thread
//
// -D parameters: KNAME OP, then  1, 2: H W OH OW KH KW SY SX PY PX (2: AVG) | 3, 4: LS CB.  Host side: plan_bck_op (native_plan.cc), native_kernels.cc.

#ifndef __HIPCC_RTC__
#include <hip/hip_runtime.h>
#endif

#pragma clang fp contract(off) reassociate(off)

struct bck_ops_args_t {   // must match native_internal.h
  float const *p0; float const *p1; float const *p2; float const *p3;   // inputs, in the function's arg order
  float *o0; float *o1;                                                 // outputs, in the function's arg order
  long n;                                                               // threads that have work
  int B, C, HW, n4;                                                     // images, channels, pels of a plane; OP 5: float4 quads
  float f0, f1, f2, f3;                                                 // LRN: alpha / local_size, beta, k, ((2 * -beta) * alpha) / local_size
};

constexpr float kFltMax = 3.402823466e+38f, kFltMin = 1.175494351e-38f;

#if OP == 1
extern "C" __global__ __launch_bounds__(256) void KNAME(bck_ops_args_t const p) {
  long const id = (long)blockIdx.x * 256 + threadIdx.x;
  if (id >= p.n) return;
  int const ox = (int)(id % OW), oy = (int)((id / OW) % OH);
  long const plane = id / (OW * OH);
  float const *const in = p.p0 + plane * (H * W);
  float best = -kFltMax; int oyx = -1;
#pragma unroll
  for (int kx = 0; kx < KW; ++kx) {
#pragma unroll
    for (int ky = 0; ky < KH; ++ky) {
      int const iy = oy * SY + ky - PY, ix = ox * SX + kx - PX;
      if (iy >= 0 && ix >= 0 && ix < W && iy < H) {
        float const v = in[iy * W + ix];
        if (v > best) { best = v; oyx = iy * W + ix; }
      }
    }
  }
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
      float const a = p.p2[ox] * powf(p.p3[ox], -p.f1);
      float const b = p.p0[ox] * ls_sum * p.f3;
      p.o0[ox] = a + b;
    }
  }
}

#elif OP == 5
typedef float f32x4 __attribute__((ext_vector_type(4)));
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

#else
#error "bck_ops_f32.hip: -DOP=1..8"
#endif
