// eval_f32.hip -- the evaluation pass of the gradient pipe (family `eval`), for gfx950; specialised by hiprtc (-DOP=<n> picks the kernel).  Three functions, this
// backend's own (the reference names an Accuracy op type, src/conv_util.cc:51, and runs none).  The file is compiled with contraction and reassociation off; the
// divide and the square root are the correctly rounded forms (no fast-math option on the compile).  Every store is a per-lane vector store, every output element has
// one owner, there are no atomics.  The same operations in the same order run on be=cpu (csrc/cpu_compute.cc) and in the numpy twins (tests/eval_ref.py).
//
// OP 1  bodahip_accuracy      in (float img:chan:1:1, the LOGITS), label (float img:1:1) -> rank (uint32 img)
//   Per image, C = chan: lf = label[img] is valid iff lf >= 0 && lf < (float)C -- hip_sm_grad_and_loss's test -- and then L = (int)lf (truncation).  A NaN label is
//   invalid.  Invalid: rank = 0xFFFFFFFF, which misses under every top_k.  Valid: rank = #{ c != L : !(in[c] < in[L]) }: the number of OTHER classes the true class
//   does not beat.  For ordered values this is Caffe's rule: the true class competes against every >= score, so ties count against it, and a net that answers a
//   constant has rank C - 1 and scores 0, not 1.  Written as !(<), a NaN on EITHER side counts against the true class too: a diverged net (all NaN) scores 0, where
//   Caffe's >= (false for every NaN) would rank the true class first and score 1.  -0 and +0 tie.
//   Layout: bodahip_softmax's.  One wave per image, four per workgroup of 256; lane l takes channels l, l + 64, ...; every lane loads in[L] from the one address; the
//   64 integer counts meet in a butterfly (integers: any order gives the same word); lane 0 stores.
//
// OP 2  bodahip_eval_accum    rank (uint32 img), loss (float y=1:x=1), ctl (uint32 v=4 = [first, 0, 0, 0]) -> counts (uint32 v=4 = [images, hits_top1, hits_topk,
//   batches]), loss_sum (float v=1)
//   One workgroup of 256.  Thread t takes images t, t + 256, ...: h1 counts rank < 1, hk counts rank < top_k; the 256 pairs meet in a tree (integers).  Then thread 0:
//     ctl[0] != 0:  counts' = [B, h1, hk, 1]            loss_sum' = loss (its bits); counts and loss_sum are NOT read
//     else:         counts' = counts + [B, h1, hk, 1]   loss_sum' = loss_sum + loss (one fp32 add)
//   hip_grad_accum's protocol: the word lives in device memory, so one captured graph serves every batch and nobody ever clears an accumulator.  images counts every
//   image, the ones with an invalid label included.
//
// OP 3  bodahip_bn_fold       run_mean, run_var, scale, bias (float chan) -> a, b (float chan)
//   One thread per channel.  conv_pipe.fold_affine([("BatchNorm", mean, var, eps), ("Scale", scale, bias)])'s chain LITERALLY, every line one fp32 rounding:
//     ve = var + eps;  sd = sqrtf(ve);  a2 = 1 / sd;  mp = mean * a2;  b2 = -mp;  a1 = a2 * 1;  z = a2 * 0;  b1 = z + b2;  a = scale * a1;  sb = scale * b1;  b = sb + bias
//   (the quotient and the root formed as hip_bn_stats forms inv_std).  fold_affine stays the one definition of the fold; the bar is its bits.  var + eps < 0 gives
//   NaN, as numpy does (which NaN is the platform's); b2 = -0 becomes +0 through z + b2; an infinite a2 gives NaN through a2 * 0.
//
// -D parameters: KNAME OP.  Host side: eval_op_of_op (rtc_types.h), plan_eval_op (native_plan.cc), native_kernels_t::eval_call (native_kernels.cc), the argument checks in
// native_run.cc.

#ifndef __HIPCC_RTC__
#include <hip/hip_runtime.h>
#endif

#pragma clang fp contract(off) reassociate(off)

#include "kernel_args.h"      // accuracy_args_t, eval_accum_args_t, bn_fold_args_t
#include "device_prelude.h"

#if OP == 1
extern "C" __global__ __launch_bounds__(256) void KNAME(accuracy_args_t const p) {
  int const lane = threadIdx.x & 63;
  long const img = (long)blockIdx.x * 4 + (threadIdx.x >> 6);   // one wave per image
  if (img >= p.B) return;                                       // (whole waves leave together: the shuffles below see full waves)
  float const lf = p.label[img];
  bool const valid = lf >= 0.0f && lf < (float)p.C;             // (the same word in every lane of the wave)
  unsigned cnt = 0u;
  if (valid) {
    int const L = (int)lf;                                      // 0 <= L < C
    float const *const in = p.in + img * p.C;
    float const t = in[L];
    for (int c = lane; c < p.C; c += 64) { float const v = in[c]; cnt += (c != L && !(v < t)) ? 1u : 0u; }
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) cnt += (unsigned)__shfl_xor((int)cnt, m, 64);
  }
  if (lane == 0) p.rank[img] = valid ? cnt : 0xFFFFFFFFu;
}

#elif OP == 2
extern "C" __global__ __launch_bounds__(256) void KNAME(eval_accum_args_t const p) {
  __shared__ unsigned s1[256], sk[256];
  int const t = threadIdx.x;
  if (blockIdx.x != 0) return;
  unsigned h1 = 0u, hk = 0u;
  for (int i = t; i < p.B; i += 256) { unsigned const r = p.rank[i]; h1 += (r < 1u) ? 1u : 0u; hk += (r < p.top_k) ? 1u : 0u; }
  s1[t] = h1; sk[t] = hk;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if (t < h) { s1[t] += s1[t + h]; sk[t] += sk[t + h]; }
    __syncthreads();
  }
  if (t != 0) return;
  unsigned const B = (unsigned)p.B;
  h1 = s1[0]; hk = sk[0];
  if (p.ctl[0] != 0u) {
    p.counts[0] = B; p.counts[1] = h1; p.counts[2] = hk; p.counts[3] = 1u;
    ((unsigned *)p.loss_sum)[0] = ((unsigned const *)p.loss)[0];   // the loss's bits
  } else {
    unsigned const c0 = p.counts[0], c1 = p.counts[1], c2 = p.counts[2], c3 = p.counts[3];
    float const ls = p.loss_sum[0];
    p.counts[0] = c0 + B; p.counts[1] = c1 + h1; p.counts[2] = c2 + hk; p.counts[3] = c3 + 1u;
    p.loss_sum[0] = ls + p.loss[0];
  }
}

#elif OP == 3
extern "C" __global__ __launch_bounds__(256) void KNAME(bn_fold_args_t const p) {
  int const c = (int)(blockIdx.x * 256 + threadIdx.x);   // one owner per channel
  if (c >= p.C) return;
  float const mean = p.run_mean[c], var = p.run_var[c], sc = p.scale[c], bi = p.bias[c];
  float const ve = var + p.eps;
  float const sd = sqrtf(ve);
  float const a2 = 1.0f / sd;
  float const mp = mean * a2;
  float const b2 = -mp;
  float const a1 = a2 * 1.0f;
  float const z = a2 * 0.0f;
  float const b1 = z + b2;
  float const a = sc * a1;
  float const sb = sc * b1;
  p.a[c] = a; p.b[c] = sb + bi;
}

#else
#error "eval_f32.hip: -DOP=1..3"
#endif
