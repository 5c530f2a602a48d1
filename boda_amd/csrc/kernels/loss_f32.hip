// loss_f32.hip -- the full SoftmaxWithLoss of the gradient pipe (family `loss`), for gfx950; specialised by hiprtc (-DOP=<n> picks the kernel).  Three functions, this
// backend's own: Caffe's SoftmaxWithLossLayer with loss_weight, ignore_label, planes larger than 1 x 1 and LossParameter's four normalisers, restated.  The reference's
// three calls (kernels/bck_ops_f32.hip OP 6 - 8) stay as they are; these are what a head with a LossSpec lowers to.  The file is compiled with contraction and
// reassociation off; the divide is the correctly rounded form (no fast-math option on the compile).  Every store is a per-lane vector store, every output element has
// one owner, there are no atomics.  The same operations in the same order run on be=cpu (csrc/cpu_compute.cc) and in the numpy twin (tests/loss_ref.py); expf and logf
// are each platform's own, so prob and loss_per_pel are held to bounds across platforms and everything behind them to bits.
//
// Shared by all three.  C = chan, HW = y * x, a pel is (img, y, x), its channel c lies at in[(img * C + c) * HW + pel] (channel stride HW).  lf = label[img * HW + pel]:
//   ignored  iff has_ignore && lf == ignore            (ignore = (float)ignore_label; tested FIRST, so an ignore_label inside [0, C) ignores that class)
//   valid    iff not ignored && lf >= 0 && lf < (float)C, then L = (int)lf (truncation)
//   invalid  otherwise (a NaN included): it matches no channel and reads no memory
//
// OP 1  bodahip_softmax_loss_fwd   in, label -> prob (img:chan:y:x), loss_per_pel (img:y:x)
//   Per pel:  m = max_c in[c]  (the TRUE maximum: m = in[0], then m = v > m ? v : m over c = 1 .. C - 1; this is NOT bodahip_softmax's max(0, .), so logits that are
//   all near -200 give finite probabilities where that one gives 0 / 0);  e[c] = exp_diff(in[c], m);  S = the sum of e[c];  prob[c] = e[c] / S;
//   exp_diff(a, m) is exp(a - m) with the difference held EXACTLY, as the pair (d, r) of Knuth's two-sum: d = a - m rounded, r what the rounding dropped;
//   e = expf(d), then e = e + e * r.  Rounding a difference of 160 alone moves its exponential by 128 u, which no bound relative to a small probability survives;
//   with the pair, logits far below the maximum keep prob's relative bound.
//   loss_per_pel = ignored ? +0 : valid ? -logf(max(prob[L], FLT_MIN)) : kInvalidLoss, prob[L] being the fp32 value stored.  kInvalidLoss is -logf(FLT_MIN) = 126 ln 2
//   correctly rounded (0x42AEAC50), written as a constant so that both platforms store the same word.  prob is written at every pel, the ignored ones included.
//   Two forms, picked by the planner from the op alone:
//   -DFORM=0, the pel form (HW >= 64): one thread per (img, pel), lanes along the pels, so every channel step of a wave reads one 256-byte line.  S is the sequential
//     chain over c = 0 .. C - 1 from +0.  One pass for the maximum, one for expf and the sum, one for the divide and the store; with -DCREG=C (1 <= C <= 32) the e[c]
//     stay in registers, with -DCREG=0 the third pass reads in[c] again (an L2 hit) and forms the same exp_diff.
//   -DFORM=1, the wave form (HW < 64; every 1 x 1 head): one wave per pel, four per workgroup of 256 -- bodahip_softmax's layout.  Lane l takes channels l, l + 64, ...:
//     its own maximum and its own sequential sum from +0, then xor butterflies (32, 16, ... 1) for both; fp32 max and add commute, so every lane ends with the same
//     word.  A lane without a channel (C < 64) enters with -inf and +0.  The third pass forms exp_diff again.  Whole waves leave together before any shuffle.
//
// OP 2  bodahip_loss_norm   label, loss_per_pel -> loss (y=1:x=1), loss_state (v=4 = [Z, s, count, sum])
//   ONE workgroup of 256.  N = B * HW < 2^24 pels.  Thread t takes pels t, t + 256, ... in order: a = a + loss_per_pel[i] from +0, and counts the pels that are not
//   ignored (an integer: exact in any order).  The 256 pairs meet in the halving tree h = 128, 64, ... 1: s[t] = s[t] + s[t + h] for t < h.  THE CHAIN of the loss sum
//   is therefore ceil(N / 256) sequential adds and 8 tree levels deep.  Then thread 0:
//     Z = valid: max(1, count) | full: N | batch_size: B | none: 1, as a float (exact: all below 2^24);  s = weight / Z  (one fp32 divide);  loss = sum / Z
//   The loss is unweighted, as Caffe's top blob is.  Invalid pels count towards Z, ignored ones do not.  All pels ignored: count = 0, Z = 1 (valid), sum = +0, loss = +0.
//
// OP 3  bodahip_softmax_loss_bck   prob, label, loss_state -> in_grad_loss
//   Per element (img, c, pel):  ignored ? +0 : (prob - (c == L ? 1 : 0)) * s, two fp32 roundings, s = loss_state[1] READ FROM DEVICE MEMORY: one captured graph serves
//   batches with different numbers of ignored pels and the host never waits for a count.  An invalid pel has no L.  A thread owns four consecutive elements of the flat
//   tensor (one 16-byte load and store; the base is 16-byte aligned), decoded once and carried pel -> chan -> img; the last thread of a tensor whose size is no multiple
//   of four moves dwords.
//
// -D parameters: KNAME OP FORM CREG.  Host side: loss_op_of_op (rtc_types.h), plan_loss_op (native_plan.cc), native_kernels_t::loss_call (native_kernels.cc), the argument
// checks in native_run.cc.

#ifndef __HIPCC_RTC__
#include <hip/hip_runtime.h>
#endif

#pragma clang fp contract(off) reassociate(off)

#include "kernel_args.h"      // softmax_loss_fwd_args_t, loss_norm_args_t, softmax_loss_bck_args_t
#include "device_prelude.h"

constexpr float kFltMin = 1.175494351e-38f;
constexpr float kInvalidLoss = 0x1.5d58a0p+6f;   // 126 ln 2 rounded to fp32: 0x42AEAC50

#if OP == 1
__device__ __forceinline__ float exp_diff(float a, float m) {
  float const d = a - m;
  float const bb = d - a;
  float const r = (a - (d - bb)) - (m + bb);   // a - m == d + r exactly
  float const e = expf(d);
  float const er = e * r;
  return e + er;
}
#if !defined(FORM) || !defined(CREG)
#error "loss_f32.hip OP 1: -DFORM=0|1 -DCREG=0..32"
#endif
__device__ __forceinline__ float pel_loss(softmax_loss_fwd_args_t const &p, float lf, float const *in, long cs, float m, float S) {
  if (p.has_ignore && lf == p.ignore) return 0.0f;
  if (!(lf >= 0.0f && lf < (float)p.C)) return kInvalidLoss;
  int const L = (int)lf;
  float const pl = exp_diff(in[L * cs], m) / S;   // (the operations that made the stored prob[L]: the same word)
  return -logf(pl > kFltMin ? pl : kFltMin);
}

#if FORM == 0
extern "C" __global__ __launch_bounds__(256) void KNAME(softmax_loss_fwd_args_t const p) {
  long const id = (long)blockIdx.x * 256 + threadIdx.x;   // (img, pel)
  if (id >= (long)p.B * p.HW) return;
  long const img = id / p.HW, pel = id - img * p.HW, cs = p.HW;
  float const *const in = p.in + img * p.C * cs + pel;
  float *const prob = p.prob + img * p.C * cs + pel;
#if CREG > 0
  float e[CREG];
#pragma unroll
  for (int c = 0; c < CREG; ++c) e[c] = in[c * cs];
  float m = e[0];
#pragma unroll
  for (int c = 1; c < CREG; ++c) m = e[c] > m ? e[c] : m;
  float S = 0.0f;
#pragma unroll
  for (int c = 0; c < CREG; ++c) { e[c] = exp_diff(e[c], m); S = S + e[c]; }
#pragma unroll
  for (int c = 0; c < CREG; ++c) prob[c * cs] = e[c] / S;
#else
  float m = in[0];
  for (int c = 1; c < p.C; ++c) { float const v = in[c * cs]; m = v > m ? v : m; }
  float S = 0.0f;
  for (int c = 0; c < p.C; ++c) S = S + exp_diff(in[c * cs], m);
  for (int c = 0; c < p.C; ++c) prob[c * cs] = exp_diff(in[c * cs], m) / S;
#endif
  p.loss_per_pel[id] = pel_loss(p, p.label[id], in, cs, m, S);
}
#else
extern "C" __global__ __launch_bounds__(256) void KNAME(softmax_loss_fwd_args_t const p) {
  int const lane = threadIdx.x & 63;
  long const id = (long)blockIdx.x * 4 + (threadIdx.x >> 6);   // one wave per (img, pel)
  if (id >= (long)p.B * p.HW) return;                          // (whole waves leave together: the shuffles below see full waves)
  long const img = id / p.HW, pel = id - img * p.HW, cs = p.HW;
  float const *const in = p.in + img * p.C * cs + pel;
  float *const prob = p.prob + img * p.C * cs + pel;
  float m = -__builtin_inff();
  for (int c = lane; c < p.C; c += 64) { float const v = in[c * cs]; m = v > m ? v : m; }
#pragma unroll
  for (int k = 32; k > 0; k >>= 1) { float const o = __shfl_xor(m, k, 64); m = o > m ? o : m; }
  float S = 0.0f;
  for (int c = lane; c < p.C; c += 64) S = S + exp_diff(in[c * cs], m);
#pragma unroll
  for (int k = 32; k > 0; k >>= 1) S = S + __shfl_xor(S, k, 64);
  for (int c = lane; c < p.C; c += 64) prob[c * cs] = exp_diff(in[c * cs], m) / S;
  if (lane == 0) p.loss_per_pel[id] = pel_loss(p, p.label[id], in, cs, m, S);
}
#endif

#elif OP == 2
extern "C" __global__ __launch_bounds__(256) void KNAME(loss_norm_args_t const p) {
  __shared__ float sa[256];
  __shared__ unsigned sc[256];
  int const t = threadIdx.x;
  if (blockIdx.x != 0) return;
  float a = 0.0f; unsigned cnt = 0u;
#pragma unroll 8
  for (int i = t; i < p.N; i += 256) {   // (unrolled: eight pels' loads in flight, the adds in order)
    a = a + p.loss_per_pel[i];
    float const lf = p.label[i];
    cnt += (p.has_ignore && lf == p.ignore) ? 0u : 1u;
  }
  sa[t] = a; sc[t] = cnt;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if (t < h) { sa[t] = sa[t] + sa[t + h]; sc[t] += sc[t + h]; }
    __syncthreads();
  }
  if (t != 0) return;
  float const sum = sa[0]; unsigned const count = sc[0];
  float Z = 1.0f;
  if (p.norm == 0) Z = (float)(count > 1u ? count : 1u); else if (p.norm == 1) Z = (float)p.N; else if (p.norm == 2) Z = (float)p.B;
  float const s = p.weight / Z;
  p.loss[0] = sum / Z;
  p.state[0] = Z; p.state[1] = s; p.state[2] = (float)count; p.state[3] = sum;
}

#elif OP == 3
extern "C" __global__ __launch_bounds__(256) void KNAME(softmax_loss_bck_args_t const p) {
  long const e0 = ((long)blockIdx.x * 256 + threadIdx.x) * 4;   // the first of this thread's four flat elements
  if (e0 >= p.n) return;
  float const s = p.state[1];
  long q = e0 / p.HW;
  int pel = (int)(e0 - q * p.HW);
  long img = q / p.C;
  int c = (int)(q - img * p.C);
  int const cnt = (p.n - e0 < 4) ? (int)(p.n - e0) : 4;
  float v[4] = {0.f, 0.f, 0.f, 0.f};
  if (cnt == 4) { f32x4 const w = *(f32x4 const *)(p.prob + e0); v[0] = w.x; v[1] = w.y; v[2] = w.z; v[3] = w.w; }
  else for (int k = 0; k < cnt; ++k) v[k] = p.prob[e0 + k];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (k < cnt) {
      float const lf = p.label[img * p.HW + pel];
      if (p.has_ignore && lf == p.ignore) v[k] = 0.0f;
      else {
        bool const valid = lf >= 0.0f && lf < (float)p.C;
        float const d = (valid && (int)lf == c) ? v[k] - 1.0f : v[k];
        v[k] = d * s;
      }
      if (++pel == p.HW) { pel = 0; if (++c == p.C) { c = 0; ++img; } }
    }
  }
  if (cnt == 4) { f32x4 w; w.x = v[0]; w.y = v[1]; w.z = v[2]; w.w = v[3]; *(f32x4 *)(p.grad + e0) = w; }
  else for (int k = 0; k < cnt; ++k) p.grad[e0 + k] = v[k];
}

#else
#error "loss_f32.hip: -DOP=1..3"
#endif
