// solver_update_f32.hip -- the solvers of the gradient pipe beyond plain SGD (family `solver`), fp32, for gfx950; specialised by hiprtc.  Three functions, and the two of gradient accumulation (OP 4 and OP 1 with ACCUM=1, below):
//     OP 1  hip_solver_update (op type SolverUpdate): SGD, Nesterov or Adam over up to 32 tensors in one launch, optionally with the gradient scaled by the clip coefficient
//     OP 2  hip_grad_sumsq    (op type GradSumsq):    one partial sum of squares per chunk of 4096 gradient elements
//     OP 3  hip_grad_norm     (op type GradNorm):     the partials summed, the global norm and the clip coefficient
// This backend's own arithmetic (the reference has no solver); written as kernels/sgd_update_f32.hip is written: contraction and reassociation off, one workgroup of 256
// per chunk of CHUNK = 4096 consecutive floats of ONE tensor, the table of tensors BY VALUE in the kernel arguments, every store a per-lane vector store.  be=cpu
// (csrc/cpu_compute.cc) and the numpy twin (tests/solver_ref.py) run the same chains; sqrtf and / are the correctly rounded forms (no fast-math option on the compile).
//
// OP 1.  hyper = [lr, momentum, weight_decay, momentum2, delta, corr, clip_gradients, unused] and state = [coef, norm, sumsq, 0] live in device memory and are read with
// ordinary loads: a captured launch freezes the table, not those words.  state is always bound and read only with CLIP=1.  Once per tensor i:
//     lr_i = lr * lr_mult_i            wd_i = weight_decay * decay_mult_i
// and per element, every line one fp32 rounding:
//     g0 = CLIP ? coef * g : g
//   SOLVER 0 (sgd):       g1 = g0 + wd_i * w;   a = momentum * h;   b = lr_i * g1;   h' = a + b;   w' = w - h'            (CLIP=0: hip_sgd_update's chain, bit for bit)
//   SOLVER 1 (nesterov):  the same g1, a, b, h';   c = 1.0f + momentum (once);   u = c * h';   u = u - a;   w' = w - u    (Caffe's)
//   SOLVER 2 (adam):      g1 = DWD ? g0 : g0 + wd_i * w;   o1 = 1.0f - momentum, o2 = 1.0f - momentum2 (once);
//                         m' = momentum * h + o1 * g1 (two products, one add);   q = g1 * g1;   v' = momentum2 * h2 + o2 * q;   d = sqrtf(v') + delta;   r = m' / d;
//                         s = lr_i * corr (once per tensor);   u = s * r;   DWD: dw = (lr_i * wd_i) * w (the product lr_i * wd_i once per tensor), u = u + dw;   w' = w - u
//                         stores h = m', h2 = v', w'
//   g is only read: <param>_grad_loss keeps the unclipped gradient (Caffe scales the diff in place; this does not).  corr = sqrt(1 - momentum2^t) / (1 - momentum^t) comes
//   from the host, computed in float64 and rounded once: no pow runs here.
//   Quads allowed (the host sets it where w, g, h and, for adam, h2 are all 16-byte aligned; a chunk starts at a multiple of 4096 floats): a thread takes up to four
//   float4 of each tensor -- quads tid, tid + 256, tid + 512, tid + 768 of the chunk -- and issues all of those loads before its first store; the up to three elements
//   behind the chunk's last whole quad are scalars.  Not allowed: the whole chunk is scalars.  One owner per element, which reads its element before it writes it.
//
// OP 2.  The workgroup of chunk k of the call (chunks numbered over the call's tensors as blk0 numbers them) writes partials[part0 + k] and nothing else.  Lane t starts from
// +0 and adds x * x (the product rounded, then the add rounded) for the chunk's elements t, t + 256, t + 512, ... in that order: the order of the chain is per-lane dwords,
// coalesced across the lanes; all of a lane's up to 16 loads are issued before its first add.  Then THE TREE over the 256 lane sums a[0 .. 255]:
//     for h = 128, 64, 32, 16, 8, 4, 2, 1:   a[t] = a[t] + a[t + h]  for every t < h          (the tree of kernels/bn_f32.hip)
// a[0] is the result.  Lane 0 stores it.
//
// OP 3.  One workgroup of 256.  Lane t starts from +0 and adds partials[t], partials[t + 256], ... in that order; then the same tree; sumsq = a[0]; norm = sqrtf(sumsq);
// clip = hyper[6]; coef = (norm > clip) ? clip / norm : 1.0f.  Lanes 0 .. 3 store state = [coef, norm, sumsq, +0], one word each; nothing else is written.  From the expression:
//     a NaN norm (a NaN gradient: squares have one sign, so nothing else makes one)  ->  the comparison is false, coef = 1
//     an infinite norm (an Inf gradient, or a sum of squares that overflows) ->  coef = clip / inf = +0
//     norm == clip  ->  coef = 1;   all-zero gradients  ->  norm = 0, coef = 1 (for clip >= 0)
//
// Gradient accumulation over iter_size micro-steps.  accum = [first, apply, scale, micro] lives in device memory and is read with ordinary loads,
// like hyper and state: one captured launch serves every micro-step.
//
// OP 4  hip_grad_accum (op type GradAccum).  Per element of every tensor, g the micro-step's gradient and a the accumulator:
//     accum[0] != 0:  a' = g  (the bits of g; a is NOT read, so the accumulators never need clearing)        else:  a' = a + g  (one fp32 add, denormals kept)
//   g is only read; nothing outside the a_i is written.  Quads where g and a are both 16-byte aligned, as OP 1: all of a thread's loads before its first store.
//
// OP 1 with ACCUM=1  hip_solver_update_acc (op type SolverUpdateAcc): OP 1 with g the accumulator, and
//     accum[1] == 0:  every workgroup returns before its first store: the launch writes nothing
//     otherwise:      g0 = CLIP ? coef * g : g;   gs = accum[2] * g0 (one rounding);   the chain of the SOLVER above with gs where it has g0
//   Caffe's order: clip on the SUMMED gradient, then normalise by 1 / iter_size, then regularise.  With accum[2] == 1 the bits are hip_solver_update's.
//
// -D parameters: KNAME, OP; OP 1: SOLVER (0 | 1 | 2), CLIP (0 | 1), DWD (0 | 1, adam only), ACCUM (0 | 1).  Host side: plan_solver (native_plan.cc),
// native_kernels_t::solver_update / grad_sumsq / grad_norm / grad_accum (native_kernels.cc), the argument checks in native_run.cc.

#ifndef __HIPCC_RTC__
#include <hip/hip_runtime.h>
#endif

#pragma clang fp contract(off) reassociate(off)

#include "kernel_args.h"      // solver_tensor_t, solver_update_args_t, sumsq_tensor_t, grad_sumsq_args_t, grad_norm_args_t, accum_tensor_t, grad_accum_args_t, solver_update_acc_args_t, kSgdMaxTens
#define SOLVER_CHUNK 4096

#ifndef SOLVER
#define SOLVER 0
#endif
#ifndef CLIP
#define CLIP 0
#endif
#ifndef DWD
#define DWD 0
#endif
#ifndef ACCUM
#define ACCUM 0
#endif

#if OP == 2 || OP == 3
// THE TREE (see the header): a[t] holds lane t's sum on entry; -> a[0] in every lane
static __device__ __forceinline__ float solver_tree(float *a, float mine, unsigned tid) {
  a[tid] = mine;
  __syncthreads();
#pragma unroll
  for (unsigned h = 128; h > 0; h >>= 1) {
    if (tid < h) { float const s = a[tid] + a[tid + h]; a[tid] = s; }
    __syncthreads();
  }
  return a[0];
}
#endif

#if OP == 1
struct solver_coef_t { float lr, wd, mom, mom2, delta, coef, c, o1, o2, s, lrwd, scale; };

// one element: -> w', h' (and v' for adam)
static __device__ __forceinline__ void solver_one(float w, float g, float h, float v, solver_coef_t const k, float &w2, float &h2, float &v2) {
#if CLIP
  float const gc = k.coef * g;
#else
  float const gc = g;
#endif
#if ACCUM
  float const g0 = k.scale * gc;
#else
  float const g0 = gc;
#endif
#if SOLVER == 2
#if DWD
  float const g1 = g0;
#else
  float const reg = k.wd * w;
  float const g1 = g0 + reg;
#endif
  float const ma = k.mom * h;
  float const mb = k.o1 * g1;
  float const m = ma + mb;
  float const q = g1 * g1;
  float const va = k.mom2 * v;
  float const vb = k.o2 * q;
  float const vn = va + vb;
  float const sq = sqrtf(vn);
  float const d = sq + k.delta;
  float const r = m / d;
  float u = k.s * r;
#if DWD
  float const dw = k.lrwd * w;
  u = u + dw;
#endif
  h2 = m; v2 = vn; w2 = w - u;
#else
  float const reg = k.wd * w;
  float const g1 = g0 + reg;
  float const a = k.mom * h;
  float const b = k.lr * g1;
  float const hn = a + b;
  h2 = hn; v2 = v;
#if SOLVER == 1
  float u = k.c * hn;
  u = u - a;
  w2 = w - u;
#else
  w2 = w - hn;
#endif
#endif
}

#if ACCUM
extern "C" __global__ __launch_bounds__(256) void KNAME(solver_update_acc_args_t const p) {
  if (p.accum[1] == 0.0f) return;   // (not the applying micro-step: nothing is written)
#else
extern "C" __global__ __launch_bounds__(256) void KNAME(solver_update_args_t const p) {
#endif
  unsigned const b = blockIdx.x;
  int ti = 0;
#pragma unroll
  for (int i = 1; i < kSgdMaxTens; ++i) if (i < (int)p.tens_num && b >= p.t[i].blk0) ti = i;
  ti = __builtin_amdgcn_readfirstlane(ti);
  solver_tensor_t const t = p.t[ti];
  unsigned const base = (b - t.blk0) * SOLVER_CHUNK;
  if (base >= t.n) return;   // (never: the grid is the sum of the chunks)
  unsigned const cnt = (t.n - base < SOLVER_CHUNK) ? (t.n - base) : SOLVER_CHUNK;
  solver_coef_t k;
  k.lr = p.hyper[0] * t.lr_mult; k.wd = p.hyper[2] * t.decay_mult; k.mom = p.hyper[1]; k.mom2 = p.hyper[3]; k.delta = p.hyper[4];
  k.coef = CLIP ? p.state[0] : 1.0f;
  k.c = 1.0f + k.mom; k.o1 = 1.0f - k.mom; k.o2 = 1.0f - k.mom2; k.s = k.lr * p.hyper[5]; k.lrwd = k.lr * k.wd;
#if ACCUM
  k.scale = p.accum[2];
#else
  k.scale = 1.0f;
#endif
  float *const w = t.w + base; float const *const g = t.g + base; float *const h = t.h + base;
#if SOLVER == 2
  float *const v = t.h2 + base;
#endif
  unsigned const tid = threadIdx.x;
  unsigned done = 0;   // elements of the chunk covered by quads
  if (t.quads) {
    unsigned const nq = cnt / 4;
    float4 W[4], G[4], H[4];
#if SOLVER == 2
    float4 V[4];
#endif
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      unsigned const q = tid + 256u * j;
      if (q < nq) {
        W[j] = ((float4 const *)w)[q]; G[j] = ((float4 const *)g)[q]; H[j] = ((float4 const *)h)[q];
#if SOLVER == 2
        V[j] = ((float4 const *)v)[q];
#endif
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      unsigned const q = tid + 256u * j;
      if (q < nq) {
        float4 w2, h2, v2;
#if SOLVER == 2
        float4 const vv = V[j];
#else
        float4 const vv = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
#endif
        solver_one(W[j].x, G[j].x, H[j].x, vv.x, k, w2.x, h2.x, v2.x);
        solver_one(W[j].y, G[j].y, H[j].y, vv.y, k, w2.y, h2.y, v2.y);
        solver_one(W[j].z, G[j].z, H[j].z, vv.z, k, w2.z, h2.z, v2.z);
        solver_one(W[j].w, G[j].w, H[j].w, vv.w, k, w2.w, h2.w, v2.w);
        ((float4 *)h)[q] = h2;
#if SOLVER == 2
        ((float4 *)v)[q] = v2;
#endif
        ((float4 *)w)[q] = w2;
      }
    }
    done = nq * 4;
  }
  for (unsigned e = done + tid; e < cnt; e += 256) {
    float w2, h2, v2;
#if SOLVER == 2
    float const vv = v[e];
#else
    float const vv = 0.0f;
#endif
    solver_one(w[e], g[e], h[e], vv, k, w2, h2, v2);
    h[e] = h2;
#if SOLVER == 2
    v[e] = v2;
#endif
    w[e] = w2;
  }
}
#endif

#if OP == 2
extern "C" __global__ __launch_bounds__(256) void KNAME(grad_sumsq_args_t const p) {
  __shared__ float a[256];
  unsigned const b = blockIdx.x;
  int ti = 0;
#pragma unroll
  for (int i = 1; i < kSgdMaxTens; ++i) if (i < (int)p.tens_num && b >= p.t[i].blk0) ti = i;
  ti = __builtin_amdgcn_readfirstlane(ti);
  sumsq_tensor_t const t = p.t[ti];
  unsigned const base = (b - t.blk0) * SOLVER_CHUNK;
  unsigned const cnt = (base < t.n) ? ((t.n - base < SOLVER_CHUNK) ? (t.n - base) : SOLVER_CHUNK) : 0u;   // (never 0: the grid is the sum of the chunks)
  float const *const g = t.g + base;
  unsigned const tid = threadIdx.x;
  float X[16];
#pragma unroll
  for (int j = 0; j < 16; ++j) { unsigned const e = tid + 256u * j; X[j] = (e < cnt) ? g[e] : 0.0f; }
  float acc = 0.0f;
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    unsigned const e = tid + 256u * j;
    if (e < cnt) { float const q = X[j] * X[j]; acc = acc + q; }   // (an element past the chunk's end adds no term: +0 stays +0)
  }
  float const r = solver_tree(a, acc, tid);
  if (tid == 0) p.partials[p.part0 + b] = r;
}
#endif

#if OP == 3
extern "C" __global__ __launch_bounds__(256) void KNAME(grad_norm_args_t const p) {
  __shared__ float a[256];
  unsigned const tid = threadIdx.x;
  float acc = 0.0f;
  for (unsigned e = tid; e < p.n_parts; e += 256) acc = acc + p.partials[e];
  float const sumsq = solver_tree(a, acc, tid);
  float const norm = sqrtf(sumsq);
  float const clip = p.hyper[6];
  float const coef = (norm > clip) ? clip / norm : 1.0f;
  if (tid < 4) p.state[tid] = (tid == 0) ? coef : (tid == 1) ? norm : (tid == 2) ? sumsq : 0.0f;
}
#endif

#if OP == 4
extern "C" __global__ __launch_bounds__(256) void KNAME(grad_accum_args_t const p) {
  unsigned const b = blockIdx.x;
  int ti = 0;
#pragma unroll
  for (int i = 1; i < kSgdMaxTens; ++i) if (i < (int)p.tens_num && b >= p.t[i].blk0) ti = i;
  ti = __builtin_amdgcn_readfirstlane(ti);
  accum_tensor_t const t = p.t[ti];
  unsigned const base = (b - t.blk0) * SOLVER_CHUNK;
  if (base >= t.n) return;   // (never: the grid is the sum of the chunks)
  unsigned const cnt = (t.n - base < SOLVER_CHUNK) ? (t.n - base) : SOLVER_CHUNK;
  bool const first = p.accum[0] != 0.0f;   // (the same word for every lane of the launch)
  float const *const g = t.g + base; float *const a = t.a + base;
  unsigned const tid = threadIdx.x;
  unsigned done = 0;   // elements of the chunk covered by quads
  if (t.quads) {
    unsigned const nq = cnt / 4;
    float4 G[4], A[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      unsigned const q = tid + 256u * j;
      if (q < nq) {
        G[j] = ((float4 const *)g)[q];
        if (!first) A[j] = ((float4 const *)a)[q];
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      unsigned const q = tid + 256u * j;
      if (q < nq) {
        float4 r = G[j];
        if (!first) { r.x = A[j].x + G[j].x; r.y = A[j].y + G[j].y; r.z = A[j].z + G[j].z; r.w = A[j].w + G[j].w; }
        ((float4 *)a)[q] = r;
      }
    }
    done = nq * 4;
  }
  for (unsigned e = done + tid; e < cnt; e += 256) {
    float r = g[e];
    if (!first) r = a[e] + r;
    a[e] = r;
  }
}
#endif
