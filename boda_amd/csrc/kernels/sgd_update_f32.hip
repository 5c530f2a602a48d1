// sgd_update_f32.hip -- the SGD update of the gradient pipe (function hip_sgd_update, op type SgdUpdate), fp32, for gfx950; specialised by hiprtc.
// This backend's own arithmetic (the reference has no solver): Caffe's SGD order -- regularise, history, update -- with the gradient left unmodified.  ONE launch
// updates up to 32 tensors of any size: the at most 24 / 16 / 100+ params of NiN / AlexNet / GoogLeNet are half bias vectors of 10 .. 4096 floats, for which a launch
// of their own is pure launch floor.
//
// Per element of tensor i, every operation a separate fp32 rounding (the file is compiled with contraction and reassociation off; be=cpu runs the same chain):
//     lr_i = lr * lr_mult_i            wd_i = weight_decay * decay_mult_i     (one multiply each, the same for every element)
//     g1   = g + wd_i * w                                                     (always computed, also when wd_i == 0)
//     h'   = momentum * h + lr_i * g1                                         (two products, then one add)
//     w'   = w - h'
//     store h', store w'                                                      (g is only read)
//   * lr, momentum, weight_decay are the first three floats of `hyper`, a 4-float tensor in device memory read with ordinary loads: a captured launch (hipGraph)
//     freezes the by-value table below, not those words, so a learning-rate schedule needs no new capture
//   * the table of tensors rides BY VALUE in the kernel arguments: per tensor three pointers, the element count, the first workgroup index (a prefix sum over the
//     tensors' chunk counts), lr_mult, decay_mult and a flag "quads allowed".  Nothing has to be resident on the device before the launch
//   * a workgroup of 256 threads owns one chunk of CHUNK = 4096 consecutive floats of ONE tensor (the last chunk of a tensor is ragged).  It finds its tensor by a scan of
//     the at most 32 prefix entries with blockIdx.x alone: the index is the same in every lane (and passed through readfirstlane so the compiler knows), the table is
//     read with scalar loads
//   * quads allowed (the host sets it where w, g and h are all 16-byte aligned; a chunk starts at a multiple of 4096 floats, so every chunk is then aligned too): a
//     thread takes up to four float4 of each of w, g, h -- quads tid, tid + 256, tid + 512, tid + 768 of the chunk -- and issues all of those loads before its first
//     store; the up to three elements behind the chunk's last whole quad are scalars.  Not allowed: the whole chunk is scalars, 16 per thread
//   * one owner per element, which reads its element before it writes it; every store is a per-lane vector store; nothing else is written
//
// -D parameters: KNAME.  Host side: plan_sgd_update (native_plan.cc), native_kernels_t::sgd_update (native_kernels.cc), the argument checks in native_run.cc.

#ifndef __HIPCC_RTC__
#include <hip/hip_runtime.h>
#endif

#pragma clang fp contract(off) reassociate(off)

#include "kernel_args.h"      // sgd_tensor_t, sgd_update_args_t, kSgdMaxTens
#define SGD_CHUNK 4096

struct sgd_coef_t { float lr, wd, mom; };

static __device__ __forceinline__ void sgd_one(float w, float g, float h, sgd_coef_t const c, float &w2, float &h2) {
  float const reg = c.wd * w;
  float const g1 = g + reg;
  float const a = c.mom * h;
  float const b = c.lr * g1;
  h2 = a + b;
  w2 = w - h2;
}

extern "C" __global__ __launch_bounds__(256) void KNAME(sgd_update_args_t const p) {
  unsigned const b = blockIdx.x;
  int ti = 0;
#pragma unroll
  for (int i = 1; i < kSgdMaxTens; ++i) if (i < (int)p.tens_num && b >= p.t[i].blk0) ti = i;
  ti = __builtin_amdgcn_readfirstlane(ti);
  sgd_tensor_t const t = p.t[ti];
  unsigned const base = (b - t.blk0) * SGD_CHUNK;
  if (base >= t.n) return;   // (never: the grid is the sum of the chunks)
  unsigned const cnt = (t.n - base < SGD_CHUNK) ? (t.n - base) : SGD_CHUNK;
  float const lr = p.hyper[0], mom = p.hyper[1], wd = p.hyper[2];
  sgd_coef_t c; c.lr = lr * t.lr_mult; c.wd = wd * t.decay_mult; c.mom = mom;
  float *const w = t.w + base; float const *const g = t.g + base; float *const h = t.h + base;
  unsigned const tid = threadIdx.x;
  unsigned done = 0;   // elements of the chunk covered by quads
  if (t.quads) {
    unsigned const nq = cnt / 4;
    float4 W[4], G[4], H[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      unsigned const q = tid + 256u * k;
      if (q < nq) { W[k] = ((float4 const *)w)[q]; G[k] = ((float4 const *)g)[q]; H[k] = ((float4 const *)h)[q]; }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      unsigned const q = tid + 256u * k;
      if (q < nq) {
        float4 w2, h2;
        sgd_one(W[k].x, G[k].x, H[k].x, c, w2.x, h2.x);
        sgd_one(W[k].y, G[k].y, H[k].y, c, w2.y, h2.y);
        sgd_one(W[k].z, G[k].z, H[k].z, c, w2.z, h2.z);
        sgd_one(W[k].w, G[k].w, H[k].w, c, w2.w, h2.w);
        ((float4 *)h)[q] = h2; ((float4 *)w)[q] = w2;
      }
    }
    done = nq * 4;
  }
  for (unsigned e = done + tid; e < cnt; e += 256) {
    float w2, h2;
    sgd_one(w[e], g[e], h[e], c, w2, h2);
    h[e] = h2; w[e] = w2;
  }
}
