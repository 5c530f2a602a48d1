// data_f32.hip -- the input transform of the gradient pipe (family `data`), for gfx950; specialised by hiprtc.  One function, this backend's own: Caffe's
// DataTransformer (crop, mirror, mean, scale) from uint8 images into the pipe's float `data` node.  The file is compiled with contraction and reassociation off.  Every
// store is a per-lane vector store, every output element has one owner, there are no atomics.  The same operations in the same order run on be=cpu
// (csrc/cpu_compute.cc) and in the numpy twin (tests/data_ref.py).
//
// bodahip_data_transform   src (uint8 img:y:x:chan, or img:chan:y:x under -DCHW=1, at the source size H x W), plan (uint32 img:v=4 = [y_off, x_off, mirror, unused]),
//   mean (float chan, or chan:y:x at the SOURCE size under -DMEAN_PEL=1) -> out (float img:chan:y:x at the crop size ch x cw, ch <= H, cw <= W)
//   Per output element (i, c, y, x):
//     yo = min(plan[i][0], H - ch);  xo = min(plan[i][1], W - cw);  m = plan[i][2] != 0
//     sy = yo + y;  sx = xo + (m ? cw - 1 - x : x)
//     v = (float)src[i, sy, sx, c]                 exact
//     mu = mean[c]  or  mean[c, sy, sx]            the mean at the SOURCE position, as Caffe indexes it
//     d = v - mu;  out = d * scale                 two fp32 roundings
//   The clamps are part of the rule: no plan word makes the kernel read outside src.  plan[i][3] is not read.
//   Layout: a thread owns four consecutive elements of the FLAT out tensor, whose base is 16-byte aligned: one 16-byte store per lane whatever cw is; the last thread of
//   a tensor whose size is no multiple of four stores dwords.  The first element is decoded with 64-bit divisions, the next three by carrying x -> y -> c -> i, so a
//   thread's four may straddle a row, a plane or an image.  The source bytes are gathered one by one through the cache: along a row the lanes of a wave read
//   neighbouring (planar) or C-strided (interleaved) bytes of a few cache lines.  All indices are 64-bit.
//
// -D parameters: KNAME CHW MEAN_PEL.  Host side: data_op_of_op (rtc_types.h), plan_data_op (native_plan.cc), native_kernels_t::data_call (native_kernels.cc), the argument
// checks in native_run.cc.

#ifndef __HIPCC_RTC__
#include <hip/hip_runtime.h>
#endif

#pragma clang fp contract(off) reassociate(off)

#include "kernel_args.h"      // data_transform_args_t
#include "device_prelude.h"

#if !defined(CHW) || !defined(MEAN_PEL)
#error "data_f32.hip: -DCHW=0|1 -DMEAN_PEL=0|1"
#endif

extern "C" __global__ __launch_bounds__(256) void KNAME(data_transform_args_t const p) {
  long const e0 = ((long)blockIdx.x * 256 + threadIdx.x) * 4;   // the first of this thread's four flat elements
  if (e0 >= p.n) return;
  long r = e0 / p.cw;
  int x = (int)(e0 - r * p.cw);
  long q = r / p.ch;
  int y = (int)(r - q * p.ch);
  long i = q / p.C;
  int c = (int)(q - i * p.C);
  int const cnt = (p.n - e0 < 4) ? (int)(p.n - e0) : 4;
  float o[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (k < cnt) {
      unsigned const *const pl = p.plan + i * 4;
      unsigned const ymax = (unsigned)(p.H - p.ch), xmax = (unsigned)(p.W - p.cw);
      unsigned const yo = pl[0] < ymax ? pl[0] : ymax, xo = pl[1] < xmax ? pl[1] : xmax;
      long const sy = (long)yo + y, sx = (long)xo + ((pl[2] != 0u) ? (p.cw - 1 - x) : x);
#if CHW
      long const si = ((i * p.C + c) * p.H + sy) * p.W + sx;
#else
      long const si = ((i * p.H + sy) * p.W + sx) * p.C + c;
#endif
#if MEAN_PEL
      float const mu = p.mean[((long)c * p.H + sy) * p.W + sx];
#else
      float const mu = p.mean[c];
#endif
      float const v = (float)p.src[si];
      float const d = v - mu;
      o[k] = d * p.scale;
      if (++x == p.cw) { x = 0; if (++y == p.ch) { y = 0; if (++c == p.C) { c = 0; ++i; } } }
    }
  }
  if (cnt == 4) {
    f32x4 w; w.x = o[0]; w.y = o[1]; w.z = o[2]; w.w = o[3];
    *(f32x4 *)(p.out + e0) = w;
  } else {
    for (int k = 0; k < cnt; ++k) p.out[e0 + k] = o[k];
  }
}
