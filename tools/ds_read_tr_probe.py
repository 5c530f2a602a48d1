#!/usr/bin/env python3
"""Lane mapping of ds_read_b64_tr_b16 (gfx950): LDS is filled with the index of every 16-bit element, lane l reads at byte address 8 * l (elements 4l .. 4l + 3),
and the four elements each lane receives are dumped.  From the dump: which lane's address feeds which lane's result, i.e. how a [k][channel] image has to be addressed
so that a lane ends up with consecutive k of one channel (kernels/bconv_fb_nhwc_bf16.hip).  A second read with a row pitch (lane l reads row
(l % 16) / 4 of a 16-lane block) checks the addressing the kernel uses.  (MI355X)  usage: python tools/ds_read_tr_probe.py"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from boda_amd.op import Dims, Op
from boda_amd.rtc import RtcArg, RtcFuncCall, RtcFuncInfo, make_rtc

SRC = """
typedef short s16x4 __attribute__((ext_vector_type(4)));
extern "C" __global__ void tr_probe( int * out ) {
  __shared__ __attribute__((aligned(16))) short lds[1024];
  int const l = threadIdx.x;
  for( int i = l; i < 1024; i += 64 ) lds[i] = (short)i;
  __syncthreads();
  // (a) lane l -> elements 4l .. 4l+3
  s16x4 const a = __builtin_amdgcn_ds_read_tr16_b64_v4i16( (__attribute__((address_space(3))) s16x4 *)( lds + 4 * l ) );
  // (b) the kernel's addressing: a [k][64 channels] image, lane l of a 16-lane block reads row k = (l % 16) / 4 (+ 4 for the second read), channels 4 * (l % 4) .. + 3
  //     of the block's 16 channels 16 * ((l / 16) % 2); k group 8 * (l / 32)
  int const t = l & 15, k = ( t >> 2 ) + 8 * ( l >> 5 ), ch = 16 * ( ( l >> 4 ) & 1 ) + 4 * ( t & 3 );
  s16x4 const b = __builtin_amdgcn_ds_read_tr16_b64_v4i16( (__attribute__((address_space(3))) s16x4 *)( lds + k * 64 + ch ) );
  for( int j = 0; j < 4; ++j ) { out[l * 4 + j] = a[j]; out[256 + l * 4 + j] = b[j]; }
}
"""
rtc = make_rtc("(be=hip)", 0); rtc.init()
rtc.compile([RtcFuncInfo("tr_probe", SRC, ["out"], Op({"type": "probe", "func_name": "tr_probe"}, {}))])
rtc.create_var_with_dims("o", Dims.make("int32_t", x=512))
rtc.run(RtcFuncCall("tr_probe", {"out": RtcArg.var("o")}, tpb=64, blks=1)); rtc.finish_and_sync()
o = rtc.copy_var_to_nda("o").reshape(2, 64, 4)
print("(a) lane l reads elements 4l..4l+3; lane: the four elements received (element e = 4 * source lane + position)")
for l in range(64):
    print(f"  lane {l:2d}: " + " ".join(f"{int(v):4d}" for v in o[0, l]) + "    source lanes " + " ".join(f"{int(v) // 4:2d}.{int(v) % 4}" for v in o[0, l]))
print("(b) [k][64] image, lane reads (k = (l%16)/4 + 8*(l/32), ch = 16*((l/16)%2) + 4*(l%4)); lane: (k, channel) of the four elements received")
for l in range(64):
    print(f"  lane {l:2d}: " + " ".join(f"({int(v) // 64:2d},{int(v) % 64:2d})" for v in o[1, l]))
want = np.array([[[(j + 8 * (l >> 5)) * 64 + (l & 31)] for j in range(4)] for l in range(64)]).reshape(64, 4)
print("(b) gives lane l channel l % 32 at k = 8 * (l / 32) + 0..3:", bool((o[1] == want).all()))
rtc.release_var("o"); rtc.close()
