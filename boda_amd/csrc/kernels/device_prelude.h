// device_prelude.h -- what the kernel sources share on the device side only: vector types, the buffer resource and the buffer loads.  Included by every kernels/*.hip
// after kernel_args.h (and after the HIP runtime header of an offline compile: __device__ / __forceinline__ come from there).
#ifndef BODAHIP_DEVICE_PRELUDE_H
#define BODAHIP_DEVICE_PRELUDE_H

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x3 __attribute__((ext_vector_type(3)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x3 __attribute__((ext_vector_type(3)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef short s16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 h16x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) void *lds_t;

// A wave-uniform buffer resource over `bytes` bytes at p: loads at an offset >= bytes return 0, stores there are dropped (raw buffer, 32-bit offsets)
typedef __amdgpu_buffer_rsrc_t rsrc_t;
__device__ __forceinline__ rsrc_t make_rsrc(void const *p, unsigned bytes) { return __builtin_amdgcn_make_buffer_rsrc((void *)p, 0, (int)bytes, 0x00020000); }
// 1 / 2 / 3 / 4 dwords at byte offset voff (per lane) + soff (wave-uniform), as floats; bload4u: the four dwords as they are
// (whole-vector bit_casts: element-wise bit_casts of the b64/b96 results get mis-shrunk to a 1-dword load by this compiler)
__device__ __forceinline__ float bload1(rsrc_t r, int voff, int soff = 0) { return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, voff, soff, 0)); }
__device__ __forceinline__ f32x2 bload2(rsrc_t r, int voff, int soff = 0) { return __builtin_bit_cast(f32x2, __builtin_amdgcn_raw_buffer_load_b64(r, voff, soff, 0)); }
__device__ __forceinline__ f32x3 bload3(rsrc_t r, int voff) { return __builtin_bit_cast(f32x3, __builtin_amdgcn_raw_buffer_load_b96(r, voff, 0, 0)); }
__device__ __forceinline__ f32x4 bload4(rsrc_t r, int voff, int soff = 0) { return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r, voff, soff, 0)); }
__device__ __forceinline__ u32x4 bload4u(rsrc_t r, int voff) { return __builtin_amdgcn_raw_buffer_load_b128(r, voff, 0, 0); }

#endif // BODAHIP_DEVICE_PRELUDE_H
