// gemm_conv_bf16.hip -- bf16-operand / fp32-accumulate MFMA contraction for gfx950 (BASELINE config 5), hiprtc-specialised.
//
//   D[i][j] = sum_k bf16(I(k,i)) * bf16(J(k,j))     fp32 accumulate  (+ bias[i], ReLU for convolutions)
//
// Same contract, operand roles, layouts-in-HBM (fp32, reference layout) and epilogue as gemm_conv_f32.hip; what changes is
// the matrix instruction (v_mfma_f32_32x32x16_bf16: 16 k per instruction, 16x the fp32 MFMA rate) and therefore the
// on-chip data path:
//   * operands are converted fp32 -> bf16 (round-to-nearest-even, v_cvt_pk_bf16_f32) while being staged, never in HBM;
//   * LDS images are x-major with k contiguous, [BX][BK+8] bf16 (80-B row pitch for BK=32: conflict-free ds_read_b128 of the
//     8-bf16 MFMA fragments: lane l reads row l&31, k = 16*kk + 8*(l>>5) .. +7);
//   * staging is column-per-thread for EVERY operand kind: a thread owns one i (or j) and 8 consecutive k, i.e. exactly one
//     16-byte LDS chunk -> one ds_write_b128 per 8 loaded values.  For the conv gather this is the natural shape (fixed
//     output position, consecutive (in_chan,ky,kx) from the scalar-cache table); k-major sgemm operands are read as 8
//     wave-coalesced dword loads per chunk.
// With 16x less matrix time per k the kernel is bound by the staging instruction stream / HBM, not the MFMA pipe
// (DESIGN.md section 3.3); it exists to serve config 5 and to put a measured bf16 number on the table.
//
// Numerics: products of bf16 values are exact in fp32; the 16-term sums inside one MFMA are not a sequential fma chain,
// so results are NOT bit-comparable with a CPU loop; parity is stated against an oracle fed the same bf16-rounded inputs
// (tolerance 2e-4) and, informationally, against the fp32 reference (normalised RMS error).  The reference has no bf16:
// parity is unpinned for this kernel by construction.
//
// -D parameters: KNAME BI BJ BK(32|64) WI WJ MINW I_MODE(0 k-major | 2 x-major float4 | 3 x-major scalar)
//                J_MODE(0 k-major | 2 gather | 3 x-major float4 | 4 x-major scalar | 5 1x1/no-pad) EPI [KH KW SY SX PY PX RELU]

#ifndef __HIPCC_RTC__
#include <hip/hip_runtime.h>
#endif
#include "kernel_args.h"      // gemm_args_t (D_bytes, bsI / bsJ / bsD: not read here)
#include "device_prelude.h"

#ifndef KNAME
#define KNAME bodahip_gemm_bf16
#endif
#ifndef GROUP_I
#define GROUP_I 8
#endif
#ifndef KH
#define KH 1
#define KW 1
#define SY 1
#define SX 1
#define PY 0
#define PX 0
#endif
#ifndef RELU
#define RELU 0
#endif
#ifndef SWAPST
#define SWAPST ((BJ / (WJ * 32)) % 2 == 0)
#endif
#ifndef SPLITK
#define SPLITK 0 // 1: the grid is tiles x p.splitk; slice s accumulates K-tiles [s*kt_per, (s+1)*kt_per) and stores its raw partial tile to slab s
#endif           // of p.ws; bodahip_splitk_reduce (gemm_conv_f32.hip) sums the slabs and applies the epilogue.  Chosen by the host for
                 // tile-starved shapes with a long K (fully-connected layers): this path is not order-exact anyway.

namespace {
constexpr int kNT = WI * WJ * 64;
constexpr int kTI = BI / (WI * 32);
constexpr int kTJ = BJ / (WJ * 32);
constexpr int kPitch = BK + 8;                  // bf16 elements per LDS row (16-B aligned, de-phased banks)
constexpr int kITile = BI * kPitch, kJTile = BJ * kPitch; // bf16 elements
constexpr int kCI = BI * BK / 8 / kNT;           // 8-k chunks per thread, operand I
constexpr int kCJ = BJ * BK / 8 / kNT;
static_assert(BK == 32 || BK == 64, "BK must be 32 or 64");
static_assert(BI % (WI * 32) == 0 && BJ % (WJ * 32) == 0, "tile must be a multiple of 32 per wave");
static_assert((BI * BK / 8) % kNT == 0 && (BJ * BK / 8) % kNT == 0, "chunks must split evenly over the threads");
static_assert(BJ % 64 == 0 || (J_MODE != 2 && J_MODE != 5), "gather: BJ must be a multiple of 64 (wave-uniform k chunk)");

constexpr int kOOB = (int)0x80000000;
constexpr int kKTail = 0x7ffffff0;

// one chunk = column x (tile-relative xr), k = k0 + 8*kc .. +7.  chunk index c = tid + p*kNT: xr = c % BX, kc = c / BX.
template <int MODE, int BX, int NCH>
__device__ __forceinline__ void load_plain(float (&r)[NCH * 8], rsrc_t P, int ld, int x0, int X, int k0, int K, int tid) {
#pragma unroll
  for (int p = 0; p < NCH; ++p) {
    int const c = tid + p * kNT, xr = c % BX, kc = c / BX;
    int const x = x0 + xr, kb = k0 + 8 * kc;
    if constexpr (MODE == 0) {          // k-major: P[k*ld + x]; 8 wave-coalesced dword loads
#pragma unroll
      for (int e = 0; e < 8; ++e) r[p * 8 + e] = bload1(P, ((kb + e < K) && (x < X)) ? (((kb + e) * ld + x) * 4) : kOOB);
    } else if constexpr (MODE == 2) {   // x-major, k contiguous, K % 4 == 0: two float4
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        f32x4 const v = bload4(P, ((x < X) && (kb + 4 * h < K)) ? ((x * ld + kb + 4 * h) * 4) : kOOB);
        r[p * 8 + 4 * h + 0] = v[0]; r[p * 8 + 4 * h + 1] = v[1]; r[p * 8 + 4 * h + 2] = v[2]; r[p * 8 + 4 * h + 3] = v[3];
      }
    } else {                            // x-major scalar
#pragma unroll
      for (int e = 0; e < 8; ++e) r[p * 8 + e] = bload1(P, ((x < X) && (kb + e < K)) ? ((x * ld + kb + e) * 4) : kOOB);
    }
  }
}

#if J_MODE == 2 || J_MODE == 5
struct gather_t { int base; int iy0, ix0; }; // base: element offset (J_MODE 2) or byte offset (J_MODE 5)
__device__ __forceinline__ void load_gather(float (&r)[kCJ * 8], rsrc_t in, gather_t const &g, gemm_args_t const &p, int k0, int tid) {
#pragma unroll
  for (int q = 0; q < kCJ; ++q) {
    int const kc = __builtin_amdgcn_readfirstlane((tid + q * kNT) / BJ); // wave-uniform (BJ % 64 == 0)
    int const kb = k0 + 8 * kc;
#if J_MODE == 5
    int const hw4 = p.H * p.W * 4;
#pragma unroll
    for (int e = 0; e < 8; ++e) { int const soff = (kb + e < p.K) ? (kb + e) * hw4 : kKTail; r[q * 8 + e] = bload1(in, g.base + soff); }
#else
    typedef int4 const __attribute__((address_space(4))) *ctab_t;
    ctab_t const t_off = (ctab_t)(p.ktab + kb), t_ky = (ctab_t)(p.ktab + p.ktab_n + kb), t_kx = (ctab_t)(p.ktab + 2 * p.ktab_n + kb);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      int4 const ko = t_off[h], ky = t_ky[h], kx = t_kx[h];
      int const kov[4] = {ko.x, ko.y, ko.z, ko.w}, kyv[4] = {ky.x, ky.y, ky.z, ky.w}, kxv[4] = {kx.x, kx.y, kx.z, kx.w};
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        int const iy = g.iy0 + kyv[e], ix = g.ix0 + kxv[e];
        int off = (g.base + kov[e]) * 4;
        asm volatile("" : "+v"(off));
        bool const ok = ((unsigned)iy < (unsigned)p.H) && ((unsigned)ix < (unsigned)p.W);
        r[q * 8 + h * 4 + e] = bload1(in, ok ? off : kOOB);
      }
    }
#endif
  }
}
#define GATHER_ARG , g
#define GATHER_PARM , gather_t const &g
#else
#define GATHER_ARG
#define GATHER_PARM
#endif

// registers -> LDS: convert 8 fp32 to one 16-byte bf16 chunk (round-to-nearest-even)
template <int BX, int NCH>
__device__ __forceinline__ void store_chunks(float const (&r)[NCH * 8], __bf16 *__restrict__ S, int tid) {
#pragma unroll
  for (int p = 0; p < NCH; ++p) {
    int const c = tid + p * kNT, xr = c % BX, kc = c / BX;
    bf16x8 v;
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = (__bf16)r[p * 8 + e];
    *reinterpret_cast<bf16x8 *>(S + xr * kPitch + 8 * kc) = v;
  }
}

__device__ __forceinline__ void load_I(float (&ri)[kCI * 8], rsrc_t I, gemm_args_t const &p, int i0, int k0, int tid) {
  load_plain<I_MODE, BI, kCI>(ri, I, p.ldI, i0, p.Mi, k0, p.K, tid);
}
__device__ __forceinline__ void load_J(float (&rj)[kCJ * 8], rsrc_t J, gemm_args_t const &p, int j0, int k0, int tid GATHER_PARM) {
#if J_MODE == 2 || J_MODE == 5
  load_gather(rj, J, g, p, k0, tid);
#elif J_MODE == 3 || J_MODE == 4
  load_plain<J_MODE - 1, BJ, kCJ>(rj, J, p.ldJ, j0, p.Nj, k0, p.K, tid);
#else
  load_plain<0, BJ, kCJ>(rj, J, p.ldJ, j0, p.Nj, k0, p.K, tid);
#endif
}
} // namespace

extern "C" __global__ __launch_bounds__(WI * WJ * 64, MINW) void KNAME(gemm_args_t const p) {
  __shared__ __attribute__((aligned(16))) __bf16 smem[2 * (kITile + kJTile)];
  int const tid = threadIdx.x, lane = tid & 63;
  int const wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  int const wi = wave / WJ, wj = wave % WJ;

  int tile_i, tile_j; // XCD-aware workgroup -> tile map, as in gemm_conv_f32.hip
  {
#if SPLITK
    int const bid = blockIdx.x / p.splitk;
#else
    int const bid = blockIdx.x;
#endif
    int const nb = p.tiles_i * p.tiles_j;
    int const q = nb >> 3, rr = nb & 7, xcd = bid & 7, idx = bid >> 3;
    int const nid = ((xcd < rr) ? xcd * (q + 1) : rr * (q + 1) + (xcd - rr) * q) + idx;
    int const group_sz = GROUP_I * p.tiles_j, gid = nid / group_sz, first_i = gid * GROUP_I;
    int const gsz = min(p.tiles_i - first_i, GROUP_I), in_g = nid - gid * group_sz;
    tile_i = first_i + in_g % gsz; tile_j = in_g / gsz;
  }
  int const i0 = tile_i * BI, j0 = tile_j * BJ;
  __bf16 *const Is0 = smem, *const Is1 = smem + kITile, *const Js0 = smem + 2 * kITile, *const Js1 = smem + 2 * kITile + kJTile;

#if J_MODE == 2 || J_MODE == 5
  gather_t g;
  {
    int const OHW = p.OH * p.OW;
    int const jg = j0 + (tid % BJ);
    int const img = jg / OHW, pel = jg - img * OHW, oy = pel / p.OW, ox = pel - oy * p.OW;
#if J_MODE == 5
    g.base = (jg < p.Nj) ? (((img * p.C * p.H + oy * SY) * p.W + ox * SX) * 4) : kOOB; g.iy0 = 0; g.ix0 = 0;
#else
    g.iy0 = (jg < p.Nj) ? (oy * SY - PY) : (1 << 29);
    g.ix0 = ox * SX - PX;
    g.base = (img * p.C * p.H + (oy * SY - PY)) * p.W + g.ix0;
#endif
  }
#endif

  f32x16 acc[kTI][kTJ];
#pragma unroll
  for (int a = 0; a < kTI; ++a)
#pragma unroll
    for (int b = 0; b < kTJ; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;

  float ri[kCI * 8], rj[kCJ * 8];
  int const nkt_all = (p.K + BK - 1) / BK;
#if SPLITK
  int const slice = blockIdx.x % p.splitk;
  int const kt_begin = slice * p.kt_per;
  int const nkt = max(0, min(nkt_all, kt_begin + p.kt_per) - kt_begin);
#else
  int const kt_begin = 0, nkt = nkt_all;
#endif
  rsrc_t const rI = make_rsrc(p.I, p.I_bytes), rJ = make_rsrc(p.J, p.J_bytes);
  load_I(ri, rI, p, i0, kt_begin * BK, tid);
  load_J(rj, rJ, p, j0, kt_begin * BK, tid GATHER_ARG);
  store_chunks<BI, kCI>(ri, Is0, tid);
  store_chunks<BJ, kCJ>(rj, Js0, tid);
  __syncthreads();

  // fragment fetch: lane l holds A[i = l&31][k = 8*(l>>5) .. +7] (and B alike) for each 16-deep MFMA step
  int const a_off = (wi * (kTI * 32) + (lane & 31)) * kPitch + 8 * (lane >> 5);
  int const b_off = (wj * (kTJ * 32) + (lane & 31)) * kPitch + 8 * (lane >> 5);

  for (int kt = 0; kt < nkt; ++kt) {
    bool const more = (kt + 1) < nkt;
    __bf16 const *const Ic = ((kt & 1) ? Is1 : Is0) + a_off;
    __bf16 const *const Jc = ((kt & 1) ? Js1 : Js0) + b_off;
    if (more) {
      load_I(ri, rI, p, i0, (kt_begin + kt + 1) * BK, tid);
      load_J(rj, rJ, p, j0, (kt_begin + kt + 1) * BK, tid GATHER_ARG);
    }
#pragma unroll
    for (int kk = 0; kk < BK / 16; ++kk) {
      bf16x8 a[kTI], b[kTJ];
#pragma unroll
      for (int t = 0; t < kTI; ++t) a[t] = *reinterpret_cast<bf16x8 const *>(Ic + t * 32 * kPitch + kk * 16);
#pragma unroll
      for (int t = 0; t < kTJ; ++t) b[t] = *reinterpret_cast<bf16x8 const *>(Jc + t * 32 * kPitch + kk * 16);
#pragma unroll
      for (int ta = 0; ta < kTI; ++ta)
#pragma unroll
        for (int tb = 0; tb < kTJ; ++tb) acc[ta][tb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[ta], b[tb], acc[ta][tb], 0, 0, 0);
    }
    if (more) {
      store_chunks<BI, kCI>(ri, (kt & 1) ? Is0 : Is1, tid);
      store_chunks<BJ, kCJ>(rj, (kt & 1) ? Js0 : Js1, tid);
    }
    __syncthreads();
  }

#if SPLITK
  { // raw partial tiles into this slice's slab, indexed like D (bias / ReLU happen in the reduce kernel)
    float *const Dp = p.ws + (long)slice * p.ws_slab;
#pragma unroll
    for (int tb = 0; tb < kTJ; ++tb) {
      int const jg = j0 + wj * (kTJ * 32) + tb * 32 + (lane & 31);
      if (jg >= p.Nj) continue;
#if EPI == 1
      int const OHW = p.OH * p.OW;
      int const img = jg / OHW, pel = jg - img * OHW;
      long const joff = (long)img * p.Mi * OHW + pel, istride = OHW;
#else
      long const joff = jg, istride = p.ldD;
#endif
#pragma unroll
      for (int ta = 0; ta < kTI; ++ta)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          int const ig = i0 + wi * (kTI * 32) + ta * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
          if (ig < p.Mi) Dp[joff + (long)ig * istride] = acc[ta][tb][r];
        }
    }
  }
#else
  // epilogue (as in gemm_conv_f32.hip): C/D layout of the 32x32 MFMA family: column j = lane&31, row i = (r&3) + 8*(r>>2) + 4*(lane>>5).
  // Biases of this lane's kTI*16 rows fetched up front, buffer stores with 32-bit offsets (per-lane column part + wave-uniform
  // per-row part in the scalar offset operand); branch-free for tiles inside the row range.
  {
    rsrc_t const rD = make_rsrc(p.D, p.D_bytes);
#if EPI == 1
    rsrc_t const rB = make_rsrc(p.bias, (unsigned)p.Mi * 4u);
    unsigned const S4 = (unsigned)(p.OH * p.OW) * 4u;
#else
    unsigned const S4 = (unsigned)p.ldD * 4u;
#endif
    int const ib = i0 + wi * (kTI * 32) + 4 * (lane >> 5);
    auto rowc = [](int ta, int r) { return ta * 32 + (r & 3) + 8 * (r >> 2); };
    unsigned const ipart = (unsigned)ib * S4;
#if EPI == 1
    float bv[kTI][16];
#pragma unroll
    for (int ta = 0; ta < kTI; ++ta)
#pragma unroll
      for (int r = 0; r < 16; ++r) bv[ta][r] = bload1(rB, (ib + rowc(ta, r)) * 4);
#endif
#if SWAPST
    // paired 256-byte row stores (see gemm_conv_f32.hip): bias / ReLU in the MFMA layout, then v_permlane32_swap so that one register
    // holds 64 consecutive pels of row i and the other of row i+4
    auto store_all = [&](bool const edge) {
      int const ibl = i0 + wi * (kTI * 32);
#pragma unroll
      for (int tp = 0; tp < kTJ / 2; ++tp) {
        int const jg = j0 + wj * (kTJ * 32) + tp * 64 + lane;
#if EPI == 1
        int const OHW = p.OH * p.OW;
        int const img = jg / OHW, pel = jg - img * OHW;
        unsigned const jpart = (jg < p.Nj) ? ((((unsigned)img * (unsigned)p.out_ctot + (unsigned)p.out_coff) * (unsigned)OHW + (unsigned)pel) * 4u + (unsigned)ibl * S4) : 0x80000000u;
#else
        unsigned const jpart = (jg < p.Nj) ? ((unsigned)jg * 4u + (unsigned)ibl * S4) : 0x80000000u;
#endif
#pragma unroll
        for (int ta = 0; ta < kTI; ++ta)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            float va = acc[ta][2 * tp][r], vb = acc[ta][2 * tp + 1][r];
#if EPI == 1
            va = va + bv[ta][r]; vb = vb + bv[ta][r];
#if RELU
            va = (va > 0.f) ? va : 0.f; vb = (vb > 0.f) ? vb : 0.f;
#endif
#endif
            auto const sw = __builtin_amdgcn_permlane32_swap(__builtin_bit_cast(unsigned, va), __builtin_bit_cast(unsigned, vb), false, false);
            int const rc = rowc(ta, r);
            if (!(edge && (ibl + rc >= p.Mi))) __builtin_amdgcn_raw_buffer_store_b32((int)sw[0], rD, (int)jpart, (int)((unsigned)rc * S4), 0);
            if (!(edge && (ibl + rc + 4 >= p.Mi))) __builtin_amdgcn_raw_buffer_store_b32((int)sw[1], rD, (int)jpart, (int)((unsigned)(rc + 4) * S4), 0);
          }
      }
    };
#else
    auto store_all = [&](bool const edge) {
#pragma unroll
      for (int tb = 0; tb < kTJ; ++tb) {
        int const jg = j0 + wj * (kTJ * 32) + tb * 32 + (lane & 31);
        if (jg >= p.Nj) continue;
#if EPI == 1
        int const OHW = p.OH * p.OW;
        int const img = jg / OHW, pel = jg - img * OHW;
        unsigned const jpart = (((unsigned)img * (unsigned)p.out_ctot + (unsigned)p.out_coff) * (unsigned)OHW + (unsigned)pel) * 4u;
#else
        unsigned const jpart = (unsigned)jg * 4u;
#endif
#pragma unroll
        for (int ta = 0; ta < kTI; ++ta)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            if (edge && (ib + rowc(ta, r) >= p.Mi)) continue;
            float v = acc[ta][tb][r];
#if EPI == 1
            v = v + bv[ta][r];
#if RELU
            v = (v > 0.f) ? v : 0.f;
#endif
#endif
            __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(int, v), rD, (int)(jpart + ipart), (int)((unsigned)rowc(ta, r) * S4), 0);
          }
      }
    };
#endif
    if (i0 + BI <= p.Mi) store_all(false); else store_all(true); // workgroup-uniform
  }
#endif // SPLITK
}
