// cpu_compute.cc -- cpu_compute_t: `be=cpu`, the host-cores counterpart of be=hip behind the SAME rtc_compute_t contract and C ABI.
//
// the reference has no CPU conv / sgemm path to time beside the GPU (its only precedent is a bare cblas_sgemm
// loop, src/qblas-test.cc:33-41), so the CPU baseline of bench.py is this backend: cache-blocked, vectorised (AVX-512 or AVX2, chosen at
// init), OpenMP over all host cores, fp32, same epilogue -- reached exactly like the GPU kernels, through the native side door
// (op.func_name hip_sgemm / hip_conv, aliases cublas_sgemm / cudnn_conv; tensors in reference layout: a K:M, b K:N, c M:N; in / out
// img:chan:y:x, filts out_chan:in_chan:y:x).  It is a backend one SELECTS (`(be=cpu)`); be=hip never falls back to it.
//   * vars are host buffers (64-byte aligned, zero-filled); copy_nda_to_var / copy_var_to_nda are memcpys; get_dur() from steady_clock
//   * compile(): only the native function names; CUCL source cannot run on a CPU -> unsup_err (the reference's harness records such
//     failures and moves on, src/rtc_prof.cc:287-296)
// Numerics: every output is ONE fp32 fma chain in ascending k (K blocking continues the chain through the tile's partial sums), bias added
// after the chain, then ReLU -- bit-identical to the reference's per-thread fmaf loop, hence to the oracle and to be=hip's fp32 kernels
// (tests/test_cpu_backend.py).
//
// Built with g++ (-fopenmp), linked into libbodahip.so (boda_amd/build.py).
#include "rtc_types.h"

#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <cmath>
#include <cstring>
#include <omp.h>
#include <vector>

namespace bodahip {

namespace {
typedef float vf __attribute__((vector_size(64), aligned(4)));   // 16 floats: one zmm, or two ymm under the AVX2 variant
constexpr int kMR = 6, kNR = 32;       // register tile: 6 rows x 32 columns = 12 accumulators of 16 floats
constexpr int kKC = 256, kMB = 96, kNB = 256;   // cache blocks: K step, rows (16 register tiles) and columns (8 register tiles) of a thread's tile

// ct[m][n] (+)= sum_{k < kc} ap[k*kMB + m] * bp[k*ldb + n]   for the kMR x kNR register tile at (m, n); one fma per (k, m, n), ascending k.
// ap: packed a block [kc][kMB] (zero beyond the matrix); bp: b panel, rows of >= kNR readable floats; ct: the thread's tile buffer [kMB][kNB].
#define MICRO_BODY                                                                                                     \
  vf acc[kMR][2];                                                                                                      \
  for (int m = 0; m < kMR; ++m) for (int h = 0; h < 2; ++h) {                                                            \
    if (first) { vf z = {0}; acc[m][h] = z; } else acc[m][h] = *(vf const *)(ct + m * kNB + 16 * h); }                   \
  for (int k = 0; k < kc; ++k) {                                                                                       \
    vf const b0 = *(vf const *)(bp + (long)k * ldb), b1 = *(vf const *)(bp + (long)k * ldb + 16);                        \
    float const *ak = ap + k * kMB;                                                                                    \
    for (int m = 0; m < kMR; ++m) {                                                                                    \
      float const av = ak[m];                                                                                          \
      vf const va = {av, av, av, av, av, av, av, av, av, av, av, av, av, av, av, av};                                  \
      acc[m][0] += va * b0; acc[m][1] += va * b1;   /* contracted to vfmadd (-ffp-contract=fast): one rounding */      \
    }                                                                                                                  \
  }                                                                                                                    \
  for (int m = 0; m < kMR; ++m) for (int h = 0; h < 2; ++h) *(vf *)(ct + m * kNB + 16 * h) = acc[m][h];
__attribute__((target("avx512f,fma"))) void micro_avx512(float const *ap, float const *bp, long ldb, float *ct, int kc, bool first) { MICRO_BODY }
__attribute__((target("avx2,fma"))) void micro_avx2(float const *ap, float const *bp, long ldb, float *ct, int kc, bool first) { MICRO_BODY }
#undef MICRO_BODY
typedef void (*micro_t)(float const *, float const *, long, float *, int, bool);

struct scratch_t { float *ap, *bp, *ct; };   // per thread: packed a block [kKC][kMB], b panel [kKC][kNB], tile [kMB][kNB]
void *aligned(size_t bytes) { void *p = nullptr; if (posix_memalign(&p, 64, std::max<size_t>(bytes, 64))) rt_err("be=cpu: out of memory"); return p; }

// D[i][j] = sum_k A(k, i) * B(k, j) over tiles of kMB x kNB; A(k, i) = at[k*lda + i] (k-major); the panel of B and the scatter of D are
// supplied by the caller (sgemm: rows of b / rows of c; conv: im2col gather / NCHW scatter with bias + ReLU).
template <typename PanelF, typename StoreF>
void tiled_contract(micro_t micro, float const *at, long lda, long Mi, long Nj, long K, PanelF panel, StoreF store) {
  long const tm = (Mi + kMB - 1) / kMB, tn = (Nj + kNB - 1) / kNB;
#pragma omp parallel
  {
    scratch_t s; s.ap = (float *)aligned(sizeof(float) * kKC * kMB); s.bp = (float *)aligned(sizeof(float) * kKC * kNB); s.ct = (float *)aligned(sizeof(float) * kMB * kNB);
#pragma omp for collapse(2) schedule(dynamic, 1)
    for (long tj = 0; tj < tn; ++tj)
      for (long ti = 0; ti < tm; ++ti) {
        long const i0 = ti * kMB, j0 = tj * kNB, mb = std::min<long>(kMB, Mi - i0), nb = std::min<long>(kNB, Nj - j0);
        for (long k0 = 0; k0 < K; k0 += kKC) {
          int const kc = (int)std::min<long>(kKC, K - k0);
          for (int k = 0; k < kc; ++k) {     // pack the a block: rows are contiguous in i; zero beyond the matrix
            memcpy(s.ap + k * kMB, at + (k0 + k) * lda + i0, sizeof(float) * mb);
            if (mb < kMB) memset(s.ap + k * kMB + mb, 0, sizeof(float) * (kMB - mb));
          }
          panel(s.bp, k0, kc, j0, nb);       // [kc][kNB], zero beyond column nb
          for (long mo = 0; mo < mb; mo += kMR)
            for (long no = 0; no < nb; no += kNR) micro(s.ap + mo, s.bp + no, kNB, s.ct + mo * kNB + no, kc, k0 == 0);
        }
        store(s.ct, i0, mb, j0, nb);
      }
    free(s.ap); free(s.bp); free(s.ct);
  }
}

// CT / OCT (a grouped convolution run per group on offset pointers: C and OC are then ONE group's channels): the channels of the whole in / out tensors, which the image
// strides follow; 0: C / OC
struct conv_geom_c { long B, C, H, W, OC, KH, KW, SY, SX, PY, PX, OH, OW; bool relu; long CT, OCT;
  long in_chans() const { return CT ? CT : C; } long out_chans() const { return OCT ? OCT : OC; } };

// ---- the non-conv ops of the gradient pipe: plain loops in exactly the reference templates' order (test/rtc/pool.cucl, spreading.cucl, lrn.cucl, bck_lrn.cucl,
// ZeroIfNonPos.cucl, softmax.cucl, sm_grad_and_loss.cucl, sum_loss_over_imgs.cucl), parallel over outputs.  They are the bit-exact checker of the HIP kernels
// (kernels/bck_ops_f32.hip states the semantics and the quirks), so nothing here may be fused or regrouped: this file builds with -ffp-contract=fast for the fmaf
// chains above, and these functions switch contraction off again.
#pragma GCC push_options
#pragma GCC optimize("fp-contract=off")
struct pool_geom_c { long B, C, H, W, OH, OW, KH, KW, SY, SX, PY, PX; bool avg; };
void pool_yx(float const *in, float *out, float *out_in_yx, pool_geom_c const &g) {
#pragma omp parallel for schedule(static)
  for (long pl = 0; pl < g.B * g.C; ++pl)
    for (long oy = 0; oy < g.OH; ++oy)
      for (long ox = 0; ox < g.OW; ++ox) {
        float best = g.avg ? 0.0f : -3.402823466e+38f, cnt = 0.0f; long oyx = -1;
        for (long kx = 0; kx < g.KW; ++kx)
          for (long ky = 0; ky < g.KH; ++ky) {
            long const iy = oy * g.SY + ky - g.PY, ix = ox * g.SX + kx - g.PX;
            if (iy < 0 || ix < 0 || ix >= g.W || iy >= g.H) continue;
            float const v = in[(pl * g.H + iy) * g.W + ix];
            if (g.avg) { best = best + v; cnt = cnt + 1.0f; }   // an average: the taps inside the plane, divided by their number; out_in_yx stays -1
            else if (v > best) { best = v; oyx = iy * g.W + ix; }
          }
        if (g.avg) best = best / cnt;
        out[(pl * g.OH + oy) * g.OW + ox] = best;
        out_in_yx[(pl * g.OH + oy) * g.OW + ox] = (float)oyx;
      }
}
// zin (spreading, bck_lrn, bconv_in; the function op's zero_if_in_non_pos=1): the forward input.  The loop is the template's; the value it forms is replaced by +0
// where !(zin > 0) just before the store -- hip_zero_if_non_pos's select with cond = in
void spreading(float const *ogl, float const *out_in_yx, float *igl, pool_geom_c const &g, float const *zin = nullptr) {
  float const spread_sz = (float)(g.KW * g.KH);   // the full window area, also where a border clips the window (the reference's own FIXME)
#pragma omp parallel for schedule(static)
  for (long pl = 0; pl < g.B * g.C; ++pl)
    for (long y = 0; y < g.H; ++y)
      for (long x = 0; x < g.W; ++x) {
        long const oxb = std::max<long>(0, x + g.PX - g.KW + g.SX) / g.SX, oxe = std::min<long>((x + g.PX) / g.SX + 1, g.OW);
        long const oyb = std::max<long>(0, y + g.PY - g.KH + g.SY) / g.SY, oye = std::min<long>((y + g.PY) / g.SY + 1, g.OH);
        float const in_yx = (float)(y * g.W + x);
        float v = 0.0f;
        for (long ox = oxb; ox < oxe; ++ox)
          for (long oy = oyb; oy < oye; ++oy) {
            long const oix = (pl * g.OH + oy) * g.OW + ox;
            if (g.avg) v = v + ogl[oix] / spread_sz;
            else if (in_yx == out_in_yx[oix]) v = v + ogl[oix];
          }
        long const ix = (pl * g.H + y) * g.W + x;
        igl[ix] = (zin && !(zin[ix] > 0.0f)) ? 0.0f : v;
      }
}
struct lrn_geom_c { long B, C, HW, LS; float alpha, beta, k; };
void lrn_sb(float const *in, float *out, float *sb, lrn_geom_c const &g) {
  long const hls = g.LS / 2;
  float const alpha_over_ls = g.alpha / (float)g.LS;
#pragma omp parallel for schedule(static)
  for (long pix = 0; pix < g.B * g.HW; ++pix) {
    long const base = (pix / g.HW) * g.C * g.HW + pix % g.HW;
    std::vector<float> ls_buf((size_t)g.LS, 0.0f);
    float ls_sum = 0.0f;
    for (long c = 0; c < g.C + hls; ++c) {
      long const slot = c % g.LS;
      float const ls_old = ls_buf[slot];
      ls_buf[slot] = (c < g.C) ? in[base + c * g.HW] : 0.0f;
      ls_sum = ls_sum + ls_buf[slot] * ls_buf[slot];
      ls_sum = ls_sum - ls_old * ls_old;
      if (c >= hls) {
        long const oc = c - hls;
        float const scale_base = g.k + ls_sum * alpha_over_ls;
        sb[base + oc * g.HW] = scale_base;
        out[base + oc * g.HW] = ls_buf[(slot + g.LS - hls) % g.LS] * powf(scale_base, -g.beta);
      }
    }
  }
}
void bck_lrn(float const *in, float const *out, float const *ogl, float const *sb, float *igl, lrn_geom_c const &g, bool zinp = false) {
  long const hls = g.LS / 2;
  float const coef = ((2.0f * -g.beta) * g.alpha) / (float)g.LS;
#pragma omp parallel for schedule(static)
  for (long pix = 0; pix < g.B * g.HW; ++pix) {
    long const base = (pix / g.HW) * g.C * g.HW + pix % g.HW;
    std::vector<float> ls_buf((size_t)g.LS, 0.0f);
    for (long c = 0; c < g.C + hls; ++c) {
      long const ix = base + c * g.HW;
      ls_buf[c % g.LS] = (c < g.C) ? (ogl[ix] * out[ix] / sb[ix]) : 0.0f;
      if (c >= hls) {
        long const ox = base + (c - hls) * g.HW;
        float ls_sum = 0.0f;
        for (long i = 0; i < g.LS; ++i) ls_sum = ls_sum + ls_buf[i];   // slot order, recomputed: not carried
        float const a = ogl[ox] * powf(sb[ox], -g.beta);
        float const b = in[ox] * ls_sum * coef;
        igl[ox] = (zinp && !(in[ox] > 0.0f)) ? 0.0f : a + b;
      }
    }
  }
}
void zero_if_non_pos(float const *in, float const *cond, float *out, long n) {
#pragma omp parallel for schedule(static)
  for (long i = 0; i < n; ++i) out[i] = (cond[i] > 0.0f) ? in[i] : 0.0f;
}
void reduce(float const *const *ins, int nin, float *out, long n) {   // a sequential chain from +0 in input order
#pragma omp parallel for schedule(static)
  for (long i = 0; i < n; ++i) {
    float v = 0.0f;
    for (int k = 0; k < nin; ++k) v = v + ins[k][i];
    out[i] = v;
  }
}
// the forward pipe's BatchNorm / Scale runs: a multiply, then an add (two roundings: contraction is off here); relu: x > 0 ? x : +0.  in == out is fine
void chan_affine(float const *in, float const *a, float const *b, float *out, long B, long C, long HW, bool relu) {
#pragma omp parallel for schedule(static)
  for (long pl = 0; pl < B * C; ++pl) {
    float const av = a[pl % C], bv = b[pl % C];
    for (long i = pl * HW; i < (pl + 1) * HW; ++i) {
      float v = in[i] * av;
      v = v + bv;
      out[i] = (relu && !(v > 0.0f)) ? 0.0f : v;
    }
  }
}
void dropout(float *inout, long n, float ratio, uint32_t seed) {
  float const scale = (float)(1.0 / (1.0 - (double)ratio));
  uint32_t const thresh = (uint32_t)((float)0xffffffffu * ratio);
#pragma omp parallel for schedule(static)
  for (long i = 0; i < n; ++i) {
    uint32_t h = (uint32_t)i + seed;
    h ^= h >> 16; h *= 0x85ebca6bu; h ^= h >> 13; h *= 0xc2b2ae35u; h ^= h >> 16;
    inout[i] = (h > thresh) ? inout[i] * scale : 0.0f;
  }
}
// concat (to_wide) / split: B images of `run` floats each <-> the floats [off, off + run) of every image of the wide tensor
void copy_chan_range(float const *in, float *out, long B, long run, long wide, long off, bool to_wide) {
#pragma omp parallel for schedule(static)
  for (long img = 0; img < B; ++img) {
    if (to_wide) memcpy(out + img * wide + off, in + img * run, sizeof(float) * run);
    else memcpy(out + img * run, in + img * wide + off, sizeof(float) * run);
  }
}
void softmax(float const *in, float *prob, long B, long C) {   // 1 x 1 planes; the reference's sequential sum
#pragma omp parallel for schedule(static)
  for (long img = 0; img < B; ++img) {
    float const *x = in + img * C; float *pr = prob + img * C;
    float pel_sum = 0.0f, pel_max = 0.0f;   // pel_max starts at 0, not at the first value
    for (long c = 0; c < C; ++c) pel_max = (x[c] > pel_max) ? x[c] : pel_max;
    for (long c = 0; c < C; ++c) { float const v = expf(x[c] - pel_max); pr[c] = v; pel_sum = pel_sum + v; }
    for (long c = 0; c < C; ++c) pr[c] = pr[c] / pel_sum;
  }
}
void sm_grad_and_loss(float const *prob, float const *label, float *igl, float *loss_per_pel, long B, long C) {
#pragma omp parallel for schedule(static)
  for (long img = 0; img < B; ++img) {
    float const lf = label[img];
    bool const valid = lf >= 0.0f && lf < (float)C;   // a label outside [0, chan) matches no channel and reads no memory
    long const lab = valid ? (long)lf : -1;
    float const pl = valid ? prob[img * C + lab] : 0.0f;
    loss_per_pel[img] = -logf(pl > 1.175494351e-38f ? pl : 1.175494351e-38f);
    for (long c = 0; c < C; ++c) {
      float v = prob[img * C + c];
      if (c == lab) v = v - 1.0f;
      v = v / (float)B;
      igl[img * C + c] = v;
    }
  }
}
void sum_loss_over_imgs(float const *loss_per_pel, float *loss, long B) {
  float v = 0.0f;
  for (long i = 0; i < B; ++i) v = v + loss_per_pel[i];
  loss[0] = v / (float)B;
}
// hip_sgd_update (kernels/sgd_update_f32.hip states the formula): the same chain, every operation its own fp32 rounding, g only read
void sgd_update(float *w, float const *g, float *h, long n, float lr_i, float wd_i, float mom) {
#pragma omp parallel for schedule(static)
  for (long e = 0; e < n; ++e) {
    float const reg = wd_i * w[e];
    float const g1 = g[e] + reg;
    float const a = mom * h[e];
    float const b = lr_i * g1;
    float const h2 = a + b;
    h[e] = h2;
    w[e] = w[e] - h2;
  }
}
// ---- the solver family (kernels/solver_update_f32.hip states the chains and the tree): the same operations in the same order, every one its own fp32 rounding
struct solver_coef_c { float lr, wd, mom, mom2, delta, coef, c, o1, o2, s, lrwd, scale; };
// acc (hip_solver_update_acc): gs = scale * g0, one rounding, in g0's place
void solver_update(int type, bool clip, bool dwd, bool acc, float *w, float const *g, float *h, float *v, long n, solver_coef_c const k) {
#pragma omp parallel for schedule(static)
  for (long e = 0; e < n; ++e) {
    float const gc = clip ? k.coef * g[e] : g[e];
    float const g0 = acc ? k.scale * gc : gc;
    if (type == kSolverAdam) {
      float g1 = g0;
      if (!dwd) { float const reg = k.wd * w[e]; g1 = g0 + reg; }
      float const ma = k.mom * h[e];
      float const mb = k.o1 * g1;
      float const m = ma + mb;
      float const q = g1 * g1;
      float const va = k.mom2 * v[e];
      float const vb = k.o2 * q;
      float const vn = va + vb;
      float const sq = sqrtf(vn);
      float const d = sq + k.delta;
      float const r = m / d;
      float u = k.s * r;
      if (dwd) { float const dw = k.lrwd * w[e]; u = u + dw; }
      h[e] = m; v[e] = vn; w[e] = w[e] - u;
    } else {
      float const reg = k.wd * w[e];
      float const g1 = g0 + reg;
      float const a = k.mom * h[e];
      float const b = k.lr * g1;
      float const hn = a + b;
      h[e] = hn;
      if (type == kSolverNesterov) { float u = k.c * hn; u = u - a; w[e] = w[e] - u; }
      else w[e] = w[e] - hn;
    }
  }
}
// hip_grad_accum: first: a' = g, a not read; else a' = a + g, one fp32 add
void grad_accum(bool first, float const *g, float *a, long n) {
  if (first) { memcpy(a, g, sizeof(float) * (size_t)n); return; }
#pragma omp parallel for schedule(static)
  for (long e = 0; e < n; ++e) a[e] = a[e] + g[e];
}
// the tree over 256 lane sums: for h = 128 .. 1: a[t] = a[t] + a[t + h], t < h
inline float solver_tree(float *a) { for (int h = 128; h > 0; h >>= 1) for (int t = 0; t < h; ++t) a[t] = a[t] + a[t + h]; return a[0]; }
// one chunk's partial: lane t adds x * x for the elements t, t + 256, ... from +0
float solver_chunk_sumsq(float const *g, long cnt) {
  float a[256];
  for (int t = 0; t < 256; ++t) { float acc = 0.0f; for (long e = t; e < cnt; e += 256) { float const q = g[e] * g[e]; acc = acc + q; } a[t] = acc; }
  return solver_tree(a);
}
void solver_grad_norm(float const *partials, long n, float clip, float *state) {
  float a[256];
  for (int t = 0; t < 256; ++t) { float acc = 0.0f; for (long e = t; e < n; e += 256) acc = acc + partials[e]; a[t] = acc; }
  float const sumsq = solver_tree(a);
  float const norm = sqrtf(sumsq);
  float const coef = (norm > clip) ? clip / norm : 1.0f;
  state[0] = coef; state[1] = norm; state[2] = sumsq; state[3] = 0.0f;
}
// ---- the training BatchNorm functions and hip_fan_out (kernels/bn_f32.hip states the formulas and the chain of the sums): the same operations in the same order.
// One slab of one channel: 256 chains, chain t owning the elements with (r / 4) mod 256 == t in ascending r, then the fixed tree.  term(e, acc0, acc1) adds element e's terms
template <typename TermF> void bn_slab_sums(long e0, long len, TermF term, float &P0, float &P1) {
  float a0[256], a1[256];
  for (int t = 0; t < 256; ++t) { a0[t] = 0.0f; a1[t] = 0.0f; }
  for (long r = 0; r < len; ++r) { int const t = (int)((r >> 2) & 255); term(e0 + r, a0[t], a1[t]); }
  for (int h = 128; h > 0; h >>= 1) for (int t = 0; t < h; ++t) { a0[t] = a0[t] + a0[t + h]; a1[t] = a1[t] + a1[t + h]; }
  P0 = a0[0]; P1 = a1[0];
}
// the sums of every channel: slab partials in slab order starting from P_0 -> S0[c], S1[c]
template <typename TermOfChanF> void bn_chan_sums(bn_op_t const &b, TermOfChanF term_of, float *S0, float *S1) {
  std::vector<float> P0((size_t)(b.C * b.nslabs)), P1((size_t)(b.C * b.nslabs));
#pragma omp parallel for schedule(static)
  for (long cs = 0; cs < b.C * b.nslabs; ++cs) {
    long const c = cs / b.nslabs, s = cs - c * b.nslabs, e0 = s * b.slab, len = std::min(b.slab, b.N - e0);
    bn_slab_sums(e0, len, term_of(c), P0[(size_t)cs], P1[(size_t)cs]);
  }
  for (long c = 0; c < b.C; ++c) {
    float A = P0[(size_t)(c * b.nslabs)], B = P1[(size_t)(c * b.nslabs)];
    for (long i = 1; i < b.nslabs; ++i) { A = A + P0[(size_t)(c * b.nslabs + i)]; B = B + P1[(size_t)(c * b.nslabs + i)]; }
    S0[c] = A; S1[c] = B;
  }
}
inline long bn_off(bn_op_t const &b, long c, long e) { long const img = e / b.HW; return (img * b.C + c) * b.HW + (e - img * b.HW); }
// the chunked chain (hip_bnc_stats / hip_bnc_bck_sums; one chunk, and every hip_bn_* call: bn_chan_sums itself): every non-empty chunk's totals by the plan of the chunk's
// own dims, its elements numbered from its first image, then ((D_a + D_b) + D_c) + ... in ascending chunk order starting FROM the first.  term_of(cb, off, c): the terms
// of channel c of the chunk whose first element in the tensors is off
template <typename TermOfChunkChanF> void bn_chunked_sums(bn_op_t const &b, TermOfChunkChanF term_of, float *S0, float *S1) {
  if (!(b.bnc && b.chunks > 1)) { bn_chan_sums(b, [&](long c) { return term_of(b, 0L, c); }, S0, S1); return; }
  std::vector<float> D0((size_t)b.C), D1((size_t)b.C);
  bool first = true;
  for (uint32_t i = 0; i < b.chunks; ++i) {
    bn_op_t const cb = bnc_chunk_op(b.kind == 1 ? "hip_bnc_stats" : "hip_bnc_bck_sums", b, i);
    if (!cb.B) continue;
    long const off = bnc_chunk_begin(b.B, b.chunks, i) * b.C * b.HW;
    bn_chan_sums(cb, [&](long c) { return term_of(cb, off, c); }, first ? S0 : D0.data(), first ? S1 : D1.data());
    if (!first) for (long c = 0; c < b.C; ++c) { S0[c] = S0[c] + D0[(size_t)c]; S1[c] = S1[c] + D1[(size_t)c]; }
    first = false;
  }
}
void bn_stats(bn_op_t const &b, float const *in, float *mean, float *inv_std, float *run_mean, float *run_var) {
  std::vector<float> S1((size_t)b.C), S2((size_t)b.C), dummy((size_t)b.C), mu((size_t)b.C);
  float const fN = (float)b.N, omm = 1.0f - b.maf, unb = b.N > 1 ? (float)b.N / (float)(b.N - 1) : 1.0f;
  bn_chunked_sums(b, [&](bn_op_t const &cb, long off, long c) { return [&cb, in, off, c](long e, float &a0, float &) { a0 = a0 + in[off + bn_off(cb, c, e)]; }; }, S1.data(), dummy.data());
  for (long c = 0; c < b.C; ++c) mu[(size_t)c] = S1[(size_t)c] / fN;
  bn_chunked_sums(b, [&](bn_op_t const &cb, long off, long c) { float const m = mu[(size_t)c]; return [&cb, in, off, c, m](long e, float &a0, float &) { float const df = in[off + bn_off(cb, c, e)] - m; float const sq = df * df; a0 = a0 + sq; }; }, S2.data(), dummy.data());
  for (long c = 0; c < b.C; ++c) {
    float const m = mu[(size_t)c];
    float const var = S2[(size_t)c] / fN;
    float const ve = var + b.eps;
    float const sd = sqrtf(ve);
    float const istd = 1.0f / sd;
    float const m1 = b.maf * run_mean[c];
    float const m2 = omm * m;
    float const uv = (b.N == 1) ? var : var * unb;
    float const v1 = b.maf * run_var[c];
    float const v2 = omm * uv;
    mean[c] = m; inv_std[c] = istd; run_mean[c] = m1 + m2; run_var[c] = v1 + v2;
  }
}
void bn_fwd(bn_op_t const &b, float const *in, float *out, float const *mean, float const *inv_std, float const *scale, float const *bias) {
#pragma omp parallel for schedule(static)
  for (long pl = 0; pl < b.B * b.C; ++pl) {
    long const c = pl % b.C;
    float const m = mean[c], is = inv_std[c], sc = scale[c], bi = bias[c];
    for (long e = pl * b.HW; e < (pl + 1) * b.HW; ++e) {
      float const df = in[e] - m;
      float const xh = df * is;
      float v = xh * sc;
      v = v + bi;
      if (b.relu) v = v > 0.0f ? v : 0.0f;
      out[e] = v;
    }
  }
}
void bn_bck_sums(bn_op_t const &b, float const *in, float const *dy, float const *mean, float const *inv_std, float *sg, float *bg) {
  bn_chunked_sums(b, [&](bn_op_t const &cb, long off, long c) { float const m = mean[c], is = inv_std[c]; return [&cb, in, dy, off, c, m, is](long e, float &a0, float &a1) {
    long const o = off + bn_off(cb, c, e); float const df = in[o] - m; float const xh = df * is; float const tm = dy[o] * xh; a0 = a0 + tm; a1 = a1 + dy[o]; }; }, sg, bg);
}
void bn_bck_in(bn_op_t const &b, float const *in, float const *dy, float *dx, float const *mean, float const *inv_std, float const *scale, float const *sg, float const *bg) {
  float const fN = (float)b.n_glob();   // (the whole batch's, also where the vars hold an img shard of it)
#pragma omp parallel for schedule(static)
  for (long pl = 0; pl < b.B * b.C; ++pl) {
    long const c = pl % b.C;
    float const m = mean[c], is = inv_std[c];
    float const k = scale[c] * is;
    float const mg = sg[c] / fN;
    float const mb = bg[c] / fN;
    for (long e = pl * b.HW; e < (pl + 1) * b.HW; ++e) {
      float const df = in[e] - m;
      float const xh = df * is;
      float const t1 = dy[e] - mb;
      float const t2 = xh * mg;
      float const t3 = t1 - t2;
      dx[e] = k * t3;
    }
  }
}
// BatchNorm on its running pair (hip_bnf_prep / hip_bnf_bck / hip_bnf_bck_in): the statistics are constants, dx = (scale * inv_std) * dy
void bnf_prep(bn_op_t const &b, float const *run_mean, float const *run_var, float *mean, float *inv_std) {
  for (long c = 0; c < b.C; ++c) {
    float const ve = run_var[c] + b.eps;
    float const sd = sqrtf(ve);
    memcpy(mean + c, run_mean + c, sizeof(float));   // the bits
    inv_std[c] = 1.0f / sd;
  }
}
void bnf_bck_in(bn_op_t const &b, float const *dy, float *dx, float const *inv_std, float const *scale) {
#pragma omp parallel for schedule(static)
  for (long pl = 0; pl < b.B * b.C; ++pl) {
    float const k = scale[pl % b.C] * inv_std[pl % b.C];
    for (long e = pl * b.HW; e < (pl + 1) * b.HW; ++e) dx[e] = k * dy[e];
  }
}
// (the sums first, over the unwritten dy: dx may be dy's buffer)
void bnf_bck(bn_op_t const &b, float const *in, float const *dy, float *dx, float const *mean, float const *inv_std, float const *scale, float *sg, float *bg) {
  bn_bck_sums(b, in, dy, mean, inv_std, sg, bg);
  bnf_bck_in(b, dy, dx, inv_std, scale);
}
// ---- the eval family (kernels/eval_f32.hip states the rules): the same tests and the same fp32 chain, one rounding per line
void accuracy(float const *in, float const *label, uint32_t *rank, long B, long C) {
#pragma omp parallel for schedule(static)
  for (long img = 0; img < B; ++img) {
    float const lf = label[img];
    bool const valid = lf >= 0.0f && lf < (float)C;
    if (!valid) { rank[img] = 0xFFFFFFFFu; continue; }
    long const L = (long)(int)lf;
    float const *const x = in + img * C;
    float const t = x[L];
    uint32_t cnt = 0;
    for (long c = 0; c < C; ++c) cnt += (c != L && !(x[c] < t)) ? 1u : 0u;
    rank[img] = cnt;
  }
}
void eval_accum(uint32_t const *rank, float const *loss, uint32_t const *ctl, uint32_t *counts, float *loss_sum, long B, uint32_t top_k) {
  uint32_t h1 = 0, hk = 0;
  for (long i = 0; i < B; ++i) { h1 += rank[i] < 1u ? 1u : 0u; hk += rank[i] < top_k ? 1u : 0u; }
  if (ctl[0] != 0u) {
    counts[0] = (uint32_t)B; counts[1] = h1; counts[2] = hk; counts[3] = 1u;
    memcpy(loss_sum, loss, sizeof(float));   // the loss's bits
  } else {
    counts[0] += (uint32_t)B; counts[1] += h1; counts[2] += hk; counts[3] += 1u;
    loss_sum[0] = loss_sum[0] + loss[0];
  }
}
void bn_fold(float const *run_mean, float const *run_var, float const *scale, float const *bias, float *a, float *b, long C, float eps) {
  for (long c = 0; c < C; ++c) {
    float const mean = run_mean[c], var = run_var[c], sc = scale[c], bi = bias[c];
    float const ve = var + eps;
    float const sd = sqrtf(ve);
    float const a2 = 1.0f / sd;
    float const mp = mean * a2;
    float const b2 = -mp;
    float const a1 = a2 * 1.0f;
    float const z = a2 * 0.0f;
    float const b1 = z + b2;
    float const av = sc * a1;
    float const sb = sc * b1;
    a[c] = av; b[c] = sb + bi;
  }
}
// ---- the data family (kernels/data_f32.hip states the rule): the same clamps, the same two fp32 roundings; OpenMP over images
void data_transform(data_op_t const &d, unsigned char const *src, uint32_t const *plan, float const *mean, float *out) {
  long const B = d.B, C = d.C, H = d.H, W = d.W, ch = d.ch, cw = d.cw;
  float const scale = d.scale;
#pragma omp parallel for schedule(static)
  for (long i = 0; i < B; ++i) {
    uint32_t const *const pl = plan + i * 4;
    uint32_t const ymax = (uint32_t)(H - ch), xmax = (uint32_t)(W - cw);
    long const yo = pl[0] < ymax ? pl[0] : ymax, xo = pl[1] < xmax ? pl[1] : xmax;
    bool const m = pl[2] != 0u;
    for (long c = 0; c < C; ++c) for (long y = 0; y < ch; ++y) for (long x = 0; x < cw; ++x) {
      long const sy = yo + y, sx = xo + (m ? cw - 1 - x : x);
      long const si = d.chw ? ((i * C + c) * H + sy) * W + sx : ((i * H + sy) * W + sx) * C + c;
      float const mu = d.mean_pel ? mean[(c * H + sy) * W + sx] : mean[c];
      float const v = (float)src[si];
      float const dv = v - mu;
      out[((i * C + c) * ch + y) * cw + x] = dv * scale;
    }
  }
}
// ---- the loss family (kernels/loss_f32.hip states the rules): the same tests, the same fp32 operations in the same order; expf and logf are this platform's
constexpr float kLossFltMin = 1.175494351e-38f, kInvalidLoss = 0x1.5d58a0p+6f;   // (126 ln 2 rounded to fp32, the kernel's constant)
static inline float loss_exp_diff(float a, float m) {   // exp(a - m) with the difference held exactly as the pair (d, r): the kernel's exp_diff
  float const d = a - m;
  float const bb = d - a;
  float const r = (a - (d - bb)) - (m + bb);
  float const e = expf(d);
  float const er = e * r;
  return e + er;
}
void softmax_loss_fwd(loss_op_t const &l, float const *in, float const *label, float *prob, float *lpp) {
  long const C = l.C, HW = l.HW; bool const wave = HW < 64;
#pragma omp parallel for schedule(static)
  for (long id = 0; id < l.B * HW; ++id) {
    long const img = id / HW, pel = id - img * HW;
    float const *const x = in + img * C * HW + pel; float *const pr = prob + img * C * HW + pel;
    float m, S;
    if (!wave) {   // the pel form: one sequential chain over the channels
      m = x[0]; for (long c = 1; c < C; ++c) { float const v = x[c * HW]; m = v > m ? v : m; }
      S = 0.0f; for (long c = 0; c < C; ++c) S = S + loss_exp_diff(x[c * HW], m);
    } else {       // the wave form: 64 lane chains over channels l, l + 64, ..., then the xor butterfly (lane l's partner at step k is l ^ k: pairwise, both get a + b)
      float lm[64], ls[64];
      for (int ln = 0; ln < 64; ++ln) { float v = -__builtin_inff(); for (long c = ln; c < C; c += 64) { float const w = x[c * HW]; v = w > v ? w : v; } lm[ln] = v; }
      for (int k = 32; k > 0; k >>= 1) for (int ln = 0; ln < 64; ++ln) if (!(ln & k)) { float const a = lm[ln], b = lm[ln ^ k]; float const r = b > a ? b : a, r2 = a > b ? a : b; lm[ln] = r; lm[ln ^ k] = r2; }
      m = lm[0];
      for (int ln = 0; ln < 64; ++ln) { float a = 0.0f; for (long c = ln; c < C; c += 64) a = a + loss_exp_diff(x[c * HW], m); ls[ln] = a; }
      for (int k = 32; k > 0; k >>= 1) for (int ln = 0; ln < 64; ++ln) if (!(ln & k)) { float const r = ls[ln] + ls[ln ^ k]; ls[ln] = r; ls[ln ^ k] = r; }
      S = ls[0];
    }
    for (long c = 0; c < C; ++c) pr[c * HW] = loss_exp_diff(x[c * HW], m) / S;
    float const lf = label[id];
    float v;
    if (l.has_ignore && lf == l.ignore) v = 0.0f;
    else if (!(lf >= 0.0f && lf < (float)C)) v = kInvalidLoss;
    else { float const pl = pr[(long)(int)lf * HW]; v = -logf(pl > kLossFltMin ? pl : kLossFltMin); }
    lpp[id] = v;
  }
}
void loss_norm(loss_op_t const &l, float const *label, float const *lpp, float *loss, float *state) {
  long const N = l.pels();
  float sa[256]; uint32_t sc[256];
  for (long t = 0; t < 256; ++t) {
    float a = 0.0f; uint32_t cnt = 0;
    for (long i = t; i < N; i += 256) { a = a + lpp[i]; cnt += (l.has_ignore && label[i] == l.ignore) ? 0u : 1u; }
    sa[t] = a; sc[t] = cnt;
  }
  for (long h = 128; h > 0; h >>= 1) for (long t = 0; t < h; ++t) { sa[t] = sa[t] + sa[t + h]; sc[t] += sc[t + h]; }
  float const sum = sa[0]; uint32_t const count = sc[0];
  float Z = 1.0f;
  if (l.norm == 0) Z = (float)(count > 1u ? count : 1u); else if (l.norm == 1) Z = (float)N; else if (l.norm == 2) Z = (float)l.B;
  float const s = l.weight / Z;
  loss[0] = sum / Z;
  state[0] = Z; state[1] = s; state[2] = (float)count; state[3] = sum;
}
void softmax_loss_bck(loss_op_t const &l, float const *prob, float const *label, float const *state, float *grad) {
  long const C = l.C, HW = l.HW;
  float const s = state[1];
#pragma omp parallel for schedule(static)
  for (long q = 0; q < l.B * C; ++q) {
    long const img = q / C, c = q - img * C;
    for (long pel = 0; pel < HW; ++pel) {
      float const lf = label[img * HW + pel]; float const p = prob[q * HW + pel];
      float g;
      if (l.has_ignore && lf == l.ignore) g = 0.0f;
      else { bool const valid = lf >= 0.0f && lf < (float)C; float const d = (valid && (long)(int)lf == c) ? p - 1.0f : p; g = d * s; }
      grad[q * HW + pel] = g;
    }
  }
}
#pragma GCC pop_options
} // namespace

struct cpu_var_t { std::shared_ptr<void> buf; dims_t dims; };
struct cpu_func_t { rtc_func_info_t info; native_func_t const *row; };   // row: the function's row of native_funcs.h, looked up when it is compiled

struct cpu_compute_t : public rtc_compute_t {
  bool init_done = false;
  micro_t micro = nullptr;
  string isa;
  std::map<string, cpu_var_t> vis;
  std::map<string, cpu_func_t> funcs;
  std::vector<std::pair<double, double>> call_t;   // (begin, end) in ms since init
  std::chrono::steady_clock::time_point t0;
  cpu_compute_t() { be = "cpu"; }

  double now_ms() const { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); }
  void init() override {
    assert_st(!init_done);
    __builtin_cpu_init();
    if (__builtin_cpu_supports("avx512f") && __builtin_cpu_supports("fma") && !getenv("BODACPU_NO_AVX512")) { micro = micro_avx512; isa = "avx512"; }
    else if (__builtin_cpu_supports("avx2") && __builtin_cpu_supports("fma")) { micro = micro_avx2; isa = "avx2"; }
    else rt_err("cpu backend: this host has neither AVX-512 nor AVX2 with FMA (the kernels need fused multiply-add for the reference's fmaf chain)");
    t0 = std::chrono::steady_clock::now(); init_done = true;
  }
  string get_plat_tag() override { assert_st(init_done); return "cpu:" + isa + ":" + std::to_string(omp_get_max_threads()) + "t"; }

  // ---- vars
  void create_var_with_dims(string const &vn, dims_t const &dims) override {
    assert_st(init_done);
    if (vis.count(vn)) rt_err("create_var_with_dims: var '" + vn + "' already exists");
    size_t const sz = dims.bytes_sz();
    cpu_var_t v; v.dims = dims; v.buf = std::shared_ptr<void>(aligned(sz), free); memset(v.buf.get(), 0, sz);
    vis.emplace(vn, std::move(v));
  }
  void create_var_with_dims_as_reshaped_view_of_var(string const &vn, dims_t const &dims, string const &src_vn) override {
    cpu_var_t const &src = must_find(vis, src_vn);
    rtc_reshape_check(dims, src.dims);
    if (vis.count(vn)) rt_err("create_var_with_dims_as_reshaped_view_of_var: var '" + vn + "' already exists");
    cpu_var_t v; v.dims = dims; v.buf = src.buf; vis.emplace(vn, std::move(v));
  }
  void release_var(string const &vn) override { must_erase(vis, vn); }
  dims_t get_var_dims(string const &vn) override { return must_find(vis, vn).dims; }
  void set_var_to_zero(string const &vn) override { cpu_var_t const &v = must_find(vis, vn); memset(v.buf.get(), 0, v.dims.bytes_sz()); }
  void copy_nda_to_var(string const &vn, p_nda_t const &nda) override {
    cpu_var_t const &v = must_find(vis, vn);
    if (!(v.dims == nda->dims)) rt_err("copy_nda_to_var: dims mismatch for var '" + vn + "': var " + v.dims.pretty_str() + " nda " + nda->dims.pretty_str());
    memcpy(v.buf.get(), nda->rp_elems(), v.dims.bytes_sz());
  }
  void copy_var_to_nda(p_nda_t const &nda, string const &vn) override {
    cpu_var_t const &v = must_find(vis, vn);
    if (!(v.dims == nda->dims)) rt_err("copy_var_to_nda: dims mismatch for var '" + vn + "': var " + v.dims.pretty_str() + " nda " + nda->dims.pretty_str());
    memcpy(nda->rp_elems(), v.buf.get(), v.dims.bytes_sz());
  }
  p_nda_t get_var_raw_native_pointer(string const &vn) override { cpu_var_t const &v = must_find(vis, vn); return std::make_shared<nda_t>(v.dims, v.buf.get()); }

  // ---- functions: the native side door only
  void compile(vect_rtc_func_info_t const &func_infos, rtc_compile_opts_t const &) override {
    assert_st(init_done);
    for (auto const &fi : func_infos) {
      if (funcs.count(fi.func_name)) rt_err("compile: function '" + fi.func_name + "' already exists");
      string const fn = fi.op.has_func_name() ? fi.op.get_func_name() : string();
      native_func_t const *f = find_native_func(fn);   // (the table of native_funcs.h says which functions be=cpu runs)
      if (!f || !(f->backends & kBeCpu))
        unsup_err("be=cpu runs the native sgemm / Convolution / BckConv functions and the gradient pipe's non-conv functions only (hip_sgemm, hip_conv and their aliases, hip_bconv_*, " +
                  native_func_names([](native_func_t const &r) { return (r.backends & kBeCpu) && r.family >= kFamBckOp; }, ", ") + "); '" +
                                                    (fn.empty() ? fi.func_name : fn) + "' is generated CUCL source, which needs a GPU backend");
      if (f->family == kFamConv) (void)fi.op.get_u32("conv_has_relu");
      (void)op_zinp_flag(fi.op);   // (refuses the flag on a function that cannot take it)
      (void)op_seed_var_flag(fi.op);   // (likewise)
      (void)op_img_shards_flag(fi.op);   // (likewise; here there is one shard: a flagged call is the unflagged one)
      (void)op_bf16_operands(fi.op);   // (str_val hip_operands: refused where the function has no bf16-operand form)
      if (f->family == kFamSgd) (void)sgd_op_of_op(fi.op);   // (the op must be whole)
      if (f->family == kFamBn || f->family == kFamBnc || f->family == kFamBnf) (void)bn_op_of_op(fi.op);   // (likewise)
      if (f->family == kFamSolver) (void)solver_op_of_op(fi.op);   // (likewise)
      if (f->family == kFamEval) (void)eval_op_of_op(fi.op);   // (likewise)
      if (f->family == kFamData) (void)data_op_of_op(fi.op);   // (likewise)
      if (f->family == kFamLoss) (void)loss_op_of_op(fi.op);   // (likewise)
      if (f->family == kFamConvGrp) (void)conv_grp_geom_of_op(fi.op, f->member);   // (likewise: the group count and the geometry it needs)
      if (f->family == kFamDeconv) (void)deconv_geom_of_op(fi.op, f->member);   // (likewise: no group, no fused ReLU, the geometry)
      if (f->family == kFamBckOp) {
        if (!f->of_type(fi.op.get_type())) rt_err(fn + ": a function of op type " + f->types[0] + ", not " + fi.op.get_type());
        bck_op_args_t const a = bck_op_args(*f, fi.op);
        for (string const &an : a.ins) (void)fi.op.get_dims(an);
        for (string const &an : a.outs) (void)fi.op.get_dims(an);
      }
      funcs.emplace(fi.func_name, cpu_func_t{fi, f});
    }
  }
  void release_func(string const &func_name) override { must_erase(funcs, func_name); }
  void release_all_funcs() override { funcs.clear(); }

  static string var_of(map_str_rtc_arg_t const &am, string const &an) {
    auto i = am.find(an);
    if (i == am.end()) rt_err("cpu_compute_t: arg '" + an + "' not found in arg_map for call.");
    if (!i->second.is_valid() || !i->second.is_var()) rt_err("cpu_compute_t: arg '" + an + "' must be a var");
    return i->second.n;
  }
  static void need_float(dims_t const &d, char const *an) { if (d.tn != "float") unsup_err(string("be=cpu: arg '") + an + "' has type " + d.tn + "; only float is supported"); }

  void sgemm(float const *a, float const *b, float *c, long M, long N, long K) {
    if (!M || !N) return;
    if (!K) { memset(c, 0, sizeof(float) * M * N); return; }
    tiled_contract(micro, a, M, M, N, K,
      [&](float *bp, long k0, int kc, long j0, long nb) {
        for (int k = 0; k < kc; ++k) { memcpy(bp + k * kNB, b + (k0 + k) * N + j0, sizeof(float) * nb); if (nb < kNB) memset(bp + k * kNB + nb, 0, sizeof(float) * (kNB - nb)); } },
      [&](float const *ct, long i0, long mb, long j0, long nb) { for (long m = 0; m < mb; ++m) memcpy(c + (i0 + m) * N + j0, ct + m * kNB, sizeof(float) * nb); });
  }
  void conv(float const *filts, float const *biases, float const *in, float *out, conv_geom_c const &g) {
    long const K = g.C * g.KH * g.KW, Nj = g.B * g.OH * g.OW, OHW = g.OH * g.OW;
    if (!Nj || !g.OC) return;
    std::vector<float> ft((size_t)K * g.OC);     // filters k-major: ft[k][oc]
#pragma omp parallel for schedule(static)
    for (long oc = 0; oc < g.OC; ++oc) for (long k = 0; k < K; ++k) ft[k * g.OC + oc] = filts[oc * K + k];
    tiled_contract(micro, ft.data(), g.OC, g.OC, Nj, K,
      [&](float *bp, long k0, int kc, long j0, long nb) {     // im2col of columns j0 .. j0+nb, rows k0 .. k0+kc (cross-correlation, zero padding: test/rtc/conv.cucl:33-36)
        long base[kNB]; int iy0[kNB], ix0[kNB];               // per column: offset of (img, chan 0, iy0, ix0) and the window origin
        for (long n = 0; n < nb; ++n) {
          long const j = j0 + n, img = j / OHW, pel = j - img * OHW, oy = pel / g.OW, ox = pel - oy * g.OW;
          iy0[n] = (int)(oy * g.SY - g.PY); ix0[n] = (int)(ox * g.SX - g.PX);
          base[n] = (img * g.in_chans() * g.H + iy0[n]) * g.W + ix0[n];
        }
        for (int kk = 0; kk < kc; ++kk) {
          long const k = k0 + kk, c = k / (g.KH * g.KW), r = k - c * (g.KH * g.KW), ky = r / g.KW, kx = r - ky * g.KW;
          long const koff = (c * g.H + ky) * g.W + kx;
          float *row = bp + kk * kNB;
          for (long n = 0; n < nb; ++n) {
            int const iy = iy0[n] + (int)ky, ix = ix0[n] + (int)kx;
            row[n] = ((unsigned)iy < (unsigned)g.H && (unsigned)ix < (unsigned)g.W) ? in[base[n] + koff] : 0.f;
          }
          if (nb < kNB) memset(row + nb, 0, sizeof(float) * (kNB - nb));
        } },
      [&](float const *ct, long i0, long mb, long j0, long nb) {   // bias after the chain, then ReLU (src/cnn_codegen.cc:35-42)
        for (long m = 0; m < mb; ++m) {
          float const bias = biases[i0 + m];
          for (long n = 0; n < nb; ++n) {
            long const j = j0 + n, img = j / OHW, pel = j - img * OHW;
            float v = ct[m * kNB + n] + bias;
            if (g.relu) v = (v > 0.f) ? v : 0.f;
            out[(img * g.out_chans() + i0 + m) * OHW + pel] = v;
          }
        } });
  }

  // BckConv's gradients: the reference templates' loops, one fmaf chain per output in exactly their order (test/rtc/BckConv_in_grad_loss.cucl,
  // BckConv_filts_grad_loss.cucl, BckConv_biases_grad_loss.cucl), parallel over outputs.  g is the forward convolution's geometry.
  static void bconv_in(float const *filts, float const *ogl, float *igl, conv_geom_c const &g, float const *zin = nullptr) {
#pragma omp parallel for collapse(2) schedule(static)
    for (long img = 0; img < g.B; ++img)
      for (long c = 0; c < g.C; ++c)
        for (long y = 0; y < g.H; ++y)
          for (long x = 0; x < g.W; ++x) {
            long const oxb = std::max<long>(0, x + g.PX - g.KW + g.SX) / g.SX, oxe = std::min<long>((x + g.PX) / g.SX + 1, g.OW);
            long const oyb = std::max<long>(0, y + g.PY - g.KH + g.SY) / g.SY, oye = std::min<long>((y + g.PY) / g.SY + 1, g.OH);
            float v = 0.f;
            for (long oc = 0; oc < g.OC; ++oc) {
              long fx = x + g.PX - oxb * g.SX;   // out_x ascending (outer), filter taps descending
              for (long ox = oxb; ox < oxe; ++ox, fx -= g.SX) {
                long fy = y + g.PY - oyb * g.SY;
                for (long oy = oyb; oy < oye; ++oy, fy -= g.SY)
                  v = fmaf(ogl[((img * g.out_chans() + oc) * g.OH + oy) * g.OW + ox], filts[((oc * g.C + c) * g.KH + fy) * g.KW + fx], v);
              }
            }
            long const ix = ((img * g.in_chans() + c) * g.H + y) * g.W + x;
            igl[ix] = (zin && !(zin[ix] > 0.0f)) ? 0.0f : v;
          }
  }
  static void bconv_filts(float const *in, float const *ogl, float *fgl, conv_geom_c const &g) {
#pragma omp parallel for collapse(2) schedule(static)
    for (long oc = 0; oc < g.OC; ++oc)
      for (long c = 0; c < g.C; ++c)
        for (long fy = 0; fy < g.KH; ++fy)
          for (long fx = 0; fx < g.KW; ++fx) {
            long oyb = 0, iyb = fy - g.PY; while (iyb < 0) { iyb += g.SY; ++oyb; }
            long oxb = 0, ixb = fx - g.PX; while (ixb < 0) { ixb += g.SX; ++oxb; }
            float v = 0.f;
            for (long img = 0; img < g.B; ++img) {
              float const *ip = in + (img * g.in_chans() + c) * g.H * g.W, *op = ogl + (img * g.out_chans() + oc) * g.OH * g.OW;
              long oy = oyb;
              for (long iy = iyb; iy < g.H && oy < g.OH; iy += g.SY, ++oy) {
                long ox = oxb;
                for (long ix = ixb; ix < g.W && ox < g.OW; ix += g.SX, ++ox) v = fmaf(ip[iy * g.W + ix], op[oy * g.OW + ox], v);
              }
            }
            fgl[((oc * g.C + c) * g.KH + fy) * g.KW + fx] = v;
          }
  }
  static void bconv_biases(float const *ogl, float *bgl, conv_geom_c const &g) {
#pragma omp parallel for schedule(static)
    for (long oc = 0; oc < g.OC; ++oc) {
      float v = 0.f;
      for (long img = 0; img < g.B; ++img)
        for (long e = 0; e < g.OH * g.OW; ++e) v += ogl[(img * g.OC + oc) * g.OH * g.OW + e];
      bgl[oc] = v;
    }
  }
  // hip_operands=bf16: fp32 -> bf16 -> fp32, round to nearest even (what v_cvt_pk_bf16_f32 does).  Inf stays inf; a NaN stays a NaN (quiet, same sign, same top seven
  // mantissa bits); a finite value at or above the largest bf16's upper half ulp becomes inf
  static float rne_bf16(float v) {
    uint32_t u; memcpy(&u, &v, 4);
    if ((u & 0x7fffffffu) > 0x7f800000u) u = (u & 0xffff0000u) | 0x00400000u;
    else u = (u + 0x7fffu + ((u >> 16) & 1u)) & 0xffff0000u;
    float r; memcpy(&r, &u, 4);
    return r;
  }
  static std::vector<float> rounded_bf16(float const *p, size_t n) {
    std::vector<float> r(n);
#pragma omp parallel for schedule(static)
    for (long i = 0; i < (long)n; ++i) r[(size_t)i] = rne_bf16(p[i]);
    return r;
  }
  void run_bck(native_func_t const &f, op_base_t const &op, map_str_rtc_arg_t const &am) {
    string const fn = f.name;
    (void)op_bf16_operands(op);   // (refuses hip_operands=bf16 on hip_bconv_filts / hip_bconv_biases)
    string const ognm = var_of(am, "out_grad_loss");
    dims_t const og = get_var_dims(ognm); need_float(og, "out_grad_loss");
    if (og.sz() != 4) rt_err(fn + ": out_grad_loss must be img:chan:y:x");
    conv_geom_c g; memset(&g, 0, sizeof(g));
    g.B = og.dsz("img"); g.OC = og.dsz("chan"); g.OH = og.dsz("y"); g.OW = og.dsz("x");
    if (f.member == kBconvBiases) {
      string const bnm = var_of(am, "biases_grad_loss"); dims_t const b = get_var_dims(bnm); need_float(b, "biases_grad_loss");
      if (b.dims_prod() != (uint64_t)g.OC) rt_err(fn + ": biases_grad_loss must hold out_chan values");
      bconv_biases((float const *)must_find(vis, ognm).buf.get(), (float *)must_find(vis, bnm).buf.get(), g);
      return;
    }
    bool const din = f.member == kBconvIn;
    string const fnm = var_of(am, din ? "filts" : "filts_grad_loss"), inm = var_of(am, din ? "in_grad_loss" : "in");
    dims_t const fd = get_var_dims(fnm), in = get_var_dims(inm);
    need_float(fd, "filts"); need_float(in, "in");
    auto si = am.find("stride"), pi = am.find("in_pad");
    if (si == am.end() || pi == am.end()) rt_err(fn + ": 'stride' and 'in_pad' REF args are required");
    dims_t const stride = si->second.get_dims(*this), in_pad = pi->second.get_dims(*this);
    if (fd.sz() != 4 || in.sz() != 4 || stride.sz() != 2 || in_pad.sz() != 2) rt_err(fn + ": filts out_chan:in_chan:y:x, in img:chan:y:x, stride / in_pad y:x");
    g.C = in.dsz("chan"); g.H = in.dsz("y"); g.W = in.dsz("x"); g.KH = fd.dsz("y"); g.KW = fd.dsz("x");
    g.SY = stride.dsz("y"); g.SX = stride.dsz("x"); g.PY = in_pad.dsz("y"); g.PX = in_pad.dsz("x");
    if (!g.SY || !g.SX) rt_err(fn + ": zero stride");
    if (fd.dsz("out_chan") != (uint32_t)g.OC || fd.dsz("in_chan") != (uint32_t)g.C || in.dsz("img") != (uint32_t)g.B) rt_err(fn + ": inconsistent filts / in / out_grad_loss dims");
    if ((g.H + 2 * g.PY - g.KH) / g.SY + 1 != g.OH || (g.W + 2 * g.PX - g.KW) / g.SX + 1 != g.OW) rt_err(fn + ": out_grad_loss dims do not match in / filts / stride / in_pad");
    float const *zin = nullptr;
    if (din && op_zinp_flag(op)) {   // the forward input: the op's in dims (the image count the other vars'), and not the var this call writes
      string const znm = var_of(am, "in"); dims_t const zd = get_var_dims(znm); need_float(zd, "in");
      dims_t want = op.get_dims("in");
      if (want.sz() == 4 && zd.sz() == 4) { want[0].sz = (uint32_t)g.B; want.calc_strides(); }
      if (!(zd == want) || !(zd == in)) rt_err(fn + ": arg 'in' has dims " + zd.pretty_str() + ", the op says " + op.get_dims("in").pretty_str());
      if (znm == inm) rt_err(fn + ": zero_if_in_non_pos=1: 'in' and 'in_grad_loss' are the same var '" + znm + "'");
      zin = (float const *)must_find(vis, znm).buf.get();
    }
    if (f.member == kBconvFiltsBiases) {   // the two loops of hip_bconv_biases and hip_bconv_filts, one call: the bits of the two calls
      string const bnm = var_of(am, "biases_grad_loss"); dims_t const b = get_var_dims(bnm); need_float(b, "biases_grad_loss");
      if (b.dims_prod() != (uint64_t)g.OC) rt_err(fn + ": biases_grad_loss must hold out_chan values");
      for (string const *o : {&fnm, &bnm}) if (*o == inm || *o == ognm) rt_err(fn + ": the output var '" + *o + "' is also an input of the call");
      if (fnm == bnm) rt_err(fn + ": filts_grad_loss and biases_grad_loss are the same var '" + fnm + "'");
      bconv_biases((float const *)must_find(vis, ognm).buf.get(), (float *)must_find(vis, bnm).buf.get(), g);
    }
    if (op_bf16_operands(op)) {   // the operands of the products rounded to bf16 (copies), then the same template loops; biases (above) and the condition zin stay unrounded
      size_t const n_f = (size_t)g.OC * g.C * g.KH * g.KW, n_in = (size_t)g.B * g.C * g.H * g.W, n_og = (size_t)g.B * g.OC * g.OH * g.OW;
      std::vector<float> const og = rounded_bf16((float const *)must_find(vis, ognm).buf.get(), n_og);
      if (din) { std::vector<float> const fr = rounded_bf16((float const *)must_find(vis, fnm).buf.get(), n_f); bconv_in(fr.data(), og.data(), (float *)must_find(vis, inm).buf.get(), g, zin); }
      else { std::vector<float> const ir = rounded_bf16((float const *)must_find(vis, inm).buf.get(), n_in); bconv_filts(ir.data(), og.data(), (float *)must_find(vis, fnm).buf.get(), g); }
      return;
    }
    if (din) bconv_in((float const *)must_find(vis, fnm).buf.get(), (float const *)must_find(vis, ognm).buf.get(), (float *)must_find(vis, inm).buf.get(), g, zin);
    else bconv_filts((float const *)must_find(vis, inm).buf.get(), (float const *)must_find(vis, ognm).buf.get(), (float *)must_find(vis, fnm).buf.get(), g);
  }

  // the grouped family (hip_conv_grp, hip_bconv_in_grp, hip_bconv_filts_grp): for every group the ungrouped function's own loops above, on pointers offset by the
  // group's channels / filter rows, the image strides those of the whole tensors (conv_geom_c::CT / OCT).  Every var has exactly the dims the op gives its arg
  void run_conv_grp(native_func_t const &f, op_base_t const &op, map_str_rtc_arg_t const &am) {
    string const fn = f.name;
    conv_grp_geom_t const cg = conv_grp_geom_of_op(op, f.member);
    auto si = am.find("stride"), pi = am.find("in_pad");
    if (si == am.end() || pi == am.end()) rt_err(fn + ": 'stride' and 'in_pad' REF args are required");
    if (!(si->second.get_dims(*this) == op.get_dims("stride")) || !(pi->second.get_dims(*this) == op.get_dims("in_pad"))) rt_err(fn + ": stride / in_pad args disagree with the op");
    std::map<string, string> seen;   // var -> the arg it is bound to
    auto var_ptr = [&](char const *an) -> float * {
      string const vn = var_of(am, an); dims_t const vd = get_var_dims(vn); need_float(vd, an);
      if (!(vd == op.get_dims(an))) rt_err(fn + ": arg '" + an + "' has dims " + vd.pretty_str() + ", the op says " + op.get_dims(an).pretty_str());
      auto ins = seen.emplace(vn, an);
      if (!ins.second) rt_err(fn + ": args '" + ins.first->second + "' and '" + an + "' are the same var '" + vn + "'");
      return (float *)must_find(vis, vn).buf.get();
    };
    conv_geom_c g; memset(&g, 0, sizeof(g));
    g.B = cg.B; g.C = cg.CG; g.H = cg.H; g.W = cg.W; g.OC = cg.OCG; g.KH = cg.KH; g.KW = cg.KW; g.SY = cg.SY; g.SX = cg.SX; g.PY = cg.PY; g.PX = cg.PX; g.OH = cg.OH; g.OW = cg.OW;
    g.relu = cg.relu; g.CT = cg.C; g.OCT = cg.OC;
    long const f_grp = (long)cg.OCG * cg.CG * cg.KH * cg.KW, in_grp = (long)cg.CG * cg.H * cg.W, out_grp = (long)cg.OCG * cg.OH * cg.OW;
    if (f.member == kConvGrpFwd) {
      float const *filts = var_ptr("filts"), *biases = var_ptr("biases"), *in = var_ptr("in"); float *out = var_ptr("out");
      for (long j = 0; j < cg.G; ++j) conv(filts + j * f_grp, biases + j * cg.OCG, in + j * in_grp, out + j * out_grp, g);
    } else if (f.member == kConvGrpBckIn) {
      float const *filts = var_ptr("filts"), *ogl = var_ptr("out_grad_loss"); float *igl = var_ptr("in_grad_loss");
      for (long j = 0; j < cg.G; ++j) bconv_in(filts + j * f_grp, ogl + j * out_grp, igl + j * in_grp, g);
    } else {
      float const *in = var_ptr("in"), *ogl = var_ptr("out_grad_loss"); float *fgl = var_ptr("filts_grad_loss");
      for (long j = 0; j < cg.G; ++j) bconv_filts(in + j * in_grp, ogl + j * out_grp, fgl + j * f_grp, g);
    }
  }

  // the Deconvolution family (hip_deconv, hip_deconv_bck_in, hip_deconv_bck_biases, hip_deconv_bck_filts): the functions ARE the ungrouped loops above with the
  // operands' roles exchanged (native_funcs.h: deconv_geom_of_op) -- no second set of loops.  x is the geometry of the convolution OC -> C whose input plane is the
  // layer's out and whose output plane is the layer's in.  Every var has exactly the dims the op gives its arg
  void run_deconv(native_func_t const &f, op_base_t const &op, map_str_rtc_arg_t const &am) {
    string const fn = f.name;
    deconv_geom_t const dg = deconv_geom_of_op(op, f.member);
    std::map<string, string> seen;   // var -> the arg it is bound to
    auto var_ptr = [&](char const *an) -> float * {
      string const vn = var_of(am, an); dims_t const vd = get_var_dims(vn); need_float(vd, an);
      if (!(vd == op.get_dims(an))) rt_err(fn + ": arg '" + an + "' has dims " + vd.pretty_str() + ", the op says " + op.get_dims(an).pretty_str());
      auto ins = seen.emplace(vn, an);
      if (!ins.second) rt_err(fn + ": args '" + ins.first->second + "' and '" + an + "' are the same var '" + vn + "'");
      return (float *)must_find(vis, vn).buf.get();
    };
    conv_geom_c x; memset(&x, 0, sizeof(x));
    x.B = dg.B; x.C = dg.OC; x.H = dg.OH; x.W = dg.OW; x.OC = dg.C; x.KH = dg.KH; x.KW = dg.KW; x.SY = dg.SY; x.SX = dg.SX; x.PY = dg.PY; x.PX = dg.PX; x.OH = dg.H; x.OW = dg.W; x.relu = false;
    if (f.member == kDeconvBckBiases) {   // hip_bconv_biases on out_grad_loss, unchanged: its loop reads the image count, the channels and the plane of out_grad_loss
      conv_geom_c b; memset(&b, 0, sizeof(b)); b.B = dg.B; b.OC = dg.OC; b.OH = dg.OH; b.OW = dg.OW;
      float const *ogl = var_ptr("out_grad_loss");
      bconv_biases(ogl, var_ptr("biases_grad_loss"), b);
      return;
    }
    auto si = am.find("stride"), pi = am.find("in_pad");
    if (si == am.end() || pi == am.end()) rt_err(fn + ": 'stride' and 'in_pad' REF args are required");
    if (!(si->second.get_dims(*this) == op.get_dims("stride")) || !(pi->second.get_dims(*this) == op.get_dims("in_pad"))) rt_err(fn + ": stride / in_pad args disagree with the op");
    if (f.member == kDeconvFwd) {   // hip_bconv_in on (filts := filts, out_grad_loss := in) -> acc; out = acc + biases[oc], one fp32 add
      float const *filts = var_ptr("filts"), *biases = var_ptr("biases"), *in = var_ptr("in"); float *out = var_ptr("out");
      bconv_in(filts, in, out, x);
      long const OHW = (long)dg.OH * dg.OW;
#pragma omp parallel for schedule(static)
      for (long pl = 0; pl < (long)dg.B * dg.OC; ++pl) { float const b = biases[pl % dg.OC]; float *o = out + pl * OHW; for (long e = 0; e < OHW; ++e) o[e] = o[e] + b; }
    } else if (f.member == kDeconvBckIn) {   // hip_conv on (filts read as out_chan=C:in_chan=OC, C biases of +0, in := out_grad_loss), no ReLU
      float const *filts = var_ptr("filts"), *ogl = var_ptr("out_grad_loss"); float *igl = var_ptr("in_grad_loss");
      std::vector<float> const zeros((size_t)dg.C, 0.f);
      conv(filts, zeros.data(), ogl, igl, x);
    } else {   // hip_bconv_filts on (in := out_grad_loss, out_grad_loss := in)
      float const *in = var_ptr("in"), *ogl = var_ptr("out_grad_loss"); float *fgl = var_ptr("filts_grad_loss");
      bconv_filts(ogl, in, fgl, x);
    }
  }

  static float op_f32(op_base_t const &op, string const &an) {
    p_nda_t const &n = op.get(an);
    if (n->dims.tn != "float" || n->dims.sz() != 0 || !n->rp) rt_err("op: '" + an + "' is not a float scalar");
    return *static_cast<float const *>(n->rp);
  }
  // the gradient pipe's non-conv functions: every var must have the dims the op gives its arg (the image count only has to agree between the vars, as on be=hip)
  void run_bck_op(native_func_t const &f, op_base_t const &op, map_str_rtc_arg_t const &am) {
    string const fn = f.name; bck_op_args_t const d = bck_op_args(f, op);
    long n_img = -1;
    auto var_ptr = [&](string const &an) -> float * {
      string const vn = var_of(am, an); dims_t const vd = get_var_dims(vn); need_float(vd, an.c_str());
      dims_t want = op.get_dims(an);
      if (want.sz() >= 1 && want.names(0) == "img" && vd.sz() == want.sz()) {
        if (n_img < 0) n_img = vd.dims(0);
        if ((long)vd.dims(0) != n_img) rt_err(fn + ": arg '" + an + "' has " + std::to_string(vd.dims(0)) + " images, another arg " + std::to_string(n_img));
        want[0].sz = vd.dims(0); want.calc_strides();
      }
      if (!(vd == want)) rt_err(fn + ": arg '" + an + "' has dims " + vd.pretty_str() + ", the op says " + op.get_dims(an).pretty_str());
      return (float *)must_find(vis, vn).buf.get();
    };
    if (d.refs) for (char const *an : {"kern_sz", "stride", "in_pad"}) {
      auto ri = am.find(an);
      if (ri == am.end()) rt_err(fn + ": the REF arg '" + an + "' is required");
      if (!(ri->second.get_dims(*this) == op.get_dims(an))) rt_err(fn + ": arg '" + an + "' disagrees with the op");
    }
    float *in[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr}, *out[2] = {nullptr, nullptr};
    std::vector<string> const &in_ans = d.ins;   // (hip_reduce: ins_0 .. ins_{ins_num-1})
    for (size_t i = 0; i < in_ans.size(); ++i) in[i] = var_ptr(in_ans[i]);
    for (size_t i = 0; i < d.outs.size(); ++i) out[i] = var_ptr(d.outs[i]);
    bool const zinp = op_zinp_flag(op);
    float const *zin = nullptr;
    if (zinp) {   // the condition is the forward input `in` (hip_bck_lrn's first arg; one more var arg of hip_spreading), never the var the call writes
      zin = var_ptr("in");
      if (var_of(am, "in") == var_of(am, "in_grad_loss")) rt_err(fn + ": zero_if_in_non_pos=1: 'in' and 'in_grad_loss' are the same var '" + var_of(am, "in") + "'");
    }
    if (d.refs) {
      dims_t const &i4 = op.get_dims("in"), &o4 = op.get_dims("out"), &ks = op.get_dims("kern_sz"), &st = op.get_dims("stride"), &pad = op.get_dims("in_pad");
      if (i4.sz() != 4 || o4.sz() != 4) rt_err(fn + ": in / out must be img:chan:y:x");
      pool_geom_c g{n_img, (long)i4.dsz("chan"), (long)i4.dsz("y"), (long)i4.dsz("x"), (long)o4.dsz("y"), (long)o4.dsz("x"), (long)ks.dsz("y"), (long)ks.dsz("x"),
                    (long)st.dsz("y"), (long)st.dsz("x"), (long)pad.dsz("y"), (long)pad.dsz("x"), op.get_u32("avg_pool") != 0};
      if (g.KH < 1 || g.KW < 1 || g.SY < 1 || g.SX < 1) rt_err(fn + ": zero kern_sz / stride");
      bool const small = g.H + 2 * g.PY < g.KH || g.W + 2 * g.PX < g.KW;   // either padded dim below the window: a 1 x 1 output
      auto osz = [&](long in_sz, long k, long s, long pd) { return small ? 1 : (in_sz + 2 * pd - k + s - 1) / s + 1; };
      if (osz(g.H, g.KH, g.SY, g.PY) != g.OH || osz(g.W, g.KW, g.SX, g.PX) != g.OW) rt_err(fn + ": out plane does not follow from in / kern_sz / stride / in_pad");
      if (f.member == kOpPoolYx) {
        if (!op.get_u32("emit_out_in_yx") && !g.avg) unsup_err(fn + ": a Pooling with emit_out_in_yx=0 belongs to the forward pipe");
        pool_yx(in[0], out[0], out[1], g);
      } else spreading(in[1], in[2], out[0], g, zin);
    } else if (f.member == kOpLrnSb || f.member == kOpBckLrn) {
      dims_t const &i4 = op.get_dims("in");
      if (i4.sz() != 4) rt_err(fn + ": in must be img:chan:y:x");
      lrn_geom_c g{n_img, (long)i4.dsz("chan"), (long)i4.dsz("y") * i4.dsz("x"), (long)op.get_u32("local_size"), op_f32(op, "alpha"), op_f32(op, "beta"), op_f32(op, "k")};
      if (g.LS < 1 || g.LS % 2 == 0) unsup_err(fn + ": local_size=" + std::to_string(g.LS) + ": only odd windows (an even local_size has no centre channel)");
      if (f.member == kOpLrnSb) {
        if (!op.get_u32("emit_out_scale_base")) unsup_err(fn + ": an LRN with emit_out_scale_base=0 belongs to the forward pipe");
        lrn_sb(in[0], out[0], out[1], g);
      } else bck_lrn(in[0], in[1], in[2], in[3], out[0], g, zinp);
    } else if (f.member == kOpZeroIfNonPos) {
      zero_if_non_pos(in[0], in[1], out[0], (long)get_var_dims(var_of(am, "in")).dims_prod());
    } else if (f.member == kOpReduce) {
      dims_t const &od = op.get_dims("out");
      for (string const &an : in_ans) if (!(op.get_dims(an) == od)) rt_err(fn + ": " + an + " dims " + op.get_dims(an).pretty_str() + " differ from out's " + od.pretty_str());
      reduce(in, (int)in_ans.size(), out[0], (long)get_var_dims(var_of(am, "out")).dims_prod());
    } else if (f.member == kOpDropout) {
      float const ratio = op_f32(op, "dropout_ratio");
      if (!(ratio > 0.0f && ratio < 1.0f)) rt_err(fn + ": dropout_ratio=" + std::to_string(ratio) + " must lie inside (0, 1)");
      auto si = am.find("det_drop_seed");
      if (si == am.end() || !si->second.is_valid() || si->second.is_var() || !si->second.v->rp_elems() || si->second.v->dims.tn != "uint32_t" || si->second.v->dims.sz() != 0)
        rt_err(fn + ": 'det_drop_seed' must be a by-value uint32_t scalar of the call");
      uint32_t seed = *(uint32_t const *)si->second.v->rp_elems();
      if (op_seed_var_flag(op)) {   // the hash seed is the var's word + the by-value seed, a uint32 add that wraps
        auto wi = am.find("det_drop_seed_var");
        if (wi == am.end() || !wi->second.is_valid() || !wi->second.is_var()) rt_err(fn + ": seed_from_var=1: the var arg 'det_drop_seed_var' is required");
        check_seed_var(fn, wi->second.n, get_var_dims(wi->second.n), var_of(am, "inout"));
        seed += *(uint32_t const *)must_find(vis, wi->second.n).buf.get();
      }
      dropout(out[0], (long)get_var_dims(var_of(am, "inout")).dims_prod(), ratio, seed);
    } else if (f.member == kOpChanAffine) {
      dims_t const &i4 = op.get_dims("in");
      if (i4.sz() != 4 || !(op.get_dims("out") == i4)) rt_err(fn + ": in and out must be img:chan:y:x tensors of equal dims");
      for (char const *an : {"a", "b"}) if (op.get_dims(an).sz() != 1 || op.get_dims(an).dims(0) != i4.dims(1)) rt_err(fn + ": " + an + " dims " + op.get_dims(an).pretty_str() + ": one float per channel of in " + i4.pretty_str());
      uint32_t const relu = op.get_u32("relu");
      if (relu > 1) rt_err(fn + ": relu must be 0 | 1");
      chan_affine(in[0], in[1], in[2], out[0], n_img, (long)i4.dsz("chan"), (long)i4.dsz("y") * i4.dsz("x"), relu != 0);
    } else if (f.member == kOpCrop || f.member == kOpCropBck) {   // the window of the op's offset; the gradient writes +0 outside it
      bool const fwd = f.member == kOpCrop;
      dims_t const &big = op.get_dims(fwd ? "in" : "in_grad_loss"), &win = op.get_dims(fwd ? "out" : "out_grad_loss"), &off = op.get_dims("offset");
      if (big.sz() != 4 || win.sz() != 4 || off.sz() != 2 || big.dims(0) != win.dims(0) || big.dims(1) != win.dims(1)) rt_err(fn + ": plane and window must be img:chan:y:x tensors of equal img / chan, offset y:x");
      long const H = big.dims(2), W = big.dims(3), OH = win.dims(2), OW = win.dims(3), oy = off.dsz("y"), ox = off.dsz("x");
      if (oy + OH > H || ox + OW > W)
        rt_err(fn + ": offset (" + std::to_string(oy) + ", " + std::to_string(ox) + ") + window (" + std::to_string(OH) + ", " + std::to_string(OW) + ") exceeds the plane (" + std::to_string(H) + ", " + std::to_string(W) + ")");
      long const planes = n_img * (long)big.dims(1);
#pragma omp parallel for schedule(static)
      for (long pl = 0; pl < planes; ++pl) {
        if (fwd) { for (long y = 0; y < OH; ++y) for (long x = 0; x < OW; ++x) out[0][(pl * OH + y) * OW + x] = in[0][(pl * H + y + oy) * W + x + ox]; }
        else for (long y = 0; y < H; ++y) for (long x = 0; x < W; ++x) {
          bool const inside = y >= oy && y < oy + OH && x >= ox && x < ox + OW;
          out[0][(pl * H + y) * W + x] = inside ? in[0][(pl * OH + y - oy) * OW + x - ox] : 0.0f;
        }
      }
    } else if (f.member == kOpConcat || f.member == kOpSplit) {
      bool const cat = f.member == kOpConcat;
      dims_t const &i4 = op.get_dims("in"), &o4 = op.get_dims("out");
      if (i4.sz() != 4 || o4.sz() != 4) rt_err(fn + ": in / out must be img:chan:y:x");
      dims_t const &nar = cat ? i4 : o4, &wid = cat ? o4 : i4;
      if (nar.dims(0) != wid.dims(0) || nar.dims(2) != wid.dims(2) || nar.dims(3) != wid.dims(3)) rt_err(fn + ": in " + i4.pretty_str() + " and out " + o4.pretty_str() + " differ in img / y / x");
      long const hw = (long)nar.dims(2) * nar.dims(3), cix = op.get_u32(cat ? "ocix" : "icix");
      if (cix + (long)nar.dims(1) > (long)wid.dims(1)) rt_err(fn + ": channels [" + std::to_string(cix) + ", " + std::to_string(cix + (long)nar.dims(1)) + ") do not fit the wide tensor's " + std::to_string(wid.dims(1)));
      copy_chan_range(in[0], out[0], n_img, (long)nar.dims(1) * hw, (long)wid.dims(1) * hw, cix * hw, cat);
    } else {
      dims_t const &i4 = op.get_dims("in");
      if (i4.sz() != 4 || i4.dims(2) != 1 || i4.dims(3) != 1) unsup_err(fn + ": only 1 x 1 planes (in img:chan:1:1, label img:1:1): the reference reads label by image");
      long const C = i4.dsz("chan");
      if (f.member == kOpSoftmax) softmax(in[0], out[0], n_img, C);
      else if (f.member == kOpSmGradAndLoss) sm_grad_and_loss(in[0], in[1], out[0], out[1], n_img, C);
      else sum_loss_over_imgs(in[0], out[0], n_img);
    }
  }

  // hip_sgd_update: the checks of be=hip (csrc/native_run.cc), then the loop per tensor with lr_i / wd_i formed once
  void run_sgd_update(op_base_t const &op, map_str_rtc_arg_t const &am) {
    string const fn = op.get_func_name();
    sgd_op_t const so = sgd_op_of_op(op);
    std::map<string, string> seen;   // var -> the arg it is bound to
    auto var_ptr = [&](string const &an) -> float * {
      string const vn = var_of(am, an); dims_t const vd = get_var_dims(vn);
      if (vd.tn != "float") rt_err(fn + ": arg '" + an + "' (var '" + vn + "') has type " + vd.tn + ": the update is fp32 only");
      if (!(vd == op.get_dims(an))) rt_err(fn + ": arg '" + an + "' has dims " + vd.pretty_str() + ", the op says " + op.get_dims(an).pretty_str());
      auto ins = seen.emplace(vn, an);
      if (!ins.second) rt_err(fn + ": args '" + ins.first->second + "' and '" + an + "' are the same var '" + vn + "'");
      return (float *)must_find(vis, vn).buf.get();
    };
    size_t const n = so.elems.size();
    std::vector<float *> w(n), h(n); std::vector<float const *> g(n);
    for (size_t i = 0; i < n; ++i) { string const sx = "_" + std::to_string(i); w[i] = var_ptr("w" + sx); g[i] = var_ptr("g" + sx); h[i] = var_ptr("h" + sx); }
    float const *hy = var_ptr("hyper");
    float const lr = hy[0], mom = hy[1], wd = hy[2];
    for (size_t i = 0; i < n; ++i) {
      float const lr_i = lr * so.lr_mult[i], wd_i = wd * so.decay_mult[i];   // (one fp32 multiply each)
      sgd_update(w[i], g[i], h[i], so.elems[i], lr_i, wd_i, mom);
    }
  }

  // the solver family: the checks of be=hip (csrc/native_run.cc), then the twins above with the per-tensor scalars formed once
  void run_solver(op_base_t const &op, map_str_rtc_arg_t const &am) {
    string const fn = op.get_func_name();
    solver_op_t const so = solver_op_of_op(op);
    std::map<string, string> seen;   // var -> the arg it is bound to
    auto var_ptr = [&](string const &an) -> float * {
      string const vn = var_of(am, an); dims_t const vd = get_var_dims(vn);
      if (vd.tn != "float") rt_err(fn + ": arg '" + an + "' (var '" + vn + "') has type " + vd.tn + ": the solver is fp32 only");
      if (!(vd == op.get_dims(an))) rt_err(fn + ": arg '" + an + "' has dims " + vd.pretty_str() + ", the op says " + op.get_dims(an).pretty_str());
      auto ins = seen.emplace(vn, an);
      if (!ins.second) rt_err(fn + ": args '" + ins.first->second + "' and '" + an + "' are the same var '" + vn + "'");
      return (float *)must_find(vis, vn).buf.get();
    };
    size_t const n = so.elems.size();
    if (so.update()) {
      std::vector<float *> w(n), h(n), v(n, nullptr); std::vector<float const *> g(n);
      for (size_t i = 0; i < n; ++i) {
        string const sx = "_" + std::to_string(i);
        w[i] = var_ptr("w" + sx); g[i] = var_ptr("g" + sx); h[i] = var_ptr("h" + sx); if (so.type == kSolverAdam) v[i] = var_ptr("h2" + sx);
      }
      float const *hy = var_ptr("hyper"); float const *st = var_ptr("state");
      float const *ac = so.kind == 5 ? var_ptr("accum") : nullptr;
      if (ac && ac[1] == 0.0f) return;   // (not the applying micro-step: nothing is written)
      for (size_t i = 0; i < n; ++i) {
        solver_coef_c k;
        k.lr = hy[0] * so.lr_mult[i]; k.wd = hy[2] * so.decay_mult[i]; k.mom = hy[1]; k.mom2 = hy[3]; k.delta = hy[4];
        k.coef = so.clip ? st[0] : 1.0f;
        k.c = 1.0f + k.mom; k.o1 = 1.0f - k.mom; k.o2 = 1.0f - k.mom2; k.s = k.lr * hy[5]; k.lrwd = k.lr * k.wd;
        k.scale = ac ? ac[2] : 1.0f;
        solver_update(so.type, so.clip, so.decoupled_wd, ac != nullptr, w[i], g[i], h[i], v[i], so.elems[i], k);
      }
    } else if (so.kind == 4) {
      std::vector<float const *> g(n); std::vector<float *> a(n);
      for (size_t i = 0; i < n; ++i) { string const sx = "_" + std::to_string(i); g[i] = var_ptr("g" + sx); a[i] = var_ptr("a" + sx); }
      float const *ac = var_ptr("accum");
      for (size_t i = 0; i < n; ++i) grad_accum(ac[0] != 0.0f, g[i], a[i], so.elems[i]);
    } else if (so.kind == 2) {
      std::vector<float const *> g(n);
      for (size_t i = 0; i < n; ++i) g[i] = var_ptr("g_" + std::to_string(i));
      float *const partials = var_ptr("partials");
      long k = so.part0;
      for (size_t i = 0; i < n; ++i)
        for (long e0 = 0; e0 < so.elems[i]; e0 += kSolverChunk, ++k) partials[k] = solver_chunk_sumsq(g[i] + e0, std::min(kSolverChunk, so.elems[i] - e0));
    } else {
      float const *partials = var_ptr("partials"); float const *hy = var_ptr("hyper");
      solver_grad_norm(partials, so.parts, hy[6], var_ptr("state"));
    }
  }

  // the training BatchNorm functions and hip_fan_out: the checks of be=hip (csrc/native_run.cc), then the twins above
  void run_bn(op_base_t const &op, map_str_rtc_arg_t const &am) {
    string const fn = op.get_func_name();
    bn_op_t b = bn_op_of_op(op);
    vect_string vars; std::vector<float *> T, Cv;
    long n_img = -1;   // of the tensor vars of a hip_bnc_* call, which leaves the image count free as on be=hip (it only has to agree between the vars)
    auto var_ptr = [&](string const &an) -> float * {
      string const vn = var_of(am, an); dims_t const vd = get_var_dims(vn);
      if (vd.tn != "float") rt_err(fn + ": arg '" + an + "' (var '" + vn + "') has type " + vd.tn + ": fp32 only");
      dims_t want = op.get_dims(an);
      if (b.bnc && want.sz() == 4 && vd.sz() == 4) {
        if (n_img < 0) n_img = vd.dims(0);
        if ((long)vd.dims(0) != n_img) rt_err(fn + ": arg '" + an + "' has " + std::to_string(vd.dims(0)) + " images, another arg " + std::to_string(n_img));
        want[0].sz = vd.dims(0); want.calc_strides();
      }
      if (!(vd == want)) rt_err(fn + ": arg '" + an + "' has dims " + vd.pretty_str() + ", the op says " + op.get_dims(an).pretty_str());
      vars.push_back(vn);
      return (float *)must_find(vis, vn).buf.get();
    };
    for (string const &an : b.tens) T.push_back(var_ptr(an));
    for (string const &an : b.chans) Cv.push_back(var_ptr(an));
    bn_check_aliases(fn, b, vars);
    if (b.bnc && (b.kind == 2 || b.kind == 4)) b = bn_op_on_imgs(b, n_img);
    else if (b.bnc && n_img != b.B) rt_err(fn + ": the call's vars hold " + std::to_string(n_img) + " images, the op says " + std::to_string(b.B) + ": the sums run over the whole batch (a multi-device backend runs them per shard)");
    switch (b.kind) {
    case 1: bn_stats(b, T[0], Cv[0], Cv[1], Cv[2], Cv[3]); break;
    case 2: bn_fwd(b, T[0], T[1], Cv[0], Cv[1], Cv[2], Cv[3]); break;
    case 3: bn_bck_sums(b, T[0], T[1], Cv[0], Cv[1], Cv[2], Cv[3]); break;
    case 4: bn_bck_in(b, T[0], T[1], T[2], Cv[0], Cv[1], Cv[2], Cv[3], Cv[4]); break;
    case 6: bnf_prep(b, Cv[0], Cv[1], Cv[2], Cv[3]); break;
    case 7: bnf_bck(b, T[0], T[1], T[2], Cv[0], Cv[1], Cv[2], Cv[3], Cv[4]); break;
    case 8: bnf_bck_in(b, T[0], T[1], Cv[0], Cv[1]); break;
    default: for (int i = 0; i < b.nout; ++i) memcpy(T[(size_t)(1 + i)], T[0], sizeof(float) * (size_t)b.elems);
    }
  }

  // the eval family: the checks of be=hip (csrc/native_run.cc), then the twins above
  void run_eval(op_base_t const &op, map_str_rtc_arg_t const &am) {
    string const fn = op.get_func_name();
    eval_op_t e = eval_op_of_op(op);
    std::map<string, string> seen;   // var -> the arg it is bound to
    std::vector<void *> P; long n_img = -1;
    for (string const &an : e.args) {
      string const vn = var_of(am, an); dims_t const vd = get_var_dims(vn);
      dims_t want = op.get_dims(an);
      if (vd.tn != want.tn) rt_err(fn + ": arg '" + an + "' (var '" + vn + "') has type " + vd.tn + ", the op says " + want.tn);
      if (e.kind == 1 && vd.sz() == want.sz() && vd.sz() >= 1) {
        if (n_img < 0) n_img = vd.dims(0);
        if ((long)vd.dims(0) != n_img) rt_err(fn + ": arg '" + an + "' has " + std::to_string(vd.dims(0)) + " images, another arg " + std::to_string(n_img));
        want[0].sz = vd.dims(0); want.calc_strides();
      }
      if (!(vd == want)) rt_err(fn + ": arg '" + an + "' has dims " + vd.pretty_str() + ", the op says " + op.get_dims(an).pretty_str());
      auto ins = seen.emplace(vn, an);
      if (!ins.second) rt_err(fn + ": args '" + ins.first->second + "' and '" + an + "' are the same var '" + vn + "'");
      P.push_back(must_find(vis, vn).buf.get());
    }
    if (e.kind == 1) accuracy((float const *)P[0], (float const *)P[1], (uint32_t *)P[2], n_img, e.C);
    else if (e.kind == 2) eval_accum((uint32_t const *)P[0], (float const *)P[1], (uint32_t const *)P[2], (uint32_t *)P[3], (float *)P[4], e.B, e.top_k);
    else bn_fold((float const *)P[0], (float const *)P[1], (float const *)P[2], (float const *)P[3], (float *)P[4], (float *)P[5], e.C, e.eps);
  }

  // the loss family: the checks of be=hip (csrc/native_run.cc), then the twins above
  void run_loss(op_base_t const &op, map_str_rtc_arg_t const &am) {
    string const fn = op.get_func_name();
    loss_op_t const l = loss_op_of_op(op);
    std::map<string, string> seen;   // var -> the arg it is bound to
    std::vector<float *> P;
    for (string const &an : l.args) {
      string const vn = var_of(am, an); dims_t const vd = get_var_dims(vn);
      dims_t const &want = op.get_dims(an);
      if (vd.tn != want.tn) rt_err(fn + ": arg '" + an + "' (var '" + vn + "') has type " + vd.tn + ", the op says " + want.tn);
      if (!(vd == want)) rt_err(fn + ": arg '" + an + "' has dims " + vd.pretty_str() + ", the op says " + want.pretty_str());
      auto ins = seen.emplace(vn, an);
      if (!ins.second) rt_err(fn + ": args '" + ins.first->second + "' and '" + an + "' are the same var '" + vn + "'");
      P.push_back((float *)must_find(vis, vn).buf.get());
    }
    if (l.kind == 1) softmax_loss_fwd(l, P[0], P[1], P[2], P[3]);
    else if (l.kind == 2) loss_norm(l, P[0], P[1], P[2], P[3]);
    else softmax_loss_bck(l, P[0], P[1], P[2], P[3]);
  }

  // the data family: the checks of be=hip (csrc/native_run.cc), then the twin above
  void run_data(op_base_t const &op, map_str_rtc_arg_t const &am) {
    string const fn = op.get_func_name();
    data_op_t d = data_op_of_op(op);
    std::map<string, string> seen;   // var -> the arg it is bound to
    std::vector<void *> P; long n_img = -1;
    for (string const &an : d.args) {
      string const vn = var_of(am, an);
      auto ins = seen.emplace(vn, an);
      if (!ins.second) rt_err(fn + ": args '" + ins.first->second + "' and '" + an + "' are the same var '" + vn + "'");
      dims_t const vd = get_var_dims(vn);
      dims_t want = op.get_dims(an);
      if (vd.tn != want.tn) rt_err(fn + ": arg '" + an + "' (var '" + vn + "') has type " + vd.tn + ", the op says " + want.tn);
      if (an != "mean" && vd.sz() == want.sz() && vd.sz() >= 1) {
        if (n_img < 0) n_img = vd.dims(0);
        if ((long)vd.dims(0) != n_img) rt_err(fn + ": arg '" + an + "' has " + std::to_string(vd.dims(0)) + " images, another arg " + std::to_string(n_img));
        want[0].sz = vd.dims(0); want.calc_strides();
      }
      if (!(vd == want)) rt_err(fn + ": arg '" + an + "' has dims " + vd.pretty_str() + ", the op says " + op.get_dims(an).pretty_str());
      P.push_back(must_find(vis, vn).buf.get());
    }
    d.B = n_img;
    if (4.0 * (double)d.out_elems() >= 2147483648.0 || (double)d.B * d.C * d.H * d.W >= 2147483648.0) unsup_err(fn + ": tensors of 2 GiB or more");
    data_transform(d, (unsigned char const *)P[0], (uint32_t const *)P[1], (float const *)P[2], (float *)P[3]);
  }

  uint32_t run(rtc_func_call_t const &rfc) override {
    assert_st(init_done);
    auto fit = funcs.find(rfc.rtc_func_name);
    if (fit == funcs.end()) rt_err("run: unknown function '" + rfc.rtc_func_name + "' (not compiled, or released)");
    rtc_func_info_t const &fi = fit->second.info;
    native_func_t const &f = *fit->second.row;
    map_str_rtc_arg_t const &am = rfc.arg_map;
    (void)op_seed_var_flag(fi.op);   // (refuses the flag on a function that cannot take it)
    (void)op_img_shards_flag(fi.op);   // (likewise)
    double const tb = now_ms();
    if (f.family == kFamSgd) run_sgd_update(fi.op, am);
    else if (f.family == kFamBn || f.family == kFamBnc || f.family == kFamBnf) run_bn(fi.op, am);
    else if (f.family == kFamSolver) run_solver(fi.op, am);
    else if (f.family == kFamEval) run_eval(fi.op, am);
    else if (f.family == kFamData) run_data(fi.op, am);
    else if (f.family == kFamLoss) run_loss(fi.op, am);
    else if (f.family == kFamBckOp) run_bck_op(f, fi.op, am);
    else if (f.family == kFamBconv) run_bck(f, fi.op, am);
    else if (f.family == kFamConvGrp) run_conv_grp(f, fi.op, am);
    else if (f.family == kFamDeconv) run_deconv(f, fi.op, am);
    else if (f.family == kFamSgemm) {
      string const an = var_of(am, "a"), bn = var_of(am, "b"), cn = var_of(am, "c");
      dims_t const a = get_var_dims(an), b = get_var_dims(bn), c = get_var_dims(cn);
      need_float(a, "a"); need_float(b, "b"); need_float(c, "c");
      assert_st(a.sz() == 2 && b.sz() == 2 && c.sz() == 2);
      assert_st(a.names(0) == "K" && a.names(1) == "M" && b.names(0) == "K" && b.names(1) == "N" && c.names(0) == "M" && c.names(1) == "N");
      uint32_t const M = a.dsz("M"), K = a.dsz("K"), N = b.dsz("N");
      assert_st(b.dsz("K") == K); assert_st(c.dsz("M") == M); assert_st(c.dsz("N") == N);
      sgemm((float const *)must_find(vis, an).buf.get(), (float const *)must_find(vis, bn).buf.get(), (float *)must_find(vis, cn).buf.get(), M, N, K);
    } else {
      string const fnm = var_of(am, "filts"), bnm = var_of(am, "biases"), inm = var_of(am, "in"), onm = var_of(am, "out");
      dims_t const f = get_var_dims(fnm), bi = get_var_dims(bnm), in = get_var_dims(inm), out = get_var_dims(onm);
      need_float(f, "filts"); need_float(bi, "biases"); need_float(in, "in"); need_float(out, "out");
      auto si = am.find("stride"), pi = am.find("in_pad");
      if (si == am.end() || pi == am.end()) rt_err("hip_conv: 'stride' and 'in_pad' REF args are required");
      dims_t const stride = si->second.get_dims(*this), in_pad = pi->second.get_dims(*this);
      assert_st(f.sz() == 4 && in.sz() == 4 && out.sz() == 4 && bi.sz() == 1 && stride.sz() == 2 && in_pad.sz() == 2);
      conv_geom_c g; memset(&g, 0, sizeof(g));
      g.B = in.dsz("img"); g.C = in.dsz("chan"); g.H = in.dsz("y"); g.W = in.dsz("x"); g.OC = f.dsz("out_chan"); g.KH = f.dsz("y"); g.KW = f.dsz("x");
      g.SY = stride.dsz("y"); g.SX = stride.dsz("x"); g.PY = in_pad.dsz("y"); g.PX = in_pad.dsz("x"); g.OH = out.dsz("y"); g.OW = out.dsz("x");
      g.relu = fi.op.get_u32("conv_has_relu") != 0;
      if (f.dsz("in_chan") != (uint32_t)g.C) rt_err("hip_conv: filts.in_chan != in.chan");
      if (bi.dsz("out_chan") != (uint32_t)g.OC || out.dsz("chan") != (uint32_t)g.OC || out.dsz("img") != (uint32_t)g.B) rt_err("hip_conv: inconsistent biases/out dims");
      if (!g.SY || !g.SX) rt_err("hip_conv: zero stride");
      if ((g.H + 2 * g.PY - g.KH) / g.SY + 1 != g.OH || (g.W + 2 * g.PX - g.KW) / g.SX + 1 != g.OW) rt_err("hip_conv: out dims do not match in/filts/stride/in_pad");
      conv((float const *)must_find(vis, fnm).buf.get(), (float const *)must_find(vis, bnm).buf.get(), (float const *)must_find(vis, inm).buf.get(),
           (float *)must_find(vis, onm).buf.get(), g);
    }
    call_t.emplace_back(tb, now_ms());
    return (uint32_t)call_t.size() - 1;
  }
  void finish_and_sync() override {}
  void release_per_call_id_data() override { call_t.clear(); }
  float get_dur(uint32_t const &b, uint32_t const &e) override {
    if (b >= call_t.size() || e >= call_t.size()) rt_err("invalid call_id");
    return (float)(call_t[e].second - call_t[b].first);
  }
  void profile_start() override {}
  void profile_stop() override {}
};

p_rtc_compute_t make_cpu_compute() { return std::make_shared<cpu_compute_t>(); }

} // namespace bodahip
