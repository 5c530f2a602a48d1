// kernel_args.h -- everything that crosses the launch boundary: the structs passed by value to a kernel or copied into a device-side table, each declared ONCE.
// The host includes this file inside namespace bodahip (native_internal.h); every kernels/*.hip includes it at global scope (hiprtc gets it as an in-memory
// header, a direct hipcc compile finds it next to the source).  Plain C++17, no includes, no HIP runtime: both compilers evaluate the layout assertions below.
#ifndef BODAHIP_KERNEL_ARGS_H
#define BODAHIP_KERNEL_ARGS_H

// Some field names below are also -D parameters of one kernel or another (never of the kernel that reads the field): those macros are set aside while the
// structs are declared and come back at the end of the file.
#pragma push_macro("CH")
#undef CH
#pragma push_macro("CIN")
#undef CIN
#pragma push_macro("COH")
#undef COH
#pragma push_macro("COW")
#undef COW
#pragma push_macro("CW")
#undef CW
#pragma push_macro("H")
#undef H
#pragma push_macro("HW")
#undef HW
#pragma push_macro("KH")
#undef KH
#pragma push_macro("KW")
#undef KW
#pragma push_macro("OH")
#undef OH
#pragma push_macro("OW")
#undef OW
#pragma push_macro("PX")
#undef PX
#pragma push_macro("PY")
#undef PY
#pragma push_macro("SX")
#undef SX
#pragma push_macro("SY")
#undef SY
#pragma push_macro("W")
#undef W

// the contraction kernels (sgemm, every forward convolution): one struct serves them all
struct gemm_args_t {
  float const *I; float const *J; float *D; float const *bias;   // (the bf16 kernels: I = filts / re-laid-out filters, J = in, D = out behind these pointer types)
  int Mi, Nj, K;          // extents of i, j, k
  int ldI, ldJ, ldD;      // row pitches (elements) of I, J (k-major: per k row; i/j-major: per i/j row) and of D per i
  int C, H, W, OH, OW;    // convolution geometry (J_MODE 2 / EPI 1)
  int tiles_i, tiles_j;   // (k1_quad: out_chan tiles | super-blocks of WJ blocks of 128 pels each)
  int splitk, kt_per;     // SPLITK: number of K slices, K-tiles per slice  (k1_quad: kt_per = workgroups per out_chan tile == the super-block stride of a workgroup)
  float *ws; long ws_slab; // SPLITK: partial-sum slabs, ws_slab elements apart
  unsigned I_bytes, J_bytes; // sizes of the I / J tensors (buffer-descriptor num_records; host guarantees <= 2^31)
  unsigned D_bytes;             // size of the output tensor (host guarantees < 2^32: 32-bit store offsets)
  int out_ctot, out_coff;      // EPI 1: channels of the output tensor and first channel written (== Mi, 0 unless the conv writes a slice
                               // of a wider tensor: Concat elimination)
  int const *ktab; int ktab_n; // J_MODE 2: per-k gather tables, three arrays of ktab_n ints: element offset of (in_chan,ky,kx)
                               // inside one image | ky | kx ; rows k >= K carry ky = 2^30 (fail the row-range test)
  long bsI, bsJ, bsD;          // batched launches (gridDim.y problems of one shape, e.g. the 16 Winograd-domain sgemms): element strides of I / J / D per blockIdx.y
};
static_assert(sizeof(gemm_args_t) == 176 && __builtin_offsetof(gemm_args_t, Mi) == 32 && __builtin_offsetof(gemm_args_t, ws) == 96 && __builtin_offsetof(gemm_args_t, I_bytes) == 112 &&
              __builtin_offsetof(gemm_args_t, ktab) == 136 && __builtin_offsetof(gemm_args_t, ktab_n) == 144 && __builtin_offsetof(gemm_args_t, bsI) == 152, "gemm_args_t layout");

// kernels/k1_quad_f32.hip -DCHAIN=1: gemm_args_t followed by the second convolution of a 1x1 chain -- its filters (M2 x MID) / biases, its out_chan count, and the
// optional copy of the intermediate tensor (img:MID:pel).
struct chain_args_t : gemm_args_t {
  float const *I2; float const *bias2; float *Dmid;
  int M2; unsigned I2_bytes, Dmid_bytes;
};
static_assert(sizeof(chain_args_t) == 216, "chain_args_t layout");

// GROUPS (kernels/conv_nhwc_bf16.hip): member m owns fused out_chans [oc0[m], oc0[m] + noc[m]) (oc0[m] multiples of the pad granularity; rows up to oc0[m+1] are zero padding)
struct grp_args_t {
  int n; int oc0[4]; int noc[4];
  void *D[4]; unsigned D_bytes[4]; int ctot[4]; int coff[4];
};
static_assert(sizeof(grp_args_t) == 120 && __builtin_offsetof(grp_args_t, D) == 40 && __builtin_offsetof(grp_args_t, D_bytes) == 72 && __builtin_offsetof(grp_args_t, coff) == 104, "grp_args_t layout");

// hip_conv_nhwc_set's wrapper kernel: member tables in device memory (m, g: one entry per member; ends: running tile counts; variant: the member's code)
struct set_args_t { gemm_args_t const *m; int const *ends; int const *variant; grp_args_t const *g; int n; };
static_assert(sizeof(set_args_t) == 40 && __builtin_offsetof(set_args_t, n) == 32, "set_args_t layout");

// kernels/conv_nhwc_multi_bf16.hip: one member convolution (128 bytes), one tile of the launch, the launch
struct multi_prob_t {
  void const *I; void const *J; void *D; float const *bias;     // filts, in, out, biases
  unsigned I_bytes, J_bytes, D_bytes; int Mi;                    // buffer extents; out_chans
  int Nj, CIN, KH, KW;                                           // output positions (img * oy * ox); stored in_chans (% 8 == 0); window
  int SY, SX, PY, PX;
  int CH, CW, COH, COW;                                          // input plane, output plane
  int kCG, kKC, nK, relu;                                        // chunks per tap (CIN / 8), chunks along k (taps * kCG), K steps, ReLU
  int out_ctot, out_coff, tiles_i, tiles_j;
};
struct multi_tile_t { int prob, tile_i, tile_j, pad; };
struct multi_args_t { multi_prob_t const *probs; multi_tile_t const *tiles; int n_tiles; int n_probs; };
static_assert(sizeof(multi_prob_t) == 128 && __builtin_offsetof(multi_prob_t, I_bytes) == 32 && __builtin_offsetof(multi_prob_t, Nj) == 48, "multi_prob_t layout");
static_assert(sizeof(multi_tile_t) == 16 && sizeof(multi_args_t) == 24 && __builtin_offsetof(multi_args_t, n_tiles) == 16, "multi_tile_t / multi_args_t layout");

// kernels/conv_nhwc_rows_bf16.hip
struct rows_args_t {
  void const *filts; void const *in; void *out; float const *bias;
  int n_img, oc;           // images; out_chans (<= 64)
  unsigned filts_bytes, in_bytes, out_bytes;
  int out_ctot, out_coff;  // channels of the output tensor's rows, first channel this convolution writes
  int n_chunks, rows_per_chunk;   // workgroups per image; output rows (pooled rows if PKH) each of them owns
  float lrn_alpha, lrn_beta, lrn_k;
};
static_assert(sizeof(rows_args_t) == 80 && __builtin_offsetof(rows_args_t, n_img) == 32 && __builtin_offsetof(rows_args_t, filts_bytes) == 40 && __builtin_offsetof(rows_args_t, lrn_alpha) == 68, "rows_args_t layout");

// kernels/conv_patch_bf16.hip -DS2D_ONLY: the space-to-depth front end
struct s2d_args_t {
  float const *src; float *dst;
  int B, C, H, W, OC, KH, KW;       // source tensor geometry (filters: OC, C, KH, KW)
  int S, C2, H2, W2;                // block size; channels (padded to a multiple of 8), rows, cols of the result (filters: rows = KHb, cols = KWb)
  int oy, ox;                       // input: Pr (rounded-up pad) per axis; filters: Pr - P per axis
  int filt;                         // 0: input tensor, 1: filters
  int mode, c2_lo;                  // mode 0: one thread per result element with channel >= c2_lo (filters; the zero pad channels of the input)
};                                  // mode 1: one thread per (b, c, Y, dy, X): S consecutive source pixels -> S channel planes (reads and writes coalesced)
static_assert(sizeof(s2d_args_t) == 80 && __builtin_offsetof(s2d_args_t, B) == 16 && __builtin_offsetof(s2d_args_t, c2_lo) == 76, "s2d_args_t layout");

// kernels/winograd_f32.hip
struct wino_args_t {
  float const *in; float const *filts; float const *bias; float *out;
  float *U; float *V; float *M;
  int B0, Bc;                 // first image and number of images of this chunk
  int C, H, W, OC, OH, OW;
  int TH, TW, Tc;             // tiles per image (rows, cols), tiles in the chunk = Bc*TH*TW
  int PY, PX, relu;
  int out_ctot, out_coff;     // channels of the output tensor, first channel written
};
static_assert(sizeof(wino_args_t) == 120 && __builtin_offsetof(wino_args_t, B0) == 56 && __builtin_offsetof(wino_args_t, out_ctot) == 112, "wino_args_t layout");

// kernels/bconv_in_f32.hip, bconv_in_bf16.hip, bconv_filts_f32.hip
struct bconv_args_t {
  float const *a; float const *b; float *d;   // bconv_in: a = filts, b = out_grad_loss, d = in_grad_loss; filts gradient: a = out_grad_loss, b = in, d = filts_grad_loss;
                                              // bias gradient: a = out_grad_loss, d = biases_grad_loss
  float *ws; long ws_slab;                    // K slices: tile tickets first, the slabs from ws + ws_slab on
  int B, C, H, W, OC, OH, OW;
  int tiles_i, tiles_j, ksl, kt_per;
  unsigned a_bytes, b_bytes, d_bytes;
  float const *zin;   // bconv_in -DZINP=1: the forward input (in_grad_loss's dims), the condition of the select on the store
};
static_assert(sizeof(bconv_args_t) == 104 && __builtin_offsetof(bconv_args_t, ws) == 24 && __builtin_offsetof(bconv_args_t, B) == 40 && __builtin_offsetof(bconv_args_t, a_bytes) == 84 &&
              __builtin_offsetof(bconv_args_t, zin) == 96, "bconv_args_t layout");

// kernels/bconv_fb_f32.hip, bconv_fb_bf16.hip
struct bconv_fb_args_t {
  float const *g; float const *x; float *df; float *db;   // out_grad_loss, in, filts_grad_loss, biases_grad_loss
  float *ws; long slab_elems;                             // SLICED: ksl slabs of slab_elems = OC*NJ + OC floats
  int B, C, H, W, OC, OH, OW;
  int tiles_i, tiles_j, ksl, kt_per;
  unsigned g_bytes, x_bytes;
};
static_assert(sizeof(bconv_fb_args_t) == 104 && __builtin_offsetof(bconv_fb_args_t, ws) == 32 && __builtin_offsetof(bconv_fb_args_t, B) == 48 && __builtin_offsetof(bconv_fb_args_t, g_bytes) == 92, "bconv_fb_args_t layout");

// kernels/bck_ops_f32.hip
struct bck_ops_args_t {
  float const *p0; float const *p1; float const *p2; float const *p3;   // inputs, in the function's arg order
  float *o0; float *o1;                                                 // outputs, in the function's arg order
  long n;                                                               // threads that have work
  int B, C, HW, n4;                                                     // images, channels, pels of a plane; OP 5: float4 quads
  float f0, f1, f2, f3;                                                 // LRN: alpha / local_size, beta, k, ((2 * -beta) * alpha) / local_size; OP 10: f0 = scale
  float const *p4; float const *p5; float const *p6; float const *p7;   // OP 9: inputs 4 .. 7; OP 10 with SEEDVAR: p4 = the uint32 word added to seed
  unsigned seed, thresh;                                                // OP 10
  int run, wide, off;                                                   // OP 11, 12: floats of one image's channel range, of one image of the wider tensor, offset of the range; OP 14: wide = the slab stride, B = the slabs
};
static_assert(sizeof(bck_ops_args_t) == 144 && __builtin_offsetof(bck_ops_args_t, n) == 48 && __builtin_offsetof(bck_ops_args_t, B) == 56 && __builtin_offsetof(bck_ops_args_t, f0) == 72 &&
              __builtin_offsetof(bck_ops_args_t, p4) == 88 && __builtin_offsetof(bck_ops_args_t, seed) == 120 && __builtin_offsetof(bck_ops_args_t, run) == 128, "bck_ops_args_t layout");

// kernels/sgd_update_f32.hip: the table of up to kSgdMaxTens tensors rides by value in the kernel arguments
constexpr int kSgdMaxTens = 32;
struct sgd_tensor_t {
  float *w; float const *g; float *h;
  unsigned n, blk0;                      // elements; index of the tensor's first workgroup
  float lr_mult, decay_mult;
  unsigned quads, pad;                   // 1: w, g and h are 16-byte aligned
};
struct sgd_update_args_t {
  float const *hyper;                    // lr, momentum, weight_decay, unused
  unsigned tens_num, pad;
  sgd_tensor_t t[kSgdMaxTens];
};
static_assert(sizeof(sgd_tensor_t) == 48 && sizeof(sgd_update_args_t) == 16 + 48 * kSgdMaxTens && __builtin_offsetof(sgd_tensor_t, n) == 24 && __builtin_offsetof(sgd_tensor_t, lr_mult) == 32 &&
              __builtin_offsetof(sgd_tensor_t, quads) == 40 && __builtin_offsetof(sgd_update_args_t, tens_num) == 8 && __builtin_offsetof(sgd_update_args_t, t) == 16, "sgd_tensor_t / sgd_update_args_t layout");

// kernels/solver_update_f32.hip: the tables of up to kSgdMaxTens tensors ride by value in the kernel arguments
struct solver_tensor_t {
  float *w; float const *g; float *h; float *h2;   // h2: adam's second history (null otherwise)
  unsigned n, blk0;                      // elements; index of the tensor's first workgroup
  float lr_mult, decay_mult;
  unsigned quads, pad;                   // 1: w, g, h (and h2) are 16-byte aligned
};
struct solver_update_args_t {
  float const *hyper;                    // lr, momentum, weight_decay, momentum2, delta, corr, clip_gradients, unused
  float const *state;                    // coef, norm, sumsq, 0: read with CLIP=1 only
  unsigned tens_num, pad;
  solver_tensor_t t[kSgdMaxTens];
};
static_assert(sizeof(solver_tensor_t) == 56 && sizeof(solver_update_args_t) == 24 + 56 * kSgdMaxTens && __builtin_offsetof(solver_tensor_t, h2) == 24 && __builtin_offsetof(solver_tensor_t, n) == 32 &&
              __builtin_offsetof(solver_tensor_t, lr_mult) == 40 && __builtin_offsetof(solver_tensor_t, quads) == 48 && __builtin_offsetof(solver_update_args_t, state) == 8 &&
              __builtin_offsetof(solver_update_args_t, tens_num) == 16 && __builtin_offsetof(solver_update_args_t, t) == 24, "solver_tensor_t / solver_update_args_t layout");
struct sumsq_tensor_t { float const *g; unsigned n, blk0; };
struct grad_sumsq_args_t {
  float *partials;                       // the workgroup of chunk k writes partials[part0 + k]
  unsigned tens_num, part0;
  sumsq_tensor_t t[kSgdMaxTens];
};
static_assert(sizeof(sumsq_tensor_t) == 16 && sizeof(grad_sumsq_args_t) == 16 + 16 * kSgdMaxTens && __builtin_offsetof(sumsq_tensor_t, n) == 8 && __builtin_offsetof(grad_sumsq_args_t, tens_num) == 8 &&
              __builtin_offsetof(grad_sumsq_args_t, part0) == 12 && __builtin_offsetof(grad_sumsq_args_t, t) == 16, "sumsq_tensor_t / grad_sumsq_args_t layout");
struct grad_norm_args_t {
  float const *partials; float const *hyper; float *state;
  unsigned n_parts, pad;
};
static_assert(sizeof(grad_norm_args_t) == 32 && __builtin_offsetof(grad_norm_args_t, state) == 16 && __builtin_offsetof(grad_norm_args_t, n_parts) == 24, "grad_norm_args_t layout");
// gradient accumulation (OP 4 and the -DACCUM=1 form of OP 1): accum = [first, apply, scale, micro] in device memory
struct accum_tensor_t {
  float const *g; float *a;              // the micro-step's gradient (read), the accumulator (written; read unless accum[0] != 0)
  unsigned n, blk0;                      // elements; index of the tensor's first workgroup
  unsigned quads, pad;                   // 1: g and a are 16-byte aligned
};
struct grad_accum_args_t {
  float const *accum;
  unsigned tens_num, pad;
  accum_tensor_t t[kSgdMaxTens];
};
static_assert(sizeof(accum_tensor_t) == 32 && sizeof(grad_accum_args_t) == 16 + 32 * kSgdMaxTens && __builtin_offsetof(accum_tensor_t, a) == 8 && __builtin_offsetof(accum_tensor_t, n) == 16 &&
              __builtin_offsetof(accum_tensor_t, quads) == 24 && __builtin_offsetof(grad_accum_args_t, tens_num) == 8 && __builtin_offsetof(grad_accum_args_t, t) == 16, "accum_tensor_t / grad_accum_args_t layout");
struct solver_update_acc_args_t {
  float const *hyper;                    // as solver_update_args_t's
  float const *state;
  float const *accum;                    // accum[1] == 0: the launch writes nothing; accum[2]: the factor on the (clipped) summed gradient
  unsigned tens_num, pad;
  solver_tensor_t t[kSgdMaxTens];        // g: the accumulator
};
static_assert(sizeof(solver_update_acc_args_t) == 32 + 56 * kSgdMaxTens && __builtin_offsetof(solver_update_acc_args_t, state) == 8 && __builtin_offsetof(solver_update_acc_args_t, accum) == 16 &&
              __builtin_offsetof(solver_update_acc_args_t, tens_num) == 24 && __builtin_offsetof(solver_update_acc_args_t, t) == 32, "solver_update_acc_args_t layout");

// kernels/bn_f32.hip: the training BatchNorm functions and hip_fan_out
struct bn_args_t {
  float const *in; float const *dy;                                   // the tensors read
  float const *c0; float const *c1; float const *c2; float const *c3; float const *c4;   // per-channel values read, in the function's arg order
  float *out;                                                         // the tensor written (OP 3: out, OP 4: in_grad_loss)
  float *w0; float *w1; float *w2; float *w3;                         // per-channel values written, in the function's arg order
  float *ws;                                                          // slab partials: [2][C][nslabs]
  float *outs[8];                                                     // OP 5
  long n;                                                             // OP 3 .. 5: threads that have work
  int B, C, HW, N;                                                    // images, channels, pels of a plane, B * HW
  int slab, nslabs;                                                   // OP 1, 2
  int quads;                                                          // OP 1: 1 = 16-byte loads; OP 3 .. 5: float4 quads of one plane (OP 5: of the tensor), 0 = none
  int step_img, step_pel;                                             // OP 1: 1024 / HW, 1024 % HW -- from one quad of a chain to its next
  float fN, eps, maf, omm, unb;
};
static_assert(sizeof(bn_args_t) == 13 * 8 + 8 * 8 + 8 + 9 * 4 + 5 * 4 && __builtin_offsetof(bn_args_t, outs) == 104 && __builtin_offsetof(bn_args_t, n) == 168 && __builtin_offsetof(bn_args_t, B) == 176 &&
              __builtin_offsetof(bn_args_t, fN) == 212, "bn_args_t layout");

// kernels/eval_f32.hip: the evaluation pass of the gradient pipe
struct accuracy_args_t {
  float const *in; float const *label;   // logits img:chan:1:1, labels img:1:1
  unsigned *rank;                        // one word per image
  int B, C;
};
static_assert(sizeof(accuracy_args_t) == 32 && __builtin_offsetof(accuracy_args_t, rank) == 16 && __builtin_offsetof(accuracy_args_t, B) == 24, "accuracy_args_t layout");
struct eval_accum_args_t {
  unsigned const *rank; float const *loss;
  unsigned const *ctl;                   // ctl[0] != 0: counts and loss_sum are overwritten and not read
  unsigned *counts; float *loss_sum;     // images, hits_top1, hits_topk, batches; the sum of the batches' losses
  int B; unsigned top_k;
};
static_assert(sizeof(eval_accum_args_t) == 48 && __builtin_offsetof(eval_accum_args_t, counts) == 24 && __builtin_offsetof(eval_accum_args_t, B) == 40, "eval_accum_args_t layout");
struct bn_fold_args_t {
  float const *run_mean; float const *run_var; float const *scale; float const *bias;
  float *a; float *b;
  int C; float eps;
};
static_assert(sizeof(bn_fold_args_t) == 56 && __builtin_offsetof(bn_fold_args_t, a) == 32 && __builtin_offsetof(bn_fold_args_t, C) == 48, "bn_fold_args_t layout");

// kernels/data_f32.hip: the input transform of the gradient pipe
struct data_transform_args_t {
  unsigned char const *src;              // img:y:x:chan or img:chan:y:x (-DCHW) at the source size H x W
  unsigned const *plan;                  // img:v=4 = y_off, x_off, mirror, unused
  float const *mean;                     // chan, or chan:y:x at the source size (-DMEAN_PEL)
  float *out;                            // img:chan:y:x at the crop size ch x cw
  long n;                                // out's elements, B * C * ch * cw
  int C, H, W, ch, cw;
  float scale;
};
static_assert(sizeof(data_transform_args_t) == 64 && __builtin_offsetof(data_transform_args_t, out) == 24 && __builtin_offsetof(data_transform_args_t, n) == 32 &&
              __builtin_offsetof(data_transform_args_t, C) == 40 && __builtin_offsetof(data_transform_args_t, scale) == 60, "data_transform_args_t layout");

// kernels/loss_f32.hip: the full SoftmaxWithLoss of the gradient pipe (loss_weight, ignore_label, planes, the four normalisers)
struct softmax_loss_fwd_args_t {
  float const *in; float const *label;   // logits img:chan:y:x, labels img:y:x
  float *prob; float *loss_per_pel;      // img:chan:y:x, img:y:x
  int B, C, HW;                          // images, channels, pels of a plane
  int has_ignore; float ignore;          // a label equal to `ignore` is ignored (has_ignore != 0)
  int pad_;
};
static_assert(sizeof(softmax_loss_fwd_args_t) == 56 && __builtin_offsetof(softmax_loss_fwd_args_t, prob) == 16 && __builtin_offsetof(softmax_loss_fwd_args_t, B) == 32 &&
              __builtin_offsetof(softmax_loss_fwd_args_t, ignore) == 48, "softmax_loss_fwd_args_t layout");
struct loss_norm_args_t {
  float const *label; float const *loss_per_pel;   // img:y:x both
  float *loss; float *state;             // y=1:x=1; v=4 = Z, s, count, the sum of loss_per_pel
  int N, B;                              // pels of the batch (B * HW, below 2^24), images
  int has_ignore; float ignore;
  float weight; int norm;                // norm: 0 valid | 1 full | 2 batch_size | 3 none
};
static_assert(sizeof(loss_norm_args_t) == 56 && __builtin_offsetof(loss_norm_args_t, loss) == 16 && __builtin_offsetof(loss_norm_args_t, N) == 32 &&
              __builtin_offsetof(loss_norm_args_t, weight) == 48, "loss_norm_args_t layout");
struct softmax_loss_bck_args_t {
  float const *prob; float const *label; float const *state;   // state[1] = s is read on the device
  float *grad;                           // in_grad_loss img:chan:y:x
  long n;                                // grad's elements, B * C * HW
  int C, HW;
  int has_ignore; float ignore;
};
static_assert(sizeof(softmax_loss_bck_args_t) == 56 && __builtin_offsetof(softmax_loss_bck_args_t, grad) == 24 && __builtin_offsetof(softmax_loss_bck_args_t, n) == 32 &&
              __builtin_offsetof(softmax_loss_bck_args_t, C) == 40 && __builtin_offsetof(softmax_loss_bck_args_t, ignore) == 52, "softmax_loss_bck_args_t layout");

// kernels/conv_grp_f32.hip: a grouped convolution and its data / filter gradients (hip_conv_grp, hip_bconv_in_grp, hip_bconv_filts_grp)
struct conv_grp_args_t {
  float const *a; float const *b; float const *bias; float *d;   // forward: a = filts, b = in, bias = biases, d = out; data gradient: a = filts, b = out_grad_loss,
                                                                 // d = in_grad_loss; filter gradient: a = out_grad_loss, b = in, d = filts_grad_loss
  int B, C, H, W, OC, OH, OW;   // the WHOLE tensors' channels: the image strides; a group's share is the kernel's -DCG / -DOCG
  int kt_per;                   // filter gradient: K steps per slice
  long n;                       // threads that have work
  unsigned a_bytes, b_bytes, d_bytes, ksl;   // ksl: the direct filter gradient's slab sum: slabs to add
  float *ws;                    // the direct filter gradient with K slices: the call's slabs, [slice][filts_grad_loss's elements]
};
static_assert(sizeof(conv_grp_args_t) == 96 && __builtin_offsetof(conv_grp_args_t, B) == 32 && __builtin_offsetof(conv_grp_args_t, n) == 64 &&
              __builtin_offsetof(conv_grp_args_t, a_bytes) == 72 && __builtin_offsetof(conv_grp_args_t, ws) == 88, "conv_grp_args_t layout");

// kernels/deconv_f32.hip: a Deconvolution and its data / filter gradients (hip_deconv, hip_deconv_bck_in, hip_deconv_bck_filts); channels and kernel are -D constants
struct deconv_args_t {
  float const *a; float const *b; float const *bias; float *d;   // forward: a = filts, b = in, bias = biases, d = out; data gradient: a = filts, b = out_grad_loss,
                                                                 // d = in_grad_loss; filter gradient: a = out_grad_loss, b = in, d = filts_grad_loss
  int B, H, W, OH, OW;          // images, the small map, the large map
  int kt_per;                   // filter gradient: K steps per slice
  int zs, per;                  // forward: chunks of a row phase's work, items (img, row, quad of x) per chunk
  long n;                       // data gradient: outputs; filter gradient and its slab sum: elements of filts_grad_loss
  unsigned a_bytes, b_bytes, d_bytes, ksl;   // ksl: the slab sum: slabs to add
  float *ws;                    // the filter gradient with K slices: the call's slabs, [slice][filts_grad_loss's elements]
};
static_assert(sizeof(deconv_args_t) == 96 && __builtin_offsetof(deconv_args_t, B) == 32 && __builtin_offsetof(deconv_args_t, n) == 64 &&
              __builtin_offsetof(deconv_args_t, a_bytes) == 72 && __builtin_offsetof(deconv_args_t, ws) == 88, "deconv_args_t layout");

#pragma pop_macro("CH")
#pragma pop_macro("CIN")
#pragma pop_macro("COH")
#pragma pop_macro("COW")
#pragma pop_macro("CW")
#pragma pop_macro("H")
#pragma pop_macro("HW")
#pragma pop_macro("KH")
#pragma pop_macro("KW")
#pragma pop_macro("OH")
#pragma pop_macro("OW")
#pragma pop_macro("PX")
#pragma pop_macro("PY")
#pragma pop_macro("SX")
#pragma pop_macro("SY")
#pragma pop_macro("W")
#endif // BODAHIP_KERNEL_ARGS_H
