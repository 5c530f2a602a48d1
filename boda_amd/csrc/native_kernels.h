// native_kernels.h -- the native side door of the hip backend: hand-written MFMA kernels bound by op func_name.
//
// Precedent in the reference: nvrtc_compute_t::run() routes functions whose op.func_name starts with cublas_ / cudnn_
// to a vendor library (src/nvrtc_util.cc:369-372, src/culibs-wrap.cc:66-247) while every tensor stays in reference
// layout (src/cnn_op.cc:47-48,142,339-340).  This backend does the same for the functions of native_funcs.h: that table lists every name with its op types, its args in
// call order, the op flags it takes, the backends that run it and what a multi-device backend does with it.  What the table cannot say:
//     hip_sgemm / hip_conv (aliases cublas_sgemm / cudnn_conv) keep the contracts of test/rtc/cublas_sgemm.cucl:1-4 and cudnn_conv.cucl:1-7; hip_sgemm_bf16 / hip_conv_bf16
//                                       take bf16 operands (converted while staging) and accumulate in fp32 (config 5); hip_conv_winograd runs 3x3 / stride-1 layers through
//                                       F(2x2,3x3) Winograd (mrd <= ~2e-3)
//     hip_conv_nhwc                     Convolution on channels-last bf16 tensors (filts out_chan:y:x:in_chan, in / out img:y:x:chan, type bfloat16;
//                                       out may be float): the layout the bf16 matrix cores want -- reached through xpose functions like the
//                                       reference's k1conv / tconv (src/rtc_prof.cc:92-121)
//     hip_conv_nhwc_grp                 up to four hip_conv_nhwc that read the same `in` with the same kernel geometry, as ONE launch (stacked filts / biases, outputs
//                                       out_0 .. out_3): an inception module's same-input 1x1 convs, a ResNet stage's branch1 + branch2a
//     hip_conv_nhwc_multi               up to 256 INDEPENDENT hip_conv_nhwc convolutions (own tensors, any geometries) as ONE launch: the tile lists of a per-layer op list's
//                                       small members handed to the hardware dispatcher together, longest first (kernels/conv_nhwc_multi_bf16.hip)
//     hip_conv_nhwc_set                 up to 16 independent hip_conv_nhwc convolutions, each on ITS OWN specialised kernel code, as one launch: an inception module's
//                                       3x3 / 5x5 / pool-projection convolutions (the kernel sources instantiated per member inside one wrapper kernel, built at run time)
//     the non-conv ops of the gradient pipe (fp32, img:chan:y:x; kernels/bck_ops_f32.hip) take their reference templates' arg lists (test/rtc/pool.cucl with
//                                       emit_out_in_yx=1, lrn.cucl with emit_out_scale_base=1, spreading.cucl, bck_lrn.cucl, ZeroIfNonPos.cucl, softmax.cucl, sm_grad_and_loss.cucl,
//                                       sum_loss_over_imgs.cucl, reduce.cucl, dropout.cucl; hip_concat / hip_split: src/rtc_fwd.cc:267-294, one call per input / output, ocix / icix
//                                       in the op); the templates' by-value scalars (avg_pool, emit_*, alpha, beta, k, local_size) ride in the op.  hip_dropout with seed_from_var=1:
//                                       the hash seed is the word of det_drop_seed_var + the by-value det_drop_seed.  hip_sm_grad_and_loss with img_shards=1 reads an optional
//                                       by-value uint32 img_total of the call: the divisor.  hip_chan_affine: out = in * a[chan] + b[chan], two roundings (relu in the op; in and
//                                       out may be one var): the forward pipe's BatchNorm / Scale runs
//     hip_sgd_update                    this backend's own (the reference has no solver): n = tens_num and the floats lr_mult_i / decay_mult_i in the op; hyper is float v=4: lr,
//                                       momentum, weight_decay, unused.  g1 = g + (wd * decay_mult_i) * w; h' = momentum * h + (lr * lr_mult_i) * g1; w' = w - h', every
//                                       operation one fp32 rounding.  One launch for all tensors (kernels/sgd_update_f32.hip); the code object is built when the function is compiled
//     hip_solver_update / hip_grad_sumsq / hip_grad_norm    this backend's own: SGD, Nesterov and Adam over up to 32 tensors per launch (str_val solver_type; hyper float v=8),
//                                       and global-norm clipping as a sum of squares per chunk, one finishing launch and the coefficient in `state` (float v=4), which the
//                                       update reads with clip=1.  kernels/solver_update_f32.hip states the chains and the tree; code objects built when the function is compiled
//     hip_grad_accum / hip_solver_update_acc    this backend's own: gradient accumulation over iter_size micro-steps.  accum (float v=4 = first, apply, scale, micro) is read
//                                       from device memory: a_i = first ? g_i : a_i + g_i; the update applies only where apply != 0, on scale * the (clipped) summed gradient
//     hip_accuracy / hip_eval_accum / hip_bn_fold    this backend's own: the evaluation pass of the gradient pipe.  The rank of the true class per image (uint32; the logits, not
//                                       prob), the batch's image / hit / batch counts and loss added into counts (uint32 v=4) and loss_sum under ctl = [first, 0, 0, 0] read
//                                       from device memory, and a [BatchNorm, Scale] run's running statistics folded into (a, b) for hip_chan_affine.  kernels/eval_f32.hip
//     hip_data_transform               this backend's own: the input transform of the gradient pipe.  uint8 images (interleaved or planar) cropped and mirrored under a
//                                       per-image plan var (uint32 img:v=4 = y_off, x_off, mirror, unused; offsets clamped), mean (per channel or per source pel)
//                                       subtracted, scaled: out = ((float)src - mean) * scale, two fp32 roundings.  kernels/data_f32.hip
//     hip_softmax_loss_fwd / hip_loss_norm / hip_softmax_loss_bck    this backend's own: the full SoftmaxWithLoss of a head with a LossSpec (loss_weight, ignore_label,
//                                       planes, the four normalisers).  prob under the true maximum and loss_per_pel; the count of the pels that are not ignored, the
//                                       normaliser Z, s = weight / Z and the loss into loss / loss_state; the gradient under s read from loss_state.  kernels/loss_f32.hip
//     hip_bn_stats / hip_bn_fwd / hip_bn_bck_sums / hip_bn_bck_in / hip_fan_out    this backend's own: the training BatchNorm of the gradient pipe (batch statistics, running
//                                       pair, normalise + scale + bias + ReLU, the two gradients) and the gradient of an Eltwise SUM.  kernels/bn_f32.hip states the arithmetic and
//                                       the order of the per-channel sums
// and lands them on kernels/gemm_conv_f32.hip (and, for short-K 1x1 convs with a long pel axis, kernels/k1_stream_f32.hip),
// specialised with hiprtc per shape class at first use.
#pragma once
#include "rtc_types.h"
#include <hip/hip_runtime.h>

namespace bodahip {

void hip_err_chk(hipError_t e, char const *what);
struct kernel_text_t { char const *name; char const *text; };   // an embedded kernels/<name>.hip or kernels/<name> header (kernels_embed.inc)
// `headers`: what `src` may #include by name (in-memory; their texts are part of the cache key like src itself)
std::vector<char> hiprtc_compile(string const &src, string const &name, string const &arch, vect_string const &opts, string *log_out, bool use_cache,
                                 std::vector<kernel_text_t> const &headers = std::vector<kernel_text_t>());
kernel_text_t const *find_kernel_source(string const &name);    // by its name in build.py's KERNELS; nullptr: none
std::vector<kernel_text_t> const &kernel_headers();             // what every kernels/*.hip includes: kernels/kernel_args.h, kernels/device_prelude.h
void hiprtc_compile_stats(uint64_t *hits, uint64_t *misses, double *compile_ms);   // process-wide: code objects from the on-disk cache / compiled, time spent compiling
string cucl_prelude();
string default_cache_dir();

// what the native kernels need from their backend
struct native_host_t {
  virtual ~native_host_t() {}
  virtual hipStream_t nh_stream() = 0;
  // launch a kernel of the current call on the backend's stream (grid gx x gy workgroups of `block` threads).  The backend decides how the call is TIMED: with marker
  // events around the call, or -- timing mode "kernel" -- with start / stop events bound to the call's own dispatches (hipExtModuleLaunchKernel)
  virtual hipError_t nh_launch(hipFunction_t f, uint32_t gx, uint32_t gy, uint32_t block, void **params) = 0;
  virtual bool nh_capturing() = 0; // stream capture (hipGraph) in progress: nothing may be compiled / allocated / synchronised
  virtual int nh_live_graphs() = 0; // captured graphs not yet destroyed (their kernel arguments may point into the kernel scratch)
  virtual string const &nh_arch() = 0;
  virtual int nh_num_cus() = 0;
  virtual int nh_device() = 0;      // HIP device ordinal this backend runs on
  virtual void *nh_var_ptr(string const &vn) = 0;
  virtual dims_t nh_var_dims(string const &vn) = 0;
  virtual rtc_compute_t &nh_rtc() = 0;
};

// blocking of one specialisation (the op_tune_t analogue for the native kernels: MNb/MNt/Kb of src/cnn_op.H:18-20
// become workgroup tile / waves / K step)
struct tile_cfg_t {
  int BI = 128, BJ = 128, BK = 16, WI = 2, WJ = 2, MINW = 2, SPLITK = 1, MT = 32, PF = 1, SW = 0;   // SW: 1 = as many staging waves as multiplying waves (gemm_conv_f32.hip -DSPECW)
  int KHO = 0;   // > 1: sequential K hand-off in KHO segments per tile (gemm_conv_f32.hip -DKHO=1: exact, persistent workgroups pulling (tile, segment) jobs)
  int threads() const { return (SW == 2 || SW == 3) ? (WI * WJ * 64 + 256) : (WI * WJ * 64 * (SW ? 2 : 1)); }   // SW 2: kernels/conv_big_f32.hip -- WI x WJ multiplying waves + four staging waves; 3: kernels/sgemm_big_f32.hip likewise
  string str() const {
    return std::to_string(BI) + "x" + std::to_string(BJ) + "x" + std::to_string(BK) + "_w" + std::to_string(WI) + "x" + std::to_string(WJ) +
           (MT != 32 ? ("_m" + std::to_string(MT)) : string()) + (SPLITK > 1 ? ("_s" + std::to_string(SPLITK)) : string()) + (PF != 1 ? ("_p" + std::to_string(PF)) : string()) + (SW == 2 ? "_big" : (SW == 3 ? "_stg" : (SW ? "_sw" : ""))) + (KHO > 1 ? ("_h" + std::to_string(KHO)) : string()); }
};

struct conv_geom_t { int B, C, H, W, OC, KH, KW, SY, SX, PY, PX, OH, OW; bool relu;
  // round 5, fp32 hip_conv only: a max pooling fused in FRONT of the convolution (kernels/gemm_conv_f32.hip, PKH).  H x W are then the POOLED plane -- the convolution's
  // input --, UH x UW the planes of the tensor actually read (the pooling's input); PKH == PKW == 1: no pooling (UH / UW unused).
  int PKH = 1, PKW = 1, PSY = 1, PSX = 1, UH = 0, UW = 0;
  bool pooled() const { return PKH * PKW > 1; } };

// channels-last bf16, rolling-rows kernel (kernels/conv_nhwc_rows_bf16.hip): what follows the convolution INSIDE the launch -- a max pooling of its output (PKH > 0:
// window, stride, padding; POH x POW = the pooled planes, the tensor the launch writes) and an across-channel LRN of the pooled values (LRN_N > 0: local size, alpha, beta, k)
struct post_ops_t { int PKH = 0, PKW = 0, PSY = 1, PSX = 1, PPY = 0, PPX = 0, POH = 0, POW = 0, LRN_N = 0; float alpha = 0.f, beta = 0.f, k = 0.f; bool pooled() const { return PKH > 0; } };

// one call of a non-conv gradient-pipe kernel (kernels/bck_ops_f32.hip): op = 1 pool_yx, 2 spreading, 3 lrn_sb, 4 bck_lrn, 5 zero_if_non_pos, 6 softmax, 7 sm_grad_and_loss,
// 8 sum_loss_over_imgs, 9 reduce, 10 dropout, 11 concat, 12 split, 13 chan_affine (the forward pipe's; relu from the op).  B images of C channels; H x W = the pooling's INPUT plane (LRN: the plane), OH x OW its output
// plane; n = elements (zero_if_non_pos, reduce, dropout).  reduce: nin inputs.  dropout: ratio from the op, seed from the
// call.  concat / split: B images of the narrow tensor's C channels (planes H x W) at channels [cix, cix + C) of the wide tensor's CT
struct bck_op_geom_t { int op = 0; long B = 0; int C = 0, H = 1, W = 1, OH = 1, OW = 1, KH = 1, KW = 1, SY = 1, SX = 1, PY = 0, PX = 0, avg = 0, LS = 1; float alpha = 0.f, beta = 0.f, k = 0.f; long n = 0;
  int nin = 0; float ratio = 0.f; uint32_t seed = 0; int CT = 0, cix = 0;
  int zinp = 0;      // spreading, bck_lrn: 1 = in_grad_loss = in > 0 ? value : +0 (the op's zero_if_in_non_pos; spreading then takes `in` as its fourth input)
  int seedvar = 0;   // dropout: 1 = the hash seed is the word of the call's det_drop_seed_var + seed (the op's seed_from_var)
  long img_total = 0;   // sm_grad_and_loss on an img shard (the op's img_shards=1): the image count of the WHOLE batch, the divisor (0: B)
  int relu = 0; };   // chan_affine: 1 = x > 0 ? x : +0 on the finished sum (the op's relu)

struct launch_info_t { string kernel; tile_cfg_t cfg; uint32_t grid = 0, block = 0; double flops = 0, algo_bytes = 0; };

struct native_kernels_t {
  explicit native_kernels_t(native_host_t *host_);
  ~native_kernels_t();
  static bool is_native_func_name(string const &fn);
  native_func_t const *check_compile_time(rtc_func_info_t const &fi);   // -> the function's row of native_funcs.h: looked up once, kept with the compiled function
  void run(native_func_t const &f, rtc_func_info_t const &fi, map_str_rtc_arg_t const &arg_map);

  // direct entry points on raw device pointers (used by run() and by the C ABI's fast paths)
  void sgemm(float const *a, float const *b, float *c, uint32_t M, uint32_t N, uint32_t K, bool bf16 = false, bool half = false);   // half: 2-byte IEEE half elements, fp32 math
  void conv(float const *filts, float const *biases, float const *in, float *out, conv_geom_t const &g, bool bf16 = false, int out_ctot = 0, int out_coff = 0,
            char const *algo = nullptr, float const *filts_km = nullptr);   // filts_km: the caller's k-major copy of filts (hip_conv_filts_kmajor), or null

  // channels-last bf16 tensors (kernels/conv_nhwc_bf16.hip): filts out_chan:y:x:in_chan, in / out img:y:x:chan; g.C = stored channels (multiple of 8)
  void conv_nhwc_rows(void const *filts, float const *biases, void const *in, void *out, conv_geom_t const &g, post_ops_t const &post, int out_ctot = 0, int out_coff = 0);   // F' filts; g.OH x g.OW = the convolution's own output planes
  void conv_nhwc(void const *filts, float const *biases, void const *in, void *out, conv_geom_t const &g, bool out_f32, int out_ctot = 0, int out_coff = 0, bool patch_filts = false, bool pool = false, void const *res = nullptr);   // res: the function op's nhwc_residual=1 -- a tensor of out's dims and type added in the epilogue before the one rounding (-DRES=1; implicit-GEMM kernel only); pool: g.KH x g.KW / g.PY, g.PX are a max-pooling window fused in front of 1x1 filters (patch form); patch_filts: filts are F'[in_grp][ky][kx][out_chan][8] -> the LDS input-patch kernel
  // horizontally fused channels-last convolutions (same `in`, same kernel geometry; filts / biases stacked along out_chan, members padded to `pad` rows)
  void conv_nhwc_grp(void const *filts, float const *biases, void const *in, conv_geom_t const &g, bool out_f32, int n, int const *noc, void *const *outs,
                     int const *ctot, int const *coff, int pad);
  // several independent channels-last convolutions as ONE launch (kernels/conv_nhwc_multi_bf16.hip); members: raw device pointers + geometry (g.C = stored channels)
  struct multi_member_t { void const *filts; float const *biases; void const *in; void *out; conv_geom_t g; int out_ctot, out_coff; bool pool = false;
                          // a horizontally fused member (hip_conv_nhwc_grp as a member of a set): filts / biases stacked, g.OC = the padded total, `out` unused
                          int grp_n = 0; int grp_noc[4] = {0, 0, 0, 0}; void *grp_out[4] = {nullptr, nullptr, nullptr, nullptr}; int grp_ctot[4] = {0, 0, 0, 0}, grp_coff[4] = {0, 0, 0, 0}; int grp_pad = 0; };   // pool: g's window / padding are a max pooling fused in front of 1x1 filters
  void conv_nhwc_multi(int n, multi_member_t const *members, bool out_f32);
  // a few independent channels-last convolutions, each on its own specialised kernel code (implicit-GEMM or input-patch form), as one launch (wrapper kernel built at run time)
  void conv_nhwc_set(int n, multi_member_t const *members, bool const *patch_filts, bool out_f32);
  // two 1x1 / stride-1 / unpadded fp32 convolutions back to back as one launch, the intermediate tensor in registers (kernels/k1_quad_f32.hip -DCHAIN=1); g = the first
  // convolution's geometry, mid (optional) also receives its output
  void conv_k1_chain(float const *filts, float const *biases, float const *filts2, float const *biases2, float const *in, float *out, float *mid, conv_geom_t const &g, int oc2,
                     bool relu2, int out_ctot, int out_coff);
  // BckConv gradients (fp32, reference layouts; g = the forward convolution's geometry, out_grad_loss has g.OH x g.OW planes): kernels/bconv_in_f32.hip (data gradient,
  // bit-identical to the reference's chain), kernels/bconv_filts_f32.hip (filter gradient with deterministic in-launch K slices; bias gradient)
  // zin (the op's zero_if_in_non_pos=1): the forward input; in_grad = zin > 0 ? gradient : +0
  void bconv_in(float const *filts, float const *out_grad, float *in_grad, conv_geom_t const &g, float const *zin = nullptr, bool bf16 = false);   // bf16 (the op's hip_operands=bf16): kernels/bconv_in_bf16.hip
  void bconv_filts(float const *in, float const *out_grad, float *filts_grad, conv_geom_t const &g);
  void bconv_biases(float const *out_grad, float *biases_grad, conv_geom_t const &g);
  // both at once, k-major staging, up to 1024 K slices in slabs summed by a second launch (kernels/bconv_fb_f32.hip); opt-in: ConvPipeBck(fuse_filts_biases=True)
  void bconv_filts_biases(float const *in, float const *out_grad, float *filts_grad, float *biases_grad, conv_geom_t const &g, bool bf16 = false);   // bf16: kernels/bconv_fb_bf16.hip, the same slabs and slab sum
  // the grouped family (kernels/conv_grp_f32.hip) on raw device pointers.  member kConvGrpFwd: a = filts, b = in, bias = biases, d = out; kConvGrpBckIn: a = filts,
  // b = out_grad_loss, d = in_grad_loss; kConvGrpBckFilts: a = out_grad_loss, b = in, d = filts_grad_loss.  One launch, no workspace
  void conv_grp(int member, conv_grp_geom_t const &g, float const *a, float const *b, float const *bias, float *d);
  // the Deconvolution family (kernels/deconv_f32.hip) on raw device pointers.  member kDeconvFwd: a = filts, b = in, bias = biases, d = out; kDeconvBckIn: a = filts,
  // b = out_grad_loss, d = in_grad_loss; kDeconvBckFilts: a = out_grad_loss, b = in, d = filts_grad_loss (with K slices: slabs in the call's workspace, a second launch)
  void deconv(int member, deconv_geom_t const &g, float const *a, float const *b, float const *bias, float *d);
  // the non-conv ops of the gradient pipe: ins / outs in the function's arg order (up to eight / two raw device pointers)
  // seed_word (dropout with g.seedvar): the device word added to g.seed
  void bck_op(bck_op_geom_t const &g, float const *const *ins, float *const *outs, uint32_t const *seed_word = nullptr);
  // the cross-device sum of a multi-device backend (kernels/bck_ops_f32.hip OP 14): nslabs slabs of n floats at slabs + d * stride (stride in floats) -> out[e] =
  // ((slab_0[e] + slab_1[e]) + slab_2[e]) + ..., plain fp32 adds in slab order starting FROM slab 0; out may be slab 0.  Launched on this backend's stream
  // hip_sgd_update on raw device pointers: n (1 .. 32) tensors of m[i].n floats, hyper = {lr, momentum, weight_decay, unused} in device memory
  struct sgd_member_t { float *w; float const *g; float *h; long n; float lr_mult, decay_mult; };
  void sgd_update(int n, sgd_member_t const *m, float const *hyper);
  // the solver family on raw device pointers (so says which kernel: solver_op_of_op).  solver_update: so.elems.size() tensors, h2 non-null for adam; hyper float[8], state
  // float[4].  grad_sumsq: chunk k of the call writes partials[so.part0 + k].  grad_norm: so.parts partials -> state
  struct solver_member_t { float *w; float const *g; float *h; float *h2; };
  void solver_update(solver_op_t const &so, solver_member_t const *m, float const *hyper, float const *state, float const *accum = nullptr);
  void grad_sumsq(solver_op_t const &so, float const *const *g, float *partials);
  void grad_norm(solver_op_t const &so, float const *partials, float const *hyper, float *state);
  // gradient accumulation: grad_accum: a_i = accum[0] != 0 ? g_i : a_i + g_i; solver_update with so.kind == 5 takes accum (float[4]) as well
  void grad_accum(solver_op_t const &so, float const *const *g, float *const *a, float const *accum);
  // the eval family on raw device pointers (kernels/eval_f32.hip): ptrs in eval_op_t::args' order; e.B of hip_accuracy is the call's image count
  void eval_call(eval_op_t const &e, void *const *ptrs);
  // hip_data_transform on raw device pointers (kernels/data_f32.hip): ptrs = src, plan, mean, out; d.B is the call's image count
  void data_call(data_op_t const &d, void *const *ptrs);
  // the loss family on raw device pointers (kernels/loss_f32.hip): ptrs in loss_op_t::args' order
  void loss_call(loss_op_t const &l, void *const *ptrs);
  void shard_sum(float const *slabs, float *out, int nslabs, long stride, long n);
  // hip_bn_stats / hip_bn_fwd / hip_bn_bck_sums / hip_bn_bck_in / hip_fan_out -- and hip_bnf_prep / hip_bnf_bck / hip_bnf_bck_in, the BatchNorm on its running pair (kFamBnf)
  // -- on raw device pointers (kernels/bn_f32.hip): tens / chans in bn_op_t's arg order
  void bn_call(bn_op_t const &b, float *const *tens, float *const *chans);
  // hip_bnc_stats / hip_bnc_bck_sums with more than one chunk, the chunked chain: the whole call on one device, and its pieces -- the call's workspace (slab partials of
  // one chunk; *tots: the totals [chunk][2][C] behind them), one chunk's totals, the cross-chunk step -- which a multi-device backend runs per device (csrc/hip_multi.cc)
  void bnc_call(bn_op_t const &b, float *const *tens, float *const *chans);
  float *bnc_ws(bn_op_t const &b, void const *key_in, void const *key_chan, float **tots);
  void bnc_chunk(bn_op_t const &cb, int mode, float const *in, float const *dy, float const *c0, float const *c1, float *part, float *tot);
  void bnc_cross(bn_op_t const &b, int fin, float *tots, int live, float *const *chans);
  void conv_winograd(float const *filts, float const *biases, float const *in, float *out, conv_geom_t const &g, int out_ctot, int out_coff);

  // tuning overrides ("" clears): key "sgemm_tile" / "conv_tile" -> "BIxBJxBKxWIxWJ[xMINW[xSPLITK[xMT]]]"; key "k1_stream" -> "off" | "WIxWJxOCBxCB[xMINW]";
  // key "conv_algo" -> "winograd": 3x3 / stride-1 convs go through the F(2x2,3x3) path (kernels/winograd_f32.hip; not bit-exact)
  // key "exact" -> "0": tolerance mode -- fp32 results within the reference's bound for re-associating kernels (mrd < 2e-3, src/rtc_prof.cc:317-319) instead of bit-identical to
  // its fma chain: deterministic K slices on tile-starved long-K layers, Winograd where it is faster.  Default ("" / "1"): bit-exact plans only
  void set_tune(string const &key, string const &val);
  static size_t prebuild(op_base_t const &op, string const &arch, int num_cus, string const &tile, string *plan_out = nullptr);
  launch_info_t last_launch;
  bool last_call_uses_ws = false;   // the last run(): its plan works in the backend's one shared scratch (ensure_ws was called for it)
  uint32_t num_specialisations() const;
  struct impl_t;
  struct call_t;   // one run(): the family handlers (native_run.cc)

 private:
  impl_t *impl;
  native_host_t *host;
};

} // namespace bodahip
