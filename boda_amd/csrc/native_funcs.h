// native_funcs.h -- the one table of the native side door: which function names exist, their family and member, the op types they belong to, their args in call order,
// the op flags they take, which backends run them and what a multi-device backend does with them.  Host-only (nothing of HIP): be=cpu reads it too.  Every other file
// asks this table; boda_amd/cnn_op.py keeps tables of its own (it imports no library) and tests/test_native_funcs_cpu.py holds them to this one.
//
// Row order: the order the refusal messages list the names in (rtc_types.h's flag messages, be=cpu's refusal).  A bare op's calls are its type's rows in ascending
// member: the reference's call order (src/rtc_fwd.cc:384-386 for SoftmaxWithLoss's three, :398-400 for BckConv's in / biases / filts).
#pragma once
#include "rtc_types.h"

namespace bodahip {

// the family (func_family_t of rtc_types.h) selects the handler (native_run.cc, native_kernels.cc: check_compile_time); handlers switch on the member, never on the name
inline constexpr char const *kFamilyNames[] = {"sgemm", "conv", "conv_nhwc", "nhwc_grp", "nhwc_multi", "k1_chain", "filts_kmajor", "bconv", "bck_op", "sgd", "bn", "bnc", "solver", "eval", "data", "bnf", "loss", "conv_grp", "deconv"};
// members.  kFamSolver: 1 update | 2 sumsq | 3 norm | 4 accum | 5 update_acc (solver_op_t::kind).  kFamSgemm: 0 fp32 | 1 bf16 operands.  kFamNhwcMulti: 0 multi | 1 set.  kFamBckOp: the OP number of kernels/bck_ops_f32.hip.  kFamBn, kFamBnc, kFamBnf: the kind of bn_op_t.  kFamEval: 1 accuracy | 2 accum | 3 bn_fold (eval_op_t::kind).  kFamData: 1 transform.  kFamLoss: 1 fwd | 2 norm | 3 bck (loss_op_t::kind).  kFamConvGrp: 1 fwd | 2 bck_in | 3 bck_filts.  kFamDeconv: 1 fwd | 2 bck_in | 3 bck_biases | 4 bck_filts
enum { kConvF32 = 0, kConvAlias = 1, kConvBf16 = 2, kConvWinograd = 3 };            // (the alias: hip_conv's contract without its fused pooling and filts_km)
enum { kBconvIn = 1, kBconvBiases = 2, kBconvFilts = 3, kBconvFiltsBiases = 4 };   // (4 is opt-in: never one of the bare op's three calls)
enum { kConvGrpFwd = 1, kConvGrpBckIn = 2, kConvGrpBckFilts = 3 };                  // (a grouped convolution and its data / filter gradients; the bias gradient knows no groups)
enum { kDeconvFwd = 1, kDeconvBckIn = 2, kDeconvBckBiases = 3, kDeconvBckFilts = 4 };   // (a Deconvolution and its three gradients in BckConv's call order; the bias gradient is hip_bconv_biases' sum under this family's op type)
enum { kOpPoolYx = 1, kOpSpreading = 2, kOpLrnSb = 3, kOpBckLrn = 4, kOpZeroIfNonPos = 5, kOpSoftmax = 6, kOpSmGradAndLoss = 7, kOpSumLossOverImgs = 8, kOpReduce = 9,
       kOpDropout = 10, kOpConcat = 11, kOpSplit = 12, kOpChanAffine = 13, kOpCrop = 15, kOpCropBck = 16 };   // (14 is bodahip_shard_sum, which no function names)

enum arg_kind_t { kIn, kOut, kInOut, kRef, kVal };   // kVal: a by-value scalar of the CALL
inline constexpr char const *kArgKindNames[] = {"IN", "OUT", "INOUT", "REF", "VAL"};
struct func_arg_t { char const *name; arg_kind_t kind; };
// the part of the arg list that depends on the op, as a rule: ins_0 .. ins_{ins_num-1} (IN, 2 to 8) in front of the last fixed arg | outs_0 .. outs_{outs_num-1} (OUT, 2 to 8)
// behind the fixed args | w_i (INOUT) g_i (IN) h_i (INOUT), i < tens_num (1 to 32), in front of the fixed args | member lists, which their handlers describe |
// w_i g_i h_i and, for solver_type=adam, h2_i (INOUT) in front | g_i (IN) in front | g_i (IN) a_i (INOUT) in front.  The last three answer the fixed args alone for an op
// WITHOUT tens_num (the arg-list query of a bare op; compiling such an op stays an error)
enum var_args_t { kVarNone, kVarInsBeforeLast, kVarOutsBehind, kVarWghInFront, kVarMembers, kVarWghH2InFront, kVarGInFront, kVarGaInFront };
// a flag that adds a var arg (IN): which flag, the arg, and where -- at >= 0: in front of fixed arg `at`; at < 0: in front of the last fixed arg.  flag 0: none
struct flag_arg_t { unsigned flag; char const *name; int at; };
enum : unsigned { kBeHip = 1, kBeCpu = 2 };

// what a multi-device backend (hip_multi.cc) does with a call on vars sharded along img.  No default: a row that does not state it does not compile
struct multi_dev_t {
  enum mode_t { on_shards,         // independent per image: runs on every device's shard as it is
                replicated_only,   // runs on every device, and refuses a sharded var
                needs_flag,        // not independent per image: refused (`why`) unless the op carries img_shards=1
                refused,           // refused (`why`) on several devices
                replicated_vars,   // replicated_only's policy: the call runs on every device's replicas, a sharded var is refused
                one_device };      // refused on several devices like `refused`, with the sentence of its FAMILY (why_one_device), which the row does not repeat
  mode_t mode; char const *why;
  constexpr multi_dev_t(mode_t mode_, char const *why_) : mode(mode_), why(why_) {}
};
constexpr multi_dev_t kOnShards{multi_dev_t::on_shards, ""}, kReplicatedOnly{multi_dev_t::replicated_only, ""}, kReplicatedVars{multi_dev_t::replicated_vars, ""};
constexpr multi_dev_t kOneDevice{multi_dev_t::one_device, ""};
constexpr multi_dev_t needs_img_shards_flag(char const *why) { return multi_dev_t(multi_dev_t::needs_flag, why); }
constexpr multi_dev_t refused_on_devices(char const *why) { return multi_dev_t(multi_dev_t::refused, why); }

struct native_func_t {
  char const *name; func_family_t family; int member;
  char const *kname;        // kFamBckOp: the kernel's name
  char const *types[2];     // the op types it is a function of
  func_arg_t args[9];       // the fixed args in call order (null name: end)
  func_arg_t opt_arg;       // one more var arg a call may bind (null name: none)
  var_args_t var;
  unsigned flags;           // the op flags it takes (kFlag* of rtc_types.h)
  flag_arg_t flag_arg;
  unsigned backends;
  multi_dev_t multi_dev;
  bool of_type(string const &t) const { return t == types[0] || (types[1] && t == types[1]); }
  // the vars of a call have the op's dims -- for a function that runs on img shards except the image count, which then only has to agree between the vars.  (All four
  // BckConv gradients read the image count from their vars: the fused one, refused on several devices, has always done so on one)
  bool img_count_free() const { return multi_dev.mode == multi_dev_t::on_shards || multi_dev.mode == multi_dev_t::needs_flag || family == kFamBconv; }
};

#define BODAHIP_CONV_ARGS {"filts", kIn}, {"biases", kIn}, {"in", kIn}, {"stride", kRef}, {"in_pad", kRef}, {"out", kOut}
inline constexpr char kWhyBconvSum[] = "(a BckConv filter / bias gradient) sums over the images, which would need a cross-device reduction; only the data gradient (hip_bconv_in) runs on img shards";
inline constexpr char kWhyBnSums[] = "(a training BatchNorm's per-channel sums) sums over the images of the WHOLE batch, which would need a cross-device reduction; statistics summed across img shards are out of scope";
inline constexpr char kWhyBnfOneDevice[] = "(a BatchNorm on its running pair, the hip_bnf_* family) takes vars of exactly its op's dims, not img shards, and hip_bnf_bck sums over the images of the WHOLE batch, which would need a cross-device reduction; frozen statistics on several devices are out of scope";
inline constexpr char kWhyLossOneDevice[] = "(the full softmax loss, the hip_softmax_loss_* / hip_loss_norm family) counts the pels that are not ignored and sums loss_per_pel over the WHOLE batch, which would need a cross-device reduction, and takes vars of exactly its op's dims, not img shards; a loss with a LossSpec on several devices is out of scope";
inline constexpr char kWhyConvGrpOneDevice[] = "(a grouped convolution, the hip_conv_grp / hip_bconv_in_grp / hip_bconv_filts_grp family) takes vars of exactly its op's dims, not img shards, and hip_bconv_filts_grp sums over the images of the WHOLE batch, which would need a cross-device reduction; grouped layers on several devices are out of scope";
inline constexpr char kWhyDeconvOneDevice[] = "(a Deconvolution, the hip_deconv / hip_deconv_bck_in / hip_deconv_bck_filts / hip_deconv_bck_biases family) takes vars of exactly its op's dims, not img shards, and its filter and bias gradients sum over the images of the WHOLE batch, which would need a cross-device reduction; Deconvolution layers on several devices are out of scope";
inline constexpr char const *why_one_device(func_family_t family) { return family == kFamLoss ? kWhyLossOneDevice : family == kFamConvGrp ? kWhyConvGrpOneDevice : family == kFamDeconv ? kWhyDeconvOneDevice : kWhyBnfOneDevice; }
inline constexpr native_func_t kNativeFuncs[] = {
  // sgemm, a:K:M b:K:N c:M:N (test/rtc/cublas_sgemm.cucl:1-4); Convolution in reference layout (test/rtc/cudnn_conv.cucl:1-7)
  {"hip_sgemm", kFamSgemm, 0, nullptr, {"sgemm"}, {{"a", kIn}, {"b", kIn}, {"c", kOut}}, {}, kVarNone, 0, {}, kBeHip | kBeCpu, kOnShards},
  {"cublas_sgemm", kFamSgemm, 0, nullptr, {"sgemm"}, {{"a", kIn}, {"b", kIn}, {"c", kOut}}, {}, kVarNone, 0, {}, kBeHip | kBeCpu, kOnShards},
  {"cpu_sgemm", kFamSgemm, 0, nullptr, {"sgemm"}, {{"a", kIn}, {"b", kIn}, {"c", kOut}}, {}, kVarNone, 0, {}, kBeCpu, kOnShards},
  {"hip_sgemm_bf16", kFamSgemm, 1, nullptr, {"sgemm"}, {{"a", kIn}, {"b", kIn}, {"c", kOut}}, {}, kVarNone, 0, {}, kBeHip, kOnShards},
  {"hip_conv", kFamConv, kConvF32, nullptr, {"Convolution"}, {BODAHIP_CONV_ARGS}, {"filts_km", kIn}, kVarNone, 0, {}, kBeHip | kBeCpu, kOnShards},
  {"cudnn_conv", kFamConv, kConvAlias, nullptr, {"Convolution"}, {BODAHIP_CONV_ARGS}, {}, kVarNone, 0, {}, kBeHip | kBeCpu, kOnShards},
  {"cpu_conv_fwd", kFamConv, kConvF32, nullptr, {"Convolution"}, {BODAHIP_CONV_ARGS}, {}, kVarNone, 0, {}, kBeCpu, kOnShards},
  {"hip_conv_bf16", kFamConv, kConvBf16, nullptr, {"Convolution"}, {BODAHIP_CONV_ARGS}, {}, kVarNone, 0, {}, kBeHip, kOnShards},
  {"hip_conv_winograd", kFamConv, kConvWinograd, nullptr, {"Convolution"}, {BODAHIP_CONV_ARGS}, {}, kVarNone, 0, {}, kBeHip, kOnShards},
  // channels-last bf16 tensors; the sibling group, the multi-problem launch and the level set take member lists
  {"hip_conv_nhwc", kFamConvNhwc, 0, nullptr, {"Convolution"}, {BODAHIP_CONV_ARGS}, {}, kVarNone, kFlagNhwcResidual, {kFlagNhwcResidual, "res", -1}, kBeHip, kOnShards},
  {"hip_conv_nhwc_grp", kFamNhwcGrp, 0, nullptr, {"Convolution"}, {}, {}, kVarMembers, 0, {}, kBeHip, kOnShards},
  {"hip_conv_nhwc_multi", kFamNhwcMulti, 0, nullptr, {"Convolution"}, {}, {}, kVarMembers, 0, {}, kBeHip, kOnShards},
  {"hip_conv_nhwc_set", kFamNhwcMulti, 1, nullptr, {"Convolution"}, {}, {}, kVarMembers, 0, {}, kBeHip, kOnShards},
  {"hip_conv_k1_chain", kFamK1Chain, 0, nullptr, {"Convolution"}, {{"filts", kIn}, {"biases", kIn}, {"filts2", kIn}, {"biases2", kIn}, {"in", kIn}, {"stride", kRef}, {"in_pad", kRef}, {"out", kOut}}, {}, kVarNone, 0, {}, kBeHip, kOnShards},
  {"hip_conv_filts_kmajor", kFamFiltsKmajor, 0, nullptr, {"Convolution"}, {{"filts", kIn}, {"filts_km", kOut}}, {}, kVarNone, 0, {}, kBeHip, kOnShards},
  // BckConv's gradients: the reference templates' arg lists (test/rtc/BckConv_in_grad_loss.cucl, BckConv_filts_grad_loss.cucl, BckConv_biases_grad_loss.cucl)
  {"hip_bconv_in", kFamBconv, kBconvIn, nullptr, {"BckConv"}, {{"filts", kIn}, {"out_grad_loss", kIn}, {"stride", kRef}, {"in_pad", kRef}, {"in_grad_loss", kOut}}, {}, kVarNone, kFlagZinp, {kFlagZinp, "in", -1}, kBeHip | kBeCpu, kOnShards},
  {"hip_bconv_filts", kFamBconv, kBconvFilts, nullptr, {"BckConv"}, {{"in", kIn}, {"out_grad_loss", kIn}, {"stride", kRef}, {"in_pad", kRef}, {"filts_grad_loss", kOut}}, {}, kVarNone, kFlagImgShards, {}, kBeHip | kBeCpu, needs_img_shards_flag(kWhyBconvSum)},
  {"hip_bconv_biases", kFamBconv, kBconvBiases, nullptr, {"BckConv"}, {{"out_grad_loss", kIn}, {"biases_grad_loss", kOut}}, {}, kVarNone, kFlagImgShards, {}, kBeHip | kBeCpu, needs_img_shards_flag(kWhyBconvSum)},
  {"hip_bconv_filts_biases", kFamBconv, kBconvFiltsBiases, nullptr, {"BckConv"}, {{"in", kIn}, {"out_grad_loss", kIn}, {"stride", kRef}, {"in_pad", kRef}, {"filts_grad_loss", kOut}, {"biases_grad_loss", kOut}}, {}, kVarNone, 0, {}, kBeHip | kBeCpu,
   refused_on_devices("(hip_bconv_filts_biases, a BckConv's fused filter and bias gradient) sums over the images into two outputs, which would need a cross-device reduction of both; on several devices use hip_bconv_filts and hip_bconv_biases with img_shards=1")},
  // the non-conv ops of the gradient pipe (kernels/bck_ops_f32.hip), in their reference templates' arg order (test/rtc/pool.cucl, lrn.cucl, spreading.cucl, bck_lrn.cucl,
  // ZeroIfNonPos.cucl, softmax.cucl, sm_grad_and_loss.cucl, sum_loss_over_imgs.cucl, reduce.cucl, dropout.cucl; the copy calls of src/rtc_fwd.cc:267-294); the templates'
  // by-value scalars ride in the op.  hip_dropout rewrites inout in place (the reference declares it OUT); it is also the function of a BckDropout
  {"hip_pool_yx", kFamBckOp, kOpPoolYx, "bodahip_pool_yx", {"Pooling"}, {{"in", kIn}, {"kern_sz", kRef}, {"stride", kRef}, {"in_pad", kRef}, {"out", kOut}, {"out_in_yx", kOut}}, {}, kVarNone, 0, {}, kBeHip | kBeCpu, kOnShards},
  {"hip_lrn_sb", kFamBckOp, kOpLrnSb, "bodahip_lrn_sb", {"LRN"}, {{"in", kIn}, {"out", kOut}, {"out_scale_base", kOut}}, {}, kVarNone, 0, {}, kBeHip | kBeCpu, kOnShards},
  {"hip_spreading", kFamBckOp, kOpSpreading, "bodahip_spreading", {"Spreading"}, {{"out", kIn}, {"out_grad_loss", kIn}, {"out_in_yx", kIn}, {"kern_sz", kRef}, {"stride", kRef}, {"in_pad", kRef}, {"in_grad_loss", kOut}}, {}, kVarNone, kFlagZinp, {kFlagZinp, "in", -1}, kBeHip | kBeCpu, kOnShards},
  {"hip_bck_lrn", kFamBckOp, kOpBckLrn, "bodahip_bck_lrn", {"BckLRN"}, {{"in", kIn}, {"out", kIn}, {"out_grad_loss", kIn}, {"out_scale_base", kIn}, {"in_grad_loss", kOut}}, {}, kVarNone, kFlagZinp, {}, kBeHip | kBeCpu, kOnShards},   // (reads `in` already)
  {"hip_zero_if_non_pos", kFamBckOp, kOpZeroIfNonPos, "bodahip_zero_if_non_pos", {"ZeroIfNonPos"}, {{"in", kIn}, {"cond", kIn}, {"out", kOut}}, {}, kVarNone, 0, {}, kBeHip | kBeCpu, kOnShards},
  {"hip_softmax", kFamBckOp, kOpSoftmax, "bodahip_softmax", {"SoftmaxWithLoss"}, {{"in", kIn}, {"prob", kOut}}, {}, kVarNone, 0, {}, kBeHip | kBeCpu, kOnShards},
  {"hip_sm_grad_and_loss", kFamBckOp, kOpSmGradAndLoss, "bodahip_sm_grad_and_loss", {"SoftmaxWithLoss"}, {{"prob", kIn}, {"label", kIn}, {"in_grad_loss", kOut}, {"loss_per_pel", kOut}}, {}, kVarNone, kFlagImgShards, {}, kBeHip | kBeCpu,
   needs_img_shards_flag("(the softmax loss gradient) divides by the GLOBAL image count, which an img shard does not know; hip_softmax runs on img shards")},
  {"hip_sum_loss_over_imgs", kFamBckOp, kOpSumLossOverImgs, "bodahip_sum_loss_over_imgs", {"SoftmaxWithLoss"}, {{"loss_per_pel", kIn}, {"loss", kOut}}, {}, kVarNone, kFlagImgShards, {}, kBeHip | kBeCpu,
   needs_img_shards_flag("(the softmax loss) sums loss_per_pel over ALL images, which would need a cross-device reduction; hip_softmax runs on img shards")},
  {"hip_reduce", kFamBckOp, kOpReduce, "bodahip_reduce", {"Reduce"}, {{"out", kOut}}, {}, kVarInsBeforeLast, 0, {}, kBeHip | kBeCpu, kOnShards},
  {"hip_dropout", kFamBckOp, kOpDropout, "bodahip_dropout", {"Dropout", "BckDropout"}, {{"inout", kOut}, {"det_drop_seed", kVal}}, {}, kVarNone, kFlagSeedVar | kFlagImgShards, {kFlagSeedVar, "det_drop_seed_var", 1}, kBeHip | kBeCpu,
   needs_img_shards_flag("(dropout) hashes every element's GLOBAL flat index, which an img shard does not know; hip_reduce / hip_concat / hip_split run on img shards")},
  {"hip_concat", kFamBckOp, kOpConcat, "bodahip_concat", {"Concat"}, {{"in", kIn}, {"out", kOut}}, {}, kVarNone, 0, {}, kBeHip | kBeCpu, kOnShards},
  {"hip_split", kFamBckOp, kOpSplit, "bodahip_split", {"Split"}, {{"in", kIn}, {"out", kOut}}, {}, kVarNone, 0, {}, kBeHip | kBeCpu, kOnShards},
  {"hip_chan_affine", kFamBckOp, kOpChanAffine, "bodahip_chan_affine", {"ChanAffine"}, {{"in", kIn}, {"a", kIn}, {"b", kIn}, {"out", kOut}}, {}, kVarNone, 0, {}, kBeHip | kBeCpu, kOnShards},   // (a and b, one value per channel, are whole on every device)
  // Caffe's Crop at axis 2 and its gradient (this backend's own): out = the op's offset window of in; in_grad_loss = out_grad_loss inside the window and +0 outside it,
  // every element written.  The offsets ride in the op (`offset`, dims y:x).  Independent per image
  {"hip_crop", kFamBckOp, kOpCrop, "bodahip_crop", {"Crop"}, {{"in", kIn}, {"out", kOut}}, {}, kVarNone, 0, {}, kBeHip | kBeCpu, kOnShards},
  {"hip_crop_bck", kFamBckOp, kOpCropBck, "bodahip_crop_bck", {"BckCrop"}, {{"out_grad_loss", kIn}, {"in_grad_loss", kOut}}, {}, kVarNone, 0, {}, kBeHip | kBeCpu, kOnShards},
  // the solver's update (this backend's own): params, gradients and momentum history are replicated vars
  {"hip_sgd_update", kFamSgd, 0, nullptr, {"SgdUpdate"}, {{"hyper", kIn}}, {}, kVarWghInFront, 0, {}, kBeHip | kBeCpu, kReplicatedOnly},
  // the solvers beyond plain SGD, global-norm clipping (this backend's own; kernels/solver_update_f32.hip): replicated vars throughout
  {"hip_solver_update", kFamSolver, 1, nullptr, {"SolverUpdate"}, {{"hyper", kIn}, {"state", kIn}}, {}, kVarWghH2InFront, 0, {}, kBeHip | kBeCpu, kReplicatedVars},
  {"hip_grad_sumsq", kFamSolver, 2, nullptr, {"GradSumsq"}, {{"partials", kInOut}}, {}, kVarGInFront, 0, {}, kBeHip | kBeCpu, kReplicatedVars},
  {"hip_grad_norm", kFamSolver, 3, nullptr, {"GradNorm"}, {{"partials", kIn}, {"hyper", kIn}, {"state", kOut}}, {}, kVarNone, 0, {}, kBeHip | kBeCpu, kReplicatedVars},
  // gradient accumulation over iter_size micro-steps (the same file): accum = [first, apply, scale, micro] says whether a_i is overwritten or added to, and whether the update applies
  {"hip_grad_accum", kFamSolver, 4, nullptr, {"GradAccum"}, {{"accum", kIn}}, {}, kVarGaInFront, 0, {}, kBeHip | kBeCpu, kReplicatedVars},
  {"hip_solver_update_acc", kFamSolver, 5, nullptr, {"SolverUpdateAcc"}, {{"hyper", kIn}, {"state", kIn}, {"accum", kIn}}, {}, kVarWghH2InFront, 0, {}, kBeHip | kBeCpu, kReplicatedVars},
  // the training BatchNorm and the Eltwise-SUM gradient (this backend's own; kernels/bn_f32.hip).  hip_bn_fwd and hip_fan_out are independent per image, but their calls
  // demand vars of exactly the op's dims, which an img shard does not have: refused with a message of their own, not left to fail on dims
  {"hip_bn_stats", kFamBn, 1, nullptr, {"BnStats"}, {{"in", kIn}, {"mean", kOut}, {"inv_std", kOut}, {"run_mean", kInOut}, {"run_var", kInOut}}, {}, kVarNone, 0, {}, kBeHip | kBeCpu, refused_on_devices(kWhyBnSums)},
  {"hip_bn_fwd", kFamBn, 2, nullptr, {"BnFwd"}, {{"in", kIn}, {"mean", kIn}, {"inv_std", kIn}, {"scale", kIn}, {"bias", kIn}, {"out", kOut}}, {}, kVarNone, 0, {}, kBeHip | kBeCpu,
   refused_on_devices("(hip_bn_fwd) takes vars of exactly its op's dims, not img shards: the training BatchNorm functions and the Eltwise gradient run on one device")},
  {"hip_bn_bck_sums", kFamBn, 3, nullptr, {"BnBckSums"}, {{"in", kIn}, {"mean", kIn}, {"inv_std", kIn}, {"out_grad_loss", kIn}, {"scale_grad_loss", kOut}, {"bias_grad_loss", kOut}}, {}, kVarNone, 0, {}, kBeHip | kBeCpu, refused_on_devices(kWhyBnSums)},
  {"hip_bn_bck_in", kFamBn, 4, nullptr, {"BnBckIn"}, {{"in", kIn}, {"mean", kIn}, {"inv_std", kIn}, {"scale", kIn}, {"scale_grad_loss", kIn}, {"bias_grad_loss", kIn}, {"out_grad_loss", kIn}, {"in_grad_loss", kOut}}, {}, kVarNone, 0, {}, kBeHip | kBeCpu,
   refused_on_devices("(a training BatchNorm's data gradient) divides by the element count of the WHOLE batch, which an img shard does not know")},
  {"hip_fan_out", kFamBn, 5, nullptr, {"FanOut"}, {{"in", kIn}}, {}, kVarOutsBehind, 0, {}, kBeHip | kBeCpu,
   refused_on_devices("(hip_fan_out) takes vars of exactly its op's dims, not img shards: the training BatchNorm functions and the Eltwise gradient run on one device")},
  // the training BatchNorm over img CHUNKS (a family of its own; the args of the hip_bn_* twins).  hip_bnc_stats / hip_bnc_bck_sums carry `chunks` and sum in the chunked
  // chain (kernels/bn_f32.hip); on several devices chunk i is device i's shard and the chunk totals cross the devices (csrc/hip_multi.cc: run_bnc_on_shards, a dispatch
  // on this family).  hip_bnc_fwd / hip_bnc_bck_in are independent per image once fN is the whole batch's, which their op's dims give: they run on shards as they are
  {"hip_bnc_stats", kFamBnc, 1, nullptr, {"BncStats"}, {{"in", kIn}, {"mean", kOut}, {"inv_std", kOut}, {"run_mean", kInOut}, {"run_var", kInOut}}, {}, kVarNone, 0, {}, kBeHip | kBeCpu, kOnShards},
  {"hip_bnc_fwd", kFamBnc, 2, nullptr, {"BncFwd"}, {{"in", kIn}, {"mean", kIn}, {"inv_std", kIn}, {"scale", kIn}, {"bias", kIn}, {"out", kOut}}, {}, kVarNone, 0, {}, kBeHip | kBeCpu, kOnShards},
  {"hip_bnc_bck_sums", kFamBnc, 3, nullptr, {"BncBckSums"}, {{"in", kIn}, {"mean", kIn}, {"inv_std", kIn}, {"out_grad_loss", kIn}, {"scale_grad_loss", kOut}, {"bias_grad_loss", kOut}}, {}, kVarNone, 0, {}, kBeHip | kBeCpu, kOnShards},
  {"hip_bnc_bck_in", kFamBnc, 4, nullptr, {"BncBckIn"}, {{"in", kIn}, {"mean", kIn}, {"inv_std", kIn}, {"scale", kIn}, {"scale_grad_loss", kIn}, {"bias_grad_loss", kIn}, {"out_grad_loss", kIn}, {"in_grad_loss", kOut}}, {}, kVarNone, 0, {}, kBeHip | kBeCpu, kOnShards},
  // BatchNorm on its running pair (fine-tuning with frozen statistics; the same file, a family of its own: kFamBn's rows are pinned).  One device only, refused on
  // several by the family's sentence (kWhyBnfOneDevice; csrc/hip_multi.cc dispatches on the mode).  hip_bnf_bck's in_grad_loss may be out_grad_loss's var
  {"hip_bnf_prep", kFamBnf, 6, nullptr, {"BnfPrep"}, {{"run_mean", kIn}, {"run_var", kIn}, {"mean", kOut}, {"inv_std", kOut}}, {}, kVarNone, 0, {}, kBeHip | kBeCpu, kOneDevice},
  {"hip_bnf_bck", kFamBnf, 7, nullptr, {"BnfBck"}, {{"in", kIn}, {"mean", kIn}, {"inv_std", kIn}, {"scale", kIn}, {"out_grad_loss", kIn}, {"in_grad_loss", kOut}, {"scale_grad_loss", kOut}, {"bias_grad_loss", kOut}}, {}, kVarNone, 0, {}, kBeHip | kBeCpu, kOneDevice},
  {"hip_bnf_bck_in", kFamBnf, 8, nullptr, {"BnfBckIn"}, {{"inv_std", kIn}, {"scale", kIn}, {"out_grad_loss", kIn}, {"in_grad_loss", kOut}}, {}, kVarNone, 0, {}, kBeHip | kBeCpu, kOneDevice},
  // a Convolution / BckConv with group > 1 (this backend's own: the reference has no grouped convolution; kernels/conv_grp_f32.hip): for every group the ungrouped
  // function on the op sliced to that group.  The arg lists of hip_conv, hip_bconv_in and hip_bconv_filts without their optional args; no flag; one device only
  // (why_one_device).  A family of its own: the rows of kFamConv and kFamBconv are pinned.  In front of the loss rows, which stay in front of the table's last four
  {"hip_conv_grp", kFamConvGrp, kConvGrpFwd, nullptr, {"Convolution"}, {BODAHIP_CONV_ARGS}, {}, kVarNone, 0, {}, kBeHip | kBeCpu, kOneDevice},
  {"hip_bconv_in_grp", kFamConvGrp, kConvGrpBckIn, nullptr, {"BckConv"}, {{"filts", kIn}, {"out_grad_loss", kIn}, {"stride", kRef}, {"in_pad", kRef}, {"in_grad_loss", kOut}}, {}, kVarNone, 0, {}, kBeHip | kBeCpu, kOneDevice},
  {"hip_bconv_filts_grp", kFamConvGrp, kConvGrpBckFilts, nullptr, {"BckConv"}, {{"in", kIn}, {"out_grad_loss", kIn}, {"stride", kRef}, {"in_pad", kRef}, {"filts_grad_loss", kOut}}, {}, kVarNone, 0, {}, kBeHip | kBeCpu, kOneDevice},
  // a Deconvolution / BckDeconv (this backend's own: the reference knows the op type and its shapes but has no function for it; kernels/deconv_f32.hip).  in is
  // img:chan=C:y:x, filts in_chan=C:out_chan=OC:y:x (Caffe's blob), out img:OC:(H-1)*SY+KH-2*PY:(W-1)*SX+KW-2*PX.  Each function is an existing one with the operands'
  // roles exchanged (deconv_geom_of_op below); no group, no fused ReLU, no flag; one device only (why_one_device).  In front of the loss rows, like the grouped rows
  {"hip_deconv", kFamDeconv, kDeconvFwd, nullptr, {"Deconvolution"}, {BODAHIP_CONV_ARGS}, {}, kVarNone, 0, {}, kBeHip | kBeCpu, kOneDevice},
  {"hip_deconv_bck_in", kFamDeconv, kDeconvBckIn, nullptr, {"BckDeconv"}, {{"filts", kIn}, {"out_grad_loss", kIn}, {"stride", kRef}, {"in_pad", kRef}, {"in_grad_loss", kOut}}, {}, kVarNone, 0, {}, kBeHip | kBeCpu, kOneDevice},
  {"hip_deconv_bck_filts", kFamDeconv, kDeconvBckFilts, nullptr, {"BckDeconv"}, {{"in", kIn}, {"out_grad_loss", kIn}, {"stride", kRef}, {"in_pad", kRef}, {"filts_grad_loss", kOut}}, {}, kVarNone, 0, {}, kBeHip | kBeCpu, kOneDevice},
  {"hip_deconv_bck_biases", kFamDeconv, kDeconvBckBiases, nullptr, {"BckDeconv"}, {{"out_grad_loss", kIn}, {"biases_grad_loss", kOut}}, {}, kVarNone, 0, {}, kBeHip | kBeCpu, kOneDevice},
  // the full SoftmaxWithLoss (this backend's own; kernels/loss_f32.hip): what a head with a LossSpec lowers to -- loss_weight, ignore_label, planes, the four
  // normalisers.  hip_softmax_loss_bck reads s = weight / Z from loss_state on the device.  One device only (why_one_device).  In front of the data and eval rows,
  // which stay the table's last four
  {"hip_softmax_loss_fwd", kFamLoss, 1, nullptr, {"SoftmaxLossFwd"}, {{"in", kIn}, {"label", kIn}, {"prob", kOut}, {"loss_per_pel", kOut}}, {}, kVarNone, 0, {}, kBeHip | kBeCpu, kOneDevice},
  {"hip_loss_norm", kFamLoss, 2, nullptr, {"LossNorm"}, {{"label", kIn}, {"loss_per_pel", kIn}, {"loss", kOut}, {"loss_state", kOut}}, {}, kVarNone, 0, {}, kBeHip | kBeCpu, kOneDevice},
  {"hip_softmax_loss_bck", kFamLoss, 3, nullptr, {"SoftmaxLossBck"}, {{"prob", kIn}, {"label", kIn}, {"loss_state", kIn}, {"in_grad_loss", kOut}}, {}, kVarNone, 0, {}, kBeHip | kBeCpu, kOneDevice},
  // the input transform of the gradient pipe (this backend's own; kernels/data_f32.hip): crop, mirror, mean and scale from uint8 images under a per-image plan var
  // (independent per image: src, plan and out are img shards, mean is whole on every device).  In front of the eval rows, which stay the table's last three
  {"hip_data_transform", kFamData, 1, nullptr, {"DataTransform"}, {{"src", kIn}, {"plan", kIn}, {"mean", kIn}, {"out", kOut}}, {}, kVarNone, 0, {}, kBeHip | kBeCpu, kOnShards},
  // the evaluation pass of the gradient pipe (this backend's own; kernels/eval_f32.hip): the rank of the true class per image (independent per image), the batch's counts
  // and loss added into two accumulators under ctl = [first, 0, 0, 0] (hip_grad_accum's protocol), and a BatchNorm + Scale run's running statistics folded into (a, b)
  {"hip_accuracy", kFamEval, 1, nullptr, {"Accuracy"}, {{"in", kIn}, {"label", kIn}, {"rank", kOut}}, {}, kVarNone, 0, {}, kBeHip | kBeCpu, kOnShards},
  {"hip_eval_accum", kFamEval, 2, nullptr, {"EvalAccum"}, {{"rank", kIn}, {"loss", kIn}, {"ctl", kIn}, {"counts", kInOut}, {"loss_sum", kInOut}}, {}, kVarNone, 0, {}, kBeHip | kBeCpu, kReplicatedVars},
  {"hip_bn_fold", kFamEval, 3, nullptr, {"BnFold"}, {{"run_mean", kIn}, {"run_var", kIn}, {"scale", kIn}, {"bias", kIn}, {"a", kOut}, {"b", kOut}}, {}, kVarNone, 0, {}, kBeHip | kBeCpu, kReplicatedVars},
};
#undef BODAHIP_CONV_ARGS

inline native_func_t const *find_native_func(string const &fn) { for (auto const &f : kNativeFuncs) if (fn == f.name) return &f; return nullptr; }
inline native_func_t const *find_native_func(func_family_t family, int member) { for (auto const &f : kNativeFuncs) if (f.family == family && f.member == member) return &f; return nullptr; }
// the functions of a bare op of type t, in call order (empty: no such op).  kBconvFiltsBiases is nobody's default call, and the grouped functions belong to annotated ops
inline std::vector<native_func_t const *> native_funcs_of_type(string const &t, unsigned backend = kBeHip) {
  std::vector<native_func_t const *> r;
  for (auto const &f : kNativeFuncs) if (f.of_type(t) && (f.backends & backend) && !(f.family == kFamBconv && f.member == kBconvFiltsBiases) && f.family != kFamConvGrp) r.push_back(&f);
  std::stable_sort(r.begin(), r.end(), [](native_func_t const *a, native_func_t const *b) { return a->member < b->member; });
  return r;
}
// "a, b and c" (last_sep " and ") or "a, b, c" (last_sep ", "): the rows `pick` accepts, in table order
template <typename F> inline string native_func_names(F const &pick, char const *last_sep) {
  std::vector<char const *> ns; for (auto const &f : kNativeFuncs) if (pick(f)) ns.push_back(f.name);
  string r; for (size_t i = 0; i < ns.size(); ++i) r += string(i ? (i + 1 == ns.size() ? last_sep : ", ") : "") + ns[i];
  return r;
}
inline bool native_func_takes_flag(string const &fn, unsigned flag) { native_func_t const *f = find_native_func(fn); return f && (f->flags & flag); }
inline bool native_type_takes_flag(string const &t, unsigned flag) { for (auto const &f : kNativeFuncs) if ((f.flags & flag) && f.of_type(t)) return true; return false; }
inline string native_funcs_taking_flag(unsigned flag) { return native_func_names([&](native_func_t const &f) { return (f.flags & flag) != 0; }, " and "); }
inline int native_func_member(string const &fn, func_family_t family) { native_func_t const *f = find_native_func(fn); return (f && f->family == family) ? f->member : 0; }
inline char const *native_func_type(func_family_t family, int member) { native_func_t const *f = find_native_func(family, member); return f ? f->types[0] : ""; }
inline string native_family_names(func_family_t family) { return native_func_names([&](native_func_t const &f) { return f.family == family; }, ", "); }

// hip_operands, a str_val of a function op that travels with it like hip_tile and hip_exact (no kFlag*: it adds no arg and changes no row).  Absent, empty or "f32": the
// function as it is.  "bf16" on hip_bconv_in / hip_bconv_filts_biases: the operands of the products are rounded to bf16 (round-to-nearest-even) and the sums stay fp32
// (kernels/bconv_in_bf16.hip, kernels/bconv_fb_bf16.hip; be=cpu rounds and runs its template loops); the bias gradient is summed from the unrounded values.  Only the
// bconv family looks at the value
inline constexpr char kWhyNoBf16Pair[] = "hip_operands=bf16: the filter and bias gradients have their bf16-operand form as ONE call, hip_bconv_filts_biases (cnn_op.bconv_filts_biases_func_op); hip_bconv_filts and hip_bconv_biases are fp32 only";
inline bool op_bf16_operands(op_base_t const &op) {
  auto const it = op.str_vals.find("hip_operands");
  if (it == op.str_vals.end() || !op.has_func_name()) return false;
  native_func_t const *f = find_native_func(op.get_func_name());
  if (!f || f->family != kFamBconv) return false;
  if (it->second.empty() || it->second == "f32") return false;
  if (it->second != "bf16") rt_err(string(f->name) + ": hip_operands must be f32 | bf16, got '" + it->second + "'");
  if (f->member != kBconvIn && f->member != kBconvFiltsBiases) unsup_err(string(f->name) + ": " + kWhyNoBf16Pair);
  return true;
}

// the grouped family (kFamConvGrp): what both backends read from the function's op, and every refusal that needs the op alone.  The op is a Convolution (member
// kConvGrpFwd: in, filts, biases, out, conv_has_relu) or a BckConv (in, filts, out_grad_loss in the place of out) that carries group = g > 1: C and OC multiples of g,
// filts = out_chan=OC : in_chan=C/g : y : x.  Group j reads channels [j*CG, (j+1)*CG) of in and filter rows / writes out_chans [j*OCG, (j+1)*OCG)
struct conv_grp_geom_t { int B, C, H, W, OC, KH, KW, SY, SX, PY, PX, OH, OW, G, CG, OCG; bool relu; };
inline uint32_t op_group(op_base_t const &op) { return op.has("group") ? op.get_u32("group") : 1u; }
inline conv_grp_geom_t conv_grp_geom_of_op(op_base_t const &op, int member) {
  native_func_t const *row = find_native_func(kFamConvGrp, member);
  string const fn = row ? row->name : "hip_conv_grp";
  if (row && !row->of_type(op.get_type())) rt_err(fn + ": a function of op type " + row->types[0] + ", not " + op.get_type());
  bool const fwd = member == kConvGrpFwd;
  dims_t const &f = op.get_dims("filts"), &in = op.get_dims("in"), &out = op.get_dims(fwd ? "out" : "out_grad_loss"), &st = op.get_dims("stride"), &pad = op.get_dims("in_pad");
  if (f.sz() != 4 || in.sz() != 4 || out.sz() != 4 || st.sz() != 2 || pad.sz() != 2 || f.tn != "float" || in.tn != "float" || out.tn != "float")
    rt_err(fn + ": float filts out_chan:in_chan:y:x, in / out img:chan:y:x, stride / in_pad y:x");
  conv_grp_geom_t g;
  g.B = (int)in.dsz("img"); g.C = (int)in.dsz("chan"); g.H = (int)in.dsz("y"); g.W = (int)in.dsz("x"); g.OC = (int)f.dsz("out_chan"); g.KH = (int)f.dsz("y"); g.KW = (int)f.dsz("x");
  g.SY = (int)st.dsz("y"); g.SX = (int)st.dsz("x"); g.PY = (int)pad.dsz("y"); g.PX = (int)pad.dsz("x"); g.OH = (int)out.dsz("y"); g.OW = (int)out.dsz("x");
  g.relu = fwd && op.get_u32("conv_has_relu") != 0;
  uint32_t const grp = op_group(op);
  if (grp < 2) rt_err(fn + ": the op carries no group > 1: an ungrouped convolution belongs to hip_conv / hip_bconv_in / hip_bconv_filts");
  if (g.C % grp || g.OC % grp || f.dsz("in_chan") * grp != (uint32_t)g.C)
    rt_err(fn + ": group=" + std::to_string(grp) + " needs in.chan=" + std::to_string(g.C) + " and filts.out_chan=" + std::to_string(g.OC) + " to be multiples of it and filts.in_chan=" + std::to_string(f.dsz("in_chan")) + " to be in.chan/group");
  g.G = (int)grp; g.CG = g.C / g.G; g.OCG = g.OC / g.G;
  if (g.B < 1 || g.H < 1 || g.W < 1 || g.KH < 1 || g.KW < 1 || g.SY < 1 || g.SX < 1 || g.PY < 0 || g.PX < 0 || g.OH < 1 || g.OW < 1 || g.SY > 16 || g.SX > 16 || g.KH > 64 || g.KW > 64) unsup_err(fn + ": unsupported geometry");
  if (out.dsz("img") != (uint32_t)g.B || out.dsz("chan") != (uint32_t)g.OC || (g.H + 2 * g.PY - g.KH) / g.SY + 1 != g.OH || (g.W + 2 * g.PX - g.KW) / g.SX + 1 != g.OW)
    rt_err(fn + ": " + (fwd ? "out" : "out_grad_loss") + " dims do not match in / filts / stride / in_pad");
  if (fwd && op.get_dims("biases").dims_prod() != (uint64_t)g.OC) rt_err(fn + ": biases must hold out_chan values");
  if (member == kConvGrpBckIn && !(op.get_dims("in_grad_loss") == in)) rt_err(fn + ": in_grad_loss must have the dims of in");
  if (member == kConvGrpBckFilts && !(op.get_dims("filts_grad_loss") == f)) rt_err(fn + ": filts_grad_loss must have the dims of filts");
  uint64_t const in_b = 4ull * g.B * g.C * g.H * g.W, out_b = 4ull * g.B * g.OC * g.OH * g.OW, f_b = 4ull * g.OC * g.CG * g.KH * g.KW;
  if (in_b >= 0x7ffffff0ull || out_b >= 0x7ffffff0ull || f_b >= 0x7ffffff0ull) unsup_err(fn + ": tensors of 2 GiB or more (32-bit offsets)");
  return g;
}

// the Deconvolution family (kFamDeconv): what both backends read from the function's op, and every refusal that needs the op alone.  The geometry is the LAYER's:
// in B x C x H x W (the small map), filts C x OC x KH x KW, out / out_grad_loss B x OC x OH x OW with OH = (H-1)*SY + KH - 2*PY.  The functions are, term for term,
//   forward          hip_bconv_in     on (filts := filts, out_grad_loss := in) -> acc; out = acc + biases[oc], one fp32 add
//   data gradient    hip_conv         on (filts := filts read as out_chan=C:in_chan=OC, biases := C values of +0, in := out_grad_loss), no ReLU
//   filter gradient  hip_bconv_filts  on (in := out_grad_loss, out_grad_loss := in): K = B*H*W of the small map
//   bias gradient    hip_bconv_biases on out_grad_loss
// of the convolution OC -> C whose input plane is OH x OW and whose output plane is H x W
struct deconv_geom_t { int B, C, H, W, OC, KH, KW, SY, SX, PY, PX, OH, OW; };
inline deconv_geom_t deconv_geom_of_op(op_base_t const &op, int member) {
  native_func_t const *row = find_native_func(kFamDeconv, member);
  string const fn = row ? row->name : "hip_deconv";
  if (row && !row->of_type(op.get_type())) rt_err(fn + ": a function of op type " + row->types[0] + ", not " + op.get_type());
  bool const fwd = member == kDeconvFwd;
  if (op.has("group") && op.get_u32("group") != 1) unsup_err(fn + ": the op carries group=" + std::to_string(op.get_u32("group")) + ": a Deconvolution with group > 1 is out of scope");
  if (op.has("conv_has_relu") && op.get_u32("conv_has_relu") != 0) unsup_err(fn + ": the op carries conv_has_relu=1: a Deconvolution has no fused ReLU");
  dims_t const &f = op.get_dims("filts"), &in = op.get_dims("in"), &out = op.get_dims(fwd ? "out" : "out_grad_loss"), &st = op.get_dims("stride"), &pad = op.get_dims("in_pad");
  if (f.sz() != 4 || in.sz() != 4 || out.sz() != 4 || st.sz() != 2 || pad.sz() != 2 || f.tn != "float" || in.tn != "float" || out.tn != "float" || f.names(0) != "in_chan" || f.names(1) != "out_chan")
    rt_err(fn + ": float filts in_chan:out_chan:y:x, in / out img:chan:y:x, stride / in_pad y:x");
  deconv_geom_t g;
  g.B = (int)in.dsz("img"); g.C = (int)in.dsz("chan"); g.H = (int)in.dsz("y"); g.W = (int)in.dsz("x"); g.OC = (int)f.dsz("out_chan"); g.KH = (int)f.dsz("y"); g.KW = (int)f.dsz("x");
  g.SY = (int)st.dsz("y"); g.SX = (int)st.dsz("x"); g.PY = (int)pad.dsz("y"); g.PX = (int)pad.dsz("x"); g.OH = (int)out.dsz("y"); g.OW = (int)out.dsz("x");
  if (f.dsz("in_chan") != (uint32_t)g.C) rt_err(fn + ": filts.in_chan=" + std::to_string(f.dsz("in_chan")) + " is not in.chan=" + std::to_string(g.C));
  if (g.B < 1 || g.C < 1 || g.OC < 1 || g.H < 1 || g.W < 1 || g.KH < 1 || g.KW < 1 || g.SY < 1 || g.SX < 1 || g.PY < 0 || g.PX < 0 || g.OH < 1 || g.OW < 1 || g.SY > 32 || g.SX > 32 || g.KH > 64 || g.KW > 64)
    unsup_err(fn + ": unsupported geometry (kernels of at most 64 x 64, strides of at most 32)");
  if (out.dsz("img") != (uint32_t)g.B || out.dsz("chan") != (uint32_t)g.OC || (g.H - 1) * g.SY + g.KH - 2 * g.PY != g.OH || (g.W - 1) * g.SX + g.KW - 2 * g.PX != g.OW)
    rt_err(fn + ": " + (fwd ? "out" : "out_grad_loss") + " dims " + out.pretty_str() + " are not img:out_chan:(y-1)*stride+kern-2*pad of in " + in.pretty_str());
  if (fwd && op.get_dims("biases").dims_prod() != (uint64_t)g.OC) rt_err(fn + ": biases must hold out_chan values");
  if (member == kDeconvBckIn && !(op.get_dims("in_grad_loss") == in)) rt_err(fn + ": in_grad_loss must have the dims of in");
  if (member == kDeconvBckFilts && !(op.get_dims("filts_grad_loss") == f)) rt_err(fn + ": filts_grad_loss must have the dims of filts");
  if (member == kDeconvBckBiases && op.get_dims("biases_grad_loss").dims_prod() != (uint64_t)g.OC) rt_err(fn + ": biases_grad_loss must hold out_chan values");
  uint64_t const in_b = 4ull * g.B * g.C * g.H * g.W, out_b = 4ull * g.B * g.OC * g.OH * g.OW, f_b = 4ull * g.OC * g.C * g.KH * g.KW;
  if (in_b >= 0x7ffffff0ull || out_b >= 0x7ffffff0ull || f_b >= 0x7ffffff0ull) unsup_err(fn + ": tensors of 2 GiB or more (32-bit offsets)");
  return g;
}

// the (arg, kind) list of an annotated function op: the fixed args with the variable part and the flag's arg applied (what boda_amd/cnn_op.py calls pipe_func_args)
inline std::vector<func_arg_t> fixed_args(native_func_t const &f) { std::vector<func_arg_t> r; for (auto const &a : f.args) { if (!a.name) break; r.push_back(a); } return r; }
typedef std::vector<std::pair<string, arg_kind_t>> vect_func_arg_t;
inline vect_func_arg_t native_func_args(native_func_t const &f, op_base_t const &op) {
  string const fn = f.name;
  vect_func_arg_t r; for (func_arg_t const &a : fixed_args(f)) r.emplace_back(a.name, a.kind);
  auto count = [&](char const *an, uint32_t lo, uint32_t hi, char const *what) {
    uint32_t const n = op.get_u32(an);
    if (n < lo || n > hi) unsup_err(fn + ": " + an + "=" + std::to_string(n) + ": " + std::to_string(lo) + " to " + std::to_string(hi) + " " + what);
    return n; };
  if (f.var == kVarMembers) unsup_err(fn + ": the arg list is a list of members, which the function's handler describes");
  if (f.var == kVarInsBeforeLast) { uint32_t const n = count("ins_num", 2, 8, "inputs"); for (uint32_t i = 0; i < n; ++i) r.emplace(r.end() - 1, "ins_" + std::to_string(i), kIn); }   // the reference's flattened names of the multi arg `ins`
  if (f.var == kVarOutsBehind) { uint32_t const n = count("outs_num", 2, kFanOutMax, "outputs"); for (uint32_t i = 0; i < n; ++i) r.emplace_back("outs_" + std::to_string(i), kOut); }
  if (f.var == kVarWghInFront) {
    uint32_t const n = count("tens_num", 1, kSgdUpdateMaxTens, "tensors"); vect_func_arg_t per;
    for (uint32_t i = 0; i < n; ++i) { string const sx = "_" + std::to_string(i); per.emplace_back("w" + sx, kInOut); per.emplace_back("g" + sx, kIn); per.emplace_back("h" + sx, kInOut); }
    r.insert(r.begin(), per.begin(), per.end());
  }
  if ((f.var == kVarWghH2InFront || f.var == kVarGInFront || f.var == kVarGaInFront) && op.has("tens_num")) {
    uint32_t const n = count("tens_num", 1, kSgdUpdateMaxTens, "tensors"); vect_func_arg_t per;
    auto const st = op.str_vals.find("solver_type");
    bool const adam = f.var == kVarWghH2InFront && st != op.str_vals.end() && st->second == "adam";
    for (uint32_t i = 0; i < n; ++i) {
      string const sx = "_" + std::to_string(i);
      if (f.var == kVarWghH2InFront) { per.emplace_back("w" + sx, kInOut); per.emplace_back("g" + sx, kIn); per.emplace_back("h" + sx, kInOut); if (adam) per.emplace_back("h2" + sx, kInOut); }
      else { per.emplace_back("g" + sx, kIn); if (f.var == kVarGaInFront) per.emplace_back("a" + sx, kInOut); }
    }
    r.insert(r.begin(), per.begin(), per.end());
  }
  if (f.flag_arg.flag && op_flag_set(op, f.flag_arg.flag)) r.emplace(f.flag_arg.at >= 0 ? r.begin() + f.flag_arg.at : r.end() - 1, f.flag_arg.name, kIn);
  return r;
}
// the IN / OUT var args of a kFamBckOp function in call order, without the flag's arg (which its handler binds by name); refs: does it take kern_sz / stride / in_pad
struct bck_op_args_t { std::vector<string> ins, outs; bool refs = false; };
inline bck_op_args_t bck_op_args(native_func_t const &f, op_base_t const &op) {
  bck_op_args_t r; native_func_t plain = f; plain.flag_arg = flag_arg_t{};
  for (auto const &a : native_func_args(plain, op)) { if (a.second == kIn) r.ins.push_back(a.first); else if (a.second == kOut) r.outs.push_back(a.first); else if (a.second == kRef) r.refs = true; }
  return r;
}

} // namespace bodahip
