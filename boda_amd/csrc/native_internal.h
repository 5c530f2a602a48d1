// native_internal.h -- what the translation units behind native_kernels.h share: kernel argument structs, the plan record, the planners' and the launch helpers' prototypes.
// native_plan.cc: tile / variant selection (host logic only); native_kernels.cc: specialisation, launch, the fp32 entry points; native_nhwc.cc: the channels-last bf16 entry
// points; native_run.cc: the rtc function interface (run, prebuild / explain_plan).
#pragma once
#include "native_kernels.h"
#include <algorithm>
#include <cstdlib>
#include <sstream>

namespace bodahip {

// The structs passed by value to a kernel or copied into a device-side table: declared once, for the host and the device compiler, with their layout assertions.
// (chain_args_t, the arguments of kernels/k1_quad_f32.hip -DCHAIN=1, is a struct of its own derived from gemm_args_t, not a longer gemm_args_t: gemm_args_t is also the
// element type of the member tables of hip_conv_nhwc_set and the argument of every other contraction kernel, so its size must not move with the chain's fields.)
#include "kernels/kernel_args.h"
static_assert(kSgdMaxTens == kSgdUpdateMaxTens, "hip_sgd_update: the op's limit is the size of the argument table");
// enum kernel_src_t: one value kSrc_<name> per embedded kernels/<name>.hip, in the order of build.py's KERNELS (kernels_embed.inc; the texts are native_kernels.cc's)
#include "kernels_embed.inc"
kernel_text_t const &kernel_source(kernel_src_t s);

struct kernel_t { hipModule_t mod = nullptr; hipFunction_t func = nullptr; int occ = 0; };   // occ: resident workgroups per CU (queried on first use by the persistent forms)

struct native_kernels_t::impl_t {
  std::map<string, kernel_t> kernels; // key = option string
  std::map<string, string> tune;
  void *ws = nullptr; size_t ws_bytes = 0; // split-K partial-sum slabs (grow-only scratch, like the reference's cudnn scratch var)
  bool ws_used = false;                    // ensure_ws was called since run() began: the call works in the shared scratch (native_kernels_t::last_call_uses_ws)
  std::vector<void *> ws_retired;          // outgrown scratch buffers that captured graphs may still point into (freed with the backend)
  std::map<string, void *> ktabs;           // im2col gather tables, one per (C,H,W,KH,KW) (device memory)
  int call_ws_hold = 0;                       // > 0: a launch is collecting several of them (hip_conv_nhwc_set): none may be dropped
  size_t call_ws_bytes = 0;                   // sum of the per-call workspaces ("ksl:" / "kho:" entries of ktabs): bounded, see call_ws_make_room
  size_t ts_off = 0, ts_bytes = 0; string ts_hdr;   // experiment hook BODAHIP_CBIG_TSTAMP=<file>:late -- the clock stamps of the LAST staging-wave launch, written out when the backend goes
  hipModule_t wino_mod = nullptr; hipFunction_t wino_filt = nullptr, wino_in = nullptr, wino_out = nullptr, wino_fused = nullptr, wino_filt_t = nullptr; // kernels/winograd_f32.hip
};


struct plan_t { tile_cfg_t cfg; vect_string defs; string kname; long split_pels = 0; tile_cfg_t tail_cfg; vect_string tail_defs;   /* split_pels > 0 (staging-wave convolution, round 6): two-level tiling along the pels -- this plan's tiles over the first split_pels pels (whole rounds of the CUs), tail_cfg's over the rest */ kernel_src_t src = kSrc_gemm_conv_f32;   /* the kernels/<name>.hip this plan specialises: set where kname is set.  The flags below: what launch code branches on */ bool ipconv = false, k1 = false, bf16 = false, patch = false, stream = false, quad = false, fc = false, cbig = false, rdec = false, patch16 = false, nhwc = false, nhwc_patch = false, ksl = false, bconv_in = false; int rows = 0, cg = 0; };

// (the functions of the gradient pipe's non-conv ops, their kernels and their args: the kFamBckOp rows of native_funcs.h)
struct bck_plan_t { plan_t p; long threads = 0; uint32_t grid = 0, block = 256; int CB = 0; double algo_bytes = 0; };
bck_plan_t plan_bck_op(bck_op_geom_t const &g, int num_cus);
bck_plan_t plan_shard_sum(int nslabs, long stride, long n);   // OP 14 of the same file: no function of its own, the multi-device backend's sum of per-shard partials

// hip_sgd_update (kernels/sgd_update_f32.hip): the table of up to kSgdMaxTens tensors rides by value in the kernel arguments (sgd_update_args_t)
constexpr long kSgdChunk = 4096;   // floats of one tensor a workgroup owns
struct sgd_plan_t { plan_t p; uint32_t grid = 0, block = 256; std::vector<uint32_t> blk0; double algo_bytes = 0; };
sgd_plan_t plan_sgd_update(std::vector<long> const &elems);
// the solver family (kernels/solver_update_f32.hip; solver_update_args_t, grad_sumsq_args_t, grad_norm_args_t): the same chunking, so the same plan record.  hip_grad_norm:
// one workgroup, blk0 empty
static_assert(kSolverChunk == kSgdChunk, "the solver family cuts tensors into hip_sgd_update's chunks");
sgd_plan_t plan_solver(solver_op_t const &so);
string solver_plan_desc(solver_op_t const &so, sgd_plan_t const &sp);

// the training BatchNorm functions and hip_fan_out (kernels/bn_f32.hip, bn_args_t)
// the kernels of one call in launch order: op 1 (a sum over slabs; mode 0 S1, 1 S2, 2 the bck_sums pair), 2 (the finalising step; fin 1 stats, 2 bck_sums), 3 fwd, 4 bck_in, 5 fan_out
struct bn_launch_t { plan_t p; int op = 0; };
struct bn_plan_t { std::vector<bn_launch_t> ls; double algo_bytes = 0; size_t ws_bytes = 0, ws_part = 0; };   // ws_part (the chunked chain): floats of slab partials in front of the totals
bn_plan_t plan_bn(bn_op_t const &b);
plan_t bn_kernel_plan(int op, char const *kname, vect_string const &defs);   // one specialisation of kernels/bn_f32.hip (plan_bn's entries are these)
string bn_plan_desc(bn_op_t const &b, bn_plan_t const &bp);

// the eval family (kernels/eval_f32.hip; accuracy_args_t, eval_accum_args_t, bn_fold_args_t): one launch per call, nothing to choose but the grid
bck_plan_t plan_eval_op(eval_op_t const &e);
string eval_plan_desc(eval_op_t const &e, bck_plan_t const &bp);

// the data family (kernels/data_f32.hip; data_transform_args_t): one launch per call; d.B is the call's image count
bck_plan_t plan_data_op(data_op_t const &d);
string data_plan_desc(data_op_t const &d, bck_plan_t const &bp);

// the loss family (kernels/loss_f32.hip; softmax_loss_fwd_args_t, loss_norm_args_t, softmax_loss_bck_args_t): one launch per call
bck_plan_t plan_loss_op(loss_op_t const &l);
string loss_plan_desc(loss_op_t const &l, bck_plan_t const &bp);

struct sgemm_split_t { uint32_t m_main = 0; string tail_tile; double t_single = 0, t_split = 0; };
static char const *const kBigTile = "256x256x16x2x4x1x1x32x2";
struct sgemm_part_t { uint32_t m0 = 0, rows = 0, n0 = 0, cols = 0; string tile; };
struct set_member_in_t { conv_geom_t g; bool patch_filts, pool; int grp_pad; };
struct set_layout_t { std::vector<int> in_set, alone, variant_of; std::vector<plan_t const *> variants; std::vector<string> vkeys; int minw = 8; string skey; };

bool parse_tile(string const &s, tile_cfg_t &c);
void launch(native_host_t *host, kernel_t &k, gemm_args_t &a, tile_cfg_t const &c);
plan_t plan_sgemm(uint32_t M, uint32_t N, uint32_t K, int num_cus, string const &tile, bool bf16 = false, int batch = 1, bool allow_big = true);
bool plan_patch_bf16(conv_geom_t const &g, int num_cus, plan_t &p);
plan_t plan_conv_nhwc(conv_geom_t const &g, int num_cus, string const &tile, bool out_f32, int grp_pad = 0, bool allow_split = true, bool res = false);   // res: -DRES=1, the residual epilogue
plan_t plan_conv_nhwc_patch(conv_geom_t const &g, int num_cus, string const &tile_arg, bool out_f32, bool pool = false);
bool plan_conv_nhwc_rows(conv_geom_t const &g, post_ops_t const &post, int num_cus, plan_t &p, string *why = nullptr);
bool rows_auto(conv_geom_t const &g, int num_cus, string const &tile);
bool apply_post_ops(op_base_t const &op, conv_geom_t &g, post_ops_t &post, char const *what);
bool plan_ipconv_dma(conv_geom_t const &g, int num_cus, plan_t &p);
plan_t plan_conv(conv_geom_t const &g, int num_cus, string const &tile, bool bf16 = false, string const &k1s = string(), bool allow_splitk = true, bool exact = true);
plan_t plan_bconv_in(conv_geom_t const &g, int num_cus, string const &tile, bool zinp = false);   // (zinp: -DZINP=1) BckConv data gradient (kernels/bconv_in_f32.hip)
plan_t plan_bconv_filts(conv_geom_t const &g, int num_cus, string const &tile);    // BckConv filter gradient, in-launch K slices (kernels/bconv_filts_f32.hip)
plan_t plan_bconv_filts_biases(conv_geom_t const &g, int num_cus, string const &tile);   // the fused filter + bias gradient, k-major staging, slab slices (kernels/bconv_fb_f32.hip)
plan_t plan_bconv_in_bf16(conv_geom_t const &g, int num_cus, string const &tile, bool zinp = false);   // hip_operands=bf16: kernels/bconv_in_bf16.hip (plan_t::bf16 is set)
plan_t plan_bconv_fb_bf16(conv_geom_t const &g, int num_cus, string const &tile);                     // hip_operands=bf16: kernels/bconv_fb_bf16.hip; its second launch is plan_bconv_slab_sum's
plan_t plan_bconv_slab_sum();                                                        // its second launch: the slabs added in slice order (kernels/bconv_fb_f32.hip -DSLAB_SUM)
plan_t plan_bconv_biases();                                                          // BckConv bias gradient (kernels/bconv_filts_f32.hip -DBIAS_ONLY)
plan_t plan_conv_grp(conv_grp_geom_t const &g, int member, int num_cus, string const &tile);   // the grouped family (kernels/conv_grp_f32.hip); member: kConvGrpFwd | kConvGrpBckIn | kConvGrpBckFilts
plan_t plan_conv_grp_slab_sum(plan_t const &main);   // the second launch of a sliced direct filter gradient
bool conv_grp_has_slab_sum(plan_t const &p);
long conv_grp_threads(conv_grp_geom_t const &g, int member, tile_cfg_t const &c, uint32_t *grid, uint32_t *block);   // -> the kernel's p.n; *grid workgroups of *block threads
plan_t plan_deconv(deconv_geom_t const &g, int member, int num_cus, string const &tile);   // the Deconvolution family (kernels/deconv_f32.hip); member: kDeconvFwd | kDeconvBckIn | kDeconvBckFilts
plan_t plan_deconv_slab_sum(plan_t const &main);     // the second launch of a sliced filter gradient
bool deconv_has_slab_sum(plan_t const &p);
void deconv_grid(deconv_geom_t const &g, int member, tile_cfg_t const &c, int num_cus, uint32_t *grid, int *zs, int *per);   // *grid workgroups of 256 threads; forward: *zs chunks of *per items
long bconv_in_tiles(conv_geom_t const &g, int BJ);                                  // pel tiles over all SY x SX phases (the kernel's walk)
std::vector<char> compile_plan(plan_t const &p, string const &arch, string *log);
void ensure_ws(native_kernels_t::impl_t *impl, native_host_t *host, size_t need);
void call_ws_make_room(native_kernels_t::impl_t *impl, native_host_t *host, size_t need);
void setup_ksl(native_kernels_t::impl_t *impl, native_host_t *host, gemm_args_t &ga, tile_cfg_t const &cfg, long nk, void const *key_ptr, char const *what);
string tune_of(native_kernels_t::impl_t *impl, char const *key);
sgemm_split_t plan_sgemm_split(uint32_t M, uint32_t N, uint32_t K, int num_cus);
string sgemm_wide_tile(uint32_t M, uint32_t N, uint32_t K, long cus);
bool parse_parts_env(uint32_t M, uint32_t N, uint32_t K, std::vector<sgemm_part_t> &out);
std::vector<sgemm_part_t> plan_sgemm_parts(uint32_t M, uint32_t N, uint32_t K, int cus);
bool s2d_geom(conv_geom_t const &g, conv_geom_t &g2, int &pry, int &prx);
bool winograd_applies(conv_geom_t const &g, string const &algo);
long wino_chunk_imgs(conv_geom_t const &g);
bool plan_k1_chain(conv_geom_t const &g, int oc2, bool relu2, plan_t &p);
plan_t plan_conv_nhwc_multi(std::vector<conv_geom_t> const &gs, string const &tile, bool out_f32);
string set_kernel_source(std::vector<plan_t const *> const &variants, int threads, int minw);
plan_t plan_set_member(set_member_in_t const &mi, int num_cus, bool out_f32);
double set_tile_cost(set_member_in_t const &mi, plan_t const &p);
set_layout_t layout_set(std::vector<plan_t> const &plans, std::vector<double> const &tile_cost);
kernel_t &get_kernel(native_kernels_t::impl_t *impl, native_host_t *host, plan_t const &p);

} // namespace bodahip
