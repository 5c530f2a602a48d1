// rtc_types.h -- value types and the abstract backend interface of the rtc_compute layer.
//
// Mirrors (same names, same field meaning, same error behaviour) the reference's plugin boundary so that a
// backend written against this header is a drop-in for Boda's own callers:
//   dims_t / dim_t            src/boda_base.H:424-450,498-690      (row-major named dims + type name)
//   nda_t                     src/boda_base.H:751-810              (dims + optional raw element pointer)
//   op_base_t                 src/op_base.H:9-43, src/op_base.cc   (str_vals + nda_vals, ordering)
//   rtc_compile_opts_t, rtc_func_info_t, rtc_arg_t, rtc_func_call_t, rtc_compute_t
//                             src/rtc_compute.H:9-127
//   rt_err / unsup_err        src/boda_base.H:98,105               (fatal vs. "unsupported, caller may record")
// Written from the interface's behaviour; this is not a copy of those headers (no NESI, no boost).
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <map>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

namespace bodahip {

using std::string;
typedef std::vector<string> vect_string;

// ---- errors -------------------------------------------------------------------------------------------------------
struct rt_exception : public std::runtime_error { explicit rt_exception(string const &m) : std::runtime_error(m) {} };
struct unsup_exception : public std::runtime_error { explicit unsup_exception(string const &m) : std::runtime_error(m) {} };
[[noreturn]] inline void rt_err(string const &m) { throw rt_exception("error: " + m); }
[[noreturn]] inline void unsup_err(string const &m) { throw unsup_exception("error: " + m); }
#define assert_st(x) do { if (!(x)) { ::bodahip::rt_err(string("assertion failed: " #x " at ") + __FILE__ + ":" + std::to_string(__LINE__)); } } while (0)

template <typename M> typename M::mapped_type &must_find(M &m, typename M::key_type const &k) {
  auto i = m.find(k); if (i == m.end()) { rt_err("missing key '" + string(k) + "'"); } return i->second; }
template <typename M> typename M::mapped_type const &must_find(M const &m, typename M::key_type const &k) {
  auto i = m.find(k); if (i == m.end()) { rt_err("missing key '" + string(k) + "'"); } return i->second; }
template <typename M, typename V> void must_insert(M &m, typename M::key_type const &k, V &&v) {
  if (!m.emplace(k, std::forward<V>(v)).second) { rt_err("duplicate key '" + string(k) + "'"); } }
template <typename M> void must_erase(M &m, typename M::key_type const &k) {
  if (!m.erase(k)) { rt_err("tried to erase missing key '" + string(k) + "'"); } }
inline bool startswith(string const &s, string const &p) { return s.size() >= p.size() && !s.compare(0, p.size(), p); }

// ---- dims_t -------------------------------------------------------------------------------------------------------
inline uint64_t tn_size(string const &tn) {
  if (tn == "none") return 0; if (tn == "half") return 2; if (tn == "bfloat16") return 2; if (tn == "float") return 4; if (tn == "double") return 8;
  if (tn == "int32_t") return 4; if (tn == "uint32_t") return 4; if (tn == "uint16_t") return 2; if (tn == "uint8_t") return 1;
  rt_err("unknown type name '" + tn + "'");
}
struct dim_t {
  uint32_t sz = 0, stride = 0; string name;
  bool operator==(dim_t const &o) const { return sz == o.sz && stride == o.stride && name == o.name; }
  bool operator<(dim_t const &o) const {
    if (sz != o.sz) return sz < o.sz; if (stride != o.stride) return stride < o.stride; return name < o.name; }
};
struct dims_t : public std::vector<dim_t> {
  string tn;                 // "float", "none", ...
  uint64_t strides_sz = 0;   // total element count (no padding support on this path)
  dims_t() {}
  dims_t(std::vector<uint32_t> const &szs, vect_string const &names_, string const &tn_) : tn(tn_) {
    assert_st(szs.size() == names_.size());
    for (size_t i = 0; i < szs.size(); ++i) { dim_t d; d.sz = szs[i]; d.name = names_[i]; push_back(d); }
    calc_strides();
  }
  void add_dims(string const &n, uint32_t sz) { dim_t d; d.sz = sz; d.name = n; push_back(d); }
  void calc_strides() { strides_sz = 1; for (size_t d = size(); d-- > 0;) { (*this)[d].stride = (uint32_t)strides_sz; strides_sz *= (*this)[d].sz; } }
  uint32_t sz() const { return (uint32_t)size(); }
  uint32_t dims(uint32_t i) const { return at(i).sz; }
  string const &names(uint32_t i) const { return at(i).name; }
  uint32_t strides(uint32_t i) const { return at(i).stride; }
  dim_t const *get_dim_by_name(string const &n) const { for (auto const &d : *this) { if (d.name == n) return &d; } return nullptr; }
  uint32_t dsz(string const &n) const { dim_t const *d = get_dim_by_name(n); if (!d) rt_err("dim not found:" + n); return d->sz; }
  uint32_t dstride(string const &n) const { dim_t const *d = get_dim_by_name(n); if (!d) rt_err("dim not found:" + n); return d->stride; }
  uint64_t dims_prod() const { uint64_t r = 1; for (auto const &d : *this) r *= d.sz; return r; }
  uint64_t tsz() const { return tn_size(tn); }
  uint64_t bytes_sz() const { return tsz() * strides_sz; }
  bool operator==(dims_t const &o) const { return tn == o.tn && static_cast<std::vector<dim_t> const &>(*this) == static_cast<std::vector<dim_t> const &>(o); }
  bool operator!=(dims_t const &o) const { return !(*this == o); }
  bool operator<(dims_t const &o) const {
    return (tn == o.tn) ? (static_cast<std::vector<dim_t> const &>(*this) < static_cast<std::vector<dim_t> const &>(o)) : (tn < o.tn); }
  string pretty_str() const { string r = "DIMS["; for (size_t i = 0; i < size(); ++i) { if (i) r += ":"; r += at(i).name + "=" + std::to_string(at(i).sz); } return r + "]"; }
};

// ---- nda_t --------------------------------------------------------------------------------------------------------
// dims + raw pointer.  Owning (host buffer, 32-byte aligned as the reference's, src/boda_base.H:784) or non-owning
// (e.g. get_var_raw_native_pointer(): dims + device pointer), or data-less (REF args: the information is the dims).
struct nda_t {
  dims_t dims;
  void *rp = nullptr;
  std::shared_ptr<void> owned;
  nda_t() {}
  explicit nda_t(dims_t const &d) : dims(d) {
    size_t const b = (size_t)d.bytes_sz();
    if (b) { void *p = nullptr; if (posix_memalign(&p, 32, (b + 31) & ~size_t(31))) rt_err("nda_t: host allocation failed"); memset(p, 0, b); owned.reset(p, free); rp = p; }
  }
  nda_t(dims_t const &d, void *rp_) : dims(d), rp(rp_) {}
  void *rp_elems() const { return rp; }
  uint64_t elems_sz() const { return dims.strides_sz; }
};
typedef std::shared_ptr<nda_t> p_nda_t;
typedef std::map<string, p_nda_t> map_str_p_nda_t;
inline p_nda_t make_dims_nda(dims_t const &d) { return std::make_shared<nda_t>(d, nullptr); }
template <typename T> inline char const *tn_of();
template <> inline char const *tn_of<float>() { return "float"; }
template <> inline char const *tn_of<uint32_t>() { return "uint32_t"; }
template <> inline char const *tn_of<int32_t>() { return "int32_t"; }
template <typename T> p_nda_t make_scalar_nda(T const &v) {
  dims_t d; d.tn = tn_of<T>(); d.calc_strides(); p_nda_t r = std::make_shared<nda_t>(d); *static_cast<T *>(r->rp) = v; return r; }

// ---- op_base_t ----------------------------------------------------------------------------------------------------
struct op_base_t {
  std::map<string, string> str_vals;
  map_str_p_nda_t nda_vals;
  bool has(string const &an) const { return nda_vals.count(an) != 0; }
  void set(string const &an, p_nda_t const &n) { must_insert(nda_vals, an, n); }
  void set_dims(string const &an, dims_t const &d) { set(an, make_dims_nda(d)); }
  p_nda_t const &get(string const &an) const { return must_find(nda_vals, an); }
  dims_t const &get_dims(string const &an) const { return get(an)->dims; }
  string const &get_str(string const &an) const { return must_find(str_vals, an); }
  uint32_t get_u32(string const &an) const {
    p_nda_t const &n = get(an); if (n->dims.tn != "uint32_t" || n->dims.sz() != 0 || !n->rp) rt_err("op: '" + an + "' is not a uint32_t scalar");
    return *static_cast<uint32_t const *>(n->rp); }
  void set_u32(string const &an, uint32_t v) { set(an, make_scalar_nda(v)); }
  bool has_type() const { return str_vals.count("type") != 0; }
  string const &get_type() const { return must_find(str_vals, "type"); }
  bool has_func_name() const { return str_vals.count("func_name") != 0; }
  string const &get_func_name() const { return must_find(str_vals, "func_name"); }
  void set_func_name(string const &f) { must_insert(str_vals, "func_name", f); }
};
typedef std::shared_ptr<op_base_t> p_op_base_t;
// ---- the op flags of a native function.  Which function takes which flag is a column of the one table, native_funcs.h (included at the end of this file), which defines:
enum func_family_t { kFamSgemm, kFamConv, kFamConvNhwc, kFamNhwcGrp, kFamNhwcMulti, kFamK1Chain, kFamFiltsKmajor, kFamBconv, kFamBckOp, kFamSgd, kFamBn, kFamBnc, kFamSolver, kFamEval, kFamData, kFamBnf, kFamLoss, kFamConvGrp, kFamDeconv };   // selects the handler
enum : unsigned { kFlagZinp = 1, kFlagSeedVar = 2, kFlagImgShards = 4, kFlagNhwcResidual = 8 };
struct op_flag_name_t { char const *name; unsigned flag; };
constexpr op_flag_name_t kOpFlagNames[] = {{"img_shards", kFlagImgShards}, {"seed_from_var", kFlagSeedVar}, {"zero_if_in_non_pos", kFlagZinp}, {"nhwc_residual", kFlagNhwcResidual}};
inline bool native_func_takes_flag(string const &fn, unsigned flag);   // (false for a name that is no row)
inline bool native_type_takes_flag(string const &t, unsigned flag);    // does a function of op type t take it
inline string native_funcs_taking_flag(unsigned flag);                 // "a, b and c", in table order
inline int native_func_member(string const &fn, func_family_t family);           // 0: no row of that family
inline char const *native_func_type(func_family_t family, int member);           // the row's (first) op type
inline string native_family_names(func_family_t family);                         // "a, b, c", in table order
inline bool op_flag_set(op_base_t const &op, unsigned flag) { for (auto const &f : kOpFlagNames) if (f.flag == flag) return op.has(f.name) && op.get_u32(f.name); return false; }
// every flag but nhwc_residual that the op carries and its function `fn` does not take is refused: "<flag>=1 on '<fn>': <what> takes no flag"
inline void refuse_flags_not_taken(op_base_t const &op, string const &fn, char const *what) {
  for (auto const &f : kOpFlagNames) if (f.flag != kFlagNhwcResidual && op_flag_set(op, f.flag) && !native_func_takes_flag(fn, f.flag)) rt_err(string(f.name) + "=1 on '" + fn + "': " + what + " takes no flag");
}
// zero_if_in_non_pos, a uint32 of a function op (absent: 0).  1: the function writes in_grad_loss[e] = in[e] > 0 ? g[e] : +0, g what it writes without the flag and `in` the
// op's forward input -- hip_zero_if_non_pos's rule on the producer's store.  Only the three functions whose in_grad_loss has the dims of `in` take it; hip_bconv_in and
// hip_spreading then take `in` as one more var arg, hip_bck_lrn reads it already
inline bool op_zinp_flag(op_base_t const &op) {
  if (!op_flag_set(op, kFlagZinp)) return false;
  string const fn = op.has_func_name() ? op.get_func_name() : string();
  if (!native_func_takes_flag(fn, kFlagZinp))
    rt_err("zero_if_in_non_pos=1 on '" + (fn.empty() ? op.get_type() : fn) + "': only " + native_funcs_taking_flag(kFlagZinp) + " write an in_grad_loss with the dims of their forward input in");
  if (!(op.get_dims("in") == op.get_dims("in_grad_loss"))) rt_err(fn + ": zero_if_in_non_pos=1 needs in and in_grad_loss of the same dims");
  return true;
}
// nhwc_residual, a uint32 of a plain hip_conv_nhwc function op (absent: 0).  1: the call takes one more var arg `res` (in front of out), a tensor of exactly out's dims
// and element type, and writes out = cvt( relu( (conv + bias) + float(res) ) ): a ResNet block's shortcut added in the convolution's epilogue, one rounding
// (kernels/conv_nhwc_bf16.hip -DRES=1).  Only the implicit-GEMM kernel of a plain call has that epilogue
inline bool op_nhwc_residual_flag(op_base_t const &op) {
  if (!op_flag_set(op, kFlagNhwcResidual)) return false;
  string const fn = op.has_func_name() ? op.get_func_name() : string();
  if (!native_func_takes_flag(fn, kFlagNhwcResidual)) unsup_err("nhwc_residual=1 on '" + (fn.empty() ? (op.has_type() ? op.get_type() : string("?")) : fn) + "': only a plain " + native_funcs_taking_flag(kFlagNhwcResidual) + " call has the residual epilogue (not a sibling group, a set or a multi-problem launch)");
  return true;
}
// seed_from_var, a uint32 of a hip_dropout function op (absent: 0).  1: the call takes one more var arg, det_drop_seed_var (uint32_t, one element), and hashes with
// seed = that word + the by-value det_drop_seed (wraps): the seed then lives in device memory, where a captured launch reads it anew at every replay
inline bool op_seed_var_flag(op_base_t const &op) {
  if (!op_flag_set(op, kFlagSeedVar)) return false;
  string const fn = op.has_func_name() ? op.get_func_name() : string();
  bool const bare_dropout = fn.empty() && op.has_type() && native_type_takes_flag(op.get_type(), kFlagSeedVar);   // (a bare Dropout / BckDropout)
  if (!native_func_takes_flag(fn, kFlagSeedVar) && !bare_dropout) rt_err("seed_from_var=1 on '" + (fn.empty() ? (op.has_type() ? op.get_type() : string("?")) : fn) + "': only " + native_funcs_taking_flag(kFlagSeedVar) + " takes a seed, and only it can read one from a var");
  return true;
}
// img_shards, a uint32 of a function op (absent: 0).  1: the call's img-leading vars may be shards of a batch, and the call leaves the bits of the WHOLE batch's call --
// the five functions that are not independent per image: hip_bconv_filts / hip_bconv_biases (a sum over the images), hip_sm_grad_and_loss (divides by the image
// count), hip_sum_loss_over_imgs (one chain over the images), hip_dropout (hashes the flat index in the whole tensor).  On one device (be=cpu, be=hip) there is one shard
// and the flagged call is the unflagged one; a multi-device backend runs it as csrc/hip_multi.cc describes.  No new var args
inline bool op_img_shards_flag(op_base_t const &op) {
  if (!op_flag_set(op, kFlagImgShards)) return false;
  string const fn = op.has_func_name() ? op.get_func_name() : string();
  if (!native_func_takes_flag(fn, kFlagImgShards))
    rt_err("img_shards=1 on '" + (fn.empty() ? (op.has_type() ? op.get_type() : string("?")) : fn) + "': only " + native_funcs_taking_flag(kFlagImgShards) + " take it (every other function is independent per image and runs on img shards as it is)");
  return true;
}
// the var bound to det_drop_seed_var: uint32_t, exactly one element, and not the tensor the call rewrites
inline void check_seed_var(string const &fn, string const &vn, dims_t const &d, string const &inout_vn) {
  if (vn == inout_vn) rt_err(fn + ": seed_from_var=1: 'det_drop_seed_var' and 'inout' are the same var '" + vn + "'");
  if (d.tn != "uint32_t" || d.dims_prod() != 1) rt_err(fn + ": seed_from_var=1: 'det_drop_seed_var' must be a uint32_t var with exactly one element, got '" + vn + "' " + d.tn + " " + d.pretty_str());
}

// ---- hip_sgd_update (op type SgdUpdate; this backend's own -- the reference has no solver): what both backends read from the function's op, and every refusal that needs
// the op alone
constexpr int kSgdUpdateMaxTens = 32;
struct sgd_op_t { std::vector<long> elems; std::vector<float> lr_mult, decay_mult; };   // per tensor: element count and the two multipliers
// hip_sgd_update: the op carries tens_num, per tensor the dims of w_i / g_i / h_i (float, identical) and the floats lr_mult_i / decay_mult_i, and hyper (float v=4)
inline sgd_op_t sgd_op_of_op(op_base_t const &op) {
  string const fn = "hip_sgd_update";
  if (op.get_type() != "SgdUpdate") rt_err(fn + ": a function of op type SgdUpdate, not " + op.get_type());
  refuse_flags_not_taken(op, fn, "the update");
  if (!op.has("tens_num")) rt_err(fn + ": the op has no 'tens_num'");
  uint32_t const n = op.get_u32("tens_num");
  if (n < 1 || n > (uint32_t)kSgdUpdateMaxTens) rt_err(fn + ": tens_num=" + std::to_string(n) + ": 1 to " + std::to_string(kSgdUpdateMaxTens) + " tensors");
  auto need = [&](string const &an) { if (!op.has(an)) rt_err(fn + ": the op has no '" + an + "'"); };
  need("hyper");
  dims_t const &hy = op.get_dims("hyper");
  if (hy.tn != "float" || hy.sz() != 1 || hy.names(0) != "v" || hy.dims(0) != 4) rt_err(fn + ": hyper must be float v=4 (lr, momentum, weight_decay, unused), got " + hy.tn + " " + hy.pretty_str());
  auto f32 = [&](string const &an) { p_nda_t const &v = op.get(an); if (v->dims.tn != "float" || v->dims.sz() != 0 || !v->rp) rt_err(fn + ": '" + an + "' is not a float scalar"); return *static_cast<float const *>(v->rp); };
  sgd_op_t r;
  for (uint32_t i = 0; i < n; ++i) {
    string const sx = "_" + std::to_string(i);
    for (char const *b : {"w", "g", "h", "lr_mult", "decay_mult"}) need(b + sx);
    dims_t const &w = op.get_dims("w" + sx);
    for (char const *b : {"w", "g", "h"}) {
      dims_t const &d = op.get_dims(b + sx);
      if (d.tn != "float") rt_err(fn + ": " + b + sx + " has type " + d.tn + ": the update is fp32 only");
      if (!(d == w)) rt_err(fn + ": " + b + sx + " dims " + d.pretty_str() + " differ from w" + sx + "'s " + w.pretty_str());
    }
    r.elems.push_back((long)w.dims_prod()); r.lr_mult.push_back(f32("lr_mult" + sx)); r.decay_mult.push_back(f32("decay_mult" + sx));
  }
  return r;
}

// ---- the solver family (this backend's own; kernels/solver_update_f32.hip states the chains): hip_solver_update (op type SolverUpdate, member 1), hip_grad_sumsq (GradSumsq,
// member 2), hip_grad_norm (GradNorm, member 3), and the two of gradient accumulation: hip_grad_accum (GradAccum, member 4: g_i read, a_i rewritten, accum float v=4 =
// [first, apply, scale, micro]) and hip_solver_update_acc (SolverUpdateAcc, member 5: the update's op plus accum).  What both backends read from the function's op, and
// every refusal that needs the op alone
constexpr long kSolverChunk = 4096;   // floats of one tensor a workgroup owns; one partial sum of squares per chunk
enum { kSolverSgd = 0, kSolverNesterov = 1, kSolverAdam = 2 };
inline constexpr char const *kSolverTypeNames[] = {"sgd", "nesterov", "adam"};
struct solver_op_t {
  int kind = 0;                          // the member: 1 update, 2 sumsq, 3 norm, 4 accum, 5 update_acc
  int type = kSolverSgd; bool clip = false, decoupled_wd = false;   // kinds 1, 5
  bool update() const { return kind == 1 || kind == 5; }
  std::vector<long> elems; std::vector<float> lr_mult, decay_mult;  // kinds 1, 2, 4, 5: per tensor (the multipliers: kinds 1, 5)
  uint32_t part0 = 0; long parts = 0;    // kind 2: the first partial this call writes; kinds 2, 3: the size of the partials var
  long chunks() const { long c = 0; for (long n : elems) c += (n + kSolverChunk - 1) / kSolverChunk; return c; }
};
inline solver_op_t solver_op_of_op(op_base_t const &op) {
  string const fn = op.get_func_name();
  solver_op_t r;
  r.kind = native_func_member(fn, kFamSolver);
  if (!r.kind) rt_err("'" + fn + "' is none of " + native_family_names(kFamSolver));
  string const type = native_func_type(kFamSolver, r.kind);
  if (op.get_type() != type) rt_err(fn + ": a function of op type " + type + ", not " + op.get_type());
  refuse_flags_not_taken(op, fn, "the solver");
  auto need = [&](string const &an) { if (!op.has(an)) rt_err(fn + ": the op has no '" + an + "'"); };
  auto vec = [&](string const &an, uint32_t v, char const *what) -> long {   // float v=<v> (v == 0: any length of at least 1)
    need(an); dims_t const &d = op.get_dims(an);
    if (d.tn != "float" || d.sz() != 1 || d.names(0) != "v" || (v ? d.dims(0) != v : d.dims(0) < 1)) rt_err(fn + ": " + an + " must be float v=" + (v ? std::to_string(v) : string("<partials>")) + " (" + what + "), got " + d.tn + " " + d.pretty_str());
    return (long)d.dims(0); };
  auto flag = [&](char const *an) { if (!op.has(an)) return false; uint32_t const v = op.get_u32(an); if (v > 1) rt_err(fn + ": " + an + " must be 0 | 1"); return v == 1; };
  auto f32 = [&](string const &an) { p_nda_t const &v = op.get(an); if (v->dims.tn != "float" || v->dims.sz() != 0 || !v->rp) rt_err(fn + ": '" + an + "' is not a float scalar"); return *static_cast<float const *>(v->rp); };
  if (r.kind == 3) {
    r.parts = vec("partials", 0, "one partial per chunk"); vec("hyper", 8, "lr, momentum, weight_decay, momentum2, delta, corr, clip_gradients, unused"); vec("state", 4, "coef, norm, sumsq, 0");
    if (4.0 * (double)r.parts >= 2147483648.0) unsup_err(fn + ": partials of 2 GiB or more");
    return r;
  }
  if (r.update()) {
    auto st = op.str_vals.find("solver_type");
    if (st == op.str_vals.end()) rt_err(fn + ": the op has no str_val 'solver_type' (sgd | nesterov | adam)");
    r.type = -1; for (int i = 0; i < 3; ++i) if (st->second == kSolverTypeNames[i]) r.type = i;
    if (r.type < 0) rt_err(fn + ": solver_type must be sgd | nesterov | adam, got '" + st->second + "'");
    r.clip = flag("clip"); r.decoupled_wd = flag("decoupled_wd");
    if (r.decoupled_wd && r.type != kSolverAdam) rt_err(fn + ": decoupled_wd=1 is adam's, not " + st->second + "'s");
  }
  if (!op.has("tens_num")) rt_err(fn + ": the op has no 'tens_num'");
  uint32_t const n = op.get_u32("tens_num");
  if (n < 1 || n > (uint32_t)kSgdUpdateMaxTens) rt_err(fn + ": tens_num=" + std::to_string(n) + ": 1 to " + std::to_string(kSgdUpdateMaxTens) + " tensors");
  if (r.update()) { vec("hyper", 8, "lr, momentum, weight_decay, momentum2, delta, corr, clip_gradients, unused"); vec("state", 4, "coef, norm, sumsq, 0"); }
  if (r.kind >= 4) vec("accum", 4, "first, apply, scale, micro");
  if (r.kind == 2) { r.parts = vec("partials", 0, "one partial per chunk"); need("part0"); r.part0 = op.get_u32("part0"); }
  for (uint32_t i = 0; i < n; ++i) {
    string const sx = "_" + std::to_string(i);
    std::vector<string> bases = r.update() ? std::vector<string>{"w", "g", "h"} : r.kind == 4 ? std::vector<string>{"g", "a"} : std::vector<string>{"g"};
    if (r.update() && r.type == kSolverAdam) bases.push_back("h2");
    for (string const &b : bases) need(b + sx);
    dims_t const &w = op.get_dims(bases[0] + sx);
    for (string const &b : bases) {
      dims_t const &d = op.get_dims(b + sx);
      if (d.tn != "float") rt_err(fn + ": " + b + sx + " has type " + d.tn + ": the solver is fp32 only");
      if (!(d == w)) rt_err(fn + ": " + b + sx + " dims " + d.pretty_str() + " differ from " + bases[0] + sx + "'s " + w.pretty_str());
    }
    r.elems.push_back((long)w.dims_prod());
    if (r.update()) { need("lr_mult" + sx); need("decay_mult" + sx); r.lr_mult.push_back(f32("lr_mult" + sx)); r.decay_mult.push_back(f32("decay_mult" + sx)); }
  }
  if (r.kind == 2 && (long)r.part0 + r.chunks() > r.parts)
    rt_err(fn + ": part0=" + std::to_string(r.part0) + " + " + std::to_string(r.chunks()) + " chunks exceed the " + std::to_string(r.parts) + " partials");
  return r;
}

// ---- the training BatchNorm functions and the Eltwise gradient (this backend's own; kernels/bn_f32.hip states the arithmetic): hip_bn_stats (op type BnStats),
// hip_bn_fwd (BnFwd), hip_bn_bck_sums (BnBckSums), hip_bn_bck_in (BnBckIn), hip_fan_out (FanOut).  What both backends read from the function's op, every refusal that
// needs the op alone, and the SLAB PLAN of the three per-channel sums: a function of the op alone, so that be=cpu and be=hip always cut at the same places
constexpr long kBnSlabUnit = 1024;     // a planned slab is a multiple of this (256 threads x one quad)
constexpr long kBnMinSlab = 4096;      // ... and never shorter than this: a short channel keeps one slab
constexpr long kBnTargetWgs = 512;     // two workgroups per CU on a fixed 256 CUs (not the device's count: the plan must not depend on the device)
constexpr long kBnMaxSlabs = 4096;     // per channel (only a forced slab length can ask for more)
constexpr int kFanOutMax = 8;
constexpr uint32_t kBncMaxChunks = 64;  // of a hip_bnc_stats / hip_bnc_bck_sums call
struct bn_op_t {
  int kind = 0;                  // 1 stats, 2 fwd, 3 bck_sums, 4 bck_in, 5 fan_out; the BatchNorm on its running pair (kFamBnf): 6 bnf_prep, 7 bnf_bck, 8 bnf_bck_in
  bool bnc = false;              // a hip_bnc_* function (kFamBnc): the sums in the chunked chain, the image count of the call's vars free where the function is per image
  uint32_t chunks = 0, forced = 0;   // bnc, kinds 1, 3: img chunks of the batch; the forced slab length every chunk's plan gets (0: the planner's)
  long B = 0, C = 0, HW = 0, N = 0;   // N = B * HW: the elements of one channel
  long Nglob = 0;                // > 0: the WHOLE batch's N where B / N are a chunk's or a shard's (fN, unb and the N == 1 case are global)
  long n_glob() const { return Nglob ? Nglob : N; }
  long elems = 0;                // of the whole tensor
  long slab = 0, nslabs = 0;     // kinds 1, 3, 7: elements of a slab of a channel's flat (img, pel) range, slabs per channel
  float eps = 0.f, maf = 0.f; uint32_t relu = 0; int nout = 0;
  vect_string tens, chans;       // the tensor args (dims of `in`) and the per-channel args (float chan=C), in the function's arg order
};
inline void bn_slab_plan(string const &fn, long C, long N, uint32_t forced, long &slab, long &nslabs) {
  if (forced) {
    if (forced % 4) rt_err(fn + ": slab=" + std::to_string(forced) + ": a forced slab length is a multiple of 4");
    slab = (long)forced;
  } else {
    long const want = std::max<long>(1, (kBnTargetWgs + C - 1) / C);
    slab = (N + want - 1) / want;
    slab = (slab + kBnSlabUnit - 1) / kBnSlabUnit * kBnSlabUnit;
    slab = std::max(slab, kBnMinSlab);
  }
  nslabs = std::max<long>(1, (N + slab - 1) / slab);
  if (nslabs > kBnMaxSlabs) unsup_err(fn + ": slab=" + std::to_string(slab) + " cuts a channel of " + std::to_string(N) + " elements into " + std::to_string(nslabs) + " slabs, more than " + std::to_string(kBnMaxSlabs));
}
// chunk i of `chunks` of a batch of T images holds images [T * i / chunks, T * (i + 1) / chunks), as csrc/hip_multi.cc cuts a batch over its devices
inline long bnc_chunk_begin(long T, uint32_t chunks, uint32_t i) { return (long)((uint64_t)T * i / chunks); }
// the op of a call whose vars hold n_img images of the op's batch (an img shard): the whole batch's N stays beside it
inline bn_op_t bn_op_on_imgs(bn_op_t const &b, long n_img) { bn_op_t c = b; c.Nglob = b.n_glob(); c.B = n_img; c.N = n_img * b.HW; c.elems = c.N * b.C; return c; }
// the op of ONE chunk of n_img images of a chunked call b: its own slab plan under the call's forced length, the whole batch's N beside it.  No images: no plan
inline bn_op_t bnc_op_of_imgs(string const &fn, bn_op_t const &b, long n_img) {
  bn_op_t c = bn_op_on_imgs(b, n_img); c.chunks = 1; c.slab = c.nslabs = 0;
  if (c.B) bn_slab_plan(fn, b.C, c.N, b.forced, c.slab, c.nslabs);
  return c;
}
inline bn_op_t bnc_chunk_op(string const &fn, bn_op_t const &b, uint32_t i) { return bnc_op_of_imgs(fn, b, bnc_chunk_begin(b.B, b.chunks, i + 1) - bnc_chunk_begin(b.B, b.chunks, i)); }
inline bn_op_t bn_op_of_op(op_base_t const &op) {
  string const fn = op.has_func_name() ? op.get_func_name() : string();
  bn_op_t r;
  r.kind = native_func_member(fn, kFamBn);
  if (!r.kind) { r.kind = native_func_member(fn, kFamBnc); r.bnc = r.kind != 0; }
  bool bnf = false;
  if (!r.kind) { r.kind = native_func_member(fn, kFamBnf); bnf = r.kind != 0; }
  if (!r.kind) rt_err("'" + fn + "' is none of " + native_family_names(kFamBn));
  string const type = native_func_type(r.bnc ? kFamBnc : bnf ? kFamBnf : kFamBn, r.kind);
  if (!op.has_type() || op.get_type() != type) rt_err(fn + ": a function of op type " + type + ", not " + (op.has_type() ? op.get_type() : string("?")));
  refuse_flags_not_taken(op, fn, "the function");
  auto f32 = [&](string const &an) { if (!op.has(an)) rt_err(fn + ": the op has no '" + an + "'"); p_nda_t const &v = op.get(an); if (v->dims.tn != "float" || v->dims.sz() != 0 || !v->rp) rt_err(fn + ": '" + an + "' is not a float scalar"); return *static_cast<float const *>(v->rp); };
  auto u32 = [&](string const &an) { if (!op.has(an)) rt_err(fn + ": the op has no '" + an + "'"); return op.get_u32(an); };
  switch (r.kind) {
  case 1: r.tens = {"in"}; r.chans = {"mean", "inv_std", "run_mean", "run_var"}; break;
  case 2: r.tens = {"in", "out"}; r.chans = {"mean", "inv_std", "scale", "bias"}; break;
  case 3: r.tens = {"in", "out_grad_loss"}; r.chans = {"mean", "inv_std", "scale_grad_loss", "bias_grad_loss"}; break;
  case 4: r.tens = {"in", "out_grad_loss", "in_grad_loss"}; r.chans = {"mean", "inv_std", "scale", "scale_grad_loss", "bias_grad_loss"}; break;
  // (kinds 6 and 8 bind no var to `in`: their op carries it for the dims alone, as every function op of this file does)
  case 6: r.chans = {"run_mean", "run_var", "mean", "inv_std"}; break;
  case 7: r.tens = {"in", "out_grad_loss", "in_grad_loss"}; r.chans = {"mean", "inv_std", "scale", "scale_grad_loss", "bias_grad_loss"}; break;
  case 8: r.tens = {"out_grad_loss", "in_grad_loss"}; r.chans = {"inv_std", "scale"}; break;
  default: {
    uint32_t const n = u32("outs_num");
    if (n < 2 || n > (uint32_t)kFanOutMax) unsup_err(fn + ": outs_num=" + std::to_string(n) + ": 2 to " + std::to_string(kFanOutMax) + " outputs");
    r.nout = (int)n; r.tens = {"in"};
    for (uint32_t i = 0; i < n; ++i) r.tens.push_back("outs_" + std::to_string(i));
  } }
  for (string const &an : r.tens) if (!op.has(an)) rt_err(fn + ": the op has no '" + an + "'");
  for (string const &an : r.chans) if (!op.has(an)) rt_err(fn + ": the op has no '" + an + "'");
  if (!op.has("in")) rt_err(fn + ": the op has no 'in'");
  dims_t const &in = op.get_dims("in");
  if (in.tn != "float") rt_err(fn + ": in has type " + in.tn + ": fp32 only");
  if (r.kind != 5 && !(in.sz() == 4 && in.names(0) == "img" && in.names(1) == "chan" && in.names(2) == "y" && in.names(3) == "x")) rt_err(fn + ": in must be img:chan:y:x, got " + in.pretty_str());
  for (string const &an : r.tens) if (!(op.get_dims(an) == in)) rt_err(fn + ": " + an + " dims " + op.get_dims(an).tn + " " + op.get_dims(an).pretty_str() + " differ from in's float " + in.pretty_str());
  r.elems = (long)in.dims_prod();
  if (r.elems < 1) rt_err(fn + ": empty in");
  if (4.0 * (double)in.dims_prod() >= 2147483648.0) unsup_err(fn + ": tensors of 2 GiB or more (32-bit element offsets)");
  if (r.kind == 5) return r;
  r.B = in.dims(0); r.C = in.dims(1); r.HW = (long)in.dims(2) * in.dims(3); r.N = r.B * r.HW;
  for (string const &an : r.chans) {
    dims_t const &d = op.get_dims(an);
    if (d.tn != "float" || d.sz() != 1 || d.names(0) != "chan" || (long)d.dims(0) != r.C) rt_err(fn + ": " + an + " dims " + d.tn + " " + d.pretty_str() + ": one float per channel of in " + in.pretty_str());
  }
  if (r.kind == 6) { r.eps = f32("eps"); if (!(r.eps >= 0.0f)) rt_err(fn + ": eps must not be negative"); }
  if (r.kind == 1) { r.eps = f32("eps"); r.maf = f32("maf"); if (!(r.eps >= 0.0f)) rt_err(fn + ": eps must not be negative"); }
  if (r.kind == 2) { r.relu = u32("relu"); if (r.relu > 1) rt_err(fn + ": relu must be 0 | 1"); }
  if (r.bnc && (r.kind == 1 || r.kind == 3)) {   // the chunked chain: every non-empty chunk gets the plan of its own dims, under the same forced length
    r.chunks = u32("chunks"); r.forced = u32("slab");
    if (r.chunks < 1 || r.chunks > kBncMaxChunks) unsup_err(fn + ": chunks=" + std::to_string(r.chunks) + ": 1 to " + std::to_string(kBncMaxChunks) + " img chunks");
    for (uint32_t i = 0; i < r.chunks; ++i) (void)bnc_chunk_op(fn, r, i);   // (refuses a forced slab that cuts a chunk's channel into too many)
    if (r.chunks == 1) { bn_op_t const cb = bnc_chunk_op(fn, r, 0); r.slab = cb.slab; r.nslabs = cb.nslabs; }   // (one chunk: the twin's chain and launches)
  } else if (r.kind == 1 || r.kind == 3 || r.kind == 7) bn_slab_plan(fn, r.C, r.N, u32("slab"), r.slab, r.nslabs);
  return r;
}
// the var-level refusals of a call, the same text on both backends: `vars` = the var bound to every tensor arg followed by every per-channel arg (bn_op_t's order)
inline void bn_check_aliases(string const &fn, bn_op_t const &b, vect_string const &vars) {
  vect_string args = b.tens; args.insert(args.end(), b.chans.begin(), b.chans.end());
  assert_st(args.size() == vars.size());
  auto same = [&](size_t i, size_t j) { return vars[i] == vars[j]; };
  for (size_t i = 0; i < args.size(); ++i) for (size_t j = i + 1; j < args.size(); ++j) {
    if (!same(i, j)) continue;
    bool ok = false;
    if (b.kind == 2 && i == 0 && j == 1) ok = true;                       // hip_bn_fwd: in and out may be one var
    if (b.kind == 4 && i == 1 && j == 2) ok = true;                       // hip_bn_bck_in: in_grad_loss may be out_grad_loss's var
    if (b.kind == 7 && i == 1 && j == 2) ok = true;                       // hip_bnf_bck likewise (the owning chain loads an element before it stores it)
    if (b.kind == 8 && i == 0 && j == 1) ok = true;                       // hip_bnf_bck_in likewise
    if (!ok) rt_err(fn + ": args '" + args[i] + "' and '" + args[j] + "' are the same var '" + vars[i] + "'");
  }
}

// ---- the eval family (this backend's own; kernels/eval_f32.hip states the rules): hip_accuracy (op type Accuracy, member 1: in float img:chan:1:1, label float img:1:1 read,
// rank uint32_t img written), hip_eval_accum (EvalAccum, member 2: rank uint32_t img, loss float y=1:x=1, ctl uint32_t v=4 read; counts uint32_t v=4, loss_sum float v=1
// rewritten; the uint32 top_k >= 1) and hip_bn_fold (BnFold, member 3: run_mean, run_var, scale, bias float chan=C read, a, b written; the float eps).  What both backends
// read from the function's op, and every refusal that needs the op alone
struct eval_op_t {
  int kind = 0;                  // the member: 1 accuracy, 2 accum, 3 bn_fold
  long B = 0, C = 0;             // kinds 1, 2: images; kinds 1, 3: channels
  uint32_t top_k = 0; float eps = 0.f;
  vect_string args;              // the var args in the function's arg order
};
inline eval_op_t eval_op_of_op(op_base_t const &op) {
  string const fn = op.has_func_name() ? op.get_func_name() : string();
  eval_op_t r;
  r.kind = native_func_member(fn, kFamEval);
  if (!r.kind) rt_err("'" + fn + "' is none of " + native_family_names(kFamEval));
  string const type = native_func_type(kFamEval, r.kind);
  if (!op.has_type() || op.get_type() != type) rt_err(fn + ": a function of op type " + type + ", not " + (op.has_type() ? op.get_type() : string("?")));
  refuse_flags_not_taken(op, fn, "the function");
  if (r.kind == 1) r.args = {"in", "label", "rank"}; else if (r.kind == 2) r.args = {"rank", "loss", "ctl", "counts", "loss_sum"}; else r.args = {"run_mean", "run_var", "scale", "bias", "a", "b"};
  for (string const &an : r.args) if (!op.has(an)) rt_err(fn + ": the op has no '" + an + "'");
  auto vec = [&](string const &an, char const *tn, char const *dn, long n, char const *what) {   // <tn> <dn>=<n> (n == 0: any length of at least 1)
    dims_t const &d = op.get_dims(an);
    if (d.tn != tn || d.sz() != 1 || d.names(0) != dn || (n ? (long)d.dims(0) != n : d.dims(0) < 1))
      rt_err(fn + ": " + an + " must be " + tn + " " + dn + "=" + (n ? std::to_string(n) : string("<n>")) + " (" + what + "), got " + d.tn + " " + d.pretty_str());
    return (long)d.dims(0); };
  if (r.kind == 1) {
    dims_t const &in = op.get_dims("in"), &lab = op.get_dims("label");
    if (in.tn != "float" || !(in.sz() == 4 && in.names(0) == "img" && in.names(1) == "chan" && in.names(2) == "y" && in.names(3) == "x")) rt_err(fn + ": in must be float img:chan:y:x, got " + in.tn + " " + in.pretty_str());
    if (in.dims(2) != 1 || in.dims(3) != 1 || lab.sz() != 3 || lab.names(0) != "img" || lab.dims(1) != 1 || lab.dims(2) != 1 || lab.dims(0) != in.dims(0))
      unsup_err(fn + ": only 1 x 1 planes (in img:chan:1:1, label img:1:1): the reference reads label by image");
    if (lab.tn != "float") rt_err(fn + ": label has type " + lab.tn + ": the loss's own var is float");
    r.B = in.dims(0); r.C = in.dims(1);
    if (r.B < 1 || r.C < 1) rt_err(fn + ": empty in");
    if (4.0 * (double)r.B * (double)r.C >= 2147483648.0) unsup_err(fn + ": tensors of 2 GiB or more (32-bit element offsets)");
    vec("rank", "uint32_t", "img", r.B, "one word per image");
  } else if (r.kind == 2) {
    r.B = vec("rank", "uint32_t", "img", 0, "one word per image");
    dims_t const &lo = op.get_dims("loss");
    if (lo.tn != "float" || lo.sz() != 2 || lo.names(0) != "y" || lo.names(1) != "x" || lo.dims(0) != 1 || lo.dims(1) != 1) rt_err(fn + ": loss must be float y=1:x=1 (the pipe's loss node), got " + lo.tn + " " + lo.pretty_str());
    vec("ctl", "uint32_t", "v", 4, "first, 0, 0, 0"); vec("counts", "uint32_t", "v", 4, "images, hits_top1, hits_topk, batches"); vec("loss_sum", "float", "v", 1, "the sum of the batches' losses");
    if (!op.has("top_k")) rt_err(fn + ": the op has no 'top_k'");
    r.top_k = op.get_u32("top_k");
    if (r.top_k < 1) rt_err(fn + ": top_k=0: top_k must be at least 1");
  } else {
    r.C = vec("run_mean", "float", "chan", 0, "one float per channel");
    for (string const &an : r.args) vec(an, "float", "chan", r.C, "one float per channel");
    if (!op.has("eps")) rt_err(fn + ": the op has no 'eps'");
    p_nda_t const &v = op.get("eps"); if (v->dims.tn != "float" || v->dims.sz() != 0 || !v->rp) rt_err(fn + ": 'eps' is not a float scalar");
    r.eps = *static_cast<float const *>(v->rp);
    if (!(r.eps >= 0.0f)) rt_err(fn + ": eps must not be negative");
  }
  return r;
}

// ---- the data family (this backend's own; kernels/data_f32.hip states the rule): hip_data_transform (op type DataTransform, member 1): src uint8_t img:y:x:chan
// (interleaved) or img:chan:y:x (planar) at the source size H x W, plan uint32_t img:v=4 = [y_off, x_off, mirror, unused] per image and mean float chan or chan:y:x (at
// the SOURCE size) read; out float img:chan:y:x at the crop size written; the float scale.  What both backends read from the function's op, and every refusal that needs
// the op alone
struct data_op_t {
  long B = 0, C = 0, H = 0, W = 0, ch = 0, cw = 0;   // images, channels, the source size, the crop size
  int chw = 0;                   // src's layout: 0 img:y:x:chan, 1 img:chan:y:x
  int mean_pel = 0;              // mean's form: 0 chan, 1 chan:y:x
  float scale = 0.f;
  vect_string args;              // the var args in the function's arg order
  long out_elems() const { return B * C * ch * cw; }
};
inline data_op_t data_op_of_op(op_base_t const &op) {
  string const fn = op.has_func_name() ? op.get_func_name() : string();
  data_op_t r;
  if (native_func_member(fn, kFamData) != 1) rt_err("'" + fn + "' is none of " + native_family_names(kFamData));
  string const type = native_func_type(kFamData, 1);
  if (!op.has_type() || op.get_type() != type) rt_err(fn + ": a function of op type " + type + ", not " + (op.has_type() ? op.get_type() : string("?")));
  refuse_flags_not_taken(op, fn, "the function");
  r.args = {"src", "plan", "mean", "out"};
  for (string const &an : r.args) if (!op.has(an)) rt_err(fn + ": the op has no '" + an + "'");
  auto named = [](dims_t const &d, std::initializer_list<char const *> ns) { if (d.sz() != ns.size()) return false; uint32_t i = 0; for (char const *n : ns) if (d.names(i++) != n) return false; return true; };
  dims_t const &src = op.get_dims("src"), &plan = op.get_dims("plan"), &mean = op.get_dims("mean"), &out = op.get_dims("out");
  bool const hwc = named(src, {"img", "y", "x", "chan"}), chw = named(src, {"img", "chan", "y", "x"});
  if (src.tn != "uint8_t" || !(hwc || chw)) rt_err(fn + ": src must be uint8_t img:y:x:chan or img:chan:y:x, got " + src.tn + " " + src.pretty_str());
  if (out.tn != "float" || !named(out, {"img", "chan", "y", "x"})) rt_err(fn + ": out must be float img:chan:y:x, got " + out.tn + " " + out.pretty_str());
  r.chw = chw ? 1 : 0;
  r.B = src.dims(0); r.C = chw ? src.dims(1) : src.dims(3); r.H = chw ? src.dims(2) : src.dims(1); r.W = chw ? src.dims(3) : src.dims(2);
  r.ch = out.dims(2); r.cw = out.dims(3);
  if ((long)out.dims(0) != r.B) rt_err(fn + ": out has " + std::to_string(out.dims(0)) + " images, src " + std::to_string(r.B));
  if ((long)out.dims(1) != r.C) rt_err(fn + ": out has chan=" + std::to_string(out.dims(1)) + ", src chan=" + std::to_string(r.C) + ": the transform keeps the channels");
  if (r.B < 1 || r.C < 1 || r.ch < 1 || r.cw < 1) rt_err(fn + ": empty out");
  if (r.ch > r.H || r.cw > r.W) rt_err(fn + ": the crop " + std::to_string(r.ch) + " x " + std::to_string(r.cw) + " is larger than the source " + std::to_string(r.H) + " x " + std::to_string(r.W));
  bool const m_chan = named(mean, {"chan"}) && (long)mean.dims(0) == r.C;
  bool const m_pel = named(mean, {"chan", "y", "x"}) && (long)mean.dims(0) == r.C && (long)mean.dims(1) == r.H && (long)mean.dims(2) == r.W;
  if (mean.tn != "float" || !(m_chan || m_pel))
    rt_err(fn + ": mean must be float chan=" + std::to_string(r.C) + " or chan=" + std::to_string(r.C) + ":y=" + std::to_string(r.H) + ":x=" + std::to_string(r.W) + " (the SOURCE size), got " + mean.tn + " " + mean.pretty_str());
  r.mean_pel = m_pel ? 1 : 0;
  if (plan.tn != "uint32_t" || !named(plan, {"img", "v"}) || (long)plan.dims(0) != r.B || plan.dims(1) != 4)
    rt_err(fn + ": plan must be uint32_t img=" + std::to_string(r.B) + ":v=4 (y_off, x_off, mirror, unused), got " + plan.tn + " " + plan.pretty_str());
  if ((double)r.B * r.C * r.H * r.W >= 2147483648.0 || 4.0 * (double)r.out_elems() >= 2147483648.0 || 4.0 * (double)r.C * r.H * r.W >= 2147483648.0)
    unsup_err(fn + ": tensors of 2 GiB or more");
  if (!op.has("scale")) rt_err(fn + ": the op has no 'scale'");
  p_nda_t const &v = op.get("scale"); if (v->dims.tn != "float" || v->dims.sz() != 0 || !v->rp) rt_err(fn + ": 'scale' is not a float scalar");
  r.scale = *static_cast<float const *>(v->rp);
  return r;
}

// ---- the loss family (this backend's own; kernels/loss_f32.hip states the rules): the full SoftmaxWithLoss a head with a LossSpec lowers to.  hip_softmax_loss_fwd
// (op type SoftmaxLossFwd, member 1: in float img:chan:y:x, label float img:y:x read; prob, loss_per_pel written), hip_loss_norm (LossNorm, member 2: label, loss_per_pel
// read; loss float y=1:x=1, loss_state float v=4 written) and hip_softmax_loss_bck (SoftmaxLossBck, member 3: prob, label, loss_state read; in_grad_loss written).  The
// spec rides in the op: the float weight, the str_val normalization (valid | full | batch_size | none), the uint32 has_ignore and the float ignore_label (the integer
// as a float, which is what a label is compared with).  What both backends read from the function's op, and every refusal that needs the op alone
struct loss_op_t {
  int kind = 0;                  // the member: 1 fwd, 2 norm, 3 bck
  long B = 0, C = 0, HW = 0;     // images, channels (kinds 1, 3), pels of a plane
  int has_ignore = 0; float ignore = 0.f;
  float weight = 1.f; int norm = 0;   // 0 valid | 1 full | 2 batch_size | 3 none
  vect_string args;              // the var args in the function's arg order
  long pels() const { return B * HW; }
};
inline constexpr char const *kLossNormNames[] = {"valid", "full", "batch_size", "none"};
inline loss_op_t loss_op_of_op(op_base_t const &op) {
  string const fn = op.has_func_name() ? op.get_func_name() : string();
  loss_op_t r;
  r.kind = native_func_member(fn, kFamLoss);
  if (!r.kind) rt_err("'" + fn + "' is none of " + native_family_names(kFamLoss));
  string const type = native_func_type(kFamLoss, r.kind);
  if (!op.has_type() || op.get_type() != type) rt_err(fn + ": a function of op type " + type + ", not " + (op.has_type() ? op.get_type() : string("?")));
  refuse_flags_not_taken(op, fn, "the function");
  if (r.kind == 1) r.args = {"in", "label", "prob", "loss_per_pel"}; else if (r.kind == 2) r.args = {"label", "loss_per_pel", "loss", "loss_state"}; else r.args = {"prob", "label", "loss_state", "in_grad_loss"};
  for (string const &an : r.args) if (!op.has(an)) rt_err(fn + ": the op has no '" + an + "'");
  auto named = [](dims_t const &d, std::initializer_list<char const *> ns) { if (d.sz() != ns.size()) return false; uint32_t i = 0; for (char const *n : ns) if (d.names(i++) != n) return false; return true; };
  dims_t const &lab = op.get_dims("label");
  if (lab.tn != "float" || !named(lab, {"img", "y", "x"})) rt_err(fn + ": label must be float img:y:x, got " + lab.tn + " " + lab.pretty_str());
  r.B = lab.dims(0); r.HW = (long)lab.dims(1) * lab.dims(2);
  if (r.B < 1 || r.HW < 1) rt_err(fn + ": empty label");
  if ((double)r.B * (double)r.HW >= 16777216.0) rt_err(fn + ": img * y * x = " + std::to_string(r.B * r.HW) + " pels: 2^24 or more, and the pel count must be exact as a float");
  auto tensor = [&](char const *an) {   // float img:chan:y:x over label's images and plane
    dims_t const &d = op.get_dims(an);
    if (d.tn != "float" || !named(d, {"img", "chan", "y", "x"})) rt_err(fn + ": " + an + " must be float img:chan:y:x, got " + d.tn + " " + d.pretty_str());
    if (d.dims(0) != lab.dims(0) || d.dims(2) != lab.dims(1) || d.dims(3) != lab.dims(2)) rt_err(fn + ": " + an + " " + d.pretty_str() + " and label " + lab.pretty_str() + " differ in img, y or x");
    if (d.dims(1) < 1) rt_err(fn + ": " + string(an) + " has no channels");
    if (4.0 * (double)d.dims_prod() >= 2147483648.0) unsup_err(fn + ": tensors of 2 GiB or more");
    return (long)d.dims(1); };
  auto same = [&](char const *an, dims_t const &want, char const *what) { dims_t const &d = op.get_dims(an); if (!(d == want)) rt_err(fn + ": " + an + " must be " + what + ", got " + d.tn + " " + d.pretty_str()); };
  auto state = [&]() { dims_t const &d = op.get_dims("loss_state"); if (d.tn != "float" || !named(d, {"v"}) || d.dims(0) != 4) rt_err(fn + ": loss_state must be float v=4 (Z, s, count, sum), got " + d.tn + " " + d.pretty_str()); };
  if (r.kind == 1) { r.C = tensor("in"); same("prob", op.get_dims("in"), "of in's dims"); same("loss_per_pel", lab, "of label's dims"); }
  else if (r.kind == 2) {
    same("loss_per_pel", lab, "of label's dims"); state();
    dims_t const &lo = op.get_dims("loss");
    if (lo.tn != "float" || !named(lo, {"y", "x"}) || lo.dims(0) != 1 || lo.dims(1) != 1) rt_err(fn + ": loss must be float y=1:x=1 (the pipe's loss node), got " + lo.tn + " " + lo.pretty_str());
  } else { r.C = tensor("prob"); same("in_grad_loss", op.get_dims("prob"), "of prob's dims"); state(); }
  auto f32 = [&](char const *an) { if (!op.has(an)) rt_err(fn + ": the op has no '" + an + "'"); p_nda_t const &v = op.get(an); if (v->dims.tn != "float" || v->dims.sz() != 0 || !v->rp) rt_err(fn + ": '" + an + "' is not a float scalar"); return *static_cast<float const *>(v->rp); };
  if (!op.has("has_ignore")) rt_err(fn + ": the op has no 'has_ignore'");
  r.has_ignore = op.get_u32("has_ignore") ? 1 : 0;
  r.ignore = f32("ignore_label");
  if (r.has_ignore && !(r.ignore == (float)(long)r.ignore)) rt_err(fn + ": ignore_label must be an integer");
  if (r.kind == 2) {
    r.weight = f32("weight");
    if (!(r.weight - r.weight == 0.0f)) rt_err(fn + ": weight must be finite");
    auto const it = op.str_vals.find("normalization");
    if (it == op.str_vals.end()) rt_err(fn + ": the op has no 'normalization'");
    r.norm = -1; for (int i = 0; i < 4; ++i) if (it->second == kLossNormNames[i]) r.norm = i;
    if (r.norm < 0) rt_err(fn + ": normalization must be valid | full | batch_size | none, got '" + it->second + "'");
  }
  return r;
}

// ---- rtc layer ----------------------------------------------------------------------------------------------------
struct rtc_compile_opts_t {
  uint32_t show_compile_log = 0, enable_lineinfo = 0, show_func_attrs = 0, show_rtc_calls = 0;
};
struct rtc_func_info_t {
  string func_name;      // name of the extern "C" kernel inside func_src; also the handle used by run()
  string func_src;       // CUCL-dialect source text
  vect_string arg_names; // kernel parameter order
  op_base_t op;          // the (annotated) op this function was generated for; op.func_name selects native kernels
};
typedef std::vector<rtc_func_info_t> vect_rtc_func_info_t;

struct rtc_compute_t;
// an argument is either the name of a var (device pointer is passed) or a value (raw bytes passed by value; a
// value with null data is a REF / optional argument: a null pointer is passed and only its dims carry information).
struct rtc_arg_t {
  string n; p_nda_t v;
  rtc_arg_t() {}
  rtc_arg_t(string const &n_) : n(n_) {}
  rtc_arg_t(char const *n_) : n(n_) {}
  rtc_arg_t(p_nda_t const &v_) : v(v_) {}
  bool is_valid() const { return bool(v) != (!n.empty()); }
  bool is_var() const { assert_st(is_valid()); return !n.empty(); }
  bool is_nda() const { assert_st(is_valid()); return bool(v); }
  string const &get_var() const { assert_st(is_var()); return n; }
  p_nda_t const &get_nda() const { assert_st(is_nda()); return v; }
  inline dims_t get_dims(rtc_compute_t &rtc) const;
};
typedef std::map<string, rtc_arg_t> map_str_rtc_arg_t;
struct rtc_func_call_t {
  string rtc_func_name;
  map_str_rtc_arg_t arg_map;
  uint32_t tpb = 0, blks = 0;
};

struct rtc_compute_t {
  string be;                                   // back-end id ("hip")
  uint32_t gen_src = 0;                        // if 1, dump generated sources / code objects before load
  string gen_src_output_dir = "rtc-gen-src";
  virtual ~rtc_compute_t() {}

  virtual void init() = 0;
  virtual string get_plat_tag() = 0;
  virtual void create_var_with_dims(string const &vn, dims_t const &dims) = 0;
  virtual void create_var_with_dims_as_reshaped_view_of_var(string const &vn, dims_t const &dims, string const &src_vn) = 0;
  virtual void release_var(string const &vn) = 0;
  virtual dims_t get_var_dims(string const &vn) = 0;
  virtual void set_var_to_zero(string const &vn) = 0;
  virtual void compile(vect_rtc_func_info_t const &func_infos, rtc_compile_opts_t const &opts) = 0;
  virtual void release_func(string const &func_name) = 0;
  virtual uint32_t run(rtc_func_call_t const &rfc) = 0;
  virtual void finish_and_sync() = 0;
  virtual void release_per_call_id_data() = 0;
  virtual void release_all_funcs() = 0;
  virtual float get_dur(uint32_t const &b, uint32_t const &e) = 0; // ms, start of call b to end of call e
  virtual void profile_start() = 0;
  virtual void profile_stop() = 0;
  virtual void copy_var_to_nda(p_nda_t const &nda, string const &vn) = 0;
  virtual p_nda_t get_var_raw_native_pointer(string const &vn) = 0;
  virtual void copy_nda_to_var(string const &vn, p_nda_t const &nda) = 0;

  // non-virtual conveniences layered on the above (src/rtc_compute.cc:43-97)
  void create_var_from_nda(p_nda_t const &nda, string const &vn) { create_var_with_dims(vn, nda->dims); copy_nda_to_var(vn, nda); }
  p_nda_t create_nda_from_var(string const &vn) { p_nda_t r = std::make_shared<nda_t>(get_var_dims(vn)); copy_var_to_nda(r, vn); return r; }
  void init_var_from_vect_float(string const &vn, std::vector<float> const &v) {
    p_nda_t nda = std::make_shared<nda_t>(dims_t({uint32_t(v.size())}, {"v"}, "float"), (void *)v.data());
    create_var_with_dims(vn, nda->dims); copy_nda_to_var(vn, nda); }
  void set_vect_float_from_var(std::vector<float> &v, string const &vn) {
    dims_t d = get_var_dims(vn); assert_st(d.sz() == 1); assert_st(v.size() == d.dims(0));
    copy_var_to_nda(std::make_shared<nda_t>(d, (void *)v.data()), vn); }
  void copy_ndas_to_vars(vect_string const &names, map_str_p_nda_t const &ndas) { for (auto const &n : names) copy_nda_to_var(n, must_find(ndas, n)); }
  void copy_vars_to_ndas(vect_string const &names, map_str_p_nda_t &ndas) {
    for (auto const &n : names) { auto i = ndas.find(n); if (i != ndas.end()) copy_var_to_nda(i->second, n); else ndas[n] = create_nda_from_var(n); } }
};
typedef std::shared_ptr<rtc_compute_t> p_rtc_compute_t;
inline dims_t rtc_arg_t::get_dims(rtc_compute_t &rtc) const { return is_nda() ? v->dims : rtc.get_var_dims(n); }

// shared-by-backends checks (src/rtc_compute.cc:21-41)
inline void rtc_launch_check_blks_and_tpb(string const &fn, uint64_t blks, uint64_t tpb) {
  if (!((blks > 0) && (tpb > 0))) {
    rt_err("boda/rtc: can't launch kernel; blks or tpb is zero: rtc_func_name=" + fn + " blks=" + std::to_string(blks) + " tpb=" +
           std::to_string(tpb) + "; perhaps is a culibs stub function that should not have been attempted to be run?"); }
}
inline void rtc_reshape_check(dims_t const &dims, dims_t const &src_dims) {
  if (dims.tn != src_dims.tn) rt_err("invalid reshape; types don't match: dims.tn=" + dims.tn + " src_vi.tn=" + src_dims.tn);
  if (dims.dims_prod() != src_dims.dims_prod())
    rt_err("invalid reshape; types match but sizes don't: dims.dims_prod()=" + std::to_string(dims.dims_prod()) +
           " src_dims.dims_prod()=" + std::to_string(src_dims.dims_prod()));
}

// op line text -> op_base_t (lexp grammar src/lexp.cc; nda text form src/nesi.cc:720-785).  lexp.cc
op_base_t parse_op_lexp(string const &s);
string op_to_str(op_base_t const &op);

// factory for the MI355X backend (hip_compute.cc)
p_rtc_compute_t make_hip_compute(int device_ordinal);
// factory for be=cpu, the host-cores backend behind the same contract (cpu_compute.cc; the CPU baseline of SURVEY.md section 8d)
p_rtc_compute_t make_cpu_compute();

} // namespace bodahip
#include "native_funcs.h"   // (the definitions of the native_func_* functions declared above)
