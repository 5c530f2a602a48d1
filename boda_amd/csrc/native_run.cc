// native_run.cc -- the rtc function interface of the native kernels: run() (argument checks, dispatch) and prebuild() / explain_plan (the same plans, ahead of time).
#include "native_internal.h"

namespace bodahip {

static conv_geom_t geom_from_dims(dims_t const &f, dims_t const &in, dims_t const &out, dims_t const &stride, dims_t const &in_pad, bool relu) {
  conv_geom_t g;
  g.B = in.dsz("img"); g.C = in.dsz("chan"); g.H = in.dsz("y"); g.W = in.dsz("x");
  g.OC = f.dsz("out_chan"); g.KH = f.dsz("y"); g.KW = f.dsz("x");
  g.SY = stride.dsz("y"); g.SX = stride.dsz("x"); g.PY = in_pad.dsz("y"); g.PX = in_pad.dsz("x");
  g.OH = out.dsz("y"); g.OW = out.dsz("x"); g.relu = relu;
  return g;
}

// Max pooling fused in front of a 1x1 convolution (annotation: uint32 nhwc_pool[<sfx>] = 1, REF-style dims pool_sz[<sfx>] / pool_pad[<sfx>] carried by the op): the
// function's `in` is the POOLING's input; the geometry handed to the patch kernel takes the pooling's window and padding (stride 1), the filters stay 1x1.
static bool apply_pool_window(op_base_t const &op, string const &sfx, conv_geom_t &g, char const *what) {
  if (!op.has("nhwc_pool" + sfx) || !op.get_u32("nhwc_pool" + sfx)) return false;
  dims_t const &ks = op.get_dims("pool_sz" + sfx), &pp = op.get_dims("pool_pad" + sfx);
  if (!(g.KH == 1 && g.KW == 1 && g.SY == 1 && g.SX == 1 && g.PY == 0 && g.PX == 0)) rt_err(string(what) + ": fused pooling needs a 1x1 / stride-1 / unpadded convolution");
  g.KH = (int)ks.dsz("y"); g.KW = (int)ks.dsz("x"); g.PY = (int)pp.dsz("y"); g.PX = (int)pp.dsz("x");
  if (g.KH * g.KW < 2 || g.KH * g.KW > 25) unsup_err(string(what) + ": fused pooling windows of 2..25 positions");
  return true;
}

// fp32 hip_conv with a max pooling fused in front (annotation: uint32 hip_pool = 1, dims pool_sz / pool_stride carried by the op; boda_amd/conv_pipe.py): `in` is the
// POOLING's input.  g arrives with H / W = that tensor's planes; they become the pooled plane.  Only windows that tile the plane exactly (no pooling pad, no clipped window).
static bool apply_f32_pool(op_base_t const &op, conv_geom_t &g, char const *what) {
  if (!op.has("hip_pool") || !op.get_u32("hip_pool")) return false;
  dims_t const &ks = op.get_dims("pool_sz"), &st = op.get_dims("pool_stride");
  g.PKH = (int)ks.dsz("y"); g.PKW = (int)ks.dsz("x"); g.PSY = (int)st.dsz("y"); g.PSX = (int)st.dsz("x"); g.UH = g.H; g.UW = g.W;
  if (g.PKH < 1 || g.PKW < 1 || g.PKH > 3 || g.PKW > 3 || g.PKH * g.PKW < 2 || g.PSY < 1 || g.PSX < 1 || g.UH < g.PKH || g.UW < g.PKW) unsup_err(string(what) + ": fused pooling takes windows of 2..9 positions, at most 3 x 3");
  if ((g.UH - g.PKH) % g.PSY || (g.UW - g.PKW) % g.PSX) unsup_err(string(what) + ": fused pooling needs windows that tile the plane exactly (no clipped last window)");
  g.H = (g.UH - g.PKH) / g.PSY + 1; g.W = (g.UW - g.PKW) / g.PSX + 1;
  return true;
}

// AOT: compile (into the on-disk code-object cache) the specialisation that run() would pick for `op`.  No device needed.
// With arch == "" nothing is compiled and *plan_out receives "<kernel> <tile> <-D options>": the planner's decision (host-logic tests).
// BckConv: the forward convolution's geometry from the op's in / filts / out_grad_loss / stride / in_pad (OP_INFO["BckConv"], boda_amd/op.py)
static void refuse_group(op_base_t const &op, string const &what) {   // every convolution function but the grouped family's three takes ungrouped ops only
  if (op_group(op) > 1) unsup_err(what + ": the op carries group=" + std::to_string(op_group(op)) + ": a grouped convolution runs as hip_conv_grp / hip_bconv_in_grp / hip_bconv_filts_grp (fp32, reference layouts) only");
}
// (any_group: the bias gradient, which knows no groups -- a grouped BckConv's hip_bconv_biases is the ungrouped function as it is)
static conv_geom_t bck_geom_of_op(op_base_t const &op, bool any_group = false) {
  if (!any_group) refuse_group(op, op.has_func_name() ? op.get_func_name() : op.get_type());
  conv_geom_t g = geom_from_dims(op.get_dims("filts"), op.get_dims("in"), op.get_dims("out_grad_loss"), op.get_dims("stride"), op.get_dims("in_pad"), false);
  if (op.get_dims("filts").dsz("in_chan") * op_group(op) != (uint32_t)g.C || op.get_dims("out_grad_loss").dsz("chan") != (uint32_t)g.OC || op.get_dims("out_grad_loss").dsz("img") != (uint32_t)g.B)
    rt_err("BckConv: in / filts / out_grad_loss dims are inconsistent");
  return g;
}

// The non-conv ops of the gradient pipe: a kernel's geometry from the op (OP_INFO of boda_amd/op.py: Pooling / Spreading carry in, out, kern_sz, stride, in_pad,
// avg_pool, emit_out_in_yx; LRN / BckLRN in, alpha, beta, k, local_size, emit_out_scale_base; ZeroIfNonPos in; SoftmaxWithLoss in, label).  The image count is the
// op's; run() replaces it with the vars'.
static float op_f32(op_base_t const &op, string const &an) {
  p_nda_t const &n = op.get(an);
  if (n->dims.tn != "float" || n->dims.sz() != 0 || !n->rp) rt_err("op: '" + an + "' is not a float scalar");
  return *static_cast<float const *>(n->rp);
}
static void need_nchw(dims_t const &d, string const &what) {
  if (!(d.sz() == 4 && d.names(0) == "img" && d.names(1) == "chan" && d.names(2) == "y" && d.names(3) == "x")) rt_err(what + " must be img:chan:y:x, got " + d.pretty_str());
}
static bck_op_geom_t bck_op_geom_of_op(op_base_t const &op, native_func_t const &f) {
  string const &t = op.get_type(); string const fn = f.name;
  if (!f.of_type(t)) rt_err(fn + ": a function of op type " + f.types[0] + ", not " + t);
  bck_op_geom_t g; g.op = f.member;
  if (g.op == 1 || g.op == 2) {
    dims_t const &in = op.get_dims("in"), &out = op.get_dims("out"), &ks = op.get_dims("kern_sz"), &st = op.get_dims("stride"), &pad = op.get_dims("in_pad");
    need_nchw(in, fn + ": in"); need_nchw(out, fn + ": out");
    if (out.dims(0) != in.dims(0) || out.dims(1) != in.dims(1)) rt_err(fn + ": out img / chan differ from in");
    g.B = in.dims(0); g.C = (int)in.dims(1); g.H = (int)in.dims(2); g.W = (int)in.dims(3); g.OH = (int)out.dims(2); g.OW = (int)out.dims(3);
    g.KH = (int)ks.dsz("y"); g.KW = (int)ks.dsz("x"); g.SY = (int)st.dsz("y"); g.SX = (int)st.dsz("x"); g.PY = (int)pad.dsz("y"); g.PX = (int)pad.dsz("x");
    g.avg = op.get_u32("avg_pool") ? 1 : 0;
    if (g.op == 1 && !op.get_u32("emit_out_in_yx") && !g.avg) unsup_err(fn + ": a Pooling with emit_out_in_yx=0 belongs to the forward pipe; hip_pool_yx is the pooling that also writes out_in_yx");
  } else if (g.op == 3 || g.op == 4) {
    dims_t const &in = op.get_dims("in"); need_nchw(in, fn + ": in");
    g.B = in.dims(0); g.C = (int)in.dims(1); g.H = (int)in.dims(2); g.W = (int)in.dims(3);
    g.LS = (int)op.get_u32("local_size"); g.alpha = op_f32(op, "alpha"); g.beta = op_f32(op, "beta"); g.k = op_f32(op, "k");
    if (g.op == 3 && !op.get_u32("emit_out_scale_base")) unsup_err(fn + ": an LRN with emit_out_scale_base=0 belongs to the forward pipe; hip_lrn_sb is the LRN that also writes out_scale_base");
  } else if (g.op == 5) {
    g.n = (long)op.get_dims("in").dims_prod();
  } else if (g.op == 9) {
    dims_t const &out = op.get_dims("out");
    g.nin = (int)op.get_u32("ins_num"); g.n = (long)out.dims_prod();
    for (string const &an : bck_op_args(f, op).ins) if (!(op.get_dims(an) == out)) rt_err(fn + ": " + an + " dims " + op.get_dims(an).pretty_str() + " differ from out's " + out.pretty_str());
  } else if (g.op == 13) {
    dims_t const &in = op.get_dims("in"), &out = op.get_dims("out"); need_nchw(in, fn + ": in");
    if (!(out == in)) rt_err(fn + ": out dims " + out.pretty_str() + " differ from in's " + in.pretty_str());
    for (char const *an : {"a", "b"}) {
      dims_t const &d1 = op.get_dims(an);
      if (d1.sz() != 1 || d1.dims(0) != in.dims(1) || d1.tn != "float") rt_err(fn + ": " + an + " dims " + d1.pretty_str() + ": one float per channel of in " + in.pretty_str());
    }
    g.B = in.dims(0); g.C = (int)in.dims(1); g.H = (int)in.dims(2); g.W = (int)in.dims(3); g.relu = (int)op.get_u32("relu");
    if (g.relu != 0 && g.relu != 1) rt_err(fn + ": relu must be 0 | 1");
  } else if (g.op == kOpCrop || g.op == kOpCropBck) {   // the plane is in's resp. in_grad_loss's, the window out's resp. out_grad_loss's, at the op's offset
    bool const fwd = g.op == kOpCrop;
    dims_t const &big = op.get_dims(fwd ? "in" : "in_grad_loss"), &win = op.get_dims(fwd ? "out" : "out_grad_loss"), &off = op.get_dims("offset");
    need_nchw(big, fn + (fwd ? ": in" : ": in_grad_loss")); need_nchw(win, fn + (fwd ? ": out" : ": out_grad_loss"));
    if (win.dims(0) != big.dims(0) || win.dims(1) != big.dims(1)) rt_err(fn + ": the window " + win.pretty_str() + " differs from the plane's tensor " + big.pretty_str() + " in img / chan");
    if (off.sz() != 2) rt_err(fn + ": offset must be y:x");
    g.B = big.dims(0); g.C = (int)big.dims(1); g.H = (int)big.dims(2); g.W = (int)big.dims(3); g.OH = (int)win.dims(2); g.OW = (int)win.dims(3);
    g.PY = (int)off.dsz("y"); g.PX = (int)off.dsz("x");
    if ((long)g.PY + g.OH > g.H || (long)g.PX + g.OW > g.W)
      rt_err(fn + ": offset (" + std::to_string(g.PY) + ", " + std::to_string(g.PX) + ") + window (" + std::to_string(g.OH) + ", " + std::to_string(g.OW) + ") exceeds the plane (" + std::to_string(g.H) + ", " + std::to_string(g.W) + ")");
  } else if (g.op == 10) {
    g.ratio = op_f32(op, "dropout_ratio"); g.n = (long)op.get_dims(op.has("inout") ? "inout" : "in").dims_prod();   // (the bare op carries in / out, its function the in-place arg inout)
  } else if (g.op == 11 || g.op == 12) {
    dims_t const &in = op.get_dims("in"), &out = op.get_dims("out"); need_nchw(in, fn + ": in"); need_nchw(out, fn + ": out");
    dims_t const &nar = (g.op == 11) ? in : out, &wid = (g.op == 11) ? out : in;
    if (nar.dims(0) != wid.dims(0) || nar.dims(2) != wid.dims(2) || nar.dims(3) != wid.dims(3)) rt_err(fn + ": in " + in.pretty_str() + " and out " + out.pretty_str() + " differ in img / y / x");
    g.B = nar.dims(0); g.C = (int)nar.dims(1); g.H = (int)nar.dims(2); g.W = (int)nar.dims(3); g.CT = (int)wid.dims(1); g.cix = (int)op.get_u32((g.op == 11) ? "ocix" : "icix");
  } else {
    dims_t const &in = op.get_dims("in"), &lab = op.get_dims("label"); need_nchw(in, fn + ": in");
    if (in.dims(2) != 1 || in.dims(3) != 1 || lab.sz() != 3 || lab.names(0) != "img" || lab.dims(1) != 1 || lab.dims(2) != 1 || lab.dims(0) != in.dims(0))
      unsup_err(fn + ": only 1 x 1 planes (in img:chan:1:1, label img:1:1): the reference reads label by image");
    g.B = in.dims(0); g.C = (int)in.dims(1);
  }
  return g;
}
static string bck_plan_desc(bck_plan_t const &bp) {
  string s = bp.p.kname + " grid=" + std::to_string(bp.grid) + " block=" + std::to_string(bp.block);
  for (size_t i = 1; i < bp.p.defs.size(); ++i) s += " " + bp.p.defs[i];
  return s;
}

size_t native_kernels_t::prebuild(op_base_t const &op, string const &arch, int num_cus, string const &tile_arg, string *plan_out) {
  string const &t = op.get_type();
  // a tile that travels with the function (str_val hip_tile: per-op tuned tiles, see tile_override_t) is what run() would use
  auto const ht = op.str_vals.find("hip_tile");
  string const tile = (tile_arg.empty() && ht != op.str_vals.end()) ? ht->second : tile_arg;
  plan_t p; string log, s2d;
  (void)op_zinp_flag(op);   // (refuses the flag on a function that cannot take it)
  (void)op_seed_var_flag(op);   // (likewise)
  (void)op_img_shards_flag(op);   // (likewise.  A flagged function plans as the unflagged one: the flag adds no define)
  bool const nhwc_res = op_nhwc_residual_flag(op);   // (likewise: a plain hip_conv_nhwc only)
  // the family: the function's row (native_funcs.h) where the op names one of its type's functions, else -- a bare op -- the family of the type's functions
  native_func_t const *f = op.has_func_name() ? find_native_func(op.get_func_name()) : nullptr;
  if (f && !f->of_type(t)) f = nullptr;
  std::vector<native_func_t const *> const of_t = native_funcs_of_type(t);
  if (!f && of_t.empty()) rt_err("prebuild: op type '" + t + "' has no native kernel");
  func_family_t const fam = f ? f->family : of_t[0]->family;
  int const member = f ? f->member : 0;   // (0: the bare op, or the family's plain form)
  bool const bf16 = (fam == kFamSgemm && member == 1) || (fam == kFamConv && member == kConvBf16);
  if (fam == kFamSgemm) {
    dims_t const &a = op.get_dims("a"), &b = op.get_dims("b");
    string const wide = (!bf16 && tile.empty() && a.tn != "half") ? sgemm_wide_tile(a.dsz("M"), b.dsz("N"), a.dsz("K"), num_cus) : string();
    sgemm_split_t sp; if (!bf16 && tile.empty() && a.tn != "half" && wide.empty()) sp = plan_sgemm_split(a.dsz("M"), b.dsz("N"), a.dsz("K"), num_cus);
    std::vector<sgemm_part_t> parts; if (!bf16 && tile.empty() && a.tn != "half") parts = plan_sgemm_parts(a.dsz("M"), b.dsz("N"), a.dsz("K"), num_cus);
    if (!parts.empty()) {   // guillotine decomposition: every part's plan is compiled, the last one reported in full
      s2d = "parts=" + std::to_string(parts.size());
      for (size_t i = 0; i < parts.size(); ++i) { sgemm_part_t const &q = parts[i];
        p = plan_sgemm(q.rows, q.cols, a.dsz("K"), num_cus, q.tile, false);
        s2d += " [" + std::to_string(q.m0) + "+" + std::to_string(q.rows) + "," + std::to_string(q.n0) + "+" + std::to_string(q.cols) + "]:" + p.cfg.str();
        if (i + 1 < parts.size() && !arch.empty()) compile_plan(p, arch, &log); }
      s2d += " last:";
    }
    else if (!wide.empty()) p = plan_sgemm(a.dsz("M"), b.dsz("N"), a.dsz("K"), num_cus, wide, false);
    else if (sp.m_main) {   // two-level tiling: the large tile over the first m_main rows (reported), small tiles over the rest
      plan_t const tp = plan_sgemm(a.dsz("M") - sp.m_main, b.dsz("N"), a.dsz("K"), num_cus, sp.tail_tile, false);
      p = plan_sgemm(sp.m_main, b.dsz("N"), a.dsz("K"), num_cus, kBigTile, false);
      s2d = "rows<" + std::to_string(sp.m_main) + ":" + p.cfg.str() + "+rest:";
      if (!arch.empty()) compile_plan(p, arch, &log);
      p = tp;
    } else p = plan_sgemm(a.dsz("M"), b.dsz("N"), a.dsz("K"), num_cus, tile, bf16);
    if (a.tn == "half") { s2d.clear(); p = plan_sgemm(a.dsz("M"), b.dsz("N"), a.dsz("K"), num_cus, tile, false, 1, false); p.kname = "bodahip_sgemm_f16s"; p.defs.push_back("-DHALF=1"); }
  }
  else if (fam <= kFamFiltsKmajor) {   // op type Convolution
    refuse_group(op, f ? string(f->name) : t);
    bool const relu = op.has("conv_has_relu") ? (op.get_u32("conv_has_relu") != 0) : true;
    bool const multi = fam == kFamNhwcMulti && member == 0;
    if (fam == kFamNhwcMulti && member == 1) {   // the wrapper kernel of the members' specialisations (and the kernels of members that stay alone)
      int const n = (int)op.get_dims("multi").dsz("n"); bool const out_f32 = op.get_dims(op.has("out_0") ? "out_0" : "out_0_0").tn == "float";
      std::vector<plan_t> plans; std::vector<double> costs; size_t bytes = 0; string desc;
      for (int m = 0; m < n; ++m) { string const sfx = "_" + std::to_string(m);
        bool const relu_m = op.has("relu_mask") ? (((op.get_u32("relu_mask") >> m) & 1u) != 0) : relu;   // (per member, fused members included)
        set_member_in_t mi; memset(&mi, 0, sizeof(mi));
        if (op.has("grp" + sfx)) {   // a horizontally fused member
          dims_t const &grp = op.get_dims("grp" + sfx);
          mi.g = geom_from_dims(op.get_dims("filts" + sfx), op.get_dims("in" + sfx), op.get_dims("out_0" + sfx), op.get_dims("stride" + sfx), op.get_dims("in_pad" + sfx), relu_m);
          mi.grp_pad = (int)grp.dims(grp.sz() - 1);
        } else {
          dims_t f = op.get_dims("filts" + sfx); mi.patch_filts = f.sz() == 5;
          if (mi.patch_filts) f = dims_t({f.dims(3), f.dims(1), f.dims(2), f.dims(0) * 8}, {"out_chan", "y", "x", "in_chan"}, f.tn);
          mi.g = geom_from_dims(f, op.get_dims("in" + sfx), op.get_dims("out" + sfx), op.get_dims("stride" + sfx), op.get_dims("in_pad" + sfx), relu_m);
          mi.pool = apply_pool_window(op, sfx, mi.g, "hip_conv_nhwc_set");
        }
        plans.push_back(plan_set_member(mi, num_cus, out_f32)); costs.push_back(set_tile_cost(mi, plans.back())); }
      set_layout_t const L = layout_set(plans, costs);   // (the ordering, variant numbering and lone-member rule of conv_nhwc_set)
      for (int m : L.alone) { plan_t const &q = plans[(size_t)m]; if (!arch.empty()) bytes += compile_plan(q, arch, &log).size(); desc += " alone:" + q.kname + ":" + q.cfg.str(); }
      for (plan_t const *q : L.variants) desc += " " + q->kname + ":" + q->cfg.str();
      if (plan_out) *plan_out = "bodahip_conv_nhwc_set variants=" + std::to_string(L.variants.size()) + desc;
      if (arch.empty()) return 0;
      if (L.variants.size() >= 1) bytes += hiprtc_compile(set_kernel_source(L.variants, 256, std::max(1, L.minw)), "bodahip_conv_nhwc_set", arch, vect_string(), &log, true, kernel_headers()).size();
      return bytes;
    }
    conv_geom_t g; memset(&g, 0, sizeof(g));
    if (!multi) g = geom_from_dims(op.get_dims("filts"), op.get_dims("in"), op.get_dims(op.has("out") ? "out" : "out_0"), op.get_dims("stride"), op.get_dims("in_pad"), relu);
    if (!multi) (void)apply_f32_pool(op, g, "prebuild");   // (hip_conv with a pooling fused in front: `in` is the pooling's input)
    conv_geom_t g2; int pry = 0, prx = 0;
    if (multi) {
      int const n = (int)op.get_dims("multi").dsz("n"); std::vector<conv_geom_t> gs;
      for (int m = 0; m < n; ++m) { string const sfx = "_" + std::to_string(m);
        gs.push_back(geom_from_dims(op.get_dims("filts" + sfx), op.get_dims("in" + sfx), op.get_dims("out" + sfx), op.get_dims("stride" + sfx), op.get_dims("in_pad" + sfx), relu)); }
      p = plan_conv_nhwc_multi(gs, tile, op.get_dims("out_0").tn == "float");
    }
    else if (fam == kFamConvNhwc && op.get_dims("filts").sz() == 5) {
      if (nhwc_res) unsup_err(string("hip_conv_nhwc: nhwc_residual=1 with ") + ((op.has("nhwc_pool") && op.get_u32("nhwc_pool")) ? "a max pooling fused in front (POOL): that form runs on the input-patch kernel, which has no residual epilogue" :
                              "the in_grp:y:x:out_chan:in_chan8 form of filts: the input-patch and rolling-rows kernels have no residual epilogue"));
      conv_geom_t gp = g; bool pool = false;
      if (op.has("nhwc_pool") && op.get_u32("nhwc_pool")) {   // (filts are in_grp:1:1:out_chan:8: geom_from_dims read in_grp / 1 as out_chan / y -- rebuild from the logical dims)
        dims_t const &f5 = op.get_dims("filts");
        dims_t const fl({f5.dims(3), f5.dims(1), f5.dims(2), f5.dims(0) * 8}, {"out_chan", "y", "x", "in_chan"}, f5.tn);
        gp = geom_from_dims(fl, op.get_dims("in"), op.get_dims("out"), op.get_dims("stride"), op.get_dims("in_pad"), relu);
        pool = apply_pool_window(op, string(), gp, "hip_conv_nhwc");
      }
      post_ops_t post; string why;
      if (apply_post_ops(op, gp, post, "prebuild")) { if (pool || !plan_conv_nhwc_rows(gp, post, num_cus, p, &why)) unsup_err("hip_conv_nhwc (rolling-rows form): " + (pool ? string("no pooling in front") : why)); }
      else if (!pool && op.get_dims("out").tn != "float" && rows_auto(gp, num_cus, tile)) plan_conv_nhwc_rows(gp, post_ops_t(), num_cus, p);
      else p = plan_conv_nhwc_patch(gp, num_cus, tile, op.get_dims("out").tn == "float", pool);
    }
    else if (fam == kFamK1Chain) {
      if (!plan_k1_chain(g, (int)op.get_dims("filts2").dsz("out_chan"), op.get_u32("conv_has_relu2") != 0, p)) unsup_err("prebuild: hip_conv_k1_chain does not cover this pair of convolutions");
    }
    else if (fam == kFamConvNhwc) {
      if (nhwc_res) {   // res: exactly out's dims and element type; the sum is defined on whole tensors
        if (!op.has("res")) rt_err("hip_conv_nhwc: nhwc_residual=1 without the arg 'res'");
        if (!(op.get_dims("res") == op.get_dims("out")) || op.get_dims("res").tn != op.get_dims("out").tn) rt_err("hip_conv_nhwc: nhwc_residual=1: res dims " + op.get_dims("res").pretty_str() + " (" + op.get_dims("res").tn + ") differ from out's " + op.get_dims("out").pretty_str() + " (" + op.get_dims("out").tn + ")");
      }
      p = plan_conv_nhwc(g, num_cus, tile, op.get_dims("out").tn == "float", 0, true, nhwc_res);
    }
    else if (fam == kFamNhwcGrp) { dims_t const &grp = op.get_dims("grp"); p = plan_conv_nhwc(g, num_cus, tile, op.get_dims("out_0").tn == "float", (int)grp.dims(grp.sz() - 1)); }
    else if (bf16 && tile.empty() && s2d_geom(g, g2, pry, prx) && plan_patch_bf16(g2, num_cus, p)) { // conv1-type layers: space-to-depth front end (see conv())
      s2d = "s2d(" + std::to_string(g2.C) + "x" + std::to_string(g2.H) + "x" + std::to_string(g2.W) + ",k" + std::to_string(g2.KH) + "x" + std::to_string(g2.KW) + ")+";
      if (!arch.empty()) { plan_t sp; sp.src = kSrc_conv_patch_bf16; sp.kname = "bodahip_s2d"; sp.defs = {"-DS2D_ONLY=1"}; compile_plan(sp, arch, &log); }
    } else {
      auto xe = op.str_vals.find("hip_exact"); bool const exact = !(xe != op.str_vals.end() && xe->second == "0");
      // the same resolution as conv(): in tolerance mode (and with no conv_algo / tile given) the 3x3 / stride-1 layers take the F(2x2,3x3) pipeline -- what is
      // compiled ahead of time and reported is then ITS kernels (the transforms' module and the batched transform-domain sgemm of every chunk size)
      if (!bf16 && !exact && tile.empty() && winograd_applies(g, "winograd")) {
        int const tpi = ((g.OH + 1) / 2) * ((g.OW + 1) / 2); long const Bc = wino_chunk_imgs(g);
        s2d = "winograd(F2x2,3x3)+";
        if (!arch.empty()) hiprtc_compile(kernel_source(kSrc_winograd_f32).text, "bodahip_winograd", arch, vect_string(), &log, true, kernel_headers());
        long const rem = g.B % Bc;
        if (rem) { plan_t const rp = plan_sgemm((uint32_t)g.OC, (uint32_t)(rem * tpi), (uint32_t)g.C, num_cus, string(), false, 16); if (!arch.empty()) compile_plan(rp, arch, &log); }
        p = plan_sgemm((uint32_t)g.OC, (uint32_t)(std::min<long>(Bc, g.B) * tpi), (uint32_t)g.C, num_cus, string(), false, 16);
      } else { char const *k1e = getenv("BODAHIP_K1_STREAM"); p = plan_conv(g, num_cus, tile, bf16, k1e ? string(k1e) : string(), true, exact); }   // (the env var a backend instance reads its k1_stream tune from)
    }
  } else if (fam == kFamBconv) {   // the three gradient functions (or, for the bare op, all three: the calls of src/rtc_fwd.cc:398-400)
    conv_geom_t const g = bck_geom_of_op(op, member == kBconvBiases);
    string const fn = op.has_func_name() ? op.get_func_name() : string();
    if (!fn.empty() && !f) rt_err("prebuild: BckConv function '" + fn + "' has no native kernel");
    std::vector<plan_t> ps;
    bool const b16 = op_bf16_operands(op);   // (refuses bf16 on hip_bconv_filts / hip_bconv_biases)
    if (!member || member == kBconvIn) ps.push_back(b16 ? plan_bconv_in_bf16(g, num_cus, tile, op_zinp_flag(op)) : plan_bconv_in(g, num_cus, tile, op_zinp_flag(op)));
    if (!member || member == kBconvBiases) ps.push_back(plan_bconv_biases());
    if (!member || member == kBconvFilts) ps.push_back(plan_bconv_filts(g, num_cus, tile));
    if (member == kBconvFiltsBiases) {   // (opt-in: never part of the bare op's three calls) the main kernel and, with K slices, the slab sum behind it
      ps.push_back(b16 ? plan_bconv_fb_bf16(g, num_cus, tile) : plan_bconv_filts_biases(g, num_cus, tile));
      if (ps.back().cfg.SPLITK > 1) ps.push_back(plan_bconv_slab_sum());
    }
    string desc; size_t bytes = 0;
    for (plan_t const &q : ps) {
      desc += (desc.empty() ? "" : " | ") + q.kname + (q.defs.size() > 1 ? " " + q.cfg.str() : string());
      if (q.bconv_in) desc += " grid=" + std::to_string((long)((g.C + q.cfg.BI - 1) / q.cfg.BI) * bconv_in_tiles(g, q.cfg.BJ)) + (q.defs.back() == "-DZINP=1" ? " -DZINP=1" : "");
      if (q.kname == "bodahip_bconv_filts" || q.kname == "bodahip_bconv_filts_biases" || q.kname == "bodahip_bconv_filts_biases_bf16") desc += " ksl=" + std::to_string(q.cfg.SPLITK);
      if (!arch.empty()) bytes += compile_plan(q, arch, &log).size();
    }
    if (op_img_shards_flag(op)) {   // a flagged filter / bias gradient on several devices also runs the sum of the per-device partials (csrc/hip_multi.cc): one kernel for every device count
      bck_plan_t const sp = plan_shard_sum(2, 4, 4);
      desc += " | " + sp.p.kname + " " + sp.p.defs[0];
      if (!arch.empty()) bytes += compile_plan(sp.p, arch, &log).size();
    }
    if (plan_out) *plan_out = desc;
    return bytes;
  } else if (fam == kFamConvGrp) {   // (kernels/conv_grp_f32.hip: one launch per call, specialised by the group's geometry)
    conv_grp_geom_t const cg = conv_grp_geom_of_op(op, member);
    plan_t const q = plan_conv_grp(cg, member, num_cus, tile);
    uint32_t grid = 0, block = 0; (void)conv_grp_threads(cg, member, q.cfg, &grid, &block);
    if (plan_out) { *plan_out = q.kname + " " + q.cfg.str() + " grid=" + std::to_string(grid); for (auto const &d : q.defs) *plan_out += " " + d; }
    if (conv_grp_has_slab_sum(q) && plan_out) *plan_out += " | bodahip_bconv_filts_grp_slab_sum";
    if (arch.empty()) return 0;
    size_t bytes = compile_plan(q, arch, &log).size();
    if (conv_grp_has_slab_sum(q)) bytes += compile_plan(plan_conv_grp_slab_sum(q), arch, &log).size();
    return bytes;
  } else if (fam == kFamDeconv) {   // (kernels/deconv_f32.hip: the direct forms, specialised by the geometry; a bare op: every function of its type)
    std::vector<int> members;
    if (member) members.push_back(member); else for (native_func_t const *r : of_t) members.push_back(r->member);
    size_t bytes = 0; string desc;
    for (int m : members) {
      deconv_geom_t const dg = deconv_geom_of_op(op, m);
      std::vector<plan_t> ps;
      string d1;
      if (m == kDeconvBckBiases) { ps.push_back(plan_bconv_biases()); d1 = ps[0].kname; }
      else {
        plan_t const q = plan_deconv(dg, m, num_cus, tile);
        uint32_t grid = 0; int zs = 1, per = 0; deconv_grid(dg, m, q.cfg, num_cus, &grid, &zs, &per);
        d1 = q.kname + " " + q.cfg.str() + " grid=" + std::to_string(grid); for (auto const &d : q.defs) d1 += " " + d;
        ps.push_back(q);
        if (deconv_has_slab_sum(q)) { ps.push_back(plan_deconv_slab_sum(q)); d1 += " | bodahip_deconv_bck_filts_slab_sum"; }
      }
      desc += (desc.empty() ? "" : " ; ") + d1;
      if (!arch.empty()) for (plan_t const &q : ps) bytes += compile_plan(q, arch, &log).size();
    }
    if (plan_out) *plan_out = desc;
    return bytes;
  } else if (fam == kFamSgd) {   // (hip_sgd_update: one kernel, no specialisation by shape; the grid is the sum of the tensors' chunks)
    sgd_plan_t const sp = plan_sgd_update(sgd_op_of_op(op).elems);
    if (plan_out) *plan_out = sp.p.kname + " grid=" + std::to_string(sp.grid) + " block=" + std::to_string(sp.block) + " tens=" + std::to_string(sp.blk0.size()) + " chunk=" + std::to_string(kSgdChunk);
    return arch.empty() ? 0 : compile_plan(sp.p, arch, &log).size();
  } else if (fam == kFamSolver) {   // (kernels/solver_update_f32.hip: one kernel per function; the update specialised by solver_type, clip and decoupled_wd, never by shape)
    if (!f) rt_err("prebuild: a bare " + t + " op: the solver's ops are function ops (cnn_op.solver_update_func_op, grad_sumsq_func_op, grad_norm_func_op, grad_accum_func_op, solver_update_acc_func_op)");
    solver_op_t const so = solver_op_of_op(op);
    sgd_plan_t const sp = plan_solver(so);
    if (plan_out) *plan_out = solver_plan_desc(so, sp);
    return arch.empty() ? 0 : compile_plan(sp.p, arch, &log).size();
  } else if (fam == kFamBn || fam == kFamBnc || fam == kFamBnf) {   // (kernels/bn_f32.hip: every launch of the call, and the slab plan)
    bn_op_t const b = bn_op_of_op(op);
    bn_plan_t const bp = plan_bn(b);
    if (plan_out) *plan_out = bn_plan_desc(b, bp);
    size_t bytes = 0;
    if (!arch.empty()) for (bn_launch_t const &l : bp.ls) bytes += compile_plan(l.p, arch, &log).size();
    return bytes;
  } else if (fam == kFamEval) {   // (kernels/eval_f32.hip: one kernel per function, never specialised by shape)
    if (!f) rt_err("prebuild: a bare " + t + " op: the eval pass's ops are function ops (cnn_op.accuracy_func_op, eval_accum_func_op, bn_fold_func_op)");
    eval_op_t const e = eval_op_of_op(op);
    bck_plan_t const bp = plan_eval_op(e);
    if (plan_out) *plan_out = eval_plan_desc(e, bp);
    return arch.empty() ? 0 : compile_plan(bp.p, arch, &log).size();
  } else if (fam == kFamData) {   // (kernels/data_f32.hip: specialised by src's layout and mean's form only)
    if (!f) rt_err("prebuild: a bare " + t + " op: the input transform's op is a function op (cnn_op.data_transform_func_op)");
    data_op_t const d = data_op_of_op(op);
    bck_plan_t const bp = plan_data_op(d);
    if (plan_out) *plan_out = data_plan_desc(d, bp);
    return arch.empty() ? 0 : compile_plan(bp.p, arch, &log).size();
  } else if (fam == kFamLoss) {   // (kernels/loss_f32.hip: the forward function specialised by its form and a small channel count, the others not at all)
    if (!f) rt_err("prebuild: a bare " + t + " op: the full softmax loss's ops are function ops (cnn_op.softmax_loss_fwd_func_op, loss_norm_func_op, softmax_loss_bck_func_op)");
    loss_op_t const l = loss_op_of_op(op);
    bck_plan_t const bp = plan_loss_op(l);
    if (plan_out) *plan_out = loss_plan_desc(l, bp);
    return arch.empty() ? 0 : compile_plan(bp.p, arch, &log).size();
  } else {   // kFamBckOp, a non-conv op of the gradient pipe: its annotated function, or (the bare op) all its functions in call order
    if (op.has_func_name() && !f) rt_err("prebuild: " + t + " function '" + op.get_func_name() + "' has no native kernel");
    std::vector<native_func_t const *> const ds = f ? std::vector<native_func_t const *>{f} : of_t;
    string desc; size_t bytes = 0;
    if (!op.has_func_name() && (t == "Concat" || t == "Split")) unsup_err("prebuild: a bare " + t + " is one call per " + (t == "Concat" ? "input" : "output") + ": annotate it (cnn_op.add_pipe_op_annotations) and pass the function ops");
    for (native_func_t const *d : ds) {
      bck_op_geom_t bg = bck_op_geom_of_op(op, *d); bg.zinp = op_zinp_flag(op) ? 1 : 0; bg.seedvar = op_seed_var_flag(op) ? 1 : 0;
      bck_plan_t const bp = plan_bck_op(bg, num_cus);
      desc += (desc.empty() ? "" : " | ") + bck_plan_desc(bp);
      if (!arch.empty()) bytes += compile_plan(bp.p, arch, &log).size();
    }
    if (plan_out) *plan_out = desc;
    return bytes;
  }
  if (plan_out) { *plan_out = s2d + p.kname + " " + p.cfg.str(); for (auto const &d : p.defs) *plan_out += " " + d;
    if (p.split_pels > 0) *plan_out += " pels<" + std::to_string(p.split_pels) + "+rest:" + p.tail_cfg.str(); }
  if (arch.empty()) return 0;
  size_t const n = compile_plan(p, arch, &log).size();
  if (p.cbig && p.split_pels > 0) { plan_t tp; tp.src = p.src; tp.kname = p.kname; tp.cfg = p.tail_cfg; tp.defs = p.tail_defs; compile_plan(tp, arch, &log); }
  if (p.cbig) { plan_t xp; xp.src = kSrc_conv_big_f32; xp.kname = "bodahip_conv_big_xpose"; xp.defs = {"-DXPOSE_ONLY=1"}; compile_plan(xp, arch, &log); }   // (the filter transposition that runs in front of it)
  if (p.patch16) { plan_t fp; fp.src = kSrc_conv_patch_bf16; fp.kname = "bodahip_filt_bf16"; fp.defs = {"-DFILT_ONLY=1"}; compile_plan(fp, arch, &log); }
  if (p.ksl) {   // (K slices reduced inside the launch: no second kernel)
  } else if (p.cfg.SPLITK > 1 && p.nhwc) {
    plan_t rp; rp.src = kSrc_conv_nhwc_bf16; rp.kname = "bodahip_nhwc_splitk_reduce";
    bool const relu = op.has("conv_has_relu") ? (op.get_u32("conv_has_relu") != 0) : true;
    rp.defs = {"-DREDUCE_ONLY=1", string("-DRELU=") + (relu ? "1" : "0"), string("-DOUT_F32=") + ((op.get_dims("out").tn == "float") ? "1" : "0")};
    compile_plan(rp, arch, &log);
  } else if (p.cfg.SPLITK > 1) { // the matching second-pass kernel
    plan_t r; r.kname = "bodahip_splitk_reduce"; bool const epi = (t == "Convolution");
    bool const relu = epi && (op.has("conv_has_relu") ? (op.get_u32("conv_has_relu") != 0) : true);
    r.defs = {"-DREDUCE_ONLY=1", string("-DRED_EPI=") + (epi ? "1" : "0"), string("-DRED_RELU=") + (relu ? "1" : "0")};
    compile_plan(r, arch, &log);
  }
  return n;
}


static string var_of(map_str_rtc_arg_t const &am, string const &an) {
  auto i = am.find(an);
  if (i == am.end()) rt_err("native hip function: arg '" + an + "' not found in arg_map for call.");
  if (!i->second.is_valid() || !i->second.is_var()) rt_err("native hip function: arg '" + an + "' must be a var");
  return i->second.n;
}
static void need_float(dims_t const &d, char const *an) {
  if (d.tn != "float") unsup_err(string("native hip kernels: arg '") + an + "' has type " + d.tn + "; only float storage is supported");
}

// a function may carry its own tile (str_val hip_tile of the annotated op: per-layer tuned tiles, the op_tune_t-per-op analogue of the
// reference's wisdom files); it overrides the backend-wide tune for that call only
struct tile_override_t {
  native_kernels_t::impl_t *impl; char const *key; bool active = false, had = false; string old;
  tile_override_t(native_kernels_t::impl_t *impl_, char const *key_, op_base_t const &op) : impl(impl_), key(key_) {
    auto it = op.str_vals.find("hip_tile");
    if (it == op.str_vals.end() || it->second.empty()) return;
    active = true; auto t = impl->tune.find(key); had = (t != impl->tune.end()); if (had) old = t->second;
    impl->tune[key] = it->second;
  }
  ~tile_override_t() { if (!active) return; if (had) impl->tune[key] = old; else impl->tune.erase(key); }
};

// str_val hip_exact of the annotated op (op_tune hip_exact=0): tolerance mode for this function's calls only
struct exact_override_t {
  native_kernels_t::impl_t *impl; bool active = false, had = false; string old;
  exact_override_t(native_kernels_t::impl_t *impl_, op_base_t const &op) : impl(impl_) {
    auto it = op.str_vals.find("hip_exact");
    if (it == op.str_vals.end() || it->second.empty()) return;
    if (it->second != "0" && it->second != "1") rt_err("hip_exact must be 0 | 1, got '" + it->second + "'");
    active = true; auto t = impl->tune.find("exact"); had = (t != impl->tune.end()); if (had) old = t->second;
    impl->tune["exact"] = it->second;
  }
  ~exact_override_t() { if (!active) return; if (had) impl->tune["exact"] = old; else impl->tune.erase("exact"); }
};

// one run(): what every family's handler reads, the check of a var against the op's dims, and the handlers.  They switch on the row's member, never on the name
struct native_kernels_t::call_t {
  native_kernels_t &nk; impl_t *impl; native_host_t *host;
  native_func_t const &row; rtc_func_info_t const &fi; map_str_rtc_arg_t const &am; string const &fn;
  bool zinp, seedvar, img_shards;
  long n_img = -1;   // of the call's img-leading vars, where the function leaves the image count free
  // the var bound to arg `an`, which must be float (fp32_only: the words of a function's own refusal) and have the dims the op gives the arg -- except, for a function that
  // runs on img shards (csrc/hip_multi.cc), the number of images, which only has to agree between the call's vars
  string var_of_op_dims(string const &an, char const *fp32_only = nullptr) {
    string const vn = var_of(am, an); dims_t const vd = host->nh_var_dims(vn);
    if (!fp32_only) need_float(vd, an.c_str());
    else if (vd.tn != "float") rt_err(fn + ": arg '" + an + "' (var '" + vn + "') has type " + vd.tn + ": " + fp32_only);
    dims_t want = fi.op.get_dims(an);
    if (row.img_count_free() && want.sz() >= 1 && want.names(0) == "img" && vd.sz() == want.sz()) {
      if (n_img < 0) n_img = vd.dims(0);
      if ((long)vd.dims(0) != n_img) rt_err(fn + ": arg '" + an + "' has " + std::to_string(vd.dims(0)) + " images, another arg " + std::to_string(n_img));
      want[0].sz = vd.dims(0); want.calc_strides();
    }
    if (!(vd == want)) rt_err(fn + ": arg '" + an + "' has dims " + vd.pretty_str() + ", the op says " + fi.op.get_dims(an).pretty_str());
    return vn;
  }
  void run_sgemm() {
    bool const bf16 = row.member == 1;
    string const an = var_of(am, "a"), bn = var_of(am, "b"), cn = var_of(am, "c");
    dims_t const a = host->nh_var_dims(an), b = host->nh_var_dims(bn), c = host->nh_var_dims(cn);
    // storage type: float, or all three `half` (16-bit storage, fp32 math: the reference's sgemm with __tn__=half dims, test/sgemm-ops-debug-half.txt)
    bool const half = (a.tn == "half" && b.tn == "half" && c.tn == "half");
    if (!half) { need_float(a, "a"); need_float(b, "b"); need_float(c, "c"); }
    uint32_t const M = a.dsz("M"), K = a.dsz("K"), N = b.dsz("N");
    // same consistency checks as culibs_wrap_t::sgemm (src/culibs-wrap.cc:218-225); a is K:M, b is K:N, c is M:N
    assert_st(a.sz() == 2 && b.sz() == 2 && c.sz() == 2);
    assert_st(a.names(0) == "K" && a.names(1) == "M" && b.names(0) == "K" && b.names(1) == "N" && c.names(0) == "M" && c.names(1) == "N");
    assert_st(b.dsz("K") == K); assert_st(c.dsz("M") == M); assert_st(c.dsz("N") == N);
    tile_override_t const tov(impl, "sgemm_tile", fi.op);
    nk.sgemm((float const *)host->nh_var_ptr(an), (float const *)host->nh_var_ptr(bn), (float *)host->nh_var_ptr(cn), M, N, K, bf16, half);
  }
  void run_nhwc_grp() {
    // horizontally fused channels-last convolutions: filts / biases stacked and padded (REF `grp`: dims m0..m{n-1} = the members' out_chans, pad = padding granularity),
    // outputs out_0 .. out_{n-1} (vars), optional by-value out_chan_off_<m> (member m writes a channel slice of a wider tensor)
    string const fnm = var_of(am, "filts"), bnm = var_of(am, "biases"), inm = var_of(am, "in");
    dims_t const f = host->nh_var_dims(fnm), bi = host->nh_var_dims(bnm), in = host->nh_var_dims(inm);
    need_float(bi, "biases");
    if (f.tn != "bfloat16" || in.tn != "bfloat16") unsup_err("hip_conv_nhwc_grp: filts / in must have type bfloat16");
    assert_st(f.sz() == 4 && in.sz() == 4 && bi.sz() == 1);
    if (!(f.names(0) == "out_chan" && f.names(1) == "y" && f.names(2) == "x" && f.names(3) == "in_chan")) rt_err("hip_conv_nhwc_grp: filts must be out_chan:y:x:in_chan, got " + f.pretty_str());
    auto si = am.find("stride"), pi = am.find("in_pad"), gi = am.find("grp");
    if (si == am.end() || pi == am.end() || gi == am.end()) rt_err("hip_conv_nhwc_grp: 'stride', 'in_pad' and 'grp' REF args are required");
    dims_t const stride = si->second.get_dims(host->nh_rtc()), in_pad = pi->second.get_dims(host->nh_rtc()), grp = gi->second.get_dims(host->nh_rtc());
    int const n = (int)grp.sz() - 1;
    if (n < 1 || n > 4 || grp.names(n) != "pad") rt_err("hip_conv_nhwc_grp: grp must be (m0=..,..,pad=..) with 1..4 members");
    int noc[4], ctot[4], coff[4]; void *outs[4]; bool out_f32 = false; dims_t out0;
    for (int m = 0; m < n; ++m) {
      string const onm = var_of(am, "out_" + std::to_string(m));
      dims_t const out = host->nh_var_dims(onm);
      if (out.tn != "bfloat16" && out.tn != "float") unsup_err("hip_conv_nhwc_grp: outputs must have type bfloat16 or float");
      if (!(out.sz() == 4 && out.names(0) == "img" && out.names(1) == "y" && out.names(2) == "x" && out.names(3) == "chan")) rt_err("hip_conv_nhwc_grp: outputs must be img:y:x:chan, got " + out.pretty_str());
      if (m == 0) { out0 = out; out_f32 = (out.tn == "float"); }
      else if (out.tn != out0.tn || out.dsz("img") != out0.dsz("img") || out.dsz("y") != out0.dsz("y") || out.dsz("x") != out0.dsz("x")) rt_err("hip_conv_nhwc_grp: the members' outputs must agree in type and map size");
      noc[m] = (int)grp.dims(m); ctot[m] = (int)out.dsz("chan"); coff[m] = 0; outs[m] = host->nh_var_ptr(onm);
      auto oi = am.find("out_chan_off_" + std::to_string(m));
      if (oi != am.end()) {
        if (oi->second.is_var() || !oi->second.v || !oi->second.v->rp_elems()) rt_err("hip_conv_nhwc_grp: out_chan_off_<m> must be a by-value uint32");
        coff[m] = (int)*(uint32_t const *)oi->second.v->rp_elems();
      } else if (ctot[m] != noc[m]) rt_err("hip_conv_nhwc_grp: member " + std::to_string(m) + " writes a wider tensor: out_chan_off_" + std::to_string(m) + " is required");
      if (coff[m] < 0 || coff[m] + noc[m] > ctot[m]) rt_err("hip_conv_nhwc_grp: out_chan_off + out_chans exceeds the channels of out_" + std::to_string(m));
    }
    conv_geom_t g = geom_from_dims(f, in, out0, stride, in_pad, fi.op.get_u32("conv_has_relu") != 0);
    if (f.dsz("in_chan") != (uint32_t)g.C || bi.dsz("out_chan") != (uint32_t)g.OC) rt_err("hip_conv_nhwc_grp: inconsistent filts / biases / in dims");
    if (!g.SY || !g.SX) rt_err("hip_conv_nhwc_grp: zero stride");
    if ((g.H + 2 * g.PY - g.KH) / g.SY + 1 != g.OH || (g.W + 2 * g.PX - g.KW) / g.SX + 1 != g.OW || out0.dsz("img") != (uint32_t)g.B) rt_err("hip_conv_nhwc_grp: out dims do not match in/filts/stride/in_pad");
    tile_override_t const tov(impl, "conv_tile", fi.op);
    nk.conv_nhwc_grp(host->nh_var_ptr(fnm), (float const *)host->nh_var_ptr(bnm), host->nh_var_ptr(inm), g, out_f32, n, noc, outs, ctot, coff, (int)grp.dims(n));
  }
  void run_nhwc_multi() {
    bool const is_set = row.member == 1;   // (a set's members keep their own specialised kernels -- implicit-GEMM or input-patch form, by the dims of their filts)
    // n independent channels-last convolutions (REF `multi`: dims n = the member count), member m: vars filts_<m> (out_chan:y:x:in_chan) biases_<m> in_<m> out_<m>,
    // REFs stride_<m> in_pad_<m>, optional by-value out_chan_off_<m>; ReLU: conv_has_relu for all, or bit m of the optional uint32 relu_mask
    auto mi = am.find("multi");
    if (mi == am.end()) rt_err("hip_conv_nhwc_multi: the REF arg 'multi' (dims n=<members>) is required");
    int const n = (int)mi->second.get_dims(host->nh_rtc()).dsz("n");
    if (n < 1 || n > 256) unsup_err("hip_conv_nhwc_multi: 1..256 members");
    bool const relu_all = fi.op.get_u32("conv_has_relu") != 0; bool const has_mask = fi.op.has("relu_mask"); uint32_t const mask = has_mask ? fi.op.get_u32("relu_mask") : 0u;
    if (has_mask && n > 32) unsup_err("hip_conv_nhwc_multi: relu_mask covers 32 members");
    std::vector<native_kernels_t::multi_member_t> ms((size_t)n); string out_tn; std::vector<char> patch_f((size_t)n, 0);
    for (int m = 0; m < n; ++m) {
      string const sfx = "_" + std::to_string(m);
      if (is_set && am.find("grp" + sfx) != am.end()) {   // a horizontally fused member (the args of hip_conv_nhwc_grp, every name with the member's suffix)
        string const fnm = var_of(am, "filts" + sfx), bnm = var_of(am, "biases" + sfx), inm = var_of(am, "in" + sfx);
        dims_t const f = host->nh_var_dims(fnm), bi = host->nh_var_dims(bnm), in = host->nh_var_dims(inm);
        need_float(bi, "biases");
        if (f.tn != "bfloat16" || in.tn != "bfloat16") unsup_err("hip_conv_nhwc_set: filts / in must have type bfloat16");
        if (!(f.sz() == 4 && f.names(0) == "out_chan" && f.names(3) == "in_chan" && in.sz() == 4)) rt_err("hip_conv_nhwc_set: a fused member's filts must be out_chan:y:x:in_chan");
        auto si = am.find("stride" + sfx), pi = am.find("in_pad" + sfx);
        if (si == am.end() || pi == am.end()) rt_err("hip_conv_nhwc_set: 'stride_<m>' and 'in_pad_<m>' REF args are required");
        dims_t const stride = si->second.get_dims(host->nh_rtc()), in_pad = pi->second.get_dims(host->nh_rtc()), grp = am.find("grp" + sfx)->second.get_dims(host->nh_rtc());
        int const gn = (int)grp.sz() - 1;
        if (gn < 1 || gn > 4 || grp.names(gn) != "pad") rt_err("hip_conv_nhwc_set: grp_<m> must be (m0=..,..,pad=..) with 1..4 members");
        native_kernels_t::multi_member_t &mm = ms[(size_t)m];
        mm.grp_n = gn; mm.grp_pad = (int)grp.dims(gn); dims_t out0;
        for (int j = 0; j < gn; ++j) {
          string const onm = var_of(am, "out_" + std::to_string(j) + sfx);
          dims_t const out = host->nh_var_dims(onm);
          if (out.tn != "bfloat16" && out.tn != "float") unsup_err("hip_conv_nhwc_set: outputs must have type bfloat16 or float");
          if (j == 0) out0 = out;
          if (m == 0 && j == 0) out_tn = out.tn; else if (out.tn != out_tn) rt_err("hip_conv_nhwc_set: the members' outputs must have one type");
          mm.grp_noc[j] = (int)grp.dims(j); mm.grp_ctot[j] = (int)out.dsz("chan"); mm.grp_coff[j] = 0; mm.grp_out[j] = host->nh_var_ptr(onm);
          auto oi = am.find("out_chan_off_" + std::to_string(j) + sfx);
          if (oi != am.end()) {
            if (oi->second.is_var() || !oi->second.v || !oi->second.v->rp_elems()) rt_err("hip_conv_nhwc_set: out_chan_off must be a by-value uint32");
            mm.grp_coff[j] = (int)*(uint32_t const *)oi->second.v->rp_elems();
          } else if (mm.grp_ctot[j] != mm.grp_noc[j]) rt_err("hip_conv_nhwc_set: a fused member writes a wider tensor: out_chan_off is required");
          if (mm.grp_coff[j] < 0 || mm.grp_coff[j] + mm.grp_noc[j] > mm.grp_ctot[j]) rt_err("hip_conv_nhwc_set: out_chan_off + out_chans exceeds the channels of the output");
        }
        mm.g = geom_from_dims(f, in, out0, stride, in_pad, has_mask ? ((mask >> m) & 1u) != 0 : relu_all);
        if (f.dsz("in_chan") != (uint32_t)mm.g.C || bi.dsz("out_chan") != (uint32_t)mm.g.OC) rt_err("hip_conv_nhwc_set: inconsistent filts / biases / in dims of a fused member");
        if (!mm.g.SY || !mm.g.SX || (mm.g.H + 2 * mm.g.PY - mm.g.KH) / mm.g.SY + 1 != mm.g.OH || (mm.g.W + 2 * mm.g.PX - mm.g.KW) / mm.g.SX + 1 != mm.g.OW) rt_err("hip_conv_nhwc_set: out dims of a fused member do not match");
        mm.filts = host->nh_var_ptr(fnm); mm.biases = (float const *)host->nh_var_ptr(bnm); mm.in = host->nh_var_ptr(inm); mm.out = nullptr; mm.out_ctot = 0; mm.out_coff = 0;
        continue;
      }
      string const fnm = var_of(am, "filts" + sfx), bnm = var_of(am, "biases" + sfx), inm = var_of(am, "in" + sfx), onm = var_of(am, "out" + sfx);
      dims_t f = host->nh_var_dims(fnm); dims_t const bi = host->nh_var_dims(bnm), in = host->nh_var_dims(inm), out = host->nh_var_dims(onm);
      if (is_set && f.sz() == 5) {   // the input-patch form F'[in_grp][ky][kx][out_chan][8]
        if (!(f.names(0) == "in_grp" && f.names(1) == "y" && f.names(2) == "x" && f.names(3) == "out_chan" && f.names(4) == "in_chan8" && f.dims(4) == 8)) rt_err("hip_conv_nhwc_set: 5-d filts must be in_grp:y:x:out_chan:in_chan8(=8), got " + f.pretty_str());
        f = dims_t({f.dims(3), f.dims(1), f.dims(2), f.dims(0) * 8}, {"out_chan", "y", "x", "in_chan"}, f.tn); patch_f[(size_t)m] = 1;
      }
      need_float(bi, "biases");
      if (f.tn != "bfloat16" || in.tn != "bfloat16") unsup_err("hip_conv_nhwc_multi: filts / in must have type bfloat16");
      if (out.tn != "bfloat16" && out.tn != "float") unsup_err("hip_conv_nhwc_multi: out must have type bfloat16 or float");
      if (m == 0) out_tn = out.tn; else if (out.tn != out_tn) rt_err("hip_conv_nhwc_multi: the members' outputs must have one type");
      assert_st(f.sz() == 4 && in.sz() == 4 && out.sz() == 4 && bi.sz() == 1);
      if (!(f.names(0) == "out_chan" && f.names(1) == "y" && f.names(2) == "x" && f.names(3) == "in_chan")) rt_err("hip_conv_nhwc_multi: filts must be out_chan:y:x:in_chan, got " + f.pretty_str());
      for (dims_t const *d : {&in, &out}) if (!(d->names(0) == "img" && d->names(1) == "y" && d->names(2) == "x" && d->names(3) == "chan")) rt_err("hip_conv_nhwc_multi: in / out must be img:y:x:chan, got " + d->pretty_str());
      auto si = am.find("stride" + sfx), pi = am.find("in_pad" + sfx);
      if (si == am.end() || pi == am.end()) rt_err("hip_conv_nhwc_multi: 'stride_<m>' and 'in_pad_<m>' REF args are required");
      dims_t const stride = si->second.get_dims(host->nh_rtc()), in_pad = pi->second.get_dims(host->nh_rtc());
      assert_st(stride.sz() == 2); assert_st(in_pad.sz() == 2);
      native_kernels_t::multi_member_t &mm = ms[(size_t)m];
      mm.g = geom_from_dims(f, in, out, stride, in_pad, has_mask ? ((mask >> m) & 1u) != 0 : relu_all);
      if (is_set) { mm.pool = apply_pool_window(fi.op, sfx, mm.g, "hip_conv_nhwc_set"); if (mm.pool && !patch_f[(size_t)m]) rt_err("hip_conv_nhwc_set: fused pooling needs the patch form of filts"); }
      conv_geom_t const &g = mm.g;
      if (f.dsz("in_chan") != (uint32_t)g.C) rt_err("hip_conv_nhwc_multi: filts.in_chan != in.chan (member " + std::to_string(m) + ")");
      mm.out_ctot = 0; mm.out_coff = 0;
      auto oi = am.find("out_chan_off" + sfx);
      if (oi != am.end()) {
        if (oi->second.is_var() || !oi->second.v || !oi->second.v->rp_elems()) rt_err("hip_conv_nhwc_multi: out_chan_off_<m> must be a by-value uint32");
        mm.out_coff = (int)*(uint32_t const *)oi->second.v->rp_elems(); mm.out_ctot = (int)out.dsz("chan");
        if (mm.out_coff < 0 || mm.out_coff + g.OC > mm.out_ctot) rt_err("hip_conv_nhwc_multi: out_chan_off + out_chan exceeds the channels of out");
      }
      if (bi.dsz("out_chan") != (uint32_t)g.OC || (!mm.out_ctot && out.dsz("chan") != (uint32_t)g.OC) || out.dsz("img") != (uint32_t)g.B) rt_err("hip_conv_nhwc_multi: inconsistent biases / out dims (member " + std::to_string(m) + ")");
      if (!g.SY || !g.SX) rt_err("hip_conv_nhwc_multi: zero stride");
      if ((g.H + 2 * g.PY - g.KH) / g.SY + 1 != g.OH || (g.W + 2 * g.PX - g.KW) / g.SX + 1 != g.OW) rt_err("hip_conv_nhwc_multi: out dims do not match in / filts / stride / in_pad (member " + std::to_string(m) + ")");
      mm.filts = host->nh_var_ptr(fnm); mm.biases = (float const *)host->nh_var_ptr(bnm); mm.in = host->nh_var_ptr(inm); mm.out = host->nh_var_ptr(onm);
    }
    if (is_set) {
      std::vector<char> pf(patch_f); bool pfb[16]; if (n > 16) unsup_err("hip_conv_nhwc_set: 1..16 members");
      for (int m = 0; m < n; ++m) pfb[m] = pf[(size_t)m] != 0;
      nk.conv_nhwc_set(n, ms.data(), pfb, out_tn == "float");
      return;
    }
    tile_override_t const tov(impl, "conv_tile", fi.op);
    nk.conv_nhwc_multi(n, ms.data(), out_tn == "float");
  }
  void run_conv_nhwc() {
    // channels-last bf16 tensors: filts out_chan:y:x:in_chan, in / out img:y:x:chan (out bf16 or float), biases float
    string const fnm = var_of(am, "filts"), bnm = var_of(am, "biases"), inm = var_of(am, "in"), onm = var_of(am, "out");
    dims_t f = host->nh_var_dims(fnm); dims_t const bi = host->nh_var_dims(bnm), in = host->nh_var_dims(inm), out = host->nh_var_dims(onm);
    need_float(bi, "biases");
    if (f.tn != "bfloat16" || in.tn != "bfloat16") unsup_err("hip_conv_nhwc: filts / in must have type bfloat16 (got " + f.tn + " / " + in.tn + ")");
    if (out.tn != "bfloat16" && out.tn != "float") unsup_err("hip_conv_nhwc: out must have type bfloat16 or float (got " + out.tn + ")");
    assert_st((f.sz() == 4 || f.sz() == 5) && in.sz() == 4 && out.sz() == 4 && bi.sz() == 1);
    // filts: out_chan:y:x:in_chan (implicit-GEMM kernel) or in_grp:y:x:out_chan:in_chan8 (LDS input-patch kernel; in_chan8 = 8): the layout the function was
    // annotated with decides the kernel
    bool const patch_filts = (f.sz() == 5);
    if (patch_filts) {
      if (!(f.names(0) == "in_grp" && f.names(1) == "y" && f.names(2) == "x" && f.names(3) == "out_chan" && f.names(4) == "in_chan8" && f.dims(4) == 8)) rt_err("hip_conv_nhwc: 5-d filts must be in_grp:y:x:out_chan:in_chan8(=8), got " + f.pretty_str());
      f = dims_t({f.dims(3), f.dims(1), f.dims(2), f.dims(0) * 8}, {"out_chan", "y", "x", "in_chan"}, f.tn);   // (the logical filter dims)
    }
    if (!(f.names(0) == "out_chan" && f.names(1) == "y" && f.names(2) == "x" && f.names(3) == "in_chan")) rt_err("hip_conv_nhwc: filts must be out_chan:y:x:in_chan, got " + f.pretty_str());
    for (dims_t const *d : {&in, &out}) if (!(d->names(0) == "img" && d->names(1) == "y" && d->names(2) == "x" && d->names(3) == "chan")) rt_err("hip_conv_nhwc: in / out must be img:y:x:chan, got " + d->pretty_str());
    auto si = am.find("stride"), pi = am.find("in_pad");
    if (si == am.end() || pi == am.end()) rt_err("hip_conv_nhwc: 'stride' and 'in_pad' REF args are required");
    dims_t const stride = si->second.get_dims(host->nh_rtc()), in_pad = pi->second.get_dims(host->nh_rtc());
    assert_st(stride.sz() == 2); assert_st(in_pad.sz() == 2);
    conv_geom_t g = geom_from_dims(f, in, out, stride, in_pad, fi.op.get_u32("conv_has_relu") != 0);
    if (f.dsz("in_chan") != (uint32_t)g.C) rt_err("hip_conv_nhwc: filts.in_chan != in.chan");
    bool const pool = apply_pool_window(fi.op, string(), g, "hip_conv_nhwc");
    if (pool && !patch_filts) rt_err("hip_conv_nhwc: fused pooling needs the in_grp:y:x:out_chan:in_chan8 form of filts");
    post_ops_t post; bool const has_post = apply_post_ops(fi.op, g, post, "hip_conv_nhwc");   // (out = the pooled tensor; g.OH x g.OW are the convolution's own planes from here on)
    if (has_post && (!patch_filts || pool || out.tn != "bfloat16")) rt_err("hip_conv_nhwc: a pooling fused behind the convolution needs the in_grp:y:x:out_chan:in_chan8 form of filts, a bfloat16 out and no pooling in front");
    int out_ctot = 0, out_coff = 0;
    auto oi = am.find("out_chan_off");
    if (oi != am.end()) {
      if (oi->second.is_var() || !oi->second.v || !oi->second.v->rp_elems()) rt_err("hip_conv_nhwc: out_chan_off must be a by-value uint32");
      out_coff = (int)*(uint32_t const *)oi->second.v->rp_elems(); out_ctot = (int)out.dsz("chan");
      if (out_coff < 0 || out_coff + g.OC > out_ctot) rt_err("hip_conv_nhwc: out_chan_off + out_chan exceeds the channels of out");
    }
    if (bi.dsz("out_chan") != (uint32_t)g.OC || (!out_ctot && out.dsz("chan") != (uint32_t)g.OC) || out.dsz("img") != (uint32_t)g.B) rt_err("hip_conv_nhwc: inconsistent biases/out dims");
    if (!g.SY || !g.SX) rt_err("hip_conv_nhwc: zero stride");
    if ((g.H + 2 * g.PY - g.KH) / g.SY + 1 != g.OH || (g.W + 2 * g.PX - g.KW) / g.SX + 1 != g.OW) rt_err("hip_conv_nhwc: out dims do not match in/filts/stride/in_pad");
    void const *res = nullptr;
    if (op_nhwc_residual_flag(fi.op)) {   // one more var arg: a tensor of exactly out's dims and element type, and not the tensor the call writes
      auto ri = am.find("res");
      if (ri == am.end() || !ri->second.is_valid() || !ri->second.is_var()) rt_err("hip_conv_nhwc: nhwc_residual=1: the var arg 'res' is required");
      dims_t const rd = host->nh_var_dims(ri->second.n);
      if (rd.tn != out.tn) rt_err("hip_conv_nhwc: nhwc_residual=1: res has type " + rd.tn + ", out " + out.tn + " (res must have out's element type)");
      if (!(rd == out)) rt_err("hip_conv_nhwc: nhwc_residual=1: res dims " + rd.pretty_str() + " differ from out's " + out.pretty_str());
      if (ri->second.n == onm) rt_err("hip_conv_nhwc: nhwc_residual=1: 'res' and 'out' are the same var '" + onm + "'");
      if (has_post) unsup_err("hip_conv_nhwc: nhwc_residual=1 with a pooling fused behind the convolution: the rolling-rows kernel has no residual epilogue");
      res = host->nh_var_ptr(ri->second.n);
    }
    if (has_post) {
      if ((int)out.dsz("y") != post.POH || (int)out.dsz("x") != post.POW) rt_err("hip_conv_nhwc: out dims do not match the fused pooling");
      nk.conv_nhwc_rows(host->nh_var_ptr(fnm), (float const *)host->nh_var_ptr(bnm), host->nh_var_ptr(inm), host->nh_var_ptr(onm), g, post, out_ctot, out_coff);
      return;
    }
    tile_override_t const tov(impl, "conv_tile", fi.op);
    nk.conv_nhwc(host->nh_var_ptr(fnm), (float const *)host->nh_var_ptr(bnm), host->nh_var_ptr(inm), host->nh_var_ptr(onm), g, out.tn == "float", out_ctot, out_coff, patch_filts, pool, res);
  }
  void run_k1_chain() {
    // two chained 1x1 convolutions (see conv_k1_chain): vars filts / biases (first conv), filts2 / biases2 (second), in, out, optionally mid (the first conv's output,
    // written as well); REFs stride / in_pad (of both: 1x1 / stride 1 / no padding); uint32 conv_has_relu / conv_has_relu2; optional by-value out_chan_off
    string const fnm = var_of(am, "filts"), bnm = var_of(am, "biases"), f2nm = var_of(am, "filts2"), b2nm = var_of(am, "biases2"), inm = var_of(am, "in"), onm = var_of(am, "out");
    dims_t const f = host->nh_var_dims(fnm), bi = host->nh_var_dims(bnm), f2 = host->nh_var_dims(f2nm), b2 = host->nh_var_dims(b2nm), in = host->nh_var_dims(inm), out = host->nh_var_dims(onm);
    need_float(f, "filts"); need_float(bi, "biases"); need_float(f2, "filts2"); need_float(b2, "biases2"); need_float(in, "in"); need_float(out, "out");
    auto si = am.find("stride"), pi = am.find("in_pad");
    if (si == am.end() || pi == am.end()) rt_err("hip_conv_k1_chain: 'stride' and 'in_pad' REF args are required");
    dims_t const stride = si->second.get_dims(host->nh_rtc()), in_pad = pi->second.get_dims(host->nh_rtc());
    assert_st(stride.sz() == 2); assert_st(in_pad.sz() == 2);
    assert_st(f.sz() == 4 && f2.sz() == 4 && in.sz() == 4 && out.sz() == 4 && bi.sz() == 1 && b2.sz() == 1);
    conv_geom_t g = geom_from_dims(f, in, out, stride, in_pad, fi.op.get_u32("conv_has_relu") != 0);
    bool const relu2 = fi.op.get_u32("conv_has_relu2") != 0;
    int const oc2 = (int)f2.dsz("out_chan");
    if (f.dsz("in_chan") != (uint32_t)g.C || f2.dsz("in_chan") != (uint32_t)g.OC) rt_err("hip_conv_k1_chain: filts.in_chan != in.chan or filts2.in_chan != filts.out_chan");
    if (f2.dsz("y") != 1 || f2.dsz("x") != 1 || g.KH != 1 || g.KW != 1 || g.SY != 1 || g.SX != 1 || g.PY || g.PX) unsup_err("hip_conv_k1_chain: both convolutions must be 1x1 / stride 1 / unpadded");
    int out_ctot = 0, out_coff = 0;
    auto oi = am.find("out_chan_off");
    if (oi != am.end()) {
      if (oi->second.is_var() || !oi->second.v || !oi->second.v->rp_elems()) rt_err("hip_conv_k1_chain: out_chan_off must be a by-value uint32");
      out_coff = (int)*(uint32_t const *)oi->second.v->rp_elems(); out_ctot = (int)out.dsz("chan");
      if (out_coff < 0 || out_coff + oc2 > out_ctot) rt_err("hip_conv_k1_chain: out_chan_off + out_chan exceeds the channels of out");
    }
    if (bi.dsz("out_chan") != (uint32_t)g.OC || b2.dsz("out_chan") != (uint32_t)oc2 || (!out_ctot && out.dsz("chan") != (uint32_t)oc2) || out.dsz("img") != (uint32_t)g.B) rt_err("hip_conv_k1_chain: inconsistent biases / out dims");
    if (g.OH != g.H || g.OW != g.W) rt_err("hip_conv_k1_chain: out dims do not match in");
    float *mid = nullptr;
    auto mi = am.find("mid");
    if (mi != am.end()) {
      string const mnm = var_of(am, "mid"); dims_t const md = host->nh_var_dims(mnm); need_float(md, "mid");
      if (md.sz() != 4 || md.dsz("img") != (uint32_t)g.B || md.dsz("chan") != (uint32_t)g.OC || md.dsz("y") != (uint32_t)g.OH || md.dsz("x") != (uint32_t)g.OW) rt_err("hip_conv_k1_chain: mid must be img:chan:y:x of the first convolution's output");
      mid = (float *)host->nh_var_ptr(mnm);
    }
    nk.conv_k1_chain((float const *)host->nh_var_ptr(fnm), (float const *)host->nh_var_ptr(bnm), (float const *)host->nh_var_ptr(f2nm), (float const *)host->nh_var_ptr(b2nm),
                  (float const *)host->nh_var_ptr(inm), (float *)host->nh_var_ptr(onm), mid, g, oc2, relu2, out_ctot, out_coff);
  }
  void run_conv() {
    bool const bf16 = row.member == kConvBf16;
    refuse_group(fi.op, fn);
    string const fnm = var_of(am, "filts"), bnm = var_of(am, "biases"), inm = var_of(am, "in"), onm = var_of(am, "out");
    dims_t const f = host->nh_var_dims(fnm), bi = host->nh_var_dims(bnm), in = host->nh_var_dims(inm), out = host->nh_var_dims(onm);
    need_float(f, "filts"); need_float(bi, "biases"); need_float(in, "in"); need_float(out, "out");
    auto si = am.find("stride"), pi = am.find("in_pad");
    if (si == am.end() || pi == am.end()) rt_err("hip_conv: 'stride' and 'in_pad' REF args are required");
    dims_t const stride = si->second.get_dims(host->nh_rtc()), in_pad = pi->second.get_dims(host->nh_rtc());
    assert_st(stride.sz() == 2); assert_st(in_pad.sz() == 2);
    assert_st(f.sz() == 4 && in.sz() == 4 && out.sz() == 4 && bi.sz() == 1);
    conv_geom_t g = geom_from_dims(f, in, out, stride, in_pad, fi.op.get_u32("conv_has_relu") != 0);
    if (f.dsz("in_chan") != (uint32_t)g.C) rt_err("hip_conv: filts.in_chan != in.chan");
    if (apply_f32_pool(fi.op, g, "hip_conv") && row.member != kConvF32) unsup_err("fused pooling (hip_pool): the fp32 hip_conv function only");
    // optional by-value arg out_chan_off: `out` is then a wider tensor (an inception module's Concat output) and this conv writes
    // channels [out_chan_off, out_chan_off + out_chan) of it -- the channel-offset copy of src/rtc_fwd.cc:267-280 folded into the store
    int out_ctot = 0, out_coff = 0;
    auto oi = am.find("out_chan_off");
    if (oi != am.end()) {
      if (oi->second.is_var() || !oi->second.v || !oi->second.v->rp_elems()) rt_err("hip_conv: out_chan_off must be a by-value uint32");
      out_coff = (int)*(uint32_t const *)oi->second.v->rp_elems(); out_ctot = (int)out.dsz("chan");
      if (out_coff < 0 || out_coff + g.OC > out_ctot) rt_err("hip_conv: out_chan_off + out_chan exceeds the channels of out");
    }
    if (bi.dsz("out_chan") != (uint32_t)g.OC || (!out_ctot && out.dsz("chan") != (uint32_t)g.OC) || out.dsz("img") != (uint32_t)g.B) rt_err("hip_conv: inconsistent biases/out dims");
    if (!g.SY || !g.SX) rt_err("hip_conv: zero stride");
    // out = (in + 2*pad - k)/stride + 1, floor (src/conv_util.cc:167-173)
    if ((g.H + 2 * g.PY - g.KH) / g.SY + 1 != g.OH || (g.W + 2 * g.PX - g.KW) / g.SX + 1 != g.OW) rt_err("hip_conv: out dims do not match in/filts/stride/in_pad");
    // optional var arg filts_km (round 6): the k-major copy of filts that hip_conv_filts_kmajor wrote -- [K + 128][out_chan padded to 4], zero rows behind K.  A plan that
    // reads its filters k-major (the staging-wave kernel) then skips the transposition it would run in front of every call; every other plan ignores it
    float const *km = nullptr;
    auto ki = am.find("filts_km");
    if (ki != am.end() && row.member == kConvF32) {
      if (!ki->second.is_var()) rt_err("hip_conv: filts_km must be a var");
      dims_t const kd = host->nh_var_dims(ki->second.n); need_float(kd, "filts_km");
      long const Ktot = (long)g.C * g.KH * g.KW, mi4 = ((long)g.OC + 3) / 4 * 4;
      if (kd.sz() != 2 || (long)kd.dims(0) != Ktot + 128 || (long)kd.dims(1) != mi4) rt_err("hip_conv: filts_km must be [K + 128][out_chan padded to a multiple of 4] floats");
      km = (float const *)host->nh_var_ptr(ki->second.n);
    }
    tile_override_t const tov(impl, "conv_tile", fi.op);
    nk.conv((float const *)host->nh_var_ptr(fnm), (float const *)host->nh_var_ptr(bnm), (float const *)host->nh_var_ptr(inm), (float *)host->nh_var_ptr(onm), g, bf16, out_ctot, out_coff,
         (row.member == kConvWinograd) ? "winograd_all" : nullptr, km); // hip_conv_winograd: the F(2x2,3x3) path for this function (3x3 / stride 1; others: direct)
  }
  void run_bconv() {
    conv_geom_t g = bck_geom_of_op(fi.op, row.member == kBconvBiases);
    if (row.member != kBconvBiases) {
      auto si = am.find("stride"), pi = am.find("in_pad");
      if (si == am.end() || pi == am.end()) rt_err(fn + ": 'stride' and 'in_pad' REF args are required");
      dims_t const stride = si->second.get_dims(host->nh_rtc()), in_pad = pi->second.get_dims(host->nh_rtc());
      if (!(stride == fi.op.get_dims("stride")) || !(in_pad == fi.op.get_dims("in_pad"))) rt_err(fn + ": stride / in_pad args disagree with the op");
    }
    string const ogl = var_of_op_dims("out_grad_loss");
    g.B = (int)n_img;
    tile_override_t const tov(impl, "conv_tile", fi.op);
    bool const bf16 = op_bf16_operands(fi.op);   // (str_val hip_operands: refuses a value that is neither f32 nor bf16, and bf16 on hip_bconv_filts / hip_bconv_biases)
    if (row.member == kBconvIn) {
      string const f = var_of_op_dims("filts"), igl = var_of_op_dims("in_grad_loss");
      if (!(fi.op.get_dims("in_grad_loss") == fi.op.get_dims("in"))) rt_err(fn + ": in_grad_loss must have the dims of in");
      float const *zin = nullptr;
      if (zinp) {   // the forward input: the op's in dims (the image count the other vars'), and not the var this call writes
        string const in = var_of_op_dims("in");
        if (in == igl) rt_err(fn + ": zero_if_in_non_pos=1: 'in' and 'in_grad_loss' are the same var '" + in + "'");
        zin = (float const *)host->nh_var_ptr(in);
      }
      nk.bconv_in((float const *)host->nh_var_ptr(f), (float const *)host->nh_var_ptr(ogl), (float *)host->nh_var_ptr(igl), g, zin, bf16);
    } else if (row.member == kBconvFilts) {
      string const in = var_of_op_dims("in"), fgl = var_of_op_dims("filts_grad_loss");
      if (!(fi.op.get_dims("filts_grad_loss") == fi.op.get_dims("filts"))) rt_err(fn + ": filts_grad_loss must have the dims of filts");
      nk.bconv_filts((float const *)host->nh_var_ptr(in), (float const *)host->nh_var_ptr(ogl), (float *)host->nh_var_ptr(fgl), g);
    } else if (row.member == kBconvFiltsBiases) {
      string const in = var_of_op_dims("in"), fgl = var_of_op_dims("filts_grad_loss"), bgl = var_of_op_dims("biases_grad_loss");
      if (!(fi.op.get_dims("filts_grad_loss") == fi.op.get_dims("filts"))) rt_err(fn + ": filts_grad_loss must have the dims of filts");
      if (fi.op.get_dims("biases_grad_loss").dims_prod() != (uint64_t)g.OC) rt_err(fn + ": biases_grad_loss must hold out_chan values");
      for (string const *o : {&fgl, &bgl}) if (*o == in || *o == ogl) rt_err(fn + ": the output var '" + *o + "' is also an input of the call");
      if (fgl == bgl) rt_err(fn + ": filts_grad_loss and biases_grad_loss are the same var '" + fgl + "'");
      nk.bconv_filts_biases((float const *)host->nh_var_ptr(in), (float const *)host->nh_var_ptr(ogl), (float *)host->nh_var_ptr(fgl), (float *)host->nh_var_ptr(bgl), g, bf16);
    } else {
      string const bgl = var_of_op_dims("biases_grad_loss");
      if (fi.op.get_dims("biases_grad_loss").dims_prod() != (uint64_t)g.OC) rt_err(fn + ": biases_grad_loss must hold out_chan values");
      nk.bconv_biases((float const *)host->nh_var_ptr(ogl), (float *)host->nh_var_ptr(bgl), g);
    }
  }
  void run_conv_grp() {   // every var has exactly the dims the op gives its arg (one device: no img shards), and the call's vars are different ones
    conv_grp_geom_t const g = conv_grp_geom_of_op(fi.op, row.member);
    auto si = am.find("stride"), pi = am.find("in_pad");
    if (si == am.end() || pi == am.end()) rt_err(fn + ": 'stride' and 'in_pad' REF args are required");
    if (!(si->second.get_dims(host->nh_rtc()) == fi.op.get_dims("stride")) || !(pi->second.get_dims(host->nh_rtc()) == fi.op.get_dims("in_pad"))) rt_err(fn + ": stride / in_pad args disagree with the op");
    std::map<string, string> seen;   // var -> the arg it is bound to
    auto var_ptr = [&](char const *an) -> float * {
      string const vn = var_of_op_dims(an);
      auto ins = seen.emplace(vn, an);
      if (!ins.second) rt_err(fn + ": args '" + ins.first->second + "' and '" + an + "' are the same var '" + vn + "'");
      return (float *)host->nh_var_ptr(vn);
    };
    tile_override_t const tov(impl, "conv_tile", fi.op);
    if (row.member == kConvGrpFwd) { float *a = var_ptr("filts"), *bias = var_ptr("biases"), *b = var_ptr("in"); nk.conv_grp(row.member, g, a, b, bias, var_ptr("out")); }
    else if (row.member == kConvGrpBckIn) { float *a = var_ptr("filts"), *b = var_ptr("out_grad_loss"); nk.conv_grp(row.member, g, a, b, nullptr, var_ptr("in_grad_loss")); }
    else { float *b = var_ptr("in"), *a = var_ptr("out_grad_loss"); nk.conv_grp(row.member, g, a, b, nullptr, var_ptr("filts_grad_loss")); }
  }
  void run_deconv() {   // every var has exactly the dims the op gives its arg (one device: no img shards), and the call's vars are different ones
    deconv_geom_t const g = deconv_geom_of_op(fi.op, row.member);
    std::map<string, string> seen;   // var -> the arg it is bound to
    auto var_ptr = [&](char const *an) -> float * {
      string const vn = var_of_op_dims(an);
      auto ins = seen.emplace(vn, an);
      if (!ins.second) rt_err(fn + ": args '" + ins.first->second + "' and '" + an + "' are the same var '" + vn + "'");
      return (float *)host->nh_var_ptr(vn);
    };
    if (row.member == kDeconvBckBiases) {
      conv_geom_t cg; memset(&cg, 0, sizeof(cg)); cg.B = g.B; cg.OC = g.OC; cg.OH = g.OH; cg.OW = g.OW;
      float *ogl = var_ptr("out_grad_loss");
      nk.bconv_biases(ogl, var_ptr("biases_grad_loss"), cg);
      return;
    }
    auto si = am.find("stride"), pi = am.find("in_pad");
    if (si == am.end() || pi == am.end()) rt_err(fn + ": 'stride' and 'in_pad' REF args are required");
    if (!(si->second.get_dims(host->nh_rtc()) == fi.op.get_dims("stride")) || !(pi->second.get_dims(host->nh_rtc()) == fi.op.get_dims("in_pad"))) rt_err(fn + ": stride / in_pad args disagree with the op");
    tile_override_t const tov(impl, "conv_tile", fi.op);
    if (row.member == kDeconvFwd) { float *a = var_ptr("filts"), *bias = var_ptr("biases"), *b = var_ptr("in"); nk.deconv(row.member, g, a, b, bias, var_ptr("out")); }
    else if (row.member == kDeconvBckIn) { float *a = var_ptr("filts"), *b = var_ptr("out_grad_loss"); nk.deconv(row.member, g, a, b, nullptr, var_ptr("in_grad_loss")); }
    else { float *b = var_ptr("in"), *a = var_ptr("out_grad_loss"); nk.deconv(row.member, g, a, b, nullptr, var_ptr("filts_grad_loss")); }
  }
  void run_sgd() {
    // every var must have exactly the dims the op gives its arg (params are no img shards), and the 3n + 1 vars must all be different: w_i and h_i are rewritten in place
    sgd_op_t const so = sgd_op_of_op(fi.op);
    int const n = (int)so.elems.size();
    std::map<string, string> seen;   // var -> the arg it is bound to
    auto var_ptr = [&](string const &an) -> void * {
      string const vn = var_of_op_dims(an, "the update is fp32 only");
      auto ins = seen.emplace(vn, an);
      if (!ins.second) rt_err(fn + ": args '" + ins.first->second + "' and '" + an + "' are the same var '" + vn + "'");
      return host->nh_var_ptr(vn);
    };
    std::vector<sgd_member_t> ms((size_t)n);
    for (int i = 0; i < n; ++i) {
      string const sx = "_" + std::to_string(i);
      sgd_member_t &m = ms[(size_t)i];
      m.w = (float *)var_ptr("w" + sx); m.g = (float const *)var_ptr("g" + sx); m.h = (float *)var_ptr("h" + sx);
      m.n = so.elems[(size_t)i]; m.lr_mult = so.lr_mult[(size_t)i]; m.decay_mult = so.decay_mult[(size_t)i];
    }
    float const *hyper = (float const *)var_ptr("hyper");
    nk.sgd_update(n, ms.data(), hyper);
  }
  void run_solver() {
    // as run_sgd: every var has exactly the dims the op gives its arg, and all the call's vars are different ones
    solver_op_t const so = solver_op_of_op(fi.op);
    size_t const n = so.elems.size();
    std::map<string, string> seen;   // var -> the arg it is bound to
    auto var_ptr = [&](string const &an) -> float * {
      string const vn = var_of_op_dims(an, "the solver is fp32 only");
      auto ins = seen.emplace(vn, an);
      if (!ins.second) rt_err(fn + ": args '" + ins.first->second + "' and '" + an + "' are the same var '" + vn + "'");
      return (float *)host->nh_var_ptr(vn);
    };
    if (so.update()) {
      std::vector<solver_member_t> ms(n);
      for (size_t i = 0; i < n; ++i) {
        string const sx = "_" + std::to_string(i);
        ms[i].w = var_ptr("w" + sx); ms[i].g = var_ptr("g" + sx); ms[i].h = var_ptr("h" + sx); ms[i].h2 = so.type == kSolverAdam ? var_ptr("h2" + sx) : nullptr;
      }
      float const *hyper = var_ptr("hyper"); float const *state = var_ptr("state");
      nk.solver_update(so, ms.data(), hyper, state, so.kind == 5 ? var_ptr("accum") : nullptr);
    } else if (so.kind == 4) {
      std::vector<float const *> gs(n); std::vector<float *> as(n);
      for (size_t i = 0; i < n; ++i) { string const sx = "_" + std::to_string(i); gs[i] = var_ptr("g" + sx); as[i] = var_ptr("a" + sx); }
      nk.grad_accum(so, gs.data(), as.data(), var_ptr("accum"));
    } else if (so.kind == 2) {
      std::vector<float const *> gs(n);
      for (size_t i = 0; i < n; ++i) gs[i] = var_ptr("g_" + std::to_string(i));
      nk.grad_sumsq(so, gs.data(), var_ptr("partials"));
    } else {
      float const *partials = var_ptr("partials"); float const *hyper = var_ptr("hyper");
      nk.grad_norm(so, partials, hyper, var_ptr("state"));
    }
  }
  void run_eval() {
    // every var has the type and the dims the op gives its arg -- except, for hip_accuracy (independent per image), the number of images, which only has to agree
    // between the call's vars -- and all the call's vars are different ones
    eval_op_t e = eval_op_of_op(fi.op);
    std::map<string, string> seen;   // var -> the arg it is bound to
    std::vector<void *> ptrs;
    for (string const &an : e.args) {
      string const vn = var_of(am, an); dims_t const vd = host->nh_var_dims(vn);
      dims_t want = fi.op.get_dims(an);
      if (vd.tn != want.tn) rt_err(fn + ": arg '" + an + "' (var '" + vn + "') has type " + vd.tn + ", the op says " + want.tn);
      if (e.kind == 1 && vd.sz() == want.sz() && vd.sz() >= 1) {
        if (n_img < 0) n_img = vd.dims(0);
        if ((long)vd.dims(0) != n_img) rt_err(fn + ": arg '" + an + "' has " + std::to_string(vd.dims(0)) + " images, another arg " + std::to_string(n_img));
        want[0].sz = vd.dims(0); want.calc_strides();
      }
      if (!(vd == want)) rt_err(fn + ": arg '" + an + "' has dims " + vd.pretty_str() + ", the op says " + fi.op.get_dims(an).pretty_str());
      auto ins = seen.emplace(vn, an);
      if (!ins.second) rt_err(fn + ": args '" + ins.first->second + "' and '" + an + "' are the same var '" + vn + "'");
      ptrs.push_back(host->nh_var_ptr(vn));
    }
    if (e.kind == 1) e.B = n_img;
    nk.eval_call(e, ptrs.data());
  }
  void run_loss() {
    // every var has the type and exactly the dims the op gives its arg (the count and the sum run over the whole batch: no img shards), and all the call's vars are
    // different ones
    loss_op_t const l = loss_op_of_op(fi.op);
    std::map<string, string> seen;   // var -> the arg it is bound to
    std::vector<void *> ptrs;
    for (string const &an : l.args) {
      string const vn = var_of(am, an); dims_t const vd = host->nh_var_dims(vn);
      dims_t const &want = fi.op.get_dims(an);
      if (vd.tn != want.tn) rt_err(fn + ": arg '" + an + "' (var '" + vn + "') has type " + vd.tn + ", the op says " + want.tn);
      if (!(vd == want)) rt_err(fn + ": arg '" + an + "' has dims " + vd.pretty_str() + ", the op says " + want.pretty_str());
      auto ins = seen.emplace(vn, an);
      if (!ins.second) rt_err(fn + ": args '" + ins.first->second + "' and '" + an + "' are the same var '" + vn + "'");
      ptrs.push_back(host->nh_var_ptr(vn));
    }
    nk.loss_call(l, ptrs.data());
  }
  void run_data() {
    // every var has the type and the dims the op gives its arg -- except the number of images of src, plan and out (the function is independent per image), which only
    // has to agree between them -- and all the call's vars are different ones
    data_op_t d = data_op_of_op(fi.op);
    std::map<string, string> seen;   // var -> the arg it is bound to
    std::vector<void *> ptrs;
    for (string const &an : d.args) {
      string const vn = var_of(am, an);
      auto ins = seen.emplace(vn, an);
      if (!ins.second) rt_err(fn + ": args '" + ins.first->second + "' and '" + an + "' are the same var '" + vn + "'");
      dims_t const vd = host->nh_var_dims(vn);
      dims_t want = fi.op.get_dims(an);
      if (vd.tn != want.tn) rt_err(fn + ": arg '" + an + "' (var '" + vn + "') has type " + vd.tn + ", the op says " + want.tn);
      if (an != "mean" && vd.sz() == want.sz() && vd.sz() >= 1) {
        if (n_img < 0) n_img = vd.dims(0);
        if ((long)vd.dims(0) != n_img) rt_err(fn + ": arg '" + an + "' has " + std::to_string(vd.dims(0)) + " images, another arg " + std::to_string(n_img));
        want[0].sz = vd.dims(0); want.calc_strides();
      }
      if (!(vd == want)) rt_err(fn + ": arg '" + an + "' has dims " + vd.pretty_str() + ", the op says " + fi.op.get_dims(an).pretty_str());
      ptrs.push_back(host->nh_var_ptr(vn));
    }
    d.B = n_img;
    nk.data_call(d, ptrs.data());
  }
  void run_bn() {
    // every var must have exactly the dims the op gives its arg (the sums run over the whole batch: no img shards), and no two args may be one var except where
    // kernels/bn_f32.hip allows in-place use
    // The hip_bnc_* functions (kFamBnc) leave the image count of their tensor vars free, as every function that runs on img shards does: fN stays the op's.  A whole
    // hip_bnc_stats / hip_bnc_bck_sums call still needs the op's batch; a multi-device backend runs them in pieces, named by two by-value uint32 args it adds to the
    // call (csrc/hip_multi.cc): bnc_stage = 1 S1 | 2 S2 | 3 the pair: the totals of THIS device's shard, one chunk, into slot bnc_slot of the call's totals here;
    // 4 mean | 5 statistics | 6 the raw pair: the cross-chunk step over the first bnc_slot slots
    bn_op_t const b = bn_op_of_op(fi.op);
    vect_string vars; std::vector<float *> tens, chans;
    auto var_ptr = [&](string const &an) -> float * {
      string const vn = var_of_op_dims(an, "fp32 only");
      vars.push_back(vn);
      return (float *)host->nh_var_ptr(vn);
    };
    for (string const &an : b.tens) tens.push_back(var_ptr(an));
    for (string const &an : b.chans) chans.push_back(var_ptr(an));
    bn_check_aliases(fn, b, vars);
    while (chans.size() < 5) chans.push_back(nullptr);
    if (!b.bnc) { nk.bn_call(b, tens.data(), chans.data()); return; }
    auto by_val = [&](char const *an) -> long {
      auto it = am.find(an);
      if (it == am.end()) return -1;
      if (!it->second.is_valid() || it->second.is_var() || !it->second.v->rp_elems() || it->second.v->dims.tn != "uint32_t" || it->second.v->dims.sz() != 0) rt_err(fn + ": '" + an + "' must be a by-value uint32_t scalar of the call");
      return (long)*(uint32_t const *)it->second.v->rp_elems();
    };
    long const stage = by_val("bnc_stage"), slot = by_val("bnc_slot");
    if (b.kind == 2 || b.kind == 4) { nk.bn_call(bn_op_on_imgs(b, n_img), tens.data(), chans.data()); return; }
    if (stage < 0) {
      if (n_img != b.B) rt_err(fn + ": the call's vars hold " + std::to_string(n_img) + " images, the op says " + std::to_string(b.B) + ": the sums run over the whole batch (a multi-device backend runs them per shard)");
      nk.bn_call(b, tens.data(), chans.data());
      return;
    }
    bool const st_ok = b.kind == 1 ? (stage == 1 || stage == 2 || stage == 4 || stage == 5) : (stage == 3 || stage == 6);
    if (!st_ok || b.chunks < 2 || slot < 0 || slot > (long)b.chunks || (stage <= 3 && slot == (long)b.chunks)) rt_err(fn + ": bnc_stage=" + std::to_string(stage) + " bnc_slot=" + std::to_string(slot) + ": not a piece of this call");
    float *tots = nullptr;
    float *const part = nk.bnc_ws(b, chans[0], chans[2], &tots);   // (keyed by per-channel vars: a device without images has no tensor pointer to tell calls apart)
    if (stage <= 3) {
      nk.bnc_chunk(bnc_op_of_imgs(fn, b, n_img), stage == 1 ? 0 : stage == 2 ? 3 : 2, tens[0], stage == 3 ? tens[1] : nullptr, stage == 1 ? nullptr : chans[0], stage == 3 ? chans[1] : nullptr, part, tots + slot * 2 * b.C);
    } else nk.bnc_cross(b, stage == 4 ? 3 : stage == 5 ? 1 : 2, tots, (int)slot, chans.data());
  }
  void run_bck_op() {
    // every var must have the dims the op gives its arg -- except the number of images, which only has to agree between the vars (a multi-device backend runs these
    // functions on img shards: csrc/hip_multi.cc); the REF args must be the op's
    bck_op_geom_t g = bck_op_geom_of_op(fi.op, row);
    bck_op_args_t const a = bck_op_args(row, fi.op);
    auto var_ptr = [&](string const &an) { return host->nh_var_ptr(var_of_op_dims(an)); };
    if (a.refs) for (char const *an : {"kern_sz", "stride", "in_pad"}) {
      auto ri = am.find(an);
      if (ri == am.end()) rt_err(fn + ": the REF arg '" + an + "' is required");
      if (!(ri->second.get_dims(host->nh_rtc()) == fi.op.get_dims(an))) rt_err(fn + ": arg '" + an + "' disagrees with the op");
    }
    float const *ins[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr}; float *outs[2] = {nullptr, nullptr};
    for (size_t i = 0; i < a.ins.size(); ++i) ins[i] = (float const *)var_ptr(a.ins[i]);
    for (size_t i = 0; i < a.outs.size(); ++i) outs[i] = (float *)var_ptr(a.outs[i]);
    if (zinp) {   // the condition is the forward input `in`: hip_bck_lrn's first arg; hip_spreading takes it as a fourth input.  Never the var the call writes
      if (g.op == 2) ins[3] = (float const *)var_ptr("in");
      if (var_of(am, "in") == var_of(am, "in_grad_loss")) rt_err(fn + ": zero_if_in_non_pos=1: 'in' and 'in_grad_loss' are the same var '" + var_of(am, "in") + "'");
      g.zinp = 1;
    }
    if (g.op == 10) {   // the seed is a by-value uint32 of the CALL: a new seed is no new function
      auto si = am.find("det_drop_seed");
      if (si == am.end() || !si->second.is_valid() || si->second.is_var() || !si->second.v->rp_elems() || si->second.v->dims.tn != "uint32_t" || si->second.v->dims.sz() != 0)
        rt_err(fn + ": 'det_drop_seed' must be a by-value uint32_t scalar of the call");
      g.seed = *(uint32_t const *)si->second.v->rp_elems();
    }
    uint32_t const *seed_word = nullptr;
    if (seedvar) {   // the word the kernel adds to the by-value seed: one uint32 in device memory, never the tensor the call rewrites
      auto wi = am.find("det_drop_seed_var");
      if (wi == am.end() || !wi->second.is_valid() || !wi->second.is_var()) rt_err(fn + ": seed_from_var=1: the var arg 'det_drop_seed_var' is required");
      check_seed_var(fn, wi->second.n, host->nh_var_dims(wi->second.n), var_of(am, "inout"));
      seed_word = (uint32_t const *)host->nh_var_ptr(wi->second.n); g.seedvar = 1;
    }
    if (g.op == 5) g.n = (long)host->nh_var_dims(var_of(am, "in")).dims_prod();
    else if (g.op == 9 || g.op == 10) g.n = (long)host->nh_var_dims(var_of(am, a.outs[0])).dims_prod();
    else if (n_img >= 0) g.B = n_img;
    if (g.op == 7 && img_shards) {   // an img shard of a batch: the divisor is the WHOLE batch's image count, which a multi-device backend adds to the call by value
      auto ti = am.find("img_total");
      if (ti != am.end()) {
        if (!ti->second.is_valid() || ti->second.is_var() || !ti->second.v->rp_elems() || ti->second.v->dims.tn != "uint32_t" || ti->second.v->dims.sz() != 0) rt_err(fn + ": img_shards=1: 'img_total' must be a by-value uint32_t scalar of the call");
        g.img_total = (long)*(uint32_t const *)ti->second.v->rp_elems();
        if (g.img_total < g.B) rt_err(fn + ": img_shards=1: img_total=" + std::to_string(g.img_total) + " is less than the " + std::to_string(g.B) + " images of this shard");
      }
    }
    nk.bck_op(g, ins, outs, seed_word);
  }
  void run_filts_kmajor() {   // filts (out_chan:in_chan:y:x) -> filts_km ([K + 128][out_chan padded to 4], zeros in the padding): see filts_km above
    string const fnm = var_of(am, "filts"), knm = var_of(am, "filts_km");
    dims_t const f = host->nh_var_dims(fnm), kd = host->nh_var_dims(knm);
    need_float(f, "filts"); need_float(kd, "filts_km"); assert_st(f.sz() == 4);
    long const OC = f.dims(0), Ktot = (long)f.dims(1) * f.dims(2) * f.dims(3), mi4 = (OC + 3) / 4 * 4, kp = Ktot + 128;
    if (kd.sz() != 2 || (long)kd.dims(0) != kp || (long)kd.dims(1) != mi4) rt_err("hip_conv_filts_kmajor: filts_km must be [K + 128][out_chan padded to a multiple of 4] floats");
    if ((uint64_t)kp * mi4 * 4 >= 0x7ffffff0ull) unsup_err("hip_conv_filts_kmajor: filts of 2 GiB or more");
    plan_t xp; xp.src = kSrc_conv_big_f32; xp.kname = "bodahip_conv_big_xpose"; xp.defs = {"-DXPOSE_ONLY=1"};
    kernel_t &xk = get_kernel(impl, host, xp);
    float const *src = (float const *)host->nh_var_ptr(fnm); float *dst = (float *)host->nh_var_ptr(knm); int Mi = (int)OC, Mi4 = (int)mi4, Kk = (int)Ktot, Kp = (int)kp;
    void *xparams[] = {&src, &dst, &Mi, &Mi4, &Kk, &Kp};
    hip_err_chk(host->nh_launch(xk.func, (uint32_t)((kp + 31) / 32), (uint32_t)((mi4 + 31) / 32), 256, xparams), "hipModuleLaunchKernel(conv_big_xpose)");
    nk.last_launch.kernel = "bodahip_conv_big_xpose"; nk.last_launch.grid = (uint32_t)(((kp + 31) / 32) * ((mi4 + 31) / 32)); nk.last_launch.block = 256; nk.last_launch.flops = 0; nk.last_launch.algo_bytes = 8.0 * OC * Ktot;
  }
};

void native_kernels_t::run(native_func_t const &f, rtc_func_info_t const &fi, map_str_rtc_arg_t const &am) {
  string const &fn = fi.op.get_func_name();
  impl->ws_used = false;   // set by ensure_ws: does this call's plan work in the shared scratch?  (what graph_end_deps' launch-order rule is about)
  struct ws_note_t { native_kernels_t *nk; impl_t *im; ~ws_note_t() { nk->last_call_uses_ws = im->ws_used; } } const ws_note{this, impl};
  exact_override_t const xov(impl, fi.op);
  bool const zinp = op_zinp_flag(fi.op);   // (refuses the flag on a function that cannot take it)
  bool const seedvar = op_seed_var_flag(fi.op);   // (likewise)
  bool const img_shards = op_img_shards_flag(fi.op);   // (likewise)
  call_t c{*this, impl, host, f, fi, am, fn, zinp, seedvar, img_shards};
  switch (f.family) {
  case kFamSgemm: c.run_sgemm(); break;
  case kFamConv: c.run_conv(); break;
  case kFamConvNhwc: c.run_conv_nhwc(); break;
  case kFamNhwcGrp: c.run_nhwc_grp(); break;
  case kFamNhwcMulti: c.run_nhwc_multi(); break;
  case kFamK1Chain: c.run_k1_chain(); break;
  case kFamFiltsKmajor: c.run_filts_kmajor(); break;
  case kFamBconv: c.run_bconv(); break;
  case kFamBckOp: c.run_bck_op(); break;
  case kFamSgd: c.run_sgd(); break;
  case kFamBn: case kFamBnc: case kFamBnf: c.run_bn(); break;
  case kFamSolver: c.run_solver(); break;
  case kFamEval: c.run_eval(); break;
  case kFamData: c.run_data(); break;
  case kFamLoss: c.run_loss(); break;
  case kFamConvGrp: c.run_conv_grp(); break;
  case kFamDeconv: c.run_deconv(); break;
  }
}

} // namespace bodahip

