"""Test infrastructure of the Deconvolution family (hip_deconv, hip_deconv_bck_in, hip_deconv_bck_biases, hip_deconv_bck_filts) and of hip_crop / hip_crop_bck: the case
list, the ops, the DEFINITION -- the existing Convolution / BckConv functions with the operands' roles exchanged -- run on a given backend, and an independent float64
twin (torch conv_transpose2d and autograd).

A case is (B, C, H, W, OC, (KH, KW), (SY, SX), (PY, PX)): in B x C x H x W, filts C x OC x KH x KW, out B x OC x OH x OW with OH = (H-1)*SY + KH - 2*PY."""
import numpy as np
import torch

from boda_amd.cnn_op import (NATIVE_ARGS, OpTune, add_bck_conv_annotations, add_bck_deconv_annotations, add_codegen_annotations, add_deconv_annotations, bck_deconv_calls,
                             deconv_calls, deconv_matrix_can, deconv_role_dims)
from boda_amd.op import parse_op
from boda_amd.rtc import RtcArg, RtcFuncCall, RtcFuncInfo


def _c(B, C, H, W, OC, k, s, p):
    two = lambda v: tuple(v) if isinstance(v, tuple) else (v, v)
    return (B, C, H, W, OC, two(k), two(s), two(p))


CASES = [
    _c(2, 3, 5, 4, 5, 4, 2, 1),
    _c(1, 21, 2, 2, 21, 64, 32, 0),           # FCN's 64/32 head in miniature: 96 x 96 out
    _c(2, 21, 4, 5, 21, 16, 8, 4),
    _c(2, 4, 5, 5, 3, 3, 2, 0),               # K not a multiple of S
    _c(1, 2, 4, 3, 2, 5, 3, 2),
    _c(2, 3, 6, 6, 3, 3, 1, 1),
    _c(2, 2, 3, 3, 2, 1, 2, 0),               # outputs no term reaches
    _c(1, 2, 3, 4, 2, 2, 3, 0),
    _c(2, 3, 4, 5, 2, (3, 5), (1, 2), (1, 0)),
]
MATRIX_CASES = [
    _c(1, 40, 6, 6, 48, 4, 2, 1),             # the planner's matrix path: min(C, OC) >= 32
    _c(1, 33, 5, 5, 70, 4, 2, 1),             # matrix path, ragged
]
PLANNER_MATRIX = MATRIX_CASES + [CASES[2]]   # (the 16/8 head: 21 channels, but gradient chains of 21 x 256 terms)
CASES = CASES + MATRIX_CASES
CASE_IDS = ["-".join("x".join(str(i) for i in v) if isinstance(v, tuple) else str(v) for v in c) for c in CASES]


def out_plane(case):
    B, C, H, W, OC, (KH, KW), (SY, SX), (PY, PX) = case
    return (H - 1) * SY + KH - 2 * PY, (W - 1) * SX + KW - 2 * PX


def _geom_fields(case):
    B, C, H, W, OC, (KH, KW), (SY, SX), (PY, PX) = case
    return f"in_pad=(tn=none,dims=(y={PY},x={PX})),kern_sz=(tn=none,dims=(y={KH},x={KW})),out_chans=(tn=uint32_t,v={OC}),stride=(tn=none,dims=(y={SY},x={SX}))"


def deconv_op(case, extra=""):
    B, C, H, W, OC, (KH, KW), _, _ = case
    OH, OW = out_plane(case)
    return parse_op(f"(str_vals=(type=Deconvolution),nda_vals=(biases=(dims=(out_chan={OC})),filts=(dims=(in_chan={C},out_chan={OC},y={KH},x={KW})),{extra}"
                    f"in=(dims=(img={B},chan={C},y={H},x={W})),out=(dims=(img={B},chan={OC},y={OH},x={OW})),{_geom_fields(case)}))")


def bck_deconv_op(case):
    B, C, H, W, OC, (KH, KW), _, _ = case
    OH, OW = out_plane(case)
    f = f"dims=(in_chan={C},out_chan={OC},y={KH},x={KW})"
    i = f"dims=(img={B},chan={C},y={H},x={W})"
    return parse_op(f"(str_vals=(type=BckDeconv),nda_vals=(biases=(dims=(out_chan={OC})),biases_grad_loss=(dims=(out_chan={OC})),filts=({f}),filts_grad_loss=({f}),"
                    f"in=({i}),in_grad_loss=({i}),out_grad_loss=(dims=(img={B},chan={OC},y={OH},x={OW})),{_geom_fields(case)}))")


def exchanged_ops(case):
    """The Convolution / BckConv ops of the exchanged roles: the convolution OC -> C whose input plane is the layer's out and whose output plane is the layer's in.
    -> (Convolution op, BckConv op)."""
    B, C, H, W, OC, (KH, KW), (SY, SX), (PY, PX) = case
    OH, OW = out_plane(case)
    f = f"dims=(out_chan={C},in_chan={OC},y={KH},x={KW})"
    i = f"dims=(img={B},chan={OC},y={OH},x={OW})"
    common = f"in_pad=(tn=none,dims=(y={PY},x={PX})),kern_sz=(tn=none,dims=(y={KH},x={KW})),out_chans=(tn=uint32_t,v={C}),stride=(tn=none,dims=(y={SY},x={SX}))"
    conv = parse_op(f"(str_vals=(type=Convolution),nda_vals=(biases=(dims=(out_chan={C})),filts=({f}),in=({i}),out=(dims=(img={B},chan={C},y={H},x={W})),{common}))")
    bck = parse_op(f"(str_vals=(type=BckConv),nda_vals=(biases=(dims=(out_chan={C})),biases_grad_loss=(dims=(out_chan={C})),filts=({f}),filts_grad_loss=({f}),"
                   f"in=({i}),in_grad_loss=({i}),out_grad_loss=(dims=(img={B},chan={C},y={H},x={W})),{common}))")
    return conv, bck


def exchanged_geom(case):
    """Op.bck_conv_geom() of the exchanged BckConv: what oracle/bck_chain takes."""
    return exchanged_ops(case)[1].bck_conv_geom()


def rand_ins(case, seed, lo=-5.0, hi=5.0):
    """The reference's test range U(-5, 5) for every operand of the four functions."""
    B, C, H, W, OC, (KH, KW), _, _ = case
    OH, OW = out_plane(case)
    rng = np.random.default_rng(seed)
    u = lambda *sh: rng.uniform(lo, hi, sh).astype(np.float32)
    return {"in": u(B, C, H, W), "filts": u(C, OC, KH, KW), "biases": u(OC), "out_grad_loss": u(B, OC, OH, OW)}


GUARD = 64   # floats of a guard var


def run_func(rtc, fop, ins, tile="", runs=1, guards=False):
    """Run one annotated function op on `rtc` with host inputs; every OUT var is NaN-filled before the call, so an element the call does not write shows.  guards: a
    guard var is created in front of and behind every var and must keep its bits.  -> (the function's first output array, the launch record of a be=hip backend or None)."""
    fn = fop.get_func_name()
    if tile:
        fop = fop.copy(); fop.str_vals["hip_tile"] = tile
    rtc.compile([RtcFuncInfo("f", "", [a for a, _ in NATIVE_ARGS[fn]], fop)])
    am, made, gvars = {}, [], []
    gpat = np.arange(GUARD, dtype=np.float32) + 0.5
    gdims = parse_op(f"(str_vals=(type=Crop),nda_vals=(in=(dims=(img=1,chan=1,y=1,x={GUARD})),out=(dims=(img=1,chan=1,y=1,x={GUARD})),offset=(tn=none,dims=(y=0,x=0))))").get_dims("in")

    def guard():
        if guards:
            gn = f"guard_{len(gvars)}"
            rtc.create_var_with_dims(gn, gdims); made.append(gn); gvars.append(gn)
            rtc.copy_nda_to_var(gn, gpat.reshape(1, 1, 1, GUARD))
    try:
        guard()
        for an, io in NATIVE_ARGS[fn]:
            if io == "REF":
                am[an] = RtcArg.ref(fop.get_dims(an)); continue
            rtc.create_var_with_dims(an, fop.get_dims(an)); made.append(an); am[an] = RtcArg.var(an)
            guard()
            if io == "IN":
                rtc.copy_nda_to_var(an, np.ascontiguousarray(ins[an], dtype=np.float32))
            else:
                rtc.copy_nda_to_var(an, np.full(fop.get_dims(an).sizes, np.nan, np.float32))
        for _ in range(runs):
            rtc.run(RtcFuncCall("f", am))
        rtc.finish_and_sync()
        launch = rtc.last_launch() if rtc.be == "hip" else None
        for gn in gvars:
            assert np.array_equal(rtc.copy_var_to_nda(gn).reshape(-1), gpat), (fn, gn)
        for an, io in NATIVE_ARGS[fn]:   # inputs are only read
            if io == "IN":
                assert bits_equal(rtc.copy_var_to_nda(an), np.ascontiguousarray(ins[an], dtype=np.float32)), (fn, an)
        return rtc.copy_var_to_nda([a for a, io in NATIVE_ARGS[fn] if io == "OUT"][0]), launch
    finally:
        for vn in made:
            rtc.release_var(vn)
        rtc.release_func("f"); rtc.release_per_call_id_data()


def deconv_funcs(case, tune=None):
    """-> {"fwd", "in", "biases", "filts"}: the four DIRECT function ops of a case (the forced direct path: the planner may choose otherwise)."""
    tune = tune or OpTune()
    fi, fb, ff = add_bck_deconv_annotations(bck_deconv_op(case), tune, form="direct")
    return {"fwd": add_deconv_annotations(deconv_op(case), tune, form="direct"), "in": fi, "biases": fb, "filts": ff}


def can_matrix(case):
    return deconv_matrix_can(deconv_op(case))


def path_calls(case, which, form="", tune=None):
    """-> (the layer's op, [(function op, {arg: role})]) of one function ("fwd" | "in" | "biases" | "filts") on the path `form` ("" = the planner's choice)."""
    tune = tune or OpTune()
    if which == "fwd":
        op = deconv_op(case)
        return op, deconv_calls(op, tune, form)
    op = bck_deconv_op(case)
    return op, [bck_deconv_calls(op, tune, form)[{"in": 0, "biases": 1, "filts": 2}[which]]]


OUT_ROLE = {"fwd": "out", "in": "in_grad_loss", "biases": "biases_grad_loss", "filts": "filts_grad_loss"}
_VIEW_OF = {"filts_x": "filts", "filts_grad_loss_x": "filts_grad_loss", "biases_x": "biases"}


def run_calls(rtc, op, calls, ins, which, guards=False):
    """Run a path's call list as a driver binds it: one var per role of the layer (NaN-filled unless it is an input), the views filts_x / filts_grad_loss_x / biases_x
    of those vars under the exchanged dims, the constants ones / zeros.  guards: a guard var in front of and behind every var.
    -> (the output array of `which`, [the launch record after each call] on be=hip)."""
    names, made, views, gvars, launches = {}, [], [], [], []
    gpat = np.arange(GUARD, dtype=np.float32) + 0.5
    gdims = crop_ops(1, 1, 1, GUARD, 1, GUARD, 0, 0)[0].get_dims("in")

    def guard():
        if guards:
            gn = f"guard_{len(gvars)}"
            rtc.create_var_with_dims(gn, gdims); made.append(gn); gvars.append(gn); rtc.copy_nda_to_var(gn, gpat.reshape(1, 1, 1, GUARD))

    def var_of(role):
        if role in names:
            return names[role]
        vn = "rc_" + role
        if role in _VIEW_OF:
            rtc.create_var_with_dims_as_reshaped_view_of_var(vn, deconv_role_dims(op, role), var_of(_VIEW_OF[role])); views.append(vn)
        else:
            guard()
            d = deconv_role_dims(op, role) if role in ("ones", "zeros") else op.get_dims(role)
            rtc.create_var_with_dims(vn, d); made.append(vn)
            fill = ins[role] if role in ins else np.full(d.sizes, {"ones": 1.0, "zeros": 0.0}.get(role, np.nan), np.float32)
            rtc.copy_nda_to_var(vn, np.ascontiguousarray(fill, dtype=np.float32).reshape(d.sizes))
            guard()
        names[role] = vn
        return vn
    funcs = []
    try:
        for i, (fop, binds) in enumerate(calls):
            fn = fop.get_func_name()
            rtc.compile([RtcFuncInfo(f"rc_f{i}", "", [a for a, _ in NATIVE_ARGS[fn]], fop)]); funcs.append(f"rc_f{i}")
            am = {an: (RtcArg.ref(fop.get_dims(an)) if io == "REF" else RtcArg.var(var_of(binds[an]))) for an, io in NATIVE_ARGS[fn]}
            rtc.run(RtcFuncCall(f"rc_f{i}", am)); rtc.finish_and_sync()
            launches.append(rtc.last_launch() if rtc.be == "hip" else None)
        for gn in gvars:
            assert np.array_equal(rtc.copy_var_to_nda(gn).reshape(-1), gpat), gn
        for role, a in ins.items():   # inputs are only read
            if role in names:
                assert bits_equal(rtc.copy_var_to_nda(names[role]), np.ascontiguousarray(a, dtype=np.float32)), role
        return rtc.copy_var_to_nda(names[OUT_ROLE[which]]), launches
    finally:
        for vn in views + made:
            rtc.release_var(vn)
        for f in funcs:
            rtc.release_func(f)
        rtc.release_per_call_id_data()


def cfg_bk_ksl(launch):
    """(BK, KSL) of a launch, from its configuration string BIxBJxBK_wWIxWJ[_sKSL] (tests/test_gpu_bck_chain.py: plan_of)."""
    cfg = launch["cfg"]
    return int(cfg.split("_")[0].split("x")[2]), (int(cfg.split("_s")[1].split("_")[0]) if "_s" in cfg else 1)


def filts_tiles(case):
    """The forced plans of the filter gradient a GPU test runs: -> [(seven-field tile, BK, KSL)] with KSL 1 / 2 / 3 / one more than the K steps (an empty slice), a BK
    that does not divide K = B*H*W, and many slices of a short step."""
    B, C, H, W = case[:4]
    K = B * H * W
    bk_odd = next(b for b in (10, 14, 6, 22, 7, 3) if K % b)
    nkt = -(-K // 32)
    plans = [(32, 1), (32, 2), (bk_odd, 3), (bk_odd, 1), (32, nkt + 1), (1, min(K + 2, 300))]
    return [(f"1x1x{bk}x2x2x1x{ksl}", bk, ksl) for bk, ksl in plans]


def exchanged(rtc, case, ins, which):
    """The definition: the EXISTING function on backend `rtc` with the roles exchanged.
      fwd     hip_bconv_in on (filts := filts, out_grad_loss := in) -> acc, then out = acc + biases[oc], one fp32 add
      in      hip_conv on (filts := filts read as out_chan=C:in_chan=OC, biases := C values of +0, in := out_grad_loss), no ReLU
      filts   hip_bconv_filts on (in := out_grad_loss, out_grad_loss := in)
      biases  hip_bconv_biases on out_grad_loss"""
    B, C, H, W, OC, (KH, KW), _, _ = case
    conv, bck = exchanged_ops(case)
    xi, xb, xf = add_bck_conv_annotations(bck, OpTune())
    as_conv_filts = np.ascontiguousarray(ins["filts"]).reshape(C, OC, KH, KW)   # the same memory, read as out_chan=C : in_chan=OC
    if which == "fwd":
        acc, _ = run_func(rtc, xi, {"filts": as_conv_filts, "out_grad_loss": ins["in"]})
        return (acc + ins["biases"].astype(np.float32).reshape(1, OC, 1, 1)).astype(np.float32)
    if which == "in":
        xc = add_codegen_annotations(conv, OpTune())
        del xc.nda_vals["conv_has_relu"]; xc.set_u32("conv_has_relu", 0)   # (the annotator's is the ops-prof ReLU)
        return run_func(rtc, xc, {"filts": as_conv_filts, "biases": np.zeros(C, np.float32), "in": ins["out_grad_loss"]})[0]
    if which == "filts":
        return run_func(rtc, xf, {"in": ins["out_grad_loss"], "out_grad_loss": ins["in"]})[0]
    OH, OW = out_plane(case)
    bop = parse_op(f"(str_vals=(type=BckConv,func_name=hip_bconv_biases),nda_vals=(out_grad_loss=(dims=(img={B},chan={OC},y={OH},x={OW})),biases_grad_loss=(dims=(out_chan={OC}))))")
    return run_func(rtc, bop, {"out_grad_loss": ins["out_grad_loss"]})[0]


def torch_twin(case, ins):
    """float64, independent of the role exchange: torch conv_transpose2d and autograd.  -> {"fwd", "in", "filts", "biases"} and, under "abs", sum |terms| per output of
    each function (the same function on absolute values): the scale of the float64 bound.  The gradients are those of sum(out * out_grad_loss)."""
    B, C, H, W, OC, (KH, KW), s, p = case
    res = {}
    for key, f in (("val", lambda a: a.astype(np.float64)), ("abs", lambda a: np.abs(a.astype(np.float64)))):
        x = torch.from_numpy(f(ins["in"])).requires_grad_(True)
        w = torch.from_numpy(f(ins["filts"])).requires_grad_(True)
        b = torch.from_numpy(f(ins["biases"])).requires_grad_(True)
        y = torch.nn.functional.conv_transpose2d(x, w, b, stride=s, padding=p)
        (y * torch.from_numpy(f(ins["out_grad_loss"]))).sum().backward()
        res[key] = {"fwd": y.detach().numpy(), "in": x.grad.numpy(), "filts": w.grad.numpy(), "biases": b.grad.numpy()}
    out = dict(res["val"]); out["abs"] = res["abs"]
    return out


def chain_len(case, which, ksl=1):
    """Roundings of one output's chain: the terms, plus the bias add (fwd, in), plus the slab adds of a sliced filter gradient."""
    B, C, H, W, OC, (KH, KW), (SY, SX), _ = case
    OH, OW = out_plane(case)
    if which == "fwd":
        return C * -(-KH // SY) * -(-KW // SX) + 1
    if which == "in":
        return OC * KH * KW + 1
    if which == "filts":
        return B * H * W + ksl
    return B * OH * OW


def within_f64_bound(got, twin, case, which, ksl=1):
    """|got - float64| <= (n + 1) * 2^-24 * sum |terms|, n the chain length (plus KSL for a sliced filter gradient)."""
    n = chain_len(case, which, ksl)
    err = np.abs(got.astype(np.float64) - twin[which])
    return bool(np.all(err <= (n + 1) * 2.0 ** -24 * twin["abs"][which]))


def crop_ops(B, C, H, W, OH, OW, oy, ox):
    """-> (Crop op, BckCrop op)."""
    big, win, off = f"dims=(img={B},chan={C},y={H},x={W})", f"dims=(img={B},chan={C},y={OH},x={OW})", f"offset=(tn=none,dims=(y={oy},x={ox}))"
    return (parse_op(f"(str_vals=(type=Crop),nda_vals=(in=({big}),out=({win}),{off}))"),
            parse_op(f"(str_vals=(type=BckCrop),nda_vals=(out_grad_loss=({win}),in_grad_loss=({big}),{off}))"))


CROP_CASES = [(2, 3, 10, 10, 8, 8, 1, 1), (1, 5, 18, 17, 16, 16, 1, 0), (1, 5, 18, 17, 16, 16, 2, 1), (2, 2, 6, 5, 6, 5, 0, 0)]   # the last: the whole plane


def bits_equal(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32))
