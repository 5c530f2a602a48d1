"""Variant selection for the hot path (host side; CPU only).

Restates the part of the reference's annotation layer that decides WHICH function runs an op and in what layout:
  * op_tune_t and its NESI text form                       src/cnn_op.H:14-30, dump rule src/nesi.cc:353-370
  * add_codegen_annotations / add_cnn_codegen_annotations  src/cnn_op.cc:16-68, 331-380
For be=hip every Convolution / sgemm is routed to the native side door -- `hip_conv` / `hip_sgemm` (or the reference's
own door names `cudnn_conv` / `cublas_sgemm` when use_culibs=1) -- which, exactly like use_culibs in the reference
(src/cnn_op.cc:47-48,142,339-340), leaves every tensor in reference layout and adds no `work` blocking.  The
reference's CUCL variants (conv/k1conv/tconv/ipconv/sgemm*) are produced by its own code generator and are reported
as unsupported here, the way ops-prof records any annotation failure (src/rtc_prof.cc:287-290).
"""
from __future__ import annotations
from dataclasses import dataclass, fields
from numbers import Integral
from typing import Dict

from .op import Nda, Op, RtErr, UnsupErr, parse_lexp


@dataclass
class OpTune:
    use_be: str = ""
    use_culibs: int = 0
    MNt: tuple = (8, 8)
    MNb: tuple = (8, 16)
    Kb: int = 8
    use_local_mem: int = 1
    prof_variant: int = 0
    vw: int = 8
    k1conv: int = 0
    tconv: int = 0
    tconv_max_ksz: tuple = (11, 11)
    ipconv: int = 0
    hip_dtype: str = ""  # extension: "" / "f32" = exact fp32 MFMA path; "bf16" = bf16 operands, fp32 accumulate (BASELINE config 5)
    hip_algo: str = ""  # extension: "" = the bit-exact direct kernels; "winograd": func hip_conv_winograd (3x3 / stride-1 layers through F(2x2,3x3), mrd <= ~2e-3)
    hip_layout: str = ""  # extension (with hip_dtype=bf16): "nhwc" = channels-last bf16 STORAGE for in / filts / out: func hip_conv_nhwc on transposed operands,
    # the originals kept as <arg>_ref and filled / read back by xpose functions outside the timed call -- the reference's own k1conv / tconv protocol (boda_amd/nhwc.py)
    hip_s2d: int = 1  # extension (with hip_layout=nhwc): 1 = conv1-type layers (stride >= 2 on <= 8 channels) run space-to-depth, the regrouping done by the layout pass of `in` (boda_amd/nhwc.py)
    hip_patch: int = 1  # extension (with hip_layout=nhwc): 1 = layers with more than one tap and stride 1 in x take the LDS input-patch kernel (filts in the in_grp:y:x:out_chan:in_chan8 form); 0 = implicit GEMM for every layer
    hip_out: str = ""  # extension (with hip_layout=nhwc): "f32" = the kernel writes float instead of bfloat16
    hip_exact: int = 1  # extension: 1 = fp32 results bit-identical to the reference's per-thread fma chain (default); 0 = tolerance mode: within the reference's bound for re-associating
    # kernels (mrd < 2e-3, src/rtc_prof.cc:317-319,436; its 2e-4 default, :161, is not met by ANY second association of a K = 9216 sum on its U(-5,5) data) -- deterministic K slices on tile-starved long-K layers, Winograd where it is faster
    hip_tile: str = ""  # extension: workgroup tile of the native kernels "BIxBJxBKxWIxWJ[xMINW[xSPLITK[xMT[xPF[xSW[xKHO]]]]]]" ("" = heuristic)

    _ALWAYS = ("MNt", "MNb", "tconv_max_ksz")  # u32_pt_t fields print as "8 8" != default text "8:8": always dumped

    @staticmethod
    def parse(s: str) -> "OpTune":
        t = OpTune()
        items = parse_lexp(s) if s.strip() else []
        if isinstance(items, str):
            raise RtErr(f"op_tune: expected list, got {items!r}")
        names = {f.name for f in fields(OpTune)}
        for k, v in items:
            if k not in names or k.startswith("_"):
                raise RtErr(f"op_tune: unknown field {k!r}")
            if k in ("MNt", "MNb", "tconv_max_ksz"):
                parts = [p for p in str(v).replace(":", " ").split() if p]
                if len(parts) != 2:
                    raise RtErr(f"op_tune: {k} needs two values")
                setattr(t, k, (int(parts[0]), int(parts[1])))
            elif k in ("use_be", "hip_tile", "hip_dtype", "hip_algo", "hip_layout", "hip_out"):
                setattr(t, k, str(v))
            else:
                setattr(t, k, int(v))
        return t

    def to_str(self) -> str:
        """NESI dump: a field is printed unless equal to its default; u32_pt_t fields always (see module doc)."""
        d = OpTune()
        parts = []
        for f in fields(OpTune):
            if f.name.startswith("_"):
                continue
            v = getattr(self, f.name)
            if f.name in OpTune._ALWAYS:
                parts.append(f"{f.name}={v[0]} {v[1]}")
            elif v != getattr(d, f.name):
                parts.append(f"{f.name}={v}")
        return "(" + ",".join(parts) + ")"


REF_CUCL_VARIANTS = ("conv", "k1conv", "tconv", "ipconv", "conv_simd", "k1conv_simd")


def ref_conv_variant(op: Op, tune: OpTune) -> str:
    """Which CUCL variant the REFERENCE would pick for this conv under `tune` (src/cnn_op.cc:46-68); informational."""
    g = op.conv_geom()
    if tune.use_culibs:
        return "cudnn_conv"
    if tune.ipconv and g["PY"] == 0 and g["PX"] == 0 and g["OH"] == 1 and g["OW"] == 1:
        return "ipconv"
    if tune.k1conv and (g["KH"], g["KW"]) == (1, 1) and (g["SY"], g["SX"]) == (1, 1) and 6 <= g["OW"] <= 300 and g["OC"] >= 64:
        if g["PY"] or g["PX"]:
            return "conv"
        return "k1conv_simd" if tune.use_local_mem == 2 else "k1conv"
    if tune.tconv and (tune.tconv == 2 or (g["KW"] <= tune.tconv_max_ksz[0] and g["KH"] <= tune.tconv_max_ksz[1]
                                            and g["KW"] >= 1 and g["KH"] >= 1 and g["OW"] >= 6)):
        return "tconv"
    return "conv_simd" if tune.use_local_mem == 2 else "conv"


_TILE_WISDOM = None   # process-wide per-op best-tile table (boda_amd.wis_ana.TileWisdom), see set_tile_wisdom


def set_tile_wisdom(tw) -> None:
    """Install (or, with None, remove) the per-op best-tile table every later add_codegen_annotations consults: a TileWisdom, or the path of its text
    form (what `python -m boda_amd.wis_ana --tile-wisdom-out-fn` writes from the wisdom files ops-prof records).  The environment variable
    BODAHIP_TILE_WISDOM=<path> installs one at import."""
    global _TILE_WISDOM
    if isinstance(tw, str):
        from .wis_ana import TileWisdom
        tw = TileWisdom.load(tw)
    _TILE_WISDOM = tw


def add_codegen_annotations(op: Op, tune: OpTune, tile_wisdom=None) -> Op:
    """-> annotated copy of `op` with func_name (and conv_has_relu for convs) set.  Raises UnsupErr for variants
    this backend does not provide.  A tile recorded for this op in `tile_wisdom` (or the table installed with set_tile_wisdom) is given to
    the function when the tune names none: it then overrides the native planner's cost model for this function's calls only."""
    tw = tile_wisdom if tile_wisdom is not None else _TILE_WISDOM
    if tw is not None and not tune.hip_tile and not tune.hip_dtype and not tune.hip_layout and tune.hip_exact:   # (the table is recorded for the bit-exact fp32 functions)
        t = tw.tile_for(op)
        if t:
            import dataclasses
            tune = dataclasses.replace(tune, hip_tile=t)
    a = op.copy()
    t = a.get_type()
    native = (tune.use_be in ("", "hip"))
    if t == "Convolution":
        grouped = "G" in a.conv_geom()
        a.set_u32("conv_has_relu", 1)  # every Convolution under ops-prof (src/cnn_op.cc:337)
        if grouped:   # group > 1: the grouped family's forward function and nothing else (fp32, reference layouts)
            refuse_grouped(a, tune)
            a.set_func_name(CONV_GRP_FUNC)
        elif tune.use_culibs:
            a.set_func_name("cudnn_conv")
        elif native and not (tune.k1conv or tune.tconv or tune.ipconv) and tune.hip_dtype == "bf16" and tune.hip_layout == "nhwc":
            from . import nhwc
            nhwc.annotate(a, "float" if tune.hip_out == "f32" else "bfloat16", allow_s2d=bool(tune.hip_s2d), allow_patch=bool(tune.hip_patch))
        elif native and not (tune.k1conv or tune.tconv or tune.ipconv):
            a.set_func_name("hip_conv_bf16" if tune.hip_dtype == "bf16" else ("hip_conv_winograd" if tune.hip_algo == "winograd" else "hip_conv"))
        else:
            raise UnsupErr(f"variant '{ref_conv_variant(op, tune)}' is generated by the reference's CUCL code generator; "
                           f"be=hip provides hip_conv / cudnn_conv (op_tune={tune.to_str()})")
    elif t == "sgemm":
        a.sgemm_geom()
        if tune.use_culibs:
            a.set_func_name("cublas_sgemm")
        elif native:
            a.set_func_name("hip_sgemm_bf16" if tune.hip_dtype == "bf16" else "hip_sgemm")
        else:
            raise UnsupErr(f"sgemm variants of use_be={tune.use_be!r} are generated by the reference's CUCL code generator")
    else:
        raise UnsupErr(f"op type {t!r} is not on the conv_fwd / sgemm hot path")
    if not tune.hip_exact and native and not tune.use_culibs and tune.hip_dtype != "bf16":
        a.str_vals["hip_exact"] = "0"   # travels with the function, like hip_tile
    if tune.hip_tile and native and not tune.use_culibs and (a.get_func_name() != CONV_GRP_FUNC or is_grp_tile(tune.hip_tile)):
        a.str_vals["hip_tile"] = tune.hip_tile   # travels with the function: the backend applies it to this function's calls only (a grouped op: its own seven-field form only)
    return a


BCONV_FUNCS = ("hip_bconv_in", "hip_bconv_biases", "hip_bconv_filts")   # the order of the reference's three calls (src/rtc_fwd.cc:398-400)

# a Convolution / BckConv with group = g > 1 (Caffe's `group`; the reference has none): for every group the ungrouped function on the op sliced to that group
# (kernels/conv_grp_f32.hip).  The bias gradient knows no groups: it stays hip_bconv_biases
CONV_GRP_FUNC = "hip_conv_grp"
BCONV_GRP_FUNCS = ("hip_bconv_in_grp", "hip_bconv_biases", "hip_bconv_filts_grp")   # the same call order


def op_group(op: Op) -> int:
    """Caffe's `group` of a Convolution / BckConv op: uint32 group, the form of out_chans; absent means 1."""
    return op.get_u32("group") if op.has("group") else 1


def is_grp_tile(tile: str) -> bool:
    """Is `tile` the grouped family's own form, seven fields BIxBJxBKxWIxWJxMINWxKSL?  A pipe-wide tile written for hip_conv / hip_bconv_* (five or six fields, or
    more than seven) is not: it passes a grouped layer by, and the planner chooses for it."""
    return bool(tile) and tile.count("x") == 6


def is_grouped(op: Op) -> bool:
    return op.get_type() in ("Convolution", "BckConv") and op_group(op) > 1


def refuse_grouped(op: Op, tune: OpTune = None, what: str = "") -> None:
    """UnsupErr that names `group` where a grouped op meets a function or an option that has no grouped form: everything but fp32 in reference layouts on the
    grouped family's own three functions."""
    g = op_group(op)
    if g <= 1:
        return
    if what:
        raise UnsupErr(f"{what}: the op carries group={g}: a grouped convolution runs as {CONV_GRP_FUNC} / {BCONV_GRP_FUNCS[0]} / {BCONV_GRP_FUNCS[2]} "
                       f"(fp32, reference layouts) only")
    if tune is None:
        return
    bad = [n for n, v in (("use_culibs", tune.use_culibs), ("k1conv", tune.k1conv), ("tconv", tune.tconv), ("ipconv", tune.ipconv), ("hip_algo", tune.hip_algo),
                          ("hip_layout", tune.hip_layout), ("hip_out", tune.hip_out)) if v]
    if tune.hip_dtype not in ("", "f32"):
        bad.append("hip_dtype")
    if tune.use_be not in ("", "hip"):
        bad.append("use_be")
    if not tune.hip_exact:
        bad.append("hip_exact=0")
    if bad:
        raise UnsupErr(f"group={g}: a grouped convolution has no form under op_tune {', '.join(bad)} ({tune.to_str()}): fp32 in reference layouts only "
                       f"({CONV_GRP_FUNC} / {BCONV_GRP_FUNCS[0]} / {BCONV_GRP_FUNCS[2]})")


def add_bck_conv_grp_annotations(op: Op, tune: OpTune) -> tuple:
    """-> (in_op, biases_op, filts_op) of a BckConv with group > 1, in the reference's call order: hip_bconv_in_grp, hip_bconv_biases (the ungrouped function as it is:
    the bias gradient does not depend on groups), hip_bconv_filts_grp.  A seven-field tile in the tune travels with the two grouped functions; any other tile (a
    pipe-wide one written for the ungrouped functions) passes them by."""
    if op.get_type() != "BckConv":
        raise RtErr(f"add_bck_conv_grp_annotations: op type {op.get_type()!r} is not BckConv")
    if "G" not in op.bck_conv_geom():
        raise RtErr("add_bck_conv_grp_annotations: the op carries no group > 1 (add_bck_conv_annotations is the annotator of an ungrouped BckConv)")
    refuse_grouped(op, tune)
    outs = []
    for fn in BCONV_GRP_FUNCS:
        a = op.copy()
        a.set_func_name(fn)
        if is_grp_tile(tune.hip_tile) and fn != "hip_bconv_biases":
            a.str_vals["hip_tile"] = tune.hip_tile
        outs.append(a)
    return tuple(outs)


# a Deconvolution / BckDeconv (this backend's own; kernels/deconv_f32.hip): each function is an existing one with the operands' roles exchanged
DECONV_FUNC = "hip_deconv"
BCK_DECONV_FUNCS = ("hip_deconv_bck_in", "hip_deconv_bck_biases", "hip_deconv_bck_filts")   # BckConv's call order


def refuse_deconv_tune(op: Op, tune: OpTune) -> None:
    """UnsupErr that names the layer type where a Deconvolution meets an option it has no form under: fp32 in reference layouts on the family's own functions only."""
    bad = [n for n, v in (("use_culibs", tune.use_culibs), ("k1conv", tune.k1conv), ("tconv", tune.tconv), ("ipconv", tune.ipconv), ("hip_algo", tune.hip_algo),
                          ("hip_layout", tune.hip_layout), ("hip_out", tune.hip_out)) if v]
    if tune.hip_dtype not in ("", "f32"):
        bad.append("hip_dtype")
    if tune.use_be not in ("", "hip"):
        bad.append("use_be")
    if bad:
        raise UnsupErr(f"{op.get_type()}: a Deconvolution has no form under op_tune {', '.join(bad)} ({tune.to_str()}): fp32 in reference layouts only "
                       f"({DECONV_FUNC} / {' / '.join(BCK_DECONV_FUNCS)})")


DECONV_MATRIX_MIN_CHANS = 32   # the planner's threshold: the matrix path where min(C, OC) reaches it (DESIGN.md section 3.25 says where it sits and why) ...
DECONV_MATRIX_MIN_TERMS = 1024 # ... or where a gradient's chain, max(C, OC) x KH x KW terms, reaches this: moved here on the record (FCN's 16/8 head, 5376 terms: 6 - 11x)
DECONV_MATRIX_MAX_STRIDE = 16  # hip_bconv_in / hip_bconv_filts: strides of at most 16 (kernels of at most 64 x 64 hold for the whole family)


def deconv_matrix_can(op: Op) -> bool:
    """Is the exchanged geometry inside the existing functions' limits (hip_bconv_in, hip_conv, hip_bconv_filts)?"""
    g = op.deconv_geom()
    return max(g["SY"], g["SX"]) <= DECONV_MATRIX_MAX_STRIDE and max(g["KH"], g["KW"]) <= 64


def deconv_form(op: Op, tune: OpTune) -> str:
    """-> "direct" | "matrix": which path a Deconvolution / BckDeconv takes.  The rule reads the op alone: the direct forms (kernels/deconv_f32.hip) where
    min(C, OC) < DECONV_MATRIX_MIN_CHANS and max(C, OC) x KH x KW < DECONV_MATRIX_MIN_TERMS, or the exchanged geometry is outside an existing function's limits,
    else the existing matrix functions on the exchanged roles.  A tile string forces either: a seven-field tile whose BI is 1 the direct forms, any tile whose BI is larger the matrix path (UnsupErr where the
    geometry is outside the limits); the tile then travels with that path's conv functions."""
    g = op.deconv_geom()
    tile = tune.hip_tile
    if tile:
        bi = tile.split("x")[0]
        if is_grp_tile(tile) and bi == "1":
            return "direct"
        if bi.isdigit() and int(bi) > 1:
            if not deconv_matrix_can(op):
                raise UnsupErr(f"{op.get_type()}: tile {tile} asks for the matrix path, but stride {g['SY']} x {g['SX']} is outside hip_bconv_in's / hip_bconv_filts' limits "
                               f"(at most {DECONV_MATRIX_MAX_STRIDE}): the direct forms only")
            return "matrix"
    wide = min(g["C"], g["OC"]) >= DECONV_MATRIX_MIN_CHANS or max(g["C"], g["OC"]) * g["KH"] * g["KW"] >= DECONV_MATRIX_MIN_TERMS
    return "matrix" if wide and deconv_matrix_can(op) else "direct"


def deconv_exchanged_ops(op: Op) -> tuple:
    """-> (Convolution op, BckConv op) of the exchanged roles of a Deconvolution / BckDeconv: the convolution OC -> C whose input plane is the layer's out and whose
    output plane is the layer's in; its filts are the layer's blob read as out_chan=C : in_chan=OC."""
    from .op import Dims
    g = op.deconv_geom()
    f = Dims(("out_chan", "in_chan", "y", "x"), (g["C"], g["OC"], g["KH"], g["KW"]), "float")
    big = Dims(("img", "chan", "y", "x"), (g["B"], g["OC"], g["OH"], g["OW"]), "float")
    small, b = op.get_dims("in"), Dims(("out_chan",), (g["C"],), "float")
    common = {"filts": Nda(dims=f, tn="float"), "biases": Nda(dims=b, tn="float"), "in": Nda(dims=big, tn="float"), "kern_sz": op.get("kern_sz"), "stride": op.get("stride"),
              "in_pad": op.get("in_pad"), "out_chans": Nda(None, "uint32_t", (g["C"],))}
    conv = Op({"type": "Convolution"}, dict(common, out=Nda(dims=small, tn="float")))
    bck = Op({"type": "BckConv"}, dict(common, out_grad_loss=Nda(dims=small, tn="float"), in_grad_loss=Nda(dims=big, tn="float"), filts_grad_loss=Nda(dims=f, tn="float"),
                                       biases_grad_loss=Nda(dims=b, tn="float")))
    conv.conv_geom(); bck.bck_conv_geom()
    return conv, bck


# the vars of a matrix-path call, by ROLE: the layer's own ("in", "out", "biases", "out_grad_loss", "in_grad_loss", "biases_grad_loss"), views of the layer's vars under
# the exchanged dims ("filts_x" / "filts_grad_loss_x": the blob as out_chan=C : in_chan=OC; "biases_x": biases as chan=OC) and the two constants the driver creates
# ("ones": chan=OC values of 1; "zeros": out_chan=C values of +0).  deconv_role_dims gives a role's dims
def deconv_role_dims(op: Op, role: str):
    from .op import Dims
    g = op.deconv_geom()
    if role in ("filts_x", "filts_grad_loss_x"):
        return Dims(("out_chan", "in_chan", "y", "x"), (g["C"], g["OC"], g["KH"], g["KW"]), "float")
    if role in ("biases_x", "ones"):
        return Dims(("chan",), (g["OC"],), "float")
    if role == "zeros":
        return Dims(("out_chan",), (g["C"],), "float")
    raise RtErr(f"deconv_role_dims: {role!r} is no view or constant of the matrix path")


def _matrix_tune(tune: OpTune) -> OpTune:
    """The tune the exchanged functions are annotated under: the caller's, without a tile that is this family's own (seven fields, BI = 1)."""
    from dataclasses import replace
    return replace(tune, hip_tile="") if is_grp_tile(tune.hip_tile) and tune.hip_tile.split("x")[0] == "1" else tune


def deconv_calls(op: Op, tune: OpTune, form: str = "") -> list:
    """-> [(function op, {arg: role})] of a Deconvolution in call order.  Direct: [hip_deconv].  Matrix: hip_bconv_in on (filts := filts_x, out_grad_loss := in) into
    out, then hip_chan_affine in place on out with a := ones, b := biases_x -- fma(x, 1, b) is the one add.  `form` forces the path ("" = deconv_form)."""
    if op.get_type() != "Deconvolution":
        raise RtErr(f"deconv_calls: op type {op.get_type()!r} is not Deconvolution")
    op.deconv_geom()
    refuse_deconv_tune(op, tune)
    if (form or deconv_form(op, tune)) == "direct":
        a = op.copy()
        a.set_func_name(DECONV_FUNC)
        return [(a, {"filts": "filts", "biases": "biases", "in": "in", "out": "out"})]
    if not deconv_matrix_can(op):
        raise UnsupErr(f"{op.get_type()}: the matrix path: the exchanged geometry is outside hip_bconv_in's limits (strides of at most {DECONV_MATRIX_MAX_STRIDE})")
    fi = add_bck_conv_annotations(deconv_exchanged_ops(op)[1], _matrix_tune(tune))[0]
    aff = chan_affine_func_op(op.get_dims("out"), 0)
    return [(fi, {"filts": "filts_x", "out_grad_loss": "in", "in_grad_loss": "out"}), (aff, {"in": "out", "a": "ones", "b": "biases_x", "out": "out"})]


def bck_deconv_calls(op: Op, tune: OpTune, form: str = "") -> list:
    """-> [(function op, {arg: role})] of a BckDeconv in BckConv's call order: data, bias and filter gradient.  Direct: hip_deconv_bck_in, hip_deconv_bck_biases,
    hip_deconv_bck_filts (a seven-field tile travels with the filter gradient: its BK / KSL).  Matrix: hip_conv without ReLU on (filts := filts_x, biases := zeros,
    in := out_grad_loss) into in_grad_loss; hip_deconv_bck_biases as it is; hip_bconv_filts on (in := out_grad_loss, out_grad_loss := in) into filts_grad_loss_x."""
    if op.get_type() != "BckDeconv":
        raise RtErr(f"bck_deconv_calls: op type {op.get_type()!r} is not BckDeconv")
    op.deconv_geom()
    refuse_deconv_tune(op, tune)
    fb = op.copy(); fb.set_func_name("hip_deconv_bck_biases")
    bias_call = (fb, {"out_grad_loss": "out_grad_loss", "biases_grad_loss": "biases_grad_loss"})
    if (form or deconv_form(op, tune)) == "direct":
        fi = op.copy(); fi.set_func_name("hip_deconv_bck_in")
        ff = op.copy(); ff.set_func_name("hip_deconv_bck_filts")
        if is_grp_tile(tune.hip_tile):
            ff.str_vals["hip_tile"] = tune.hip_tile
        return [(fi, {"filts": "filts", "out_grad_loss": "out_grad_loss", "in_grad_loss": "in_grad_loss"}), bias_call,
                (ff, {"in": "in", "out_grad_loss": "out_grad_loss", "filts_grad_loss": "filts_grad_loss"})]
    if not deconv_matrix_can(op):
        raise UnsupErr(f"{op.get_type()}: the matrix path: the exchanged geometry is outside hip_bconv_filts' limits (strides of at most {DECONV_MATRIX_MAX_STRIDE})")
    xc, xb = deconv_exchanged_ops(op)
    mt = _matrix_tune(tune)
    fc = add_codegen_annotations(xc, mt)
    fc.nda_vals["conv_has_relu"] = Nda(None, "uint32_t", (0,))
    ff = add_bck_conv_annotations(xb, mt)[2]
    return [(fc, {"filts": "filts_x", "biases": "zeros", "in": "out_grad_loss", "out": "in_grad_loss"}), bias_call,
            (ff, {"in": "out_grad_loss", "out_grad_loss": "in", "filts_grad_loss": "filts_grad_loss_x"})]


def add_deconv_annotations(op: Op, tune: OpTune, form: str = ""):
    """-> the function op(s) of a Deconvolution under the planner's rule (deconv_form), a forcing tile or `form`: hip_deconv, the direct form, as ONE Op; or the tuple
    (hip_bconv_in, hip_chan_affine) of the matrix path, built on the exchanged dims.  deconv_calls gives the same functions with their arg bindings."""
    calls = deconv_calls(op, tune, form)
    return calls[0][0] if len(calls) == 1 else tuple(f for f, _ in calls)


def add_bck_deconv_annotations(op: Op, tune: OpTune, form: str = "") -> tuple:
    """-> (in_op, biases_op, filts_op) of a BckDeconv in BckConv's call order under the planner's rule (deconv_form), a forcing tile or `form`: the direct
    hip_deconv_bck_in, hip_deconv_bck_biases (hip_bconv_biases' sum on out_grad_loss), hip_deconv_bck_filts -- a seven-field tile (BK and KSL) travels with the filter
    gradient --, or the matrix path's hip_conv (zero biases, no ReLU), hip_deconv_bck_biases, hip_bconv_filts on the exchanged dims (bck_deconv_calls: the bindings)."""
    if op.get_type() != "BckDeconv":
        raise RtErr(f"add_bck_deconv_annotations: op type {op.get_type()!r} is not BckDeconv")
    return tuple(f for f, _ in bck_deconv_calls(op, tune, form))


def add_bck_conv_annotations(op: Op, tune: OpTune) -> tuple:
    """-> (in_op, biases_op, filts_op): the three annotated function ops of a BckConv, in the order src/rtc_fwd.cc:398-400 calls them -- the data gradient
    (hip_bconv_in), the bias gradient (hip_bconv_biases), the filter gradient (hip_bconv_filts).  fp32 and reference layouts only (bf16 / channels-last gradients
    are not provided); a tile in the tune travels with the data and filter gradient functions."""
    if op.get_type() != "BckConv":
        raise RtErr(f"add_bck_conv_annotations: op type {op.get_type()!r} is not BckConv")
    if "G" in op.bck_conv_geom():   # group > 1: the grouped family's annotator
        return add_bck_conv_grp_annotations(op, tune)
    if tune.use_be not in ("", "hip") or tune.use_culibs or tune.k1conv or tune.tconv or tune.ipconv:
        raise UnsupErr(f"BckConv variants of op_tune={tune.to_str()} are generated by the reference's CUCL code generator; be=hip provides hip_bconv_*")
    if tune.hip_dtype not in ("", "f32") or tune.hip_layout or tune.hip_algo or tune.hip_out:
        raise UnsupErr("BckConv: fp32 gradients in reference layout only (no bf16, channels-last or Winograd variant)")
    outs = []
    for fn in BCONV_FUNCS:
        a = op.copy()
        a.set_func_name(fn)
        if tune.hip_tile and fn != "hip_bconv_biases":
            a.str_vals["hip_tile"] = tune.hip_tile
        outs.append(a)
    return tuple(outs)


BCONV_FB_FUNC = "hip_bconv_filts_biases"   # the filter and bias gradients in one call (kernels/bconv_fb_f32.hip); opt-in: ConvPipeBck(fuse_filts_biases=True)


def bconv_filts_biases_func_op(op: Op, tune: OpTune) -> Op:
    """-> the annotated hip_bconv_filts_biases function op of a BckConv: ONE call in place of the hip_bconv_biases + hip_bconv_filts pair of add_bck_conv_annotations
    (which stays as it is), writing filts_grad_loss and biases_grad_loss.  On be=hip both operands are staged k-major and K is cut into up to 1024 slices summed in
    slice order; on be=cpu the call is the two single chains.  The same refusals as add_bck_conv_annotations; a tile in the tune travels
    with the function."""
    if op.get_type() != "BckConv":
        raise RtErr(f"bconv_filts_biases_func_op: op type {op.get_type()!r} is not BckConv")
    refuse_grouped(op, what=BCONV_FB_FUNC)
    op.bck_conv_geom()
    if tune.use_be not in ("", "hip") or tune.use_culibs or tune.k1conv or tune.tconv or tune.ipconv:
        raise UnsupErr(f"BckConv variants of op_tune={tune.to_str()} are generated by the reference's CUCL code generator; be=hip provides hip_bconv_*")
    if tune.hip_dtype not in ("", "f32") or tune.hip_layout or tune.hip_algo or tune.hip_out:
        raise UnsupErr("BckConv: fp32 gradients in reference layout only (no bf16, channels-last or Winograd variant)")
    a = op.copy()
    a.set_func_name(BCONV_FB_FUNC)
    if tune.hip_tile:
        a.str_vals["hip_tile"] = tune.hip_tile
    return a


# the native functions of the non-conv backward ops, in the reference's call order (src/rtc_fwd.cc:345-404), and of the two forward ops whose side outputs the
# backward pass reads: the max-pooling argmax out_in_yx (test/rtc/pool.cucl, emit_out_in_yx) and the LRN out_scale_base (test/rtc/lrn.cucl, emit_out_scale_base)
BCK_OP_FUNCS: Dict[str, tuple] = {
    "Spreading": ("hip_spreading",),
    "BckLRN": ("hip_bck_lrn",),
    "ZeroIfNonPos": ("hip_zero_if_non_pos",),
    "SoftmaxWithLoss": ("hip_softmax", "hip_sm_grad_and_loss", "hip_sum_loss_over_imgs"),
    "Pooling": ("hip_pool_yx",),
    "LRN": ("hip_lrn_sb",),
    "Crop": ("hip_crop",),         # Caffe's Crop at axis 2 and its gradient (this backend's own; OP 15 / 16 of kernels/bck_ops_f32.hip): the offsets ride in the op
    "BckCrop": ("hip_crop_bck",),
}


def add_bck_op_annotations(op: Op, tune: OpTune) -> tuple:
    """-> the annotated native function ops of one non-conv op of the gradient pipe, in the order the reference calls them: Spreading -> (hip_spreading,), BckLRN ->
    (hip_bck_lrn,), ZeroIfNonPos -> (hip_zero_if_non_pos,), SoftmaxWithLoss -> (hip_softmax, hip_sm_grad_and_loss, hip_sum_loss_over_imgs) with the intermediate vars
    prob (in's dims) and loss_per_pel (label's dims) added to the op under the reference's names.  A Pooling with emit_out_in_yx=1 gives (hip_pool_yx,) and an LRN with
    emit_out_scale_base=1 (hip_lrn_sb,): the forward functions that also write what Spreading / BckLRN read (out_in_yx / out_scale_base, added to the op with out's
    dims).  Without the emit flag those two ops belong to the forward pipe (conv_pipe.ConvPipeFwd) and are refused here.  fp32, reference layouts only."""
    t = op.get_type()
    if t not in BCK_OP_FUNCS:
        raise RtErr(f"add_bck_op_annotations: op type {t!r} is none of {sorted(BCK_OP_FUNCS)}")
    if tune.use_be not in ("", "hip") or tune.use_culibs:
        raise UnsupErr(f"{t} variants of op_tune={tune.to_str()} are generated by the reference's CUCL code generator; be=hip provides {' / '.join(BCK_OP_FUNCS[t])}")
    if tune.hip_dtype not in ("", "f32") or tune.hip_layout or tune.hip_algo or tune.hip_out:
        raise UnsupErr(f"{t}: fp32 in reference layout only (no bf16, channels-last or Winograd variant)")
    a = op.copy()
    if t in ("Pooling", "Spreading"):
        g = a.pool_geom()
        if t == "Pooling" and not g["emit"] and not g["avg_pool"]:   # (an average has no argmax: the gradient pipe's average poolings keep emit_out_in_yx=0, hip_pool_yx writes -1)
            raise UnsupErr("Pooling with emit_out_in_yx=0 is the forward pipe's (conv_pipe.ConvPipeFwd, POOL_TEMPLATE); hip_pool_yx is the pooling that also writes out_in_yx")
        a.nda_vals["out_in_yx"] = Nda(dims=a.get_dims("out"), tn="float")
    elif t in ("LRN", "BckLRN"):
        g = a.lrn_geom()
        if t == "LRN" and not g["emit"]:
            raise UnsupErr("LRN with emit_out_scale_base=0 is the forward pipe's (conv_pipe.ConvPipeFwd, LRN_TEMPLATE); hip_lrn_sb is the LRN that also writes out_scale_base")
        a.nda_vals["out_scale_base"] = Nda(dims=a.get_dims("out"), tn="float")
    elif t == "ZeroIfNonPos":
        a.zinp_geom()
    elif t in ("Crop", "BckCrop"):
        a.crop_geom()
    else:
        a.softmax_geom()
        a.nda_vals["prob"] = Nda(dims=a.get_dims("in"), tn="float")
        a.nda_vals["loss_per_pel"] = Nda(dims=a.get_dims("label"), tn="float")
    outs = []
    for fn in BCK_OP_FUNCS[t]:
        f = a.copy()
        f.set_func_name(fn)
        outs.append(f)
    return tuple(outs)


# the plumbing ops of the full-net gradient pipe (boda_amd/bck_pipe.py), kept apart from BCK_OP_FUNCS: Reduce sums a fan-out's partial gradients, Dropout / BckDropout are
# the same in-place function, Concat / Split are one copy call per narrow tensor (src/rtc_fwd.cc:267-294,348-364,402-403)
PIPE_OP_FUNCS: Dict[str, tuple] = {
    "Reduce": ("hip_reduce",),
    "Dropout": ("hip_dropout",),
    "BckDropout": ("hip_dropout",),
    "Concat": ("hip_concat",),
    "Split": ("hip_split",),
}


def add_pipe_op_annotations(op: Op, tune: OpTune) -> tuple:
    """-> the annotated native function ops of one plumbing op of the gradient pipe, in call order: Reduce -> (hip_reduce,) with args ins_0 .. ins_{n-1}, out; Dropout /
    BckDropout -> (hip_dropout,) with the in-place arg `inout` (the reference's name) and the by-value det_drop_seed of the CALL; Concat -> one hip_concat per input,
    each carrying that input as `in` and its first output channel as ocix; Split -> one hip_split per output (`out`, icix).  fp32, reference layouts only."""
    t = op.get_type()
    if t not in PIPE_OP_FUNCS:
        raise RtErr(f"add_pipe_op_annotations: op type {t!r} is none of {sorted(PIPE_OP_FUNCS)}")
    if tune.use_be not in ("", "hip") or tune.use_culibs:
        raise UnsupErr(f"{t} variants of op_tune={tune.to_str()} are generated by the reference's CUCL code generator; be=hip provides {PIPE_OP_FUNCS[t][0]}")
    if tune.hip_dtype not in ("", "f32") or tune.hip_layout or tune.hip_algo or tune.hip_out:
        raise UnsupErr(f"{t}: fp32 in reference layout only (no bf16, channels-last or Winograd variant)")
    fn = PIPE_OP_FUNCS[t][0]
    outs = []
    if t == "Reduce":
        op.reduce_geom()
        a = op.copy(); a.set_func_name(fn); outs.append(a)
    elif t in ("Dropout", "BckDropout"):
        op.dropout_geom()
        a = op.copy(); a.nda_vals["inout"] = Nda(dims=a.get_dims("in"), tn="float"); a.set_func_name(fn); outs.append(a)
    else:
        g = op.concat_geom()
        narrow, ix = ("in", "ocix") if t == "Concat" else ("out", "icix")
        for an, c0, _ in g["chans"]:
            a = Op(dict(op.str_vals), {narrow: op.get(an), ("out" if t == "Concat" else "in"): op.get("out" if t == "Concat" else "in")})
            a.set_u32(ix, c0); a.set_func_name(fn); outs.append(a)
    return tuple(outs)


CHAN_AFFINE_FUNC = "hip_chan_affine"


def chan_affine_func_op(dims, relu: int) -> Op:
    """-> the annotated function op of hip_chan_affine on a float img:chan:y:x tensor `dims`: out = in * a[chan] + b[chan] (a multiply, then an add), with relu=1
    followed by x > 0 ? x : +0.  Args in, a, b, out; in and out may be one var.  What ConvPipeFwd runs for a BatchNorm / Scale run of an fp32 net."""
    from .op import Dims
    ch = Dims(("chan",), (dims.dsz("chan"),), "float")
    a = Op({"type": "ChanAffine"}, {"in": Nda(dims=dims, tn="float"), "out": Nda(dims=dims, tn="float"), "a": Nda(dims=ch, tn="float"), "b": Nda(dims=ch, tn="float"),
                                    "relu": Nda(None, "uint32_t", (int(relu),))})
    a.chan_affine_geom()
    a.set_func_name(CHAN_AFFINE_FUNC)
    return a


SGD_UPDATE_FUNC = "hip_sgd_update"
SGD_MAX_TENS = 32
# the solver's function, in a table of its own (PIPE_OP_FUNCS is the gradient pipe's plumbing): no op of a pipe maps to it, ConvPipeBck appends its calls behind the gradient ops
SGD_OP_FUNCS: Dict[str, tuple] = {"SgdUpdate": (SGD_UPDATE_FUNC,)}


def sgd_update_func_op(dims_list, lr_mults=None, decay_mults=None) -> Op:
    """-> the annotated function op of hip_sgd_update over the float tensors `dims_list` (1 to 32, any dims): per tensor i the var args w_i (param), g_i (gradient),
    h_i (momentum history), all of dims_list[i], and the floats lr_mult_i / decay_mult_i (default 1); one var arg hyper, float v=4 = [lr, momentum, weight_decay, unused].
    Per element, every operation one fp32 rounding:  g1 = g + (weight_decay * decay_mult_i) * w;  h' = momentum * h + (lr * lr_mult_i) * g1;  w' = w - h'.
    w_i and h_i are rewritten in place, g_i and hyper only read.  This backend's own: the reference has no solver."""
    from .op import Dims
    dims_list = list(dims_list)
    n = len(dims_list)
    lr_mults = [1.0] * n if lr_mults is None else list(lr_mults)
    decay_mults = [1.0] * n if decay_mults is None else list(decay_mults)
    if len(lr_mults) != n or len(decay_mults) != n:
        raise RtErr(f"sgd_update_func_op: {n} tensors, {len(lr_mults)} lr_mults, {len(decay_mults)} decay_mults")
    v = {"tens_num": Nda(None, "uint32_t", (n,)), "hyper": Nda(dims=Dims(("v",), (4,), "float"), tn="float")}
    for i, d in enumerate(dims_list):
        for b in ("w", "g", "h"):
            v[f"{b}_{i}"] = Nda(dims=d, tn=d.tn)
        v[f"lr_mult_{i}"] = Nda(None, "float", (float(lr_mults[i]),))
        v[f"decay_mult_{i}"] = Nda(None, "float", (float(decay_mults[i]),))
    a = Op({"type": "SgdUpdate"}, v)
    a.sgd_geom()
    a.set_func_name(SGD_UPDATE_FUNC)
    return a


SOLVER_UPDATE_FUNC, GRAD_SUMSQ_FUNC, GRAD_NORM_FUNC = "hip_solver_update", "hip_grad_sumsq", "hip_grad_norm"
SOLVER_TYPES = ("sgd", "nesterov", "adam")
# the solvers beyond plain SGD and global-norm clipping, in a table of their own (SGD_OP_FUNCS is pinned): ConvPipeBck appends their calls behind the gradient ops
SOLVER_OP_FUNCS: Dict[str, tuple] = {"SolverUpdate": (SOLVER_UPDATE_FUNC,), "GradSumsq": (GRAD_SUMSQ_FUNC,), "GradNorm": (GRAD_NORM_FUNC,)}


def _solver_vec(n: int) -> Nda:
    from .op import Dims
    return Nda(dims=Dims(("v",), (int(n),), "float"), tn="float")


def solver_update_func_op(dims_list, solver_type, lr_mults=None, decay_mults=None, clip=False, decoupled_wd=False) -> Op:
    """-> the annotated function op of hip_solver_update over the float tensors `dims_list` (1 to 32, any dims): per tensor i the var args w_i (param), g_i (gradient),
    h_i (first history) and, for solver_type "adam", h2_i (second history), all of dims_list[i], and the floats lr_mult_i / decay_mult_i (default 1); then the var args
    hyper, float v=8 = [lr, momentum, weight_decay, momentum2, delta, corr, clip_gradients, unused], and state, float v=4 = [coef, norm, sumsq, 0], which is read only with
    clip=1 (g0 = coef * g).  solver_type "sgd" | "nesterov" | "adam" rides as a str_val, clip and (adam) decoupled_wd as uint32s.  csrc/kernels/solver_update_f32.hip and
    DESIGN.md section 3.18 state the chains, every operation one fp32 rounding.  w_i, h_i, h2_i are rewritten in place; g_i, hyper and state only read."""
    dims_list = list(dims_list)
    n = len(dims_list)
    lr_mults = [1.0] * n if lr_mults is None else list(lr_mults)
    decay_mults = [1.0] * n if decay_mults is None else list(decay_mults)
    if len(lr_mults) != n or len(decay_mults) != n:
        raise RtErr(f"solver_update_func_op: {n} tensors, {len(lr_mults)} lr_mults, {len(decay_mults)} decay_mults")
    v = {"tens_num": Nda(None, "uint32_t", (n,)), "hyper": _solver_vec(8), "state": _solver_vec(4), "clip": Nda(None, "uint32_t", (1 if clip else 0,))}
    if solver_type == "adam":
        v["decoupled_wd"] = Nda(None, "uint32_t", (1 if decoupled_wd else 0,))
    elif decoupled_wd:
        raise RtErr(f"solver_update_func_op: decoupled_wd is adam's, not {solver_type}'s")
    for i, d in enumerate(dims_list):
        for b in ("w", "g", "h") + (("h2",) if solver_type == "adam" else ()):
            v[f"{b}_{i}"] = Nda(dims=d, tn=d.tn)
        v[f"lr_mult_{i}"] = Nda(None, "float", (float(lr_mults[i]),))
        v[f"decay_mult_{i}"] = Nda(None, "float", (float(decay_mults[i]),))
    a = Op({"type": "SolverUpdate", "solver_type": str(solver_type)}, v)
    a.solver_geom()
    a.set_func_name(SOLVER_UPDATE_FUNC)
    return a


def grad_sumsq_func_op(dims_list, part0, parts_total) -> Op:
    """-> the annotated function op of hip_grad_sumsq over the float tensors `dims_list` (1 to 32): var args g_i, then partials (float v=parts_total, INOUT: the call
    writes only its own slots).  The chunk k of the call -- chunks of 4096 floats numbered over the call's tensors -- leaves its sum of squares in partials[part0 + k]."""
    dims_list = list(dims_list)
    v = {"tens_num": Nda(None, "uint32_t", (len(dims_list),)), "part0": Nda(None, "uint32_t", (int(part0),)), "partials": _solver_vec(parts_total)}
    for i, d in enumerate(dims_list):
        v[f"g_{i}"] = Nda(dims=d, tn=d.tn)
    a = Op({"type": "GradSumsq"}, v)
    a.solver_geom()
    a.set_func_name(GRAD_SUMSQ_FUNC)
    return a


def grad_norm_func_op(parts_total) -> Op:
    """-> the annotated function op of hip_grad_norm: partials (float v=parts_total) and hyper (float v=8) read, state (float v=4) written:
    sumsq = the partials through the written chain; norm = sqrtf(sumsq); coef = norm > clip_gradients ? clip_gradients / norm : 1."""
    a = Op({"type": "GradNorm"}, {"partials": _solver_vec(parts_total), "hyper": _solver_vec(8), "state": _solver_vec(4)})
    a.solver_geom()
    a.set_func_name(GRAD_NORM_FUNC)
    return a


GRAD_ACCUM_FUNC, SOLVER_UPDATE_ACC_FUNC = "hip_grad_accum", "hip_solver_update_acc"
# gradient accumulation over iter_size micro-steps, in a table of its own (SOLVER_OP_FUNCS is pinned): ConvPipeBck(iter_size=n > 1) appends their calls behind the gradient ops
ACCUM_OP_FUNCS: Dict[str, tuple] = {"GradAccum": (GRAD_ACCUM_FUNC,), "SolverUpdateAcc": (SOLVER_UPDATE_ACC_FUNC,)}


def grad_accum_func_op(dims_list) -> Op:
    """-> the annotated function op of hip_grad_accum over the float tensors `dims_list` (1 to 32): per tensor i the var args g_i (the micro-step's gradient, read) and a_i
    (the accumulator, rewritten), then accum, float v=4 = [first, apply, scale, micro], read from device memory.  Per element: first != 0: a' = g (a is not read); else
    a' = a + g, one fp32 add."""
    dims_list = list(dims_list)
    v = {"tens_num": Nda(None, "uint32_t", (len(dims_list),)), "accum": _solver_vec(4)}
    for i, d in enumerate(dims_list):
        v[f"g_{i}"] = Nda(dims=d, tn=d.tn)
        v[f"a_{i}"] = Nda(dims=d, tn=d.tn)
    a = Op({"type": "GradAccum"}, v)
    a.solver_geom()
    a.set_func_name(GRAD_ACCUM_FUNC)
    return a


def solver_update_acc_func_op(dims_list, solver_type, lr_mults=None, decay_mults=None, clip=False, decoupled_wd=False) -> Op:
    """-> the annotated function op of hip_solver_update_acc: solver_update_func_op's op and args (g_i bound to the accumulators) plus the var arg accum, float v=4 =
    [first, apply, scale, micro].  apply == 0: the launch writes nothing.  Otherwise hip_solver_update's chain on gs = scale * g0 (one rounding), g0 = clip ? coef * g : g:
    clip on the summed gradient, then normalise, then regularise (Caffe's order).  With scale == 1 the bits are hip_solver_update's."""
    a = solver_update_func_op(dims_list, solver_type, lr_mults, decay_mults, clip=clip, decoupled_wd=decoupled_wd)
    a = Op(dict(a.str_vals, type="SolverUpdateAcc", func_name=SOLVER_UPDATE_ACC_FUNC), dict(a.nda_vals, accum=_solver_vec(4)))
    a.solver_geom()
    return a


ACCURACY_FUNC, EVAL_ACCUM_FUNC, BN_FOLD_FUNC = "hip_accuracy", "hip_eval_accum", "hip_bn_fold"
# the evaluation pass of the gradient pipe, in a table of its own (the pinned ones stay as they are): what eval_pipe.EvalPipe adds to a driver's forward calls.  This
# backend's own: csrc/kernels/eval_f32.hip states the rules
EVAL_OP_FUNCS: Dict[str, tuple] = {"Accuracy": (ACCURACY_FUNC,), "EvalAccum": (EVAL_ACCUM_FUNC,), "BnFold": (BN_FOLD_FUNC,)}


def accuracy_func_op(in_dims) -> Op:
    """-> the annotated function op of hip_accuracy on the logits `in_dims` (float img:chan:1:1): args in, label (float img:1:1, the loss's own var) read, rank (uint32_t
    img) written.  Per image: the label lf is valid iff lf >= 0 and lf < chan (a NaN is not), L = int(lf); invalid: rank = 0xFFFFFFFF; valid: rank = the number of
    classes c != L with not (in[c] < in[L]) -- ties, and a NaN on either side, count against the true class.  A top-k hit is rank < k."""
    from .op import Dims
    if in_dims.names != ("img", "chan", "y", "x") or in_dims.tn != "float":
        raise RtErr(f"accuracy_func_op: in must be float img:chan:y:x, got {in_dims.tn} {in_dims.pretty()}")
    b = in_dims.dsz("img")
    a = Op({"type": "Accuracy"}, {"in": Nda(dims=in_dims, tn="float"), "label": Nda(dims=Dims(("img", "y", "x"), (b, 1, 1), "float"), tn="float"),
                                  "rank": Nda(dims=Dims(("img",), (b,), "uint32_t"), tn="uint32_t")})
    a.eval_geom()
    a.set_func_name(ACCURACY_FUNC)
    return a


def eval_accum_func_op(img: int, top_k: int) -> Op:
    """-> the annotated function op of hip_eval_accum over `img` images: rank (uint32_t img), loss (float y=1:x=1) and ctl (uint32_t v=4 = [first, 0, 0, 0]) read; counts
    (uint32_t v=4 = [images, hits_top1, hits_topk, batches]) and loss_sum (float v=1) rewritten.  first != 0: counts' = [img, h1, hk, 1], loss_sum' = loss, neither read;
    else counts' = counts + [img, h1, hk, 1] and loss_sum' = loss_sum + loss (one fp32 add).  h1 counts rank < 1, hk rank < top_k (>= 1, rides in the op)."""
    from .op import Dims
    u4 = Dims(("v",), (4,), "uint32_t")
    a = Op({"type": "EvalAccum"}, {"rank": Nda(dims=Dims(("img",), (int(img),), "uint32_t"), tn="uint32_t"), "loss": Nda(dims=Dims(("y", "x"), (1, 1), "float"), tn="float"),
                                   "ctl": Nda(dims=u4, tn="uint32_t"), "counts": Nda(dims=u4, tn="uint32_t"), "loss_sum": Nda(dims=Dims(("v",), (1,), "float"), tn="float"),
                                   "top_k": Nda(None, "uint32_t", (int(top_k),))})
    a.eval_geom()
    a.set_func_name(EVAL_ACCUM_FUNC)
    return a


def bn_fold_func_op(chan: int, eps: float) -> Op:
    """-> the annotated function op of hip_bn_fold over `chan` channels: run_mean, run_var, scale, bias (float chan) read, a, b written -- the bits of
    conv_pipe.fold_affine([("BatchNorm", run_mean, run_var, eps), ("Scale", scale, bias)]), what hip_chan_affine takes.  eps (>= 0) rides in the op."""
    from .op import Dims
    ch = Dims(("chan",), (int(chan),), "float")
    v = {an: Nda(dims=ch, tn="float") for an in ("run_mean", "run_var", "scale", "bias", "a", "b")}
    v["eps"] = Nda(None, "float", (_as_f32(eps),))
    a = Op({"type": "BnFold"}, v)
    a.eval_geom()
    a.set_func_name(BN_FOLD_FUNC)
    return a


DATA_TRANSFORM_FUNC = "hip_data_transform"
# the input transform of the gradient pipe, in a table of its own again: what a ConvPipeBck built with input_transform= puts in front of its step.  This backend's
# own: csrc/kernels/data_f32.hip states the rule
DATA_OP_FUNCS: Dict[str, tuple] = {"DataTransform": (DATA_TRANSFORM_FUNC,)}


def data_transform_func_op(src_dims, crop_yx, mean_dims, scale: float) -> Op:
    """-> the annotated function op of hip_data_transform: src (uint8_t img:y:x:chan or img:chan:y:x, `src_dims`), plan (uint32_t img:v=4 = y_off, x_off, mirror,
    unused) and mean (`mean_dims`: float chan, or chan:y:x at the source size) read, out (float img:chan:y:x at the crop size `crop_yx`) written.  Per output element
    (i, c, y, x): yo = min(plan[i][0], H - ch), xo = min(plan[i][1], W - cw), sy = yo + y, sx = xo + (plan[i][2] != 0 ? cw - 1 - x : x), out = ((float)src[i, sy, sx, c] -
    mean[c] or mean[c, sy, sx]) * scale, two fp32 roundings.  scale rides in the op."""
    from .op import Dims
    if src_dims.tn != "uint8_t" or src_dims.names not in (("img", "y", "x", "chan"), ("img", "chan", "y", "x")):
        raise RtErr(f"data_transform_func_op: src must be uint8_t img:y:x:chan or img:chan:y:x, got {src_dims.tn} {src_dims.pretty()}")
    b, c = src_dims.dsz("img"), src_dims.dsz("chan")
    a = Op({"type": "DataTransform"}, {"src": Nda(dims=src_dims, tn="uint8_t"), "plan": Nda(dims=Dims(("img", "v"), (b, 4), "uint32_t"), tn="uint32_t"),
                                       "mean": Nda(dims=mean_dims, tn=mean_dims.tn),
                                       "out": Nda(dims=Dims(("img", "chan", "y", "x"), (b, c, int(crop_yx[0]), int(crop_yx[1])), "float"), tn="float"),
                                       "scale": Nda(None, "float", (_as_f32(scale),))})
    a.data_geom()
    a.set_func_name(DATA_TRANSFORM_FUNC)
    return a


SOFTMAX_LOSS_FWD_FUNC, LOSS_NORM_FUNC, SOFTMAX_LOSS_BCK_FUNC = "hip_softmax_loss_fwd", "hip_loss_norm", "hip_softmax_loss_bck"
# the full SoftmaxWithLoss, in a table of its own: what a head with a bck_graph.LossSpec lowers to (loss_weight, ignore_label, planes, the four normalisers).  This
# backend's own: csrc/kernels/loss_f32.hip states the rules
LOSS_OP_FUNCS: Dict[str, tuple] = {"SoftmaxLossFwd": (SOFTMAX_LOSS_FWD_FUNC,), "LossNorm": (LOSS_NORM_FUNC,), "SoftmaxLossBck": (SOFTMAX_LOSS_BCK_FUNC,)}
LOSS_FUNCS = tuple(v[0] for v in LOSS_OP_FUNCS.values())


def _loss_func_op(t: str, in_dims, spec, args) -> Op:
    """One of the three, over the logits `in_dims` (float img:chan:y:x); spec: anything with weight / ignore_label / normalization (bck_graph.LossSpec, whose check()
    runs first).  Every op of the family carries the whole spec; the kernels take from it what they need."""
    from .op import Dims
    if in_dims.names != ("img", "chan", "y", "x") or in_dims.tn != "float":
        raise RtErr(f"{t}: in must be float img:chan:y:x, got {in_dims.tn} {in_dims.pretty()}")
    if hasattr(spec, "check"):
        spec.check()
    ig = spec.ignore_label
    if ig is not None and (isinstance(ig, bool) or not isinstance(ig, Integral)):
        raise RtErr(f"{t}: ignore_label must be an integer or None, got {ig!r}")
    try:
        w = float(spec.weight)
    except (TypeError, ValueError):
        raise RtErr(f"{t}: weight must be a finite number, got {spec.weight!r}")
    plane = Dims(("img", "y", "x"), (in_dims.dsz("img"), in_dims.dsz("y"), in_dims.dsz("x")), "float")
    dims = {"in": in_dims, "prob": in_dims, "in_grad_loss": in_dims, "label": plane, "loss_per_pel": plane, "loss": Dims(("y", "x"), (1, 1), "float"), "loss_state": Dims(("v",), (4,), "float")}
    v = {an: Nda(dims=dims[an], tn="float") for an in args}
    v.update({"weight": Nda(None, "float", (_as_f32(w) if w == w and abs(w) != float("inf") else w,)), "has_ignore": Nda(None, "uint32_t", (0 if ig is None else 1,)),
              "ignore_label": Nda(None, "float", (_as_f32(0 if ig is None else int(ig)),))})
    a = Op({"type": t, "normalization": str(spec.normalization)}, v)
    a.loss_geom()
    a.set_func_name(LOSS_OP_FUNCS[t][0])
    return a


def softmax_loss_fwd_func_op(in_dims, spec) -> Op:
    """-> hip_softmax_loss_fwd over the logits `in_dims`: in, label (float img:y:x of in's plane) read; prob (in's dims) and loss_per_pel (label's dims) written.  Per
    pel: prob = exp(in - m) / sum under the TRUE channel maximum m; a label equal to spec.ignore_label is ignored (loss_per_pel +0), one in [0, chan) is valid
    (-logf(max(prob[L], FLT_MIN))), any other, a NaN included, is invalid (-logf(FLT_MIN)) and reads no memory.  Planes of 64 pels or more take the pel form (one thread
    per pel), smaller ones the wave form (one wave per pel)."""
    return _loss_func_op("SoftmaxLossFwd", in_dims, spec, ("in", "label", "prob", "loss_per_pel"))


def loss_norm_func_op(in_dims, spec) -> Op:
    """-> hip_loss_norm for the head on `in_dims`: label, loss_per_pel read; loss (float y=1:x=1) and loss_state (float v=4 = Z, s, count, sum) written.  count: the pels
    that are not ignored; Z = valid: max(1, count) | full: img * y * x | batch_size: img | none: 1; s = weight / Z (one fp32 divide); loss = sum / Z, unweighted.  The
    sum is one written chain (csrc/kernels/loss_f32.hip)."""
    return _loss_func_op("LossNorm", in_dims, spec, ("label", "loss_per_pel", "loss", "loss_state"))


def softmax_loss_bck_func_op(in_dims, spec) -> Op:
    """-> hip_softmax_loss_bck for the head on `in_dims`: prob, label, loss_state read; in_grad_loss = ignored ? +0 : (prob - [c == L]) * s written, two fp32 roundings,
    s = loss_state[1] read on the device (never passed by value: one captured graph serves every count of ignored pels)."""
    return _loss_func_op("SoftmaxLossBck", in_dims, spec, ("prob", "label", "loss_state", "in_grad_loss"))


# the training BatchNorm of the gradient pipe and the Eltwise-SUM gradient, in a table of their own (PIPE_OP_FUNCS is pinned): what bck_pipe.ConvPipeBck runs for a
# BatchNorm + Scale (+ ReLU) run and its gradient, and for a BckEltwise.  This backend's own arithmetic: csrc/kernels/bn_f32.hip and DESIGN.md section 3.15 state it
BN_OP_FUNCS: Dict[str, tuple] = {
    "BnStats": ("hip_bn_stats",),
    "BnFwd": ("hip_bn_fwd",),
    "BnBckSums": ("hip_bn_bck_sums",),
    "BnBckIn": ("hip_bn_bck_in",),
    "FanOut": ("hip_fan_out",),
}
# BatchNorm on its running pair (fine-tuning with frozen statistics), a table of its own again (BN_OP_FUNCS is pinned): what ConvPipeBck runs for a
# [BatchNorm, Scale (, ReLU)] run that Freeze(bn_global_stats=...) lists
BNF_OP_FUNCS: Dict[str, tuple] = {
    "BnfPrep": ("hip_bnf_prep",),
    "BnfBck": ("hip_bnf_bck",),
    "BnfBckIn": ("hip_bnf_bck_in",),
}
BNF_FUNCS = tuple(v[0] for v in BNF_OP_FUNCS.values())
BN_FUNCS = tuple(v[0] for v in BN_OP_FUNCS.values()) + BNF_FUNCS


def _as_f32(v: float) -> float:
    """The value a float scalar of an op holds: rounded to fp32 once, here."""
    import struct
    return struct.unpack("f", struct.pack("f", float(v)))[0]


def _bn_func_op(t: str, dims, tens, chans, **scalars) -> Op:
    from .op import Dims
    if dims.names != ("img", "chan", "y", "x") or dims.tn != "float":
        raise RtErr(f"{t}: in must be float img:chan:y:x, got {dims.tn} {dims.pretty()}")
    ch = Dims(("chan",), (dims.dsz("chan"),), "float")
    v = {an: Nda(dims=dims, tn="float") for an in tens}
    v.update({an: Nda(dims=ch, tn="float") for an in chans})
    for k, (tn, val) in scalars.items():
        v[k] = Nda(None, tn, (_as_f32(val) if tn == "float" else val,))
    a = Op({"type": t}, v)
    a.bn_geom()
    a.set_func_name((BN_OP_FUNCS[t] if t in BN_OP_FUNCS else BNF_OP_FUNCS[t])[0])
    return a


def bn_stats_func_op(dims, eps: float, maf: float, slab: int = 0) -> Op:
    """-> the annotated function op of hip_bn_stats on a float img:chan:y:x tensor `dims`: args in (IN), mean, inv_std (OUT), run_mean, run_var (INOUT), the per-channel
    ones float chan=C.  mean = S1 / N, var = S2 / N (two passes, biased), inv_std = 1 / sqrtf(var + eps), run' = maf * run + (1 - maf) * (mean | var * N / (N - 1)).
    slab > 0 (a multiple of 4) forces the slab length of the sums' chain; 0: the planner's."""
    return _bn_func_op("BnStats", dims, ("in",), ("mean", "inv_std", "run_mean", "run_var"), eps=("float", float(eps)), maf=("float", float(maf)), slab=("uint32_t", int(slab)))


def bn_fwd_func_op(dims, relu: int) -> Op:
    """-> hip_bn_fwd: out = ((in - mean[c]) * inv_std[c]) * scale[c] + bias[c], with relu=1 followed by y > 0 ? y : +0.  Args in, mean, inv_std, scale, bias (IN), out
    (OUT); in and out may be one var."""
    return _bn_func_op("BnFwd", dims, ("in", "out"), ("mean", "inv_std", "scale", "bias"), relu=("uint32_t", int(relu)))


def bn_bck_sums_func_op(dims, slab: int = 0) -> Op:
    """-> hip_bn_bck_sums: scale_grad_loss = SUM dy * xh, bias_grad_loss = SUM dy per channel, xh recomputed from in, mean, inv_std.  Args in, mean, inv_std,
    out_grad_loss (IN), scale_grad_loss, bias_grad_loss (OUT)."""
    return _bn_func_op("BnBckSums", dims, ("in", "out_grad_loss"), ("mean", "inv_std", "scale_grad_loss", "bias_grad_loss"), slab=("uint32_t", int(slab)))


def bn_bck_in_func_op(dims) -> Op:
    """-> hip_bn_bck_in: dx = (scale * inv_std) * ((dy - bias_grad_loss / N) - xh * (scale_grad_loss / N)).  Args in, mean, inv_std, scale, scale_grad_loss,
    bias_grad_loss, out_grad_loss (IN), in_grad_loss (OUT, may be out_grad_loss's var)."""
    return _bn_func_op("BnBckIn", dims, ("in", "out_grad_loss", "in_grad_loss"), ("mean", "inv_std", "scale", "scale_grad_loss", "bias_grad_loss"))


def bnf_prep_func_op(dims, eps: float) -> Op:
    """-> hip_bnf_prep, a BatchNorm on its running pair: args run_mean, run_var (IN, only read), mean, inv_std (OUT), float chan=C of the tensor `dims` (which the op
    carries as `in`; no var is bound to it).  mean = run_mean (the bits), inv_std = 1 / sqrtf(run_var + eps): what hip_bn_fwd and hip_bnf_bck then take."""
    return _bn_func_op("BnfPrep", dims, ("in",), ("run_mean", "run_var", "mean", "inv_std"), eps=("float", float(eps)))


def bnf_bck_func_op(dims, slab: int = 0) -> Op:
    """-> hip_bnf_bck, the whole backward pass of a [BatchNorm on its running pair, Scale] run in ONE pass over in and out_grad_loss: scale_grad_loss = SUM dy * xh,
    bias_grad_loss = SUM dy in hip_bn_bck_sums' chain (the same bits), dx = (scale * inv_std) * dy.  Args in, mean, inv_std, scale, out_grad_loss (IN), in_grad_loss (OUT,
    may be out_grad_loss's var), scale_grad_loss, bias_grad_loss (OUT)."""
    return _bn_func_op("BnfBck", dims, ("in", "out_grad_loss", "in_grad_loss"), ("mean", "inv_std", "scale", "scale_grad_loss", "bias_grad_loss"), slab=("uint32_t", int(slab)))


def bnf_bck_in_func_op(dims) -> Op:
    """-> hip_bnf_bck_in, the data gradient alone (both Scale params frozen): dx = (scale * inv_std) * dy.  Args inv_std, scale, out_grad_loss (IN), in_grad_loss (OUT,
    may be out_grad_loss's var); the op carries `in` for the dims, no var is bound to it."""
    return _bn_func_op("BnfBckIn", dims, ("in", "out_grad_loss", "in_grad_loss"), ("inv_std", "scale"))


def fan_out_func_op(dims, n: int) -> Op:
    """-> hip_fan_out, the gradient of an Eltwise SUM: args in (IN), outs_0 .. outs_{n-1} (OUT), 2 <= n <= 8, float tensors of equal dims; every outs_i = in bit for bit."""
    if dims.tn != "float":
        raise RtErr(f"FanOut: in has type {dims.tn}: fp32 only")
    v = {"in": Nda(dims=dims, tn="float"), "outs_num": Nda(None, "uint32_t", (int(n),))}
    for i in range(int(n)):
        v[f"outs_{i}"] = Nda(dims=dims, tn="float")
    a = Op({"type": "FanOut"}, v)
    a.bn_geom()
    a.set_func_name("hip_fan_out")
    return a


# the training BatchNorm over img CHUNKS, a table of its own again (BN_OP_FUNCS is pinned): the hip_bn_* functions' args and formulas, with the
# three per-channel sums in the chunked chain -- the batch cut into `chunks` pieces as a multi-device backend cuts it over its devices, every chunk's total by the plan of
# the chunk's own dims, the totals added in chunk order.  The same bits on be=cpu, on one device and on `chunks` devices; chunks=1 is the hip_bn_* chain
BNC_OP_FUNCS: Dict[str, tuple] = {
    "BncStats": ("hip_bnc_stats",),
    "BncFwd": ("hip_bnc_fwd",),
    "BncBckSums": ("hip_bnc_bck_sums",),
    "BncBckIn": ("hip_bnc_bck_in",),
}
BNC_FUNCS = tuple(v[0] for v in BNC_OP_FUNCS.values())
BNC_MAX_CHUNKS = 64


def _bnc_func_op(twin: Op, t: str, **u32s) -> Op:
    """The hip_bn_* function op `twin` (checked by its constructor) as the hip_bnc_* function op of type t, with the uint32 scalars given added."""
    a = Op(dict(twin.str_vals, type=t, func_name=BNC_OP_FUNCS[t][0]), dict(twin.nda_vals))
    for k, val in u32s.items():
        a.nda_vals[k] = Nda(None, "uint32_t", (int(val),))
    return a


def _bnc_chunks(t: str, chunks: int) -> int:
    if not 1 <= int(chunks) <= BNC_MAX_CHUNKS:
        raise UnsupErr(f"{t}: chunks={chunks}: 1 to {BNC_MAX_CHUNKS} img chunks")
    return int(chunks)


def bnc_stats_func_op(dims, eps: float, maf: float, chunks: int, slab: int = 0) -> Op:
    """-> hip_bnc_stats: hip_bn_stats' args and formulas on the WHOLE batch's `dims`, S1 and S2 in the chunked chain over `chunks` img chunks (chunk i = images
    [T * i / chunks, T * (i + 1) / chunks); an empty chunk adds no term); fN, the unbiasing factor and S2's mean are the whole batch's.  slab > 0 forces the slab length of
    every chunk's plan.  On `(be=hip,devices=...)` chunks must be the device count."""
    return _bnc_func_op(bn_stats_func_op(dims, eps, maf, slab), "BncStats", chunks=_bnc_chunks("BncStats", chunks))


def bnc_fwd_func_op(dims, relu: int) -> Op:
    """-> hip_bnc_fwd: hip_bn_fwd, whose vars may hold fewer images than `dims` (an img shard): independent per image."""
    return _bnc_func_op(bn_fwd_func_op(dims, relu), "BncFwd")


def bnc_bck_sums_func_op(dims, chunks: int, slab: int = 0) -> Op:
    """-> hip_bnc_bck_sums: hip_bn_bck_sums with both sums in the chunked chain over `chunks` img chunks (bnc_stats_func_op)."""
    return _bnc_func_op(bn_bck_sums_func_op(dims, slab), "BncBckSums", chunks=_bnc_chunks("BncBckSums", chunks))


def bnc_bck_in_func_op(dims) -> Op:
    """-> hip_bnc_bck_in: hip_bn_bck_in dividing by the element count of the WHOLE batch, which `dims` gives; its vars may hold fewer images (an img shard)."""
    return _bnc_func_op(bn_bck_in_func_op(dims), "BncBckIn")


ZINP_FLAG = "zero_if_in_non_pos"   # uint32 of a function op: in_grad_loss[e] = in[e] > 0 ? g[e] : +0, hip_zero_if_non_pos's rule applied on the producer's store
ZINP_FUNCS = ("hip_bconv_in", "hip_spreading", "hip_bck_lrn")   # the functions that write an in_grad_loss with the dims of their op's forward input `in`


def has_zinp_flag(fop: Op) -> bool:
    return fop.has(ZINP_FLAG) and fop.get_u32(ZINP_FLAG) != 0


def fuse_zero_if_in_non_pos(fop: Op) -> Op:
    """-> a copy of an annotated hip_bconv_in / hip_spreading / hip_bck_lrn function op with zero_if_in_non_pos=1: the function then writes
    in_grad_loss[e] = in[e] > 0 ? g[e] : +0, g being what the unflagged function writes and `in` the op's forward input -- the ReLU gradient (hip_zero_if_non_pos
    with cond = in) folded into the store.  hip_bconv_in and hip_spreading take `in` as one more var arg (pipe_func_args); hip_bck_lrn reads it already."""
    fn = fop.get_func_name() if fop.has_func_name() else ""
    if is_grouped(fop):
        refuse_grouped(fop, what=f"fuse_zero_if_in_non_pos ({fn or fop.get_type()})")
    if fn not in ZINP_FUNCS:
        raise RtErr(f"fuse_zero_if_in_non_pos: {fn or fop.get_type()!r} is none of {', '.join(ZINP_FUNCS)} (the functions whose in_grad_loss has the dims of their forward input)")
    if fop.get_dims("in") != fop.get_dims("in_grad_loss"):
        raise RtErr(f"fuse_zero_if_in_non_pos: {fn}: in and in_grad_loss dims differ")
    a = fop.copy()
    a.nda_vals[ZINP_FLAG] = Nda(None, "uint32_t", (1,))
    return a


OPERANDS_VAL = "hip_operands"   # str_val of a function op, travels with it like hip_tile: "" / "f32" the function as it is | "bf16" bf16 operands, fp32 sums
BF16_OPERAND_FUNCS = ("hip_bconv_in", BCONV_FB_FUNC)   # the functions that have a bf16-operand form (kernels/bconv_in_bf16.hip, kernels/bconv_fb_bf16.hip)


def has_bf16_operands(fop: Op) -> bool:
    return fop.str_vals.get(OPERANDS_VAL, "") == "bf16"


def bf16_operands(fop: Op) -> Op:
    """-> a copy of an annotated hip_bconv_in / hip_bconv_filts_biases function op with hip_operands=bf16: tensors and arg list stay as they are (fp32, reference
    layouts); the operands of the products are rounded to bf16 (round-to-nearest-even) while they are staged and the sums stay fp32 -- v_mfma_f32_32x32x16_bf16 on
    be=hip, the template loops on rounded copies on be=cpu.  The bias gradient of the fused call is summed from the unrounded out_grad_loss, bit for bit the fp32 call's
    chain; zero_if_in_non_pos=1 composes (the condition is read unrounded).  The data and filter gradients are held to a bound, not to bits.
    hip_bconv_filts and hip_bconv_biases have no bf16 form of their own: UnsupErr, as on the backends."""
    fn = fop.get_func_name() if fop.has_func_name() else ""
    if is_grouped(fop):
        refuse_grouped(fop, what=f"bf16_operands ({fn or fop.get_type()})")
    if fn in ("hip_bconv_filts", "hip_bconv_biases"):
        raise UnsupErr(f"{fn}: hip_operands=bf16: the filter and bias gradients have their bf16-operand form as ONE call, {BCONV_FB_FUNC} "
                       f"(cnn_op.bconv_filts_biases_func_op); hip_bconv_filts and hip_bconv_biases are fp32 only")
    if fn not in BF16_OPERAND_FUNCS:
        raise RtErr(f"bf16_operands: {fn or fop.get_type()!r} is none of {', '.join(BF16_OPERAND_FUNCS)} (the functions that have a bf16-operand form)")
    a = fop.copy()
    a.str_vals[OPERANDS_VAL] = "bf16"
    return a


SEED_VAR_FLAG = "seed_from_var"   # uint32 of a hip_dropout function op: the hash seed is the word of the var arg det_drop_seed_var + the by-value det_drop_seed (wraps)
SEED_VAR_ARG = "det_drop_seed_var"


def has_seed_var_flag(fop: Op) -> bool:
    return fop.has(SEED_VAR_FLAG) and fop.get_u32(SEED_VAR_FLAG) != 0


def seed_from_var(fop: Op) -> Op:
    """-> a copy of an annotated hip_dropout function op (a Dropout's or a BckDropout's) with seed_from_var=1: the call takes one more var arg behind inout,
    det_drop_seed_var (uint32_t, dims v=1, added to the op), and hashes with seed = that word + the by-value det_drop_seed, a uint32 add that wraps.  A flagged call
    with word w and by-value o writes the bits of the unflagged call with by-value (w + o) mod 2^32.  The seed then lives in device memory: a launch captured into a
    hipGraph freezes the by-value argument, not the word."""
    fn = fop.get_func_name() if fop.has_func_name() else ""
    if fn != "hip_dropout":
        raise RtErr(f"seed_from_var: {fn or fop.get_type()!r} is not hip_dropout (the only function that takes a seed)")
    from .op import Dims
    a = fop.copy()
    a.nda_vals[SEED_VAR_FLAG] = Nda(None, "uint32_t", (1,))
    a.nda_vals[SEED_VAR_ARG] = Nda(dims=Dims(("v",), (1,), "uint32_t"), tn="uint32_t")
    return a


IMG_SHARDS_FLAG = "img_shards"   # uint32 of a function op: the call's img-leading vars may be shards of a batch, and the call leaves the bits of the whole batch's call
IMG_SHARDS_FUNCS = ("hip_bconv_filts", "hip_bconv_biases", "hip_sm_grad_and_loss", "hip_sum_loss_over_imgs", "hip_dropout")   # the functions that are not independent per image


def has_img_shards_flag(fop: Op) -> bool:
    return fop.has(IMG_SHARDS_FLAG) and fop.get_u32(IMG_SHARDS_FLAG) != 0


def on_img_shards(fop: Op) -> Op:
    """-> a copy of an annotated hip_bconv_filts / hip_bconv_biases / hip_sm_grad_and_loss / hip_sum_loss_over_imgs / hip_dropout function op with img_shards=1: the
    five functions a multi-device backend (`(be=hip,devices=...)`, vars sharded on img) refuses, because they are not independent per image.  A flagged call runs there
    and leaves, for the whole batch, the bits DESIGN.md section 3.13 writes down: dropout, the loss gradient, loss_per_pel and loss those of the one-device call; a
    filter / bias gradient the per-shard gradients of the unflagged function added in device order, plain fp32 adds from the first shard's.  No new var args
    (pipe_func_args is unchanged).  be=cpu and a single be=hip device accept the flag and run the unflagged function: one shard, a chain of one term."""
    fn = fop.get_func_name() if fop.has_func_name() else ""
    if fn not in IMG_SHARDS_FUNCS:
        raise RtErr(f"on_img_shards: {fn or fop.get_type()!r} is none of {', '.join(IMG_SHARDS_FUNCS)} (every other function is independent per image and runs on img shards as it is)")
    a = fop.copy()
    a.nda_vals[IMG_SHARDS_FLAG] = Nda(None, "uint32_t", (1,))
    return a


def pipe_func_args(fop: Op) -> tuple:
    """The (arg, IN | OUT | REF | VAL) list of an annotated function op: NATIVE_ARGS; for hip_reduce its ins_0 .. ins_{n-1} followed by out; for a hip_bconv_in /
    hip_spreading with zero_if_in_non_pos=1 the var arg `in` in front of in_grad_loss; for a hip_dropout with seed_from_var=1 the var arg det_drop_seed_var behind inout;
    for a hip_conv_nhwc with nhwc_residual=1 the var arg `res` in front of out; for hip_sgd_update w_0 g_0 h_0 .. w_{n-1} g_{n-1} h_{n-1} hyper, with the kind INOUT
    (read and written in place) for w_i and h_i."""
    fn = fop.get_func_name()
    if fn == SGD_UPDATE_FUNC:
        per = tuple(x for i in range(fop.get_u32("tens_num")) for x in ((f"w_{i}", "INOUT"), (f"g_{i}", "IN"), (f"h_{i}", "INOUT")))
        return per + NATIVE_ARGS[fn]
    if fn in (SOLVER_UPDATE_FUNC, GRAD_SUMSQ_FUNC, GRAD_ACCUM_FUNC, SOLVER_UPDATE_ACC_FUNC) and fop.has("tens_num"):   # (an op without tens_num: the fixed args alone)
        adam = fop.str_vals.get("solver_type") == "adam"
        one = lambda i: ((f"w_{i}", "INOUT"), (f"g_{i}", "IN"), (f"h_{i}", "INOUT")) + (((f"h2_{i}", "INOUT"),) if adam else ()) if fn in (SOLVER_UPDATE_FUNC, SOLVER_UPDATE_ACC_FUNC) else \
            ((f"g_{i}", "IN"), (f"a_{i}", "INOUT")) if fn == GRAD_ACCUM_FUNC else ((f"g_{i}", "IN"),)
        return tuple(x for i in range(fop.get_u32("tens_num")) for x in one(i)) + NATIVE_ARGS[fn]
    if fn == "hip_fan_out":
        return NATIVE_ARGS[fn] + tuple((an, "OUT") for an in fop.multi_names("outs"))
    if fn == "hip_dropout" and has_seed_var_flag(fop):
        return NATIVE_ARGS[fn][:1] + ((SEED_VAR_ARG, "IN"),) + NATIVE_ARGS[fn][1:]
    if fn == "hip_reduce":
        return tuple((an, "IN") for an in fop.multi_names("ins")) + NATIVE_ARGS[fn]
    if fn in ("hip_bconv_in", "hip_spreading") and has_zinp_flag(fop):
        return NATIVE_ARGS[fn][:-1] + (("in", "IN"),) + NATIVE_ARGS[fn][-1:]
    if fn == "hip_conv_nhwc" and fop.has("nhwc_residual") and fop.get_u32("nhwc_residual"):     # (nhwc.fuse_residual: the shortcut, in front of out)
        return NATIVE_ARGS[fn][:-1] + (("res", "IN"),) + NATIVE_ARGS[fn][-1:]
    return NATIVE_ARGS[fn]


# arg tables of the native side-door functions (the stubs test/rtc/cublas_sgemm.cucl:1-4, cudnn_conv.cucl:1-7).  The backend keeps the same facts in one table of its own,
# csrc/native_funcs.h; tests/test_native_funcs_cpu.py holds this table, pipe_func_args and the *_FUNCS tuples of this file to it
NATIVE_ARGS: Dict[str, tuple] = {
    "hip_sgemm": (("a", "IN"), ("b", "IN"), ("c", "OUT")),
    "cublas_sgemm": (("a", "IN"), ("b", "IN"), ("c", "OUT")),
    "hip_sgemm_bf16": (("a", "IN"), ("b", "IN"), ("c", "OUT")),
    "hip_conv_bf16": (("filts", "IN"), ("biases", "IN"), ("in", "IN"), ("stride", "REF"), ("in_pad", "REF"), ("out", "OUT")),
    "hip_conv": (("filts", "IN"), ("biases", "IN"), ("in", "IN"), ("stride", "REF"), ("in_pad", "REF"), ("out", "OUT")),
    "cudnn_conv": (("filts", "IN"), ("biases", "IN"), ("in", "IN"), ("stride", "REF"), ("in_pad", "REF"), ("out", "OUT")),
    "hip_conv_winograd": (("filts", "IN"), ("biases", "IN"), ("in", "IN"), ("stride", "REF"), ("in_pad", "REF"), ("out", "OUT")),
    "hip_conv_nhwc": (("filts", "IN"), ("biases", "IN"), ("in", "IN"), ("stride", "REF"), ("in_pad", "REF"), ("out", "OUT")),
    "hip_conv_k1_chain": (("filts", "IN"), ("biases", "IN"), ("filts2", "IN"), ("biases2", "IN"), ("in", "IN"), ("stride", "REF"), ("in_pad", "REF"), ("out", "OUT")),
    "hip_conv_filts_kmajor": (("filts", "IN"), ("filts_km", "OUT")),
    # BckConv's gradients: the reference templates' arg lists (test/rtc/BckConv_in_grad_loss.cucl, BckConv_filts_grad_loss.cucl, BckConv_biases_grad_loss.cucl)
    "hip_bconv_in": (("filts", "IN"), ("out_grad_loss", "IN"), ("stride", "REF"), ("in_pad", "REF"), ("in_grad_loss", "OUT")),
    "hip_bconv_filts": (("in", "IN"), ("out_grad_loss", "IN"), ("stride", "REF"), ("in_pad", "REF"), ("filts_grad_loss", "OUT")),
    "hip_bconv_filts_biases": (("in", "IN"), ("out_grad_loss", "IN"), ("stride", "REF"), ("in_pad", "REF"), ("filts_grad_loss", "OUT"), ("biases_grad_loss", "OUT")),
    # a Convolution / BckConv with group > 1: the lists of hip_conv, hip_bconv_in and hip_bconv_filts without their optional args
    "hip_conv_grp": (("filts", "IN"), ("biases", "IN"), ("in", "IN"), ("stride", "REF"), ("in_pad", "REF"), ("out", "OUT")),
    "hip_bconv_in_grp": (("filts", "IN"), ("out_grad_loss", "IN"), ("stride", "REF"), ("in_pad", "REF"), ("in_grad_loss", "OUT")),
    "hip_bconv_filts_grp": (("in", "IN"), ("out_grad_loss", "IN"), ("stride", "REF"), ("in_pad", "REF"), ("filts_grad_loss", "OUT")),
    # a Deconvolution / BckDeconv: the lists of hip_conv and of BckConv's three gradients without their optional args; Caffe's Crop and its gradient
    "hip_deconv": (("filts", "IN"), ("biases", "IN"), ("in", "IN"), ("stride", "REF"), ("in_pad", "REF"), ("out", "OUT")),
    "hip_deconv_bck_in": (("filts", "IN"), ("out_grad_loss", "IN"), ("stride", "REF"), ("in_pad", "REF"), ("in_grad_loss", "OUT")),
    "hip_deconv_bck_filts": (("in", "IN"), ("out_grad_loss", "IN"), ("stride", "REF"), ("in_pad", "REF"), ("filts_grad_loss", "OUT")),
    "hip_deconv_bck_biases": (("out_grad_loss", "IN"), ("biases_grad_loss", "OUT")),
    "hip_crop": (("in", "IN"), ("out", "OUT")),
    "hip_crop_bck": (("out_grad_loss", "IN"), ("in_grad_loss", "OUT")),
    "hip_bconv_biases": (("out_grad_loss", "IN"), ("biases_grad_loss", "OUT")),   # filts as [K + 128][out_chan padded to 4]: what hip_conv's optional filts_km arg takes
    # the non-conv backward ops, in their reference templates' arg order (test/rtc/pool.cucl, lrn.cucl, spreading.cucl, bck_lrn.cucl, ZeroIfNonPos.cucl, softmax.cucl,
    # sm_grad_and_loss.cucl, sum_loss_over_imgs.cucl); the by-value scalars of those templates (avg_pool, alpha, ...) ride in the op
    "hip_pool_yx": (("in", "IN"), ("kern_sz", "REF"), ("stride", "REF"), ("in_pad", "REF"), ("out", "OUT"), ("out_in_yx", "OUT")),
    "hip_lrn_sb": (("in", "IN"), ("out", "OUT"), ("out_scale_base", "OUT")),
    "hip_spreading": (("out", "IN"), ("out_grad_loss", "IN"), ("out_in_yx", "IN"), ("kern_sz", "REF"), ("stride", "REF"), ("in_pad", "REF"), ("in_grad_loss", "OUT")),
    "hip_bck_lrn": (("in", "IN"), ("out", "IN"), ("out_grad_loss", "IN"), ("out_scale_base", "IN"), ("in_grad_loss", "OUT")),
    "hip_zero_if_non_pos": (("in", "IN"), ("cond", "IN"), ("out", "OUT")),
    "hip_softmax": (("in", "IN"), ("prob", "OUT")),
    "hip_sm_grad_and_loss": (("prob", "IN"), ("label", "IN"), ("in_grad_loss", "OUT"), ("loss_per_pel", "OUT")),
    "hip_sum_loss_over_imgs": (("loss_per_pel", "IN"), ("loss", "OUT")),
    # the gradient pipe's plumbing (test/rtc/dropout.cucl; the copy calls of src/rtc_fwd.cc:267-294).  VAL: a by-value scalar of the CALL (uint32 det_drop_seed).
    # hip_reduce's list depends on the op (ins_0 .. ins_{n-1}, out), hip_dropout's on seed_from_var (inout, det_drop_seed_var, det_drop_seed): pipe_func_args
    "hip_reduce": (("out", "OUT"),),
    "hip_dropout": (("inout", "OUT"), ("det_drop_seed", "VAL")),
    "hip_concat": (("in", "IN"), ("out", "OUT")),
    "hip_split": (("in", "IN"), ("out", "OUT")),
    # the forward pipe's BatchNorm / Scale runs (this backend's own; relu rides in the op)
    "hip_chan_affine": (("in", "IN"), ("a", "IN"), ("b", "IN"), ("out", "OUT")),
    # the solver's update (this backend's own).  The list depends on the op: w_i (INOUT) g_i (IN) h_i (INOUT) per tensor in front of hyper (pipe_func_args)
    "hip_sgd_update": (("hyper", "IN"),),
    # the solvers beyond plain SGD and global-norm clipping (this backend's own).  In front of these (pipe_func_args): w_i (INOUT) g_i (IN) h_i (INOUT) and, for adam,
    # h2_i (INOUT) per tensor | g_i (IN) per tensor.  partials is INOUT for hip_grad_sumsq: a call writes its own slots and leaves the others
    "hip_solver_update": (("hyper", "IN"), ("state", "IN")),
    "hip_grad_sumsq": (("partials", "INOUT"),),
    "hip_grad_norm": (("partials", "IN"), ("hyper", "IN"), ("state", "OUT")),
    # gradient accumulation (this backend's own).  In front of these (pipe_func_args): g_i (IN) a_i (INOUT) per tensor | hip_solver_update's w_i g_i h_i [h2_i]
    "hip_grad_accum": (("accum", "IN"),),
    "hip_solver_update_acc": (("hyper", "IN"), ("state", "IN"), ("accum", "IN")),
    # the evaluation pass (this backend's own; top_k / eps ride in the op).  counts and loss_sum are read unless ctl[0] != 0, and rewritten
    "hip_accuracy": (("in", "IN"), ("label", "IN"), ("rank", "OUT")),
    "hip_eval_accum": (("rank", "IN"), ("loss", "IN"), ("ctl", "IN"), ("counts", "INOUT"), ("loss_sum", "INOUT")),
    "hip_bn_fold": (("run_mean", "IN"), ("run_var", "IN"), ("scale", "IN"), ("bias", "IN"), ("a", "OUT"), ("b", "OUT")),
    # the full SoftmaxWithLoss of a head with a LossSpec (this backend's own; weight / normalization / has_ignore / ignore_label ride in the op)
    "hip_softmax_loss_fwd": (("in", "IN"), ("label", "IN"), ("prob", "OUT"), ("loss_per_pel", "OUT")),
    "hip_loss_norm": (("label", "IN"), ("loss_per_pel", "IN"), ("loss", "OUT"), ("loss_state", "OUT")),
    "hip_softmax_loss_bck": (("prob", "IN"), ("label", "IN"), ("loss_state", "IN"), ("in_grad_loss", "OUT")),
    # the input transform (this backend's own; scale rides in the op)
    "hip_data_transform": (("src", "IN"), ("plan", "IN"), ("mean", "IN"), ("out", "OUT")),
    # the training BatchNorm and the Eltwise-SUM gradient (this backend's own; eps / maf / slab / relu ride in the op).  hip_fan_out's list depends on the op: in,
    # then outs_0 .. outs_{n-1} (pipe_func_args)
    "hip_bn_stats": (("in", "IN"), ("mean", "OUT"), ("inv_std", "OUT"), ("run_mean", "INOUT"), ("run_var", "INOUT")),
    "hip_bn_fwd": (("in", "IN"), ("mean", "IN"), ("inv_std", "IN"), ("scale", "IN"), ("bias", "IN"), ("out", "OUT")),
    "hip_bn_bck_sums": (("in", "IN"), ("mean", "IN"), ("inv_std", "IN"), ("out_grad_loss", "IN"), ("scale_grad_loss", "OUT"), ("bias_grad_loss", "OUT")),
    "hip_bn_bck_in": (("in", "IN"), ("mean", "IN"), ("inv_std", "IN"), ("scale", "IN"), ("scale_grad_loss", "IN"), ("bias_grad_loss", "IN"), ("out_grad_loss", "IN"), ("in_grad_loss", "OUT")),
    "hip_fan_out": (("in", "IN"),),
    # BatchNorm on its running pair (this backend's own; eps / slab ride in the op)
    "hip_bnf_prep": (("run_mean", "IN"), ("run_var", "IN"), ("mean", "OUT"), ("inv_std", "OUT")),
    "hip_bnf_bck": (("in", "IN"), ("mean", "IN"), ("inv_std", "IN"), ("scale", "IN"), ("out_grad_loss", "IN"), ("in_grad_loss", "OUT"), ("scale_grad_loss", "OUT"), ("bias_grad_loss", "OUT")),
    "hip_bnf_bck_in": (("inv_std", "IN"), ("scale", "IN"), ("out_grad_loss", "IN"), ("in_grad_loss", "OUT")),
    # the training BatchNorm over img chunks: the args of their hip_bn_* twins (chunks rides in the op)
    "hip_bnc_stats": (("in", "IN"), ("mean", "OUT"), ("inv_std", "OUT"), ("run_mean", "INOUT"), ("run_var", "INOUT")),
    "hip_bnc_fwd": (("in", "IN"), ("mean", "IN"), ("inv_std", "IN"), ("scale", "IN"), ("bias", "IN"), ("out", "OUT")),
    "hip_bnc_bck_sums": (("in", "IN"), ("mean", "IN"), ("inv_std", "IN"), ("out_grad_loss", "IN"), ("scale_grad_loss", "OUT"), ("bias_grad_loss", "OUT")),
    "hip_bnc_bck_in": (("in", "IN"), ("mean", "IN"), ("inv_std", "IN"), ("scale", "IN"), ("scale_grad_loss", "IN"), ("bias_grad_loss", "IN"), ("out_grad_loss", "IN"), ("in_grad_loss", "OUT")),
}


K1_CHAIN_FUNC = "hip_conv_k1_chain"
FILTS_KMAJOR_FUNC = "hip_conv_filts_kmajor"


def filts_kmajor_func_op(conv: Op) -> Op:
    """-> the hip_conv_filts_kmajor function op of an annotated hip_conv function: filts -> their k-major copy, [K + 128][out_chan padded to 4].  A grouped op is
    refused by name: hip_conv_grp reads its filters as they are."""
    refuse_grouped(conv, what=FILTS_KMAJOR_FUNC)
    return Op({"type": "Convolution", "func_name": FILTS_KMAJOR_FUNC}, {})


def k1_chain_applies(a: Op, b: Op) -> bool:
    """Can the fp32 convolutions a -> b (b reads a's output) run as one hip_conv_k1_chain launch?  Mirrors plan_k1_chain (csrc/native_kernels.cc): both 1x1 /
    stride 1 / unpadded, at most 96 intermediate channels, at most 128 out_chans, both filter images (k-major, odd pitch) within the LDS."""
    if is_grouped(a) or is_grouped(b):   # (a grouped convolution passes the chain by)
        return False
    ga, gb = a.conv_geom(), b.conv_geom()
    for g in (ga, gb):
        if (g["KH"], g["KW"], g["SY"], g["SX"], g["PY"], g["PX"]) != (1, 1, 1, 1, 0, 0):
            return False
    if gb["C"] != ga["OC"] or (gb["H"], gb["W"], gb["B"]) != (ga["OH"], ga["OW"], ga["B"]) or ga["OH"] * ga["OW"] < 4:
        return False
    if not (1 <= ga["OC"] <= 96 and 1 <= gb["OC"] <= 128):
        return False
    ocb, ocb2 = -(-ga["OC"] // 32), -(-gb["OC"] // 32)
    kp, kp2 = (ga["C"] + 1) // 2 * 2, (ga["OC"] + 1) // 2 * 2
    return 4 * (kp * ((ocb * 32) | 1) + ocb * 32 + kp2 * ((ocb2 * 32) | 1) + ocb2 * 32) <= 160 * 1024


def annotate_k1_chain(a: Op, b: Op, relu_a: int, relu_b: int) -> Op:
    """The function op of hip_conv_k1_chain for the annotated hip_conv ops a -> b: a's in / filts / biases / stride / in_pad, b's filts / biases as filts2 /
    biases2, b's out; conv_has_relu / conv_has_relu2 the two fused ReLUs."""
    for x in (a, b):
        refuse_grouped(x, what=K1_CHAIN_FUNC)
    if not k1_chain_applies(a, b):
        raise UnsupErr("hip_conv_k1_chain: two chained 1x1 / stride-1 / unpadded convolutions with <= 96 intermediate channels and <= 128 out_chans")
    c = a.copy()
    c.nda_vals["filts2"] = b.nda_vals["filts"]; c.nda_vals["biases2"] = b.nda_vals["biases"]; c.nda_vals["out"] = b.nda_vals["out"]
    if "out_chans" in b.nda_vals:
        c.nda_vals["out_chans"] = b.nda_vals["out_chans"]
    from .op import Nda
    c.nda_vals["conv_has_relu"] = Nda(None, "uint32_t", (int(relu_a),)); c.nda_vals["conv_has_relu2"] = Nda(None, "uint32_t", (int(relu_b),))
    c.str_vals["func_name"] = K1_CHAIN_FUNC
    c.str_vals.pop("hip_tile", None)
    return c


def f32_pool_fusable(conv: Op, pool_in, kern, stride, in_pad, avg_pool) -> bool:
    """Can a max pooling (input dims pool_in, window kern, stride, padding in_pad) be taken into the annotated fp32 hip_conv function that alone reads its output?
    Mirrors apply_f32_pool (csrc/native_run.cc) / plan_conv (csrc/native_plan.cc): max, no pooling pad, windows of at most 3 x 3 that tile the plane exactly (no clipped last window),
    and a convolution that takes the LDS-patch form (stride 1 in x, more than one tap, not output 1 x 1)."""
    if avg_pool or tuple(in_pad) != (0, 0) or conv.get_func_name() != "hip_conv" or "hip_tile" in conv.str_vals or conv.has("hip_pool"):
        return False
    kh, kw = kern; sy, sx = stride; H, W = pool_in.dsz("y"), pool_in.dsz("x")
    if not (1 <= kh <= 3 and 1 <= kw <= 3 and kh * kw >= 2 and sy >= 1 and sx >= 1 and H >= kh and W >= kw and (H - kh) % sy == 0 and (W - kw) % sx == 0):
        return False
    g = conv.conv_geom()
    if (g["H"], g["W"]) != ((H - kh) // sy + 1, (W - kw) // sx + 1) or pool_in.dsz("chan") != g["C"] or pool_in.dsz("img") != g["B"]:
        return False
    return g["SX"] == 1 and g["KH"] * g["KW"] >= 2 and g["KH"] >= g["SY"] and not (g["OH"] == 1 and g["OW"] == 1)


def fuse_f32_pool(conv: Op, pool_in, kern, stride) -> None:
    """In place: the annotated fp32 hip_conv function takes the max pooling in front of it (f32_pool_fusable).  Its `in` becomes the POOLING's input and the window travels
    with the function: uint32 hip_pool, dims pool_sz / pool_stride.  The reference runs two functions (test/rtc/pool.cucl, then the conv: src/rtc_fwd.cc:545-549); here a
    patch element of the convolution's LDS input patch is the window maximum, formed while the patch is staged (kernels/gemm_conv_f32.hip, PKH).  Bit-identical."""
    from .op import Dims, Nda
    refuse_grouped(conv, what="fuse_f32_pool (a pooling fused in front of hip_conv)")
    none = lambda y, x: Nda(Dims(("y", "x"), (y, x), "none"), "none")
    conv.nda_vals["in"] = Nda(dims=pool_in, tn=pool_in.tn)
    conv.set_u32("hip_pool", 1)
    conv.nda_vals["pool_sz"] = none(*kern); conv.nda_vals["pool_stride"] = none(*stride)


import os as _os
if _os.environ.get("BODAHIP_TILE_WISDOM"):
    set_tile_wisdom(_os.environ["BODAHIP_TILE_WISDOM"])
