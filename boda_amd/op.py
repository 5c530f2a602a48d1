"""Op descriptions: dims_t / nda_t text forms, lexp grammar, op_base_t.

Restates (behaviour only) the reference's
  * lexp grammar                      src/lexp.cc (value = leaf | '(' name '=' value {',' ...} ')', '\\' escapes)
  * nda / dims text forms             src/nesi.cc:661-785, printer src/boda_base.cc:403-440
  * op_base_t {str_vals, nda_vals}    src/op_base.H:9-43, ordering src/op_base.cc:16-23
  * legacy '(type=T,dims_vals=(...))' form still used by test/sgemm-ops-{micro,tiny,small,full}.txt
  * Convolution / sgemm arg tables    src/conv_util.cc:25-35
  * the non-conv forward / backward op tables (Pooling, LRN, Spreading, BckLRN, ZeroIfNonPos, SoftmaxWithLoss, Reduce, Concat, Split, Dropout, BckDropout)   src/conv_util.cc:33-64
"""
from __future__ import annotations
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Tuple, Union

TYPE_SIZES = {"none": 0, "half": 2, "bfloat16": 2, "float": 4, "double": 8, "int32_t": 4, "uint32_t": 4, "uint16_t": 2, "uint8_t": 1}


class RtErr(RuntimeError):
    """rt_err: fatal error (src/boda_base.H:98)."""


class UnsupErr(RuntimeError):
    """unsup_err: 'this configuration is unsupported'; callers may catch and record (src/boda_base.H:105)."""


# ------------------------------------------------------------------------------------------------
# lexp
# ------------------------------------------------------------------------------------------------
Lexp = Union[str, List[Tuple[str, "Lexp"]]]


def parse_lexp(s: str) -> Lexp:
    """Parse one lexp.  Leaf -> str; list -> [(name, value), ...] (order preserved)."""
    pos = 0
    n = len(s)

    def parse_value() -> Lexp:
        nonlocal pos
        if pos < n and s[pos] == "(":
            pos += 1
            items: List[Tuple[str, Lexp]] = []
            if pos < n and s[pos] == ")":
                pos += 1
                return items
            while True:
                name = []
                while pos < n and s[pos] != "=":
                    if s[pos] in "(),":
                        raise RtErr(f"lexp: invalid char {s[pos]!r} in name at {pos}: {s[:pos+1]!r}")
                    if s[pos] == "\\":
                        pos += 1
                    name.append(s[pos])
                    pos += 1
                if pos >= n:
                    raise RtErr("lexp: unexpected end in name")
                pos += 1  # '='
                val = parse_value()
                items.append(("".join(name), val))
                if pos >= n:
                    raise RtErr("lexp: unexpected end of input in list")
                if s[pos] == ",":
                    pos += 1
                    continue
                if s[pos] == ")":
                    pos += 1
                    return items
                raise RtErr(f"lexp: expected ',' or ')' at {pos}")
        leaf = []
        while pos < n and s[pos] not in ",)":
            if s[pos] == "(":
                raise RtErr(f"lexp: unexpected '(' in leaf at {pos}")
            if s[pos] == "\\":
                pos += 1
            leaf.append(s[pos])
            pos += 1
        return "".join(leaf)

    v = parse_value()
    if pos != n:
        raise RtErr(f"lexp: trailing characters at {pos}: {s[pos:]!r}")
    return v


def _kv(l: Lexp) -> Dict[str, Lexp]:
    if isinstance(l, str):
        raise RtErr(f"lexp: expected list, got leaf {l!r}")
    d: Dict[str, Lexp] = {}
    for k, v in l:
        if k in d:
            raise RtErr(f"lexp: duplicate key {k!r}")
        d[k] = v
    return d


# ------------------------------------------------------------------------------------------------
# dims_t / nda_t
# ------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Dims:
    """Row-major named dims + element type name (src/boda_base.H:498-690). Unpadded strides only."""
    names: Tuple[str, ...] = ()
    sizes: Tuple[int, ...] = ()
    tn: str = "float"

    def __post_init__(self):
        if len(self.names) != len(self.sizes):
            raise RtErr("dims: names/sizes length mismatch")
        if self.tn not in TYPE_SIZES:
            raise RtErr(f"dims: unknown type name {self.tn!r}")

    @staticmethod
    def make(tn: str = "float", **kw: int) -> "Dims":
        return Dims(tuple(kw.keys()), tuple(int(v) for v in kw.values()), tn)

    def dsz(self, name: str) -> int:
        try:
            return self.sizes[self.names.index(name)]
        except ValueError:
            raise RtErr("dim not found:" + name)

    def has(self, name: str) -> bool:
        return name in self.names

    @property
    def strides(self) -> Tuple[int, ...]:
        st, acc = [], 1
        for sz in reversed(self.sizes):
            st.append(acc)
            acc *= sz
        return tuple(reversed(st))

    def dstride(self, name: str) -> int:
        return self.strides[self.names.index(name)]

    def dims_prod(self) -> int:
        p = 1
        for s in self.sizes:
            p *= s
        return p

    def bytes_sz(self) -> int:
        return self.dims_prod() * TYPE_SIZES[self.tn]

    def is_zeros(self) -> bool:
        return all(s == 0 for s in self.sizes)

    def with_tn(self, tn: str) -> "Dims":
        return Dims(self.names, self.sizes, tn)

    def param_str(self) -> str:
        return "(" + ",".join(f"{n}={s}" for n, s in zip(self.names, self.sizes)) + ")"

    def pretty(self) -> str:
        return "DIMS[" + ":".join(f"{n}={s}" for n, s in zip(self.names, self.sizes)) + "]"


@dataclass
class Nda:
    """nda_t restricted to what op descriptions need: dims (+ optional small value list)."""
    dims: Optional[Dims] = None  # None => scalar
    tn: str = "float"
    v: Optional[Tuple[Union[int, float], ...]] = None

    def key(self):
        return (self.tn, self.dims.names if self.dims else (), self.dims.sizes if self.dims else (), self.v or ())

    def scalar(self):
        if self.v is None or len(self.v) != 1:
            raise RtErr("nda: not a scalar-with-value")
        return self.v[0]

    def to_str(self) -> str:
        """Canonical printer: `tn` only when dims absent or tn != float (src/boda_base.cc:421-440)."""
        parts = []
        if self.dims is None or self.tn != "float":
            parts.append(f"tn={self.tn}")
        if self.dims is not None:
            parts.append("dims=" + self.dims.param_str())
        if self.v is not None:
            parts.append("v=" + ":".join(_fmt_val(x, self.tn) for x in self.v))
        return "(" + ",".join(parts) + ")"


def _f32_shortest(x: float) -> float:
    """The shortest decimal that reads back as the same fp32 value (what the backend's op printer writes, csrc/lexp.cc)."""
    import struct
    rt = lambda v: struct.unpack("f", struct.pack("f", v))[0]
    try:
        want = rt(x)
    except OverflowError:
        return x
    for p in range(1, 10):
        s = float("%.*e" % (p - 1, want))
        if rt(s) == want:
            return s
    return want


def _fmt_val(x, tn: str) -> str:
    if tn == "float" and float(x) == float(x) and abs(float(x)) != float("inf"):
        x = _f32_shortest(float(x))
    if tn in ("float", "double", "half"):
        if tn == "float" and abs(float(x)) >= 1e15:   # (the backend's printer writes such values in exponent form)
            return repr(float(x))
        return repr(float(x)) if float(x) != int(float(x)) else str(int(float(x)))
    return str(int(x))


def _parse_dims(l: Lexp, tn: str) -> Tuple[Dims, str]:
    names, sizes = [], []
    for k, v in (l if not isinstance(l, str) else []):
        if k == "__tn__":
            tn = str(v)
            continue
        names.append(k)
        sizes.append(int(v))
    return Dims(tuple(names), tuple(sizes), tn), tn


def parse_nda(l: Lexp) -> Nda:
    d = _kv(l)
    unknown = set(d) - {"tn", "dims", "v"}
    if unknown:
        raise RtErr(f"nda: unknown fields {sorted(unknown)}")
    has_dims = "dims" in d
    tn = str(d["tn"]) if "tn" in d else ("float" if has_dims else None)
    if tn is None:
        raise RtErr("nda: scalar without tn")
    dims = None
    if has_dims:
        dims, tn = _parse_dims(d["dims"], tn)
    vals = None
    if "v" in d:
        toks = [t for t in str(d["v"]).replace(" ", ":").split(":") if t]
        conv = float if tn in ("float", "double", "half") else int
        vals = tuple(conv(t) for t in toks)
        n_expect = dims.dims_prod() if dims is not None else 1
        if len(vals) != n_expect:
            raise RtErr(f"nda: expected {n_expect} values, got {len(vals)}")
    return Nda(dims=dims, tn=tn, v=vals)


# ------------------------------------------------------------------------------------------------
# op_base_t
# ------------------------------------------------------------------------------------------------
# (type) -> (bottom/input arg names, top/output arg names, required non-tensor fields); src/conv_util.cc:25-35
_POOL_PARAMS = ("kern_sz", "stride", "in_pad", "avg_pool", "emit_out_in_yx")
_LRN_PARAMS = ("alpha", "beta", "k", "local_size", "emit_out_scale_base")
OP_INFO = {
    "Convolution": (("in", "filts", "biases"), ("out",), ("kern_sz", "stride", "in_pad", "out_chans")),
    "sgemm": (("a", "b"), ("c",), ()),
    # { in, filts, biases, out_grad_loss } -> { in_grad_loss, filts_grad_loss, biases_grad_loss }: each output has its matching input's dims (src/conv_util.cc:65-66,411-416)
    "BckConv": (("in", "filts", "biases", "out_grad_loss"), ("in_grad_loss", "filts_grad_loss", "biases_grad_loss"), ("kern_sz", "stride", "in_pad", "out_chans")),
    # this backend's own (the reference knows the type and its shapes, src/conv_util.cc:35, but has no function for it): in img:chan=C:y:x, filts in_chan=C:out_chan=OC:y:x
    # (Caffe's blob), out img:OC:(H-1)*SY+KH-2*PY:(W-1)*SX+KW-2*PX; no group, no fused ReLU.  BckDeconv: every gradient with its matching input's dims
    "Deconvolution": (("in", "filts", "biases"), ("out",), ("kern_sz", "stride", "in_pad", "out_chans")),
    "BckDeconv": (("in", "filts", "biases", "out_grad_loss"), ("in_grad_loss", "filts_grad_loss", "biases_grad_loss"), ("kern_sz", "stride", "in_pad", "out_chans")),
    # this backend's own: Caffe's Crop at axis 2 -- out is the window of in at `offset` (dims y:x, tn none) -- and its gradient, +0 outside the window
    "Crop": (("in",), ("out",), ("offset",)),
    "BckCrop": (("out_grad_loss",), ("in_grad_loss",), ("offset",)),
    # the non-conv ops of the gradient pipe, with the reference's arg names (src/conv_util.cc:33-64).  Scalars (uint32 / float ndas) and kern_sz / stride / in_pad ride in the op.
    # Spreading is the pooling gradient and BckLRN the LRN gradient: each carries its forward op's parameters; ZeroIfNonPos is the ReLU gradient.
    "Pooling": (("in",), ("out",), _POOL_PARAMS),
    "LRN": (("in",), ("out",), _LRN_PARAMS),
    "Spreading": (("out", "out_grad_loss", "in"), ("in_grad_loss",), _POOL_PARAMS),
    "BckLRN": (("in", "out", "out_grad_loss"), ("in_grad_loss",), _LRN_PARAMS),
    "ZeroIfNonPos": (("in", "cond"), ("out",), ()),
    "SoftmaxWithLoss": (("in", "label"), ("in_grad_loss", "loss"), ()),
    # the plumbing ops of the gradient pipe (src/conv_util.cc:39-40,55-58).  Reduce and Concat read the MULTI arg `ins`, Split writes the multi arg `outs`: such an arg is
    # carried under the reference's flattened names ins_0 .. ins_{ins_num-1} / outs_0 .. outs_{outs_num-1} (Op.multi_names); the tuples here list the fixed args only
    "Reduce": ((), ("out",), ("ins_num",)),
    "Concat": ((), ("out",), ("ins_num",)),
    "Split": (("in",), (), ("outs_num",)),
    "Dropout": (("in",), ("out",), ("dropout_ratio",)),
    "BckDropout": (("in",), ("out",), ("dropout_ratio",)),
    # this backend's own (the forward pipe's BatchNorm / Scale runs at inference, conv_pipe.fold_affine): out = in * a[chan] + b[chan], then a ReLU if relu=1
    "ChanAffine": (("in", "a", "b"), ("out",), ("relu",)),
    # this backend's own (the reference has no solver): the SGD update of up to 32 tensors.  The multi args w / g / h ride flattened as w_0 .. w_{tens_num-1} etc., with the
    # floats lr_mult_i / decay_mult_i beside them; w and h are read and written, g and hyper (float v=4: lr, momentum, weight_decay, unused) read
    "SgdUpdate": (("hyper",), (), ("tens_num",)),
    # this backend's own: the solvers beyond plain SGD and global-norm clipping (csrc/kernels/solver_update_f32.hip states the chains).  SolverUpdate: the multi args w / g / h
    # (and h2 for solver_type=adam) flattened as for SgdUpdate; hyper float v=8 (lr, momentum, weight_decay, momentum2, delta, corr, clip_gradients, unused), state float v=4
    # (coef, norm, sumsq, 0).  GradSumsq: the multi arg g, one partial per chunk of 4096 elements into partials[part0 ..].  GradNorm: partials -> state
    "SolverUpdate": (("hyper", "state"), (), ("tens_num",)),
    "GradSumsq": ((), ("partials",), ("tens_num", "part0")),
    "GradNorm": (("partials", "hyper"), ("state",), ()),
    # this backend's own: gradient accumulation over iter_size micro-steps.  accum float v=4 (first, apply, scale, micro).  GradAccum: the multi args g (read) and a (the
    # accumulators, rewritten).  SolverUpdateAcc: a SolverUpdate that also reads accum, its g the accumulators
    "GradAccum": (("accum",), (), ("tens_num",)),
    "SolverUpdateAcc": (("hyper", "state", "accum"), (), ("tens_num",)),
    # this backend's own: the training BatchNorm of the gradient pipe and the gradient of an Eltwise SUM (csrc/kernels/bn_f32.hip states the arithmetic).  The per-channel
    # args are float chan=C; run_mean / run_var are read and written; slab (0: the planner's) forces the slab length of the per-channel sums; FanOut writes the multi arg outs
    "BnStats": (("in",), ("mean", "inv_std", "run_mean", "run_var"), ("eps", "maf", "slab")),
    "BnFwd": (("in", "mean", "inv_std", "scale", "bias"), ("out",), ("relu",)),
    "BnBckSums": (("in", "mean", "inv_std", "out_grad_loss"), ("scale_grad_loss", "bias_grad_loss"), ("slab",)),
    "BnBckIn": (("in", "mean", "inv_std", "scale", "scale_grad_loss", "bias_grad_loss", "out_grad_loss"), ("in_grad_loss",), ()),
    "FanOut": (("in",), (), ("outs_num",)),
    # this backend's own: BatchNorm on its running pair (fine-tuning with frozen statistics; csrc/kernels/bn_f32.hip).  BnfPrep and BnfBckIn bind no var to `in`: their op
    # carries it for the dims alone.  in_grad_loss may be out_grad_loss's var
    "BnfPrep": (("run_mean", "run_var"), ("mean", "inv_std"), ("eps",)),
    "BnfBck": (("in", "mean", "inv_std", "scale", "out_grad_loss"), ("in_grad_loss", "scale_grad_loss", "bias_grad_loss"), ("slab",)),
    "BnfBckIn": (("inv_std", "scale", "out_grad_loss"), ("in_grad_loss",), ()),
    # this backend's own: the evaluation pass of the gradient pipe (csrc/kernels/eval_f32.hip states the rules).  Accuracy: the rank of the true class per image from the
    # logits and the loss's label var.  EvalAccum: the batch's counts and loss into counts (uint32 v=4) / loss_sum (float v=1), which it reads and rewrites, under ctl (uint32
    # v=4 = first, 0, 0, 0).  BnFold: a [BatchNorm, Scale] run's running statistics and scale / bias as the pair (a, b) of conv_pipe.fold_affine
    "Accuracy": (("in", "label"), ("rank",), ()),
    "EvalAccum": (("rank", "loss", "ctl"), ("counts", "loss_sum"), ("top_k",)),
    "BnFold": (("run_mean", "run_var", "scale", "bias"), ("a", "b"), ("eps",)),
    # this backend's own: the input transform of the gradient pipe (csrc/kernels/data_f32.hip states the rule).  src uint8_t img:y:x:chan or img:chan:y:x, plan uint32_t
    # img:v=4 = (y_off, x_off, mirror, unused), mean float chan or chan:y:x at the source size; out float img:chan:y:x at the crop size = ((float)src - mean) * scale
    "DataTransform": (("src", "plan", "mean"), ("out",), ("scale",)),
    # this backend's own: the full SoftmaxWithLoss of a head with a LossSpec (csrc/kernels/loss_f32.hip states the rules): loss_weight, ignore_label, planes larger than
    # 1 x 1 and Caffe's four normalisers.  in / prob / in_grad_loss float img:chan:y:x, label / loss_per_pel float img:y:x, loss float y=1:x=1, loss_state float v=4 =
    # (Z, s, count, sum).  The spec rides in every one of them: the float weight, the str_val normalization, the uint32 has_ignore and the float ignore_label
    "SoftmaxLossFwd": (("in", "label"), ("prob", "loss_per_pel"), ("weight", "has_ignore", "ignore_label")),
    "LossNorm": (("label", "loss_per_pel"), ("loss", "loss_state"), ("weight", "has_ignore", "ignore_label")),
    "SoftmaxLossBck": (("prob", "label", "loss_state"), ("in_grad_loss",), ("weight", "has_ignore", "ignore_label")),
}
BN_TYPES = ("BnStats", "BnFwd", "BnBckSums", "BnBckIn", "FanOut")
BNF_TYPES = ("BnfPrep", "BnfBck", "BnfBckIn")
SOLVER_TYPES = ("SolverUpdate", "GradSumsq", "GradNorm", "GradAccum", "SolverUpdateAcc")
EVAL_TYPES = ("Accuracy", "EvalAccum", "BnFold")
DATA_TYPES = ("DataTransform",)
LOSS_TYPES = ("SoftmaxLossFwd", "LossNorm", "SoftmaxLossBck")
LOSS_NORMALIZATIONS = ("valid", "full", "batch_size", "none")
SOLVER_CHUNK = 4096   # floats of one tensor a workgroup owns; one partial sum of squares per chunk


_NON_GEMM_TYPES = ("Crop", "BckCrop", "Pooling", "LRN", "Spreading", "BckLRN", "ZeroIfNonPos", "SoftmaxWithLoss", "Reduce", "Concat", "Split", "Dropout", "BckDropout", "ChanAffine", "SgdUpdate") + BN_TYPES + BNF_TYPES + SOLVER_TYPES + EVAL_TYPES + DATA_TYPES + LOSS_TYPES


@dataclass
class Op:
    str_vals: Dict[str, str] = field(default_factory=dict)
    nda_vals: Dict[str, Nda] = field(default_factory=dict)

    # -- op_base_t convenience accessors (src/op_base.cc:25-51); same names
    def has(self, an: str) -> bool:
        return an in self.nda_vals

    def get(self, an: str) -> Nda:
        if an not in self.nda_vals:
            raise RtErr(f"op: missing nda_val {an!r}")
        return self.nda_vals[an]

    def get_dims(self, an: str) -> Dims:
        d = self.get(an).dims
        if d is None:
            raise RtErr(f"op: {an!r} is a scalar, has no dims")
        return d

    def set_dims(self, an: str, dims: Dims) -> None:
        if an in self.nda_vals:
            raise RtErr(f"op: {an!r} already set")  # must_insert
        self.nda_vals[an] = Nda(dims=dims, tn=dims.tn)

    def reset_dims(self, an: str, dims: Dims) -> None:
        self.get(an)
        self.nda_vals[an] = Nda(dims=dims, tn=dims.tn)

    def get_u32(self, an: str) -> int:
        return int(self.get(an).scalar())

    def set_u32(self, an: str, v: int) -> None:
        if an in self.nda_vals:
            raise RtErr(f"op: {an!r} already set")
        self.nda_vals[an] = Nda(dims=None, tn="uint32_t", v=(int(v),))

    def get_str(self, k: str) -> str:
        if k not in self.str_vals:
            raise RtErr(f"op: missing str_val {k!r}")
        return self.str_vals[k]

    def get_type(self) -> str:
        return self.get_str("type")

    def has_func_name(self) -> bool:
        return "func_name" in self.str_vals

    def get_func_name(self) -> str:
        return self.get_str("func_name")

    def set_func_name(self, fn: str) -> None:
        if "func_name" in self.str_vals:
            raise RtErr("op: func_name already set")
        self.str_vals["func_name"] = fn

    def copy(self) -> "Op":
        return Op(dict(self.str_vals), {k: Nda(v.dims, v.tn, v.v) for k, v in self.nda_vals.items()})

    def sort_key(self):
        """op_base_t::operator< : str_vals map, then nda_vals map, lexicographic (src/op_base.cc:16-23)."""
        return (tuple(sorted(self.str_vals.items())), tuple((k, self.nda_vals[k].key()) for k in sorted(self.nda_vals)))

    def __eq__(self, o):
        return isinstance(o, Op) and self.sort_key() == o.sort_key()

    def to_str(self) -> str:
        """Canonical one-line form; std::map order (sorted keys), as NESI prints it."""
        sv = ",".join(f"{k}={self.str_vals[k]}" for k in sorted(self.str_vals))
        nv = ",".join(f"{k}={self.nda_vals[k].to_str()}" for k in sorted(self.nda_vals))
        return f"(str_vals=({sv}),nda_vals=({nv}))"

    # -- shape helpers for the two op types on the hot path
    def conv_geom(self) -> dict:
        """Named geometry of a Convolution; validates out = (in + 2*pad - k)/stride + 1 (src/conv_util.cc:167-173)."""
        i, f, o = self.get_dims("in"), self.get_dims("filts"), self.get_dims("out")
        st, pad = self.get_dims("stride"), self.get_dims("in_pad")
        g = dict(B=i.dsz("img"), C=i.dsz("chan"), H=i.dsz("y"), W=i.dsz("x"),
                 OC=f.dsz("out_chan"), KH=f.dsz("y"), KW=f.dsz("x"),
                 SY=st.dsz("y"), SX=st.dsz("x"), PY=pad.dsz("y"), PX=pad.dsz("x"),
                 OH=o.dsz("y"), OW=o.dsz("x"))
        if self.has("hip_pool") and self.get_u32("hip_pool"):   # a max pooling fused in front (cnn_op.fuse_f32_pool): `in` is the POOLING's input, H x W the pooled plane
            ks, ps = self.get_dims("pool_sz"), self.get_dims("pool_stride")
            g.update(UH=g["H"], UW=g["W"], PKH=ks.dsz("y"), PKW=ks.dsz("x"), PSY=ps.dsz("y"), PSX=ps.dsz("x"))
            g["H"] = (g["UH"] - g["PKH"]) // g["PSY"] + 1; g["W"] = (g["UW"] - g["PKW"]) // g["PSX"] + 1
        f_in = f.dsz("in_grp") * f.dsz("in_chan8") if f.has("in_grp") else f.dsz("in_chan")   # (filts in the input-patch kernel's in_grp:y:x:out_chan:in_chan8 form, boda_amd/nhwc.py)
        grp = self.get_u32("group") if self.has("group") else 1   # Caffe's `group`, the form of out_chans; absent or 1: the ungrouped op
        if grp > 1:   # filts = out_chan=OC : in_chan=C/g : y : x; group j reads channels j*CG .. and writes out_chans j*OCG ..
            if f.has("in_grp") or g["C"] % grp or g["OC"] % grp or f_in * grp != g["C"]:
                raise RtErr(f"conv: group={grp} needs in.chan={g['C']} and filts.out_chan={g['OC']} to be multiples of it and filts.in_chan={f_in} to be in.chan/group")
            g.update(G=grp, CG=g["C"] // grp, OCG=g["OC"] // grp)
        elif grp < 1:
            raise RtErr(f"conv: group={grp} with in.chan={g['C']}, filts.out_chan={g['OC']}: group must be at least 1")
        elif f_in != g["C"]:
            raise RtErr("conv: filts.in_chan != in.chan (groups are not on this path)")
        if o.dsz("img") != g["B"] or o.dsz("chan") != g["OC"]:
            raise RtErr("conv: out dims inconsistent with in/filts")
        for hw, k, s, p, oo in (("H", "KH", "SY", "PY", "OH"), ("W", "KW", "SX", "PX", "OW")):
            if (g[hw] + 2 * g[p] - g[k]) // g[s] + 1 != g[oo]:
                raise RtErr(f"conv: out {oo}={g[oo]} != ({hw}+2*{p}-{k})/{s}+1")
        return g

    def bck_conv_geom(self) -> dict:
        """Geometry of a BckConv: the forward Convolution's (in, filts, stride, in_pad; out_grad_loss in the place of out), validated like conv_geom, and every
        gradient with its matching input's dims."""
        fwd = Op(dict(self.str_vals), {k: v for k, v in self.nda_vals.items() if k not in ("out", "hip_pool")})
        fwd.nda_vals["out"] = self.get("out_grad_loss")
        g = fwd.conv_geom()
        for src, dst in (("in", "in_grad_loss"), ("filts", "filts_grad_loss"), ("biases", "biases_grad_loss")):
            if self.get_dims(dst) != self.get_dims(src):
                raise RtErr(f"BckConv: {dst} dims {self.get_dims(dst).pretty()} != {src} dims {self.get_dims(src).pretty()}")
        if self.get_dims("biases").dims_prod() != g["OC"]:
            raise RtErr("BckConv: biases must hold out_chan values")
        return g

    def deconv_geom(self) -> dict:
        """Named geometry of a Deconvolution (or, with out_grad_loss in the place of out, a BckDeconv): B C H W the input (the SMALL map), OC KH KW from filts
        in_chan:out_chan:y:x, OH = (H-1)*SY + KH - 2*PY and OW likewise (the inverse of conv_geom's rule: the reference's conv_out_sz_to_in_sz).  group > 1 and a
        fused ReLU are refused by name."""
        t = self.get_type()
        bck = t == "BckDeconv"
        i, f, o = self.get_dims("in"), self.get_dims("filts"), self.get_dims("out_grad_loss" if bck else "out")
        st, pad = self.get_dims("stride"), self.get_dims("in_pad")
        if self.has("group") and self.get_u32("group") != 1:
            raise UnsupErr(f"{t}: group={self.get_u32('group')}: a Deconvolution with group > 1 is out of scope")
        if self.has("conv_has_relu") and self.get_u32("conv_has_relu"):
            raise UnsupErr(f"{t}: conv_has_relu=1: a Deconvolution has no fused ReLU")
        if f.names != ("in_chan", "out_chan", "y", "x"):
            raise RtErr(f"{t}: filts must be in_chan:out_chan:y:x (Caffe's blob), got {f.pretty()}")
        g = dict(B=i.dsz("img"), C=i.dsz("chan"), H=i.dsz("y"), W=i.dsz("x"), OC=f.dsz("out_chan"), KH=f.dsz("y"), KW=f.dsz("x"),
                 SY=st.dsz("y"), SX=st.dsz("x"), PY=pad.dsz("y"), PX=pad.dsz("x"), OH=o.dsz("y"), OW=o.dsz("x"))
        if f.dsz("in_chan") != g["C"]:
            raise RtErr(f"{t}: filts.in_chan={f.dsz('in_chan')} != in.chan={g['C']}")
        if o.dsz("img") != g["B"] or o.dsz("chan") != g["OC"]:
            raise RtErr(f"{t}: out dims inconsistent with in/filts")
        if min(g["SY"], g["SX"]) < 1:
            raise RtErr(f"{t}: zero stride")
        for hw, k, s, p, oo in (("H", "KH", "SY", "PY", "OH"), ("W", "KW", "SX", "PX", "OW")):
            if (g[hw] - 1) * g[s] + g[k] - 2 * g[p] != g[oo]:
                raise RtErr(f"{t}: out {oo}={g[oo]} != ({hw}-1)*{s}+{k}-2*{p} = {(g[hw] - 1) * g[s] + g[k] - 2 * g[p]}")
        if self.get_dims("biases").dims_prod() != g["OC"]:
            raise RtErr(f"{t}: biases must hold out_chan values")
        if bck:
            for src, dst in (("in", "in_grad_loss"), ("filts", "filts_grad_loss"), ("biases", "biases_grad_loss")):
                if self.get_dims(dst) != self.get_dims(src):
                    raise RtErr(f"BckDeconv: {dst} dims {self.get_dims(dst).pretty()} != {src} dims {self.get_dims(src).pretty()}")
        return g

    def crop_geom(self) -> dict:
        """A Crop (in -> out) or a BckCrop (out_grad_loss -> in_grad_loss): the window OH x OW at offset (oy, ox) of the plane H x W, img / chan equal."""
        t = self.get_type()
        big, win = (self.get_dims("in"), self.get_dims("out")) if t == "Crop" else (self.get_dims("in_grad_loss"), self.get_dims("out_grad_loss"))
        off = self.get_dims("offset")
        if big.names != ("img", "chan", "y", "x") or win.names != big.names or big.tn != "float" or win.tn != "float":
            raise RtErr(f"{t}: plane and window must be float img:chan:y:x")
        if win.dsz("img") != big.dsz("img") or win.dsz("chan") != big.dsz("chan"):
            raise RtErr(f"{t}: the window {win.pretty()} differs from the plane's tensor {big.pretty()} in img / chan")
        g = dict(B=big.dsz("img"), C=big.dsz("chan"), H=big.dsz("y"), W=big.dsz("x"), OH=win.dsz("y"), OW=win.dsz("x"), oy=off.dsz("y"), ox=off.dsz("x"))
        if g["oy"] + g["OH"] > g["H"] or g["ox"] + g["OW"] > g["W"]:
            raise RtErr(f"{t}: offset ({g['oy']}, {g['ox']}) + window ({g['OH']}, {g['OW']}) exceeds the plane ({g['H']}, {g['W']})")
        return g

    def get_f32(self, an: str) -> float:
        n = self.get(an)
        if n.dims is not None or n.tn != "float":
            raise RtErr(f"op: {an!r} is not a float scalar")
        return float(n.scalar())

    def pool_geom(self) -> dict:
        """Geometry of a Pooling or a Spreading (the pooling gradient, which carries the pooling's parameters): in (the pooling's input) img:chan:y:x, window, stride,
        padding, and an output plane that follows the pooling rule -- a partial last window makes an output of its own, and an input smaller than the window gives
        1 x 1 (src/conv_util.cc:198-204; what conv_pipe computes for its Pooling ops).  Spreading: out_grad_loss has out's dims, in_grad_loss has in's."""
        t = self.get_type()
        i, o = self.get_dims("in"), self.get_dims("out")
        ks, st, pad = self.get_dims("kern_sz"), self.get_dims("stride"), self.get_dims("in_pad")
        g = dict(B=i.dsz("img"), C=i.dsz("chan"), H=i.dsz("y"), W=i.dsz("x"), KH=ks.dsz("y"), KW=ks.dsz("x"), SY=st.dsz("y"), SX=st.dsz("x"),
                 PY=pad.dsz("y"), PX=pad.dsz("x"), OH=o.dsz("y"), OW=o.dsz("x"), avg_pool=self.get_u32("avg_pool"), emit=self.get_u32("emit_out_in_yx"))
        if i.names != ("img", "chan", "y", "x") or o.names != i.names or i.tn != "float" or o.tn != "float":
            raise RtErr(f"{t}: in / out must be float img:chan:y:x")
        if min(g["KH"], g["KW"], g["SY"], g["SX"]) < 1:
            raise RtErr(f"{t}: zero kern_sz / stride")
        if o.dsz("img") != g["B"] or o.dsz("chan") != g["C"]:
            raise RtErr(f"{t}: out img / chan differ from in")
        small = g["H"] + 2 * g["PY"] < g["KH"] or g["W"] + 2 * g["PX"] < g["KW"]   # EITHER padded dim below the window: 1 x 1 (pad_in_sz.both_dims_ge)
        for hw, k, s, p, oo in (("H", "KH", "SY", "PY", "OH"), ("W", "KW", "SX", "PX", "OW")):
            want = 1 if small else -(-(g[hw] + 2 * g[p] - g[k]) // g[s]) + 1
            if want != g[oo]:
                raise RtErr(f"{t}: out {oo}={g[oo]} != ceil(({hw}+2*{p}-{k})/{s})+1 = {want}")
        if g["avg_pool"] not in (0, 1) or g["emit"] not in (0, 1):
            raise RtErr(f"{t}: avg_pool / emit_out_in_yx must be 0 | 1")
        if t == "Pooling" and g["emit"] and g["avg_pool"]:
            raise UnsupErr("Pooling: emit_out_in_yx needs avg_pool=0 (an average has no argmax; test/rtc/pool.cucl says so)")
        if t == "Spreading":
            if self.get_dims("out_grad_loss") != o or self.get_dims("in_grad_loss") != i:
                raise RtErr("Spreading: out_grad_loss must have out's dims and in_grad_loss in's")
        return g

    def lrn_geom(self) -> dict:
        """An LRN or a BckLRN (which carries the LRN's parameters): every tensor float img:chan:y:x with equal dims; an odd local_size."""
        t = self.get_type()
        i = self.get_dims("in")
        if i.names != ("img", "chan", "y", "x") or i.tn != "float":
            raise RtErr(f"{t}: in must be float img:chan:y:x")
        for an in OP_INFO[t][0] + OP_INFO[t][1]:
            if self.get_dims(an) != i:
                raise RtErr(f"{t}: {an} dims {self.get_dims(an).pretty()} != in dims {i.pretty()}")
        g = dict(B=i.dsz("img"), C=i.dsz("chan"), H=i.dsz("y"), W=i.dsz("x"), local_size=self.get_u32("local_size"), emit=self.get_u32("emit_out_scale_base"),
                 alpha=self.get_f32("alpha"), beta=self.get_f32("beta"), k=self.get_f32("k"))
        if g["local_size"] < 1 or g["local_size"] % 2 == 0:
            raise UnsupErr(f"{t}: local_size={g['local_size']}: only odd windows (a centred window over the channels)")
        if g["emit"] not in (0, 1):
            raise RtErr(f"{t}: emit_out_scale_base must be 0 | 1")
        return g

    def zinp_geom(self) -> dict:
        i = self.get_dims("in")
        if i.tn != "float" or self.get_dims("cond") != i or self.get_dims("out") != i:
            raise RtErr("ZeroIfNonPos: in, cond and out must be float tensors of equal dims")
        return dict(N=i.dims_prod())

    def softmax_geom(self) -> dict:
        """SoftmaxWithLoss: in / in_grad_loss img:chan:1:1, label img:1:1, loss 1:1.  Larger planes are refused on purpose: the reference template reads `label` by image only
        (test/rtc/sm_grad_and_loss.cucl), which is wrong for them.  A head on a larger plane runs as the full loss (loss_geom; bck_graph.LossSpec)."""
        i, l = self.get_dims("in"), self.get_dims("label")
        if i.names != ("img", "chan", "y", "x") or l.names != ("img", "y", "x") or i.tn != "float" or l.tn != "float":
            raise UnsupErr("SoftmaxWithLoss: in must be float img:chan:y:x and label float img:y:x")
        if (i.dsz("y"), i.dsz("x")) != (1, 1) or (l.dsz("y"), l.dsz("x")) != (1, 1):
            raise UnsupErr("SoftmaxWithLoss: only 1 x 1 planes (in img:chan:1:1, label img:1:1): the reference reads label by image")
        if l.dsz("img") != i.dsz("img"):
            raise RtErr("SoftmaxWithLoss: label img != in img")
        if self.get_dims("in_grad_loss") != i:
            raise RtErr("SoftmaxWithLoss: in_grad_loss must have in's dims")
        lo = self.get_dims("loss")
        if lo.names != ("y", "x") or lo.sizes != (1, 1) or lo.tn != "float":
            raise RtErr("SoftmaxWithLoss: loss must be float y=1:x=1")
        if i.dsz("img") < 1 or i.dsz("chan") < 1:
            raise RtErr("SoftmaxWithLoss: empty in")
        return dict(B=i.dsz("img"), C=i.dsz("chan"))

    def multi_names(self, an: str) -> tuple:
        """The flattened names of a multi arg: `ins` -> ins_0 .. ins_{ins_num-1} (likewise `outs`), each of which must be in the op."""
        names = tuple(f"{an}_{i}" for i in range(self.get_u32(an + "_num")))
        for n in names:
            self.get_dims(n)
        return names

    def reduce_geom(self) -> dict:
        """Reduce: out = the sum of 2 to 8 float tensors of out's dims (GoogLeNet's widest fan-out needs 4)."""
        o = self.get_dims("out")
        n = self.get_u32("ins_num")
        if n < 2 or n > 8:
            raise UnsupErr(f"Reduce: ins_num={n}: 2 to 8 inputs")
        for an in self.multi_names("ins"):
            if self.get_dims(an) != o or o.tn != "float":
                raise RtErr(f"Reduce: {an} dims {self.get_dims(an).pretty()} != out dims {o.pretty()} (float tensors of equal dims)")
        return dict(N=o.dims_prod(), n=n)

    def dropout_geom(self) -> dict:
        """Dropout / BckDropout: in place (in and out of equal dims), a ratio strictly inside (0, 1) as the reference asserts (src/rtc_fwd.cc:353-355)."""
        t = self.get_type()
        i = self.get_dims("in")
        if self.get_dims("out") != i or i.tn != "float":
            raise RtErr(f"{t}: in and out must be float tensors of equal dims")
        r = self.get_f32("dropout_ratio")
        if not (0.0 < r < 1.0):
            raise RtErr(f"{t}: dropout_ratio={r} must lie inside (0, 1)")
        return dict(N=i.dims_prod(), ratio=r)

    def chan_affine_geom(self) -> dict:
        """ChanAffine: in and out float img:chan:y:x of equal dims, a and b one float per channel, relu 0 | 1."""
        i = self.get_dims("in")
        if i.names != ("img", "chan", "y", "x") or i.tn != "float" or self.get_dims("out") != i:
            raise RtErr("ChanAffine: in and out must be float img:chan:y:x tensors of equal dims")
        for an in ("a", "b"):
            d = self.get_dims(an)
            if d.names != ("chan",) or d.sizes != (i.dsz("chan"),) or d.tn != "float":
                raise RtErr(f"ChanAffine: {an} dims {d.pretty()}: one float per channel of in {i.pretty()}")
        if self.get_u32("relu") not in (0, 1):
            raise RtErr("ChanAffine: relu must be 0 | 1")
        return dict(B=i.dsz("img"), C=i.dsz("chan"), H=i.dsz("y"), W=i.dsz("x"), relu=self.get_u32("relu"))

    def sgd_geom(self) -> dict:
        """SgdUpdate: 1 to 32 tensors, w_i / g_i / h_i float of identical dims, the float scalars lr_mult_i / decay_mult_i, hyper float v=4."""
        n = self.get_u32("tens_num")
        if n < 1 or n > 32:
            raise RtErr(f"SgdUpdate: tens_num={n}: 1 to 32 tensors")
        hy = self.get_dims("hyper")
        if hy.names != ("v",) or hy.sizes != (4,) or hy.tn != "float":
            raise RtErr(f"SgdUpdate: hyper must be float v=4 (lr, momentum, weight_decay, unused), got {hy.tn} {hy.pretty()}")
        elems = []
        for i in range(n):
            w = self.get_dims(f"w_{i}")
            for b in ("w", "g", "h"):
                d = self.get_dims(f"{b}_{i}")
                if d.tn != "float":
                    raise RtErr(f"SgdUpdate: {b}_{i} has type {d.tn}: the update is fp32 only")
                if d != w:
                    raise RtErr(f"SgdUpdate: {b}_{i} dims {d.pretty()} differ from w_{i}'s {w.pretty()}")
            self.get_f32(f"lr_mult_{i}"); self.get_f32(f"decay_mult_{i}")
            elems.append(w.dims_prod())
        return dict(n=n, elems=elems)

    def solver_geom(self) -> dict:
        """SolverUpdate / GradSumsq / GradNorm, with sgd_geom's checks: 1 to 32 tensors of identical float dims per tensor (w_i g_i h_i, h2_i for adam | g_i), hyper float
        v=8, state float v=4, partials float v=P with part0 + the call's chunks <= P.  GradAccum (g_i a_i) and SolverUpdateAcc (a SolverUpdate's op) also carry accum
        float v=4.  -> n, elems, chunks (GradNorm: parts)."""
        t = self.get_type()

        def vec(an, v, what):
            d = self.get_dims(an)
            if d.names != ("v",) or d.tn != "float" or (d.sizes != (v,) if v else d.sizes[0] < 1):
                raise RtErr(f"{t}: {an} must be float v={v or '<partials>'} ({what}), got {d.tn} {d.pretty()}")
            return d.sizes[0]
        hyper = "lr, momentum, weight_decay, momentum2, delta, corr, clip_gradients, unused"
        if t == "GradNorm":
            parts = vec("partials", 0, "one partial per chunk"); vec("hyper", 8, hyper); vec("state", 4, "coef, norm, sumsq, 0")
            return dict(parts=parts)
        bases = ("g", "a") if t == "GradAccum" else ("g",)
        update = t in ("SolverUpdate", "SolverUpdateAcc")
        if update:
            st = self.str_vals.get("solver_type")
            if st not in ("sgd", "nesterov", "adam"):
                raise RtErr(f"{t}: solver_type must be sgd | nesterov | adam, got {st!r}")
            for fl in ("clip", "decoupled_wd"):
                if self.has(fl) and self.get_u32(fl) not in (0, 1):
                    raise RtErr(f"{t}: {fl} must be 0 | 1")
            if self.has("decoupled_wd") and self.get_u32("decoupled_wd") and st != "adam":
                raise RtErr(f"{t}: decoupled_wd=1 is adam's, not {st}'s")
            bases = ("w", "g", "h") + (("h2",) if st == "adam" else ())
        n = self.get_u32("tens_num")
        if n < 1 or n > 32:
            raise RtErr(f"{t}: tens_num={n}: 1 to 32 tensors")
        if update:
            vec("hyper", 8, hyper); vec("state", 4, "coef, norm, sumsq, 0")
        if t in ("GradAccum", "SolverUpdateAcc"):
            vec("accum", 4, "first, apply, scale, micro")
        elems = []
        for i in range(n):
            w = self.get_dims(f"{bases[0]}_{i}")
            for b in bases:
                d = self.get_dims(f"{b}_{i}")
                if d.tn != "float":
                    raise RtErr(f"{t}: {b}_{i} has type {d.tn}: the solver is fp32 only")
                if d != w:
                    raise RtErr(f"{t}: {b}_{i} dims {d.pretty()} differ from {bases[0]}_{i}'s {w.pretty()}")
            if update:
                self.get_f32(f"lr_mult_{i}"); self.get_f32(f"decay_mult_{i}")
            elems.append(w.dims_prod())
        chunks = sum(-(-e // SOLVER_CHUNK) for e in elems)
        if t == "GradSumsq":
            parts = vec("partials", 0, "one partial per chunk")
            if self.get_u32("part0") + chunks > parts:
                raise RtErr(f"GradSumsq: part0={self.get_u32('part0')} + {chunks} chunks exceed the {parts} partials")
        return dict(n=n, elems=elems, chunks=chunks)

    def eval_geom(self) -> dict:
        """Accuracy: in float img:chan:1:1, label float img:1:1, rank uint32_t img.  EvalAccum: rank uint32_t img, loss float y=1:x=1, ctl and counts uint32_t v=4, loss_sum
        float v=1, top_k >= 1.  BnFold: six float chan=C vectors, eps >= 0."""
        t = self.get_type()
        ins, outs, req = OP_INFO[t]
        for an in ins + outs + req:
            if not self.has(an):
                raise RtErr(f"{t}: the op has no {an!r}")

        def vec(an, tn, dn, n):
            d = self.get_dims(an)
            if d.tn != tn or d.names != (dn,) or (d.sizes[0] != n if n else d.sizes[0] < 1):
                raise RtErr(f"{t}: {an} must be {tn} {dn}={n or '<n>'}, got {d.tn} {d.pretty()}")
            return d.sizes[0]
        if t == "Accuracy":
            i, lab = self.get_dims("in"), self.get_dims("label")
            if i.names != ("img", "chan", "y", "x") or i.tn != "float":
                raise RtErr(f"Accuracy: in must be float img:chan:y:x, got {i.tn} {i.pretty()}")
            if (i.dsz("y"), i.dsz("x")) != (1, 1) or lab.names != ("img", "y", "x") or lab.sizes != (i.dsz("img"), 1, 1):
                raise UnsupErr("Accuracy: only 1 x 1 planes (in img:chan:1:1, label img:1:1): the reference reads label by image")
            if lab.tn != "float":
                raise RtErr(f"Accuracy: label has type {lab.tn}: the loss's own var is float")
            vec("rank", "uint32_t", "img", i.dsz("img"))
            return dict(B=i.dsz("img"), C=i.dsz("chan"))
        if t == "EvalAccum":
            B = vec("rank", "uint32_t", "img", 0)
            lo = self.get_dims("loss")
            if lo.tn != "float" or lo.names != ("y", "x") or lo.sizes != (1, 1):
                raise RtErr(f"EvalAccum: loss must be float y=1:x=1, got {lo.tn} {lo.pretty()}")
            vec("ctl", "uint32_t", "v", 4); vec("counts", "uint32_t", "v", 4); vec("loss_sum", "float", "v", 1)
            if self.get_u32("top_k") < 1:
                raise RtErr("EvalAccum: top_k=0: top_k must be at least 1")
            return dict(B=B, top_k=self.get_u32("top_k"))
        C = vec("run_mean", "float", "chan", 0)
        for an in ins + outs:
            vec(an, "float", "chan", C)
        if not self.get("eps").v[0] >= 0.0:
            raise RtErr("BnFold: eps must not be negative")
        return dict(C=C)

    def loss_geom(self) -> dict:
        """SoftmaxLossFwd / LossNorm / SoftmaxLossBck: label and loss_per_pel float img:y:x, the tensors float img:chan:y:x over the same images and plane, loss float
        y=1:x=1, loss_state float v=4; a finite weight, a normalization of the four, has_ignore and an integer ignore_label; fewer than 2^24 pels."""
        import math
        t = self.get_type()
        ins, outs, req = OP_INFO[t]
        for an in ins + outs + req:
            if not self.has(an):
                raise RtErr(f"{t}: the op has no {an!r}")
        lab = self.get_dims("label")
        if lab.tn != "float" or lab.names != ("img", "y", "x"):
            raise RtErr(f"{t}: label must be float img:y:x, got {lab.tn} {lab.pretty()}")
        B, HW = lab.dsz("img"), lab.dsz("y") * lab.dsz("x")
        if B < 1 or HW < 1:
            raise RtErr(f"{t}: empty label")
        if B * HW >= 2 ** 24:
            raise RtErr(f"{t}: img * y * x = {B * HW} pels: 2^24 or more, and the pel count must be exact as a float")
        C = 0
        for an in ins + outs:
            d = self.get_dims(an)
            if an in ("in", "prob", "in_grad_loss"):
                if d.tn != "float" or d.names != ("img", "chan", "y", "x"):
                    raise RtErr(f"{t}: {an} must be float img:chan:y:x, got {d.tn} {d.pretty()}")
                if (d.dsz("img"), d.dsz("y"), d.dsz("x")) != lab.sizes or d.dsz("chan") < 1 or (C and d.dsz("chan") != C):
                    raise RtErr(f"{t}: {an} {d.pretty()} does not fit label {lab.pretty()}" + (f" and chan={C}" if C else ""))
                C = d.dsz("chan")
                if 4 * d.dims_prod() >= 2 ** 31:
                    raise UnsupErr(f"{t}: tensors of 2 GiB or more")
            elif an == "loss_per_pel" and d != lab:
                raise RtErr(f"{t}: loss_per_pel must have label's dims, got {d.tn} {d.pretty()}")
            elif an == "loss" and (d.tn != "float" or d.names != ("y", "x") or d.sizes != (1, 1)):
                raise RtErr(f"{t}: loss must be float y=1:x=1, got {d.tn} {d.pretty()}")
            elif an == "loss_state" and (d.tn != "float" or d.names != ("v",) or d.sizes != (4,)):
                raise RtErr(f"{t}: loss_state must be float v=4 (Z, s, count, sum), got {d.tn} {d.pretty()}")
        w, ig = self.get("weight").v[0], self.get("ignore_label").v[0]
        if not math.isfinite(w):
            raise RtErr(f"{t}: weight must be finite, got {w!r}")
        norm = self.str_vals.get("normalization")
        if norm not in LOSS_NORMALIZATIONS:
            raise RtErr(f"{t}: normalization must be {' | '.join(LOSS_NORMALIZATIONS)}, got {norm!r}")
        if self.get_u32("has_ignore") and not (math.isfinite(ig) and ig == int(ig)):
            raise RtErr(f"{t}: ignore_label must be an integer, got {ig!r}")
        return dict(B=B, C=C, HW=HW, form="pel" if HW >= 64 else "wave", weight=w, normalization=norm, ignore_label=int(ig) if self.get_u32("has_ignore") else None)

    def data_geom(self) -> dict:
        """DataTransform: src uint8_t img:y:x:chan ("hwc") or img:chan:y:x ("chw") at the source size H x W; out float img:chan:y:x with src's img and chan and the crop
        size ch <= H, cw <= W; mean float chan=C or chan=C:y=H:x=W; plan uint32_t img=B:v=4; the float scale."""
        fn = "DataTransform"
        for an in ("src", "plan", "mean", "out"):
            if not self.has(an):
                raise RtErr(f"{fn}: the op has no {an!r}")
        src, plan, mean, out = (self.get_dims(an) for an in ("src", "plan", "mean", "out"))
        layout = {("img", "y", "x", "chan"): "hwc", ("img", "chan", "y", "x"): "chw"}.get(src.names)
        if src.tn != "uint8_t" or layout is None:
            raise RtErr(f"{fn}: src must be uint8_t img:y:x:chan or img:chan:y:x, got {src.tn} {src.pretty()}")
        if out.tn != "float" or out.names != ("img", "chan", "y", "x"):
            raise RtErr(f"{fn}: out must be float img:chan:y:x, got {out.tn} {out.pretty()}")
        B, C, H, W = (src.dsz(n) for n in ("img", "chan", "y", "x"))
        ch, cw = out.dsz("y"), out.dsz("x")
        if out.dsz("img") != B:
            raise RtErr(f"{fn}: out has {out.dsz('img')} images, src {B}")
        if out.dsz("chan") != C:
            raise RtErr(f"{fn}: out has chan={out.dsz('chan')}, src chan={C}: the transform keeps the channels")
        if min(B, C, ch, cw) < 1:
            raise RtErr(f"{fn}: empty out")
        if ch > H or cw > W:
            raise RtErr(f"{fn}: the crop {ch} x {cw} is larger than the source {H} x {W}")
        forms = {(("chan",), (C,)): "chan", (("chan", "y", "x"), (C, H, W)): "chan:y:x"}
        if mean.tn != "float" or (mean.names, mean.sizes) not in forms:
            raise RtErr(f"{fn}: mean must be float chan={C} or chan={C}:y={H}:x={W} (the SOURCE size), got {mean.tn} {mean.pretty()}")
        if plan.tn != "uint32_t" or plan.names != ("img", "v") or plan.sizes != (B, 4):
            raise RtErr(f"{fn}: plan must be uint32_t img={B}:v=4 (y_off, x_off, mirror, unused), got {plan.tn} {plan.pretty()}")
        if B * C * H * W >= 2 ** 31 or 4 * B * C * ch * cw >= 2 ** 31 or 4 * C * H * W >= 2 ** 31:
            raise UnsupErr(f"{fn}: tensors of 2 GiB or more")
        if not self.has("scale"):
            raise RtErr(f"{fn}: the op has no 'scale'")
        return dict(B=B, C=C, H=H, W=W, ch=ch, cw=cw, layout=layout, mean_form=forms[(mean.names, mean.sizes)], scale=self.get("scale").v[0])

    def bn_geom(self) -> dict:
        """BnStats / BnFwd / BnBckSums / BnBckIn and BnfPrep / BnfBck / BnfBckIn (`in` gives the dims even where no var is bound to it): float img:chan:y:x tensors of equal dims, the per-channel args float chan=C; FanOut: in and 2 to 8 outs of equal float dims."""
        t = self.get_type()
        i = self.get_dims("in")
        if i.tn != "float":
            raise RtErr(f"{t}: in has type {i.tn}: fp32 only")
        ins, outs, _ = OP_INFO[t]
        if t == "FanOut":
            n = self.get_u32("outs_num")
            if n < 2 or n > 8:
                raise UnsupErr(f"FanOut: outs_num={n}: 2 to 8 outputs")
            for an in self.multi_names("outs"):
                if self.get_dims(an) != i:
                    raise RtErr(f"FanOut: {an} dims {self.get_dims(an).pretty()} differ from in's {i.pretty()}")
            return dict(N=i.dims_prod(), n=n)
        if i.names != ("img", "chan", "y", "x"):
            raise RtErr(f"{t}: in must be img:chan:y:x, got {i.pretty()}")
        for an in ins + outs:
            d = self.get_dims(an)
            if an in ("in", "out", "out_grad_loss", "in_grad_loss"):
                if d != i:
                    raise RtErr(f"{t}: {an} dims {d.pretty()} differ from in's {i.pretty()}")
            elif d.names != ("chan",) or d.sizes != (i.dsz("chan"),) or d.tn != "float":
                raise RtErr(f"{t}: {an} dims {d.pretty()}: one float per channel of in {i.pretty()}")
        if t == "BnStats":
            self.get_f32("eps"); self.get_f32("maf")
        if t == "BnfPrep" and not self.get_f32("eps") >= 0.0:
            raise RtErr("BnfPrep: eps must not be negative")
        if t in ("BnStats", "BnBckSums", "BnfBck") and self.get_u32("slab") % 4:
            raise RtErr(f"{t}: slab={self.get_u32('slab')}: a forced slab length is a multiple of 4")
        if t == "BnFwd" and self.get_u32("relu") not in (0, 1):
            raise RtErr("BnFwd: relu must be 0 | 1")
        return dict(B=i.dsz("img"), C=i.dsz("chan"), H=i.dsz("y"), W=i.dsz("x"))

    def concat_geom(self) -> dict:
        """Concat (ins_i -> out) / Split (in -> outs_i): float img:chan:y:x tensors of equal img / y / x whose channels add up to the wide tensor's.  -> B, H, W, CT and
        chans: per narrow tensor (arg name, first channel in the wide tensor, channels)."""
        t = self.get_type()
        wide, names = (self.get_dims("out"), self.multi_names("ins")) if t == "Concat" else (self.get_dims("in"), self.multi_names("outs"))
        if wide.names != ("img", "chan", "y", "x") or wide.tn != "float" or not names:
            raise RtErr(f"{t}: tensors must be float img:chan:y:x, and at least one narrow tensor")
        chans, c0 = [], 0
        for an in names:
            d = self.get_dims(an)
            if d.names != wide.names or d.tn != "float" or (d.dsz("img"), d.dsz("y"), d.dsz("x")) != (wide.dsz("img"), wide.dsz("y"), wide.dsz("x")):
                raise RtErr(f"{t}: {an} dims {d.pretty()} differ from the wide tensor's {wide.pretty()} in img / y / x")
            chans.append((an, c0, d.dsz("chan"))); c0 += d.dsz("chan")
        if c0 != wide.dsz("chan"):
            raise RtErr(f"{t}: the narrow tensors hold {c0} channels, the wide one {wide.dsz('chan')}")
        return dict(B=wide.dsz("img"), CT=wide.dsz("chan"), H=wide.dsz("y"), W=wide.dsz("x"), chans=chans)

    def sgemm_geom(self) -> dict:
        a, b, c = self.get_dims("a"), self.get_dims("b"), self.get_dims("c")
        g = dict(M=a.dsz("M"), K=a.dsz("K"), N=b.dsz("N"))
        if b.dsz("K") != g["K"] or c.dsz("M") != g["M"] or c.dsz("N") != g["N"]:
            raise RtErr("sgemm: inconsistent a/b/c dims")
        return g

    def flops(self) -> int:
        """2*M*N*K with the reference's accounting (src/latex-util.H:116-120,126-133)."""
        if self.get_type() == "sgemm":
            g = self.sgemm_geom()
            return 2 * g["M"] * g["N"] * g["K"]
        if self.get_type() in _NON_GEMM_TYPES:   # bandwidth ops: no multiply-accumulate work is accounted
            return 0
        if self.get_type() in ("Deconvolution", "BckDeconv"):   # every in element meets every tap of every out_chan: 2*B*C*H*W*OC*KH*KW; the gradients twice that
            g = self.deconv_geom()
            return (4 if self.get_type() == "BckDeconv" else 2) * g["B"] * g["C"] * g["H"] * g["W"] * g["OC"] * g["KH"] * g["KW"]
        if self.get_type() == "BckConv":   # two GEMMs of the forward size: the data and the filter gradient
            g = self.bck_conv_geom()
            return 4 * (g["B"] * g["OH"] * g["OW"]) * g["OC"] * (g.get("CG", g["C"]) * g["KH"] * g["KW"])
        g = self.conv_geom()   # (group > 1: every out_chan reduces over its group's CG = C/g channels only)
        return 2 * (g["B"] * g["OH"] * g["OW"]) * g["OC"] * (g.get("CG", g["C"]) * g["KH"] * g["KW"])

    def algo_bytes(self) -> int:
        """4*(in+out+filts+biases) resp. 4*(a+b+c) (src/latex-util.H:119,133)."""
        if self.get_type() == "SgdUpdate":   # w, g, h read, h and w written
            return 20 * sum(self.sgd_geom()["elems"])
        if self.get_type() == "GradAccum":   # g and a read, a written
            return 12 * sum(self.solver_geom()["elems"])
        if self.get_type() in ("SolverUpdate", "SolverUpdateAcc"):   # adam reads and writes h2 as well
            return (28 if self.str_vals.get("solver_type") == "adam" else 20) * sum(self.solver_geom()["elems"])
        if self.get_type() == "GradSumsq":   # every gradient read once, one partial written per chunk
            g = self.solver_geom()
            return 4 * sum(g["elems"]) + 4 * g["chunks"]
        if self.get_type() == "GradNorm":   # the partials read, four words written
            return 4 * self.solver_geom()["parts"] + 16
        ins, outs, _ = OP_INFO[self.get_type()]
        multi = {"Reduce": ("ins",), "Concat": ("ins",), "Split": ("outs",), "FanOut": ("outs",)}.get(self.get_type(), ())
        return sum(self.get_dims(a).bytes_sz() for a in ins + outs + tuple(n for m in multi for n in self.multi_names(m)))


def parse_op(line: str) -> Op:
    """Parse one op line in either the current or the legacy form."""
    d = _kv(parse_lexp(line.strip()))
    op = Op()
    if "dims_vals" in d or "type" in d:  # legacy form
        unknown = set(d) - {"type", "dims_vals", "str_vals"}
        if unknown:
            raise RtErr(f"op(legacy): unknown fields {sorted(unknown)}")
        op.str_vals["type"] = str(d["type"])
        none_dims = {"kern_sz", "stride", "in_pad", "offset"}
        for k, v in _kv(d.get("dims_vals", [])).items():
            tn = "none" if k in none_dims else "float"
            dims, tn = _parse_dims(v, tn)
            op.nda_vals[k] = Nda(dims=dims, tn=tn)
        for k, v in _kv(d.get("str_vals", [])).items():
            if k == "out_chans":  # became a uint32 nda in the current form
                op.nda_vals[k] = Nda(dims=None, tn="uint32_t", v=(int(v),))
            else:
                op.str_vals[k] = str(v)
    else:
        unknown = set(d) - {"str_vals", "nda_vals"}
        if unknown:
            raise RtErr(f"op: unknown fields {sorted(unknown)}")
        for k, v in _kv(d.get("str_vals", [])).items():
            op.str_vals[k] = str(v)
        for k, v in _kv(d.get("nda_vals", [])).items():
            op.nda_vals[k] = parse_nda(v)
    t = op.str_vals.get("type")
    if t in OP_INFO and "func_name" not in op.str_vals:  # annotated ops carry variant-specific layouts: not validated
        ins, outs, req = OP_INFO[t]
        for an in ins + outs + req:
            if an not in op.nda_vals:
                raise RtErr(f"op: {t} is missing required field {an!r}")
        if t == "Convolution":
            op.conv_geom()
        elif t == "BckConv":
            op.bck_conv_geom()
        elif t in ("Deconvolution", "BckDeconv"):
            op.deconv_geom()
        elif t in ("Crop", "BckCrop"):
            op.crop_geom()
        elif t in ("Pooling", "Spreading"):
            op.pool_geom()
        elif t in ("LRN", "BckLRN"):
            op.lrn_geom()
        elif t == "ZeroIfNonPos":
            op.zinp_geom()
        elif t == "SoftmaxWithLoss":
            op.softmax_geom()
        elif t == "Reduce":
            op.reduce_geom()
        elif t in ("Concat", "Split"):
            op.concat_geom()
        elif t in ("Dropout", "BckDropout"):
            op.dropout_geom()
        elif t == "ChanAffine":
            op.chan_affine_geom()
        elif t == "SgdUpdate":
            op.sgd_geom()
        elif t in BN_TYPES or t in BNF_TYPES:
            op.bn_geom()
        elif t in SOLVER_TYPES:
            op.solver_geom()
        elif t in EVAL_TYPES:
            op.eval_geom()
        elif t in DATA_TYPES:
            op.data_geom()
        elif t in LOSS_TYPES:
            op.loss_geom()
        else:
            op.sgemm_geom()
    return op


def read_ops(path: str) -> List[Op]:
    with open(path) as f:
        return [parse_op(l) for l in f if l.strip()]


def data_path(*parts: str) -> str:
    """Path of a shape-data file the package ships (boda_amd/data/): the op lists / net records of the BASELINE workloads.  Test fixtures
    (reference-held digests, the reference's other op lists) live under tests/golden/ and are never read by product code."""
    import os
    return os.path.join(os.path.dirname(os.path.abspath(__file__)), "data", *parts)
