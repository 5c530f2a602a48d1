"""Caffe prototxt (text format) -> layer list -> per-layer Convolution ops with inferred shapes.

Restates what the reference's net reader needs for this path (src/caffepb.cc:166-326, src/conv_util.cc:405-529):
TEST-phase layers only; Convolution out = (in + 2*pad - k)/stride + 1 (floor); Pooling uses ceil and `global_pooling`;
Concat sums channels; ReLU / LRN / Dropout / BatchNorm / Scale / Eltwise keep the shape; InnerProduct is a convolution
whose kernel is the whole input; Accuracy / Softmax* / loss layers are ignored (accuracy_layers lists the Accuracy ones).  Every Convolution gets a bias input
(the reference always attaches `<name>_biases`, src/caffepb.cc:227-228, even when the prototxt says bias_term: false).
Only the subset of the text format that net definitions use is parsed: `key: value` and `key { ... }`.
"""
from __future__ import annotations
import re
from typing import Dict, List, Tuple, Union

from .op import Op, RtErr, UnsupErr, parse_op
from .solver_cfg import Freeze, LrPolicy, Solver

Node = Dict[str, list]


def parse(text: str) -> Node:
    toks = re.findall(r'"[^"]*"|[{}]|[^\s{}:]+:?', re.sub(r"#.*", "", text))
    pos = 0

    def block() -> Node:
        nonlocal pos
        d: Node = {}
        while pos < len(toks) and toks[pos] != "}":
            key = toks[pos]; pos += 1
            if key.endswith(":"):
                key = key[:-1]
                val = toks[pos]; pos += 1
                d.setdefault(key, []).append(val.strip('"'))
            else:
                if toks[pos] != "{":
                    raise RtErr(f"prototxt: expected '{{' after {key!r}")
                pos += 1
                d.setdefault(key, []).append(block())
                if pos >= len(toks) or toks[pos] != "}":
                    raise RtErr("prototxt: unbalanced braces")
                pos += 1
        return d
    root = block()
    if pos != len(toks):
        raise RtErr("prototxt: trailing tokens")
    return root


def _one(d: Node, k: str, default=None):
    v = d.get(k)
    return v[0] if v else default


def _is_test_phase(layer: Node) -> bool:
    for inc in layer.get("include", []):
        if _one(inc, "phase") == "TRAIN":
            return False
    return True


def conv_ops(text: str, batch: int, in_chw: Tuple[int, int, int] = (3, 224, 224)) -> List[Tuple[str, Op]]:
    """-> [(layer name, Convolution op at `batch`)] in definition order, shapes inferred through the whole net."""
    root = parse(text)
    layers = root.get("layer", []) or root.get("layers", [])
    shapes: Dict[str, Tuple[int, int, int]] = {}
    if "input" in root:
        dims = [int(x) for x in root.get("input_dim", [])]
        shapes[_one(root, "input")] = (dims[1], dims[2], dims[3]) if len(dims) == 4 else in_chw
    out: List[Tuple[str, Op]] = []
    for L in layers:
        if not _is_test_phase(L):
            continue
        t = str(_one(L, "type")).upper().replace("_", "")
        bots, tops, name = L.get("bottom", []), L.get("top", []), _one(L, "name")
        if t == "DATA":
            cs = int(_one(_one(L, "transform_param", {}), "crop_size", in_chw[1]))
            shapes[tops[0]] = (in_chw[0], cs, cs)
            continue
        if t in ("ACCURACY", "SOFTMAX", "SOFTMAXWITHLOSS", "SOFTMAXLOSS"):
            continue
        if not bots or bots[0] not in shapes:
            raise RtErr(f"prototxt: layer {name!r} reads unknown blob {bots[:1]}")
        C, H, W = shapes[bots[0]]
        if t in ("CONVOLUTION", "INNERPRODUCT"):
            if t == "CONVOLUTION":
                cp = _one(L, "convolution_param", {})
                oc = int(_one(cp, "num_output")); k = int(_one(cp, "kernel_size", 1)); s = int(_one(cp, "stride", 1)); p = int(_one(cp, "pad", 0))
                grp = int(_one(cp, "group", 1))
                if grp < 1 or C % grp or oc % grp:
                    raise RtErr(f"prototxt: convolution {name!r}: group={grp} must divide its {C} input channels and its num_output={oc}")
                kh = kw = k
            else:
                oc = int(_one(_one(L, "inner_product_param", {}), "num_output")); kh, kw, s, p, grp = H, W, 1, 0, 1
            oh = (H + 2 * p - kh) // s + 1; ow = (W + 2 * p - kw) // s + 1
            out.append((name, parse_op(
                f"(str_vals=(type=Convolution),nda_vals=(biases=(dims=(out_chan={oc})),filts=(dims=(out_chan={oc},in_chan={C // grp},y={kh},x={kw})),"
                + (f"group=(tn=uint32_t,v={grp})," if grp > 1 else "") +
                f"in=(dims=(img={batch},chan={C},y={H},x={W})),in_pad=(tn=none,dims=(y={p},x={p})),kern_sz=(tn=none,dims=(y={kh},x={kw})),"
                f"out=(dims=(img={batch},chan={oc},y={oh},x={ow})),out_chans=(tn=uint32_t,v={oc}),stride=(tn=none,dims=(y={s},x={s}))))")))
            shapes[tops[0]] = (oc, oh, ow)
        elif t == "DECONVOLUTION":   # out = (in - 1) * stride + k - 2 * pad; filts are Caffe's blob in_chan : out_chan : y : x
            oc, k, s, p = _deconv_param(L, name)
            oh = (H - 1) * s + k - 2 * p; ow = (W - 1) * s + k - 2 * p
            out.append((name, parse_op(
                f"(str_vals=(type=Deconvolution),nda_vals=(biases=(dims=(out_chan={oc})),filts=(dims=(in_chan={C},out_chan={oc},y={k},x={k})),"
                f"in=(dims=(img={batch},chan={C},y={H},x={W})),in_pad=(tn=none,dims=(y={p},x={p})),kern_sz=(tn=none,dims=(y={k},x={k})),"
                f"out=(dims=(img={batch},chan={oc},y={oh},x={ow})),out_chans=(tn=uint32_t,v={oc}),stride=(tn=none,dims=(y={s},x={s}))))")))
            shapes[tops[0]] = (oc, oh, ow)
        elif t == "CROP":
            oy, ox = _crop_param(L, name)
            if len(bots) != 2 or bots[1] not in shapes:
                raise RtErr(f"prototxt: crop {name!r} needs two known bottoms (a, ref)")
            rh, rw = shapes[bots[1]][1:]
            if oy + rh > H or ox + rw > W:
                raise RtErr(f"prototxt: crop {name!r}: offset ({oy}, {ox}) + {bots[1]!r}'s plane ({rh}, {rw}) exceeds {bots[0]!r}'s plane ({H}, {W})")
            shapes[tops[0]] = (C, rh, rw)
        elif t == "POOLING":
            pp = _one(L, "pooling_param", {})
            if str(_one(pp, "global_pooling", "false")).lower() == "true":
                shapes[tops[0]] = (C, 1, 1)
            else:
                k = int(_one(pp, "kernel_size")); s = int(_one(pp, "stride", 1)); p = int(_one(pp, "pad", 0))
                osz = lambda i: 1 if i + 2 * p < k else -(-(i + 2 * p - k) // s) + 1
                shapes[tops[0]] = (C, osz(H), osz(W))
        elif t == "CONCAT":
            cs = [shapes[b] for b in bots]
            if any(c[1:] != cs[0][1:] for c in cs):
                raise RtErr(f"prototxt: concat {name!r} of mismatched spatial sizes")
            shapes[tops[0]] = (sum(c[0] for c in cs), H, W)
        elif t in ("RELU", "LRN", "DROPOUT", "BATCHNORM", "SCALE", "ELTWISE", "SPLIT"):
            for tp in tops:
                shapes[tp] = (C, H, W)
        else:
            raise RtErr(f"prototxt: unhandled layer type {t!r} ({name!r})")
    return out


def _deconv_param(L: Node, name) -> Tuple[int, int, int, int]:
    """-> (num_output, kernel_size, stride, pad) of a Deconvolution layer; group > 1 is refused by name."""
    cp = _one(L, "convolution_param", {})
    grp = int(_one(cp, "group", 1))
    if grp != 1:
        raise UnsupErr(f"prototxt: deconvolution {name!r}: group={grp}: a Deconvolution with group > 1 is out of scope")
    return int(_one(cp, "num_output")), int(_one(cp, "kernel_size", 1)), int(_one(cp, "stride", 1)), int(_one(cp, "pad", 0))


def _crop_param(L: Node, name) -> Tuple[int, int]:
    """-> (oy, ox) of a Crop layer: crop_param { axis offset }, one offset for both axes or one per axis; axis other than 2 is refused by name."""
    cp = _one(L, "crop_param", {})
    axis = int(_one(cp, "axis", 2))
    if axis != 2:
        raise UnsupErr(f"prototxt: crop {name!r}: axis={axis}: only axis 2 (the plane: y and x) is supported")
    offs = [int(x) for x in cp.get("offset", [])] if isinstance(cp, dict) else []
    if len(offs) > 2:
        raise RtErr(f"prototxt: crop {name!r}: {len(offs)} offsets for the two axes y, x")
    return (0, 0) if not offs else (offs[0], offs[0]) if len(offs) == 1 else (offs[0], offs[1])


def conv_bottoms(text: str) -> List[Tuple[str, str]]:
    """-> [(layer name, bottom blob)] of the TEST-phase Convolution / InnerProduct layers in definition order (the order of conv_ops): which convolutions read the
    same blob -- sibling convolutions that can run as one fused launch -- is a fact of the net graph, not of the layer shapes."""
    root = parse(text)
    out: List[Tuple[str, str]] = []
    for L in root.get("layer", []) or root.get("layers", []):
        if _is_test_phase(L) and str(_one(L, "type")).upper().replace("_", "") in ("CONVOLUTION", "INNERPRODUCT"):
            out.append((str(_one(L, "name")), str(L.get("bottom", [""])[0])))
    return out


def pipe_spec(text: str, in_chw: Tuple[int, int, int] = (3, 224, 224)) -> List[str]:
    """-> the TEST-phase forward ops of a net definition as compact one-line records (boda_amd.conv_pipe.pipe_from_spec reads
    them back): what the reference's reader keeps of each layer for conv_pipe_t (src/caffepb.cc:166-326).
      input C H W | conv tag bot top oc kh kw sy sx py px [group] | pool tag bot top kh kw sy sx py px avg global
      lrn tag bot top local_size alpha beta k | relu tag bot top | drop tag bot top | concat tag top bot1,bot2,...
      deconv tag bot top oc kh kw sy sx py px | crop tag bot ref top oy ox"""
    root = parse(text)
    layers = root.get("layer", []) or root.get("layers", [])
    out: List[str] = []
    have_input = False
    for L in layers:
        if not _is_test_phase(L):
            continue
        t = str(_one(L, "type")).upper().replace("_", "")
        bots, tops, name = L.get("bottom", []), L.get("top", []), _one(L, "name")
        if t == "DATA":
            cs = int(_one(_one(L, "transform_param", {}), "crop_size", in_chw[1]))
            out.append(f"input {tops[0]} {in_chw[0]} {cs} {cs}"); have_input = True
        elif t in ("ACCURACY", "SOFTMAX", "SOFTMAXWITHLOSS", "SOFTMAXLOSS"):
            continue
        elif t == "CONVOLUTION":
            cp = _one(L, "convolution_param", {})
            grp = int(_one(cp, "group", 1))
            if grp < 1:
                raise RtErr(f"prototxt: convolution {name!r}: group={grp}: at least 1")
            k, s_, p_ = int(_one(cp, "kernel_size", 1)), int(_one(cp, "stride", 1)), int(_one(cp, "pad", 0))
            out.append(f"conv {name} {bots[0]} {tops[0]} {int(_one(cp, 'num_output'))} {k} {k} {s_} {s_} {p_} {p_}" + (f" {grp}" if grp > 1 else ""))
        elif t == "INNERPRODUCT":
            out.append(f"conv {name} {bots[0]} {tops[0]} {int(_one(_one(L, 'inner_product_param', {}), 'num_output'))} 0 0 1 1 0 0")  # kernel = whole input
        elif t == "DECONVOLUTION":
            oc, k, s_, p_ = _deconv_param(L, name)
            out.append(f"deconv {name} {bots[0]} {tops[0]} {oc} {k} {k} {s_} {s_} {p_} {p_}")
        elif t == "CROP":
            oy, ox = _crop_param(L, name)
            if len(bots) != 2:
                raise RtErr(f"prototxt: crop {name!r} needs two bottoms (a, ref)")
            out.append(f"crop {name} {bots[0]} {bots[1]} {tops[0]} {oy} {ox}")
        elif t == "POOLING":
            pp = _one(L, "pooling_param", {})
            glob = int(str(_one(pp, "global_pooling", "false")).lower() == "true")
            k = 0 if glob else int(_one(pp, "kernel_size")); s_ = int(_one(pp, "stride", 1)); p_ = int(_one(pp, "pad", 0))
            avg = int(str(_one(pp, "pool", "MAX")).upper() == "AVE")
            out.append(f"pool {name} {bots[0]} {tops[0]} {k} {k} {s_} {s_} {p_} {p_} {avg} {glob}")
        elif t == "LRN":
            lp = _one(L, "lrn_param", {})
            out.append(f"lrn {name} {bots[0]} {tops[0]} {int(_one(lp, 'local_size', 5))} {float(_one(lp, 'alpha', 1.0))} {float(_one(lp, 'beta', 0.75))} {float(_one(lp, 'k', 1.0))}")
        elif t == "RELU":
            out.append(f"relu {name} {bots[0]} {tops[0]}")
        elif t == "DROPOUT":
            out.append(f"drop {name} {bots[0]} {tops[0]}")
        elif t == "CONCAT":
            out.append(f"concat {name} {tops[0]} {','.join(bots)}")
        else:
            raise RtErr(f"prototxt: layer type {t!r} ({name!r}) has no forward op on this path")
    if not have_input and "input" in root:
        dims = [int(x) for x in root.get("input_dim", [])]
        c, h, w = (dims[1], dims[2], dims[3]) if len(dims) == 4 else in_chw
        out.insert(0, f"input {_one(root, 'input')} {c} {h} {w}")
    return out


# ---- Caffe's SolverParameter (solver.prototxt) -> solver_cfg.Solver
_SOLVER_TYPES = {"SGD": "sgd", "Nesterov": "nesterov", "Adam": "adam"}                 # type: "<name>"
_SOLVER_ENUMS = {"SGD": "sgd", "NESTEROV": "nesterov", "ADAM": "adam"}                 # the legacy solver_type: <ENUM>
_SOLVER_UNSUP = ("AdaGrad", "RMSProp", "AdaDelta", "ADAGRAD", "RMSPROP", "ADADELTA")   # Caffe's other three: no kernel here
_SOLVER_KEYS = ("type", "solver_type", "base_lr", "lr_policy", "gamma", "power", "stepsize", "stepvalue", "max_iter", "momentum", "momentum2", "delta", "weight_decay",
                "clip_gradients", "iter_size", "regularization_type")


def solver_spec(text: str):
    """Caffe's SolverParameter text form -> (bck_pipe.Solver, iter_size, ignored): what ConvPipeBck(rtc, solver=..., iter_size=...) takes.
    Read: type "SGD" | "Nesterov" | "Adam" (or the legacy solver_type SGD | NESTEROV | ADAM) -> type; base_lr -> lr; lr_policy with gamma / power / stepsize / the repeated
    stepvalue / max_iter -> an LrPolicy holding the keys the file gives (no lr_policy key: None, a fixed rate); momentum, momentum2, delta, weight_decay, clip_gradients;
    iter_size.  Absent keys get CAFFE's defaults, not the dataclass's: momentum 0, weight_decay 0, momentum2 0.999, delta 1e-8, clip_gradients -1 (off: 0.0 here),
    iter_size 1, type SGD.  AdaGrad / RMSProp / AdaDelta and regularization_type "L1" are an UnsupErr that names the value.  Every other key (net, test_iter, display,
    snapshot*, solver_mode, random_seed, ...) comes back in `ignored`, key -> the list of its values."""
    from .op import UnsupErr
    d = parse(text)
    for k in _SOLVER_KEYS:
        if k != "stepvalue" and len(d.get(k, [])) > 1:
            raise RtErr(f"solver prototxt: {k!r} is given {len(d[k])} times")
        if any(isinstance(v, dict) for v in d.get(k, [])):
            raise RtErr(f"solver prototxt: {k!r} must be a value, not a block")

    def num(k, default, conv=float):
        v = _one(d, k)
        if v is None:
            return default
        try:
            return conv(v)
        except ValueError:
            raise RtErr(f"solver prototxt: {k}: {v!r} is not a number")
    if "type" in d and "solver_type" in d:
        raise RtErr("solver prototxt: both 'type' and the legacy 'solver_type' are given")
    name, table = (_one(d, "type"), _SOLVER_TYPES) if "type" in d else (_one(d, "solver_type", "SGD"), _SOLVER_ENUMS)
    if name in _SOLVER_UNSUP:
        raise UnsupErr(f"solver prototxt: solver type {name!r}: only SGD, Nesterov and Adam have an update kernel (AdaGrad, RMSProp and AdaDelta are not built)")
    if name not in table:
        raise RtErr(f"solver prototxt: solver type {name!r}: one of {' | '.join(table)}")
    reg = _one(d, "regularization_type", "L2")
    if reg != "L2":
        if reg == "L1":
            raise UnsupErr("solver prototxt: regularization_type 'L1': the update kernels regularise with weight_decay * w (L2) only")
        raise RtErr(f"solver prototxt: regularization_type {reg!r}: L2 | L1")
    if "base_lr" not in d:
        raise RtErr("solver prototxt: no base_lr")
    policy = None
    if "lr_policy" in d:
        kw = {k: num(k, None) for k in ("gamma", "power") if k in d}
        kw.update({k: num(k, None, int) for k in ("stepsize", "max_iter") if k in d})
        if "stepvalue" in d:
            try:
                kw["stepvalues"] = tuple(int(v) for v in d["stepvalue"])
            except (ValueError, TypeError):
                raise RtErr(f"solver prototxt: stepvalue: {d['stepvalue']!r} are not all integers")
        policy = LrPolicy(_one(d, "lr_policy"), **kw)
    clip = num("clip_gradients", -1.0)
    iter_size = num("iter_size", 1, int)
    if iter_size < 1:
        raise RtErr(f"solver prototxt: iter_size={iter_size}: at least 1")
    sv = Solver(type=table[name], lr=num("base_lr", None), momentum=num("momentum", 0.0), momentum2=num("momentum2", 0.999), delta=num("delta", 1e-8),
                weight_decay=num("weight_decay", 0.0), clip_gradients=clip if clip > 0 else 0.0, lr_policy=policy)
    return sv, iter_size, {k: v for k, v in d.items() if k not in _SOLVER_KEYS}


def test_spec(text: str) -> dict:
    """The test keys of a Caffe solver.prototxt -> {"test_iter", "test_interval", "test_initialization"}: how many batches an evaluation runs (EvalPipe.evaluate's
    n_batches), every how many updates, and whether one runs before the first update.  Absent keys get Caffe's defaults: no test_iter -> 0 (test_iter is repeated, one
    per test net: the first is taken), test_interval 0, test_initialization true.  solver_spec keeps handing these keys back in `ignored`; the caller's loop drives the
    interval."""
    d = parse(text)
    for k in ("test_iter", "test_interval", "test_initialization"):
        if any(isinstance(v, dict) for v in d.get(k, [])):
            raise RtErr(f"solver prototxt: {k!r} must be a value, not a block")
    for k in ("test_interval", "test_initialization"):
        if len(d.get(k, [])) > 1:
            raise RtErr(f"solver prototxt: {k!r} is given {len(d[k])} times")

    def count(k):
        v = _one(d, k, "0")
        try:
            n = int(v)
        except ValueError:
            raise RtErr(f"solver prototxt: {k}: {v!r} is not an integer")
        if n < 0:
            raise RtErr(f"solver prototxt: {k}={n}: not negative")
        return n
    ti = str(_one(d, "test_initialization", "true")).lower()
    if ti not in ("true", "false"):
        raise RtErr(f"solver prototxt: test_initialization: {ti!r} is neither true nor false")
    return {"test_iter": count("test_iter"), "test_interval": count("test_interval"), "test_initialization": ti == "true"}


def accuracy_layers(text: str) -> List[Tuple[str, str, str, int]]:
    """-> [(name, bottom, label, top_k)] of a net definition's Accuracy layers, in definition order (a TRAIN-phase-only layer is left out): what to score (the blob an
    EvalPipe's loss reads) and under which k.  top_k defaults to 1 (AccuracyParameter, src/ext/caffe.proto).  ignore_label and an axis other than 1 are an UnsupErr
    that names the key.  The shape-inference readers above keep ignoring these layers."""
    from .op import UnsupErr
    root = parse(text)
    out: List[Tuple[str, str, str, int]] = []
    for L in root.get("layer", []) or root.get("layers", []):
        if not _is_test_phase(L) or str(_one(L, "type")).upper().replace("_", "") != "ACCURACY":
            continue
        name, bots = str(_one(L, "name")), L.get("bottom", [])
        if len(bots) != 2:
            raise RtErr(f"prototxt: Accuracy layer {name!r} has {len(bots)} bottoms: the scores and the label")
        ap = _one(L, "accuracy_param", {})
        if "ignore_label" in ap:
            raise UnsupErr(f"prototxt: Accuracy layer {name!r}: ignore_label is not provided (hip_accuracy counts every image; a label outside [0, chan) is a miss)")
        if int(_one(ap, "axis", 1)) != 1:
            raise UnsupErr(f"prototxt: Accuracy layer {name!r}: axis={_one(ap, 'axis')}: only axis 1, the channels, is provided")
        k = int(_one(ap, "top_k", 1))
        if k < 1:
            raise RtErr(f"prototxt: Accuracy layer {name!r}: top_k={k}: at least 1")
        out.append((name, str(bots[0]), str(bots[1]), k))
    return out


def transform_spec(text: str, phase: str) -> dict:
    """The transform_param of a net definition's Data layer of `phase` ("train" | "test") -> {"crop_size", "mirror", "scale", "mean_value", "mean_file"}: what
    input_pipe.InputTransform takes (the caller reads mean_file into an array).  A layer without an include block belongs to both phases.  Absent keys get Caffe's
    defaults: crop_size 0 (the whole source), mirror false, scale 1, mean_value [], mean_file "".  mean_file and mean_value together are an RtErr, as in Caffe; force_color
    / force_gray set are an UnsupErr that names the key.  conv_ops and pipe_spec keep reading crop_size alone."""
    from .op import UnsupErr
    if phase not in ("train", "test"):
        raise RtErr(f"prototxt: transform_spec: phase must be 'train' | 'test', got {phase!r}")
    root = parse(text)
    for L in root.get("layer", []) or root.get("layers", []):
        if str(_one(L, "type")).upper().replace("_", "") != "DATA":
            continue
        incs = [str(_one(inc, "phase", "")).upper() for inc in L.get("include", [])]
        if incs and phase.upper() not in incs:
            continue
        name = _one(L, "name")
        tp = _one(L, "transform_param", {})
        if not isinstance(tp, dict):
            raise RtErr(f"prototxt: Data layer {name!r}: transform_param must be a block")
        for k in ("force_color", "force_gray"):
            if str(_one(tp, k, "false")).lower() == "true":
                raise UnsupErr(f"prototxt: Data layer {name!r}: {k} is not provided (hip_data_transform keeps the source's channels)")
        for k in ("crop_size", "mirror", "scale", "mean_file"):
            if len(tp.get(k, [])) > 1:
                raise RtErr(f"prototxt: Data layer {name!r}: {k!r} is given {len(tp[k])} times")
        try:
            crop, scale, mv = int(_one(tp, "crop_size", 0)), float(_one(tp, "scale", 1.0)), [float(v) for v in tp.get("mean_value", [])]
        except (ValueError, TypeError):
            raise RtErr(f"prototxt: Data layer {name!r}: crop_size, scale and mean_value must be numbers")
        mirror = str(_one(tp, "mirror", "false")).lower()
        if mirror not in ("true", "false"):
            raise RtErr(f"prototxt: Data layer {name!r}: mirror: {mirror!r} is neither true nor false")
        mf = str(_one(tp, "mean_file", ""))
        if mf and mv:
            raise RtErr(f"prototxt: Data layer {name!r}: both mean_file and mean_value are given; Caffe takes one of them")
        if crop < 0:
            raise RtErr(f"prototxt: Data layer {name!r}: crop_size={crop}: not negative")
        return {"crop_size": crop, "mirror": mirror == "true", "scale": scale, "mean_value": mv, "mean_file": mf}
    raise RtErr(f"prototxt: transform_spec: no Data layer of the {phase} phase")


def freeze_spec(text: str, cp=None):
    """What a net definition says about fine-tuning -> bck_pipe.Freeze.  A Convolution / InnerProduct / Scale layer all of whose
    `param { lr_mult }` entries are 0 (at least one entry; an entry without lr_mult has Caffe's default 1) becomes a frozen op tag in `params`; a BatchNorm layer with
    `batch_norm_param { use_global_stats: true }` becomes a `bn_global_stats` entry (none: False).  A BatchNorm layer's own three `lr_mult: 0` blobs are ignored: its
    statistics are never solver params here.  Layers of every phase are read, each name once.  use_global_stats on a layer that is no BatchNorm is an RtErr.  cp (a
    ConvPipe, optional): every layer named must then be an op of that pipe, and a name that is not is an RtErr that names it."""
    root = parse(text)
    params: List[str] = []
    bn_global: List[str] = []
    seen = set()
    for L in root.get("layer", []) or root.get("layers", []):
        name, t = str(_one(L, "name")), str(_one(L, "type")).upper().replace("_", "")
        if name in seen:
            continue
        seen.add(name)
        bnp = _one(L, "batch_norm_param", {})
        if isinstance(bnp, dict) and "use_global_stats" in bnp and t != "BATCHNORM":
            raise RtErr(f"prototxt: freeze_spec: layer {name!r} is a {_one(L, 'type')}, not a BatchNorm: use_global_stats is a BatchNorm layer's")
        if t == "BATCHNORM":
            if isinstance(bnp, dict) and str(_one(bnp, "use_global_stats", "false")).lower() == "true":
                bn_global.append(name)
            continue
        if t not in ("CONVOLUTION", "INNERPRODUCT", "SCALE"):
            continue
        try:
            mults = [float(_one(p, "lr_mult", 1.0)) for p in L.get("param", []) if isinstance(p, dict)]
        except (ValueError, TypeError):
            raise RtErr(f"prototxt: freeze_spec: layer {name!r}: lr_mult must be a number")
        if mults and all(m == 0.0 for m in mults):
            params.append(name)
    if cp is not None:
        tags = {o.tag for o in cp.ops}
        for name in params + bn_global:
            if name not in tags:
                raise RtErr(f"prototxt: freeze_spec: layer {name!r} is no op of the pipe {cp.name!r}")
    return Freeze(params=tuple(params), bn_global_stats=list(bn_global) if bn_global else False)


_LOSS_NORMS = {"FULL": "full", "VALID": "valid", "BATCH_SIZE": "batch_size", "NONE": "none"}


def loss_spec(text: str, phase: str = "TRAIN"):
    """-> [(name, bottom, label, bck_graph.LossSpec)] of a net definition's SoftmaxWithLoss layers of `phase` ("TRAIN" | "TEST"), in definition order: what add_bck_ops
    takes as loss_tops and loss_specs.  A layer without an include block belongs to both phases; one of the other phase alone is left out.
    Read: loss_weight (the first one: the loss top's) -> weight; loss_param { ignore_label, normalization: FULL | VALID | BATCH_SIZE | NONE } and the legacy
    `normalize:` key, which counts only where normalization is absent (true -> valid, false -> batch_size), as in Caffe.  Absent keys get Caffe's defaults: weight 1,
    no ignore_label, VALID.  Any other layer whose type ends in Loss is an UnsupErr that names the type: only the softmax loss has kernels here."""
    from .bck_graph import LossSpec
    from .op import UnsupErr
    phase = str(phase).upper()
    if phase not in ("TRAIN", "TEST"):
        raise RtErr(f"prototxt: loss_spec: phase must be 'TRAIN' | 'TEST', got {phase!r}")
    root = parse(text)
    out = []
    for L in root.get("layer", []) or root.get("layers", []):
        tname = str(_one(L, "type"))
        t = tname.upper().replace("_", "")
        if not t.endswith("LOSS"):
            continue
        incs = [str(_one(inc, "phase", "")).upper() for inc in L.get("include", []) if isinstance(inc, dict)]
        if incs and phase not in incs:
            continue
        name, bots = str(_one(L, "name")), L.get("bottom", [])
        if t not in ("SOFTMAXWITHLOSS", "SOFTMAXLOSS"):
            raise UnsupErr(f"prototxt: loss_spec: layer {name!r} is a {tname}: only SoftmaxWithLoss has kernels here (other loss layers are not built)")
        if len(bots) != 2:
            raise RtErr(f"prototxt: SoftmaxWithLoss layer {name!r} has {len(bots)} bottoms: the scores and the label")
        lp = _one(L, "loss_param", {})
        if not isinstance(lp, dict):
            raise RtErr(f"prototxt: SoftmaxWithLoss layer {name!r}: loss_param must be a block")
        for k in ("ignore_label", "normalization", "normalize"):
            if len(lp.get(k, [])) > 1:
                raise RtErr(f"prototxt: SoftmaxWithLoss layer {name!r}: {k!r} is given {len(lp[k])} times")
        try:
            weight = float(_one(L, "loss_weight", 1.0))
        except (ValueError, TypeError):
            raise RtErr(f"prototxt: SoftmaxWithLoss layer {name!r}: loss_weight must be a number")
        ig = _one(lp, "ignore_label")
        if ig is not None:
            try:
                ig = int(ig)
            except (ValueError, TypeError):
                raise RtErr(f"prototxt: SoftmaxWithLoss layer {name!r}: ignore_label: {ig!r} is not an integer")
        if "normalization" in lp:
            nz = str(_one(lp, "normalization")).upper()
            if nz not in _LOSS_NORMS:
                raise RtErr(f"prototxt: SoftmaxWithLoss layer {name!r}: normalization: {nz!r} is none of {' | '.join(_LOSS_NORMS)}")
            norm = _LOSS_NORMS[nz]
        elif "normalize" in lp:
            nb = str(_one(lp, "normalize")).lower()
            if nb not in ("true", "false"):
                raise RtErr(f"prototxt: SoftmaxWithLoss layer {name!r}: normalize: {nb!r} is neither true nor false")
            norm = "valid" if nb == "true" else "batch_size"
        else:
            norm = "valid"
        out.append((name, str(bots[0]), str(bots[1]), LossSpec(weight=weight, ignore_label=ig, normalization=norm).check()))
    return out
