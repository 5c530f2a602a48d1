"""The graph reversal of the gradient pipe, pure and without a backend: `add_bck_ops` turns a ConvPipe into the BckPipe of forward, loss and gradient ops (GradOp),
`grad_op_to_op` writes one of them as an op_base_t, `plan_relu_grad_folds` says which ReLU gradients the call before them can take.

Restates the behaviour of the reference's add_bck_ops=1 path (not its code):
  * conv_pipe_t::add_bck_ops / add_bck_ops_rec / add_bck_ops_op / get_grad_loss_onn     src/conv_util.cc:729-879
      every forward top is capped with a SoftmaxWithLoss (which itself writes <in>_grad_loss); every other forward op gets its gradient op -- Pooling -> Spreading,
      LRN -> BckLRN, ReLU -> ZeroIfNonPos, Dropout -> BckDropout, Convolution -> BckConv, Concat -> Split; a node read by more than one op gets one partial gradient
      per reader and a Reduce that sums them.  The list is built by a topological walk from the sources and appended REVERSED.
Where this departs from the reference, on purpose:
  * an AVERAGE pooling keeps emit_out_in_yx=0 (an average has no argmax; the op layer refuses avg_pool=1 with emit_out_in_yx=1): hip_pool_yx then writes the average and
    an <out>_in_yx of -1s, which is what the reference's template leaves there
  * the forward ops run in the ConvPipe's definition order, which is a topological order like the reference's walk
"""
from __future__ import annotations
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from .conv_pipe import ConvPipe, PipeOp
from .op import LOSS_NORMALIZATIONS, Dims, Nda, Op, RtErr, UnsupErr

IN_PLACE_TYPES = ("ReLU", "Dropout", "BckDropout")   # and a ZeroIfNonPos whose out is its in (src/conv_util.cc:273-279)
AFFINE_IN_PLACE_TYPES = ("BatchNorm", "Scale")       # ResNet's: in place on the node a convolution wrote, like a ReLU; their gradient ops must run in TRUE reverse order
DROPOUT_RATIO = 0.5   # Dropout_coi's default (src/conv_util.cc:39); the ConvPipe records carry no ratio


@dataclass(frozen=True)
class LossSpec:
    """A SoftmaxWithLoss as Caffe defines it (SoftmaxWithLossLayer, LossParameter), restated.  weight: loss_weight, which scales the head's gradient and not the loss
    node (Caffe's top blob is unweighted too).  ignore_label: an integer; a pel whose label equals it adds nothing to the loss, gets a +0 gradient and is not counted by
    the normaliser (None: no label is ignored; a value inside [0, chan) ignores that class).  normalization: what the summed loss and the gradient are divided by --
    "valid": max(1, the pels that are not ignored), "full": img * y * x, "batch_size": img, "none": 1.  A label outside [0, chan) that is not ignored (a NaN included)
    is INVALID: it matches no channel, costs -logf(FLT_MIN) and counts towards the normaliser.  The defaults are Caffe's."""
    weight: float = 1.0
    ignore_label: Optional[int] = None
    normalization: str = "valid"

    def check(self) -> "LossSpec":
        if self.normalization not in LOSS_NORMALIZATIONS:
            raise RtErr(f"LossSpec: normalization must be {' | '.join(LOSS_NORMALIZATIONS)}, got {self.normalization!r}")
        w = self.weight
        if isinstance(w, bool) or not isinstance(w, (int, float, np.floating, np.integer)) or not np.isfinite(w):
            raise RtErr(f"LossSpec: weight must be a finite number, got {w!r}")
        ig = self.ignore_label
        if ig is not None and (isinstance(ig, bool) or not isinstance(ig, (int, np.integer))):
            raise RtErr(f"LossSpec: ignore_label must be an integer or None, got {ig!r}")
        return self


@dataclass
class GradOp:
    """One op of the pipe with gradient ops: the reference's conv_op_t reduced to tag / type / bots / tops.  `src` is the forward PipeOp whose parameters it carries;
    `spec` the LossSpec of a SoftmaxWithLoss that runs as the full loss (None: the reference's three calls)."""
    tag: str
    type: str
    bots: List[str]
    tops: List[str]
    src: Optional[PipeOp] = None
    spec: Optional[LossSpec] = None

    @property
    def in_place(self) -> bool:
        return self.type in IN_PLACE_TYPES or self.type in AFFINE_IN_PLACE_TYPES or (self.type == "ZeroIfNonPos" and self.tops[0] == self.bots[0])


@dataclass
class _Node:
    top_for: List[str] = field(default_factory=list)
    bot_for: List[str] = field(default_factory=list)
    in_place_ops: List[GradOp] = field(default_factory=list)


@dataclass
class BckPipe:
    """What add_bck_ops returns: the forward ops, the loss ops and the gradient ops in run order, and every node's dims."""
    cp: ConvPipe
    ops: List[GradOp]
    nodes: Dict[str, Dims]
    label_node: str
    n_fwd: int                                  # ops[:n_fwd] are the forward ops and the SoftmaxWithLoss caps
    loss_nodes: List[str] = field(default_factory=list)

    def fwd_ops(self) -> List[GradOp]:
        return self.ops[:self.n_fwd]

    def bck_ops(self) -> List[GradOp]:
        return self.ops[self.n_fwd:]


def _fwd_grad_op(cp: ConvPipe, o: PipeOp) -> GradOp:
    if o.type in ("Convolution", "Deconvolution"):
        return GradOp(o.tag, o.type, [o.bot, o.tag + "_filts", o.tag + "_biases"], [o.top], o)
    if o.type == "Crop":   # (reads bots[0] alone: the second bottom gives only the size, and gets no gradient from a Crop)
        return GradOp(o.tag, o.type, [o.bot], [o.top], o)
    if o.type in ("Concat", "Eltwise"):
        return GradOp(o.tag, o.type, list(o.bots), [o.top], o)
    if o.type == "BatchNorm":   # in place; the running statistics are params it reads AND rewrites
        return GradOp(o.tag, o.type, [o.bot, o.tag + "_mean", o.tag + "_var"], [o.top], o)
    if o.type == "Scale":
        return GradOp(o.tag, o.type, [o.bot, o.tag + "_scale", o.tag + "_bias"], [o.top], o)
    return GradOp(o.tag, o.type, [o.bot], [o.top], o)


def _reader_graph(fwd: List[GradOp]) -> Tuple[Dict[str, _Node], Dict[str, GradOp]]:
    """The graph as the reference holds it: in-place ops hang off their node and are in nobody's bot_for / top_for (src/conv_util.cc:273-292); and the ops by tag."""
    g: Dict[str, _Node] = {}
    by_tag: Dict[str, GradOp] = {}
    for o in fwd:
        if o.tag in by_tag:
            raise RtErr(f"add_bck_ops: op tag {o.tag!r} used twice")
        by_tag[o.tag] = o
        if o.in_place:
            g.setdefault(o.bots[0], _Node()).in_place_ops.append(o)
            continue
        for t in o.tops:
            g.setdefault(t, _Node()).top_for.append(o.tag)
        for b in o.bots:
            g.setdefault(b, _Node()).bot_for.append(o.tag)
    return g, by_tag


def _bck_of(cop: GradOp, grad_loss_onn) -> Optional[GradOp]:
    """The gradient op of forward op cop; grad_loss_onn(cop, inn) names the node that takes cop's contribution to inn's gradient."""
    t, tag = cop.type, cop.tag + "_bck"
    if t == "SoftmaxWithLoss":
        assert cop.bots[0] + "_grad_loss" == cop.tops[0]
        return None
    if t == "Pooling":    # { out, out_grad_loss, in } -> in_grad_loss
        return GradOp(tag, "Spreading", [cop.tops[0], cop.tops[0] + "_grad_loss", cop.bots[0]], [grad_loss_onn(cop, cop.bots[0])], cop.src)
    if t == "ReLU":       # { in = X_grad_loss, cond = X } -> X_grad_loss
        return GradOp(tag, "ZeroIfNonPos", [cop.tops[0] + "_grad_loss", cop.bots[0]], [grad_loss_onn(cop, cop.bots[0])], cop.src)
    if t == "Dropout":
        return GradOp(tag, "BckDropout", [cop.tops[0] + "_grad_loss"], [grad_loss_onn(cop, cop.bots[0])], cop.src)
    if t == "Convolution":   # { in, filts, biases, out_grad_loss } -> the three gradients
        return GradOp(tag, "BckConv", cop.bots + [cop.tops[0] + "_grad_loss"], [grad_loss_onn(cop, b) for b in cop.bots], cop.src)
    if t == "Deconvolution":   # BckConv's shape: { in, filts, biases, out_grad_loss } -> the three gradients
        return GradOp(tag, "BckDeconv", cop.bots + [cop.tops[0] + "_grad_loss"], [grad_loss_onn(cop, b) for b in cop.bots], cop.src)
    if t == "Crop":            # { out_grad_loss } -> a_grad_loss: out_grad_loss inside the window, +0 outside it
        return GradOp(tag, "BckCrop", [cop.tops[0] + "_grad_loss"], [grad_loss_onn(cop, cop.bots[0])], cop.src)
    if t == "Concat":
        return GradOp(tag, "Split", [cop.tops[0] + "_grad_loss"], [grad_loss_onn(cop, b) for b in cop.bots], cop.src)
    if t == "LRN":        # { in, out, out_grad_loss } -> in_grad_loss
        return GradOp(tag, "BckLRN", [cop.bots[0], cop.tops[0], cop.tops[0] + "_grad_loss"], [grad_loss_onn(cop, cop.bots[0])], cop.src)
    if t == "Scale":      # { X_grad_loss, X, scale } -> X_grad_loss in place, and the two param gradients
        gl = grad_loss_onn(cop, cop.bots[0])
        return GradOp(tag, "BckScale", [cop.tops[0] + "_grad_loss", cop.bots[0], cop.bots[1]], [gl, cop.bots[1] + "_grad_loss", cop.bots[2] + "_grad_loss"], cop.src)
    if t == "BatchNorm":  # { X_grad_loss, X } -> X_grad_loss in place; _mean / _var get no gradient node
        return GradOp(tag, "BckBatchNorm", [cop.tops[0] + "_grad_loss", cop.bots[0]], [grad_loss_onn(cop, cop.bots[0])], cop.src)
    if t == "Eltwise":    # { top_grad_loss } -> one gradient node per bottom (a SUM hands its gradient to every term)
        return GradOp(tag, "BckEltwise", [cop.tops[0] + "_grad_loss"], [grad_loss_onn(cop, b) for b in cop.bots], cop.src)
    raise RtErr(f"FIXME: add_bck_ops: unhandled cop->type={t}")


def _append_reversed(cp: ConvPipe, nodes: Dict[str, Dims], fwd: List[GradOp], walk: List[GradOp]) -> List[GradOp]:
    """fwd + the walk's gradient ops appended in reverse, each given its tops' dims in `nodes`; a Reduce is kept only if nobody wrote its output yet and its first
    input exists (src/conv_util.cc:866-877): `label` has none."""
    out = list(fwd)
    for b in reversed(walk):
        if b.type == "Reduce" and not (b.tops[0] not in nodes and b.bots[0] in nodes):
            continue
        for i in b.bots:
            if i not in nodes:
                raise RtErr(f"add_bck_ops: gradient op {b.tag} reads {i!r}, which no earlier op writes")
        if b.type in ("BckConv", "BckDeconv"):
            for t, s in zip(b.tops, b.bots[:3]):
                nodes[t] = nodes[s]
        elif b.type in ("Split", "BckEltwise"):
            if b.type == "BckEltwise" and len(set(b.tops)) != len(b.tops):
                raise UnsupErr(f"add_bck_ops: {b.tag}: the Eltwise sums one node twice")
            for t, s in zip(b.tops, b.src.bots):
                nodes[t] = nodes[s]
        elif b.type == "BckScale":
            nodes[b.tops[0]] = nodes[b.bots[0]]
            nodes[b.tops[1]] = cp.params[b.src.tag + "_scale"]; nodes[b.tops[2]] = cp.params[b.src.tag + "_bias"]
        elif b.type in ("Spreading", "BckLRN", "BckCrop"):
            nodes[b.tops[0]] = nodes[b.src.bot]
        elif b.type == "Reduce":
            if not 2 <= len(b.bots) <= 8:
                raise UnsupErr(f"add_bck_ops: {b.tag} sums {len(b.bots)} partial gradients; hip_reduce takes 2 to 8")
            nodes[b.tops[0]] = nodes[b.bots[0]]
        else:                 # ZeroIfNonPos, BckDropout: in place on the gradient
            nodes[b.tops[0]] = nodes[b.bots[0]]
        out.append(b)
    return out


def _specs_of(loss_tops: List[str], loss_specs) -> List[Optional[LossSpec]]:
    """loss_specs as add_bck_ops takes it -> one LossSpec or None per loss top, each checked."""
    if loss_specs is None:
        specs: List[Optional[LossSpec]] = [None] * len(loss_tops)
    elif isinstance(loss_specs, LossSpec):
        specs = [loss_specs] * len(loss_tops)
    elif isinstance(loss_specs, dict):
        for t in loss_specs:
            if t not in loss_tops:
                raise RtErr(f"add_bck_ops: loss_specs names {t!r}, which is no loss top ({', '.join(loss_tops)})")
        specs = [loss_specs.get(t) for t in loss_tops]
    elif isinstance(loss_specs, (list, tuple)):
        if len(loss_specs) != len(loss_tops):
            raise RtErr(f"add_bck_ops: {len(loss_specs)} loss_specs for {len(loss_tops)} loss tops")
        specs = list(loss_specs)
    else:
        raise RtErr(f"add_bck_ops: loss_specs must be None, a LossSpec, a dict top -> LossSpec or a sequence aligned with loss_tops, got {type(loss_specs).__name__}")
    for s in specs:
        if s is not None and not isinstance(s, LossSpec):
            raise RtErr(f"add_bck_ops: loss_specs holds a {type(s).__name__}, not a LossSpec")
    return [s.check() if s is not None else None for s in specs]


def add_bck_ops(cp: ConvPipe, label_node: str = "label", loss_tops: Optional[Sequence[str]] = None, loss_specs=None) -> BckPipe:
    """The pipe of `cp` with gradient ops.  `loss_tops`: the forward nodes to cap with a SoftmaxWithLoss (default: the pipe's out node; GoogLeNet's auxiliary heads are
    named here).  One cap is tagged `loss` and writes the node `loss`; several are tagged loss1, loss2, ... in the order given.  All of them read `label_node`, whose
    dims are img:y:x of the heads' plane (heads that share it must share the plane).
    `loss_specs`: None, one LossSpec for every head, a dict top -> LossSpec, or a sequence aligned with loss_tops.  A head without a spec on a 1 x 1 plane is the
    reference's gradient-test loss (three calls, divided by the image count); a head with a spec, and any head on a larger plane (as if given LossSpec()), is the full
    SoftmaxWithLoss: GradOp.spec carries it."""
    loss_tops = list(loss_tops) if loss_tops else [cp.out_node()]
    specs = _specs_of(loss_tops, loss_specs)
    fwd = [_fwd_grad_op(cp, o) for o in cp.ops]
    nodes: Dict[str, Dims] = dict(cp.nodes); nodes.update(cp.params)
    if label_node in nodes:
        raise RtErr(f"add_bck_ops: the pipe already has a node {label_node!r}")
    loss_nodes = []
    for i, t in enumerate(loss_tops):
        if t not in cp.nodes:
            raise RtErr(f"add_bck_ops: loss top {t!r} is no node of the pipe")
        tag = "loss" if len(loss_tops) == 1 else f"loss{i + 1}"
        if tag in nodes or t + "_grad_loss" in nodes:
            raise RtErr(f"add_bck_ops: node {tag!r} / {t + '_grad_loss'!r} already exists")
        td = cp.nodes[t]
        plane = (td.dsz("img"), td.dsz("y"), td.dsz("x")) if td.names == ("img", "chan", "y", "x") else (td.dsz("img"), 1, 1)
        spec = specs[i] if specs[i] is not None or plane[1:] == (1, 1) else LossSpec()
        if spec is not None and plane[0] * plane[1] * plane[2] >= 2 ** 24:
            raise RtErr(f"add_bck_ops: loss top {t!r}: img * y * x = {plane[0] * plane[1] * plane[2]} pels: 2^24 or more, and the pel count must be exact as a float")
        label_dims = Dims.make("float", img=plane[0], y=plane[1], x=plane[2])
        if label_node in nodes and nodes[label_node] != label_dims:
            raise RtErr(f"add_bck_ops: loss top {t!r} has the plane {label_dims.pretty()}, an earlier head {nodes[label_node].pretty()}: heads that share the label node "
                        f"{label_node!r} must share its plane")
        fwd.append(GradOp(tag, "SoftmaxWithLoss", [t, label_node], [t + "_grad_loss", tag], spec=spec))
        nodes[t + "_grad_loss"] = cp.nodes[t]
        nodes[tag] = Dims.make("float", y=1, x=1)
        nodes[label_node] = label_dims
        loss_nodes.append(tag)

    g, by_tag = _reader_graph(fwd)

    def grad_loss_onn(cop: GradOp, inn: str) -> str:
        """The node that takes cop's contribution to inn's gradient: inn_grad_loss, or -- inn read by several ops and cop not in place -- the partial
        inn_<producer or last in-place op>_0_split_<reader index>_grad_loss (get_grad_loss_onn)."""
        n = g[inn]
        if len(n.bot_for) == 1 or cop.in_place:
            return inn + "_grad_loss"
        wopn = "_" + inn   # data / label ...
        if n.top_for:
            wopn = "_" + (n.in_place_ops[-1].tag if n.in_place_ops else n.top_for[0])
        return f"{inn}{wopn}_0_split_{n.bot_for.index(cop.tag)}_grad_loss"

    seen: Dict[str, int] = {}
    walk: List[GradOp] = []

    def rec(nn: str) -> None:
        n = g[nn]
        if not n.bot_for:   # a sink: must be what a SoftmaxWithLoss wrote
            if len(n.top_for) != 1 or by_tag[n.top_for[0]].type != "SoftmaxWithLoss":
                raise RtErr(f"add_bck_ops: unhandled: top node {nn} not produced by SoftmaxWithLoss op")
        # the walk appends a node's in-place gradient ops reversed and the whole list is reversed again below: they RUN in forward order, which is harmless for ReLU /
        # Dropout (they commute; the reference does the same and existing lists pin it) and wrong for [BatchNorm, Scale, ReLU].  A node with a BatchNorm or a Scale
        # among its in-place ops gets them in true reverse: ZeroIfNonPos, BckScale, BckBatchNorm
        affine = any(ip.type in AFFINE_IN_PLACE_TYPES for ip in n.in_place_ops)
        for ip in (n.in_place_ops if affine else reversed(n.in_place_ops)):
            b = _bck_of(ip, grad_loss_onn)
            if b:
                walk.append(b)
        if len(n.bot_for) > 1:
            walk.append(GradOp("reduce_" + nn + "_grad_loss", "Reduce", [grad_loss_onn(by_tag[r], nn) for r in n.bot_for], [nn + "_grad_loss"]))
        for r in n.bot_for:
            cop = by_tag[r]
            seen[r] = seen.get(r, 0) + 1
            if seen[r] != len(cop.bots):   # wait until all its bottoms were seen
                continue
            b = _bck_of(cop, grad_loss_onn)
            if b:
                walk.append(b)
            for t in cop.tops:
                rec(t)

    for src in sorted(nn for nn, n in g.items() if not n.top_for):   # the reference's `bots`, a sorted set of names
        rec(src)

    return BckPipe(cp, _append_reversed(cp, nodes, fwd, walk), nodes, label_node, len(fwd), loss_nodes)


# ------------------------------------------------------------------------------------------------
# ops of the pipe as op_base_t lines
# ------------------------------------------------------------------------------------------------
_none = lambda y, x: Nda(Dims(("y", "x"), (y, x), "none"), "none")
_u32 = lambda v: Nda(None, "uint32_t", (int(v),))
_f32 = lambda v: Nda(None, "float", (float(np.float32(v)),))


def grad_op_to_op(bp: BckPipe, o: GradOp) -> Op:
    """The op_base_t of one op of the pipe, with the reference's arg names (boda_amd/op.py OP_INFO)."""
    nd = lambda n: Nda(bp.nodes[n])
    s, t = o.src, o.type
    if t in ("Convolution", "BckConv"):
        v = {"in": nd(o.bots[0]), "filts": nd(o.bots[1]), "biases": nd(o.bots[2]), "kern_sz": _none(*s.kern_sz), "stride": _none(*s.stride), "in_pad": _none(*s.in_pad),
             "out_chans": _u32(s.out_chans)}
        if getattr(s, "group", 1) > 1:   # (an ungrouped layer's op is what it has always been)
            v["group"] = _u32(s.group)
        if t == "Convolution":
            v["out"] = nd(o.tops[0])
        else:
            v.update({"out_grad_loss": nd(o.bots[3]), "in_grad_loss": Nda(bp.nodes[o.bots[0]]), "filts_grad_loss": nd(o.tops[1]), "biases_grad_loss": nd(o.tops[2])})
        return Op({"type": t}, v)
    if t in ("Deconvolution", "BckDeconv"):
        v = {"in": nd(o.bots[0]), "filts": nd(o.bots[1]), "biases": nd(o.bots[2]), "kern_sz": _none(*s.kern_sz), "stride": _none(*s.stride), "in_pad": _none(*s.in_pad),
             "out_chans": _u32(s.out_chans)}
        if t == "Deconvolution":
            v["out"] = nd(o.tops[0])
        else:
            v.update({"out_grad_loss": nd(o.bots[3]), "in_grad_loss": Nda(bp.nodes[o.bots[0]]), "filts_grad_loss": nd(o.tops[1]), "biases_grad_loss": nd(o.tops[2])})
        return Op({"type": t}, v)
    if t == "Crop":
        return Op({"type": t}, {"in": nd(o.bots[0]), "out": nd(o.tops[0]), "offset": _none(*s.offset)})
    if t == "BckCrop":
        return Op({"type": t}, {"out_grad_loss": nd(o.bots[0]), "in_grad_loss": Nda(bp.nodes[s.bot]), "offset": _none(*s.offset)})
    if t in ("Pooling", "Spreading"):
        v = {"kern_sz": _none(*s.kern_sz), "stride": _none(*s.stride), "in_pad": _none(*s.in_pad), "avg_pool": _u32(s.avg_pool), "emit_out_in_yx": _u32(0 if s.avg_pool else 1)}
        if t == "Pooling":
            v.update({"in": nd(o.bots[0]), "out": nd(o.tops[0])})
        else:
            v.update({"out": nd(o.bots[0]), "out_grad_loss": nd(o.bots[1]), "in": nd(o.bots[2]), "in_grad_loss": nd(o.tops[0])})
        return Op({"type": t}, v)
    if t in ("LRN", "BckLRN"):
        ls, alpha, beta, k = s.lrn
        v = {"local_size": _u32(ls), "alpha": _f32(alpha), "beta": _f32(beta), "k": _f32(k), "emit_out_scale_base": _u32(1)}
        if t == "LRN":
            v.update({"in": nd(o.bots[0]), "out": nd(o.tops[0])})
        else:
            v.update({"in": nd(o.bots[0]), "out": nd(o.bots[1]), "out_grad_loss": nd(o.bots[2]), "in_grad_loss": nd(o.tops[0])})
        return Op({"type": t}, v)
    if t == "ZeroIfNonPos":
        return Op({"type": t}, {"in": nd(o.bots[0]), "cond": nd(o.bots[1]), "out": nd(o.tops[0])})
    if t == "ReLU":
        return Op({"type": t}, {"in": nd(o.bots[0]), "out": nd(o.tops[0])})
    if t in ("Dropout", "BckDropout"):
        return Op({"type": t}, {"in": nd(o.bots[0]), "out": nd(o.tops[0]), "dropout_ratio": _f32(getattr(s, "dropout_ratio", DROPOUT_RATIO))})
    if t == "SoftmaxWithLoss":
        return Op({"type": t}, {"in": nd(o.bots[0]), "label": nd(o.bots[1]), "in_grad_loss": nd(o.tops[0]), "loss": nd(o.tops[1])})
    if t in ("Reduce", "Concat", "Eltwise"):   # (an Eltwise SUM runs as a Reduce: a sequential fp32 chain from +0 in the order of its bottoms)
        v = {f"ins_{i}": nd(b) for i, b in enumerate(o.bots)}
        v.update({"ins_num": _u32(len(o.bots)), "out": nd(o.tops[0])})
        return Op({"type": "Reduce" if t == "Eltwise" else t}, v)
    if t == "Split":
        v = {f"outs_{i}": nd(b) for i, b in enumerate(o.tops)}
        v.update({"outs_num": _u32(len(o.tops)), "in": nd(o.bots[0])})
        return Op({"type": t}, v)
    raise UnsupErr(f"bck_pipe: op type {t!r} (op {o.tag}) has no native function")


RELU_GRAD_PRODUCERS = {"BckConv": 0, "Spreading": 2, "BckLRN": 0}   # gradient op type -> index among its bots of the forward op's `in`


def plan_relu_grad_folds(bp: BckPipe) -> Tuple[Dict[str, str], Dict[str, str]]:
    """Which ReLU gradients can be taken into the call before them -> ({ZeroIfNonPos tag: tag of the gradient op that takes it}, {ZeroIfNonPos tag: why not}).
    A ZeroIfNonPos folds exactly when it is in place on X_grad_loss, the gradient op immediately before it is a BckConv / Spreading / BckLRN whose in_grad_loss node
    is that X_grad_loss, and that op's forward `in` node is the ZeroIfNonPos's cond X: the producer then applies the mask on its own store (zero_if_in_non_pos=1)."""
    bck = bp.bck_ops()
    folds: Dict[str, str] = {}
    why: Dict[str, str] = {}
    for i, o in enumerate(bck):
        if o.type != "ZeroIfNonPos":
            continue
        gl, x = o.bots
        prev = bck[i - 1] if i else None
        if o.tops[0] != gl:
            why[o.tag] = f"not in place: reads {gl}, writes {o.tops[0]}"
        elif any(q.type == "BckDropout" and q.tops[0] == gl for q in bck):
            # (a Dropout rewrites X in place behind the ReLU, so X is no longer the ReLU's output alone.  The reference's walk puts that BckDropout AFTER this op, right
            # behind the producer's call; the pair is left as it is all the same: fusing across a BckDropout is a change of its own)
            why[o.tag] = f"a BckDropout works in place on {gl} as well: {x} is rewritten by a Dropout behind the ReLU"
        elif prev is None:
            why[o.tag] = f"{gl} is written by a SoftmaxWithLoss, no gradient op runs before it"
        elif prev.type not in RELU_GRAD_PRODUCERS:
            why[o.tag] = f"the op before it is {prev.tag}, a {prev.type}" + (f": {gl} sums the partial gradients of {x}'s readers" if prev.type == "Reduce" else
                                                                             f" between {gl}'s producer and the ReLU gradient" if prev.type == "BckDropout" else "")
        elif prev.type == "BckConv" and getattr(prev.src, "group", 1) > 1:
            why[o.tag] = f"the op before it, {prev.tag}, is a grouped convolution's gradient (group={prev.src.group}): hip_bconv_in_grp takes no zero_if_in_non_pos"
        elif prev.tops[0] != gl:
            why[o.tag] = f"the op before it, {prev.tag}, writes {prev.tops[0]}, not {gl}"
        elif prev.bots[RELU_GRAD_PRODUCERS[prev.type]] != x:
            why[o.tag] = f"the op before it, {prev.tag}, has the forward input {prev.bots[RELU_GRAD_PRODUCERS[prev.type]]}, not {x}"
        else:
            folds[o.tag] = prev.tag
    return folds, why
