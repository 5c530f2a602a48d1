"""Full-net gradient pipe: the graph reversal `add_bck_ops` and the training-form driver `ConvPipeBck`.

Restates the behaviour of the reference's add_bck_ops=1 path (not its code):
  * conv_pipe_t::add_bck_ops / add_bck_ops_rec / add_bck_ops_op / get_grad_loss_onn     src/conv_util.cc:729-879
      every forward top is capped with a SoftmaxWithLoss (which itself writes <in>_grad_loss); every other forward op gets its gradient op -- Pooling -> Spreading,
      LRN -> BckLRN, ReLU -> ZeroIfNonPos, Dropout -> BckDropout, Convolution -> BckConv, Concat -> Split; a node read by more than one op gets one partial gradient
      per reader and a Reduce that sums them.  The list is built by a topological walk from the sources and appended REVERSED.
  * conv_pipe_fwd_t::gen_op, the gradient half                                          src/rtc_fwd.cc:263-405
      one call per function, vars kept on the device, the side vars <out>_in_yx / <out>_scale_base / <tag>_prob / <loss>_per_pel under those names, dropout's
      det_drop_seed a by-value argument of the call that is rewritten per step.
Every function is a native one (boda_amd/cnn_op.py: hip_conv, BCONV_FUNCS, BCK_OP_FUNCS, PIPE_OP_FUNCS), so the same pipe runs on be=hip and on be=cpu, the bit-exact
checker.  Unfused, fp32, reference layouts, one device; ConvPipe / ConvPipeFwd (the inference pipe) are not touched.

Where this departs from the reference, on purpose:
  * an AVERAGE pooling keeps emit_out_in_yx=0 (an average has no argmax; the op layer refuses avg_pool=1 with emit_out_in_yx=1): hip_pool_yx then writes the average and
    an <out>_in_yx of -1s, which is what the reference's template leaves there
  * the forward ops run in the ConvPipe's definition order, which is a topological order like the reference's walk
"""
from __future__ import annotations
import zlib
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from .cnn_op import (NATIVE_ARGS, OpTune, SGD_MAX_TENS, bn_bck_in_func_op, bn_bck_sums_func_op, bn_fwd_func_op, bn_stats_func_op, bnc_bck_in_func_op, bnc_bck_sums_func_op, bnc_fwd_func_op, bnc_stats_func_op, BNC_MAX_CHUNKS, fan_out_func_op, sgd_update_func_op, solver_update_func_op, grad_sumsq_func_op, grad_norm_func_op, grad_accum_func_op, solver_update_acc_func_op, add_bck_conv_annotations, bconv_filts_biases_func_op, add_bck_op_annotations, add_codegen_annotations, add_pipe_op_annotations, fuse_zero_if_in_non_pos, IMG_SHARDS_FUNCS, on_img_shards,
                     pipe_func_args, seed_from_var, SEED_VAR_ARG, bf16_operands)
from .cnn_op import bnf_bck_func_op, bnf_bck_in_func_op, bnf_prep_func_op, data_transform_func_op
from .conv_pipe import ConvPipe, PipeOp
from .input_pipe import DATA_RAW_VAR, DATA_XF_MEAN_VAR, DATA_XF_PLAN_VAR, DATA_XF_TAG, InputTransform
from .op import Dims, Nda, Op, RtErr, SOLVER_CHUNK, UnsupErr
from .rtc import RtcArg, RtcFuncCall, RtcFuncInfo

IN_PLACE_TYPES = ("ReLU", "Dropout", "BckDropout")   # and a ZeroIfNonPos whose out is its in (src/conv_util.cc:273-279)
AFFINE_IN_PLACE_TYPES = ("BatchNorm", "Scale")       # ResNet's: in place on the node a convolution wrote, like a ReLU; their gradient ops must run in TRUE reverse order
BN_IN_SFX = "_bn_in"                # <X>_bn_in: what the convolution in front of a BatchNorm wrote (X itself holds the normalised, scaled, rectified values)
BN_MEAN_SFX, BN_ISTD_SFX = "_batch_mean", "_batch_inv_std"   # <bn-tag>_batch_mean / _batch_inv_std: the statistics of the step's batch
BN_STAT_SFXS = ("_mean", "_var")    # a BatchNorm's params: running statistics, rewritten by the forward pass and never by a solver
DROPOUT_RATIO = 0.5   # Dropout_coi's default (src/conv_util.cc:39); the ConvPipe records carry no ratio
SEED_VAR = "det_drop_seed"   # ConvPipeBck(seed_in_var=True): the one-word uint32 var every dropout call reads its seed from
DROP_LAYER_STEP = 0x9E3779B1   # the k-th Dropout layer of a pipe hashes with seed + k * this (mod 2^32)
SGD_HYPER_VAR = "sgd_hyper"    # ConvPipeBck(solver=...): float v=4 = [lr, momentum, weight_decay, unused], read by every update call
SGD_HIST_SFX = "_sgd_hist"     # <param>_sgd_hist: the param's momentum history


@dataclass
class SgdSolver:
    """SGD with momentum and weight decay for ConvPipeBck(solver=...), Caffe's order (regularise, history, update) with the gradient left unmodified.  Per element of
    param tensor i, every operation one fp32 rounding (hip_sgd_update, cnn_op.sgd_update_func_op):
        g1 = g + (weight_decay * decay_mult_i) * w;   h' = momentum * h + (lr * lr_mult_i) * g1;   w' = w - h'
    lr_mult / decay_mult: dicts keyed by param name (`conv1_filts`) or by the suffix `filts` / `biases` / `scale` / `bias`; a name wins over a suffix, the default is 1.
    A BatchNorm's params (<tag>_mean / <tag>_var, the running statistics) are not updated: the forward pass rewrites them.
    tensors_per_call (1 .. 32): params per hip_sgd_update call, packed in the order of the pipe's params."""
    lr: float
    momentum: float = 0.9
    weight_decay: float = 5e-4
    lr_mult: Optional[Dict[str, float]] = None
    decay_mult: Optional[Dict[str, float]] = None
    tensors_per_call: int = 32

    def mult_of(self, which: Optional[Dict[str, float]], param: str) -> float:
        d = which or {}
        if param in d:
            return float(d[param])
        return float(d.get(param.rsplit("_", 1)[-1], 1.0))

    def hyper(self) -> np.ndarray:
        return np.array([self.lr, self.momentum, self.weight_decay, 0.0], np.float32)


SOLVER_HYPER_VAR = "solver_hyper"    # ConvPipeBck(solver=Solver(...)): float v=8 = [lr, momentum, weight_decay, momentum2, delta, corr, clip_gradients, unused]
SOLVER_STATE_VAR = "solver_state"    # float v=4 = [coef, norm, sumsq, 0]: what hip_grad_norm leaves and the clipping update reads
SOLVER_PARTS_VAR = "solver_gnorm_partials"   # one partial sum of squares per chunk of 4096 floats of every updated param
SGD_HIST2_SFX = "_sgd_hist2"         # <param>_sgd_hist2: adam's second-moment history
SOLVER_ACCUM_VAR = "solver_accum"    # ConvPipeBck(iter_size=n > 1): float v=4 = [first, apply, scale, micro], uploaded before every micro-step
GRAD_ACC_SFX = "_grad_acc"           # <param>_grad_acc: the sum of the param's gradients over the micro-steps since the last update


@dataclass
class LrPolicy:
    """Caffe's seven learning-rate policies, evaluated on the host in float64 (Python floats) from the written formulas; lr_at(base_lr, it) is what the driver rounds to
    fp32 and uploads for step `it` (0-based):
        fixed      base_lr
        step       base_lr * gamma ^ floor(it / stepsize)
        exp        base_lr * gamma ^ it
        inv        base_lr * (1 + gamma * it) ^ (-power)
        multistep  base_lr * gamma ^ (number of stepvalues <= it)
        poly       base_lr * (1 - it / max_iter) ^ power
        sigmoid    base_lr * (1 / (1 + exp(-gamma * (it - stepsize))))"""
    policy: str = "fixed"
    gamma: float = 0.1
    power: float = 1.0
    stepsize: int = 1
    stepvalues: Sequence[int] = ()
    max_iter: int = 1

    POLICIES = ("fixed", "step", "exp", "inv", "multistep", "poly", "sigmoid")

    def __post_init__(self):
        if self.policy not in self.POLICIES:
            raise RtErr(f"LrPolicy: policy must be one of {' | '.join(self.POLICIES)}, got {self.policy!r}")
        if self.policy in ("step", "sigmoid") and int(self.stepsize) < 1:
            raise RtErr(f"LrPolicy: {self.policy} needs stepsize >= 1, got {self.stepsize!r}")
        if self.policy == "poly" and int(self.max_iter) < 1:
            raise RtErr(f"LrPolicy: poly needs max_iter >= 1, got {self.max_iter!r}")

    def lr_at(self, base_lr: float, it: int) -> float:
        import math
        b, g, p, it = float(base_lr), float(self.gamma), float(self.power), int(it)
        if self.policy == "fixed":
            return b
        if self.policy == "step":
            return b * g ** (it // int(self.stepsize))
        if self.policy == "exp":
            return b * g ** it
        if self.policy == "inv":
            return b * (1.0 + g * it) ** (-p)
        if self.policy == "multistep":
            return b * g ** sum(1 for s in self.stepvalues if int(s) <= it)
        if self.policy == "poly":
            return b * (1.0 - it / float(self.max_iter)) ** p
        return b * (1.0 / (1.0 + math.exp(-g * (it - int(self.stepsize)))))


@dataclass
class Solver:
    """SGD, Nesterov or Adam for ConvPipeBck(solver=...), with optional global-norm gradient clipping and a learning-rate policy (hip_solver_update, hip_grad_sumsq,
    hip_grad_norm; DESIGN.md section 3.18 states the chains, every operation one fp32 rounding).  type: "sgd" | "nesterov" | "adam".  momentum is adam's beta1, momentum2 its
    beta2, delta its epsilon; decoupled_wd (adam only) applies the decay to the param (AdamW) instead of adding it to the gradient.  clip_gradients > 0: every gradient is
    scaled by coef = norm > clip ? clip / norm : 1, norm the l2 norm over ALL updated params' gradients; <param>_grad_loss keeps the unclipped gradient.  lr_policy: an
    LrPolicy; the driver then uploads lr = lr_policy.lr_at(lr, iter) before every step.  lr_mult / decay_mult / tensors_per_call: as SgdSolver's."""
    type: str
    lr: float
    momentum: float = 0.9
    momentum2: float = 0.999
    delta: float = 1e-8
    weight_decay: float = 5e-4
    decoupled_wd: bool = False
    clip_gradients: float = 0.0
    lr_policy: Optional[LrPolicy] = None
    lr_mult: Optional[Dict[str, float]] = None
    decay_mult: Optional[Dict[str, float]] = None
    tensors_per_call: int = 32

    mult_of = SgdSolver.mult_of

    @staticmethod
    def corr(momentum: float, momentum2: float, t: int) -> float:
        """adam's bias correction sqrt(1 - momentum2^t) / (1 - momentum^t) in float64 from the fp32 values of the two momenta (a momentum of 0: the factor is 1)."""
        m1, m2 = float(np.float32(momentum)), float(np.float32(momentum2))
        return float(np.sqrt(1.0 - m2 ** t) / (1.0 - m1 ** t))

    def hyper(self, it: int = 0) -> np.ndarray:
        """The eight floats of solver_hyper for step `it`."""
        lr = self.lr_policy.lr_at(self.lr, it) if self.lr_policy is not None else self.lr
        return np.array([lr, self.momentum, self.weight_decay, self.momentum2, self.delta, self.corr(self.momentum, self.momentum2, it + 1) if self.type == "adam" else 1.0,
                         self.clip_gradients, 0.0], np.float32)


@dataclass
class Freeze:
    """Fine-tuning for ConvPipeBck(freeze=...): which params stay fixed, which BatchNorms run on their running pair, and the pruned backward walk.
    params: param names (`res2a_branch2a_filts`), op tags (`conv1`: all of that op's params) or a suffix (`filts` | `biases` | `scale` | `bias`, as lr_mult keys are
    written); a name that matches nothing is an RtErr that names it.  A frozen param has no history, second history or accumulator var, takes no part in the clipping norm
    and is in no update call: its bits never change.
    bn_global_stats: True (every BatchNorm), False, or a list of BatchNorm op tags.  A listed [BatchNorm, Scale (, ReLU)] run normalises by its running pair, which is then
    only read (hip_bnf_prep in place of hip_bn_stats; backward hip_bnf_bck / hip_bnf_bck_in, dx = (scale * inv_std) * dy).
    keep_grads: node names whose gradient is wanted although nothing trainable lies below them, e.g. ("data",) for a saliency map.
    THE PRUNING RULE is Caffe's need_backward, applied by init to the pipe add_bck_ops returned.  Walking the forward ops in order, a node needs a gradient if its producer
    has a trainable param, or if any of the producer's inputs needs one, or if it is in keep_grads; the input node and `label` never need one unless listed.  A gradient op
    keeps a param-gradient output only if that param is trainable -- an op whose two params are not both frozen keeps both -- and its in_grad_loss output only if that
    bottom node needs a gradient; a gradient op with no output left emits no call, and the vars of dropped gradients are not created.  (A training BatchNorm's data
    gradient reads the two sums: where it is kept, they are computed even for a frozen Scale.)
    Freeze() with nothing in it therefore drops only what feeds <input>_grad_loss: the data gradient of every layer below the first that reads a trainable layer's output
    -- in a plain net the first convolution's hip_bconv_in."""
    params: Sequence[str] = ()
    bn_global_stats: object = False
    keep_grads: Sequence[str] = ()


PARAM_SFXS = ("filts", "biases", "scale", "bias")   # what an lr_mult / Freeze.params key may name besides a param or an op tag
WHY_DROPPED = ("Freeze's pruning rule computes a node's gradient only if the node's producer has a trainable param, or an input of the producer needs a gradient, or the "
               "node is in Freeze.keep_grads; a param's gradient only if the param (or the other param of its op) is trainable")


@dataclass
class GradOp:
    """One op of the pipe with gradient ops: the reference's conv_op_t reduced to tag / type / bots / tops.  `src` is the forward PipeOp whose parameters it carries."""
    tag: str
    type: str
    bots: List[str]
    tops: List[str]
    src: Optional[PipeOp] = None

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
    if o.type == "Convolution":
        return GradOp(o.tag, o.type, [o.bot, o.tag + "_filts", o.tag + "_biases"], [o.top], o)
    if o.type in ("Concat", "Eltwise"):
        return GradOp(o.tag, o.type, list(o.bots), [o.top], o)
    if o.type == "BatchNorm":   # in place; the running statistics are params it reads AND rewrites
        return GradOp(o.tag, o.type, [o.bot, o.tag + "_mean", o.tag + "_var"], [o.top], o)
    if o.type == "Scale":
        return GradOp(o.tag, o.type, [o.bot, o.tag + "_scale", o.tag + "_bias"], [o.top], o)
    return GradOp(o.tag, o.type, [o.bot], [o.top], o)


def add_bck_ops(cp: ConvPipe, label_node: str = "label", loss_tops: Optional[Sequence[str]] = None) -> BckPipe:
    """The pipe of `cp` with gradient ops.  `loss_tops`: the forward nodes to cap with a SoftmaxWithLoss (default: the pipe's out node; GoogLeNet's auxiliary heads are
    named here).  One cap is tagged `loss` and writes the node `loss`; several are tagged loss1, loss2, ... in the order given.  All of them read `label_node`."""
    loss_tops = list(loss_tops) if loss_tops else [cp.out_node()]
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
        fwd.append(GradOp(tag, "SoftmaxWithLoss", [t, label_node], [t + "_grad_loss", tag]))
        nodes[t + "_grad_loss"] = cp.nodes[t]
        nodes[tag] = Dims.make("float", y=1, x=1)
        nodes[label_node] = Dims.make("float", img=cp.nodes[t].dsz("img"), y=1, x=1)
        loss_nodes.append(tag)

    # the graph as the reference holds it: in-place ops hang off their node and are in nobody's bot_for / top_for (src/conv_util.cc:273-292)
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

    def bck_of(cop: GradOp) -> Optional[GradOp]:
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
            b = bck_of(ip)
            if b:
                walk.append(b)
        if len(n.bot_for) > 1:
            walk.append(GradOp("reduce_" + nn + "_grad_loss", "Reduce", [grad_loss_onn(by_tag[r], nn) for r in n.bot_for], [nn + "_grad_loss"]))
        for r in n.bot_for:
            cop = by_tag[r]
            seen[r] = seen.get(r, 0) + 1
            if seen[r] != len(cop.bots):   # wait until all its bottoms were seen
                continue
            b = bck_of(cop)
            if b:
                walk.append(b)
            for t in cop.tops:
                rec(t)

    for src in sorted(nn for nn, n in g.items() if not n.top_for):   # the reference's `bots`, a sorted set of names
        rec(src)

    # appended in reverse; a Reduce is kept only if nobody wrote its output yet and its first input exists (src/conv_util.cc:866-877): `label` has none
    out = list(fwd)
    for b in reversed(walk):
        if b.type == "Reduce" and not (b.tops[0] not in nodes and b.bots[0] in nodes):
            continue
        for i in b.bots:
            if i not in nodes:
                raise RtErr(f"add_bck_ops: gradient op {b.tag} reads {i!r}, which no earlier op writes")
        if b.type == "BckConv":
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
        elif b.type in ("Spreading", "BckLRN"):
            nodes[b.tops[0]] = nodes[b.src.bot]
        elif b.type == "Reduce":
            if not 2 <= len(b.bots) <= 8:
                raise UnsupErr(f"add_bck_ops: {b.tag} sums {len(b.bots)} partial gradients; hip_reduce takes 2 to 8")
            nodes[b.tops[0]] = nodes[b.bots[0]]
        else:                 # ZeroIfNonPos, BckDropout: in place on the gradient
            nodes[b.tops[0]] = nodes[b.bots[0]]
        out.append(b)
    return BckPipe(cp, out, nodes, label_node, len(fwd), loss_nodes)


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
        if t == "Convolution":
            v["out"] = nd(o.tops[0])
        else:
            v.update({"out_grad_loss": nd(o.bots[3]), "in_grad_loss": Nda(bp.nodes[o.bots[0]]), "filts_grad_loss": nd(o.tops[1]), "biases_grad_loss": nd(o.tops[2])})
        return Op({"type": t}, v)
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


# ------------------------------------------------------------------------------------------------
# driver
# ------------------------------------------------------------------------------------------------
@dataclass
class BckCall:
    tag: str
    fop: Op                      # the annotated function op
    args: Dict[str, str]         # arg name -> var name (var args only; REF / by-value args follow from the function op)
    rfc: RtcFuncCall
    call_id: int = -1


def bn_stat_params(cp: ConvPipe) -> List[str]:
    """The running-statistics params of the pipe's BatchNorm ops (<tag>_mean, <tag>_var): rewritten by the forward pass, without a gradient, never updated by a solver."""
    return [o.tag + sfx for o in cp.ops if o.type == "BatchNorm" for sfx in BN_STAT_SFXS]


def host_params(bp: BckPipe, seed: int = 0) -> Dict[str, np.ndarray]:
    """Deterministic host-made params for a pipe without trained weights: filts ~ N(0, 2 / fan_in) (so activations neither die nor blow up through the ReLUs), biases
    ~ U(-0.1, 0.1), a BatchNorm's _mean 0 and _var 1, a Scale's _scale ~ U(0.9, 1.1) and _bias ~ U(-0.05, 0.05), each seeded by its name.  (ConvPipeFwd's device generator is generated CUCL source, which be=cpu cannot run.)"""
    out = {}
    stats = bn_stat_params(bp.cp)
    scales = {o.tag + "_scale" for o in bp.cp.ops if o.type == "Scale"}; sbias = {o.tag + "_bias" for o in bp.cp.ops if o.type == "Scale"}
    for n, d in bp.cp.params.items():
        rng = np.random.default_rng([zlib.crc32(n.encode()), seed])
        if n.endswith("_filts"):
            fan_in = d.dsz("in_chan") * d.dsz("y") * d.dsz("x")
            out[n] = (rng.standard_normal(d.sizes) * np.sqrt(2.0 / fan_in)).astype(np.float32)
        elif n in stats:         # a BatchNorm's running pair starts at (0, 1)
            out[n] = (np.zeros if n.endswith("_mean") else np.ones)(d.sizes, np.float32)
        elif n in scales:
            out[n] = rng.uniform(0.9, 1.1, d.sizes).astype(np.float32)
        elif n in sbias:
            out[n] = rng.uniform(-0.05, 0.05, d.sizes).astype(np.float32)
        else:
            out[n] = rng.uniform(-0.1, 0.1, d.sizes).astype(np.float32)
    return out


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
        elif prev.tops[0] != gl:
            why[o.tag] = f"the op before it, {prev.tag}, writes {prev.tops[0]}, not {gl}"
        elif prev.bots[RELU_GRAD_PRODUCERS[prev.type]] != x:
            why[o.tag] = f"the op before it, {prev.tag}, has the forward input {prev.bots[RELU_GRAD_PRODUCERS[prev.type]]}, not {x}"
        else:
            folds[o.tag] = prev.tag
    return folds, why


class ConvPipeBck:
    """The training-form step of a pipe with gradient ops over one backend (be=hip or be=cpu): forward, loss and every gradient, one call per native function.
    fuse_relu_grad=True (opt-in): every ReLU gradient that plan_relu_grad_folds allows emits no call; the BckConv data gradient / Spreading / BckLRN before it runs with
    zero_if_in_non_pos=1 and writes the masked gradient itself.  Every node holds the same values after a step either way.  `fused_relu_grads` says what init did:
    {"folded": [ZeroIfNonPos tags], "unfolded": {ZeroIfNonPos tag: reason}}.
    seed_in_var=True (opt-in): the dropout seed lives in the one-word uint32 var `det_drop_seed`.  Every dropout call runs with seed_from_var=1, reads that var and
    carries only its layer's fixed offset by value; set_det_drop_seed uploads four bytes and touches no call.  Every node holds the same bits as under the default driver
    given the same seed.  This is what lets a step with dropout be captured: capture_graph / run_graph / run_bck(graph=True) replay the whole call list as one
    hipGraph (be=hip, one device), serially or -- parallel=True -- with the calls' true dependencies (_call_deps), and leave the same bits in every var as the eager
    step.
    On a multi-device backend (`(be=hip,devices=0:1:...)`, vars sharded on img) init flags the five functions that are not independent per image with img_shards=1
    (cnn_op.on_img_shards); run_bck, set_det_drop_seed, seed_in_var, fuse_relu_grad and calls() work as on one device.  Every img-leading node and every loss then
    hold the bits of the one-device step, every filter / bias gradient the per-shard gradients added in device order.
    solver=SgdSolver(...) (opt-in; None leaves the vars, calls(), _call_deps() and every bit of a step as they are): the step also UPDATES the params on the device.
    init creates one zero-filled history var <param>_sgd_hist per param and the var sgd_hyper, and appends the hip_sgd_update calls, tagged sgd_update_0 ..., at the
    END of the call list, behind every gradient op: tensors_per_call params per call in the order of the pipe's params, g_i bound to <param>_grad_loss.
    set_sgd_hyper uploads 16 bytes and touches no call (valid between graph replays: a learning-rate schedule needs no new capture); zero_sgd_history clears the
    history.  capture_graph captures the update calls with the rest and leaves params and history as they were.  On a multi-device backend the update runs on every
    device's replicas, which hold the same summed gradients and so stay equal.
    solver=Solver(...) (an SgdSolver goes down the path above untouched): SGD, Nesterov or Adam with optional global-norm clipping and a
    learning-rate policy.  init creates solver_hyper (float v=8), solver_state (float v=4), <param>_sgd_hist, for adam <param>_sgd_hist2 and, when clipping,
    solver_gnorm_partials, and appends behind every gradient op: when clipping the hip_grad_sumsq calls (grad_sumsq_k) and one grad_norm, then the hip_solver_update calls
    (solver_update_k); n_sgd_calls counts all of them.  `iter` starts at 0; before every step that runs those calls -- eager or a replay -- the 32 bytes of solver_hyper are
    uploaded for step `iter` (lr from the policy, adam's bias correction for t = iter + 1), and `iter` advances behind it.  <param>_grad_loss keeps the unclipped gradient.
    iter_size=n > 1 (1, the default, leaves the calls, the vars and every bit as they are; needs a Solver): Caffe's gradient accumulation.  A
    step is a MICRO-step: its gradients are added into <param>_grad_acc (hip_grad_accum; the first micro-step of n overwrites, so nothing is ever cleared), and only the
    n-th applies the update (hip_solver_update_acc) on 1 / n times the sum -- clipped, when clipping, by the norm of the SUM.  init creates <param>_grad_acc per updated
    param and solver_accum (float v=4), and appends behind the gradient ops: the grad_accum_k calls, when clipping the grad_sumsq_k calls bound to the accumulators and
    grad_norm, then the solver_update_k calls; n_sgd_calls counts all of them.  All of them run on every micro-step; before each the 16 bytes [micro == 0, micro == n - 1,
    fp32(1 / n), micro] are uploaded into solver_accum, which the launches read from device memory: one captured graph serves every micro-step.  `micro` advances modulo
    n, `iter` only behind the applying micro-step (a learning-rate policy and adam's bias correction count updates).  <param>_grad_loss, the loss and a BatchNorm's
    statistics are the micro-batch's; the running pair moves on every pass.
    fuse_filts_biases=True (opt-in; False leaves the calls, their names and every bit as they are): every BckConv emits hip_bconv_in followed by ONE
    hip_bconv_filts_biases in place of the hip_bconv_biases + hip_bconv_filts pair.  Every other node holds the same bits; the filter and
    bias gradients follow that function's written chains (on be=cpu: the single chains, the same bits as the pair).  Not on a multi-device backend: init raises UnsupErr.
    grad_operands="bf16" (opt-in; "" leaves everything as it is): every BckConv emits hip_bconv_in and hip_bconv_filts_biases with hip_operands=bf16
    (cnn_op.bf16_operands) -- the option therefore IMPLIES fuse_filts_biases=True.  Tensors stay fp32; the operands of the two convolution
    gradients are rounded to bf16 on the way into the matrix pipe and summed in fp32; the bias gradients, the forward pass, the loss and every non-conv gradient are
    untouched.  The two conv gradients are then held to a bound, not to bits, and are the same bits run to run and from graph replay to eager.  Composes with
    fuse_relu_grad, seed_in_var, solver= and capture_graph.  Any other string is an RtErr; on a multi-device backend init raises UnsupErr before creating anything.
    BatchNorm / Scale: exactly the run [BatchNorm, Scale] plus an optional in-place ReLU behind it, on a node X a Convolution produces, is
    supported -- all ResNet-50 has.  It runs as a TRAINING BatchNorm: the convolution (conv_has_relu=0) writes the side var <X>_bn_in; hip_bn_stats reads it and writes
    <bn-tag>_batch_mean / _batch_inv_std and moves the running pair <bn-tag>_mean / _var by bn_maf; hip_bn_fwd writes X, ReLU included.  Backward, BckScale is
    hip_bn_bck_sums (-> <scale-tag>_scale_grad_loss / _bias_grad_loss) and BckBatchNorm hip_bn_bck_in, in place on X_grad_loss, both recomputing the normalised value
    from <X>_bn_in.  An Eltwise runs as hip_reduce, its gradient as one hip_fan_out.  A solver leaves <bn-tag>_mean / _var alone.  Not on a multi-device backend: init refuses a pipe with a BatchNorm or an Eltwise there before creating anything
    -- unless img_chunks is set.
    img_chunks=n >= 1 (opt-in; 0 leaves everything as it is, both refusals included): every [BatchNorm, Scale (, ReLU)] run uses the four hip_bnc_*
    functions with chunks=n -- the per-channel sums in the chunked chain, the batch cut into n img chunks as a multi-device backend cuts it -- and every BckEltwise runs
    as one hip_split call per output (icix=0, out of in's dims: a bit-for-bit copy by a function that runs on img shards).  Var names, side vars, call tags and order
    are unchanged.  On one device and on be=cpu any n is allowed, and n=1 leaves today's bits in every node; on `(be=hip,devices=...)` n must be the device count (RtErr
    before anything is created) and the pipe then runs there: every node but the convolutions' filter / bias gradients (summed per shard, section 3.13) holds the bits of
    the one-device step with the same n.  fuse_relu_grad, seed_in_var, solver= and, on one device, capture_graph work as before; fuse_filts_biases and grad_operands
    stay refused on a multi-device backend.
    input_transform=InputTransform(...) (opt-in; None leaves the vars, calls() and every bit as they are): the step takes its input as uint8
    images and crops, mirrors, subtracts the mean and scales on the device.  init creates data_raw (uint8, the batch at the source size in the transform's layout),
    data_xf_plan (uint32 img:v=4) and data_xf_mean (uploaded once; set_input_mean uploads it again) and puts ONE call in front of the step's first, tagged data_xf:
    hip_data_transform from data_raw into the pipe's input node.  run_bck(["data_raw", "label"], ...) uploads bytes.  Before every pass -- a micro-step of iter_size
    included, eager or a replay -- the B x 16 bytes of the plan are uploaded: input_transform.plan("train", xf_images, B), or the plan set_input_plan gave for this one
    pass, checked by check_plan; behind the pass xf_images advances by B.  The plan lives in a var, so one captured graph serves every pass.  Feeding the input node
    itself is an RtErr: the call would overwrite it.  On a multi-device backend the call runs on the img shards of data_raw, data_xf_plan and the input node.
    freeze=Freeze(...) (opt-in; None leaves the vars, calls(), _call_deps() and every bit of a step as they are): fine-tuning.  The params it names
    stay fixed (not in sgd_params, no solver var, in no update or norm call), the BatchNorms it lists run on their running pair, which is then only read, and the backward
    walk is pruned by Caffe's need_backward rule (Freeze's docstring): a gradient op emits only the calls whose outputs are still wanted, the vars of dropped gradients
    are not created and asking run_bck for one is an RtErr.  `frozen` says what init did: {"params": the frozen params, "dropped_calls": the tags of the gradient ops
    that emit no call, "bn_global": the BatchNorm tags on their running pair}.  A listed [BatchNorm, Scale (, ReLU)] run emits hip_bnf_prep (-> <bn-tag>_batch_mean /
    _batch_inv_std from the running pair) and hip_bn_fwd as it is; backward ONE call: hip_bnf_bck (BckScale: both sums and dx = (scale * inv_std) * dy in one pass, in
    place on X_grad_loss), hip_bn_bck_sums where nothing below needs a gradient, or hip_bnf_bck_in (BckBatchNorm) where both Scale params are frozen.  The one output
    Freeze leaves of an Eltwise gradient is a hip_split copy.  Composes with every option above; on a multi-device backend param freezing alone works, bn_global_stats is
    refused there and together with img_chunks before anything is created.  A pipe in which nothing is trainable is an RtErr.  A Freeze cannot be changed after init."""

    def __init__(self, rtc, op_tune: Optional[OpTune] = None, fuse_relu_grad: bool = False, seed_in_var: bool = False, solver: Optional[object] = None, bn_maf: float = 0.999, fuse_filts_biases: bool = False,
                 grad_operands: str = "", img_chunks: int = 0, iter_size: int = 1, input_transform: Optional[InputTransform] = None, freeze: Optional[Freeze] = None):
        self.rtc = rtc
        if freeze is not None and not isinstance(freeze, Freeze):
            raise RtErr(f"ConvPipeBck: freeze must be a bck_pipe.Freeze or None, got {type(freeze).__name__}")
        self.freeze = freeze
        self.frozen: Dict[str, object] = {"params": [], "dropped_calls": [], "bn_global": []}   # what init did with `freeze`
        self._dropped_vars: set = set()   # the gradient vars the pruning rule left out
        if input_transform is not None and not isinstance(input_transform, InputTransform):
            raise RtErr(f"ConvPipeBck: input_transform must be an input_pipe.InputTransform or None, got {type(input_transform).__name__}")
        self.input_transform = input_transform
        self.xf_images = 0           # the global index of the next pass's first image: what the train plan is made for
        self._input_plan: Optional[np.ndarray] = None   # set_input_plan's, for one pass
        if not isinstance(iter_size, int) or isinstance(iter_size, bool) or iter_size < 1:
            raise RtErr(f"ConvPipeBck: iter_size must be an int >= 1, got {iter_size!r}")
        if iter_size > 1 and not isinstance(solver, Solver):
            raise RtErr(f"ConvPipeBck: iter_size={iter_size} accumulates gradients for a Solver's update; build the driver with solver=Solver(type=\"sgd\", ...) "
                        f"(got {'no solver' if solver is None else type(solver).__name__})")
        self.iter_size = iter_size   # > 1: a step is a micro-step; the update applies on every iter_size-th
        self.micro = 0               # the next micro-step's index in 0 .. iter_size - 1
        if not isinstance(img_chunks, int) or isinstance(img_chunks, bool) or not 0 <= img_chunks <= BNC_MAX_CHUNKS:
            raise RtErr(f"ConvPipeBck: img_chunks must be an int, 0 (off) or 1 to {BNC_MAX_CHUNKS}, got {img_chunks!r}")
        self.img_chunks = img_chunks   # > 0: the training BatchNorm's sums in the chunked chain over this many img chunks, an Eltwise gradient as hip_split copies
        if grad_operands not in ("", "bf16"):
            raise RtErr(f"ConvPipeBck: grad_operands must be '' | 'bf16', got {grad_operands!r}")
        self.grad_operands = grad_operands
        self.fuse_filts_biases = bool(fuse_filts_biases) or self.grad_operands == "bf16"   # (the filter and bias gradients have their bf16 form as the fused call only)
        self.solver = solver
        self.bn_maf = float(bn_maf)   # a training BatchNorm's moving-average fraction: run' = maf * run + (1 - maf) * batch
        self.sgd_params: List[str] = []   # the params the solver updates: all of them but the BatchNorm running statistics
        self.n_sgd_calls = 0       # the solver's calls (a Solver's clipping calls included), the last n_sgd_calls of bck_calls
        self.iter = 0              # a Solver's step count: what its lr_policy and adam's bias correction are evaluated at
        self._base_lr = float(solver.lr) if solver is not None else 0.0
        self.op_tune = op_tune or OpTune()
        self.fuse_relu_grad = bool(fuse_relu_grad)
        self.seed_in_var = bool(seed_in_var)
        self._graph: Optional[int] = None
        self._stepped = False      # an ordinary step has run since init: every workspace and lazily built kernel exists
        self.call_deps: List[List[int]] = []
        self.fused_relu_grads: Dict[str, object] = {"folded": [], "unfolded": {}}
        self.bck_calls: List[BckCall] = []
        self.vars: List[str] = []
        self.funcs: List[str] = []
        self.per_call_ms: List[Tuple[str, str, float]] = []
        self.compute_dur_ms = 0.0

    def _var(self, vn: str, dims: Dims) -> None:
        if vn not in self.vars:
            self.rtc.create_var_with_dims(vn, dims); self.vars.append(vn)

    def init(self, bp: BckPipe, op_params: Optional[Dict[str, np.ndarray]] = None, gen_mode: int = 5) -> None:
        """Create every var, annotate every op, compile, upload the params once.  Without op_params the params are host_params(bp, gen_mode)."""
        if not isinstance(bp, BckPipe):
            raise RtErr("ConvPipeBck.init: pass the pipe add_bck_ops returned")
        self.bp = bp
        rtc, tune = self.rtc, self.op_tune
        self._stepped = False
        if self.seed_in_var and SEED_VAR in bp.nodes:
            raise RtErr(f"ConvPipeBck.init: seed_in_var=True needs the var name {SEED_VAR!r}, which is a node of the pipe")
        multi_dev = isinstance(getattr(rtc, "devices", None), list) and len(rtc.devices) > 1
        if self.grad_operands and multi_dev:
            raise UnsupErr("ConvPipeBck.init: grad_operands='bf16': the filter and bias gradients have their bf16-operand form as hip_bconv_filts_biases only, which sums over "
                           "the images into two outputs and is not provided on a multi-device backend (devices=...); leave the option off there")
        if self.fuse_filts_biases and multi_dev:
            raise UnsupErr("ConvPipeBck.init: fuse_filts_biases=True: hip_bconv_filts_biases sums over the images into two outputs and is not provided on a multi-device "
                           "backend (devices=...); leave the option off there")
        if self.img_chunks and multi_dev and self.img_chunks != len(rtc.devices):
            raise RtErr(f"ConvPipeBck.init: img_chunks={self.img_chunks} on {len(rtc.devices)} devices: chunk i of a BatchNorm's sums is device i's img shard, so img_chunks must "
                        "be the device count")
        bn_runs = self._plan_bn_runs(bp)   # node X -> (BatchNorm op, Scale op, the ReLU behind them or None); every other shape of BatchNorm / Scale is refused here
        if bn_runs and multi_dev and not self.img_chunks:
            raise UnsupErr("ConvPipeBck.init: the pipe has a BatchNorm, whose batch statistics sum over the images of the WHOLE batch: not provided on a multi-device backend "
                           "(devices=...); statistics summed across img shards are out of scope")
        if multi_dev and not self.img_chunks and any(o.type == "BckEltwise" for o in bp.bck_ops()):
            raise UnsupErr("ConvPipeBck.init: the pipe has an Eltwise, whose gradient (hip_fan_out) takes vars of exactly its op's dims, not img shards: not provided on a "
                           "multi-device backend (devices=...)")
        stats = set(bn_stat_params(bp.cp))
        self.sgd_params = [pn for pn in bp.cp.params if pn not in stats]
        keep, bn_global = self._plan_freeze(bp, bn_runs, multi_dev)   # (None, empty without freeze=; refuses before anything is created)
        if self.solver is not None:   # (refused before anything is created)
            if not 1 <= int(self.solver.tensors_per_call) <= SGD_MAX_TENS:
                raise RtErr(f"ConvPipeBck.init: SgdSolver.tensors_per_call={self.solver.tensors_per_call}: 1 to {SGD_MAX_TENS}")
            gen = isinstance(self.solver, Solver)
            if not gen and not isinstance(self.solver, SgdSolver):
                raise RtErr(f"ConvPipeBck.init: solver must be an SgdSolver or a Solver, got {type(self.solver).__name__}")
            if gen:
                sv = self.solver
                if sv.type not in ("sgd", "nesterov", "adam"):
                    raise RtErr(f"ConvPipeBck.init: Solver.type must be sgd | nesterov | adam, got {sv.type!r}")
                if sv.decoupled_wd and sv.type != "adam":
                    raise RtErr(f"ConvPipeBck.init: Solver.decoupled_wd is adam's, not {sv.type}'s")
                if not float(sv.clip_gradients) >= 0.0:
                    raise RtErr(f"ConvPipeBck.init: Solver.clip_gradients={sv.clip_gradients!r}: 0 (off) or a positive norm")
                if sv.lr_policy is not None and not isinstance(sv.lr_policy, LrPolicy):
                    raise RtErr("ConvPipeBck.init: Solver.lr_policy must be an LrPolicy or None")
            names = [SGD_HYPER_VAR] if not gen else [SOLVER_HYPER_VAR, SOLVER_STATE_VAR] + ([SOLVER_PARTS_VAR] if self.solver.clip_gradients > 0 else []) + \
                ([pn + SGD_HIST2_SFX for pn in self.sgd_params] if self.solver.type == "adam" else [])
            if self.iter_size > 1:
                names += [SOLVER_ACCUM_VAR] + [pn + GRAD_ACC_SFX for pn in self.sgd_params]
            for vn in [pn + SGD_HIST_SFX for pn in self.sgd_params] + names:
                if vn in bp.nodes:
                    raise RtErr(f"ConvPipeBck.init: the solver needs the var name {vn!r}, which is a node of the pipe")
            for pn in self.sgd_params:
                if pn + "_grad_loss" not in bp.nodes:
                    raise RtErr(f"ConvPipeBck.init: the solver: no gradient op writes {pn + '_grad_loss'!r}")
        for x, (bn, sc, _) in bn_runs.items():
            for vn in (x + BN_IN_SFX, bn.tag + BN_MEAN_SFX, bn.tag + BN_ISTD_SFX):
                if vn in bp.nodes:
                    raise RtErr(f"ConvPipeBck.init: the BatchNorm on {x} needs the var name {vn!r}, which is a node of the pipe")
        xf = self.input_transform
        if xf is not None:   # (refused before anything is created)
            dn = bp.cp.in_node; dd = bp.nodes[dn]
            if dd.tn != "float" or dd.names != ("img", "chan", "y", "x") or (dd.dsz("y"), dd.dsz("x")) != (xf.ch, xf.cw):
                raise RtErr(f"ConvPipeBck.init: input_transform crops to {xf.ch} x {xf.cw}: the pipe's input node {dn!r} must be float img:chan:y={xf.ch}:x={xf.cw}, got {dd.tn} {dd.pretty()}")
            for vn in (DATA_RAW_VAR, DATA_XF_PLAN_VAR, DATA_XF_MEAN_VAR):
                if vn in bp.nodes:
                    raise RtErr(f"ConvPipeBck.init: input_transform needs the var name {vn!r}, which is a node of the pipe")
            xf_mean = xf.mean_array(dd.dsz("chan"))
        for n, d in bp.nodes.items():
            if n not in self._dropped_vars:
                self._var(n, d)
        if xf is not None:
            self._var(DATA_RAW_VAR, xf.src_dims(dd.dsz("img"), dd.dsz("chan")))
            self._var(DATA_XF_PLAN_VAR, Dims(("img", "v"), (dd.dsz("img"), 4), "uint32_t"))
            self._var(DATA_XF_MEAN_VAR, xf.mean_dims(dd.dsz("chan")))
        for x, (bn, sc, _) in bn_runs.items():
            self._var(x + BN_IN_SFX, bp.nodes[x])
            for sfx in (BN_MEAN_SFX, BN_ISTD_SFX):
                self._var(bn.tag + sfx, bp.cp.params[bn.tag + "_mean"])
        if self.seed_in_var:
            self._var(SEED_VAR, Dims(("v",), (1,), "uint32_t"))
        fused = set()   # ReLUs taken into their convolution (src/rtc_fwd.cc:486-493): no forward call, their ZeroIfNonPos still runs
        relu_of: Dict[str, bool] = {}
        ops = bp.ops
        for i, o in enumerate(ops[:bp.n_fwd]):
            if o.type == "Convolution":
                first_ip = next((q for q in ops[i + 1:bp.n_fwd] if q.in_place and q.bots[0] == o.tops[0]), None)
                relu_of[o.tag] = bool(first_ip and first_ip.type == "ReLU")
                if relu_of[o.tag]:
                    fused.add(first_ip.tag)
        for x, (bn, sc, relu) in bn_runs.items():   # the ReLU behind a [BatchNorm, Scale] run is hip_bn_fwd's
            if relu is not None:
                fused.add(relu.tag)
        bn_of_tag = {q.tag: (x, run) for x, run in bn_runs.items() for q in run[:2]}
        by_tag_bck = {o.tag: o for o in bp.bck_ops()}
        folds, why = plan_relu_grad_folds(bp) if self.fuse_relu_grad else ({}, {o.tag: "fuse_relu_grad is off" for o in bp.bck_ops() if o.type == "ZeroIfNonPos"})
        self.fused_relu_grads = {"folded": list(folds), "unfolded": why}
        takes_relu = set(folds.values())   # the gradient ops that apply the mask of the ZeroIfNonPos behind them
        zinp = lambda o, f: fuse_zero_if_in_non_pos(f) if o.tag in takes_relu else f
        infos: List[RtcFuncInfo] = []

        def emit(tag: str, fop: Op, args: Dict[str, str]) -> None:
            if multi_dev and fop.get_func_name() in IMG_SHARDS_FUNCS:   # (the only way these five run on img shards)
                fop = on_img_shards(fop)
            fname = f"bck_{len(self.bck_calls)}_{fop.get_func_name()}"
            spec = pipe_func_args(fop)
            am: Dict[str, RtcArg] = {}
            for an, io in spec:
                if io == "REF":
                    am[an] = RtcArg.ref(fop.get_dims(an))
                elif io == "VAL":
                    am[an] = RtcArg.scalar(0, "uint32_t")
                else:
                    am[an] = RtcArg.var(args[an])
            infos.append(RtcFuncInfo(fname, "", [an for an, _ in spec], fop))
            self.bck_calls.append(BckCall(tag, fop, dict(args), RtcFuncCall(fname, am)))
            self.funcs.append(fname)

        if xf is not None:   # in front of the step's first call: the input node from the bytes
            emit(DATA_XF_TAG, data_transform_func_op(xf.src_dims(dd.dsz("img"), dd.dsz("chan")), (xf.ch, xf.cw), xf.mean_dims(dd.dsz("chan")), xf.scale),
                 {"src": DATA_RAW_VAR, "plan": DATA_XF_PLAN_VAR, "mean": DATA_XF_MEAN_VAR, "out": dn})
        kept = lambda o, i: keep is None or o.tag not in keep or keep[o.tag][i]   # does gradient op o still write its i-th top?
        for o in ops:
            if o.tag in fused or o.tag in folds:
                continue
            if keep is not None and o.tag in keep and not any(keep[o.tag]):
                continue
            t = o.type
            calls: List[Tuple[Op, Dict[str, str]]] = []
            if t in ("BatchNorm", "Scale", "BckScale", "BckBatchNorm"):
                # a [BatchNorm, Scale (, ReLU)] run on X: statistics at the BatchNorm, normalise + scale + bias + ReLU at the Scale; backward the two sums at BckScale and
                # the data gradient at BckBatchNorm, in place on X_grad_loss.  The normalised value is recomputed from <X>_bn_in everywhere: nothing is saved twice
                x, (bn, sc, relu) = bn_of_tag[o.src.tag]
                xd = bp.nodes[x]
                common = {"in": x + BN_IN_SFX, "mean": bn.tag + BN_MEAN_SFX, "inv_std": bn.tag + BN_ISTD_SFX}
                nc = self.img_chunks
                stats_op = (lambda d, eps, maf: bnc_stats_func_op(d, eps, maf, nc)) if nc else bn_stats_func_op
                fwd_op = bnc_fwd_func_op if nc else bn_fwd_func_op
                sums_op = (lambda d: bnc_bck_sums_func_op(d, nc)) if nc else bn_bck_sums_func_op
                in_op = bnc_bck_in_func_op if nc else bn_bck_in_func_op
                if bn.tag in bn_global:   # on the running pair: hip_bnf_prep, hip_bn_fwd as it is, and ONE backward call -- which one, the pruning rule says
                    in_need, sc_train = kept(o, 0), kept(o, 1) if t == "BckScale" else kept(by_tag_bck[sc.tag + "_bck"], 1)
                    gl = {"out_grad_loss": o.bots[0], "in_grad_loss": o.tops[0]}
                    if t == "BatchNorm":
                        calls.append((bnf_prep_func_op(xd, bn.eps), {"run_mean": bn.tag + "_mean", "run_var": bn.tag + "_var", "mean": common["mean"], "inv_std": common["inv_std"]}))
                    elif t == "Scale":
                        calls.append((fwd_op(xd, 1 if relu is not None else 0), dict(common, scale=sc.tag + "_scale", bias=sc.tag + "_bias", out=x)))
                    elif t == "BckScale" and sc_train and in_need:      # the sums and dx in one pass, in place on X_grad_loss
                        calls.append((bnf_bck_func_op(xd), dict(common, scale=sc.tag + "_scale", scale_grad_loss=o.tops[1], bias_grad_loss=o.tops[2], **gl)))
                    elif t == "BckScale" and sc_train:     # nothing below needs a gradient: the sums alone
                        calls.append((sums_op(xd), dict(common, out_grad_loss=o.bots[0], scale_grad_loss=o.tops[1], bias_grad_loss=o.tops[2])))
                    elif t == "BckBatchNorm" and not sc_train:   # behind a frozen Scale (with a trainable one hip_bnf_bck has written dx already)
                        calls.append((bnf_bck_in_func_op(xd), dict(inv_std=common["inv_std"], scale=sc.tag + "_scale", **gl)))
                elif t == "BatchNorm":
                    calls.append((stats_op(xd, bn.eps, self.bn_maf), dict(common, run_mean=bn.tag + "_mean", run_var=bn.tag + "_var")))
                elif t == "Scale":
                    calls.append((fwd_op(xd, 1 if relu is not None else 0), dict(common, scale=sc.tag + "_scale", bias=sc.tag + "_bias", out=x)))
                elif t == "BckScale":
                    calls.append((sums_op(xd), dict(common, out_grad_loss=o.bots[0], scale_grad_loss=o.tops[1], bias_grad_loss=o.tops[2])))
                elif kept(o, 0):
                    calls.append((in_op(xd), dict(common, scale=sc.tag + "_scale", scale_grad_loss=sc.tag + "_scale_grad_loss", bias_grad_loss=sc.tag + "_bias_grad_loss",
                                                              out_grad_loss=o.bots[0], in_grad_loss=o.tops[0])))
                for fop, args in calls:
                    emit(o.tag, fop, args)
                continue
            n_kept = sum(1 for i in range(len(o.tops)) if kept(o, i))
            if t == "BckEltwise" and (self.img_chunks or n_kept == 1):   # one copy per output by a function that runs on img shards: hip_split of ALL of in's channels
                d = bp.nodes[o.bots[0]]    # (also the one output Freeze leaves of a fan-out: hip_fan_out writes two or more)
                for tp in [tp for i, tp in enumerate(o.tops) if kept(o, i)]:
                    emit(o.tag, add_pipe_op_annotations(Op({"type": "Split"}, {"in": Nda(d), "outs_0": Nda(d), "outs_num": _u32(1)}), tune)[0], {"in": o.bots[0], "out": tp})
                continue
            if t == "BckEltwise":
                tps = [tp for i, tp in enumerate(o.tops) if kept(o, i)]
                emit(o.tag, fan_out_func_op(bp.nodes[o.bots[0]], len(tps)), dict({f"outs_{i}": tp for i, tp in enumerate(tps)}, **{"in": o.bots[0]}))
                continue
            op = grad_op_to_op(bp, o)
            if t == "Convolution":
                a = add_codegen_annotations(op, tune)
                a.nda_vals["conv_has_relu"] = _u32(1 if relu_of[o.tag] else 0)
                # (in front of a BatchNorm the convolution writes the side var <X>_bn_in: X itself is written by hip_bn_fwd)
                calls.append((a, {"filts": o.bots[1], "biases": o.bots[2], "in": o.bots[0], "out": o.tops[0] + BN_IN_SFX if o.tops[0] in bn_runs else o.tops[0]}))
            elif t == "ReLU":    # one that follows no convolution: out = in > 0 ? in : +0 is hip_zero_if_non_pos with the node as its own condition
                z = Op({"type": "ZeroIfNonPos"}, {"in": op_nd(bp, o.bots[0]), "cond": op_nd(bp, o.bots[0]), "out": op_nd(bp, o.bots[0])})
                calls.append((add_bck_op_annotations(z, tune)[0], {"in": o.bots[0], "cond": o.bots[0], "out": o.bots[0]}))
            elif t == "BckConv":
                fi, fb, ff = add_bck_conv_annotations(op, tune)
                b16 = bf16_operands if self.grad_operands else (lambda f: f)
                if kept(o, 0):
                    calls.append((b16(zinp(o, fi)), dict({"filts": o.bots[1], "out_grad_loss": o.bots[3], "in_grad_loss": o.tops[0]}, **({"in": o.bots[0]} if o.tag in takes_relu else {}))))
                if kept(o, 1) and self.fuse_filts_biases:   # one call writes both gradients  (not kept: both params frozen, the data gradient alone)
                    calls.append((b16(bconv_filts_biases_func_op(op, tune)), {"in": o.bots[0], "out_grad_loss": o.bots[3], "filts_grad_loss": o.tops[1], "biases_grad_loss": o.tops[2]}))
                elif kept(o, 1):
                    calls.append((fb, {"out_grad_loss": o.bots[3], "biases_grad_loss": o.tops[2]}))
                    calls.append((ff, {"in": o.bots[0], "out_grad_loss": o.bots[3], "filts_grad_loss": o.tops[1]}))
            elif t == "Pooling":
                self._var(o.tops[0] + "_in_yx", bp.nodes[o.tops[0]])
                calls.append((add_bck_op_annotations(op, tune)[0], {"in": o.bots[0], "out": o.tops[0], "out_in_yx": o.tops[0] + "_in_yx"}))
            elif t == "Spreading":
                calls.append((zinp(o, add_bck_op_annotations(op, tune)[0]), dict({"out": o.bots[0], "out_grad_loss": o.bots[1], "out_in_yx": o.bots[0] + "_in_yx", "in_grad_loss": o.tops[0]},
                                                                                 **({"in": o.bots[2]} if o.tag in takes_relu else {}))))
            elif t == "LRN":
                self._var(o.tops[0] + "_scale_base", bp.nodes[o.tops[0]])
                calls.append((add_bck_op_annotations(op, tune)[0], {"in": o.bots[0], "out": o.tops[0], "out_scale_base": o.tops[0] + "_scale_base"}))
            elif t == "BckLRN":
                calls.append((zinp(o, add_bck_op_annotations(op, tune)[0]), {"in": o.bots[0], "out": o.bots[1], "out_grad_loss": o.bots[2], "out_scale_base": o.bots[1] + "_scale_base",
                                                                             "in_grad_loss": o.tops[0]}))
            elif t == "ZeroIfNonPos":
                calls.append((add_bck_op_annotations(op, tune)[0], {"in": o.bots[0], "cond": o.bots[1], "out": o.tops[0]}))
            elif t == "SoftmaxWithLoss":
                prob, lpp = o.tag + "_prob", o.tops[1] + "_per_pel"
                self._var(prob, bp.nodes[o.bots[0]]); self._var(lpp, bp.nodes[o.bots[1]])
                fs, fg, fl = add_bck_op_annotations(op, tune)
                calls.append((fs, {"in": o.bots[0], "prob": prob}))
                calls.append((fg, {"prob": prob, "label": o.bots[1], "in_grad_loss": o.tops[0], "loss_per_pel": lpp}))
                calls.append((fl, {"loss_per_pel": lpp, "loss": o.tops[1]}))
            elif t in ("Dropout", "BckDropout"):
                fd = add_pipe_op_annotations(op, tune)[0]
                calls.append((seed_from_var(fd), {"inout": o.tops[0], SEED_VAR_ARG: SEED_VAR}) if self.seed_in_var else (fd, {"inout": o.tops[0]}))
            elif t in ("Reduce", "Eltwise"):
                calls.append((add_pipe_op_annotations(op, tune)[0], dict({f"ins_{i}": b for i, b in enumerate(o.bots)}, out=o.tops[0])))
            elif t == "Concat":
                for f, b in zip(add_pipe_op_annotations(op, tune), o.bots):
                    calls.append((f, {"in": b, "out": o.tops[0]}))
            elif t == "Split":
                for i, (f, tp) in enumerate(zip(add_pipe_op_annotations(op, tune), o.tops)):
                    if kept(o, i):
                        calls.append((f, {"in": o.bots[0], "out": tp}))
            else:
                raise UnsupErr(f"ConvPipeBck: op type {t!r} (op {o.tag}) has no native function")
            for fop, args in calls:
                emit(o.tag, fop, args)
        self.n_sgd_calls = 0
        if isinstance(self.solver, Solver):   # sum of squares per chunk, the norm, then the update calls: all behind every gradient op, all counted in n_sgd_calls
            sv = self.solver
            pnames = list(self.sgd_params)
            adam, clip = sv.type == "adam", sv.clip_gradients > 0
            for pn in pnames:
                self._var(pn + SGD_HIST_SFX, bp.cp.params[pn])
                if adam:
                    self._var(pn + SGD_HIST2_SFX, bp.cp.params[pn])
            self._var(SOLVER_HYPER_VAR, Dims(("v",), (8,), "float"))
            self._var(SOLVER_STATE_VAR, Dims(("v",), (4,), "float"))
            per = int(sv.tensors_per_call)
            groups = [pnames[k:k + per] for k in range(0, len(pnames), per)]
            acc = self.iter_size > 1
            gsfx = GRAD_ACC_SFX if acc else "_grad_loss"   # what the norm and the update read: the accumulators, or the step's own gradients
            if acc:   # the accumulate calls in front of the norm and the update, which then read the accumulators
                for pn in pnames:
                    self._var(pn + GRAD_ACC_SFX, bp.cp.params[pn])
                self._var(SOLVER_ACCUM_VAR, Dims(("v",), (4,), "float"))
                for k, grp in enumerate(groups):
                    args = {"accum": SOLVER_ACCUM_VAR}
                    for i, pn in enumerate(grp):
                        args.update({f"g_{i}": pn + "_grad_loss", f"a_{i}": pn + GRAD_ACC_SFX})
                    emit(f"grad_accum_{k}", grad_accum_func_op([bp.cp.params[pn] for pn in grp]), args)
                    self.n_sgd_calls += 1
            if clip:
                parts = sum(-(-bp.cp.params[pn].dims_prod() // SOLVER_CHUNK) for pn in pnames)
                self._var(SOLVER_PARTS_VAR, Dims(("v",), (parts,), "float"))
                part0 = 0
                for k, grp in enumerate(groups):
                    fop = grad_sumsq_func_op([bp.cp.params[pn] for pn in grp], part0, parts)
                    emit(f"grad_sumsq_{k}", fop, dict({f"g_{i}": pn + gsfx for i, pn in enumerate(grp)}, partials=SOLVER_PARTS_VAR))
                    part0 += fop.solver_geom()["chunks"]; self.n_sgd_calls += 1
                emit("grad_norm", grad_norm_func_op(parts), {"partials": SOLVER_PARTS_VAR, "hyper": SOLVER_HYPER_VAR, "state": SOLVER_STATE_VAR})
                self.n_sgd_calls += 1
            for k, grp in enumerate(groups):
                fop = (solver_update_acc_func_op if acc else solver_update_func_op)([bp.cp.params[pn] for pn in grp], sv.type, [sv.mult_of(sv.lr_mult, pn) for pn in grp],
                                                                                    [sv.mult_of(sv.decay_mult, pn) for pn in grp], clip=clip, decoupled_wd=sv.decoupled_wd)
                args = {"hyper": SOLVER_HYPER_VAR, "state": SOLVER_STATE_VAR}
                if acc:
                    args["accum"] = SOLVER_ACCUM_VAR
                for i, pn in enumerate(grp):
                    args.update({f"w_{i}": pn, f"g_{i}": pn + gsfx, f"h_{i}": pn + SGD_HIST_SFX})
                    if adam:
                        args[f"h2_{i}"] = pn + SGD_HIST2_SFX
                emit(f"solver_update_{k}", fop, args)
                self.n_sgd_calls += 1
        elif self.solver is not None:   # the update calls, behind every gradient op
            sv = self.solver
            pnames = list(self.sgd_params)
            for pn in pnames:
                self._var(pn + SGD_HIST_SFX, bp.cp.params[pn])
            self._var(SGD_HYPER_VAR, Dims(("v",), (4,), "float"))
            per = int(sv.tensors_per_call)
            for k in range(0, len(pnames), per):
                grp = pnames[k:k + per]
                fop = sgd_update_func_op([bp.cp.params[pn] for pn in grp], [sv.mult_of(sv.lr_mult, pn) for pn in grp], [sv.mult_of(sv.decay_mult, pn) for pn in grp])
                args = {"hyper": SGD_HYPER_VAR}
                for i, pn in enumerate(grp):
                    args.update({f"w_{i}": pn, f"g_{i}": pn + "_grad_loss", f"h_{i}": pn + SGD_HIST_SFX})
                emit(f"sgd_update_{self.n_sgd_calls}", fop, args)
                self.n_sgd_calls += 1
        rtc.compile(infos)
        params = op_params if op_params is not None else host_params(bp, gen_mode)
        for n, d in bp.cp.params.items():
            if n not in params:
                raise RtErr(f"ConvPipeBck.init: no value for param {n!r}")
            rtc.copy_nda_to_var(n, np.ascontiguousarray(params[n], np.float32).reshape(d.sizes))
        if xf is not None:   # the mean once; a valid plan, so that a pass capture_graph runs on its own reads inside data_raw
            rtc.copy_nda_to_var(DATA_XF_MEAN_VAR, xf_mean)
            self.xf_images = 0; self._input_plan = None
            rtc.copy_nda_to_var(DATA_XF_PLAN_VAR, xf.plan("train", 0, dd.dsz("img")))
        if self.seed_in_var:   # each layer's fixed offset, by value, once: from here on a new seed is four bytes into the var
            for c, k in self._dropout_calls():
                c.rfc.arg_map["det_drop_seed"] = RtcArg.scalar((k * DROP_LAYER_STEP) & 0xFFFFFFFF, "uint32_t")
        self.set_det_drop_seed(0)
        if self.solver is not None:
            self._sgd_hyper = self.solver.hyper()
            self.zero_sgd_history()
            if isinstance(self.solver, Solver):
                self.rtc.copy_nda_to_var(SOLVER_STATE_VAR, np.array([1.0, 0.0, 0.0, 0.0], np.float32))
                if self.iter_size > 1:
                    self.rtc.copy_nda_to_var(SOLVER_ACCUM_VAR, self.accum_words())
            self.set_sgd_hyper()

    def _plan_freeze(self, bp: BckPipe, bn_runs: Dict[str, tuple], multi_dev: bool):
        """Freeze's rule on the pipe -> ({gradient op tag: [is its i-th top still written]}, the set of BatchNorm tags on their running pair); (None, empty set) without
        freeze=.  Sets sgd_params (the trainable params), frozen and _dropped_vars; every refusal comes before anything is created."""
        fz = self.freeze
        self.frozen = {"params": [], "dropped_calls": [], "bn_global": []}
        self._dropped_vars = set()
        if fz is None:
            return None, set()
        cp = bp.cp
        fwd = [o for o in bp.fwd_ops() if o.type != "SoftmaxWithLoss"]
        bn_tags = [o.tag for o in fwd if o.type == "BatchNorm"]
        g = fz.bn_global_stats
        if g is True or g is False or g is None:
            bn_global = list(bn_tags) if g is True else []
        elif isinstance(g, (str, bytes)):
            raise RtErr(f"Freeze: bn_global_stats must be True, False or a list of BatchNorm op tags, got {g!r}")
        else:
            bn_global = list(g)
            for tg in bn_global:
                if tg not in bn_tags:
                    raise RtErr(f"Freeze: bn_global_stats names {tg!r}, which is no BatchNorm op of the pipe")
        if bn_global and multi_dev:
            raise UnsupErr("ConvPipeBck.init: Freeze(bn_global_stats=...): a BatchNorm on its running pair runs as hip_bnf_prep / hip_bnf_bck / hip_bnf_bck_in, which take vars of "
                           "exactly their op's dims and sum over the whole batch: not provided on a multi-device backend (devices=...); freeze params alone there")
        if bn_global and self.img_chunks:
            raise UnsupErr(f"ConvPipeBck.init: Freeze(bn_global_stats=...) together with img_chunks={self.img_chunks}: the hip_bnf_* functions have no chunked chain; a "
                           "BatchNorm on its running pair runs on one device with img_chunks=0")
        cand = list(self.sgd_params)   # every param but the BatchNorm running statistics, in the pipe's order
        params_of = {o.tag: [b for b in o.bots[1:] if b in cand] for o in fwd}
        frozen = set()
        for e in fz.params:
            hit = [e] if e in cand else params_of.get(e) or ([pn for pn in cand if pn.rsplit("_", 1)[-1] == e] if e in PARAM_SFXS else [])
            if not hit:
                raise RtErr(f"Freeze: params names {e!r}, which is no param of the pipe, no tag of an op with params and none of the suffixes {' | '.join(PARAM_SFXS)} of a param "
                            "(a BatchNorm's running statistics are never solver params: see bn_global_stats)")
            frozen.update(hit)
        trainable = [pn for pn in cand if pn not in frozen]
        if not trainable:
            raise RtErr("ConvPipeBck.init: Freeze leaves nothing trainable: every param of the pipe is frozen, so a step would compute no gradient")
        for nn in fz.keep_grads:
            if nn not in cp.nodes:
                raise RtErr(f"Freeze: keep_grads names {nn!r}, which is no node of the pipe (`{bp.label_node}` has no gradient)")
        # the forward walk: need[node] = does the node's CURRENT value need a gradient (an in-place op rewrites the node it reads)
        need = {cp.in_node: cp.in_node in fz.keep_grads}
        in_need: Dict[str, List[bool]] = {}
        op_train: Dict[str, bool] = {}
        for o in fwd:
            data_bots = [b for b in o.bots if b in cp.nodes]
            in_need[o.tag] = [need.get(b, False) for b in data_bots]
            op_train[o.tag] = any(pn not in frozen for pn in params_of[o.tag])
            need[o.tops[0]] = op_train[o.tag] or any(in_need[o.tag]) or (not o.in_place and o.tops[0] in fz.keep_grads)
        glob_x = {x for x, (bn, _, _) in bn_runs.items() if bn.tag in bn_global}
        keep: Dict[str, List[bool]] = {}
        for b in bp.bck_ops():
            if b.type == "Reduce":
                continue
            f = b.tag[:-4]   # <forward tag>_bck
            if b.type in ("BckConv", "BckScale"):
                k = [in_need[f][0], op_train[f], op_train[f]]
                if b.type == "BckScale" and b.bots[1] not in glob_x and in_need[f][0]:
                    k[1] = k[2] = True   # a training BatchNorm's data gradient reads the two sums
            else:
                k = list(in_need[f])
            keep[b.tag] = k
        written = {tp for b in bp.bck_ops() if b.type != "Reduce" for i, tp in enumerate(b.tops) if keep[b.tag][i]}
        written.update(tp for o in bp.fwd_ops() for tp in o.tops)
        for b in bp.bck_ops():   # a Reduce at a fan-out is kept or dropped whole: every reader of a node that needs a gradient produces its partial
            if b.type == "Reduce":
                have = [i in written for i in b.bots]
                if any(have) != all(have):
                    raise RtErr(f"ConvPipeBck.init: Freeze: {b.tag} would sum {sum(have)} of its {len(have)} partial gradients")
                keep[b.tag] = [all(have)]
                if all(have):
                    written.add(b.tops[0])
        self._dropped_vars = {tp for b in bp.bck_ops() for tp in b.tops} - written
        self.sgd_params = trainable
        self.frozen = {"params": [pn for pn in cand if pn in frozen], "dropped_calls": [b.tag for b in bp.bck_ops() if not any(keep[b.tag])],
                       "bn_global": [tg for tg in bn_tags if tg in bn_global]}
        return keep, set(bn_global)

    @staticmethod
    def _plan_bn_runs(bp: BckPipe) -> Dict[str, tuple]:
        """node X -> (BatchNorm op, Scale op, the in-place ReLU behind them or None) for every BatchNorm / Scale of the pipe; raises UnsupErr for every shape but
        [BatchNorm, Scale] (+ ReLU) on a node a Convolution produces."""
        fwd = [o.src for o in bp.fwd_ops() if o.src is not None]
        runs: Dict[str, tuple] = {}
        producer = {o.top: o for o in fwd if not o.in_place}
        for x in dict.fromkeys(o.bot for o in fwd if o.type in AFFINE_IN_PLACE_TYPES):
            ips = [o for o in fwd if o.in_place and o.bot == x]
            kinds = [o.type for o in ips]
            what = f"the in-place ops on {x} are {' '.join(kinds)}"
            if x not in producer or producer[x].type != "Convolution":
                raise UnsupErr(f"ConvPipeBck: a BatchNorm / Scale on {x}, which {'a ' + producer[x].type if x in producer else 'no op'} produces; only [BatchNorm, Scale] (+ ReLU) behind a Convolution is supported")
            if kinds[:2] != ["BatchNorm", "Scale"]:
                raise UnsupErr(f"ConvPipeBck: {what}; only the run [BatchNorm, Scale] (+ ReLU) is supported (a training BatchNorm and its Scale run as one function)")
            if kinds[2:] not in ([], ["ReLU"]):
                raise UnsupErr(f"ConvPipeBck: {what}; behind [BatchNorm, Scale] only one in-place ReLU is supported")
            runs[x] = (ips[0], ips[1], ips[2] if len(ips) > 2 else None)
        return runs

    def set_sgd_hyper(self, lr: Optional[float] = None, momentum: Optional[float] = None, weight_decay: Optional[float] = None, momentum2: Optional[float] = None,
                      delta: Optional[float] = None, clip_gradients: Optional[float] = None) -> None:
        """Upload the 16 bytes of sgd_hyper (a Solver: the 32 bytes of solver_hyper, for step `iter`) with the values given replaced (None: kept).  Touches no call: the
        next step -- eager or a graph replay -- reads them.  momentum2 / delta / clip_gradients are a Solver's; with a Solver that has an lr_policy the policy owns lr, and
        setting it is an RtErr.  clip_gradients can be changed, not switched on or off: the calls were made for one or the other."""
        if self.solver is None:
            raise RtErr("ConvPipeBck.set_sgd_hyper: the driver was built without a solver")
        gen = isinstance(self.solver, Solver)
        if not gen and any(v is not None for v in (momentum2, delta, clip_gradients)):
            raise RtErr("ConvPipeBck.set_sgd_hyper: momentum2 / delta / clip_gradients are a Solver's; the driver was built with an SgdSolver")
        if gen and lr is not None and self.solver.lr_policy is not None:
            raise RtErr(f"ConvPipeBck.set_sgd_hyper: lr is set by the solver's lr_policy ({self.solver.lr_policy.policy}); build the Solver without one to set it by hand")
        if gen and clip_gradients is not None and (float(clip_gradients) > 0) != (self.solver.clip_gradients > 0):
            raise RtErr("ConvPipeBck.set_sgd_hyper: clip_gradients cannot be switched on or off after init (the clipping calls exist or they do not); build the Solver with it")
        for i, v in ((0, lr), (1, momentum), (2, weight_decay)) + (((3, momentum2), (4, delta), (6, clip_gradients)) if gen else ()):
            if v is not None:
                self._sgd_hyper[i] = np.float32(v)
        if gen:
            if lr is not None:
                self._base_lr = float(lr)
            self._upload_solver_hyper()
        else:
            self.rtc.copy_nda_to_var(SGD_HYPER_VAR, self._sgd_hyper)

    def _upload_solver_hyper(self) -> None:
        """The 32 bytes of solver_hyper for step self.iter: lr from the policy (where there is one), adam's corr for t = iter + 1 from the fp32 momenta."""
        sv, h = self.solver, self._sgd_hyper
        if sv.lr_policy is not None:
            h[0] = np.float32(sv.lr_policy.lr_at(self._base_lr, self.iter))
        h[5] = np.float32(Solver.corr(h[1], h[3], self.iter + 1)) if sv.type == "adam" else np.float32(1.0)
        self.rtc.copy_nda_to_var(SOLVER_HYPER_VAR, h)

    def accum_words(self) -> np.ndarray:
        """The 16 bytes of solver_accum for the next micro-step: [micro == 0, micro == iter_size - 1, fp32(1 / iter_size), micro]."""
        n, m = self.iter_size, self.micro
        return np.array([1.0 if m == 0 else 0.0, 1.0 if m == n - 1 else 0.0, np.float32(1.0 / n), m], np.float32)

    # -- the input transform
    def _xf_batch(self) -> int:
        return self.bp.nodes[self.bp.cp.in_node].dsz("img")

    def set_input_mean(self, mean) -> None:
        """Upload data_xf_mean again: an array of the var's dims (chan, or chan:y:x at the source size, as the driver was built)."""
        if self.input_transform is None:
            raise RtErr("ConvPipeBck.set_input_mean: the driver was built without an input_transform")
        d = self.input_transform.mean_dims(self.bp.nodes[self.bp.cp.in_node].dsz("chan"))
        a = np.ascontiguousarray(mean, np.float32)
        if a.shape != d.sizes:
            raise RtErr(f"ConvPipeBck.set_input_mean: {DATA_XF_MEAN_VAR} is float {d.pretty()}, got shape {a.shape}")
        self.rtc.copy_nda_to_var(DATA_XF_MEAN_VAR, a)

    def set_input_plan(self, plan) -> None:
        """The next pass -- one pass -- runs under this plan (uint32 (B, 4) = y_off, x_off, mirror, unused per image) instead of the train plan; checked here and
        again before the upload.  xf_images advances behind that pass all the same."""
        if self.input_transform is None:
            raise RtErr("ConvPipeBck.set_input_plan: the driver was built without an input_transform")
        self._input_plan = self.input_transform.check_plan(plan, self._xf_batch())

    def _before_pass(self) -> None:
        xf = self.input_transform
        if xf is not None:
            B = self._xf_batch()
            plan = self._input_plan if self._input_plan is not None else xf.plan("train", self.xf_images, B)
            self.rtc.copy_nda_to_var(DATA_XF_PLAN_VAR, xf.check_plan(plan, B))

    def _after_pass(self) -> None:
        if self.input_transform is not None:
            self.xf_images += self._xf_batch()
            self._input_plan = None

    def _before_update_step(self) -> None:
        self._before_pass()
        if isinstance(self.solver, Solver):
            self._upload_solver_hyper()
            if self.iter_size > 1:
                self.rtc.copy_nda_to_var(SOLVER_ACCUM_VAR, self.accum_words())

    def _after_update_step(self) -> None:
        self._after_pass()
        if isinstance(self.solver, Solver):
            if self.iter_size > 1:   # `iter` counts updates: it advances behind the applying micro-step only
                applied = self.micro == self.iter_size - 1
                self.micro = (self.micro + 1) % self.iter_size
                if not applied:
                    return
            self.iter += 1

    def zero_sgd_history(self) -> None:
        """Clear every <param>_sgd_hist (and, for adam, <param>_sgd_hist2), and start a Solver's step count `iter` -- and, with iter_size > 1, `micro` -- again at 0
        (the accumulators need no clearing: the first micro-step overwrites them)."""
        if self.solver is None:
            raise RtErr("ConvPipeBck.zero_sgd_history: the driver was built without a solver")
        adam = isinstance(self.solver, Solver) and self.solver.type == "adam"
        for pn in self.sgd_params:
            self.rtc.copy_nda_to_var(pn + SGD_HIST_SFX, np.zeros(self.bp.cp.params[pn].sizes, np.float32))
            if adam:
                self.rtc.copy_nda_to_var(pn + SGD_HIST2_SFX, np.zeros(self.bp.cp.params[pn].sizes, np.float32))
        self.iter = 0
        self.micro = 0

    def _dropout_calls(self) -> List[Tuple[BckCall, int]]:
        """The dropout calls of the step with their layer's index among the pipe's Dropout ops (a layer's forward and backward call share it)."""
        layer: Dict[str, int] = {}
        out = []
        for c in self.bck_calls:
            if c.fop.get_func_name() == "hip_dropout":
                tag = c.tag[:-4] if c.tag.endswith("_bck") else c.tag
                out.append((c, layer.setdefault(tag, len(layer))))
        return out

    def set_det_drop_seed(self, seed: int) -> None:
        """Rewrite the by-value det_drop_seed of every dropout call.  The forward and the backward call of one layer get the same seed (the gradient must drop what
        the forward pass dropped); layers differ by their position among the pipe's Dropout ops.  With seed_in_var the calls stay as they are -- they carry their layer's
        offset -- and the seed is uploaded into the var they all read."""
        if self.seed_in_var:
            self.rtc.copy_nda_to_var(SEED_VAR, np.array([int(seed) & 0xFFFFFFFF], np.uint32))
            return
        for c, k in self._dropout_calls():
            c.rfc.arg_map["det_drop_seed"] = RtcArg.scalar((int(seed) + k * DROP_LAYER_STEP) & 0xFFFFFFFF, "uint32_t")
            c.rfc.invalidate()

    def calls(self) -> List[Tuple[str, Op, Dict[str, RtcArg]]]:
        """The ordered (tag, function op, arg map) list of the step."""
        return [(c.tag, c.fop, dict(c.rfc.arg_map)) for c in self.bck_calls]

    def run_bck(self, to_set_vns: Sequence[str], fwd: Dict[str, np.ndarray], to_get_vns: Sequence[str], graph: bool = False) -> None:
        """Set inputs (data, label) -> run all calls -> get outputs into `fwd`: ConvPipeFwd.run_fwd's contract.  graph=True: the calls run as one replay of the
        graph capture_graph made."""
        rtc = self.rtc
        if graph and self._graph is None:
            raise RtErr("ConvPipeBck.run_bck(graph=True): no captured graph -- call capture_graph() first")
        for v in to_get_vns:
            if v in self._dropped_vars:
                raise RtErr(f"ConvPipeBck.run_bck: {v!r} is not computed by this driver: {WHY_DROPPED}")
        if self.input_transform is not None and self.bp.cp.in_node in to_set_vns:
            raise RtErr(f"ConvPipeBck.run_bck: the driver was built with an input_transform: its {DATA_XF_TAG} call writes {self.bp.cp.in_node!r} from {DATA_RAW_VAR!r} on every "
                        f"pass and would overwrite what is fed; feed {DATA_RAW_VAR!r} (uint8), or build the driver without input_transform")
        for v in to_set_vns:
            rtc.copy_nda_to_var(v, fwd[v])
        rtc.finish_and_sync()
        if graph:
            self.run_graph()
        else:
            self.run_device_only()
        for v in to_get_vns:
            fwd[v] = rtc.copy_var_to_nda(v)

    def run_device_only(self, skip_sgd: bool = False) -> float:
        """Run all calls once with the inputs already resident; -> ms first-call-start to last-call-end.  per_call_ms: (tag, function, ms) per call.
        skip_sgd: leave the solver's update calls out (what capture_graph's preparing step does: params and history stay as they are)."""
        rtc = self.rtc
        todo = self.bck_calls[:len(self.bck_calls) - self.n_sgd_calls] if skip_sgd else self.bck_calls
        if not skip_sgd:
            self._before_update_step()
        for c in todo:
            c.call_id = rtc.run(c.rfc)
        rtc.finish_and_sync()
        if not skip_sgd:
            self._after_update_step()
        ids = [c.call_id for c in todo]
        self.compute_dur_ms = rtc.get_dur(ids[0], ids[-1]) if ids else 0.0
        self.per_call_ms = [(c.tag, c.fop.get_func_name(), rtc.get_dur(i, i)) for c, i in zip(todo, ids)]
        rtc.release_per_call_id_data()
        self._stepped = True
        return self.compute_dur_ms

    # -- hipGraph form of run_device_only: the call list captured once, replayed with one host call per step
    def capture_graph(self, parallel: bool = False) -> int:
        """Capture the step's call list into a hipGraph; -> number of captured calls.  If no ordinary step has run since init, one runs first on whatever the vars
        hold: the K-slice workspaces and lazily built kernels must exist before a capture.  parallel=True: the graph gets the calls' true dependencies (_call_deps)
        instead of the launch order, so that independent calls -- the three gradients of one BckConv, the branches of a fan-out -- may overlap.  A second capture
        destroys the first.  Not provided on a multi-device backend (devices=...): the step runs there eagerly, its cross-device sums are no part of a device's capture."""
        rtc = self.rtc
        drops = [c.tag for c, _ in self._dropout_calls()]
        if drops and not self.seed_in_var:
            raise RtErr(f"ConvPipeBck.capture_graph: the pipe has dropout calls ({', '.join(drops)}) whose det_drop_seed is a by-value argument: a captured launch freezes "
                        "it, and every replay would drop the same elements.  Build the driver with seed_in_var=True: the seed then lives in a var the replay reads")
        if isinstance(getattr(rtc, "devices", None), list):
            raise UnsupErr("ConvPipeBck.capture_graph: not provided on a multi-device backend (devices=...)")
        deps = self._call_deps() if parallel else None   # (before the capture opens: a host-side error here leaves none behind)
        if self._graph is not None:
            rtc.graph_destroy(self._graph); self._graph = None
        if not self._stepped:   # (without the update calls: a capture leaves params and history as they were; their kernel was built when they were compiled)
            stats = {vn: rtc.copy_var_to_nda(vn) for vn in bn_stat_params(self.bp.cp)}   # (a forward pass moves a BatchNorm's running pair: put back below)
            self.run_device_only(skip_sgd=True)
            for vn, a in stats.items():
                rtc.copy_nda_to_var(vn, a)
        rtc.finish_and_sync()
        rtc.graph_begin()
        for c in self.bck_calls:   # (a call that raises inside a capture: the backend drops the capture before it rethrows)
            rtc.run(c.rfc)
        if parallel:
            self.call_deps = deps
            self._graph = rtc.graph_end_deps(deps); n = len(self.bck_calls)
        else:
            self._graph, n = rtc.graph_end()
        return n

    def _call_deps(self) -> List[List[int]]:
        """deps[i] = the earlier calls that call i must run after, from the IN / OUT kinds of each call's pipe_func_args on WHOLE vars: a call runs after the last
        writer of every var it reads or writes (read-after-write, write-after-write) and after every reader since of a var it writes (write-after-read).  The in-place
        arg `inout` is read and written; a var bound to an IN and an OUT arg of one call (an in-place hip_zero_if_non_pos) likewise.  The `in` of a zero_if_in_non_pos
        call is an IN like any other.  The params and det_drop_seed are only read inside a step and order nothing -- unless the
        driver has a solver: an arg of kind INOUT (w_i, h_i of hip_sgd_update) is read and written, so an update call follows every forward and backward reader of
        its params (write after read) and the writers of its gradients.  The hip_concat calls of one op fill disjoint
        channel ranges of one var; as whole-var writers they simply stay in list order among themselves, and a reader of the var follows the last of them."""
        writer: Dict[str, int] = {}
        readers: Dict[str, List[int]] = {}
        deps: List[List[int]] = []
        for i, c in enumerate(self.bck_calls):
            am = c.rfc.arg_map
            rd, wr = set(), set()
            for an, io in pipe_func_args(c.fop):
                if io in ("IN", "INOUT") or an == "inout":
                    rd.add(am[an].n)
                if io in ("OUT", "INOUT"):
                    wr.add(am[an].n)
            d = {writer[v] for v in rd | wr if v in writer}
            for v in wr:
                d.update(readers.get(v, ()))
            d.discard(i)
            for v in rd:
                readers.setdefault(v, []).append(i)
            for v in wr:
                writer[v] = i; readers[v] = []
            deps.append(sorted(d))
        return deps

    def run_graph(self) -> float:
        """One step as one graph launch; -> ms of the whole replay.  A replay has no per-call times: per_call_ms is []."""
        rtc = self.rtc
        if self._graph is None:
            raise RtErr("ConvPipeBck.run_graph: no captured graph -- call capture_graph() first")
        self._before_update_step()
        cid = rtc.graph_launch(self._graph)
        rtc.finish_and_sync()
        self._after_update_step()
        self.compute_dur_ms = rtc.get_dur(cid, cid)
        self.per_call_ms = []
        rtc.release_per_call_id_data()
        return self.compute_dur_ms

    def release(self) -> None:
        if self._graph is not None:   # (before the funcs and vars its kernel nodes point into)
            self.rtc.graph_destroy(self._graph); self._graph = None
        for f in self.funcs:
            self.rtc.release_func(f)
        for v in self.vars:
            self.rtc.release_var(v)
        self.funcs, self.vars, self.bck_calls = [], [], []
        self.n_sgd_calls = 0
        self._stepped = False


def op_nd(bp: BckPipe, node: str) -> Nda:
    return Nda(bp.nodes[node])
