"""Full-net gradient pipe: the training-form driver `ConvPipeBck`.  The graph reversal it runs (`add_bck_ops`, boda_amd/bck_graph.py), what it is configured with
(the solvers and Freeze, boda_amd/solver_cfg.py) and its call list (boda_amd/call_list.py) are modules of their own; every name of theirs is imported from here as before.

Restates the behaviour of the gradient half of the reference's conv_pipe_fwd_t::gen_op (not its code), src/rtc_fwd.cc:263-405:
      one call per function, vars kept on the device, the side vars <out>_in_yx / <out>_scale_base / <tag>_prob / <loss>_per_pel under those names, dropout's
      det_drop_seed a by-value argument of the call that is rewritten per step.
Every function is a native one (boda_amd/cnn_op.py: hip_conv, BCONV_FUNCS, BCK_OP_FUNCS, PIPE_OP_FUNCS), so the same pipe runs on be=hip and on be=cpu, the bit-exact
checker.  Unfused, fp32, reference layouts, one device; ConvPipe / ConvPipeFwd (the inference pipe) are not touched.
"""
from __future__ import annotations
import zlib
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from .bck_graph import (AFFINE_IN_PLACE_TYPES, DROPOUT_RATIO, IN_PLACE_TYPES, RELU_GRAD_PRODUCERS, BckPipe, GradOp, LossSpec, _u32, add_bck_ops, grad_op_to_op,
                        plan_relu_grad_folds)
from .call_list import BckCall, CallList
from .cnn_op import (OpTune, SGD_MAX_TENS, bn_bck_in_func_op, bn_bck_sums_func_op, bn_fwd_func_op, bn_stats_func_op, bnc_bck_in_func_op, bnc_bck_sums_func_op, bnc_fwd_func_op, bnc_stats_func_op, BNC_MAX_CHUNKS, fan_out_func_op, sgd_update_func_op, solver_update_func_op, grad_sumsq_func_op, grad_norm_func_op, grad_accum_func_op, solver_update_acc_func_op, add_bck_conv_annotations, bconv_filts_biases_func_op, add_bck_op_annotations, add_codegen_annotations, add_pipe_op_annotations, fuse_zero_if_in_non_pos,
                     seed_from_var, SEED_VAR_ARG, bf16_operands, is_grouped)
from .cnn_op import bck_deconv_calls, deconv_calls, deconv_role_dims, bnf_bck_func_op, bnf_bck_in_func_op, bnf_prep_func_op, data_transform_func_op, loss_norm_func_op, softmax_loss_bck_func_op, softmax_loss_fwd_func_op
from .conv_pipe import ConvPipe, PipeOp
from .input_pipe import DATA_RAW_VAR, DATA_XF_MEAN_VAR, DATA_XF_PLAN_VAR, DATA_XF_TAG, InputTransform
from .op import Dims, Nda, Op, RtErr, SOLVER_CHUNK, UnsupErr
from .rtc import RtcArg
from .solver_cfg import (GRAD_ACC_SFX, PARAM_SFXS, SGD_HIST2_SFX, SGD_HIST_SFX, SGD_HYPER_VAR, SOLVER_ACCUM_VAR, SOLVER_HYPER_VAR, SOLVER_PARTS_VAR, SOLVER_STATE_VAR,
                         WHY_DROPPED, Freeze, LrPolicy, SgdSolver, Solver)

BN_IN_SFX = "_bn_in"                # <X>_bn_in: what the convolution in front of a BatchNorm wrote (X itself holds the normalised, scaled, rectified values)
BN_MEAN_SFX, BN_ISTD_SFX = "_batch_mean", "_batch_inv_std"   # <bn-tag>_batch_mean / _batch_inv_std: the statistics of the step's batch
BN_STAT_SFXS = ("_mean", "_var")    # a BatchNorm's params: running statistics, rewritten by the forward pass and never by a solver
LOSS_STATE_SFX = "_state"           # <loss>_state: float v=4 = (Z, s, count, sum) of a head with a LossSpec; hip_softmax_loss_bck reads s from it
SEED_VAR = "det_drop_seed"   # ConvPipeBck(seed_in_var=True): the one-word uint32 var every dropout call reads its seed from
DROP_LAYER_STEP = 0x9E3779B1   # the k-th Dropout layer of a pipe hashes with seed + k * this (mod 2^32)


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


@dataclass
class BckPlan:
    """What ConvPipeBck.plan returns, made without one backend call: what init creates, and what it reports."""
    vars: List[Tuple[str, Dims]]                     # in creation order
    calls: List[Tuple[str, Op, Dict[str, str]]]      # (tag, annotated function op, {arg: var}) in run order; the last n_sgd_calls are the solver's
    n_sgd_calls: int
    sgd_params: List[str]
    frozen: Dict[str, object]
    fused_relu_grads: Dict[str, object]
    dropped_vars: set
    bn_runs: Dict[str, tuple]                        # node X -> (BatchNorm op, Scale op, the ReLU behind them or None); EvalPipe reads them from the driver
    xf_mean: Optional[np.ndarray] = None             # what data_xf_mean is uploaded with


@dataclass
class SideVar:
    """A var of a plan that is more than its dims: a reshaped view of another var (the same memory under other dim names), or a constant filled once at init."""
    dims: Dims
    view_of: Optional[str] = None
    fill: Optional[float] = None


class _Lower:
    """The lowering of one pipe's ops under one driver's options.  One method per op family, picked by BY_TYPE from GradOp.type; each -> ([(function op, {arg: var})] in
    call order, [(side var, Dims)]).  lower(o) is the entry: no call for a ReLU its convolution or BatchNorm run took, for a folded ReLU gradient, and for a gradient op
    Freeze left no output."""

    def __init__(self, drv: "ConvPipeBck", bp: BckPipe, bn_runs: Dict[str, tuple], keep: Optional[Dict[str, List[bool]]], bn_global: set, folds: Dict[str, str]):
        self.d, self.bp, self.tune, self.bn_runs, self.keep, self.bn_global = drv, bp, drv.op_tune, bn_runs, keep, bn_global
        self.takes_relu = set(folds.values())   # the gradient ops that apply the mask of the ZeroIfNonPos behind them
        self.no_call = set(folds)   # + the ReLUs taken into their convolution (src/rtc_fwd.cc:486-493): no forward call, their ZeroIfNonPos still runs
        self.relu_of: Dict[str, bool] = {}
        ops = bp.ops
        for i, o in enumerate(ops[:bp.n_fwd]):
            if o.type == "Convolution":
                first_ip = next((q for q in ops[i + 1:bp.n_fwd] if q.in_place and q.bots[0] == o.tops[0]), None)
                self.relu_of[o.tag] = bool(first_ip and first_ip.type == "ReLU")
                if self.relu_of[o.tag]:
                    self.no_call.add(first_ip.tag)
        self.no_call.update(relu.tag for _, _, relu in bn_runs.values() if relu is not None)   # the ReLU behind a [BatchNorm, Scale] run is hip_bn_fwd's
        self.bn_of_tag = {q.tag: (x, run) for x, run in bn_runs.items() for q in run[:2]}
        self.by_tag_bck = {o.tag: o for o in bp.bck_ops()}

    def kept(self, o: GradOp, i: int) -> bool:
        """Does gradient op o still write its i-th top?"""
        return self.keep is None or o.tag not in self.keep or self.keep[o.tag][i]

    def lower(self, o: GradOp) -> Tuple[list, list]:
        if o.tag in self.no_call or (self.keep is not None and o.tag in self.keep and not any(self.keep[o.tag])):
            return [], []
        if o.type not in self.BY_TYPE:
            raise UnsupErr(f"bck_pipe: op type {o.type!r} (op {o.tag}) has no native function")
        return self.BY_TYPE[o.type](self, o)

    def _bck_ann(self, o: GradOp) -> Op:
        """The one function of a non-conv op, with the mask of the ReLU gradient it took."""
        f = add_bck_op_annotations(grad_op_to_op(self.bp, o), self.tune)[0]
        return fuse_zero_if_in_non_pos(f) if o.tag in self.takes_relu else f

    def conv(self, o):
        a = add_codegen_annotations(grad_op_to_op(self.bp, o), self.tune)
        a.nda_vals["conv_has_relu"] = _u32(1 if self.relu_of[o.tag] else 0)
        # (in front of a BatchNorm the convolution writes the side var <X>_bn_in: X itself is written by hip_bn_fwd)
        return [(a, {"filts": o.bots[1], "biases": o.bots[2], "in": o.bots[0], "out": o.tops[0] + BN_IN_SFX if o.tops[0] in self.bn_runs else o.tops[0]})], []

    def relu(self, o):    # one that follows no convolution: out = in > 0 ? in : +0 is hip_zero_if_non_pos with the node as its own condition
        z = Op({"type": "ZeroIfNonPos"}, {an: Nda(self.bp.nodes[o.bots[0]]) for an in ("in", "cond", "out")})
        return [(add_bck_op_annotations(z, self.tune)[0], {"in": o.bots[0], "cond": o.bots[0], "out": o.bots[0]})], []

    def bck_conv(self, o):
        op = grad_op_to_op(self.bp, o)
        fi, fb, ff = add_bck_conv_annotations(op, self.tune)
        b16 = bf16_operands if self.d.grad_operands else (lambda f: f)
        calls = []
        if self.kept(o, 0):
            takes = o.tag in self.takes_relu
            calls.append((b16(fuse_zero_if_in_non_pos(fi) if takes else fi), dict({"filts": o.bots[1], "out_grad_loss": o.bots[3], "in_grad_loss": o.tops[0]}, **({"in": o.bots[0]} if takes else {}))))
        if self.kept(o, 1) and self.d.fuse_filts_biases and not is_grouped(op):   # one call writes both gradients  (not kept: both params frozen, the data gradient alone; a grouped layer stays on its two calls)
            calls.append((b16(bconv_filts_biases_func_op(op, self.tune)), {"in": o.bots[0], "out_grad_loss": o.bots[3], "filts_grad_loss": o.tops[1], "biases_grad_loss": o.tops[2]}))
        elif self.kept(o, 1):
            calls.append((fb, {"out_grad_loss": o.bots[3], "biases_grad_loss": o.tops[2]}))
            calls.append((ff, {"in": o.bots[0], "out_grad_loss": o.bots[3], "filts_grad_loss": o.tops[1]}))
        return calls, []

    def _deconv_bound(self, o, op, calls, roles):
        """The calls of cnn_op.deconv_calls / bck_deconv_calls with their roles bound: the layer's own vars from `roles`; on the matrix path the views of the layer's
        vars under the exchanged dims (<tag>_filts_x, <tag>_filts_grad_loss_x, <tag>_biases_x) and the constants <tag>_ones / <tag>_zeros as side vars."""
        tag, out, side = o.src.tag, [], []
        view_of = {"filts_x": "filts", "filts_grad_loss_x": "filts_grad_loss", "biases_x": "biases"}
        fill = {"ones": 1.0, "zeros": 0.0}
        for fop, binds in calls:
            args = {}
            for an, role in binds.items():
                if role in roles:
                    args[an] = roles[role]; continue
                vn = f"{tag}_{role}"
                sv = SideVar(deconv_role_dims(op, role), view_of=roles[view_of[role]]) if role in view_of else SideVar(deconv_role_dims(op, role), fill=fill[role])
                if vn in self.bp.nodes:
                    raise RtErr(f"ConvPipeBck.init: the Deconvolution {tag!r} needs the var name {vn!r}, which is a node of the pipe")
                side.append((vn, sv)); args[an] = vn
            out.append((fop, args))
        return out, side

    def deconv(self, o):   # hip_deconv, or the matrix path's hip_bconv_in + hip_chan_affine; a ReLU behind it is `relu` above, as behind any op that is no Convolution
        op = grad_op_to_op(self.bp, o)
        return self._deconv_bound(o, op, deconv_calls(op, self.tune), {"filts": o.bots[1], "biases": o.bots[2], "in": o.bots[0], "out": o.tops[0]})

    def bck_deconv(self, o):   # BckConv's three calls in its order; Freeze drops the data gradient or the filter / bias pair as for a BckConv
        op = grad_op_to_op(self.bp, o)
        ci, cb, cf = bck_deconv_calls(op, self.tune)
        calls = ([ci] if self.kept(o, 0) else []) + ([cb, cf] if self.kept(o, 1) else [])
        return self._deconv_bound(o, op, calls, {"in": o.bots[0], "filts": o.bots[1], "biases": o.bots[2], "out_grad_loss": o.bots[3], "in_grad_loss": o.tops[0],
                                                 "filts_grad_loss": o.tops[1], "biases_grad_loss": o.tops[2]})

    def crop(self, o):
        return [(self._bck_ann(o), {"in": o.bots[0], "out": o.tops[0]})], []

    def bck_crop(self, o):
        return [(self._bck_ann(o), {"out_grad_loss": o.bots[0], "in_grad_loss": o.tops[0]})], []

    def pool(self, o):
        yx = o.tops[0] + "_in_yx"
        return [(self._bck_ann(o), {"in": o.bots[0], "out": o.tops[0], "out_in_yx": yx})], [(yx, self.bp.nodes[o.tops[0]])]

    def spreading(self, o):
        args = {"out": o.bots[0], "out_grad_loss": o.bots[1], "out_in_yx": o.bots[0] + "_in_yx", "in_grad_loss": o.tops[0]}
        return [(self._bck_ann(o), dict(args, **({"in": o.bots[2]} if o.tag in self.takes_relu else {})))], []

    def lrn(self, o):
        sb = o.tops[0] + "_scale_base"
        return [(self._bck_ann(o), {"in": o.bots[0], "out": o.tops[0], "out_scale_base": sb})], [(sb, self.bp.nodes[o.tops[0]])]

    def bck_lrn(self, o):
        return [(self._bck_ann(o), {"in": o.bots[0], "out": o.bots[1], "out_grad_loss": o.bots[2], "out_scale_base": o.bots[1] + "_scale_base", "in_grad_loss": o.tops[0]})], []

    def zero_if_non_pos(self, o):
        return [(self._bck_ann(o), {"in": o.bots[0], "cond": o.bots[1], "out": o.tops[0]})], []

    def loss(self, o):
        prob, lpp = o.tag + "_prob", o.tops[1] + "_per_pel"
        if o.spec is not None:   # the full SoftmaxWithLoss (kernels/loss_f32.hip): the normaliser and s = weight / Z live in <loss>_state, on the device
            d, st = self.bp.nodes[o.bots[0]], o.tops[1] + LOSS_STATE_SFX
            return ([(softmax_loss_fwd_func_op(d, o.spec), {"in": o.bots[0], "label": o.bots[1], "prob": prob, "loss_per_pel": lpp}),
                     (loss_norm_func_op(d, o.spec), {"label": o.bots[1], "loss_per_pel": lpp, "loss": o.tops[1], "loss_state": st}),
                     (softmax_loss_bck_func_op(d, o.spec), {"prob": prob, "label": o.bots[1], "loss_state": st, "in_grad_loss": o.tops[0]})],
                    [(prob, d), (lpp, self.bp.nodes[o.bots[1]]), (st, Dims(("v",), (4,), "float"))])
        fs, fg, fl = add_bck_op_annotations(grad_op_to_op(self.bp, o), self.tune)
        return ([(fs, {"in": o.bots[0], "prob": prob}), (fg, {"prob": prob, "label": o.bots[1], "in_grad_loss": o.tops[0], "loss_per_pel": lpp}),
                 (fl, {"loss_per_pel": lpp, "loss": o.tops[1]})], [(prob, self.bp.nodes[o.bots[0]]), (lpp, self.bp.nodes[o.bots[1]])])

    def dropout(self, o):
        fd = add_pipe_op_annotations(grad_op_to_op(self.bp, o), self.tune)[0]
        return [(seed_from_var(fd), {"inout": o.tops[0], SEED_VAR_ARG: SEED_VAR}) if self.d.seed_in_var else (fd, {"inout": o.tops[0]})], []

    def reduce(self, o):
        return [(add_pipe_op_annotations(grad_op_to_op(self.bp, o), self.tune)[0], dict({f"ins_{i}": b for i, b in enumerate(o.bots)}, out=o.tops[0]))], []

    def concat(self, o):
        return [(f, {"in": b, "out": o.tops[0]}) for f, b in zip(add_pipe_op_annotations(grad_op_to_op(self.bp, o), self.tune), o.bots)], []

    def split(self, o):
        fs = add_pipe_op_annotations(grad_op_to_op(self.bp, o), self.tune)
        return [(f, {"in": o.bots[0], "out": tp}) for i, (f, tp) in enumerate(zip(fs, o.tops)) if self.kept(o, i)], []

    def bck_eltwise(self, o):
        d = self.bp.nodes[o.bots[0]]
        tps = [tp for i, tp in enumerate(o.tops) if self.kept(o, i)]
        if self.d.img_chunks or len(tps) == 1:   # one copy per output by a function that runs on img shards: hip_split of ALL of in's channels
            one = lambda: add_pipe_op_annotations(Op({"type": "Split"}, {"in": Nda(d), "outs_0": Nda(d), "outs_num": _u32(1)}), self.tune)[0]
            return [(one(), {"in": o.bots[0], "out": tp}) for tp in tps], []   # (also the one output Freeze leaves of a fan-out: hip_fan_out writes two or more)
        return [(fan_out_func_op(d, len(tps)), dict({f"outs_{i}": tp for i, tp in enumerate(tps)}, **{"in": o.bots[0]}))], []

    def bn_run(self, o):
        """A [BatchNorm, Scale (, ReLU)] run on X: statistics at the BatchNorm, normalise + scale + bias + ReLU at the Scale; backward the two sums at BckScale and the
        data gradient at BckBatchNorm, in place on X_grad_loss.  The normalised value is recomputed from <X>_bn_in everywhere: nothing is saved twice.  On the running
        pair (Freeze.bn_global_stats): hip_bnf_prep, hip_bn_fwd as it is, and ONE backward call -- which one, the pruning rule says."""
        x, (bn, sc, relu) = self.bn_of_tag[o.src.tag]
        xd, t, nc, glob = self.bp.nodes[x], o.type, self.d.img_chunks, bn.tag in self.bn_global
        common = {"in": x + BN_IN_SFX, "mean": bn.tag + BN_MEAN_SFX, "inv_std": bn.tag + BN_ISTD_SFX}
        if t == "BatchNorm" and glob:
            return [(bnf_prep_func_op(xd, bn.eps), {"run_mean": bn.tag + "_mean", "run_var": bn.tag + "_var", "mean": common["mean"], "inv_std": common["inv_std"]})], []
        if t == "BatchNorm":
            fop = bnc_stats_func_op(xd, bn.eps, self.d.bn_maf, nc) if nc else bn_stats_func_op(xd, bn.eps, self.d.bn_maf)
            return [(fop, dict(common, run_mean=bn.tag + "_mean", run_var=bn.tag + "_var"))], []
        if t == "Scale":
            return [((bnc_fwd_func_op if nc else bn_fwd_func_op)(xd, 1 if relu is not None else 0), dict(common, scale=sc.tag + "_scale", bias=sc.tag + "_bias", out=x))], []
        bsc = self.by_tag_bck[sc.tag + "_bck"]
        sums = {"scale_grad_loss": bsc.tops[1], "bias_grad_loss": bsc.tops[2]}
        gl = {"out_grad_loss": o.bots[0], "in_grad_loss": o.tops[0]}
        in_need, sc_train = self.kept(o, 0), not glob or self.kept(bsc, 1)   # (a training run's sums are always computed: its data gradient reads them)
        if t == "BckScale" and glob and sc_train and in_need:      # the sums and dx in one pass, in place on X_grad_loss
            return [(bnf_bck_func_op(xd), dict(common, scale=sc.tag + "_scale", **sums, **gl))], []
        if t == "BckScale" and sc_train:     # (on the running pair: nothing below needs a gradient, the sums alone)
            return [(bnc_bck_sums_func_op(xd, nc) if nc else bn_bck_sums_func_op(xd), dict(common, out_grad_loss=o.bots[0], **sums))], []
        if t == "BckBatchNorm" and glob and not sc_train:   # behind a frozen Scale (with a trainable one hip_bnf_bck has written dx already)
            return [(bnf_bck_in_func_op(xd), dict(inv_std=common["inv_std"], scale=sc.tag + "_scale", **gl))], []
        if t == "BckBatchNorm" and not glob and in_need:
            return [((bnc_bck_in_func_op if nc else bn_bck_in_func_op)(xd), dict(common, scale=sc.tag + "_scale", **sums, **gl))], []
        return [], []

    BY_TYPE = {"Convolution": conv, "ReLU": relu, "BckConv": bck_conv, "Pooling": pool, "Spreading": spreading, "LRN": lrn, "BckLRN": bck_lrn,
               "ZeroIfNonPos": zero_if_non_pos, "SoftmaxWithLoss": loss, "Dropout": dropout, "BckDropout": dropout, "Reduce": reduce, "Eltwise": reduce, "Concat": concat,
               "Split": split, "BckEltwise": bck_eltwise, "BatchNorm": bn_run, "Scale": bn_run, "BckScale": bn_run, "BckBatchNorm": bn_run,
               "Deconvolution": deconv, "BckDeconv": bck_deconv, "Crop": crop, "BckCrop": bck_crop}


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
        self._general = isinstance(solver, Solver)   # a Solver: solver_hyper per step, `iter`, clipping and accumulation; an SgdSolver has sgd_hyper alone
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
        if iter_size > 1 and not self._general:
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
        self._stepped = False      # an ordinary step has run since init: every workspace and lazily built kernel exists
        self.call_deps: List[List[int]] = []
        self.fused_relu_grads: Dict[str, object] = {"folded": [], "unfolded": {}}
        self.bn_runs: Dict[str, tuple] = {}   # node X -> (BatchNorm op, Scale op, the ReLU behind them or None), as init planned them
        self._calls = CallList(rtc, "bck")    # the step's calls, their functions and the captured graph
        self.vars: List[str] = []
        self.per_call_ms: List[Tuple[str, str, float]] = []
        self.compute_dur_ms = 0.0

    def _var(self, vn: str, dims) -> None:
        if vn in self.vars:
            return
        if isinstance(dims, SideVar):   # a view of another var (its calls are ordered as calls on that var), or a constant
            if dims.view_of is not None:
                self.rtc.create_var_with_dims_as_reshaped_view_of_var(vn, dims.dims, dims.view_of); self._calls.alias[vn] = dims.view_of
            else:
                self.rtc.create_var_with_dims(vn, dims.dims); self.rtc.copy_nda_to_var(vn, np.full(dims.dims.sizes, dims.fill, np.float32))
        else:
            self.rtc.create_var_with_dims(vn, dims)
        self.vars.append(vn)

    bck_calls = property(lambda self: self._calls.calls)    # the step's BckCalls in run order
    funcs = property(lambda self: self._calls.funcs)
    _graph = property(lambda self: self._calls.graph)

    def init(self, bp: BckPipe, op_params: Optional[Dict[str, np.ndarray]] = None, gen_mode: int = 5) -> None:
        """Three stages.  PLAN (plan(): no backend call; every RtErr / UnsupErr of init comes from there, so a refused init has created nothing), CREATE (every var,
        every call, one compile), BIND (_bind: the params and the other uploads, once).  Without op_params the params are host_params(bp, gen_mode)."""
        p = self.plan(bp)
        self.bp, self._stepped = bp, False
        self.sgd_params, self.frozen, self.fused_relu_grads, self._dropped_vars, self.bn_runs = p.sgd_params, p.frozen, p.fused_relu_grads, p.dropped_vars, p.bn_runs
        for vn, d in p.vars:
            self._var(vn, d)
        for tag, fop, args in p.calls:
            self._calls.emit(tag, fop, args)
        self.n_sgd_calls = p.n_sgd_calls
        self._calls.compile()
        self._bind(p, op_params if op_params is not None else host_params(bp, gen_mode))

    def plan(self, bp: BckPipe) -> BckPlan:
        """Everything init decides, without one backend call: the checks of every option against the pipe and the backend, the planners (_plan_bn_runs, _plan_freeze,
        plan_relu_grad_folds), every op's lowering (_Lower) and the solver's calls (_plan_solver_tail)."""
        if not isinstance(bp, BckPipe):
            raise RtErr("ConvPipeBck.init: pass the pipe add_bck_ops returned")
        multi_dev = isinstance(getattr(self.rtc, "devices", None), list) and len(self.rtc.devices) > 1
        if self.seed_in_var and SEED_VAR in bp.nodes:
            raise RtErr(f"ConvPipeBck.init: seed_in_var=True needs the var name {SEED_VAR!r}, which is a node of the pipe")
        if self.grad_operands and multi_dev:
            raise UnsupErr("ConvPipeBck.init: grad_operands='bf16': the filter and bias gradients have their bf16-operand form as hip_bconv_filts_biases only, which sums over "
                           "the images into two outputs and is not provided on a multi-device backend (devices=...); leave the option off there")
        if self.fuse_filts_biases and multi_dev:
            raise UnsupErr("ConvPipeBck.init: fuse_filts_biases=True: hip_bconv_filts_biases sums over the images into two outputs and is not provided on a multi-device "
                           "backend (devices=...); leave the option off there")
        if self.img_chunks and multi_dev and self.img_chunks != len(self.rtc.devices):
            raise RtErr(f"ConvPipeBck.init: img_chunks={self.img_chunks} on {len(self.rtc.devices)} devices: chunk i of a BatchNorm's sums is device i's img shard, so img_chunks must "
                        "be the device count")
        grouped = [o for o in bp.fwd_ops() if o.type == "Convolution" and getattr(o.src, "group", 1) > 1]
        if grouped and self.grad_operands:
            raise UnsupErr(f"ConvPipeBck.init: grad_operands='bf16': the convolution {grouped[0].tag!r} has group={grouped[0].src.group}, and a grouped convolution's gradients "
                           "(hip_bconv_in_grp, hip_bconv_filts_grp) are fp32 only; leave the option off for a pipe with grouped layers")
        if grouped and multi_dev:
            raise UnsupErr(f"ConvPipeBck.init: the convolution {grouped[0].tag!r} has group={grouped[0].src.group}: the grouped functions take vars of exactly their op's dims, "
                           "not img shards, and are not provided on a multi-device backend (devices=...); grouped layers on several devices are out of scope")
        deconvs = [o for o in bp.fwd_ops() if o.type == "Deconvolution"]
        if deconvs and multi_dev:
            raise UnsupErr(f"ConvPipeBck.init: the layer {deconvs[0].tag!r} is a Deconvolution: its functions take vars of exactly their op's dims, not img shards, and are "
                           "not provided on a multi-device backend (devices=...); Deconvolution layers on several devices are out of scope")
        spec_heads = [o for o in bp.fwd_ops() if o.type == "SoftmaxWithLoss" and o.spec is not None]
        if spec_heads and multi_dev:
            raise UnsupErr(f"ConvPipeBck.init: the loss {spec_heads[0].tag!r} has a LossSpec: the full softmax loss (hip_softmax_loss_fwd, hip_loss_norm, hip_softmax_loss_bck) "
                           "counts the pels that are not ignored and sums over the WHOLE batch, which would need a cross-device reduction: not provided on a multi-device "
                           "backend (devices=...); leave loss_specs off there")
        for o in spec_heads:
            for vn in (o.tag + "_prob", o.tops[1] + "_per_pel", o.tops[1] + LOSS_STATE_SFX):
                if vn in bp.nodes:
                    raise RtErr(f"ConvPipeBck.init: the loss {o.tag!r} needs the var name {vn!r}, which is a node of the pipe")
        bn_runs = self._plan_bn_runs(bp)   # node X -> (BatchNorm op, Scale op, the ReLU behind them or None); every other shape of BatchNorm / Scale is refused here
        if bn_runs and multi_dev and not self.img_chunks:
            raise UnsupErr("ConvPipeBck.init: the pipe has a BatchNorm, whose batch statistics sum over the images of the WHOLE batch: not provided on a multi-device backend "
                           "(devices=...); statistics summed across img shards are out of scope")
        if multi_dev and not self.img_chunks and any(o.type == "BckEltwise" for o in bp.bck_ops()):
            raise UnsupErr("ConvPipeBck.init: the pipe has an Eltwise, whose gradient (hip_fan_out) takes vars of exactly its op's dims, not img shards: not provided on a "
                           "multi-device backend (devices=...)")
        stats = set(bn_stat_params(bp.cp))
        keep, bn_global, sgd_params, frozen, dropped = self._plan_freeze(bp, bn_runs, multi_dev, [pn for pn in bp.cp.params if pn not in stats])
        self._check_solver(bp, sgd_params)
        for x, (bn, sc, _) in bn_runs.items():
            for vn in (x + BN_IN_SFX, bn.tag + BN_MEAN_SFX, bn.tag + BN_ISTD_SFX):
                if vn in bp.nodes:
                    raise RtErr(f"ConvPipeBck.init: the BatchNorm on {x} needs the var name {vn!r}, which is a node of the pipe")
        xf_vars, calls, xf_mean = self._plan_input_transform(bp)
        vars = [(n, d) for n, d in bp.nodes.items() if n not in dropped] + xf_vars
        for x, (bn, sc, _) in bn_runs.items():
            vars += [(x + BN_IN_SFX, bp.nodes[x])] + [(bn.tag + sfx, bp.cp.params[bn.tag + "_mean"]) for sfx in (BN_MEAN_SFX, BN_ISTD_SFX)]
        if self.seed_in_var:
            vars.append((SEED_VAR, Dims(("v",), (1,), "uint32_t")))
        folds, why = plan_relu_grad_folds(bp) if self.fuse_relu_grad else ({}, {o.tag: "fuse_relu_grad is off" for o in bp.bck_ops() if o.type == "ZeroIfNonPos"})
        low = _Lower(self, bp, bn_runs, keep, bn_global, folds)
        for o in bp.ops:
            op_calls, side_vars = low.lower(o)
            calls += [(o.tag, fop, args) for fop, args in op_calls]; vars += side_vars
        sv_vars, sv_calls = self._plan_solver_tail(bp, sgd_params)   # behind every gradient op
        return BckPlan(vars + sv_vars, calls + sv_calls, len(sv_calls), sgd_params, frozen, {"folded": list(folds), "unfolded": why}, dropped, bn_runs, xf_mean)

    def _check_solver(self, bp: BckPipe, sgd_params: List[str]) -> None:
        sv, gen = self.solver, self._general
        if sv is None:
            return
        if not 1 <= int(sv.tensors_per_call) <= SGD_MAX_TENS:
            raise RtErr(f"ConvPipeBck.init: SgdSolver.tensors_per_call={sv.tensors_per_call}: 1 to {SGD_MAX_TENS}")
        if not gen and not isinstance(sv, SgdSolver):
            raise RtErr(f"ConvPipeBck.init: solver must be an SgdSolver or a Solver, got {type(sv).__name__}")
        if gen:
            if sv.type not in ("sgd", "nesterov", "adam"):
                raise RtErr(f"ConvPipeBck.init: Solver.type must be sgd | nesterov | adam, got {sv.type!r}")
            if sv.decoupled_wd and sv.type != "adam":
                raise RtErr(f"ConvPipeBck.init: Solver.decoupled_wd is adam's, not {sv.type}'s")
            if not float(sv.clip_gradients) >= 0.0:
                raise RtErr(f"ConvPipeBck.init: Solver.clip_gradients={sv.clip_gradients!r}: 0 (off) or a positive norm")
            if sv.lr_policy is not None and not isinstance(sv.lr_policy, LrPolicy):
                raise RtErr("ConvPipeBck.init: Solver.lr_policy must be an LrPolicy or None")
        names = [SGD_HYPER_VAR] if not gen else [SOLVER_HYPER_VAR, SOLVER_STATE_VAR] + ([SOLVER_PARTS_VAR] if sv.clip_gradients > 0 else []) + \
            ([pn + SGD_HIST2_SFX for pn in sgd_params] if sv.type == "adam" else [])
        if self.iter_size > 1:
            names += [SOLVER_ACCUM_VAR] + [pn + GRAD_ACC_SFX for pn in sgd_params]
        for vn in [pn + SGD_HIST_SFX for pn in sgd_params] + names:
            if vn in bp.nodes:
                raise RtErr(f"ConvPipeBck.init: the solver needs the var name {vn!r}, which is a node of the pipe")
        for pn in sgd_params:
            if pn + "_grad_loss" not in bp.nodes:
                raise RtErr(f"ConvPipeBck.init: the solver: no gradient op writes {pn + '_grad_loss'!r}")

    def _plan_input_transform(self, bp: BckPipe):
        """-> (the three vars, [the data_xf call, in front of the step's first: the input node from the bytes], the mean to upload); ([], [], None) without one."""
        xf = self.input_transform
        if xf is None:
            return [], [], None
        dn = bp.cp.in_node; dd = bp.nodes[dn]
        if dd.tn != "float" or dd.names != ("img", "chan", "y", "x") or (dd.dsz("y"), dd.dsz("x")) != (xf.ch, xf.cw):
            raise RtErr(f"ConvPipeBck.init: input_transform crops to {xf.ch} x {xf.cw}: the pipe's input node {dn!r} must be float img:chan:y={xf.ch}:x={xf.cw}, got {dd.tn} {dd.pretty()}")
        for vn in (DATA_RAW_VAR, DATA_XF_PLAN_VAR, DATA_XF_MEAN_VAR):
            if vn in bp.nodes:
                raise RtErr(f"ConvPipeBck.init: input_transform needs the var name {vn!r}, which is a node of the pipe")
        xf_mean = xf.mean_array(dd.dsz("chan"))
        src, mean = xf.src_dims(dd.dsz("img"), dd.dsz("chan")), xf.mean_dims(dd.dsz("chan"))
        vars = [(DATA_RAW_VAR, src), (DATA_XF_PLAN_VAR, Dims(("img", "v"), (dd.dsz("img"), 4), "uint32_t")), (DATA_XF_MEAN_VAR, mean)]
        call = (DATA_XF_TAG, data_transform_func_op(src, (xf.ch, xf.cw), mean, xf.scale), {"src": DATA_RAW_VAR, "plan": DATA_XF_PLAN_VAR, "mean": DATA_XF_MEAN_VAR, "out": dn})
        return vars, [call], xf_mean

    def _plan_solver_tail(self, bp: BckPipe, pnames: List[str]):
        """The solver's vars and calls, all behind every gradient op, as the class docstring lists them for an SgdSolver, a Solver and iter_size > 1
        -> ([(var, Dims)], [(tag, function op, {arg: var})]); tensors_per_call params per call in the order of the pipe's params."""
        sv, gen, P = self.solver, self._general, bp.cp.params
        if sv is None:
            return [], []
        adam, clip, acc = gen and sv.type == "adam", gen and sv.clip_gradients > 0, self.iter_size > 1
        hyper, v4 = SOLVER_HYPER_VAR if gen else SGD_HYPER_VAR, Dims(("v",), (4,), "float")
        vars = [(pn + sfx, P[pn]) for pn in pnames for sfx in ((SGD_HIST_SFX, SGD_HIST2_SFX) if adam else (SGD_HIST_SFX,))]
        vars += [(hyper, Dims(("v",), (8,), "float")), (SOLVER_STATE_VAR, v4)] if gen else [(hyper, v4)]
        per = int(sv.tensors_per_call)
        groups = [pnames[k:k + per] for k in range(0, len(pnames), per)]
        gsfx = GRAD_ACC_SFX if acc else "_grad_loss"   # what the norm and the update read: the accumulators, or the step's own gradients
        calls = []
        if acc:   # the accumulate calls in front of the norm and the update
            vars += [(pn + GRAD_ACC_SFX, P[pn]) for pn in pnames] + [(SOLVER_ACCUM_VAR, v4)]
            for k, grp in enumerate(groups):
                args = {"accum": SOLVER_ACCUM_VAR}
                for i, pn in enumerate(grp):
                    args.update({f"g_{i}": pn + "_grad_loss", f"a_{i}": pn + GRAD_ACC_SFX})
                calls.append((f"grad_accum_{k}", grad_accum_func_op([P[pn] for pn in grp]), args))
        if clip:
            parts = sum(-(-P[pn].dims_prod() // SOLVER_CHUNK) for pn in pnames)
            vars.append((SOLVER_PARTS_VAR, Dims(("v",), (parts,), "float")))
            part0 = 0
            for k, grp in enumerate(groups):
                fop = grad_sumsq_func_op([P[pn] for pn in grp], part0, parts)
                calls.append((f"grad_sumsq_{k}", fop, dict({f"g_{i}": pn + gsfx for i, pn in enumerate(grp)}, partials=SOLVER_PARTS_VAR)))
                part0 += fop.solver_geom()["chunks"]
            calls.append(("grad_norm", grad_norm_func_op(parts), {"partials": SOLVER_PARTS_VAR, "hyper": SOLVER_HYPER_VAR, "state": SOLVER_STATE_VAR}))
        for k, grp in enumerate(groups):
            dims, lr_mult, decay_mult = [P[pn] for pn in grp], [sv.mult_of(sv.lr_mult, pn) for pn in grp], [sv.mult_of(sv.decay_mult, pn) for pn in grp]
            if gen:
                fop = (solver_update_acc_func_op if acc else solver_update_func_op)(dims, sv.type, lr_mult, decay_mult, clip=clip, decoupled_wd=sv.decoupled_wd)
            else:
                fop = sgd_update_func_op(dims, lr_mult, decay_mult)
            args = dict({"hyper": hyper}, **({"state": SOLVER_STATE_VAR} if gen else {}), **({"accum": SOLVER_ACCUM_VAR} if acc else {}))
            for i, pn in enumerate(grp):
                args.update({f"w_{i}": pn, f"g_{i}": pn + gsfx, f"h_{i}": pn + SGD_HIST_SFX}, **({f"h2_{i}": pn + SGD_HIST2_SFX} if adam else {}))
            calls.append((f"{'solver' if gen else 'sgd'}_update_{k}", fop, args))
        return vars, calls

    def _bind(self, p: BckPlan, params: Dict[str, np.ndarray]) -> None:
        """The uploads behind the one compile: the params, the input transform's mean and a first plan, each dropout layer's offset, the seed, the solver's state."""
        rtc, bp, xf = self.rtc, self.bp, self.input_transform
        for n, d in bp.cp.params.items():
            if n not in params:
                raise RtErr(f"ConvPipeBck.init: no value for param {n!r}")
            rtc.copy_nda_to_var(n, np.ascontiguousarray(params[n], np.float32).reshape(d.sizes))
        if xf is not None:   # the mean once; a valid plan, so that a pass capture_graph runs on its own reads inside data_raw
            rtc.copy_nda_to_var(DATA_XF_MEAN_VAR, p.xf_mean)
            self.xf_images = 0; self._input_plan = None
            rtc.copy_nda_to_var(DATA_XF_PLAN_VAR, xf.plan("train", 0, self._xf_batch()))
        if self.seed_in_var:   # each layer's fixed offset, by value, once: from here on a new seed is four bytes into the var
            for c, k in self._dropout_calls():
                c.rfc.arg_map["det_drop_seed"] = RtcArg.scalar((k * DROP_LAYER_STEP) & 0xFFFFFFFF, "uint32_t")
        self.set_det_drop_seed(0)
        if self.solver is not None:
            self._sgd_hyper = self.solver.hyper()
            self.zero_sgd_history()
            if self._general:
                self.rtc.copy_nda_to_var(SOLVER_STATE_VAR, np.array([1.0, 0.0, 0.0, 0.0], np.float32))
                if self.iter_size > 1:
                    self.rtc.copy_nda_to_var(SOLVER_ACCUM_VAR, self.accum_words())
            self.set_sgd_hyper()

    def _plan_freeze(self, bp: BckPipe, bn_runs: Dict[str, tuple], multi_dev: bool, cand: List[str]):
        """Freeze's rule on the pipe; cand: every param but the BatchNorm running statistics, in the pipe's order.  -> ({gradient op tag: [is its i-th top still
        written]}, the set of BatchNorm tags on their running pair, the trainable params, what `frozen` reports, the gradient vars the rule leaves out); without freeze=
        (None, empty set, cand, an empty report, empty set)."""
        fz = self.freeze
        if fz is None:
            return None, set(), cand, {"params": [], "dropped_calls": [], "bn_global": []}, set()
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
            if b.type in ("BckConv", "BckDeconv", "BckScale"):
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
        report = {"params": [pn for pn in cand if pn in frozen], "dropped_calls": [b.tag for b in bp.bck_ops() if not any(keep[b.tag])],
                  "bn_global": [tg for tg in bn_tags if tg in bn_global]}
        return keep, set(bn_global), trainable, report, {tp for b in bp.bck_ops() for tp in b.tops} - written

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
        gen = self._general
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

    def _before_update_step(self) -> None:
        """What is uploaded before every pass that runs all calls, eager or a replay: the input transform's plan, a Solver's hyper words and accumulate words."""
        xf = self.input_transform
        if xf is not None:
            B = self._xf_batch()
            plan = self._input_plan if self._input_plan is not None else xf.plan("train", self.xf_images, B)
            self.rtc.copy_nda_to_var(DATA_XF_PLAN_VAR, xf.check_plan(plan, B))
        if self._general:
            self._upload_solver_hyper()
            if self.iter_size > 1:
                self.rtc.copy_nda_to_var(SOLVER_ACCUM_VAR, self.accum_words())

    def _after_update_step(self) -> None:
        if self.input_transform is not None:
            self.xf_images += self._xf_batch()
            self._input_plan = None
        if self._general:
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
        adam = self._general and self.solver.type == "adam"
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
        if not skip_sgd:
            self._before_update_step()
        self.compute_dur_ms, self.per_call_ms = self._calls.run(all_but_last=self.n_sgd_calls if skip_sgd else 0)
        if not skip_sgd:
            self._after_update_step()
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
        self._calls.destroy_graph()
        if not self._stepped:   # (without the update calls: a capture leaves params and history as they were; their kernel was built when they were compiled)
            stats = {vn: rtc.copy_var_to_nda(vn) for vn in bn_stat_params(self.bp.cp)}   # (a forward pass moves a BatchNorm's running pair: put back below)
            self.run_device_only(skip_sgd=True)
            for vn, a in stats.items():
                rtc.copy_nda_to_var(vn, a)
        n = self._calls.capture(deps)
        if parallel:
            self.call_deps = deps
        return n

    def _call_deps(self) -> List[List[int]]:
        """deps[i] = the earlier calls of the step that call i must run after (CallList.deps states the rule)."""
        return self._calls.deps()

    def run_graph(self) -> float:
        """One step as one graph launch; -> ms of the whole replay.  A replay has no per-call times: per_call_ms is []."""
        if self._graph is None:
            raise RtErr("ConvPipeBck.run_graph: no captured graph -- call capture_graph() first")
        self._before_update_step()
        self.compute_dur_ms, self.per_call_ms = self._calls.replay(), []
        self._after_update_step()
        return self.compute_dur_ms

    def release(self) -> None:
        self._calls.release()
        for v in reversed(self.vars):   # (a view goes before the var it is a view of)
            self.rtc.release_var(v)
        self.vars = []
        self.n_sgd_calls = 0
        self._stepped = False
