"""What a ConvPipeBck is configured with, as plain data: the solvers (SgdSolver, Solver with its LrPolicy), fine-tuning (Freeze) and the names of the vars they add.
Nothing here touches a backend; boda_amd/bck_pipe.py reads these, boda_amd/prototxt.py makes them from Caffe's text forms."""
from __future__ import annotations
from dataclasses import dataclass
from typing import Dict, Optional, Sequence

import numpy as np

from .op import RtErr

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
