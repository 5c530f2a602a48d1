"""The evaluation pass of the gradient pipe: `EvalPipe`, a TEST-phase forward pass over the vars a ConvPipeBck trains, with top-1 / top-k accuracy and the mean loss
accumulated on the device (csrc/kernels/eval_f32.hip: hip_accuracy, hip_eval_accum, hip_bn_fold).

The reference names an Accuracy op type (src/conv_util.cc:51, AccuracyParameter in src/ext/caffe.proto) and runs none; the rules here are Caffe's accuracy layer's, with the
two departures kernels/eval_f32.hip states (a NaN score counts against the true class; an invalid label is a miss, not an error)."""
from __future__ import annotations
from typing import Callable, Dict, List, Optional, Tuple

import numpy as np

from .bck_pipe import BN_IN_SFX, BckCall, ConvPipeBck
from .call_list import CallList
from .cnn_op import accuracy_func_op, bn_fold_func_op, chan_affine_func_op, eval_accum_func_op
from .input_pipe import DATA_RAW_VAR, DATA_XF_PLAN_VAR, DATA_XF_TAG
from .op import Dims, Op, RtErr, UnsupErr
from .rtc import RtcArg

EVAL_CTL_VAR = "eval_ctl"            # uint32 v=4 = [first, 0, 0, 0], uploaded before every batch
EVAL_COUNTS_VAR = "eval_counts"      # uint32 v=4 = [images, hits_top1, hits_topk, batches]
EVAL_LOSS_SUM_VAR = "eval_loss_sum"  # float v=1: the sum of the batches' losses
EVAL_RANK_VAR = "eval_rank"          # uint32 img: the rank of the true class per image of the last batch
EVAL_A_SFX, EVAL_B_SFX = "_eval_a", "_eval_b"   # <bn-tag>_eval_a / _eval_b: a [BatchNorm, Scale] run's running statistics folded into out = in * a + b


class EvalPipe:
    """ev = EvalPipe(drv, top_k=5, loss=None) -- drv an initialised ConvPipeBck on one device (be=hip or be=cpu); loss the SoftmaxWithLoss top to score (default: the
    pipe's last).  run_batch(feed) uploads feed's vars (data, label), runs one TEST-phase forward pass and adds the batch to the accumulators; evaluate(n, feed) resets
    and runs n batches of feed(i); result() fetches 20 bytes and forms the quotients in float64 on the host.

    The call list is built from the driver's forward calls -- the calls in front of its first gradient op -- in the driver's order, reusing the driver's compiled
    functions and arg bindings wherever the op is unchanged (no convolution, pooling or LRN is compiled twice):
      * Dropout: no call.  The training dropout scales the kept elements, so the test phase is the identity.
      * BatchNorm of a [BatchNorm, Scale (, ReLU)] run on X: hip_bn_fold of the RUNNING pair <bn>_mean / <bn>_var and <scale>_scale / _bias into <bn>_eval_a / _eval_b
        (the bits of conv_pipe.fold_affine); the Scale is then hip_chan_affine from <X>_bn_in to X, ReLU included.  The same for a driver built with img_chunks, which
        has no meaning in the test phase.
      * the selected SoftmaxWithLoss with a LossSpec (1 x 1 plane, no ignore_label; anything else is an UnsupErr here): hip_softmax_loss_fwd and hip_loss_norm, then
        hip_accuracy and hip_eval_accum as below; its gradient call is left out.
      * the selected SoftmaxWithLoss: the driver's three calls, then hip_accuracy on the loss's `in` node (the logits) and `label` into eval_rank, then hip_eval_accum
        into eval_counts / eval_loss_sum.  The loss calls of other heads are left out.
      * the data_xf call of a driver built with input_transform: the driver's own call, first; run_batch({"data_raw": bytes, "label": y}).
      * everything else: the driver's own call.
    Before every batch, eager or replay, the 16 bytes of eval_ctl are uploaded: [1, 0, 0, 0] on the first batch after reset(), [0, 0, 0, 0] afterwards.  hip_eval_accum
    reads the word from device memory, so nobody clears an accumulator and one captured graph serves every batch.  capture_graph() captures the list serially into a
    graph of its own, beside the driver's; capturing either one does not destroy the other.

    WHAT A PASS MAY WRITE.  A pass writes the activation nodes and their side vars (<X>_bn_in, <out>_in_yx, <out>_scale_base, <loss>_prob, <loss>_per_pel, the loss node
    and the logits' _grad_loss, which the loss function writes) and the vars named above (eval_ctl, eval_rank, eval_counts, eval_loss_sum, <bn>_eval_a / _eval_b) and, on a driver built
    with input_transform, data_xf_plan (the TEST plan, uploaded beside eval_ctl; the driver uploads its own again before its next pass) and the fed data_raw.  A pass
    NEVER writes a param, a BatchNorm's running or batch statistics, a history, a _grad_acc, any other gradient, a solver var, det_drop_seed, drv.iter or drv.micro: a
    training run with evaluations in between leaves the bits of the same run without them.

    On a multi-device backend (devices=...) the constructor raises UnsupErr before creating anything: the batch's counts would need a cross-device sum."""

    def __init__(self, drv: ConvPipeBck, top_k: int = 5, loss: Optional[str] = None):
        if not isinstance(drv, ConvPipeBck) or not drv.bck_calls:
            raise RtErr("EvalPipe: pass an initialised ConvPipeBck (init() creates the vars and calls the evaluation pass reuses)")
        rtc, bp = drv.rtc, drv.bp
        if isinstance(getattr(rtc, "devices", None), list):
            raise UnsupErr("EvalPipe: not provided on a multi-device backend (devices=...): hip_eval_accum counts the hits of the vars it is given, and the counts of a "
                           "batch sharded on img would need a cross-device sum; evaluate on one device")
        if not isinstance(top_k, int) or isinstance(top_k, bool) or top_k < 1:
            raise RtErr(f"EvalPipe: top_k must be an int >= 1, got {top_k!r}")
        loss = bp.loss_nodes[-1] if loss is None else loss
        if loss not in bp.loss_nodes:
            raise RtErr(f"EvalPipe: loss={loss!r} is no SoftmaxWithLoss top of the pipe ({', '.join(bp.loss_nodes)})")
        self.drv, self.rtc, self.top_k, self.loss = drv, rtc, top_k, loss
        fwd_ops = {o.tag: o for o in bp.fwd_ops()}
        fwd_calls = []
        self.xf_call: Optional[BckCall] = None
        for c in drv.bck_calls:   # the calls in front of the first gradient op -- behind the input transform's call, where the driver has one: reused as it is
            if c.tag == DATA_XF_TAG and drv.input_transform is not None and not fwd_calls and self.xf_call is None:
                self.xf_call = c
                continue
            if c.tag not in fwd_ops:
                break
            fwd_calls.append(c)
        bn_runs = drv.bn_runs   # (as the driver's init planned them)
        bn_of_tag = {q.tag: (x, run) for x, run in bn_runs.items() for q in run[:2]}
        lop = fwd_ops[loss]
        logits, label = lop.bots
        if lop.spec is not None and (bp.nodes[label].sizes[1:] != (1, 1) or lop.spec.ignore_label is not None):
            raise UnsupErr(f"EvalPipe: the loss {loss!r} " + ("has a plane larger than 1 x 1" if bp.nodes[label].sizes[1:] != (1, 1) else f"has ignore_label={lop.spec.ignore_label}") +
                           ": accuracy over a plane or with an ignore_label is not built (hip_accuracy ranks one label per image and counts every image)")
        n_img = bp.nodes[logits].dsz("img")
        new_vars: Dict[str, Dims] = {EVAL_CTL_VAR: Dims(("v",), (4,), "uint32_t"), EVAL_COUNTS_VAR: Dims(("v",), (4,), "uint32_t"),
                                     EVAL_LOSS_SUM_VAR: Dims(("v",), (1,), "float"), EVAL_RANK_VAR: Dims(("img",), (n_img,), "uint32_t")}
        for x, (bn, sc, _) in bn_runs.items():
            for sfx in (EVAL_A_SFX, EVAL_B_SFX):
                new_vars[bn.tag + sfx] = bp.cp.params[bn.tag + "_mean"]
        for vn in new_vars:   # (before anything is created)
            if vn in bp.nodes or vn in drv.vars:
                raise RtErr(f"EvalPipe: the evaluation pass needs the var name {vn!r}, which is a {'node of the pipe' if vn in bp.nodes else 'var of the driver'}")
        self.vars: List[str] = []
        self._calls = CallList(rtc, "eval")   # the batch's calls, the functions made for it and its own graph
        self._stepped = False
        self._first = True
        self._batches = 0   # since reset()
        self.per_call_ms: List[Tuple[str, str, float]] = []
        self.compute_dur_ms = 0.0
        emit = self._calls.emit
        if self.xf_call is not None:
            self._calls.reuse(self.xf_call)
        for c in fwd_calls:
            o = fwd_ops[c.tag]
            if o.type == "Dropout":
                continue
            if o.type == "BatchNorm":
                x, (bn, sc, relu) = bn_of_tag[o.src.tag]
                emit(o.tag, bn_fold_func_op(bp.nodes[x].dsz("chan"), bn.eps), {"run_mean": bn.tag + "_mean", "run_var": bn.tag + "_var", "scale": sc.tag + "_scale", "bias": sc.tag + "_bias",
                                                                               "a": bn.tag + EVAL_A_SFX, "b": bn.tag + EVAL_B_SFX})
                continue
            if o.type == "Scale":
                x, (bn, sc, relu) = bn_of_tag[o.src.tag]
                emit(o.tag, chan_affine_func_op(bp.nodes[x], 1 if relu is not None else 0), {"in": x + BN_IN_SFX, "a": bn.tag + EVAL_A_SFX, "b": bn.tag + EVAL_B_SFX, "out": x})
                continue
            if o.type == "SoftmaxWithLoss" and o.tag != loss:
                continue
            if o.type == "SoftmaxWithLoss" and c.fop.get_func_name() == "hip_softmax_loss_bck":
                continue   # (a head with a LossSpec: the gradient call of the full loss is behind the loss node's; an evaluation pass needs no gradient)
            self._calls.reuse(c)   # the driver's own function and bindings
            if o.type == "SoftmaxWithLoss" and c.fop.get_func_name() in ("hip_sum_loss_over_imgs", "hip_loss_norm"):
                emit(o.tag, accuracy_func_op(bp.nodes[logits]), {"in": logits, "label": label, "rank": EVAL_RANK_VAR})
                emit(o.tag, eval_accum_func_op(n_img, top_k), {"rank": EVAL_RANK_VAR, "loss": loss, "ctl": EVAL_CTL_VAR, "counts": EVAL_COUNTS_VAR, "loss_sum": EVAL_LOSS_SUM_VAR})
        if not self.funcs or self.eval_calls[-1].fop.get_func_name() != "hip_eval_accum":
            raise RtErr(f"EvalPipe: the driver's forward calls hold no loss calls of {loss!r}")
        for vn, d in new_vars.items():
            rtc.create_var_with_dims(vn, d); self.vars.append(vn)
        try:
            self._calls.compile()
        except Exception:
            for vn in self.vars:
                rtc.release_var(vn)
            self.vars = []
            raise

    # -- the accumulators
    def reset(self) -> None:
        """The next batch starts the sums anew: its ctl word says `first`, and hip_eval_accum then overwrites the accumulators without reading them.  Touches no var."""
        self._first = True
        self._batches = 0

    def _ctl_words(self) -> np.ndarray:
        return np.array([1 if self._first else 0, 0, 0, 0], np.uint32)

    def _upload_ctl(self) -> None:
        """What is uploaded before every batch: eval_ctl and, on a driver with an input transform, the TEST plan (the centre crop, no mirror) into data_xf_plan --
        which the driver uploads again before its next pass.  drv.xf_images is not advanced."""
        self.rtc.copy_nda_to_var(EVAL_CTL_VAR, self._ctl_words())
        xf = self.drv.input_transform
        if xf is not None:
            self.rtc.copy_nda_to_var(DATA_XF_PLAN_VAR, xf.plan("test", 0, self.drv._xf_batch()))

    eval_calls = property(lambda self: self._calls.calls)   # the batch's BckCalls in run order
    funcs = property(lambda self: self._calls.funcs)
    _graph = property(lambda self: self._calls.graph)

    def calls(self) -> List[Tuple[str, Op, Dict[str, RtcArg]]]:
        """The ordered (tag, function op, arg map) list of one evaluation batch."""
        return [(c.tag, c.fop, dict(c.rfc.arg_map)) for c in self.eval_calls]

    def run_device_only(self, graph: bool = False) -> float:
        """One evaluation batch on the inputs already resident; -> ms of the pass.  per_call_ms: (tag, function, ms) per call of an eager batch, [] for a replay."""
        if graph and self._graph is None:
            raise RtErr("EvalPipe.run_batch(graph=True): no captured graph -- call capture_graph() first")
        self._upload_ctl()
        if graph:
            self.compute_dur_ms, self.per_call_ms = self._calls.replay(), []
        else:
            self.compute_dur_ms, self.per_call_ms = self._calls.run()
            self._stepped = True
        self._first = False
        self._batches += 1
        return self.compute_dur_ms

    def run_batch(self, feed: Dict[str, np.ndarray], graph: bool = False) -> None:
        """Upload feed's vars ({"data": x, "label": y}), run one TEST-phase forward pass and add the batch to the accumulators.  graph=True: the pass is one replay of
        the graph capture_graph made."""
        if graph and self._graph is None:
            raise RtErr("EvalPipe.run_batch(graph=True): no captured graph -- call capture_graph() first")
        if self.xf_call is not None and self.drv.bp.cp.in_node in feed:
            raise RtErr(f"EvalPipe.run_batch: the driver was built with an input_transform: its {DATA_XF_TAG} call would overwrite {self.drv.bp.cp.in_node!r}; feed {DATA_RAW_VAR!r} (uint8)")
        for vn, a in feed.items():
            self.rtc.copy_nda_to_var(vn, a)
        self.rtc.finish_and_sync()
        self.run_device_only(graph=graph)

    def evaluate(self, n_batches: int, feed: Callable[[int], Dict[str, np.ndarray]], graph: bool = False) -> dict:
        """reset(), then n_batches of run_batch(feed(i)); -> result()."""
        self.reset()
        for i in range(int(n_batches)):
            self.run_batch(feed(i), graph=graph)
        return self.result()

    def result(self) -> dict:
        """{"images", "batches", "hits_top1", "hits_topk", "top1", "topk", "loss"} of the batches since reset(): the counts as the device holds them, the quotients
        hits / images and loss_sum / batches formed in float64 on the host.  No batch since reset(): zero counts and NaN quotients."""
        if not self._batches:
            return {"images": 0, "batches": 0, "hits_top1": 0, "hits_topk": 0, "top1": float("nan"), "topk": float("nan"), "loss": float("nan")}
        c = self.rtc.copy_var_to_nda(EVAL_COUNTS_VAR).reshape(-1)
        ls = self.rtc.copy_var_to_nda(EVAL_LOSS_SUM_VAR).reshape(-1)
        images, h1, hk, batches = (int(v) for v in c)
        return {"images": images, "batches": batches, "hits_top1": h1, "hits_topk": hk, "top1": h1 / images if images else float("nan"),
                "topk": hk / images if images else float("nan"), "loss": float(np.float64(ls[0]) / np.float64(batches)) if batches else float("nan")}

    # -- hipGraph form
    def capture_graph(self) -> int:
        """Capture the evaluation batch's call list, serially, into a hipGraph of its own; -> number of captured calls.  If no eager batch has run yet, one runs first on
        whatever the vars hold (workspaces and lazily built kernels must exist before a capture); the accumulators are put back behind it.  A second capture destroys
        the first; the driver's graph is not touched."""
        rtc = self.rtc
        self._calls.destroy_graph()
        if not self._stepped:
            keep = {vn: rtc.copy_var_to_nda(vn) for vn in (EVAL_COUNTS_VAR, EVAL_LOSS_SUM_VAR)}
            self._upload_ctl()
            self.compute_dur_ms, self.per_call_ms = self._calls.run()
            self._stepped = True
            for vn, a in keep.items():
                rtc.copy_nda_to_var(vn, a)
        return self._calls.capture()

    def release(self) -> None:
        """Destroy the graph, release the functions and vars this object made.  The driver, its functions, vars and graph stay as they are."""
        self._calls.release()
        for v in self.vars:
            self.rtc.release_var(v)
        self.vars = []
        self._stepped = False
