"""Times the full-net gradient step (boda_amd/bck_pipe.py: forward, softmax loss and every gradient, one call per native function, unfused) on be=hip: NiN and
AlexNet at 256 images, the batch of tools/bck_conv_bench.py.  Per net one JSON line with the whole-step time (median of --runs steps after --warmup), images/s
and the share of the step each native function takes (sums of the backend's per-call durations).  No target is set: the first record is the baseline.

    python tools/bck_pipe_bench.py [--nets nin,alexnet] [--batch 256] [--runs 5] [--warmup 2] [--out profiles/r09_bck_pipe_bench.txt]
    python tools/bck_pipe_bench.py --fuse-relu-grad [--repeats 3] [--out profiles/r09_bck_fuse_ab.txt]
    python tools/bck_pipe_bench.py --fuse-filts-biases --nets resnet50 --batch 32 [--repeats 3] [--limit 900] [--out profiles/r15_resnet50_step_fb.txt]
    python tools/bck_pipe_bench.py --graph [--repeats 3] [--out profiles/r10_bck_graph_ab.txt]
    python tools/bck_pipe_bench.py --devices 0:1:2:3 [--out profiles/bck_pipe_devices.txt]
    python tools/bck_pipe_bench.py --sgd [--repeats 3] [--out profiles/r13_sgd_update.txt]
    python tools/bck_pipe_bench.py --nets resnet50 --batch 32 [--limit 900] [--out profiles/r14_resnet50_step.txt]
    python tools/bck_pipe_bench.py --grad-operands bf16 --nets resnet50 --batch 32 [--repeats 3] [--limit 900] [--out profiles/r16_step_bf16.txt]
    python tools/bck_pipe_bench.py --eval 8 [--nets nin,alexnet] [--repeats 3] [--out profiles/r20_eval.txt]
    python tools/bck_pipe_bench.py --img-chunks 2 --nets resnet50 --batch 32 [--devices 0:0] [--repeats 3] [--limit 900] [--out profiles/r17_resnet50_chunks.txt]

--fuse-relu-grad: the same step both ways in ONE process -- ConvPipeBck() and ConvPipeBck(fuse_relu_grad=True), each on a backend instance of its own with the same
params and inputs -- after the usual warm-up, in --repeats alternating blocks of --runs steps.  Per net two JSON lines ("way": "unfused" / "fused": step ms as the median
over all blocks, the medians of the single blocks (their spread is the run-to-run spread a difference has to beat), images/s, the call count, the per-function share)
and a third with the launches removed and the fused / unfused ratio.  The comparison is between the two ways of one run, never against a recorded figure.

--fuse-filts-biases: the same A/B for ConvPipeBck(fuse_filts_biases=True): every BckConv's hip_bconv_biases + hip_bconv_filts pair as one hip_bconv_filts_biases call
(DESIGN.md section 3.11).  The losses need not have the same bits: nothing the loss depends on changes, and they do; the gradients follow other chains.

--grad-operands bf16: the same construction for ConvPipeBck(grad_operands="bf16").  Three ways in ONE process, each on a backend instance of
its own with the same params and inputs, in alternating blocks: "f32" (the default step), "f32_fused" (fuse_filts_biases=True: the fp32 step with the same call list as
the bf16 one) and "bf16".  Per net one JSON line per way, with the loss of each, and one with the two quotients of the same run.  The losses agree in every bit (nothing
the loss depends on changes); no quotient is required.

--graph: the same construction for the step as one hipGraph replay.  Three ways in ONE process, each a ConvPipeBck(seed_in_var=True) on a backend instance of its own
with the same params and inputs: "eager" (run_device_only), "graph" (capture_graph(), run_graph) and "graph_parallel" (capture_graph(parallel=True): the calls' true
dependencies instead of the launch order).  The seed advances per step in all three (four bytes into the det_drop_seed var).  Per net one JSON line per way (step ms as
the median over all blocks, the block medians, images/s, the captured call count) and one with the two ratios against the eager step of the same run and whether all
three ended with the same loss bits.  No ratio is required: the spread of the block medians is what a difference has to beat.

--sgd: the same construction for the step that also updates its params (ConvPipeBck(solver=SgdSolver(...)), hip_sgd_update).  Three ways in ONE process, each on a backend
instance of its own with the same params and inputs: "no_solver" (the step as it was), "sgd_packed" (the update as multi-tensor calls, tensors_per_call=32) and
"sgd_per_tensor" (tensors_per_call=1: one launch per param tensor).  Per net one JSON line per way (step ms as the median over all blocks, the block medians, images/s,
the call count; for the two solver ways the update calls alone: how many, their summed microseconds per step, and GB/s = algo_bytes / that time, algo_bytes = 20 bytes
per param element) and one with the ratios of the same run.  The copy rate profiles/ records for this device is 6.29 TB/s.  The comparison that decides the default of
tensors_per_call is sgd_packed against sgd_per_tensor in the same run; no figure is required.

--solver sgd|nesterov|adam [--clip X]: beside --sgd, the step with ConvPipeBck(solver=Solver(type=..., clip_gradients=X)) (hip_solver_update; with X > 0 also the
hip_grad_sumsq calls and hip_grad_norm) against the step with hip_sgd_update, in alternating blocks in ONE process.  Per way one JSON line: step ms, block medians and,
per update function, the median us of its calls per step, the bytes they move (20 B per element for sgd / nesterov, 28 for adam, 4 for the sum of squares) and GB/s.
--swap builds and runs the Solver leg first (which of the process's two backends allocates first is then the other one); --solver sgd runs hip_sgd_update's chain in the new
kernel.  Several invocations go to one file by hand (profiles/r18_solver.txt); no figure is required.
--iter-size N (with --solver): the two legs are the Solver's step with iter_size=1 and with iter_size=N of the same build: every pass then runs
hip_grad_accum (12 B per element) and, when clipping, the norm over the accumulators; hip_solver_update_acc's us and GB/s are those of the passes that apply
(us_not_applying: the others).  --runs should be a multiple of N.  Written to profiles/r19_grad_accum.txt.

--eval N: the training step (hip_sgd_update) and the evaluation pass of eval_pipe.EvalPipe(top_k=5) over the SAME vars, in ONE process: --repeats
alternating blocks of --runs training steps and N eval batches, all eager.  Per net one JSON line: ms per training step and ms per eval batch (medians over all blocks,
and the block medians), their quotient, the call counts, the us per batch of hip_accuracy, hip_eval_accum and (summed over its calls) hip_bn_fold, and the last block's
result().  Written to profiles/r20_eval.txt.  No figure is required.

--devices d0:d1:...: the plain step on the multi-device backend `(be=hip,devices=...)`: the batch sharded on img, the five functions that are not independent per image
run with img_shards=1.  Step ms is the longest of the devices' times; a call's share counts the time its device-side launches took, not the
cross-device copies behind them.  No figure for more than one physical GPU is recorded yet.

--freeze SPEC / --bn-global: the full step beside the step under ConvPipeBck(freeze=Freeze(...)), in ONE process in alternating blocks.  SPEC: a
comma list of param names / op tags / suffixes, or all-but:TAG[,TAG] (a linear probe: --freeze all-but:fc1000).  --bn-global: a leg with every BatchNorm on its running
pair; with both, a third leg with both.  Per leg the step's median ms, its ratio to the full step's, the calls, and ms per function.  Appended to profiles/r22_freeze.txt.
    python tools/bck_pipe_bench.py --nets resnet50 --batch 32 --freeze all-but:fc1000 --bn-global
--img-chunks N: ConvPipeBck(img_chunks=...), the training BatchNorm's sums in the chunked chain and the Eltwise gradients as hip_split copies.
Legs, ONE PROCESS EACH (a multi-device backend and a one-device backend do not share a process here), in --repeats alternating blocks -- every block starts every leg's
process anew, runs --warmup steps and times --runs: "default" (the step as it is), "chunks1" (img_chunks=1: the same kernels and bits; expected inside the blocks'
spread), "chunksN" (img_chunks=N on one device) and, with --devices d0:d1:... (N must be the device count), "devices" (the step on `(be=hip,devices=...)`).  Per leg one
JSON line (step ms as the median over all blocks, the block medians, images/s, the call count, the loss, the per-function share) and one with the quotients against
"default" of the same run.  No figure is required.  Devices that are shards of ONE physical GPU (0:0) run the exchange and say NOTHING about scaling: the shards
share the GPU, and step ms is the longest of the shards' times.  On several devices a chunked call's share counts its first device-side piece only.

--nets resnet50: the fourth net, with its 53 BatchNorm + Scale runs as training BatchNorms (hip_bn_stats / hip_bn_fwd / hip_bn_bck_sums / hip_bn_bck_in) and its 16 Eltwise
gradients as hip_fan_out.  The step must end with a finite loss (the child fails otherwise).  Its first step compiles some 150 specialisations: give it --limit 900.

Every net runs in a child process of its own under a time limit (--limit seconds); the first one that fails ends the run.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _pipe(net, batch):
    """nin | alexnet | resnet50 (BatchNorm / Scale as a training BatchNorm) at `batch` images."""
    from boda_amd import conv_pipe
    return {"nin": conv_pipe.nin_imagenet, "alexnet": conv_pipe.alexnet_ng_conv, "resnet50": conv_pipe.resnet50}[net](batch)


def fuse_ab(net, batch, runs, warmup, repeats, option="fuse_relu_grad"):
    import numpy as np
    from boda_amd import conv_pipe
    from boda_amd.bck_pipe import ConvPipeBck, add_bck_ops, host_params
    from boda_amd.rtc import make_rtc
    cp = _pipe(net, batch)
    bp = add_bck_ops(cp)
    params = host_params(bp, 5)
    rng = np.random.default_rng(0)
    data = rng.uniform(-1, 1, cp.nodes["data"].sizes).astype(np.float32)
    label = rng.integers(0, 1000, (batch, 1, 1)).astype(np.float32)
    ways = {}
    for way, fuse in (("unfused", False), ("fused", True)):
        rtc = make_rtc("(be=hip)", 0)
        rtc.init()
        drv = ConvPipeBck(rtc, **{option: fuse})
        drv.init(bp, params)
        rtc.copy_nda_to_var("data", data); rtc.copy_nda_to_var("label", label)
        ways[way] = {"rtc": rtc, "drv": drv, "blocks": [], "ms": [], "share": {}}
    for w in ways.values():
        for i in range(warmup):
            w["drv"].set_det_drop_seed(i); w["drv"].run_device_only()
    for rep in range(repeats):
        for w in ways.values():
            ms = []
            for i in range(runs):
                w["drv"].set_det_drop_seed(warmup + rep * runs + i)
                ms.append(w["drv"].run_device_only())
                for _, fn, d in w["drv"].per_call_ms:
                    w["share"][fn] = w["share"].get(fn, 0.0) + d
            w["ms"] += ms; w["blocks"].append(round(statistics.median(ms), 3))
    loss = {k: float(w["rtc"].copy_var_to_nda("loss").item()) for k, w in ways.items()}
    for way, w in ways.items():
        tot = sum(w["share"].values()); step = statistics.median(w["ms"])
        print(json.dumps({"net": net, "batch": batch, "way": way, "calls": len(w["drv"].calls()), "step_ms": round(step, 3), "block_medians_ms": w["blocks"],
                          "imgs_per_s": round(batch / (step * 1e-3), 1), "loss": round(loss[way], 4),
                          "share": {k: round(v / tot, 4) for k, v in sorted(w["share"].items(), key=lambda kv: -kv[1])},
                          "ms_per_step": {k: round(v / len(w["ms"]), 3) for k, v in sorted(w["share"].items(), key=lambda kv: -kv[1])}}), flush=True)
    u, f = ways["unfused"], ways["fused"]
    print(json.dumps({"net": net, "launches_removed": len(u["drv"].calls()) - len(f["drv"].calls()), "folded": f["drv"].fused_relu_grads["folded"],
                      "unfolded": sorted(f["drv"].fused_relu_grads["unfolded"]), "fused_over_unfused": round(statistics.median(f["ms"]) / statistics.median(u["ms"]), 4),
                      "same_loss_bits": loss["unfused"] == loss["fused"]}), flush=True)
    for w in ways.values():
        w["drv"].release(); w["rtc"].close()


GOOGLENET_TOPS = ["cls3_fc", "cls1_fc2", "cls2_fc2"]   # the main head first, then the two auxiliary ones: add_bck_ops tags them loss1, loss2, loss3


def loss_ab(batch, runs, warmup, repeats, weights):
    """--loss-weights W1,W2,W3: GoogLeNet's step with its three heads capped by the reference's unweighted losses, beside the step with
    LossSpec(weight=W) per head IN THE ORDER OF THE NET'S LOSS LAYERS (loss1 and loss2 the auxiliary heads, loss3 the main one: Caffe's 0.3,0.3,1), in ONE process in
    alternating blocks; per way the step, the calls, the three losses and the us per step of the loss functions."""
    import numpy as np
    from boda_amd import conv_pipe
    from boda_amd.bck_pipe import ConvPipeBck, LossSpec, add_bck_ops, host_params
    from boda_amd.rtc import make_rtc
    cp = conv_pipe.googlenet_conv(batch)
    w1, w2, w3 = weights
    specs = {"cls1_fc2": LossSpec(w1), "cls2_fc2": LossSpec(w2), "cls3_fc": LossSpec(w3)}
    rng = np.random.default_rng(0)
    data = rng.uniform(-1, 1, cp.nodes["data"].sizes).astype(np.float32)
    label = rng.integers(0, 1000, (batch, 1, 1)).astype(np.float32)
    ways = {}
    for way, sp in (("unweighted", None), ("weighted", specs)):
        bp = add_bck_ops(cp, loss_tops=GOOGLENET_TOPS, loss_specs=sp)
        rtc = make_rtc("(be=hip)", 0)
        rtc.init()
        drv = ConvPipeBck(rtc)
        drv.init(bp, host_params(bp, 5))
        rtc.copy_nda_to_var("data", data); rtc.copy_nda_to_var("label", label)
        ways[way] = {"rtc": rtc, "drv": drv, "bp": bp, "blocks": [], "ms": [], "share": {}}
    for w in ways.values():
        for i in range(warmup):
            w["drv"].set_det_drop_seed(i); w["drv"].run_device_only()
    for rep in range(repeats):
        for w in ways.values():
            ms = []
            for i in range(runs):
                w["drv"].set_det_drop_seed(warmup + rep * runs + i)
                ms.append(w["drv"].run_device_only())
                for _, fn, d in w["drv"].per_call_ms:
                    w["share"][fn] = w["share"].get(fn, 0.0) + d
            w["ms"] += ms; w["blocks"].append(round(statistics.median(ms), 3))
    loss_fns = ("hip_softmax", "hip_sm_grad_and_loss", "hip_sum_loss_over_imgs", "hip_softmax_loss_fwd", "hip_loss_norm", "hip_softmax_loss_bck")
    for way, w in ways.items():
        step = statistics.median(w["ms"])
        losses = {n: round(float(w["rtc"].copy_var_to_nda(n).item()), 4) for n in w["bp"].loss_nodes}
        if not all(np.isfinite(v) for v in losses.values()):
            raise SystemExit(f"googlenet {way}: a loss is not finite: {losses}")
        print(json.dumps({"net": "googlenet", "batch": batch, "way": way, "loss_weights": list(weights) if way == "weighted" else None, "calls": len(w["drv"].calls()),
                          "step_ms": round(step, 3), "block_medians_ms": w["blocks"], "imgs_per_s": round(batch / (step * 1e-3), 1), "losses": losses,
                          "loss_calls_us_per_step": {fn: round(1e3 * w["share"][fn] / len(w["ms"]), 1) for fn in loss_fns if fn in w["share"]}}), flush=True)
    print(json.dumps({"net": "googlenet", "weighted_over_unweighted": round(statistics.median(ways["weighted"]["ms"]) / statistics.median(ways["unweighted"]["ms"]), 4)}), flush=True)
    for w in ways.values():
        w["drv"].release(); w["rtc"].close()


def freeze_of(cp, spec, bn_global):
    """--freeze SPEC -> Freeze: SPEC a comma list of param names / op tags / suffixes, or all-but:TAG[,TAG...] (every param but those of the ops named)."""
    from boda_amd.bck_pipe import Freeze, bn_stat_params
    params = ()
    if spec.startswith("all-but:"):
        keep = spec[len("all-but:"):].split(",")
        stats = set(bn_stat_params(cp))
        params = tuple(p for p in cp.params if p not in stats and p.rsplit("_", 1)[0] not in keep)
    elif spec:
        params = tuple(spec.split(","))
    return Freeze(params=params, bn_global_stats=bool(bn_global))


def freeze_ab(net, batch, runs, warmup, repeats, spec, bn_global):
    """The full step, (--bn-global) the step with every BatchNorm on its running pair, and (--freeze SPEC) the step under that Freeze, in ONE process in alternating
    blocks, each leg a ConvPipeBck on a backend instance of its own with the same params and inputs."""
    import numpy as np
    from boda_amd.bck_pipe import ConvPipeBck, Freeze, add_bck_ops, host_params
    from boda_amd.rtc import make_rtc
    cp = _pipe(net, batch)
    bp = add_bck_ops(cp)
    params = host_params(bp, 5)
    rng = np.random.default_rng(0)
    data = rng.uniform(-1, 1, cp.nodes["data"].sizes).astype(np.float32)
    label = rng.integers(0, 1000, (batch, 1, 1)).astype(np.float32)
    legs = [("full", None)] + ([("bn_global", Freeze(bn_global_stats=True))] if bn_global else []) + ([("freeze", freeze_of(cp, spec, bn_global))] if spec else [])
    ways = {}
    for way, fz in legs:
        rtc = make_rtc("(be=hip)", 0)
        rtc.init()
        drv = ConvPipeBck(rtc, freeze=fz)
        drv.init(add_bck_ops(cp), params)
        rtc.copy_nda_to_var("data", data); rtc.copy_nda_to_var("label", label)
        ways[way] = {"rtc": rtc, "drv": drv, "blocks": [], "ms": [], "share": {}}
    for w in ways.values():
        for i in range(warmup):
            w["drv"].set_det_drop_seed(i); w["drv"].run_device_only()
    for rep_ in range(repeats):
        for w in ways.values():
            ms = []
            for i in range(runs):
                w["drv"].set_det_drop_seed(warmup + rep_ * runs + i)
                ms.append(w["drv"].run_device_only())
                for _, fn, d in w["drv"].per_call_ms:
                    w["share"][fn] = w["share"].get(fn, 0.0) + d
            w["ms"] += ms; w["blocks"].append(round(statistics.median(ms), 3))
    full = statistics.median(ways["full"]["ms"])
    for way, w in ways.items():
        step = statistics.median(w["ms"]); fr = w["drv"].frozen
        print(json.dumps({"net": net, "batch": batch, "way": way, "calls": len(w["drv"].calls()), "step_ms": round(step, 3), "block_medians_ms": w["blocks"], "over_full": round(step / full, 4),
                          "imgs_per_s": round(batch / (step * 1e-3), 1), "loss": round(float(w["rtc"].copy_var_to_nda("loss").item()), 4),
                          "frozen_params": len(fr["params"]), "dropped_gradient_ops": len(fr["dropped_calls"]), "bn_global": len(fr["bn_global"]),
                          "ms_per_step": {k: round(v / len(w["ms"]), 3) for k, v in sorted(w["share"].items(), key=lambda kv: -kv[1])}}), flush=True)
    for w in ways.values():
        w["drv"].release(); w["rtc"].close()


def operands_ab(net, batch, runs, warmup, repeats, mode):
    import numpy as np
    from boda_amd.bck_pipe import ConvPipeBck, add_bck_ops, host_params
    from boda_amd.rtc import make_rtc
    cp = _pipe(net, batch)
    bp = add_bck_ops(cp)
    params = host_params(bp, 5)
    rng = np.random.default_rng(0)
    data = rng.uniform(-1, 1, cp.nodes["data"].sizes).astype(np.float32)
    label = rng.integers(0, 1000, (batch, 1, 1)).astype(np.float32)
    ways = {}
    for way, kw in (("f32", {}), ("f32_fused", {"fuse_filts_biases": True}), (mode, {"grad_operands": mode})):
        rtc = make_rtc("(be=hip)", 0)
        rtc.init()
        drv = ConvPipeBck(rtc, **kw)
        drv.init(bp, params)
        rtc.copy_nda_to_var("data", data); rtc.copy_nda_to_var("label", label)
        ways[way] = {"rtc": rtc, "drv": drv, "blocks": [], "ms": [], "share": {}}
    for w in ways.values():
        for i in range(warmup):
            w["drv"].set_det_drop_seed(i); w["drv"].run_device_only()
    for rep in range(repeats):
        for w in ways.values():
            ms = []
            for i in range(runs):
                w["drv"].set_det_drop_seed(warmup + rep * runs + i)
                ms.append(w["drv"].run_device_only())
                for _, fn, d in w["drv"].per_call_ms:
                    w["share"][fn] = w["share"].get(fn, 0.0) + d
            w["ms"] += ms; w["blocks"].append(round(statistics.median(ms), 3))
    loss = {k: w["rtc"].copy_var_to_nda("loss").tobytes() for k, w in ways.items()}
    for way, w in ways.items():
        tot = sum(w["share"].values()); step = statistics.median(w["ms"])
        lv = float(np.frombuffer(loss[way], np.float32)[0])
        if not np.isfinite(lv):
            raise SystemExit(f"{net} {way}: the step ended with the loss {lv}")
        print(json.dumps({"net": net, "batch": batch, "way": way, "calls": len(w["drv"].calls()), "step_ms": round(step, 3), "block_medians_ms": w["blocks"],
                          "imgs_per_s": round(batch / (step * 1e-3), 1), "loss": round(lv, 4),
                          "share": {k: round(v / tot, 4) for k, v in sorted(w["share"].items(), key=lambda kv: -kv[1])},
                          "ms_per_step": {k: round(v / len(w["ms"]), 3) for k, v in sorted(w["share"].items(), key=lambda kv: -kv[1])}}), flush=True)
    med = lambda k: statistics.median(ways[k]["ms"])
    print(json.dumps({"net": net, f"{mode}_over_f32": round(med(mode) / med("f32"), 4), f"{mode}_over_f32_fused": round(med(mode) / med("f32_fused"), 4),
                      "same_loss_bits": loss["f32"] == loss["f32_fused"] == loss[mode]}), flush=True)
    for w in ways.values():
        w["drv"].release(); w["rtc"].close()


def graph_ab(net, batch, runs, warmup, repeats):
    import numpy as np
    from boda_amd import conv_pipe
    from boda_amd.bck_pipe import ConvPipeBck, add_bck_ops, host_params
    from boda_amd.rtc import make_rtc
    cp = _pipe(net, batch)
    bp = add_bck_ops(cp)
    params = host_params(bp, 5)
    rng = np.random.default_rng(0)
    data = rng.uniform(-1, 1, cp.nodes["data"].sizes).astype(np.float32)
    label = rng.integers(0, 1000, (batch, 1, 1)).astype(np.float32)
    ways = {}
    for way in ("eager", "graph", "graph_parallel"):
        rtc = make_rtc("(be=hip)", 0)
        rtc.init()
        drv = ConvPipeBck(rtc, seed_in_var=True)
        drv.init(bp, params)
        rtc.copy_nda_to_var("data", data); rtc.copy_nda_to_var("label", label)
        drv.set_det_drop_seed(0); drv.run_device_only()   # (every way's first step is an eager one: kernels and workspaces)
        captured = drv.capture_graph(parallel=(way == "graph_parallel")) if way != "eager" else 0
        ways[way] = {"rtc": rtc, "drv": drv, "blocks": [], "ms": [], "captured": captured, "run": drv.run_device_only if way == "eager" else drv.run_graph}
    for w in ways.values():
        for i in range(warmup):
            w["drv"].set_det_drop_seed(i); w["run"]()
    for rep in range(repeats):
        for w in ways.values():
            ms = []
            for i in range(runs):
                w["drv"].set_det_drop_seed(warmup + rep * runs + i)
                ms.append(w["run"]())
            w["ms"] += ms; w["blocks"].append(round(statistics.median(ms), 3))
    loss = {k: w["rtc"].copy_var_to_nda("loss").tobytes() for k, w in ways.items()}
    for way, w in ways.items():
        step = statistics.median(w["ms"])
        print(json.dumps({"net": net, "batch": batch, "way": way, "calls": len(w["drv"].calls()), "captured_calls": w["captured"], "step_ms": round(step, 3),
                          "block_medians_ms": w["blocks"], "imgs_per_s": round(batch / (step * 1e-3), 1),
                          "loss": round(float(np.frombuffer(loss[way], np.float32)[0]), 4)}), flush=True)
    e = statistics.median(ways["eager"]["ms"])
    print(json.dumps({"net": net, "graph_over_eager": round(statistics.median(ways["graph"]["ms"]) / e, 4),
                      "graph_parallel_over_eager": round(statistics.median(ways["graph_parallel"]["ms"]) / e, 4),
                      "same_loss_bits": loss["eager"] == loss["graph"] == loss["graph_parallel"]}), flush=True)
    for w in ways.values():
        w["drv"].release(); w["rtc"].close()


def sgd_ab(net, batch, runs, warmup, repeats):
    import numpy as np
    from boda_amd import conv_pipe
    from boda_amd.bck_pipe import ConvPipeBck, SgdSolver, add_bck_ops, host_params
    from boda_amd.rtc import make_rtc
    cp = _pipe(net, batch)
    bp = add_bck_ops(cp)
    params = host_params(bp, 5)
    rng = np.random.default_rng(0)
    data = rng.uniform(-1, 1, cp.nodes["data"].sizes).astype(np.float32)
    label = rng.integers(0, 1000, (batch, 1, 1)).astype(np.float32)
    algo_bytes = 20.0 * sum(d.dims_prod() for d in cp.params.values())
    ways = {}
    for way, per in (("no_solver", 0), ("sgd_packed", 32), ("sgd_per_tensor", 1)):
        rtc = make_rtc("(be=hip)", 0)
        rtc.init()
        solver = SgdSolver(lr=1e-5, momentum=0.9, weight_decay=5e-4, lr_mult={"biases": 2.0}, decay_mult={"biases": 0.0}, tensors_per_call=per) if per else None   # (a rate at which random labels keep every value finite)
        drv = ConvPipeBck(rtc, solver=solver)
        drv.init(bp, params)
        rtc.copy_nda_to_var("data", data); rtc.copy_nda_to_var("label", label)
        ways[way] = {"rtc": rtc, "drv": drv, "blocks": [], "ms": [], "upd_ms": []}
    for w in ways.values():
        for i in range(warmup):
            w["drv"].set_det_drop_seed(i); w["drv"].run_device_only()
    for rep in range(repeats):
        for w in ways.values():
            ms = []
            for i in range(runs):
                w["drv"].set_det_drop_seed(warmup + rep * runs + i)
                ms.append(w["drv"].run_device_only())
                w["upd_ms"].append(sum(d for _, fn, d in w["drv"].per_call_ms if fn == "hip_sgd_update"))
            w["ms"] += ms; w["blocks"].append(round(statistics.median(ms), 3))
    for way, w in ways.items():
        step = statistics.median(w["ms"]); upd = statistics.median(w["upd_ms"])
        rec = {"net": net, "batch": batch, "way": way, "calls": len(w["drv"].calls()), "step_ms": round(step, 3), "block_medians_ms": w["blocks"],
               "imgs_per_s": round(batch / (step * 1e-3), 1), "loss": round(float(w["rtc"].copy_var_to_nda("loss").item()), 4)}
        if w["drv"].n_sgd_calls:
            rec.update({"update_calls": w["drv"].n_sgd_calls, "param_tensors": len(cp.params), "update_us": round(upd * 1e3, 1), "update_algo_bytes": algo_bytes,
                        "update_GBps": round(algo_bytes / (upd * 1e-3) / 1e9, 1), "copy_rate_GBps_recorded": 6290.0})
        print(json.dumps(rec), flush=True)
    med = lambda k, f: statistics.median(ways[k][f])
    print(json.dumps({"net": net, "sgd_packed_over_no_solver": round(med("sgd_packed", "ms") / med("no_solver", "ms"), 4),
                      "sgd_per_tensor_over_no_solver": round(med("sgd_per_tensor", "ms") / med("no_solver", "ms"), 4),
                      "packed_over_per_tensor_step": round(med("sgd_packed", "ms") / med("sgd_per_tensor", "ms"), 4),
                      "packed_over_per_tensor_update": round(med("sgd_packed", "upd_ms") / med("sgd_per_tensor", "upd_ms"), 4)}), flush=True)
    for w in ways.values():
        w["drv"].release(); w["rtc"].close()


def solver_ab(net, batch, runs, warmup, repeats, solver_type, clip, swap=False, iter_size=1):
    """--solver: the step with hip_sgd_update (SgdSolver, the rate every other figure is held against) and with Solver(type=solver_type, clip_gradients=clip), in
    alternating blocks in one process: per way one JSON line with, per update function, the median us of its calls per step, the bytes they move and GB/s.
    iter_size > 1 (--iter-size): the two legs are the Solver's step with iter_size=1 and with iter_size=n (hip_grad_accum on every pass, hip_solver_update_acc; DESIGN.md
    section 3.19) of the same build; hip_solver_update_acc's us and GB/s are those of the passes that apply, "us_not_applying" those of the others."""
    import numpy as np
    from boda_amd.bck_pipe import ConvPipeBck, SgdSolver, Solver, add_bck_ops, bn_stat_params, host_params
    from boda_amd.rtc import make_rtc
    cp = _pipe(net, batch)
    bp = add_bck_ops(cp)
    params = host_params(bp, 5)
    rng = np.random.default_rng(0)
    data = rng.uniform(-1, 1, cp.nodes["data"].sizes).astype(np.float32)
    label = rng.integers(0, 1000, (batch, 1, 1)).astype(np.float32)
    kw = dict(lr=1e-5, momentum=0.9, weight_decay=5e-4, lr_mult={"biases": 2.0}, decay_mult={"biases": 0.0})   # (a rate at which random labels keep every value finite)
    way2 = "solver_" + solver_type + ("_clip" if clip > 0 else "")   # ("solver_sgd": the same chain as the "sgd" leg, in the new kernel)
    ways = {}
    legs = [("sgd", SgdSolver(**kw), 1), (way2, Solver(type=solver_type, clip_gradients=clip, **kw), 1)]
    if iter_size > 1:
        base, way2 = way2, way2 + f"_iter{iter_size}"
        legs = [(base, Solver(type=solver_type, clip_gradients=clip, **kw), 1), (way2, Solver(type=solver_type, clip_gradients=clip, **kw), iter_size)]
    for way, solver, n_it in (legs[::-1] if swap else legs):   # (swap: the Solver leg is built and run first -- which backend allocates first is then the other one)
        rtc = make_rtc("(be=hip)", 0)
        rtc.init()
        drv = ConvPipeBck(rtc, solver=solver, iter_size=n_it)
        drv.init(bp, params)
        rtc.copy_nda_to_var("data", data); rtc.copy_nda_to_var("label", label)
        ways[way] = {"rtc": rtc, "drv": drv, "blocks": [], "ms": [], "fn_ms": {}, "idle_ms": {}}
    for w in ways.values():
        for i in range(warmup):
            w["drv"].set_det_drop_seed(i); w["drv"].run_device_only()
    for rep in range(repeats):
        for w in ways.values():
            ms = []
            for i in range(runs):
                w["drv"].set_det_drop_seed(warmup + rep * runs + i)
                applies = w["drv"].micro == w["drv"].iter_size - 1
                ms.append(w["drv"].run_device_only())
                tail = w["drv"].per_call_ms[len(w["drv"].per_call_ms) - w["drv"].n_sgd_calls:]
                for fn in {fn for _, fn, _ in tail}:
                    (w["fn_ms"] if applies or fn != "hip_solver_update_acc" else w["idle_ms"]).setdefault(fn, []).append(sum(d for _, f, d in tail if f == fn))
            w["ms"] += ms; w["blocks"].append(round(statistics.median(ms), 3))
    for way, w in ways.items():
        step = statistics.median(w["ms"])
        fns = {}
        for fn, ds in w["fn_ms"].items():
            us = statistics.median(ds) * 1e3
            nbytes = sum(f.algo_bytes() for _, f, _ in w["drv"].calls() if f.get_func_name() == fn)
            fns[fn] = {"calls": sum(1 for _, f, _ in w["drv"].calls() if f.get_func_name() == fn), "us": round(us, 1), "algo_bytes": nbytes, "GBps": round(nbytes / (us * 1e-6) / 1e9, 1)}
            if fn in w["idle_ms"]:
                fns[fn]["us_not_applying"] = round(statistics.median(w["idle_ms"][fn]) * 1e3, 1)
        print(json.dumps({"net": net, "batch": batch, "way": way, "calls": len(w["drv"].calls()), "step_ms": round(step, 3), "block_medians_ms": w["blocks"],
                          "imgs_per_s": round(batch / (step * 1e-3), 1), "loss": round(float(w["rtc"].copy_var_to_nda("loss").item()), 4),
                          "param_tensors": len(w["drv"].sgd_params), "update_functions": fns, "copy_rate_GBps_recorded": 6290.0}), flush=True)
    first = legs[0][0]
    print(json.dumps({"net": net, f"{way2}_over_{first}_step": round(statistics.median(ways[way2]["ms"]) / statistics.median(ways[first]["ms"]), 4)}), flush=True)
    for w in ways.values():
        w["drv"].release(); w["rtc"].close()


def eval_ab(net, batch, runs, warmup, repeats, n_eval):
    """--eval: alternating blocks of `runs` training steps and `n_eval` evaluation batches of an EvalPipe over the same driver, one process."""
    import numpy as np
    from boda_amd.bck_pipe import ConvPipeBck, SgdSolver, add_bck_ops, host_params
    from boda_amd.eval_pipe import EvalPipe
    from boda_amd.rtc import make_rtc
    cp = _pipe(net, batch)
    bp = add_bck_ops(cp)
    rng = np.random.default_rng(0)
    data = rng.uniform(-1, 1, cp.nodes["data"].sizes).astype(np.float32)
    label = rng.integers(0, 1000, (batch, 1, 1)).astype(np.float32)
    rtc = make_rtc("(be=hip)", 0)
    rtc.init()
    drv = ConvPipeBck(rtc, solver=SgdSolver(lr=1e-5, momentum=0.9, weight_decay=5e-4, lr_mult={"biases": 2.0}, decay_mult={"biases": 0.0}))   # (a rate at which random labels keep every value finite)
    drv.init(bp, host_params(bp, 5))
    ev = EvalPipe(drv, top_k=5)
    rtc.copy_nda_to_var("data", data); rtc.copy_nda_to_var("label", label)
    for i in range(warmup):
        drv.set_det_drop_seed(i); drv.run_device_only()
        ev.run_device_only()
    step_ms, eval_ms, step_blocks, eval_blocks, fn_us = [], [], [], [], {}
    for rep in range(repeats):
        ms = []
        for i in range(runs):
            drv.set_det_drop_seed(warmup + rep * runs + i)
            ms.append(drv.run_device_only())
        step_ms += ms; step_blocks.append(round(statistics.median(ms), 3))
        ev.reset()
        ms = []
        for i in range(n_eval):
            ms.append(ev.run_device_only())
            for fn in ("hip_accuracy", "hip_eval_accum", "hip_bn_fold", "hip_chan_affine"):
                ds = [d for _, f, d in ev.per_call_ms if f == fn]
                if ds:
                    fn_us.setdefault(fn, []).append(sum(ds) * 1e3)
        eval_ms += ms; eval_blocks.append(round(statistics.median(ms), 3))
    res = ev.result()
    loss = float(rtc.copy_var_to_nda("loss").item())
    if not np.isfinite(loss) or res["batches"] != n_eval or res["images"] != n_eval * batch:
        raise SystemExit(f"{net}: loss {loss}, result {res}")
    st, et = statistics.median(step_ms), statistics.median(eval_ms)
    n_of = lambda fn: sum(1 for _, f, _ in ev.calls() if f.get_func_name() == fn)
    print(json.dumps({"net": net, "batch": batch, "eval_batches_per_block": n_eval, "step_calls": len(drv.calls()), "eval_calls": len(ev.calls()), "step_ms": round(st, 3),
                      "eval_batch_ms": round(et, 3), "eval_over_step": round(et / st, 4), "step_block_medians_ms": step_blocks, "eval_block_medians_ms": eval_blocks,
                      "imgs_per_s_training": round(batch / (st * 1e-3), 1), "imgs_per_s_eval": round(batch / (et * 1e-3), 1),
                      "eval_functions": {fn: {"calls": n_of(fn), "us_per_batch": round(statistics.median(v), 1)} for fn, v in fn_us.items()},
                      "result": {k: (round(v, 6) if isinstance(v, float) else v) for k, v in res.items()}}), flush=True)
    ev.release(); drv.release(); rtc.close()


def one_net(net, batch, runs, warmup, devices="", img_chunks=0, raw=False):
    import numpy as np
    from boda_amd import conv_pipe
    from boda_amd.bck_pipe import ConvPipeBck, add_bck_ops
    from boda_amd.rtc import make_rtc
    cp = _pipe(net, batch)
    bp = add_bck_ops(cp)
    rtc = make_rtc(f"(be=hip,devices={devices})" if devices else "(be=hip)", 0)   # (several devices: the driver flags the five functions that are not independent per image)
    rtc.init()
    drv = ConvPipeBck(rtc, img_chunks=img_chunks)
    drv.init(bp)
    rng = np.random.default_rng(0)
    rtc.copy_nda_to_var("data", rng.uniform(-1, 1, cp.nodes["data"].sizes).astype(np.float32))
    rtc.copy_nda_to_var("label", rng.integers(0, 1000, (batch, 1, 1)).astype(np.float32))
    ms, share = [], {}
    for i in range(warmup + runs):
        drv.set_det_drop_seed(i)
        t = drv.run_device_only()
        if i >= warmup:
            ms.append(t)
            for _, fn, d in drv.per_call_ms:
                share[fn] = share.get(fn, 0.0) + d
    loss = float(rtc.copy_var_to_nda("loss").item())
    if not np.isfinite(loss):
        raise SystemExit(f"{net}: the step ended with the loss {loss}")
    tot = sum(share.values())
    step = statistics.median(ms)
    if raw:   # one block of one leg of --img-chunks: the parent puts the blocks together
        print(json.dumps({"ms": ms, "share_ms": share, "calls": len(drv.calls()), "loss": loss}), flush=True)
        drv.release(); rtc.close()
        return
    print(json.dumps({"net": net, "batch": batch, **({"devices": devices} if devices else {}), "calls": len(drv.calls()), "step_ms": round(step, 3), "imgs_per_s": round(batch / (step * 1e-3), 1), "loss": round(loss, 4),
                      "share": {k: round(v / tot, 4) for k, v in sorted(share.items(), key=lambda kv: -kv[1])}}), flush=True)
    drv.release(); rtc.close()


def chunks_ab(a, net):
    """The legs of --img-chunks, one process per leg and block, alternating -> the JSON lines (None after a failure: nothing more is started on the GPU)."""
    legs = [("default", 0, ""), ("chunks1", 1, ""), (f"chunks{a.img_chunks}", a.img_chunks, "")] + ([("devices", a.img_chunks, a.devices)] if a.devices else [])
    acc = {name: {"ms": [], "blocks": [], "share": {}, "calls": 0, "loss": None} for name, _, _ in legs}
    for rep in range(a.repeats):
        for name, n, devs in legs:
            cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--child", net, "--batch", str(a.batch), "--runs", str(a.runs), "--warmup", str(a.warmup),
                   "--img-chunks", str(n), "--raw"] + (["--devices", devs] if devs else [])
            r = subprocess.run(cmd, capture_output=True, text=True)
            if r.returncode != 0:
                print(f"{net} {name}: exit status {r.returncode}\n{r.stderr[-2000:]}", file=sys.stderr)
                return None
            rec = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
            w = acc[name]
            w["ms"] += rec["ms"]; w["blocks"].append(round(statistics.median(rec["ms"]), 3)); w["calls"] = rec["calls"]; w["loss"] = rec["loss"]
            print(f"{net} block {rep} {name}: {w['blocks'][-1]} ms", file=sys.stderr, flush=True)
            for k, v in rec["share_ms"].items():
                w["share"][k] = w["share"].get(k, 0.0) + v
    lines = []
    for name, n, devs in legs:
        w = acc[name]; tot = sum(w["share"].values()); step = statistics.median(w["ms"])
        lines.append(json.dumps({"net": net, "batch": a.batch, "leg": name, "img_chunks": n, **({"devices": devs} if devs else {}), "calls": w["calls"], "step_ms": round(step, 3),
                                 "block_medians_ms": w["blocks"], "imgs_per_s": round(a.batch / (step * 1e-3), 1), "loss": round(w["loss"], 4),
                                 "share": {k: round(v / tot, 4) for k, v in sorted(w["share"].items(), key=lambda kv: -kv[1])}}))
    base = statistics.median(acc["default"]["ms"])
    lines.append(json.dumps(dict({"net": net}, **{f"{name}_over_default": round(statistics.median(acc[name]["ms"]) / base, 4) for name, _, _ in legs[1:]},
                                 note="shards of one physical GPU say nothing about scaling" if a.devices and len(set(a.devices.split(":"))) == 1 else "")))
    return lines


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--nets", default="nin,alexnet")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--limit", type=int, default=240, help="seconds per net")
    ap.add_argument("--out", default="")
    ap.add_argument("--fuse-relu-grad", action="store_true", help="A/B: the step with and without the ReLU gradients folded into their producers, in one process")
    ap.add_argument("--fuse-filts-biases", action="store_true", help="A/B: the step with every BckConv's bias + filter gradient pair, and with the one fused hip_bconv_filts_biases call, in one process")
    ap.add_argument("--graph", action="store_true", help="A/B: the eager step, the step as one hipGraph replay, and the replay with the calls' true dependencies, in one process")
    ap.add_argument("--sgd", action="store_true", help="A/B: the step without a solver, with the SGD update as multi-tensor calls, and with one update call per tensor, in one process")
    ap.add_argument("--solver", default="", choices=["", "sgd", "nesterov", "adam"], help="A/B: the step with hip_sgd_update and with Solver(type=...) (hip_solver_update), in alternating blocks in one process; per update function us and GB/s")
    ap.add_argument("--swap", action="store_true", help="with --solver: build and run the Solver leg before the hip_sgd_update leg")
    ap.add_argument("--clip", type=float, default=0.0, help="with --solver: clip_gradients (0: off); adds the hip_grad_sumsq calls and hip_grad_norm")
    ap.add_argument("--iter-size", type=int, default=1, help="with --solver: the legs are the Solver's step with iter_size=1 and with iter_size=N (hip_grad_accum, hip_solver_update_acc)")
    ap.add_argument("--grad-operands", default="", choices=["", "bf16"], help="A/B: the fp32 step, the fp32 step with the fused filter + bias call, and the step with bf16 gradient operands, in one process")
    ap.add_argument("--repeats", type=int, default=3, help="with --fuse-relu-grad / --graph / --sgd: alternating blocks of --runs steps per way")
    ap.add_argument("--devices", default="", help="e.g. 0:1:2:3: the plain step on the multi-device backend (be=hip,devices=...), batch sharded on img")
    ap.add_argument("--img-chunks", type=int, default=0, help="A/B, one process per leg: the default step, img_chunks=1, img_chunks=N on one device and, with --devices, on the multi-device backend")
    ap.add_argument("--eval", type=int, default=0, dest="n_eval", help="alternating blocks of --runs training steps and N evaluation batches (eval_pipe.EvalPipe) in one process: ms per eval batch beside ms per step")
    ap.add_argument("--freeze", default="", help="A/B in one process: the full step beside the step under Freeze(params=SPEC): a comma list of param names / op tags / suffixes, or all-but:TAG[,TAG]")
    ap.add_argument("--bn-global", action="store_true", help="A/B in one process: the full step beside the step with every BatchNorm on its running pair; with --freeze the third leg has both")
    ap.add_argument("--loss-weights", default="", help="e.g. 0.3,0.3,1: A/B in one process on GoogLeNet (whatever --nets says): its three heads under the reference's unweighted losses beside LossSpec(weight=W) per loss layer")
    ap.add_argument("--raw", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--child", default="")
    a = ap.parse_args(argv)
    if a.img_chunks and not a.child and (a.graph or a.fuse_relu_grad or a.sgd or a.fuse_filts_biases or a.grad_operands):
        ap.error("--img-chunks is a comparison of its own: run it without the other A/Bs")
    if a.img_chunks and a.devices and a.img_chunks != len(a.devices.split(":")):
        ap.error("--img-chunks with --devices: chunk i is device i's shard, so N must be the device count")
    if a.devices and (a.graph or a.fuse_relu_grad or a.sgd or a.fuse_filts_biases or a.grad_operands):
        ap.error("--devices times the plain step: graph capture is not provided on several devices, and the fused and the solver A/B run on one")
    if a.graph + a.fuse_relu_grad + a.sgd + a.fuse_filts_biases + bool(a.grad_operands) + bool(a.solver) > 1:
        ap.error("--graph, --fuse-relu-grad, --fuse-filts-biases, --grad-operands, --sgd and --solver are six comparisons: run them one at a time")
    if a.solver and (a.devices or a.img_chunks):
        ap.error("--solver is a comparison of its own on one device")
    if a.n_eval and (a.graph or a.fuse_relu_grad or a.sgd or a.fuse_filts_biases or a.grad_operands or a.solver or a.devices or a.img_chunks):
        ap.error("--eval is a comparison of its own on one device")
    if (a.freeze or a.bn_global) and (a.graph or a.fuse_relu_grad or a.sgd or a.fuse_filts_biases or a.grad_operands or a.solver or a.devices or a.img_chunks or a.n_eval):
        ap.error("--freeze / --bn-global are a comparison of their own on one device")
    if a.loss_weights:
        if a.graph or a.fuse_relu_grad or a.sgd or a.fuse_filts_biases or a.grad_operands or a.solver or a.devices or a.img_chunks or a.n_eval or a.freeze or a.bn_global:
            ap.error("--loss-weights is a comparison of its own on one device")
        try:
            a.weights = tuple(float(v) for v in a.loss_weights.split(","))
        except ValueError:
            a.weights = ()
        if len(a.weights) != 3:
            ap.error("--loss-weights takes three numbers, one per loss layer of GoogLeNet: 0.3,0.3,1")
        a.nets = "googlenet"
    if a.n_eval < 0:
        ap.error("--eval N: at least 1 batch")
    if a.clip and not a.solver:
        ap.error("--clip goes with --solver")
    if a.iter_size != 1 and (not a.solver or a.iter_size < 1):
        ap.error("--iter-size goes with --solver and is at least 1")
    a.out = a.out or os.path.join(ROOT, "profiles", "r23_loss_googlenet.txt" if a.loss_weights else "r22_freeze.txt" if (a.freeze or a.bn_global) else "r20_eval.txt" if a.n_eval else "r17_resnet50_chunks.txt" if a.img_chunks else "r16_step_bf16.txt" if a.grad_operands else "r19_grad_accum.txt" if a.solver and a.iter_size > 1 else "r18_solver.txt" if a.solver else "r13_sgd_update.txt" if a.sgd else "r10_bck_graph_ab.txt" if a.graph else "r09_bck_fuse_ab.txt" if a.fuse_relu_grad else "r15_resnet50_step_fb.txt" if a.fuse_filts_biases else "bck_pipe_devices.txt" if a.devices else "r14_resnet50_step.txt" if a.nets == "resnet50" else "r09_bck_pipe_bench.txt")
    if a.child:
        if a.loss_weights:
            return loss_ab(a.batch, a.runs, a.warmup, a.repeats, a.weights)
        if a.freeze or a.bn_global:
            return freeze_ab(a.child, a.batch, a.runs, a.warmup, a.repeats, a.freeze, a.bn_global)
        if a.n_eval:
            return eval_ab(a.child, a.batch, a.runs, a.warmup, a.repeats, a.n_eval)
        if a.grad_operands:
            return operands_ab(a.child, a.batch, a.runs, a.warmup, a.repeats, a.grad_operands)
        if a.solver:
            return solver_ab(a.child, a.batch, a.runs, a.warmup, a.repeats, a.solver, a.clip, a.swap, a.iter_size)
        if a.sgd:
            return sgd_ab(a.child, a.batch, a.runs, a.warmup, a.repeats)
        if a.graph:
            return graph_ab(a.child, a.batch, a.runs, a.warmup, a.repeats)
        if a.fuse_filts_biases:
            return fuse_ab(a.child, a.batch, a.runs, a.warmup, a.repeats, "fuse_filts_biases")
        return fuse_ab(a.child, a.batch, a.runs, a.warmup, a.repeats) if a.fuse_relu_grad else one_net(a.child, a.batch, a.runs, a.warmup, a.devices, a.img_chunks, a.raw)
    lines = []
    for net in a.nets.split(","):
        if a.img_chunks:
            got = chunks_ab(a, net)
            if got is None:
                return 1
            lines += got
            print("\n".join(got), flush=True)
            continue
        cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--child", net, "--batch", str(a.batch), "--runs", str(a.runs), "--warmup", str(a.warmup)]
        cmd += ["--fuse-relu-grad", "--repeats", str(a.repeats)] if a.fuse_relu_grad else []
        cmd += ["--fuse-filts-biases", "--repeats", str(a.repeats)] if a.fuse_filts_biases else []
        cmd += ["--grad-operands", a.grad_operands, "--repeats", str(a.repeats)] if a.grad_operands else []
        cmd += ["--graph", "--repeats", str(a.repeats)] if a.graph else []
        cmd += ["--sgd", "--repeats", str(a.repeats)] if a.sgd else []
        cmd += ["--solver", a.solver, "--clip", str(a.clip), "--repeats", str(a.repeats)] + (["--swap"] if a.swap else []) + (["--iter-size", str(a.iter_size)] if a.iter_size > 1 else []) if a.solver else []
        cmd += ["--devices", a.devices] if a.devices else []
        cmd += (["--freeze", a.freeze] if a.freeze else []) + (["--bn-global"] if a.bn_global else []) + (["--repeats", str(a.repeats)] if (a.freeze or a.bn_global) else [])
        cmd += ["--eval", str(a.n_eval), "--repeats", str(a.repeats)] if a.n_eval else []
        cmd += ["--loss-weights", a.loss_weights, "--repeats", str(a.repeats)] if a.loss_weights else []
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:   # nothing more is started on the GPU after a failure
            print(f"{net}: exit status {r.returncode}\n{r.stderr[-2000:]}", file=sys.stderr)
            return r.returncode
        lines += [l for l in r.stdout.splitlines() if l.startswith("{")]
        print("\n".join(lines[-3:] if (a.freeze or a.bn_global or a.loss_weights) else lines[-4:] if (a.graph or a.sgd or a.grad_operands) else lines[-3:] if (a.fuse_relu_grad or a.fuse_filts_biases or a.solver) else lines[-1:]), flush=True)
    with open(a.out, "a" if (a.freeze or a.bn_global) else "w") as f:     # (profiles/r22_freeze.txt also holds tools/bn_bench.py --frozen's record)
        extra = f" --loss-weights {a.loss_weights} --repeats {a.repeats}" if a.loss_weights else f"{' --freeze ' + a.freeze if a.freeze else ''}{' --bn-global' if a.bn_global else ''} --repeats {a.repeats}" if (a.freeze or a.bn_global) else f" --eval {a.n_eval} --repeats {a.repeats}" if a.n_eval else f" --img-chunks {a.img_chunks}{' --devices ' + a.devices if a.devices else ''} --repeats {a.repeats}" if a.img_chunks else f" --grad-operands {a.grad_operands} --repeats {a.repeats}" if a.grad_operands else f" --devices {a.devices}" if a.devices else f" --solver {a.solver} --clip {a.clip}{' --swap' if a.swap else ''}{f' --iter-size {a.iter_size}' if a.iter_size > 1 else ''} --repeats {a.repeats}" if a.solver else f" --sgd --repeats {a.repeats}" if a.sgd else f" --graph --repeats {a.repeats}" if a.graph else f" --fuse-relu-grad --repeats {a.repeats}" if a.fuse_relu_grad else f" --fuse-filts-biases --repeats {a.repeats}" if a.fuse_filts_biases else ""
        f.write(f"# python tools/bck_pipe_bench.py --nets {a.nets} --batch {a.batch} --runs {a.runs} --warmup {a.warmup}{extra}\n" + "\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main() or 0)
