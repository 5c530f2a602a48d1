"""Times the three functions of the full SoftmaxWithLoss (boda_amd/csrc/kernels/loss_f32.hip) on be=hip, in ONE process, in --repeats
alternating blocks of --runs calls (after --warmup calls of everything), as tools/bn_bench.py does.  A record, not a gate: the default loss path is untouched.

Against the old path, at 128 x 1000 x 1 x 1: hip_softmax_loss_fwd / hip_loss_norm / hip_softmax_loss_bck beside the reference's three calls (hip_softmax,
hip_sm_grad_and_loss, hip_sum_loss_over_imgs) on the same logits and labels: microseconds each (device events around the call), the totals, and the block-to-block
spread of the old calls' total, which is what a difference has to beat.
Against the copy rate, at 32 x 21 x 64 x 64 and 8 x 21 x 500 x 500: the three calls as GB/s of the bytes each must move (fwd: in and prob once, label and loss_per_pel;
norm: label and loss_per_pel; bck: prob and in_grad_loss once, label), beside the copy rate profiles/ records for this device, 6.29 TB/s -- tools/bck_ops_bench.py's
presentation.

    python tools/loss_bench.py [--runs 20] [--warmup 5] [--repeats 3] [--out profiles/r23_loss.txt]

A measurement path that finds no GPU fails.  Run it under a time limit (timeout -k 10 600 python tools/loss_bench.py)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COPY_RATE_GBPS = 6290.0
OLD_SHAPE = (128, 1000, 1, 1)
RATE_SHAPES = ((32, 21, 64, 64), (8, 21, 500, 500))
NEW = ("hip_softmax_loss_fwd", "hip_loss_norm", "hip_softmax_loss_bck")
OLD = ("hip_softmax", "hip_sm_grad_and_loss", "hip_sum_loss_over_imgs")


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r23_loss.txt"))
    a = ap.parse_args(argv)
    import numpy as np
    import torch   # (before the package: see __graft_entry__._recompile_with_the_wheels_hiprtc; only asked whether there is a GPU)
    if not torch.cuda.is_available():
        raise SystemExit("loss_bench: no GPU")
    from boda_amd.bck_graph import LossSpec
    from boda_amd.cnn_op import OpTune, add_bck_op_annotations, loss_norm_func_op, pipe_func_args, softmax_loss_bck_func_op, softmax_loss_fwd_func_op
    from boda_amd.op import Dims, Nda, Op
    from boda_amd.rtc import RtcArg, RtcFuncCall, RtcFuncInfo, make_rtc
    rtc = make_rtc("(be=hip)", 0)
    rtc.init()
    lines = []
    for shape in (OLD_SHAPE,) + RATE_SHAPES:
        B, C, H, W = shape
        d = Dims.make("float", img=B, chan=C, y=H, x=W)
        plane, one, st = Dims.make("float", img=B, y=H, x=W), Dims.make("float", y=1, x=1), Dims(("v",), (4,), "float")
        rng = np.random.default_rng([B, C, H, W])
        lab = rng.integers(0, C, (B, H, W)).astype(np.float32)
        spec = LossSpec(0.3, 255 if shape != OLD_SHAPE else None, "valid")
        if spec.ignore_label is not None:
            lab[rng.uniform(size=lab.shape) < 0.3] = 255
        vars = {"lb_in": (d, rng.uniform(-4, 4, shape).astype(np.float32)), "lb_label": (plane, lab), "lb_prob": (d, None), "lb_lpp": (plane, None), "lb_loss": (one, None),
                "lb_state": (st, None), "lb_grad": (d, None)}
        funcs = [(softmax_loss_fwd_func_op(d, spec), {"in": "lb_in", "label": "lb_label", "prob": "lb_prob", "loss_per_pel": "lb_lpp"}),
                 (loss_norm_func_op(d, spec), {"label": "lb_label", "loss_per_pel": "lb_lpp", "loss": "lb_loss", "loss_state": "lb_state"}),
                 (softmax_loss_bck_func_op(d, spec), {"prob": "lb_prob", "label": "lb_label", "loss_state": "lb_state", "in_grad_loss": "lb_grad"})]
        if shape == OLD_SHAPE:   # the reference's three calls on the same logits and labels, into vars of their own
            vars.update({"lb_oprob": (d, None), "lb_olpp": (plane, None), "lb_oloss": (one, None), "lb_ograd": (d, None)})
            fs, fg, fl = add_bck_op_annotations(Op({"type": "SoftmaxWithLoss"}, {"in": Nda(d), "label": Nda(plane), "in_grad_loss": Nda(d), "loss": Nda(one)}), OpTune())
            funcs += [(fs, {"in": "lb_in", "prob": "lb_oprob"}), (fg, {"prob": "lb_oprob", "label": "lb_label", "in_grad_loss": "lb_ograd", "loss_per_pel": "lb_olpp"}),
                      (fl, {"loss_per_pel": "lb_olpp", "loss": "lb_oloss"})]
        for vn, (dd, v) in vars.items():
            rtc.create_var_with_dims(vn, dd)
            if v is not None:
                rtc.copy_nda_to_var(vn, v)
        calls = []
        for i, (f, args) in enumerate(funcs):
            sp = pipe_func_args(f)
            rtc.compile([RtcFuncInfo(f"lb_f{i}", "", [an for an, _ in sp], f)])
            calls.append((f.get_func_name(), RtcFuncCall(f"lb_f{i}", {an: RtcArg.var(args[an]) for an, _ in sp})))

        def block(n, keep):
            for fn, call in calls:
                ids = [rtc.run(call) for _ in range(n)]
                rtc.finish_and_sync()
                if keep is not None:
                    keep.setdefault(fn, []).append([1e3 * rtc.get_dur(i, i) for i in ids])
                rtc.release_per_call_id_data()
        block(a.warmup, None)
        keep = {}
        for _ in range(a.repeats):
            block(a.runs, keep)
        E, N = 4.0 * B * C * H * W, 4.0 * B * H * W
        nbytes = {"hip_softmax_loss_fwd": 2 * E + 2 * N, "hip_loss_norm": 2 * N, "hip_softmax_loss_bck": 2 * E + N}
        rec = {"shape": list(shape), "form": "pel" if H * W >= 64 else "wave", "tensor_MB": round(E / 1e6, 2), "copy_rate_GBps_recorded": COPY_RATE_GBPS}
        med = {fn: statistics.median([v for b in blocks for v in b]) for fn, blocks in keep.items()}
        for fn in NEW:
            rec[fn] = {"us": round(med[fn], 1), "GBps": round(nbytes[fn] / (med[fn] * 1e-6) / 1e9, 1), "block_medians_us": [round(statistics.median(b), 1) for b in keep[fn]]}
        rec["new_total_us"] = round(sum(med[fn] for fn in NEW), 1)
        if shape == OLD_SHAPE:
            for fn in OLD:
                rec[fn] = {"us": round(med[fn], 1), "block_medians_us": [round(statistics.median(b), 1) for b in keep[fn]]}
            tot = [sum(statistics.median(keep[fn][r]) for fn in OLD) for r in range(a.repeats)]
            rec["old_total_us"] = round(sum(med[fn] for fn in OLD), 1)
            rec["old_total_block_spread_us"] = round(max(tot) - min(tot), 1)
            rec["new_minus_old_us"] = round(rec["new_total_us"] - rec["old_total_us"], 1)
        rec["count"] = float(rtc.copy_var_to_nda("lb_state")[2]); rec["loss"] = float(rtc.copy_var_to_nda("lb_loss").item())
        print(json.dumps(rec), flush=True)
        lines.append(json.dumps(rec))
        for i in range(len(funcs)):
            rtc.release_func(f"lb_f{i}")
        for vn in vars:
            rtc.release_var(vn)
    rtc.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(f"# python tools/loss_bench.py --runs {a.runs} --warmup {a.warmup} --repeats {a.repeats}\n" + "\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
