"""Times the training-BatchNorm functions (boda_amd/csrc/kernels/bn_f32.hip) on be=hip at the nine distinct BatchNorm shapes of ResNet-50 at
224 x 224 and --batch images (default 64), beside torch.nn.functional.batch_norm(training=True) and its autograd backward on fp32 NCHW tensors of the same shapes
and values, in the SAME process, in --repeats alternating blocks of --runs calls (after --warmup calls of everything).

Per shape one JSON line: per function the median microseconds of a call (device events around the call: a call of hip_bn_stats is three launches, of hip_bn_bck_sums
two) and GB/s from the algorithmic bytes (every tensor of the call once: stats 1, fwd 2, bck_sums 2, bck_in 3 tensor passes), the medians of the single blocks (their
spread is what a difference has to beat), and the yardstick: torch's forward (our stats + fwd) and backward (our bck_sums + bck_in) in microseconds with the same
byte counts.  The copy rate profiles/ records for this device is 6.29 TB/s.  No figure is required: the first record is the baseline.
Both sides are timed alike: a block of --runs calls is enqueued back to back and synchronised once, a call's time is the device time between the events around it.
Where the device finishes a call sooner than the host enqueues the next -- torch's Python-level forward and autograd on the small maps -- the interval between two events
still holds the wait for the host: such a figure is a dispatch time, not a kernel time, and each JSON line says which of torch's two figures do not grow with the tensor
("torch_host_bound": true where torch's time on this shape is within 15 % of its time on the smallest shape, which itself is not judged: null).

    python tools/bn_bench.py [--batch 64] [--runs 20] [--warmup 5] [--repeats 3] [--out profiles/r14_bn_train.txt]

--frozen: instead, the backward pass of a BatchNorm on its running pair -- hip_bnf_bck, ONE pass over in and out_grad_loss that leaves both sums
and dx (3 tensor passes) -- beside the training BatchNorm's hip_bn_bck_sums + hip_bn_bck_in (5) on the same vars, per shape in microseconds and GB/s beside the recorded
copy rate, in the same alternating blocks; no torch side.  The records are APPENDED to --out (default profiles/r22_freeze.txt) under a comment line with the command.
    python tools/bn_bench.py --frozen [--batch 32]

A measurement path that finds no GPU fails.  Run it under a time limit (timeout -k 10 600 python tools/bn_bench.py)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COPY_RATE_GBPS = 6290.0
PASSES = {"hip_bn_stats": 1, "hip_bn_fwd": 2, "hip_bn_bck_sums": 2, "hip_bn_bck_in": 3, "hip_bnf_bck": 3}


def bn_shapes(batch):
    """The distinct (img, chan, y, x) a BatchNorm of ResNet-50 works on, in net order."""
    from boda_amd import conv_pipe
    cp = conv_pipe.resnet50(batch)
    out = []
    for o in cp.ops:
        if o.type == "BatchNorm":
            s = tuple(cp.nodes[o.bot].sizes)
            if s not in out:
                out.append(s)
    return out


def frozen_main(a):
    """--frozen: hip_bnf_bck beside hip_bn_bck_sums + hip_bn_bck_in, one process, alternating blocks."""
    import numpy as np
    import torch   # (before the package, as in main; only asked whether there is a GPU)
    if not torch.cuda.is_available():
        raise SystemExit("bn_bench: no GPU")
    from boda_amd.cnn_op import bn_bck_in_func_op, bn_bck_sums_func_op, bnf_bck_func_op, bnf_prep_func_op, pipe_func_args
    from boda_amd.op import Dims
    from boda_amd.rtc import RtcArg, RtcFuncCall, RtcFuncInfo, make_rtc
    rtc = make_rtc("(be=hip)", 0)
    rtc.init()
    lines = []
    for shape in bn_shapes(a.batch):
        B, C, H, W = shape
        d = Dims.make("float", img=B, chan=C, y=H, x=W)
        ch = Dims(("chan",), (C,), "float")
        rng = np.random.default_rng([B, C, H, W])
        vals = {"bb_x": rng.standard_normal(shape, dtype=np.float32) * 1.5 + 0.4, "bb_dy": rng.standard_normal(shape, dtype=np.float32), "bb_dx": None, "bb_dxf": None}
        chans = {"bb_rm": rng.uniform(-1, 1, C).astype(np.float32), "bb_rv": rng.uniform(0.5, 2, C).astype(np.float32), "bb_mean": None, "bb_istd": None,
                 "bb_scale": rng.uniform(0.5, 1.5, C).astype(np.float32), "bb_sg": None, "bb_bg": None, "bb_sgf": None, "bb_bgf": None}
        for vs, dd in ((vals, d), (chans, ch)):
            for vn, v in vs.items():
                rtc.create_var_with_dims(vn, dd)
                if v is not None:
                    rtc.copy_nda_to_var(vn, v)
        common = {"in": "bb_x", "mean": "bb_mean", "inv_std": "bb_istd"}
        funcs = [(bnf_prep_func_op(d, 1e-5), {"run_mean": "bb_rm", "run_var": "bb_rv", "mean": "bb_mean", "inv_std": "bb_istd"}),
                 (bn_bck_sums_func_op(d), dict(common, out_grad_loss="bb_dy", scale_grad_loss="bb_sg", bias_grad_loss="bb_bg")),
                 (bn_bck_in_func_op(d), dict(common, scale="bb_scale", scale_grad_loss="bb_sg", bias_grad_loss="bb_bg", out_grad_loss="bb_dy", in_grad_loss="bb_dx")),
                 (bnf_bck_func_op(d), dict(common, scale="bb_scale", out_grad_loss="bb_dy", in_grad_loss="bb_dxf", scale_grad_loss="bb_sgf", bias_grad_loss="bb_bgf"))]
        calls = []
        for i, (f, args) in enumerate(funcs):
            spec = pipe_func_args(f)
            rtc.compile([RtcFuncInfo(f"bb_f{i}", "", [an for an, _ in spec], f)])
            calls.append((f.get_func_name(), RtcFuncCall(f"bb_f{i}", {an: RtcArg.var(args[an]) for an, _ in spec})))
        rtc.run(calls[0][1]); rtc.finish_and_sync(); rtc.release_per_call_id_data()     # mean / inv_std from the running pair, once

        def block(n, keep):
            for fn, call in calls[1:]:
                ids = [rtc.run(call) for _ in range(n)]
                rtc.finish_and_sync()
                if keep is not None:
                    keep.setdefault(fn, []).append([1e3 * rtc.get_dur(i, i) for i in ids])
                rtc.release_per_call_id_data()
        block(a.warmup, None)
        keep = {}
        for _ in range(a.repeats):
            block(a.runs, keep)
        T = 4.0 * B * C * H * W
        rec = {"shape": list(shape), "tensor_MB": round(T / 1e6, 2), "copy_rate_GBps_recorded": COPY_RATE_GBPS}
        med = {}
        for fn, blocks in keep.items():
            med[fn] = statistics.median([v for b in blocks for v in b])
            rec[fn] = {"us": round(med[fn], 1), "GBps": round(PASSES[fn] * T / (med[fn] * 1e-6) / 1e9, 1), "block_medians_us": [round(statistics.median(b), 1) for b in blocks]}
        rec["frozen_over_training_bwd"] = round(med["hip_bnf_bck"] / (med["hip_bn_bck_sums"] + med["hip_bn_bck_in"]), 3)
        # the same sums bit for bit (one chain on the same mean / inv_std)
        rec["sums_equal_bits"] = bool(np.array_equal(rtc.copy_var_to_nda("bb_sg").view(np.uint32), rtc.copy_var_to_nda("bb_sgf").view(np.uint32)) and
                                      np.array_equal(rtc.copy_var_to_nda("bb_bg").view(np.uint32), rtc.copy_var_to_nda("bb_bgf").view(np.uint32)))
        print(json.dumps(rec), flush=True)
        lines.append(json.dumps(rec))
        for i in range(len(funcs)):
            rtc.release_func(f"bb_f{i}")
        for vn in list(vals) + list(chans):
            rtc.release_var(vn)
    rtc.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(f"# python tools/bn_bench.py --frozen --batch {a.batch} --runs {a.runs} --warmup {a.warmup} --repeats {a.repeats}\n" + "\n".join(lines) + "\n")
    return 0


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--frozen", action="store_true", help="time hip_bnf_bck beside hip_bn_bck_sums + hip_bn_bck_in instead")
    a = ap.parse_args(argv)
    a.out = a.out or os.path.join(ROOT, "profiles", "r22_freeze.txt" if a.frozen else "r14_bn_train.txt")
    if a.frozen:
        return frozen_main(a)
    import numpy as np
    import torch   # (before the package: see __graft_entry__._recompile_with_the_wheels_hiprtc)
    import torch.nn.functional as F
    if not torch.cuda.is_available():
        raise SystemExit("bn_bench: no GPU")
    from boda_amd.cnn_op import bn_bck_in_func_op, bn_bck_sums_func_op, bn_fwd_func_op, bn_stats_func_op, pipe_func_args
    from boda_amd.op import Dims
    from boda_amd.rtc import RtcArg, RtcFuncCall, RtcFuncInfo, make_rtc
    rtc = make_rtc("(be=hip)", 0)
    rtc.init()
    eps, maf = 1e-5, 0.999
    lines, recs = [], []
    for shape in bn_shapes(a.batch):
        B, C, H, W = shape
        d = Dims.make("float", img=B, chan=C, y=H, x=W)
        ch = Dims(("chan",), (C,), "float")
        rng = np.random.default_rng([B, C, H, W])
        x = (rng.standard_normal(shape, dtype=np.float32) * 1.5 + 0.4); dy = rng.standard_normal(shape, dtype=np.float32)
        scale = rng.uniform(0.5, 1.5, C).astype(np.float32); bias = rng.uniform(-0.5, 0.5, C).astype(np.float32)
        tens = {"bb_x": x, "bb_dy": dy, "bb_out": None, "bb_dx": None}
        chans = {"bb_mean": None, "bb_istd": None, "bb_rm": np.zeros(C, np.float32), "bb_rv": np.ones(C, np.float32), "bb_scale": scale, "bb_bias": bias, "bb_sg": None, "bb_bg": None}
        for vn, v in tens.items():
            rtc.create_var_with_dims(vn, d)
            if v is not None:
                rtc.copy_nda_to_var(vn, v)
        for vn, v in chans.items():
            rtc.create_var_with_dims(vn, ch)
            if v is not None:
                rtc.copy_nda_to_var(vn, v)
        common = {"in": "bb_x", "mean": "bb_mean", "inv_std": "bb_istd"}
        funcs = [(bn_stats_func_op(d, eps, maf), dict(common, run_mean="bb_rm", run_var="bb_rv")),
                 (bn_fwd_func_op(d, 0), dict(common, scale="bb_scale", bias="bb_bias", out="bb_out")),
                 (bn_bck_sums_func_op(d), dict(common, out_grad_loss="bb_dy", scale_grad_loss="bb_sg", bias_grad_loss="bb_bg")),
                 (bn_bck_in_func_op(d), dict(common, scale="bb_scale", scale_grad_loss="bb_sg", bias_grad_loss="bb_bg", out_grad_loss="bb_dy", in_grad_loss="bb_dx"))]
        calls = []
        for i, (f, args) in enumerate(funcs):
            spec = pipe_func_args(f)
            rtc.compile([RtcFuncInfo(f"bb_f{i}", "", [an for an, _ in spec], f)])
            calls.append((f.get_func_name(), RtcFuncCall(f"bb_f{i}", {an: RtcArg.var(args[an]) for an, _ in spec})))
        tx = torch.from_numpy(x).cuda().requires_grad_(True); tdy = torch.from_numpy(dy).cuda()
        tw = torch.from_numpy(scale).cuda().requires_grad_(True); tb = torch.from_numpy(bias).cuda().requires_grad_(True)
        trm = torch.zeros(C, device="cuda"); trv = torch.ones(C, device="cuda")
        ev = lambda: torch.cuda.Event(enable_timing=True)

        def ours(n, keep):
            for fn, call in calls:
                ids = [rtc.run(call) for _ in range(n)]
                rtc.finish_and_sync()
                if keep is not None:
                    keep.setdefault(fn, []).append([1e3 * rtc.get_dur(i, i) for i in ids])
                rtc.release_per_call_id_data()

        def theirs(n, keep):     # timed like ours: the whole block is enqueued back to back, events between the calls, ONE synchronise at its end
            evs = []
            for _ in range(n):
                e0, e1, e2 = ev(), ev(), ev()
                e0.record()
                y = F.batch_norm(tx, trm, trv, tw, tb, training=True, momentum=1.0 - maf, eps=eps)
                e1.record()
                torch.autograd.grad(y, (tx, tw, tb), tdy)
                e2.record()
                evs.append((e0, e1, e2))
            torch.cuda.synchronize()
            fw = [1e3 * e0.elapsed_time(e1) for e0, e1, _ in evs]; bw = [1e3 * e1.elapsed_time(e2) for _, e1, e2 in evs]
            if keep is not None:
                keep.setdefault("torch_fwd", []).append(fw); keep.setdefault("torch_bwd", []).append(bw)
        ours(a.warmup, None); theirs(a.warmup, None)
        keep = {}
        for _ in range(a.repeats):
            ours(a.runs, keep); theirs(a.runs, keep)
        T = 4.0 * B * C * H * W
        rec = {"shape": list(shape), "tensor_MB": round(T / 1e6, 2), "copy_rate_GBps_recorded": COPY_RATE_GBPS}
        med = {}
        for fn, blocks in keep.items():
            med[fn] = statistics.median([v for b in blocks for v in b])
            passes = PASSES.get(fn, 2 if fn == "torch_fwd" else 5)   # (torch is given our byte counts: the forward our stats + fwd = 3 passes would flatter it, so 2 -- x read once, y written --; the backward our two functions' 5)
            rec[fn] = {"us": round(med[fn], 1), "GBps": round(passes * T / (med[fn] * 1e-6) / 1e9, 1), "block_medians_us": [round(statistics.median(b), 1) for b in blocks]}
        rec["fwd_ours_over_torch"] = round((med["hip_bn_stats"] + med["hip_bn_fwd"]) / med["torch_fwd"], 3)
        rec["bwd_ours_over_torch"] = round((med["hip_bn_bck_sums"] + med["hip_bn_bck_in"]) / med["torch_bwd"], 3)
        # same results: the batch statistics and dx of the two, at the sizes timed (different summation orders: last bits)
        got_dx = rtc.copy_var_to_nda("bb_dx")
        tgx = torch.autograd.grad(F.batch_norm(tx, None, None, tw, tb, training=True, eps=eps), (tx,), tdy)[0].cpu().numpy()
        y = rtc.copy_var_to_nda("bb_out")
        ty = F.batch_norm(tx, None, None, tw, tb, training=True, eps=eps).detach().cpu().numpy()
        rec["out_max_abs_dev_vs_torch"] = float(np.max(np.abs(y - ty)))
        rec["dx_max_abs_dev_vs_torch"] = float(np.max(np.abs(got_dx - tgx)))
        recs.append(rec)
        for i in range(len(funcs)):
            rtc.release_func(f"bb_f{i}")
        for vn in list(tens) + list(chans):
            rtc.release_var(vn)
        del tx, tdy, tw, tb, y, ty, tgx
        torch.cuda.empty_cache()
    rtc.close()
    # a torch figure that does not grow with the tensor is host dispatch, not device time: flag it against the smallest shape's
    small = min(recs, key=lambda r: r["tensor_MB"])
    for rec in recs:
        for k in ("torch_fwd", "torch_bwd"):
            rec[k]["torch_host_bound"] = None if rec is small else bool(rec[k]["us"] <= 1.15 * small[k]["us"])     # (None: the smallest shape has nothing to be held against)
        print(json.dumps(rec), flush=True)
        lines.append(json.dumps(rec))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(f"# python tools/bn_bench.py --batch {a.batch} --runs {a.runs} --warmup {a.warmup} --repeats {a.repeats}\n" + "\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main() or 0)
