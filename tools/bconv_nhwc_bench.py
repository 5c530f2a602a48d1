"""Times hip_bconv_fb_nhwc (kernels/bconv_fb_nhwc_bf16.hip), the filter and bias gradient from channels-last bf16 tensors, on ResNet-50's distinct convolution shapes at
32 images, beside the yardstick of the same run: hip_bconv_filts_biases with hip_operands=bf16 on the same values as fp32 tensors in the reference layouts.  Needs
the MI355X; not part of the suite.

    python tools/bconv_nhwc_bench.py [--batch 32] [--runs 10] [--warmup 2] [--blocks 3] [--tile fbn:BIxBJxBKxKSL[xXB]] [--layers 3x3]

One process, alternating blocks (new, old, new, ...).  Per layer one JSON line: the median us of each call (its launches together, device events around the call), TF/s
from 2 K OC C KH KW, GB/s from the call's algorithmic bytes (new: the two bf16 operands once and the fp32 outputs; old: the same tensors in fp32) beside the recorded
copy rate of 6.29 TB/s, and old / new.  The stem (in.chan = 3) is outside the new function's scope and is not in the list.  No ratio is fixed in advance."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from boda_amd import nhwc  # noqa: E402
from boda_amd.cnn_op import NATIVE_ARGS, OpTune, bconv_filts_biases_func_op, bf16_operands  # noqa: E402
from boda_amd.op import parse_op  # noqa: E402
from boda_amd.rtc import RtcArg, RtcFuncCall, RtcFuncInfo, make_rtc  # noqa: E402

COPY_TBS = 6.29
# (C, OC, H = W of in, kernel, stride, pad): ResNet-50's distinct convolutions behind the stem, and the classifier as a 1 x 1 convolution
SHAPES = [(64, 64, 56, 1, 1, 0), (64, 64, 56, 3, 1, 1), (64, 256, 56, 1, 1, 0), (256, 64, 56, 1, 1, 0), (256, 128, 56, 1, 2, 0), (256, 512, 56, 1, 2, 0),
          (128, 128, 28, 3, 1, 1), (128, 512, 28, 1, 1, 0), (512, 128, 28, 1, 1, 0), (512, 256, 28, 1, 2, 0), (512, 1024, 28, 1, 2, 0),
          (256, 256, 14, 3, 1, 1), (256, 1024, 14, 1, 1, 0), (1024, 256, 14, 1, 1, 0), (1024, 512, 14, 1, 2, 0), (1024, 2048, 14, 1, 2, 0),
          (512, 512, 7, 3, 1, 1), (512, 2048, 7, 1, 1, 0), (2048, 512, 7, 1, 1, 0), (2048, 1000, 1, 1, 1, 0)]


def bck_op(B, C, OC, HW, K, S, P):
    O = (HW + 2 * P - K) // S + 1
    return parse_op(f"(str_vals=(type=BckConv),nda_vals=(biases=(dims=(out_chan={OC})),biases_grad_loss=(dims=(out_chan={OC})),filts=(dims=(out_chan={OC},in_chan={C},y={K},x={K})),"
                    f"filts_grad_loss=(dims=(out_chan={OC},in_chan={C},y={K},x={K})),in=(dims=(img={B},chan={C},y={HW},x={HW})),in_grad_loss=(dims=(img={B},chan={C},y={HW},x={HW})),"
                    f"in_pad=(tn=none,dims=(y={P},x={P})),kern_sz=(tn=none,dims=(y={K},x={K})),out_chans=(tn=uint32_t,v={OC}),out_grad_loss=(dims=(img={B},chan={OC},y={O},x={O})),"
                    f"stride=(tn=none,dims=(y={S},x={S}))))")


def bench_layer(rtc, B, shape, runs, warmup, blocks, tile):
    C, OC, HW, K, S, P = shape
    bare = bck_op(B, C, OC, HW, K, S, P)
    fops = {"new": nhwc.annotate_bconv_fb(bare, tile), "old": bf16_operands(bconv_filts_biases_func_op(bare, OpTune()))}
    rng = np.random.default_rng(C + OC + HW)
    vals = {an: (rng.uniform(-1, 1, bare.get_dims(an).sizes).astype(np.float32).view(np.uint32) & 0xffff0000).view(np.float32) for an in ("in", "out_grad_loss")}   # bf16 values, img:chan:y:x
    calls, made = {}, []
    try:
        for which, fop in fops.items():
            args = NATIVE_ARGS[fop.get_func_name()]
            for an, io in args:
                if io == "REF":
                    continue
                vn = f"{which}_{an}"; rtc.create_var_with_dims(vn, fop.get_dims(an)); made.append(vn)
                if io == "IN":
                    rtc.copy_nda_to_var(vn, vals[an] if which == "old" else (np.ascontiguousarray(vals[an].transpose(0, 2, 3, 1)).view(np.uint32) >> 16).astype(np.uint16))
            rtc.compile([RtcFuncInfo(which + "_call", "", [a for a, _ in args], fop)])
            calls[which] = RtcFuncCall(which + "_call", {an: (RtcArg.ref(fop.get_dims(an)) if io == "REF" else RtcArg.var(f"{which}_{an}")) for an, io in args})
        info = {}
        for which in calls:
            for _ in range(max(1, warmup)):
                rtc.run(calls[which])
            rtc.finish_and_sync(); info[which] = rtc.last_launch()
        new_f = np.asarray(rtc.copy_var_to_nda("new_filts_grad_loss")).transpose(0, 3, 1, 2).astype(np.float64); old_f = np.asarray(rtc.copy_var_to_nda("old_filts_grad_loss")).astype(np.float64)
        us = {"new": [], "old": []}
        for _ in range(blocks):
            for which in ("new", "old"):
                ids = [rtc.run(calls[which]) for _ in range(runs)]
                rtc.finish_and_sync()
                us[which] += [rtc.get_dur(i, i) * 1e3 for i in ids]; rtc.release_per_call_id_data()
        row = {"layer": f"{C}->{OC} {HW}x{HW} k{K} s{S}", "max_abs_diff_over_max_abs": float(np.abs(new_f - old_f).max() / max(np.abs(old_f).max(), 1e-30))}
        for which in ("new", "old"):
            m, li = statistics.median(us[which]), info[which]
            row[which] = {"us": round(m, 1), "us_min_max": [round(min(us[which]), 1), round(max(us[which]), 1)], "tfs": round(info["new"]["flops"] / m / 1e6, 1),
                          "gbs": round(li["algo_bytes"] / m / 1e3, 1), "frac_of_copy_rate": round(li["algo_bytes"] / m / 1e3 / (COPY_TBS * 1e3), 3), "kernel": li["kernel"], "cfg": li["cfg"], "grid": li["grid"]}
        row["old_over_new"] = round(row["old"]["us"] / row["new"]["us"], 2); row["new_is_slower"] = row["old_over_new"] < 1.0
        return row
    finally:
        rtc.finish_and_sync()
        for vn in made:
            rtc.release_var(vn)
        for which in calls:
            rtc.release_func(which + "_call")
        rtc.release_per_call_id_data()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32); ap.add_argument("--runs", type=int, default=10); ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--blocks", type=int, default=3); ap.add_argument("--tile", default=""); ap.add_argument("--layers", default="")
    a = ap.parse_args()
    rtc = make_rtc("(be=hip)", 0); rtc.init()
    try:
        for shape in SHAPES:
            if a.layers and a.layers not in f"{shape[3]}x{shape[3]}":
                continue
            print(json.dumps(bench_layer(rtc, a.batch, shape, a.runs, a.warmup, a.blocks, a.tile)), flush=True)
    finally:
        rtc.close()


if __name__ == "__main__":
    main()
