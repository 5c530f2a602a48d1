"""Times BckConv's two GEMM gradients on be=hip, layer by layer: AlexNet conv1-5 and NiN's convolutions at 256 images, GoogLeNet's at 64 (the layer tables of
bench.py).  Per layer and gradient one JSON line: us (median get_dur of --runs calls after --warmup), effective TF/s (2 M N K of the GEMM the gradient is --
data: M = img x in pels, N = in_chan, K = out_chan x taps of a phase; filter: M = out_chan, N = in_chan x KH x KW, K = img x out pels) and its fraction of the
fp32 MFMA roof.

    python tools/bck_conv_bench.py [--nets alexnet,nin,googlenet,resnet50] [--runs 10] [--warmup 3] [--layers N] [--batch B]

--fb: per layer (layers of one geometry once, with their count), the default pipe's pair hip_bconv_biases + hip_bconv_filts beside the one fused call
hip_bconv_filts_biases, in ONE process on the same vars, in --blocks alternating blocks of --runs calls each (pair, fused, pair, fused, ...): the median of the pair's
summed times, the median of the fused call's time (both its launches), their ratio, and both plans.

--bf16: per layer (layers of one geometry once, with their count), the fp32 call beside the same call with hip_operands=bf16 (cnn_op.bf16_operands), in ONE process
on the same vars, in --blocks alternating blocks of --runs calls each (fp32, bf16, fp32, bf16, ...): hip_bconv_in, and with --fb also hip_bconv_filts_biases.  Per call
one JSON line: the medians in us, their quotient bf16 / fp32, and the GB/s of the call's algorithmic bytes (fp32 tensors either way) beside the recorded 6.29 TB/s copy
rate.  The yardstick is the fp32 call of the same run; no figure is fixed in advance.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
from boda_amd import gen_data as gd  # noqa: E402
from boda_amd.cnn_op import NATIVE_ARGS, OpTune, add_bck_conv_annotations, bconv_filts_biases_func_op, bf16_operands  # noqa: E402
from boda_amd.op import parse_op  # noqa: E402
from boda_amd.ops_prof import OpsBackend, profile_rcg_call  # noqa: E402
from boda_amd.rtc import RtcArg, RtcFuncCall, RtcFuncInfo, make_rtc  # noqa: E402


def bck_of(conv):
    """The BckConv op of a forward Convolution op (same geometry; out becomes out_grad_loss, every input gets its gradient)."""
    s = conv.to_str().replace("type=Convolution", "type=BckConv").replace(",out=(", ",out_grad_loss=(")
    op = parse_op(s.replace("nda_vals=(", "nda_vals=(biases_grad_loss=" + conv.get("biases").to_str() + ",filts_grad_loss=" + conv.get("filts").to_str() +
                            ",in_grad_loss=" + conv.get("in").to_str() + ",", 1))
    op.bck_conv_geom()
    return op


def nets(names, batch=0):
    out = []
    for n in names:
        if n == "alexnet":
            out += [("alexnet", f"conv{i + 1}", op) for i, op in enumerate(bench.alexnet_b256_ops(*([batch] if batch else []))[:5])]
        elif n == "nin":
            out += [("nin", f"L{i}", op) for i, op in enumerate(bench.nin_ops(*([batch] if batch else [])))]
        elif n == "googlenet":
            out += [("googlenet", f"L{i}", op) for i, op in enumerate(bench.net_conv_ops("googlenet_conv", batch or 64))]
        elif n == "resnet50":
            out += [("resnet50", f"L{i}", op) for i, op in enumerate(bench.net_conv_ops("resnet-50", batch or 64))]
        else:
            raise SystemExit(f"unknown net {n!r}")
    return out


def time_pair_and_fused(rtc, op, runs, warmup, blocks):
    """-> (median us of hip_bconv_biases + hip_bconv_filts, median us of hip_bconv_filts_biases, the two launches) on device-generated inputs, alternating blocks."""
    _, fb_, ff = add_bck_conv_annotations(op, OpTune())
    fused = bconv_filts_biases_func_op(op, OpTune())
    made, funcs, calls = [], [], {}
    try:
        for an in ("in", "out_grad_loss", "filts_grad_loss", "biases_grad_loss"):
            rtc.create_var_with_dims("fb_" + an, op.get_dims(an)); made.append("fb_" + an)
        for an in ("in", "out_grad_loss"):
            rtc.run(gd.gen_call("BckConv", an, "fb_" + an, op.get_dims(an), 5, 0.0))
        for f in (fb_, ff, fused):
            fn = f.get_func_name()
            rtc.compile([RtcFuncInfo("fb_" + fn, "", [a for a, _ in NATIVE_ARGS[fn]], f)]); funcs.append("fb_" + fn)
            calls[fn] = RtcFuncCall("fb_" + fn, {an: (RtcArg.ref(f.get_dims(an)) if io == "REF" else RtcArg.var("fb_" + an)) for an, io in NATIVE_ARGS[fn]})
        launches = {}
        for fn in ("hip_bconv_filts", "hip_bconv_filts_biases"):
            for _ in range(warmup):
                rtc.run(calls[fn])
            launches[fn] = rtc.last_launch()
        rtc.run(calls["hip_bconv_biases"])
        pair, one = [], []
        for _ in range(blocks):
            ids = [(rtc.run(calls["hip_bconv_biases"]), rtc.run(calls["hip_bconv_filts"])) for _ in range(runs)]
            idf = [rtc.run(calls["hip_bconv_filts_biases"]) for _ in range(runs)]
            rtc.finish_and_sync()
            pair += [rtc.get_dur(b, b) + rtc.get_dur(f, f) for b, f in ids]
            one += [rtc.get_dur(i, i) for i in idf]
            rtc.release_per_call_id_data()
        return statistics.median(pair) * 1e3, statistics.median(one) * 1e3, launches
    finally:
        rtc.finish_and_sync()
        for vn in made:
            rtc.release_var(vn)
        for fn in funcs:
            rtc.release_func(fn)
        rtc.release_per_call_id_data()


COPY_GBS = 6290.0   # the recorded device-to-device copy rate


def time_f32_and_bf16(rtc, f32_fop, runs, warmup, blocks):
    """-> (median us of the fp32 call, median us of the same call with hip_operands=bf16, the two launches) on device-generated inputs, alternating blocks."""
    fn = f32_fop.get_func_name()
    fops = {"f32": f32_fop, "bf16": bf16_operands(f32_fop)}
    made, funcs, calls = [], [], {}
    try:
        for an, io in NATIVE_ARGS[fn]:
            if io != "REF":
                rtc.create_var_with_dims("ob_" + an, f32_fop.get_dims(an)); made.append("ob_" + an)
                if io == "IN":
                    rtc.run(gd.gen_call("BckConv", an, "ob_" + an, f32_fop.get_dims(an), 5, 0.0))
        for mode, f in fops.items():
            rtc.compile([RtcFuncInfo(f"ob_{mode}", "", [a for a, _ in NATIVE_ARGS[fn]], f)]); funcs.append(f"ob_{mode}")
            calls[mode] = RtcFuncCall(f"ob_{mode}", {an: (RtcArg.ref(f.get_dims(an)) if io == "REF" else RtcArg.var("ob_" + an)) for an, io in NATIVE_ARGS[fn]})
        launches = {}
        for mode in fops:
            for _ in range(max(1, warmup)):
                rtc.run(calls[mode])
            launches[mode] = rtc.last_launch()
        secs = {"f32": [], "bf16": []}
        for _ in range(blocks):
            ids = {mode: [rtc.run(calls[mode]) for _ in range(runs)] for mode in ("f32", "bf16")}
            rtc.finish_and_sync()
            for mode in ids:
                secs[mode] += [rtc.get_dur(i, i) for i in ids[mode]]
            rtc.release_per_call_id_data()
        return statistics.median(secs["f32"]) * 1e3, statistics.median(secs["bf16"]) * 1e3, launches
    finally:
        rtc.finish_and_sync()
        for vn in made:
            rtc.release_var(vn)
        for f in funcs:
            rtc.release_func(f)
        rtc.release_per_call_id_data()


def unique_layers(a):
    seen, layers = {}, []
    for net, name, conv in nets(a.nets.split(","), a.batch):
        key = (net, bck_of(conv).to_str())
        if key in seen:
            seen[key]["count"] += 1; continue
        seen[key] = {"net": net, "layer": name, "op": bck_of(conv), "count": 1}
        layers.append(seen[key])
    return layers


def main_bf16(a):
    rtc = make_rtc("(be=hip)", 0)
    rtc.init()
    OpsBackend(rtc)   # (compiles the input generators)
    per_net = {}
    for L in unique_layers(a):
        per_net[L["net"]] = per_net.get(L["net"], 0) + 1
        if a.layers and per_net[L["net"]] > a.layers:
            continue
        op = L["op"]; g = op.bck_conv_geom()
        fops = [("data", add_bck_conv_annotations(op, OpTune())[0])] + ([("filts_biases", bconv_filts_biases_func_op(op, OpTune()))] if a.fb else [])
        for grad, f in fops:
            f32_us, bf16_us, lch = time_f32_and_bf16(rtc, f, a.runs, a.warmup, a.blocks)
            by = lch["bf16"]["algo_bytes"]
            print(json.dumps({"net": L["net"], "layer": L["layer"], "count": L["count"], "grad": grad, "B": g["B"], "C": g["C"], "HW": g["H"], "OC": g["OC"], "k": g["KH"], "s": g["SY"],
                              "f32_us": round(f32_us, 2), "bf16_us": round(bf16_us, 2), "bf16_over_f32": round(bf16_us / f32_us, 3),
                              "f32_gbs": round(by / (f32_us * 1e-6) / 1e9, 1), "bf16_gbs": round(by / (bf16_us * 1e-6) / 1e9, 1), "copy_gbs": COPY_GBS,
                              "bf16_tflops": round(lch["bf16"]["flops"] / (bf16_us * 1e-6) / 1e12, 2),
                              "f32_cfg": str(lch["f32"].get("cfg", "")), "bf16_cfg": str(lch["bf16"].get("cfg", "")), "bf16_kernel": lch["bf16"]["kernel"]}), flush=True)
    rtc.close()


def main_fb(a):
    rtc = make_rtc("(be=hip)", 0)
    rtc.init()
    OpsBackend(rtc)   # (compiles the input generators)
    seen = {}
    layers = []
    for net, name, conv in nets(a.nets.split(","), a.batch):
        key = (net, bck_of(conv).to_str())
        if key in seen:
            seen[key]["count"] += 1; continue
        seen[key] = {"net": net, "layer": name, "op": bck_of(conv), "count": 1}
        layers.append(seen[key])
    for L in layers:
        op = L["op"]; g = op.bck_conv_geom()
        pair_us, fused_us, lch = time_pair_and_fused(rtc, op, a.runs, a.warmup, a.blocks)
        flops = lch["hip_bconv_filts_biases"]["flops"]
        print(json.dumps({"net": L["net"], "layer": L["layer"], "count": L["count"], "B": g["B"], "C": g["C"], "HW": g["H"], "OC": g["OC"], "k": g["KH"], "s": g["SY"],
                          "pair_us": round(pair_us, 2), "fused_us": round(fused_us, 2), "fused_over_pair": round(fused_us / pair_us, 3),
                          "fused_tflops": round(flops / (fused_us * 1e-6) / 1e12, 2), "fused_roof_frac": round(flops / (fused_us * 1e-6) / 1e12 / bench.PEAK_FP32_MFMA_TFLOPS, 3),
                          "pair_cfg": str(lch["hip_bconv_filts"].get("cfg", "")), "fused_cfg": str(lch["hip_bconv_filts_biases"].get("cfg", "")),
                          "fused_grid": lch["hip_bconv_filts_biases"].get("grid", 0)}), flush=True)
    rtc.close()


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--nets", default="alexnet,nin,googlenet")
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--layers", type=int, default=0, help="at most this many layers per net (0: all)")
    ap.add_argument("--batch", type=int, default=0, help="images per layer (0: the layer tables' own batches)")
    ap.add_argument("--fb", action="store_true", help="the pair hip_bconv_biases + hip_bconv_filts beside hip_bconv_filts_biases, in alternating blocks")
    ap.add_argument("--blocks", type=int, default=4, help="--fb / --bf16: alternating blocks of --runs calls each")
    ap.add_argument("--bf16", action="store_true", help="the fp32 call beside the hip_operands=bf16 call, in alternating blocks: hip_bconv_in, and with --fb hip_bconv_filts_biases")
    a = ap.parse_args(argv)
    if a.bf16:
        return main_bf16(a)
    if a.fb:
        return main_fb(a)
    rtc = make_rtc("(be=hip)", 0)
    rtc.init()
    be = OpsBackend(rtc)
    per_net = {}
    for net, name, conv in nets(a.nets.split(","), a.batch):
        per_net[net] = per_net.get(net, 0) + 1
        if a.layers and per_net[net] > a.layers:
            continue
        op = bck_of(conv)
        g = op.bck_conv_geom()
        fi, _, ff = add_bck_conv_annotations(op, OpTune())
        for grad, f in (("data", fi), ("filts", ff)):
            _, prc = profile_rcg_call(be, f, 5, run_iter=a.warmup + a.runs, want_outs=False)
            us = statistics.median(prc.all_secs[a.warmup:]) * 1e6
            flops = prc.launch["flops"]
            tfs = flops / (us * 1e-6) / 1e12
            print(json.dumps({"net": net, "layer": name, "grad": grad, "B": g["B"], "C": g["C"], "HW": g["H"], "OC": g["OC"], "k": g["KH"], "s": g["SY"],
                              "us": round(us, 2), "tflops": round(tfs, 2), "roof_frac": round(tfs / bench.PEAK_FP32_MFMA_TFLOPS, 3),
                              "kernel": prc.launch["kernel"], "cfg": str(prc.launch.get("cfg", ""))}), flush=True)
    rtc.close()


if __name__ == "__main__":
    main()
