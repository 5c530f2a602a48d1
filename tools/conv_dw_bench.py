"""Times the depthwise channels-last bf16 convolution (hip_conv_nhwc_dw; kernels/conv_nhwc_dw_bf16.hip) on MobileNet-v1's nine distinct depthwise shapes at 64 images,
and with --net the whole mobilenet_v1(64) forward pass as one graph replay.  With --fused: MobileNet-v1's nine distinct depthwise + pointwise pairs as ONE
hip_conv_nhwc_dw_pw launch (kernels/conv_nhwc_dwpw_bf16.hip) beside the sum of the two calls it replaces, and the whole net as one replay with fuse_dw_pw off, "all" and
True.  Needs the MI355X; not part of the suite.

    python tools/conv_dw_bench.py [--batch 64] [--runs 20] [--warmup 3] [--blocks 3] [--tile dw:TYxTXxCB | dwpw:TYxTXxCB] [--layers s1] [--net] [--fused]

Per layer one JSON line: the median us of the call and its launch, GB/s of the in + out bytes, and -- measured IN THE SAME PROCESS in alternating blocks (ours, torch,
copy, ours, ...) -- torch's channels-last bf16 conv2d(groups=C) with bias and ReLU, and a device-to-device copy of (in + out) / 2 bytes (it reads and writes as many
bytes as the layer reads and writes together): the rate the layer would run at if it were nothing but its traffic.  No figure is fixed in advance."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from boda_amd import conv_pipe  # noqa: E402
from boda_amd.cnn_op import NATIVE_ARGS, OpTune, add_codegen_annotations  # noqa: E402
from boda_amd.conv_pipe import ConvPipeFwd  # noqa: E402
from boda_amd.op import parse_op  # noqa: E402
from boda_amd.rtc import RtcArg, RtcFuncCall, RtcFuncInfo, make_rtc  # noqa: E402

SHAPES = [(32, 112, 1), (64, 112, 2), (128, 56, 1), (128, 56, 2), (256, 28, 1), (256, 28, 2), (512, 14, 1), (512, 14, 2), (1024, 7, 1)]   # (C, H = W, stride): 3 x 3, pad 1
TUNE = dict(hip_dtype="bf16", hip_layout="nhwc")


def dw_op(B, C, HW, s):
    O = (HW + 2 - 3) // s + 1
    return parse_op(f"(str_vals=(type=Convolution),nda_vals=(biases=(dims=(out_chan={C})),filts=(dims=(out_chan={C},in_chan=1,y=3,x=3)),group=(tn=uint32_t,v={C}),"
                    f"in=(dims=(img={B},chan={C},y={HW},x={HW})),in_pad=(tn=none,dims=(y=1,x=1)),kern_sz=(tn=none,dims=(y=3,x=3)),"
                    f"out=(dims=(img={B},chan={C},y={O},x={O})),out_chans=(tn=uint32_t,v={C}),stride=(tn=none,dims=(y={s},x={s}))))")


def bf16_bits(rng, sizes):
    return (rng.uniform(-1, 1, sizes).astype(np.float32).view(np.uint32) >> 16).astype(np.uint16)


def torch_us(fn, runs):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(runs)]
    for a, b in ev:
        a.record(); fn(); b.record()
    torch.cuda.synchronize()
    return [a.elapsed_time(b) * 1e3 for a, b in ev]


def bench_layer(rtc, B, C, HW, s, runs, warmup, blocks, tile):
    fop = add_codegen_annotations(dw_op(B, C, HW, s), OpTune(hip_tile=tile, **TUNE))
    rng = np.random.default_rng(C + HW + s)
    names = [an for an, io in NATIVE_ARGS[fop.get_func_name()] if io != "REF"]
    try:
        for an in names:
            d = fop.get_dims(an); rtc.create_var_with_dims("b_" + an, d)
            if an != "out":
                rtc.copy_nda_to_var("b_" + an, bf16_bits(rng, d.sizes) if d.tn == "bfloat16" else rng.uniform(-1, 1, d.sizes).astype(np.float32))
        rtc.compile([RtcFuncInfo("b_call", "", [a for a, _ in NATIVE_ARGS[fop.get_func_name()]], fop)])
        call = RtcFuncCall("b_call", {an: (RtcArg.ref(fop.get_dims(an)) if io == "REF" else RtcArg.var("b_" + an)) for an, io in NATIVE_ARGS[fop.get_func_name()]})
        x = torch.randn(B, C, HW, HW, device="cuda", dtype=torch.bfloat16).contiguous(memory_format=torch.channels_last)
        w = torch.randn(C, 1, 3, 3, device="cuda", dtype=torch.bfloat16).contiguous(memory_format=torch.channels_last); bias = torch.randn(C, device="cuda", dtype=torch.bfloat16)
        nbytes = fop.get_dims("in").bytes_sz() + fop.get_dims("out").bytes_sz()
        src = torch.empty(nbytes // 2, device="cuda", dtype=torch.uint8); dst = torch.empty_like(src)
        t_conv = lambda: torch.relu_(torch.nn.functional.conv2d(x, w, bias, stride=s, padding=1, groups=C))
        t_copy = lambda: dst.copy_(src)
        for _ in range(max(1, warmup)):
            rtc.run(call); t_conv(); t_copy()
        rtc.finish_and_sync(); torch.cuda.synchronize()
        launch = rtc.last_launch()
        ours, theirs, copy = [], [], []
        for _ in range(blocks):
            ids = [rtc.run(call) for _ in range(runs)]
            rtc.finish_and_sync()
            ours += [rtc.get_dur(i, i) * 1e3 for i in ids]; rtc.release_per_call_id_data()
            theirs += torch_us(t_conv, runs); copy += torch_us(t_copy, runs)
        us, tus, cus = statistics.median(ours), statistics.median(theirs), statistics.median(copy)
        return {"layer": f"dw{C}_{HW}_s{s}", "us": round(us, 1), "us_min_max": [round(min(ours), 1), round(max(ours), 1)], "kernel": launch["kernel"], "cfg": launch["cfg"], "grid": launch["grid"],
                "block": launch["block"], "in_out_bytes": nbytes, "gbs": round(nbytes / us / 1e3, 1), "copy_us": round(cus, 1), "copy_gbs": round(nbytes / cus / 1e3, 1),
                "frac_of_copy_rate": round(cus / us, 3), "torch_us": round(tus, 1), "torch_over_ours": round(tus / us, 2)}
    finally:
        rtc.finish_and_sync()
        for an in names:
            rtc.release_var("b_" + an)
        rtc.release_func("b_call"); rtc.release_per_call_id_data()


PAIRS = [(32, 112, 1, 64), (64, 112, 2, 128), (128, 56, 1, 128), (128, 56, 2, 256), (256, 28, 1, 256), (256, 28, 2, 512), (512, 14, 1, 512), (512, 14, 2, 1024), (1024, 7, 1, 1024)]   # (C, H = W, stride, OC)


def bench_pair(rtc, B, C, HW, s, OC, runs, warmup, blocks, tile):
    """One JSON row: the fused call beside the two calls it replaces (their device times added), same vars, one process, alternating blocks; the min / max of the
    unfused blocks' medians is the noise band a difference has to clear."""
    from boda_amd import nhwc
    O = (HW + 2 - 3) // s + 1
    da = add_codegen_annotations(dw_op(B, C, HW, s), OpTune(**TUNE))
    pa = add_codegen_annotations(parse_op(f"(str_vals=(type=Convolution),nda_vals=(biases=(dims=(out_chan={OC})),filts=(dims=(out_chan={OC},in_chan={C},y=1,x=1)),in=(dims=(img={B},chan={C},y={O},x={O})),"
                                          f"in_pad=(tn=none,dims=(y=0,x=0)),kern_sz=(tn=none,dims=(y=1,x=1)),out=(dims=(img={B},chan={OC},y={O},x={O})),out_chans=(tn=uint32_t,v={OC}),stride=(tn=none,dims=(y=1,x=1))))"), OpTune(**TUNE))
    fa = nhwc.annotate_dw_pw(da, pa, tile)
    rng = np.random.default_rng(C + HW + s)
    vars_ = {"p_in": da.get_dims("in"), "p_filts": da.get_dims("filts"), "p_biases": da.get_dims("biases"), "p_mid": da.get_dims("out"), "p_filts2": pa.get_dims("filts"),
             "p_biases2": pa.get_dims("biases"), "p_out": pa.get_dims("out"), "p_out_fused": pa.get_dims("out")}
    funcs = {"p_dw": da, "p_pw": pa, "p_fused": fa}
    try:
        for vn, d in vars_.items():
            rtc.create_var_with_dims(vn, d)
            if not vn.startswith(("p_mid", "p_out")):
                rtc.copy_nda_to_var(vn, bf16_bits(rng, d.sizes) if d.tn == "bfloat16" else rng.uniform(-1, 1, d.sizes).astype(np.float32))
        for fn, op in funcs.items():
            rtc.compile([RtcFuncInfo(fn, "", [a for a, _ in NATIVE_ARGS[op.get_func_name()]], op)])
        ref = lambda op: {"stride": RtcArg.ref(op.get_dims("stride")), "in_pad": RtcArg.ref(op.get_dims("in_pad"))}
        v = RtcArg.var
        c_dw = RtcFuncCall("p_dw", dict(ref(da), filts=v("p_filts"), biases=v("p_biases"), **{"in": v("p_in")}, out=v("p_mid")))
        c_pw = RtcFuncCall("p_pw", dict(ref(pa), filts=v("p_filts2"), biases=v("p_biases2"), **{"in": v("p_mid")}, out=v("p_out")))
        c_f = RtcFuncCall("p_fused", dict(ref(fa), filts=v("p_filts"), biases=v("p_biases"), filts2=v("p_filts2"), biases2=v("p_biases2"), **{"in": v("p_in")}, out=v("p_out_fused")))
        for _ in range(max(1, warmup)):
            rtc.run(c_dw); rtc.run(c_pw); rtc.run(c_f)
        rtc.finish_and_sync()
        launch = rtc.last_launch()
        same = float(np.mean(np.asarray(rtc.copy_var_to_nda("p_out")) == np.asarray(rtc.copy_var_to_nda("p_out_fused"))))   # (both round the same intermediate; the fp32 sums differ in order)
        two, dws, pws, one = [], [], [], []
        for _ in range(blocks):
            ids = [(rtc.run(c_dw), rtc.run(c_pw)) for _ in range(runs)]
            rtc.finish_and_sync()
            d = [rtc.get_dur(i, i) * 1e3 for i, _ in ids]; q = [rtc.get_dur(j, j) * 1e3 for _, j in ids]; rtc.release_per_call_id_data()
            dws.append(statistics.median(d)); pws.append(statistics.median(q)); two.append(statistics.median([x + y for x, y in zip(d, q)]))
            ids = [rtc.run(c_f) for _ in range(runs)]
            rtc.finish_and_sync()
            one.append(statistics.median([rtc.get_dur(i, i) * 1e3 for i in ids])); rtc.release_per_call_id_data()
        t2, t1 = statistics.median(two), statistics.median(one)
        io = vars_["p_in"].bytes_sz() + vars_["p_out"].bytes_sz() + vars_["p_filts"].bytes_sz() + vars_["p_filts2"].bytes_sz()
        return {"pair": f"dw{C}_{HW}_s{s}+pw{OC}", "two_calls_us": round(t2, 1), "dw_us": round(statistics.median(dws), 1), "pw_us": round(statistics.median(pws), 1),
                "two_calls_us_min_max": [round(min(two), 1), round(max(two), 1)], "fused_us": round(t1, 1), "fused_us_min_max": [round(min(one), 1), round(max(one), 1)],
                "fused_over_two": round(t1 / t2, 3), "wins_beyond_noise": bool(max(one) < min(two)), "kernel": launch["kernel"], "cfg": launch["cfg"], "grid": launch["grid"], "block": launch["block"],
                "bytes_fused": io, "bytes_two_calls": io + 2 * vars_["p_mid"].bytes_sz(), "equal_out_elems": round(same, 4)}
    finally:
        rtc.finish_and_sync()
        for vn in vars_:
            rtc.release_var(vn)
        for fn in funcs:
            rtc.release_func(fn)
        rtc.release_per_call_id_data()


def bench_net_fused(B, runs, warmup, blocks):
    """mobilenet_v1(B) as one graph replay under fuse_dw_pw off, "all" and True: three pipes (a backend instance each: their vars carry the net's names) in one
    process, their replays in alternating blocks."""
    pipes, rtcs = {}, []
    try:
        for mode in (False, "all", True):
            rtc = make_rtc("(be=hip)", 0); rtc.init(); rtcs.append(rtc)
            f = ConvPipeFwd(rtc, OpTune(**TUNE), fuse_dw_pw=mode); f.init(conv_pipe.mobilenet_v1(B)); pipes[str(mode)] = f
            for _ in range(max(1, warmup)):
                f.run_fwd_device_only()
            f.capture_graph()
            for _ in range(max(1, warmup)):
                f.run_graph()
        meds = {m: [] for m in pipes}
        for _ in range(blocks):
            for m, f in pipes.items():
                meds[m].append(statistics.median([f.run_graph() for _ in range(runs)]))
        return {"net": "mobilenet_v1", "batch": B, **{f"ms_fuse_{m}": round(statistics.median(v), 3) for m, v in meds.items()},
                **{f"ms_fuse_{m}_min_max": [round(min(v), 3), round(max(v), 3)] for m, v in meds.items()}, **{f"fused_pairs_{m}": len(f.fused_dw_pw) for m, f in pipes.items()}}
    finally:
        for f in pipes.values():
            f.release()
        for rtc in rtcs:
            rtc.close()


def bench_net(rtc, B, runs, warmup):
    f = ConvPipeFwd(rtc, OpTune(**TUNE)); f.init(conv_pipe.mobilenet_v1(B))
    try:
        for _ in range(max(1, warmup)):
            f.run_fwd_device_only()
        n = f.capture_graph()
        for _ in range(max(1, warmup)):
            f.run_graph()
        ms = [f.run_graph() for _ in range(runs)]
        m = statistics.median(ms)
        return {"net": "mobilenet_v1", "batch": B, "graph_calls": n, "dw_calls": sum(c.func == "hip_conv_nhwc_dw" for c in f.fwd_calls), "ms": round(m, 3),
                "ms_min_max": [round(min(ms), 3), round(max(ms), 3)], "img_per_s": round(B / m * 1e3, 0)}
    finally:
        f.release()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--batch", type=int, default=64); ap.add_argument("--runs", type=int, default=20); ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--blocks", type=int, default=3); ap.add_argument("--tile", default="", help="dw:TYxTXxCB: a forced work split (a comparison run)")
    ap.add_argument("--layers", default="", help="comma list: only the layers whose name contains one of these"); ap.add_argument("--net", action="store_true")
    ap.add_argument("--fused", action="store_true", help="the depthwise + pointwise pairs as one hip_conv_nhwc_dw_pw launch beside their two calls; --tile dwpw:TYxTXxCB forces the fused split")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("conv_dw_bench: no GPU: a time is measured on the MI355X or not at all")
    rtc = make_rtc("(be=hip)", 0); rtc.init()
    try:
        for C, HW, s, OC in (PAIRS if a.fused else []):
            if not a.layers or any(x in f"dw{C}_{HW}_s{s}" for x in a.layers.split(",")):
                print(json.dumps(dict(bench_pair(rtc, a.batch, C, HW, s, OC, a.runs, a.warmup, a.blocks, a.tile), **({"forced_tile": a.tile} if a.tile else {}))), flush=True)
        if a.fused and a.net:
            print(json.dumps(bench_net_fused(a.batch, a.runs, a.warmup, a.blocks)), flush=True)
        for C, HW, s in ([] if a.fused else SHAPES):
            if a.layers and not any(x in f"dw{C}_{HW}_s{s}" for x in a.layers.split(",")):
                continue
            print(json.dumps(dict(bench_layer(rtc, a.batch, C, HW, s, a.runs, a.warmup, a.blocks, a.tile), **({"forced_tile": a.tile} if a.tile else {}))), flush=True)
        if a.net and not a.fused:
            print(json.dumps(bench_net(rtc, a.batch, a.runs, a.warmup)), flush=True)
    finally:
        rtc.close()


if __name__ == "__main__":
    main()
