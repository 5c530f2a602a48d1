"""Times the depthwise channels-last bf16 convolution (hip_conv_nhwc_dw; kernels/conv_nhwc_dw_bf16.hip) on MobileNet-v1's nine distinct depthwise shapes at 64 images,
and with --net the whole mobilenet_v1(64) forward pass as one graph replay.  Needs the MI355X; not part of the suite.

    python tools/conv_dw_bench.py [--batch 64] [--runs 20] [--warmup 3] [--blocks 3] [--tile dw:TYxTXxCB] [--layers s1] [--net]

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
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("conv_dw_bench: no GPU: a time is measured on the MI355X or not at all")
    rtc = make_rtc("(be=hip)", 0); rtc.init()
    try:
        for C, HW, s in SHAPES:
            if a.layers and not any(x in f"dw{C}_{HW}_s{s}" for x in a.layers.split(",")):
                continue
            print(json.dumps(dict(bench_layer(rtc, a.batch, C, HW, s, a.runs, a.warmup, a.blocks, a.tile), **({"forced_tile": a.tile} if a.tile else {}))), flush=True)
        if a.net:
            print(json.dumps(bench_net(rtc, a.batch, a.runs, a.warmup)), flush=True)
    finally:
        rtc.close()


if __name__ == "__main__":
    main()
