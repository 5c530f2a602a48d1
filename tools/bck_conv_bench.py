"""Times BckConv's two GEMM gradients on be=hip, layer by layer: AlexNet conv1-5 and NiN's convolutions at 256 images, GoogLeNet's at 64 (the layer tables of
bench.py).  Per layer and gradient one JSON line: us (median get_dur of --runs calls after --warmup), effective TF/s (2 M N K of the GEMM the gradient is --
data: M = img x in pels, N = in_chan, K = out_chan x taps of a phase; filter: M = out_chan, N = in_chan x KH x KW, K = img x out pels) and its fraction of the
fp32 MFMA roof.

    python tools/bck_conv_bench.py [--nets alexnet,nin,googlenet] [--runs 10] [--warmup 3] [--layers N]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
from boda_amd.cnn_op import OpTune, add_bck_conv_annotations  # noqa: E402
from boda_amd.op import parse_op  # noqa: E402
from boda_amd.ops_prof import OpsBackend, profile_rcg_call  # noqa: E402
from boda_amd.rtc import make_rtc  # noqa: E402


def bck_of(conv):
    """The BckConv op of a forward Convolution op (same geometry; out becomes out_grad_loss, every input gets its gradient)."""
    s = conv.to_str().replace("type=Convolution", "type=BckConv").replace(",out=(", ",out_grad_loss=(")
    op = parse_op(s.replace("nda_vals=(", "nda_vals=(biases_grad_loss=" + conv.get("biases").to_str() + ",filts_grad_loss=" + conv.get("filts").to_str() +
                            ",in_grad_loss=" + conv.get("in").to_str() + ",", 1))
    op.bck_conv_geom()
    return op


def nets(names):
    out = []
    for n in names:
        if n == "alexnet":
            out += [("alexnet", f"conv{i + 1}", op) for i, op in enumerate(bench.alexnet_b256_ops()[:5])]
        elif n == "nin":
            out += [("nin", f"L{i}", op) for i, op in enumerate(bench.nin_ops())]
        elif n == "googlenet":
            out += [("googlenet", f"L{i}", op) for i, op in enumerate(bench.net_conv_ops("googlenet_conv", 64))]
        else:
            raise SystemExit(f"unknown net {n!r}")
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--nets", default="alexnet,nin,googlenet")
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--layers", type=int, default=0, help="at most this many layers per net (0: all)")
    a = ap.parse_args(argv)
    rtc = make_rtc("(be=hip)", 0)
    rtc.init()
    be = OpsBackend(rtc)
    per_net = {}
    for net, name, conv in nets(a.nets.split(",")):
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
