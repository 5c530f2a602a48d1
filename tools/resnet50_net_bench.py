"""Times the whole ResNet-50 forward pass (conv_pipe.resnet50, TEST phase) on be=hip in the channels-last bf16 tune, one hipGraph replay per pass, both ways of
forming a block's res = ReLU(shortcut + branch2c) in ONE process: "fused" -- ConvPipeFwd(fuse_residual=True), the shortcut added in the epilogue of the block's last
convolution (kernels/conv_nhwc_bf16.hip -DRES=1) -- and "unfused" -- fuse_residual=False, 16 nhwc_eltwise calls.  Each way runs on a backend instance of its own with
the same params and input; after the warm-up the two alternate in --repeats blocks of --runs replays.  Per way one JSON line (step ms as the median over all
blocks, the medians of the single blocks -- their spread is what a difference has to beat --, images/s, the call count) and a third with the launches removed, the
fused / unfused ratio and the residual folds.  The comparison is between the two ways of one run, never against a recorded figure; no target is set.

    python tools/resnet50_net_bench.py [--batch 64] [--runs 20] [--warmup 5] [--repeats 3] [--out profiles/r11_resnet50_net.txt]

The measurement runs in a child process under a time limit (--limit seconds).
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def he_params(cp, seed=0):
    """He-scaled filters, BatchNorm var in [0.5, 2] and Scale scale in [0.5, 1.5]: 50 layers of bf16 activations stay finite (times do not depend on the values;
    finite ones keep the run honest)."""
    import numpy as np
    rng = np.random.default_rng(seed)
    P = {}
    for pn, d in cp.params.items():
        if pn.endswith("_filts"):
            P[pn] = (rng.standard_normal(d.sizes) * np.sqrt(2.0 / (d.dsz("in_chan") * d.dsz("y") * d.dsz("x")))).astype(np.float32)
        elif pn.endswith("_var"):
            P[pn] = rng.uniform(0.5, 2.0, d.sizes).astype(np.float32)
        elif pn.endswith("_scale"):
            P[pn] = rng.uniform(0.5, 1.5, d.sizes).astype(np.float32)
        else:
            P[pn] = rng.uniform(-0.1, 0.1, d.sizes).astype(np.float32)
    return P


def child(batch, runs, warmup, repeats):
    import numpy as np
    from boda_amd import conv_pipe
    from boda_amd.cnn_op import OpTune
    from boda_amd.rtc import make_rtc
    cp = conv_pipe.resnet50(batch)
    params = he_params(cp)
    data = np.random.default_rng(1).uniform(-1, 1, cp.nodes["data"].sizes).astype(np.float32)
    ways = {}
    for way, fuse in (("unfused", False), ("fused", True)):
        rtc = make_rtc("(be=hip)", 0)
        rtc.init()
        drv = conv_pipe.ConvPipeFwd(rtc, OpTune(hip_dtype="bf16", hip_layout="nhwc"), fuse_residual=fuse)
        drv.init(cp, params)
        fwd = {"data": data}
        drv.run_fwd(["data"], fwd, ["fc1000"])      # (the first pass is an eager one: kernels and workspaces exist before the capture)
        captured = drv.capture_graph()
        ways[way] = {"rtc": rtc, "drv": drv, "blocks": [], "ms": [], "captured": captured, "out": fwd["fc1000"]}
    for w in ways.values():
        for _ in range(warmup):
            w["drv"].run_graph()
    for _ in range(repeats):
        for w in ways.values():
            ms = [w["drv"].run_graph() for _ in range(runs)]
            w["ms"] += ms; w["blocks"].append(round(statistics.median(ms), 4))
    for way, w in ways.items():
        step = statistics.median(w["ms"])
        print(json.dumps({"net": "resnet50", "tune": "bf16 nhwc", "batch": batch, "way": way, "calls": len(w["drv"].fwd_calls), "captured_calls": w["captured"],
                          "step_ms": round(step, 4), "block_medians_ms": w["blocks"], "imgs_per_s": round(batch / (step * 1e-3), 1),
                          "out_finite": bool(np.isfinite(w["out"]).all())}), flush=True)
    u, f = ways["unfused"], ways["fused"]
    d = np.abs(u["out"].astype(np.float64) - f["out"].astype(np.float64))
    print(json.dumps({"net": "resnet50", "launches_removed": len(u["drv"].fwd_calls) - len(f["drv"].fwd_calls), "folded": len(f["drv"].fused_residuals["folded"]),
                      "unfolded": f["drv"].fused_residuals["unfolded"], "fused_over_unfused": round(statistics.median(f["ms"]) / statistics.median(u["ms"]), 4),
                      "max_abs_diff_of_the_two_outputs": float(d.max()), "max_abs_output": float(np.abs(u["out"]).max())}), flush=True)
    for w in ways.values():
        w["drv"].release(); w["rtc"].close()


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3, help="alternating blocks of --runs replays per way")
    ap.add_argument("--limit", type=int, default=300, help="seconds for the measurement")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r11_resnet50_net.txt"))
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args(argv)
    if a.child:
        return child(a.batch, a.runs, a.warmup, a.repeats)
    args = ["--batch", str(a.batch), "--runs", str(a.runs), "--warmup", str(a.warmup), "--repeats", str(a.repeats)]
    r = subprocess.run(["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--child"] + args, capture_output=True, text=True)
    if r.returncode != 0:   # nothing more is started on the GPU after a failure
        print(f"exit status {r.returncode}\n{r.stderr[-2000:]}", file=sys.stderr)
        return r.returncode
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    print("\n".join(lines), flush=True)
    with open(a.out, "w") as f:
        f.write("# python tools/resnet50_net_bench.py " + " ".join(args) + "\n" + "\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
