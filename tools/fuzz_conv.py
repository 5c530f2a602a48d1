#!/usr/bin/env python3
"""Random-shape parity sweep: hip_conv (default plan: whatever operand mode / tile the planner picks) vs the CPU oracle, bit-exact.
usage: fuzz_conv.py [n_cases] [seed] [big|small] [hip_tile]    (GPU box; prints the failing shapes, exit code 1 on any mismatch)
MODE=exact (default) | bf16 (hip_conv_bf16 incl. the LDS-patch kernel; mrd < 1e-3 vs the oracle on bf16-rounded operands) |
     winograd (conv_algo=winograd_all; mrd < 2e-3, the reference's Winograd bound) | k1s (1x1 stride-1 shapes through random k1_stream
     specs; bit-exact)"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np
from fuzz_fwd import conv_cases as cases, conv_mode_cases as cases_mode, k1s_specs   # the generators (tools/fuzz_fwd.py; tests/test_fwd_fuzz_cpu.py checks them)


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 100
    seed = int(sys.argv[2]) if len(sys.argv) > 2 else 1
    big = len(sys.argv) > 3 and sys.argv[3] == "big"
    tile = sys.argv[4] if len(sys.argv) > 4 else ""      # optional explicit workgroup tile (hip_tile) for every case
    from boda_amd.cnn_op import OpTune
    from test_gpu_parity import _conv_op, _run
    from boda_amd.rtc import make_rtc
    from boda_amd.ops_prof import OpsBackend
    from oracle import boda_oracle as bo
    rtc = make_rtc("(be=hip)", 0); rtc.init(); be = OpsBackend(rtc)
    bad = 0; modes = {}
    mode = os.environ.get("MODE", "exact")
    from boda_amd.digest import SsdsDiff
    worst = 0.0
    shapes = cases(n, seed, big) if mode == "exact" else cases_mode(n, seed, big, mode)
    specs = k1s_specs(shapes, seed) if mode == "k1s" else [""] * len(shapes)
    for sh, spec in zip(shapes, specs):
        op = _conv_op(*sh)
        if mode == "winograd": rtc.set_tune("conv_algo", "winograd_all")
        if mode == "k1s":
            rtc.set_tune("k1_stream", spec)
        try:
            outs, prc = _run(be, op, 5, tune=OpTune(hip_tile=tile, hip_dtype="bf16" if mode == "bf16" else ""), include_ins=True)
        except Exception as e:
            if mode == "k1s" and "unsupported configuration" in str(e): modes["(spec refused)"] = modes.get("(spec refused)", 0) + 1; continue
            raise
        g = op.conv_geom()
        cfg = prc.launch["kernel"].replace("bodahip_", "") + " " + prc.launch["cfg"]; modes[cfg] = modes.get(cfg, 0) + 1
        if mode == "bf16":
            want = bo.conv_fwd(bo.to_bf16(outs["in"]), bo.to_bf16(outs["filts"]), outs["biases"], (g["SY"], g["SX"]), (g["PY"], g["PX"]), True)
        else:
            want = bo.conv_fwd(outs["in"], outs["filts"], outs["biases"], (g["SY"], g["SX"]), (g["PY"], g["PX"]), True)
        if mode in ("exact", "k1s"):
            ok = np.array_equal(want, outs["out"])
        else:
            sd = SsdsDiff.of(want, outs["out"]); worst = max(worst, sd.mrd); K = sh[1] * sh[5] * sh[6]   # fp32 accumulation-order noise on near-zero outputs grows like K (eps x partial-sum magnitude, K times): the stated bf16 bound is 1e-3 up to K = 2400
            ok = (not sd.has_nan()) and sd.mrd < (1e-3 * max(1.0, K / 2400.0) if mode == "bf16" else 2e-3)
        if mode == "k1s" and prc.launch["kernel"] != ("bodahip_k1_quad_f32" if spec.startswith("q") else "bodahip_k1_stream_f32"): ok = False
        if not ok:
            bad += 1; print("MISMATCH", sh, cfg, spec, int((want != outs["out"]).sum()), "of", want.size, flush=True)
    print(f"MODE={mode}: {n} cases, {bad} mismatches" + (f", worst mrd {worst:.2e}" if worst else "") + "; kernels / tile configs used:", dict(sorted(modes.items(), key=lambda kv: -kv[1])))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
