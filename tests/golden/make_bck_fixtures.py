"""Writes tests/golden/ops/bck-conv-ops.txt: one BckConv op line per distinct convolution geometry the reference's gradient tests recorded
(BckConv_in_grad_loss / BckConv_filts_grad_loss signatures in its test/rtc_func_sigs.txt: firenet, GoogLeNet, NiN, AlexNet, bconv_strides at img 1-5).
Shape data only.  Run where a Boda checkout exists:

    python tests/golden/make_bck_fixtures.py /path/to/boda
"""
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))


def _dims(s, name):
    m = re.search(r"\b" + name + r"=\(([^()]*)\)", s)
    return dict((k, int(v)) for k, v in (kv.split("=") for kv in m.group(1).split(",")))


def bck_line(B, C, H, W, OC, KH, KW, SY, SX, PY, PX):
    OH, OW = (H + 2 * PY - KH) // SY + 1, (W + 2 * PX - KW) // SX + 1
    f = f"dims=(out_chan={OC},in_chan={C},y={KH},x={KW})"
    i = f"dims=(img={B},chan={C},y={H},x={W})"
    return (f"(str_vals=(type=BckConv),nda_vals=(biases=(dims=(out_chan={OC})),biases_grad_loss=(dims=(out_chan={OC})),filts=({f}),filts_grad_loss=({f}),"
            f"in=({i}),in_grad_loss=({i}),in_pad=(tn=none,dims=(y={PY},x={PX})),kern_sz=(tn=none,dims=(y={KH},x={KW})),"
            f"out_chans=(tn=uint32_t,v={OC}),out_grad_loss=(dims=(img={B},chan={OC},y={OH},x={OW})),stride=(tn=none,dims=(y={SY},x={SX}))))")


def main(boda_root):
    seen, lines = set(), []
    with open(os.path.join(boda_root, "test", "rtc_func_sigs.txt")) as f:
        for s in f:
            if not s.startswith("(fn=BckConv_in_grad_loss,") and not s.startswith("(fn=BckConv_filts_grad_loss,"):
                continue
            filts = _dims(s, "filts" if "BckConv_in_grad_loss" in s else "filts_grad_loss")
            inp = _dims(s, "in_grad_loss" if "BckConv_in_grad_loss" in s else "in")
            ogl, st, pad = _dims(s, "out_grad_loss"), _dims(s, "stride"), _dims(s, "in_pad")
            key = (inp["img"], inp["chan"], inp["y"], inp["x"], filts["out_chan"], filts["y"], filts["x"], st["y"], st["x"], pad["y"], pad["x"])
            assert (ogl["img"], ogl["chan"]) == (key[0], key[4])
            assert (ogl["y"], ogl["x"]) == ((key[2] + 2 * key[9] - key[5]) // key[7] + 1, (key[3] + 2 * key[10] - key[6]) // key[8] + 1)
            if key not in seen:
                seen.add(key); lines.append(bck_line(*key))
    out = os.path.join(HERE, "ops", "bck-conv-ops.txt")
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(f"{out}: {len(lines)} BckConv ops")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
