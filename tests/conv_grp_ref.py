"""Test infrastructure of the grouped convolution (hip_conv_grp, hip_bconv_in_grp, hip_bconv_filts_grp): the case list, grouped ops, the DEFINITION -- for every
group the ungrouped function on the op sliced to that group, the results side by side -- run on a given backend, and an independent float64 twin.

A case is (B, g, C, OC, H, W, k, stride, pad); k, stride and pad are each one number (both axes) or a (y, x) pair.  mrd = max|x - r| / max|r| over a tensor (r the
float64 result).  run_func is tests/deconv_ref.py's: NaN-filled outputs, inputs that keep their bits and, with guards=True, a guard var in front of and behind every var."""
import numpy as np
import torch

from boda_amd.cnn_op import OpTune, add_bck_conv_annotations, add_codegen_annotations
from boda_amd.op import parse_op

from deconv_ref import run_func   # noqa: F401  (one implementation for both families; the tests import it from here)

CASES = [
    (3, 2, 6, 10, 7, 6, 3, 1, 1),      # ragged CG = 3, OCG = 5, two groups inside one tile's reach
    (2, 3, 12, 96, 9, 11, 5, 2, 2),    # OCG = 32; stride not dividing the kernel
    (2, 2, 96, 80, 13, 13, 5, 1, 2),   # AlexNet conv2 shrunk: K = 1200
    (2, 4, 32, 64, 7, 7, 1, 1, 0),     # grouped 1x1
    (2, 4, 32, 64, 7, 7, 1, 2, 0),     # grouped 1x1 at stride 2: data-gradient positions that no term reaches are +0
    (3, 19, 19, 19, 10, 9, 3, 1, 1),   # depthwise, odd channel count, rows that are no multiple of 4
    (3, 19, 19, 19, 10, 9, 3, 2, 1),   # depthwise at stride 2
    (2, 8, 8, 16, 6, 5, 3, 1, 1),      # depthwise, channel multiplier 2
    (5, 2, 4, 4, 3, 3, 3, 1, 1),       # plane no larger than the kernel
]
CASE_IDS = ["x".join(str(v) for v in c) for c in CASES]


def two(v):
    """A kernel, stride or pad as its (y, x) pair."""
    return tuple(int(i) for i in v) if isinstance(v, (tuple, list)) else (int(v), int(v))


def out_plane(H, W, k, s, p):
    (KH, KW), (SY, SX), (PY, PX) = two(k), two(s), two(p)
    return (H + 2 * PY - KH) // SY + 1, (W + 2 * PX - KW) // SX + 1


def _geom_fields(k, s, p):
    (KH, KW), (SY, SX), (PY, PX) = two(k), two(s), two(p)
    return f"in_pad=(tn=none,dims=(y={PY},x={PX})),kern_sz=(tn=none,dims=(y={KH},x={KW})),stride=(tn=none,dims=(y={SY},x={SX}))"


def conv_op(B, g, C, OC, H, W, k, s, p, group_field=True):
    """A Convolution with filts OC x C/g x KH x KW; group_field=False leaves `group` out (g must then be 1)."""
    OH, OW = out_plane(H, W, k, s, p)
    KH, KW = two(k)
    grp = f"group=(tn=uint32_t,v={g})," if group_field else ""
    return parse_op(f"(str_vals=(type=Convolution),nda_vals=(biases=(dims=(out_chan={OC})),filts=(dims=(out_chan={OC},in_chan={C // g},y={KH},x={KW})),{grp}"
                    f"in=(dims=(img={B},chan={C},y={H},x={W})),out=(dims=(img={B},chan={OC},y={OH},x={OW})),out_chans=(tn=uint32_t,v={OC}),{_geom_fields(k, s, p)}))")


def bck_op(B, g, C, OC, H, W, k, s, p, group_field=True):
    OH, OW = out_plane(H, W, k, s, p)
    KH, KW = two(k)
    grp = f"group=(tn=uint32_t,v={g})," if group_field else ""
    f = f"dims=(out_chan={OC},in_chan={C // g},y={KH},x={KW})"
    i = f"dims=(img={B},chan={C},y={H},x={W})"
    return parse_op(f"(str_vals=(type=BckConv),nda_vals=(biases=(dims=(out_chan={OC})),biases_grad_loss=(dims=(out_chan={OC})),filts=({f}),filts_grad_loss=({f}),{grp}"
                    f"in=({i}),in_grad_loss=({i}),out_chans=(tn=uint32_t,v={OC}),out_grad_loss=(dims=(img={B},chan={OC},y={OH},x={OW})),{_geom_fields(k, s, p)}))")


def rand_ins(case, seed, lo=-5.0, hi=5.0):
    """The reference's test range U(-5, 5) for every operand of the three functions."""
    B, g, C, OC, H, W, k, s, p = case
    OH, OW = out_plane(H, W, k, s, p)
    rng = np.random.default_rng(seed)
    u = lambda *sh: rng.uniform(lo, hi, sh).astype(np.float32)
    return {"in": u(B, C, H, W), "filts": u(OC, C // g, *two(k)), "biases": u(OC), "out_grad_loss": u(B, OC, OH, OW)}


def grouped_funcs(case, tune=None):
    """-> (hip_conv_grp, hip_bconv_in_grp, hip_bconv_biases, hip_bconv_filts_grp) function ops of a case."""
    tune = tune or OpTune()
    fi, fb, ff = add_bck_conv_annotations(bck_op(*case), tune)
    return add_codegen_annotations(conv_op(*case), tune), fi, fb, ff


def slice_case(case):
    """The ungrouped case one group is."""
    B, g, C, OC, H, W, k, s, p = case
    return (B, 1, C // g, OC // g, H, W, k, s, p)


def slice_ins(case, ins, j):
    """Group j's share of every operand."""
    g, C, OC = case[1], case[2], case[3]
    cg, ocg = C // g, OC // g
    cut = {"in": lambda a: a[:, j * cg:(j + 1) * cg], "filts": lambda a: a[j * ocg:(j + 1) * ocg], "biases": lambda a: a[j * ocg:(j + 1) * ocg],
           "out_grad_loss": lambda a: a[:, j * ocg:(j + 1) * ocg]}
    return {an: cut[an](a) for an, a in ins.items() if a is not None}   # (an operand the function at hand does not read may be absent)


def sliced(rtc, case, ins, which, tile=""):
    """The definition: the UNGROUPED function `which` ("fwd" | "in" | "filts") on backend `rtc` once per group, on the op sliced to that group, concatenated along
    the channel (fwd, in) or filter-row (filts) axis."""
    sc = slice_case(case)
    fwd = add_codegen_annotations(conv_op(*sc, group_field=False), OpTune())
    fi, _, ff = add_bck_conv_annotations(bck_op(*sc, group_field=False), OpTune())
    fop = {"fwd": fwd, "in": fi, "filts": ff}[which]
    parts = [run_func(rtc, fop, slice_ins(case, ins, j), tile)[0] for j in range(case[1])]
    return np.concatenate(parts, axis=0 if which == "filts" else 1)


def torch_twin(case, ins, relu=True):
    """float64, independent of the slicing helper: torch conv2d(groups=g) and autograd.  -> (out, in_grad_loss, filts_grad_loss); the gradients are those of
    sum(conv(in, filts) * out_grad_loss) (no bias, no ReLU), which is what the BckConv functions compute."""
    B, g, C, OC, H, W, k, s, p = case
    x = torch.from_numpy(ins["in"].astype(np.float64)).requires_grad_(True)
    w = torch.from_numpy(ins["filts"].astype(np.float64)).requires_grad_(True)
    b = torch.from_numpy(ins["biases"].astype(np.float64))
    y = torch.nn.functional.conv2d(x, w, None, stride=two(s), padding=two(p), groups=g)
    out = y.detach() + b.view(1, -1, 1, 1)
    if relu:
        out = torch.clamp(out, min=0.0)
    (y * torch.from_numpy(ins["out_grad_loss"].astype(np.float64))).sum().backward()
    return out.numpy(), x.grad.numpy(), w.grad.numpy()


def mrd(x, r):
    return float(np.max(np.abs(np.asarray(x, np.float64) - r)) / max(np.max(np.abs(r)), 1e-30))


def bits_equal(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32))
