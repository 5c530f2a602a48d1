"""What a function with img_shards=1 must leave on a multi-device backend, built from ONE-device calls and numpy, never from the multi-device
backend itself.

  * chunk_begin / chunks: the backend's floor split of T images over n devices (device i holds [T*i/n, T*(i+1)/n); a chunk may be empty)
  * chunk_op: an annotated function op cut down to the images of one chunk -- the call a device makes on its shard, and what the planner sees there
  * sharded_grad: the expected filter / bias gradient of a flagged call: the UNFLAGGED function on every non-empty chunk on a given one-device backend, the results
    added in device order in numpy fp32, (p_0 + p_1) + p_2 + ..., starting from the first chunk's result (one chunk: no add)
  * run_func: one annotated function on host inputs; OUT vars are filled with NaN first, uint32 vars keep their bits, `then` runs while the vars are alive
  * probe_copies: what EVERY device's copy of a replicated float var holds, read through a per-image call (hip_chan_affine on zeros: out[img, c] = 0 * 1 + b[c])"""
import numpy as np

from boda_amd.cnn_op import IMG_SHARDS_FLAG, chan_affine_func_op, pipe_func_args
from boda_amd.op import Dims, Nda
from boda_amd.rtc import RtcArg, RtcFuncCall, RtcFuncInfo


def chunk_begin(T, i, n):
    return T * i // n


def chunks(T, n):
    """The (begin, end) image ranges of the n devices, empty ones included."""
    return [(chunk_begin(T, i, n), chunk_begin(T, i + 1, n)) for i in range(n)]


def unflagged(fop):
    a = fop.copy()
    a.nda_vals.pop(IMG_SHARDS_FLAG, None)
    return a


def chunk_op(fop, cnt):
    """A copy of `fop` whose img-leading tensors hold `cnt` images."""
    a = fop.copy()
    for an, nd in list(a.nda_vals.items()):
        d = nd.dims
        if d is not None and d.names and d.names[0] == "img":
            a.nda_vals[an] = Nda(dims=Dims(d.names, (cnt,) + tuple(d.sizes[1:]), d.tn), tn=nd.tn, v=nd.v)
    return a


def run_func(rtc, fop, ins, seed=None, then=None):
    """Run one annotated function with host inputs -> {OUT arg: array} (with `then`: (that, then(rtc, arg map)), called before the vars are released).  Every OUT var
    not preloaded from `ins` is filled with NaN first: an element the call does not write shows."""
    spec = pipe_func_args(fop)
    rtc.compile([RtcFuncInfo("f", "", [a for a, _ in spec], fop)])
    am, made = {}, []
    try:
        for an, io in spec:
            if io == "REF":
                am[an] = RtcArg.ref(fop.get_dims(an)); continue
            if io == "VAL":
                am[an] = RtcArg.scalar(int(seed) & 0xFFFFFFFF, "uint32_t"); continue
            d = fop.get_dims(an)
            rtc.create_var_with_dims(an, d); made.append(an); am[an] = RtcArg.var(an)
            if an in ins:
                rtc.copy_nda_to_var(an, np.ascontiguousarray(ins[an]).reshape(d.sizes))
            elif io == "OUT":
                rtc.copy_nda_to_var(an, np.full(d.sizes, np.nan, np.float32))
        rtc.run(RtcFuncCall("f", am))
        rtc.finish_and_sync()
        outs = {a: rtc.copy_var_to_nda(am[a].n) for a, io in spec if io == "OUT"}
        return (outs, then(rtc, am)) if then else outs
    finally:
        for vn in made:
            rtc.release_var(vn)
        rtc.release_func("f"); rtc.release_per_call_id_data()


def grad_arg(fop):
    return {"hip_bconv_filts": "filts_grad_loss", "hip_bconv_biases": "biases_grad_loss"}[fop.get_func_name()]


def sharded_grad(rtc, fop, ins, n):
    """The filter / bias gradient a flagged `fop` must leave on n devices: `rtc` (one device) runs the unflagged function per non-empty image chunk, the chunks are added
    in device order in numpy fp32.  ins: the whole batch's IN args."""
    plain, out_an = unflagged(fop), grad_arg(fop)
    T = fop.get_dims("out_grad_loss").dsz("img")
    total = None
    for b, e in chunks(T, n):
        if e == b:
            continue
        part = run_func(rtc, chunk_op(plain, e - b), {an: np.ascontiguousarray(x[b:e]) for an, x in ins.items()})[out_an]
        total = part if total is None else (total + part).astype(np.float32)
    return total


def probe_copies(rtc, vn, n_dev):
    """-> (n_dev, elements) float32: row i is what device i's copy of the replicated float var `vn` holds.  A batch of n_dev images gives every device one image;
    hip_chan_affine on a zero input with a = 1 writes out[img, c] = 0 * 1 + b[c] = b[c] (a -0 reads back as +0), b being a view of the device's own copy."""
    N = rtc.get_var_dims(vn).dims_prod()
    t = Dims(("img", "chan", "y", "x"), (n_dev, N, 1, 1), "float")
    ch = Dims(("chan",), (N,), "float")
    op = chan_affine_func_op(t, 0)
    spec = pipe_func_args(op)
    rtc.compile([RtcFuncInfo("probe", "", [a for a, _ in spec], op)])
    made = []
    try:
        rtc.create_var_with_dims_as_reshaped_view_of_var("probe_b", ch, vn); made.append("probe_b")
        for v, d, x in (("probe_a", ch, np.ones(N, np.float32)), ("probe_in", t, np.zeros(t.sizes, np.float32)), ("probe_out", t, np.full(t.sizes, np.nan, np.float32))):
            rtc.create_var_with_dims(v, d); made.append(v); rtc.copy_nda_to_var(v, x)
        rtc.run(RtcFuncCall("probe", {"in": RtcArg.var("probe_in"), "a": RtcArg.var("probe_a"), "b": RtcArg.var("probe_b"), "out": RtcArg.var("probe_out")}))
        rtc.finish_and_sync()
        return rtc.copy_var_to_nda("probe_out").reshape(n_dev, N)
    finally:
        for v in made:
            rtc.release_var(v)
        rtc.release_func("probe"); rtc.release_per_call_id_data()


def bits_eq(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))
