"""What the evaluation-pass tests share (tests/test_eval_cpu.py, tests/test_gpu_eval.py): the numpy twins of hip_accuracy and hip_eval_accum (csrc/kernels/eval_f32.hip
states the rules; hip_bn_fold's twin is conv_pipe.fold_affine itself), a runner for a bare function with typed vars and guard vars, the op-level checks and the checks of
an EvalPipe's passes, all of which take the backend as an argument.

Equality is on the bits.  Integers are compared as they are.  Floats are compared on their uint32 views, except that where the twin yields NaN the backend must yield
NaN: IEEE 754 leaves a NaN's sign and payload to the platform (x86's sqrt of a negative is 0xFFC00000, the GPU's 0x7FC00000), and numpy's NaN is the host's."""
import numpy as np

import solver_ref as V
from boda_amd.bck_pipe import BN_IN_SFX, BN_ISTD_SFX, BN_MEAN_SFX, ConvPipeBck, Solver, add_bck_ops, bn_stat_params
from boda_amd.cnn_op import accuracy_func_op, bn_fold_func_op, chan_affine_func_op, eval_accum_func_op, pipe_func_args
from boda_amd.conv_pipe import ConvPipe, PipeOp, _conv, fold_affine
from boda_amd.eval_pipe import EVAL_A_SFX, EVAL_B_SFX, EVAL_COUNTS_VAR, EVAL_CTL_VAR, EVAL_LOSS_SUM_VAR, EVAL_RANK_VAR, EvalPipe
from boda_amd.op import Dims
from boda_amd.rtc import RtcArg, RtcFuncCall, RtcFuncInfo

import bn_ref
from resnet_ref import chan_affine_ref
from test_bck_pipe_cpu import N_CLASS, PIPES, small_inputs, small_params

F, U32 = np.float32, np.uint32
GUARD_BITS = 0x7FC0BEEF     # a payload NaN: what a guard var and a pre-filled float output hold
POISON = 0xDEADBEEF         # what a pre-filled uint32 output holds
INVALID = 0xFFFFFFFF
NP_OF = {"float": F, "uint32_t": U32}


def same_bits(got, want):
    """got: the backend's, want: the twin's; both float32 or both uint32."""
    got, want = np.ascontiguousarray(got).reshape(-1), np.ascontiguousarray(want).reshape(-1)
    if got.dtype != want.dtype or got.shape != want.shape:
        return False
    if got.dtype == U32:
        return bool(np.array_equal(got, want))
    return V.same_bits(got, want)


# ---- the twins
def accuracy_np(x, label):
    """hip_accuracy: x float (B, C, 1, 1) or (B, C), label float (B, ...) -> uint32 (B,)."""
    x = np.asarray(x, F).reshape(len(x), -1); lab = np.asarray(label, F).reshape(-1)
    B, C = x.shape
    out = np.empty(B, U32)
    for i in range(B):
        lf = lab[i]
        if not (lf >= 0 and lf < F(C)):     # (a NaN label fails both)
            out[i] = INVALID; continue
        L = int(lf)
        with np.errstate(invalid="ignore"):
            beaten = x[i] < x[i, L]
        out[i] = int(np.count_nonzero(~beaten)) - 1     # (c == L never beats itself: take it out of the count)
    return out


def eval_accum_np(rank, loss, ctl, counts, loss_sum, top_k):
    """hip_eval_accum -> (counts', loss_sum'): uint32 (4,), float32 (1,)."""
    rank = np.asarray(rank, U32).reshape(-1)
    add = np.array([rank.size, np.count_nonzero(rank < 1), np.count_nonzero(rank < np.uint64(top_k)), 1], U32)
    loss = np.asarray(loss, F).reshape(-1)[:1]
    if ctl[0] != 0:
        return add, loss.copy()
    with np.errstate(all="ignore"):
        return (np.asarray(counts, U32) + add).astype(U32), (np.asarray(loss_sum, F).reshape(-1)[:1] + loss).astype(F)


def result_np(counts, loss_sum):
    images, h1, hk, batches = (int(v) for v in counts)
    return {"images": images, "batches": batches, "hits_top1": h1, "hits_topk": hk, "top1": h1 / images, "topk": hk / images, "loss": float(np.float64(loss_sum[0]) / np.float64(batches))}


# ---- a bare function on typed vars, its vars rewritten between the calls
def run_steps(rtc, name, fop, vals, steps, keep=None):
    """Compile `fop`, create one var per var arg (the op's dims and type) and a 4-float guard var behind each; upload `vals` {arg: array}; then per entry of `steps`
    ({arg: array}) upload it and run the call once -> ([{arg: array fetched} after each call], {guard var: array} at the end)."""
    spec = [(an, io) for an, io in pipe_func_args(fop) if io in ("IN", "OUT", "INOUT")]
    rtc.compile([RtcFuncInfo(name, "", [a for a, _ in spec], fop)])
    made, am = [], {}
    guard = np.full(4, GUARD_BITS, U32).view(F)
    up = lambda an, a: rtc.copy_nda_to_var(f"{name}_{an}", np.ascontiguousarray(a, NP_OF[fop.get_dims(an).tn]).reshape(fop.get_dims(an).sizes))
    try:
        for an, _ in spec:
            vn = f"{name}_{an}"
            rtc.create_var_with_dims(vn, fop.get_dims(an)); made.append(vn); am[an] = RtcArg.var(vn)
            rtc.create_var_with_dims(vn + "_guard", Dims.make("float", v=4)); made.append(vn + "_guard")
            rtc.copy_nda_to_var(vn + "_guard", guard)
        for an, a in vals.items():
            up(an, a)
        call = RtcFuncCall(name, am)
        seen = []
        for st in steps:
            for an, a in st.items():
                up(an, a)
            rtc.run(call); rtc.finish_and_sync()
            if keep is not None:
                keep.append(rtc.last_launch() if rtc.be == "hip" else {})
            seen.append({an: rtc.copy_var_to_nda(f"{name}_{an}").reshape(-1) for an, _ in spec})
        gv = {vn: rtc.copy_var_to_nda(vn) for vn in made if vn.endswith("_guard")}
        return seen, gv
    finally:
        for vn in made:
            rtc.release_var(vn)
        rtc.release_func(name); rtc.release_per_call_id_data()


def guards_intact(gv, n):
    assert len(gv) == n, (len(gv), n)
    for vn, a in gv.items():
        assert np.array_equal(a.view(U32), np.full(4, GUARD_BITS, U32)), (vn, "an element outside the vars changed")


# ---- hip_accuracy
ACC_CHANS = (1, 2, 63, 64, 65, 1000)
ACC_IMGS = (1, 3, 4, 5, 9)     # four waves per workgroup: one partly filled workgroup, a full one, and a ragged last one


def accuracy_images(C, seed=0):
    """-> [(what, scores (C,), label, the rank the rule gives or None: the twin's)] -- every image the issue names, at C channels."""
    rng = np.random.default_rng([C, seed])
    nan, inf = F(np.nan), F(np.inf)
    distinct = lambda: rng.permutation(C).astype(F) - F(C // 2)     # tie-free, both signs
    out = []
    x = distinct(); out.append(("label 0", x, 0.0, int(np.count_nonzero(x > x[0]))))
    x = distinct(); out.append(("label C-1", x, float(C - 1), int(np.count_nonzero(x > x[C - 1]))))
    fl, cl = (2.5, 2) if C >= 3 else (0.5, 0)
    x = distinct(); out.append(("fractional label", x, fl, int(np.count_nonzero(x > x[cl]))))
    for what, lab in (("label -1", -1.0), ("label C", float(C)), ("label 1e9", 1e9), ("label NaN", float("nan"))):
        out.append((what, distinct(), lab, INVALID))
    out.append(("all scores equal", np.full(C, 0.25, F), float(C // 2), C - 1))
    L = C // 3
    if C >= 2:
        x = distinct(); o = (L + 1) % C; x[o] = x[L]
        out.append(("a tie with exactly one other class", x, float(L), int(np.count_nonzero(x > x[L])) + 1))
        x = -1 - rng.permutation(C).astype(F); x[L] = 0.0; x[(L + 1) % C] = -0.0
        out.append(("+0 true against -0", x, float(L), 1))
        x = -1 - rng.permutation(C).astype(F); x[L] = -0.0; x[(L + 1) % C] = 0.0
        out.append(("-0 true against +0", x, float(L), 1))
        x = distinct(); x[L] = inf; x[(L + 1) % C] = -inf
        out.append(("+Inf true", x, float(L), 0))
        x = distinct(); x[L] = -inf; x[(L + 1) % C] = inf
        out.append(("-Inf true", x, float(L), C - 1))
        x = distinct(); x[L] = x.max() + 1; x[(L + 1) % C] = nan
        out.append(("a NaN in another class", x, float(L), 1))
    x = distinct(); x[L] = nan
    out.append(("a NaN in the true class", x, float(L), C - 1))
    out.append(("all NaN", np.full(C, nan, F), float(L), C - 1))
    x = rng.permutation(4 * C)[:C].astype(F) / F(8) - F(C / 4); lab = int(rng.integers(0, C))
    order = np.argsort(-x, kind="stable")     # tie-free: the true class's place in the sorted scores is its rank
    out.append(("random, against argsort", x, float(lab), int(np.nonzero(order == lab)[0][0])))
    return out


def check_accuracy(rtc, C, keep=None):
    """Every image of accuracy_images(C), dealt over calls of ACC_IMGS images (every image lands in some call, at changing wave slots); rank pre-filled with POISON."""
    imgs = accuracy_images(C)
    at = 0
    for B in ACC_IMGS:
        pick = [imgs[(at + i) % len(imgs)] for i in range(B)]; at += B
        x = np.stack([p[1] for p in pick]).reshape(B, C, 1, 1); lab = np.array([p[2] for p in pick], F).reshape(B, 1, 1)
        want = accuracy_np(x, lab)
        for i, p in enumerate(pick):
            assert p[3] is None or int(want[i]) == p[3], (C, p[0], int(want[i]), p[3], "the twin against the rule")
        fop = accuracy_func_op(Dims.make("float", img=B, chan=C, y=1, x=1))
        (seen,), gv = run_steps(rtc, "acc", fop, {"in": x, "label": lab, "rank": np.full(B, POISON, U32)}, [{}], keep=keep)
        assert seen["rank"].dtype == U32 and np.array_equal(seen["rank"], want), (C, B, [p[0] for p in pick], seen["rank"], want)
        assert same_bits(seen["in"], x) and np.array_equal(np.isnan(seen["in"]), np.isnan(x.reshape(-1))) and seen["label"].tobytes() == lab.tobytes(), "an input was written"
        guards_intact(gv, 3)
    assert at >= len(imgs)


# ---- hip_eval_accum
ACCUM_IMGS = (1, 255, 256, 257, 1000)
ACCUM_C = 7
ACCUM_TOP_KS = (1, 5, ACCUM_C + 3)


def accum_ranks(B, seed):
    rng = np.random.default_rng([B, seed])
    r = rng.integers(0, ACCUM_C, B).astype(U32)
    if B == 1:
        r[0] = (0, INVALID, 3)[seed % 3]
    else:
        r[rng.integers(1, B, max(1, B // 8))] = INVALID     # invalid labels: a miss under every top_k
        r[0] = 0
    return r


def check_eval_accum(rtc, B, top_k, keep=None):
    """first, add, add with ctl, rank and loss rewritten in between; counts start as POISON and loss_sum as the payload NaN, so `first` provably reads neither."""
    fop = eval_accum_func_op(B, top_k)
    ranks = [accum_ranks(B, k) for k in range(3)]
    losses = [np.array([v], F) for v in (1.9172, 0.3333333, 2.0 ** -20)]
    ctls = [np.array([1, 0, 0, 0], U32), np.array([0, 0, 0, 0], U32), np.array([0, 7, 7, 7], U32)]     # (only ctl[0] is looked at)
    vals = {"counts": np.full(4, POISON, U32), "loss_sum": np.full(1, GUARD_BITS, U32).view(F)}
    seen, gv = run_steps(rtc, "eacc", fop, vals, [{"rank": ranks[k], "loss": losses[k], "ctl": ctls[k]} for k in range(3)], keep=keep)
    counts, ls = vals["counts"], vals["loss_sum"]
    seq = None
    for k in range(3):
        counts, ls = eval_accum_np(ranks[k], losses[k], ctls[k], counts, ls, top_k)
        seq = losses[k][0] if k == 0 else F(seq + losses[k][0])
        assert np.array_equal(seen[k]["counts"], counts), (B, top_k, k, seen[k]["counts"], counts)
        assert seen[k]["loss_sum"].view(U32)[0] == ls.view(U32)[0] == np.array([seq], F).view(U32)[0], (B, top_k, k, "the sequential fp32 sum")
        assert np.array_equal(seen[k]["rank"], ranks[k]) and seen[k]["loss"].tobytes() == losses[k].tobytes() and np.array_equal(seen[k]["ctl"], ctls[k]), "an input was written"
    assert counts[0] == 3 * B and counts[3] == 3
    n_inv = sum(int(np.count_nonzero(r == INVALID)) for r in ranks)
    assert n_inv > 0 and counts[2] <= 3 * B - n_inv and counts[1] <= counts[2]     # an invalid label misses even under top_k = C + 3
    if top_k > ACCUM_C:
        assert counts[2] == 3 * B - n_inv
    guards_intact(gv, 5)


# ---- hip_bn_fold
FOLD_CHANS = (1, 63, 64, 65, 257)
FOLD_EPS = 1e-5


def fold_inputs(C, seed=0):
    """mean, var, scale, bias (C,) with, from channel 1 on (C = 1: mean = 0 alone): mean = 0; var = 0; var + eps < 0; a denormal var; var = Inf; mean = Inf; mean = -0
    with a negative scale; the rest random (var positive, scale of both signs)."""
    rng = np.random.default_rng([C, seed])
    mean = rng.uniform(-2, 2, C).astype(F); var = rng.uniform(0.01, 3, C).astype(F)
    scale = (rng.uniform(0.5, 1.5, C) * rng.choice([-1.0, 1.0], C)).astype(F); bias = rng.uniform(-1, 1, C).astype(F)
    special = [("mean", 0.0), ("var", 0.0), ("var", -1.0), ("var", 1e-40), ("var", np.inf), ("mean", np.inf), ("mean", -0.0)]
    if C > len(special):
        for i, (which, v) in enumerate(special):
            (mean if which == "mean" else var)[i + 1] = v
    else:     # (C = 1)
        mean[0] = 0.0
    return mean, var, scale, bias


def check_bn_fold(rtc, C, eps=FOLD_EPS, keep=None):
    """a, b against conv_pipe.fold_affine on the bits; then hip_chan_affine with the backend's own (a, b) against resnet_ref.chan_affine_ref."""
    mean, var, scale, bias = fold_inputs(C)
    if eps == 0:
        var = var.copy(); var[0] = 0.0     # 1 / sqrt(0) = Inf: a = scale * Inf, b through Inf * 0 = NaN
    fop = bn_fold_func_op(C, eps)
    nanf = lambda: np.full(C, GUARD_BITS, U32).view(F)
    (seen,), gv = run_steps(rtc, "fold", fop, {"run_mean": mean, "run_var": var, "scale": scale, "bias": bias, "a": nanf(), "b": nanf()}, [{}], keep=keep)
    with np.errstate(all="ignore"):
        wa, wb = fold_affine([("BatchNorm", mean, var, eps), ("Scale", scale, bias)])
    assert same_bits(seen["a"], wa), (C, eps, "a", seen["a"], wa)
    assert same_bits(seen["b"], wb), (C, eps, "b", seen["b"], wb)
    assert np.array_equal(np.isnan(seen["a"]), np.isnan(wa)) and np.array_equal(np.isnan(seen["b"]), np.isnan(wb))
    for an, v in (("run_mean", mean), ("run_var", var), ("scale", scale), ("bias", bias)):
        assert seen[an].tobytes() == v.tobytes(), (an, "was written")
    guards_intact(gv, 6)
    x = np.random.default_rng([C, 3]).uniform(-2, 2, (2, C, 1, 3)).astype(F); x.reshape(-1)[::7] = 0.0
    for relu in (0, 1):
        aop = chan_affine_func_op(Dims.make("float", img=2, chan=C, y=1, x=3), relu)
        (s2,), gv2 = run_steps(rtc, "caff", aop, {"in": x, "a": seen["a"], "b": seen["b"], "out": np.full(x.shape, GUARD_BITS, U32).view(F)}, [{}])
        with np.errstate(all="ignore"):
            want = chan_affine_ref(x, seen["a"], seen["b"], relu)
        if relu:     # (x > 0 ? x : +0 sends a NaN to +0: the twin's np.where does the same)
            assert not np.any(np.isnan(want))
        assert same_bits(s2["out"], want), (C, relu)
        guards_intact(gv2, 4)
    return wa, wb


# ---- the passes of an EvalPipe
def chain_without_dropout(B=2):
    """tests/test_bck_pipe_cpu.py's `chain` without its Dropout op: what the test phase of `chain` computes."""
    p = ConvPipe("chain_nd", "data", Dims.make("float", img=B, chan=3, y=13, x=13))
    _conv(p, "conv1", "data", 8, 3, 2)
    p.add(PipeOp("norm1", "LRN", "conv1", "norm1", lrn=(3, 0.05, 0.75, 1.0)))
    p.add(PipeOp("pool1", "Pooling", "norm1", "pool1", kern_sz=(3, 3), stride=(2, 2)))
    p.add(PipeOp("fc", "Convolution", "pool1", "fc", out_chans=N_CLASS, kern_sz=(0, 0)))
    return p


def make_driver(rtc, name, solver=None, **kw):
    if name == "residual":
        cp = bn_ref.residual(); bp = add_bck_ops(cp)
        drv = ConvPipeBck(rtc, solver=solver, **kw); drv.init(bp, bn_ref.res_params(cp))
        return drv, bp
    return V.make_driver(rtc, name, solver, **kw)


def inputs_of(name, cp, seed):
    if name == "residual":
        rng = np.random.default_rng([seed, 11])
        data = rng.uniform(-1, 1, cp.nodes["data"].sizes).astype(F)
        return data, rng.integers(0, bn_ref.N_CLASS, (data.shape[0], 1, 1)).astype(F)
    return small_inputs(cp, seed)


def eval_feed(name, cp, k):
    """Batch k of an evaluation: other data than any training pass gets; one label outside the classes."""
    data, label = inputs_of(name, cp, 500 + k)
    if k == 1:
        label = label.copy(); label[0] = -1.0
    return {"data": data, "label": label}


def check_chain_is_the_pipe_without_dropout(rtc):
    """Every node of `chain` after an eval batch = the forward nodes of a driver on chain-without-Dropout, same params and inputs; the same under another seed."""
    cp_nd = chain_without_dropout(); bp_nd = add_bck_ops(cp_nd)
    params = small_params(PIPES["chain"][0](), 0)
    data, label = small_inputs(cp_nd, 3)
    nd = ConvPipeBck(rtc); nd.init(bp_nd, params)
    try:
        fwd = {"data": data, "label": label}
        nd.run_bck(["data", "label"], fwd, list(cp_nd.nodes) + ["loss"])
    finally:
        nd.release()
    for seed_in_var in (False, True):
        drv, bp = make_driver(rtc, "chain", seed_in_var=seed_in_var)
        try:
            ev = EvalPipe(drv, top_k=2)
            assert "hip_dropout" not in [f.get_func_name() for _, f, _ in ev.calls()] and "hip_dropout" in [f.get_func_name() for _, f, _ in drv.calls()]
            for seed in (11, 4242):
                drv.set_det_drop_seed(seed)
                ev.reset(); ev.run_batch({"data": data, "label": label})
                for n in list(cp_nd.nodes) + ["loss"]:
                    assert rtc.copy_var_to_nda(n).tobytes() == fwd[n].tobytes(), (seed_in_var, seed, n)
            ev.release()
        finally:
            drv.release()


def check_result_is_the_twin(rtc, name, loss=None, top_k=2, graph=False):
    """Three batches: result() = the twins applied to the backend's own logits and per-batch loss values; evaluate() twice gives the same; -> (result, [logits], [loss])."""
    drv, bp = make_driver(rtc, name, seed_in_var=graph)
    try:
        ev = EvalPipe(drv, top_k=top_k, loss=loss)
        sel = ev.loss
        logits = next(o for o in bp.fwd_ops() if o.tag == sel).bots[0]
        others = [l for l in bp.loss_nodes if l != sel]
        if graph:
            assert ev.capture_graph() == len(ev.calls())
        for l in others:     # the loss calls of other heads are left out: their nodes keep what they hold
            rtc.copy_nda_to_var(l, np.full((1, 1), 123.5, F))
        ev.reset()
        counts, ls = None, None
        zs, ws = [], []
        for k in range(3):
            fd = eval_feed(name, bp.cp, k)
            ev.run_batch(fd, graph=graph)
            assert np.array_equal(rtc.copy_var_to_nda(EVAL_CTL_VAR), np.array([1 if k == 0 else 0, 0, 0, 0], U32)), (k, "the uploaded ctl words")
            z, w = rtc.copy_var_to_nda(logits), rtc.copy_var_to_nda(sel)
            rank = accuracy_np(z, fd["label"])
            assert np.array_equal(rtc.copy_var_to_nda(EVAL_RANK_VAR), rank), (name, sel, k)
            counts, ls = eval_accum_np(rank, w, [1 if k == 0 else 0], counts, ls, top_k)
            zs.append(z); ws.append(w)
        got = ev.result()
        assert got == result_np(counts, ls), (got, result_np(counts, ls))
        assert got["images"] == 3 * bp.nodes[logits].dsz("img") and got["batches"] == 3 and 0 <= got["hits_top1"] <= got["hits_topk"] < got["images"]     # (one label is invalid)
        for l in others:
            assert rtc.copy_var_to_nda(l).item() == 123.5, (l, "another head's loss was written")
        feed = lambda i: eval_feed(name, bp.cp, i)
        again = ev.evaluate(3, feed, graph=graph)
        assert again == got and ev.evaluate(3, feed, graph=graph) == got     # reset works through `first`: nothing is cleared
        ev.release()
        fwd = {"data": feed(0)["data"], "label": feed(0)["label"]}
        drv.run_bck(["data", "label"], fwd, bp.loss_nodes)     # release() leaves the driver usable
        assert all(np.isfinite(fwd[l]).all() for l in bp.loss_nodes)
        return got, zs, ws
    finally:
        drv.release()


def bn_runs_of(drv):
    return drv._plan_bn_runs(drv.bp)


def check_residual_uses_the_running_pair(rtc, img_chunks=0):
    """After two training steps: X of every [BatchNorm, Scale (, ReLU)] run = hip_chan_affine's twin on <X>_bn_in with fold_affine of the FETCHED running pair; X differs
    from the training pass's; the running pair and the batch statistics are untouched by the evaluation."""
    drv, bp = make_driver(rtc, "residual", Solver(type="sgd", lr=0.05, momentum=0.9), img_chunks=img_chunks)
    try:
        ev = EvalPipe(drv, top_k=2)
        fns = [f.get_func_name() for _, f, _ in ev.calls()]
        runs = bn_runs_of(drv)
        assert fns.count("hip_bn_fold") == fns.count("hip_chan_affine") == len(runs) == 8 and not any(f.startswith(("hip_bn_stats", "hip_bn_fwd", "hip_bnc_")) for f in fns)
        for k in range(2):
            data, label = inputs_of("residual", bp.cp, k)
            drv.run_bck(["data", "label"], {"data": data, "label": label}, [])
        stat_vars = bn_stat_params(bp.cp) + [bn.tag + sfx for _, (bn, _, _) in runs.items() for sfx in (BN_MEAN_SFX, BN_ISTD_SFX)]
        before = {vn: rtc.copy_var_to_nda(vn).tobytes() for vn in stat_vars}
        train_x = {x: rtc.copy_var_to_nda(x) for x in runs}
        ev.run_batch({"data": data, "label": label})     # the very batch the last training step saw
        for vn in stat_vars:
            assert rtc.copy_var_to_nda(vn).tobytes() == before[vn], (vn, "written by the evaluation")
        for x, (bn, sc, relu) in runs.items():
            mean, var, scale, bias = (rtc.copy_var_to_nda(vn) for vn in (bn.tag + "_mean", bn.tag + "_var", sc.tag + "_scale", sc.tag + "_bias"))
            assert not np.array_equal(mean, np.zeros_like(mean))     # (the training steps moved it)
            a, b = fold_affine([("BatchNorm", mean, var, bn.eps), ("Scale", scale, bias)])
            assert same_bits(rtc.copy_var_to_nda(bn.tag + EVAL_A_SFX), a) and same_bits(rtc.copy_var_to_nda(bn.tag + EVAL_B_SFX), b), x
            got = rtc.copy_var_to_nda(x)
            assert same_bits(got, chan_affine_ref(rtc.copy_var_to_nda(x + BN_IN_SFX), a, b, relu is not None)), x
            assert not np.array_equal(got, train_x[x]), (x, "the test phase gave the training pass's values")
        ev.release()
    finally:
        drv.release()


TRAIN_SOLVER = dict(type="adam", lr=0.01, momentum=0.9, weight_decay=5e-4, clip_gradients=0.05)


def training_run(rtc, name, with_eval, graph=False):
    """Three updates of adam with clipping and iter_size=2 (six passes); with_eval: a two-batch evaluation between every pair of passes.  graph: both the driver's and
    the EvalPipe's graphs captured, every pass and every eval batch a replay.  -> ({var: bytes} of every var of the driver, iter, micro)."""
    drv, bp = make_driver(rtc, name, Solver(**TRAIN_SOLVER), iter_size=2, seed_in_var=True)
    try:
        ev = EvalPipe(drv, top_k=2) if with_eval else None
        if graph:
            assert drv.capture_graph() == len(drv.calls())
            if ev is not None:
                assert ev.capture_graph() == len(ev.calls())
                assert drv._graph is not None and ev._graph is not None and drv._graph != ev._graph
        for k in range(6):
            if ev is not None and k:
                it, mi = drv.iter, drv.micro
                r = ev.evaluate(2, lambda i: eval_feed(name, bp.cp, 10 * k + i), graph=graph)
                assert r["batches"] == 2 and (drv.iter, drv.micro) == (it, mi)
            data, label = inputs_of(name, bp.cp, k)
            drv.set_det_drop_seed(1000 + k)
            drv.run_bck(["data", "label"], {"data": data, "label": label}, [], graph=graph)
        assert (drv.iter, drv.micro) == (3, 0)
        return {vn: rtc.copy_var_to_nda(vn).tobytes() for vn in drv.vars}, drv.iter, drv.micro
    finally:
        if ev is not None:
            ev.release()
        drv.release()


def check_training_is_undisturbed(rtc, name, graph=False):
    plain = training_run(rtc, name, False)     # eager, no evaluation
    mixed = training_run(rtc, name, True, graph=graph)
    assert plain[1:] == mixed[1:] and set(plain[0]) == set(mixed[0])
    for vn in plain[0]:
        assert plain[0][vn] == mixed[0][vn], (name, vn, "differs from the run without evaluations")
