"""The seeded random-geometry sweeps of the training BatchNorm (the hip_bn_*, hip_bnc_* and hip_bnf_* families), the full SoftmaxWithLoss,
the solver family, the evaluation functions and the input transform without a GPU: the case
generators of tools/fuzz_step.py, the one table of seeds and lists that tests/test_gpu_step_fuzz.py runs on be=hip, the check_*_case functions both files and the tool
run, and every check on be=cpu against the numpy twins on those very cases -- so that a mismatch on the GPU can only be the kernel.

  * generators: pure functions of (n, seed); every case stays inside its ranges; every branch category of fuzz_step.bn_categories / bnc_categories / loss_categories named
    in the list's wants is reached by the list as used; the restated plans (bn_slab_plan, plan_loss_op) give the planner's own grids (rtc.explain_plan, on the host)
  * bn: the five functions and hip_fan_out against tests/bn_ref.py's twin by bits, both relu forms, every reducing function launched twice on one workspace, the in-place
    forms on two cases per path; bn_ref.f64_bounds_fractions <= 1 on the `normal` cases with N >= 8 (the bounds were derived for data of that kind: DESIGN.md 3.15)
  * bnc: the four functions against tests/bnc_ref.py's chunked twin by bits;  bnf: the three functions and their in-place forms against tests/freeze_ref.py by bits
  * loss: prob and loss_per_pel under loss_ref's bounds against float64; loss, loss_state and in_grad_loss by bits against the twins on the backend's own prob and
    loss_per_pel
  * solver: hip_solver_update under every form of solver_ref.FORMS, hip_sgd_update, hip_grad_accum, hip_solver_update_acc on drawn tensor lists, and hip_grad_sumsq +
    hip_grad_norm on drawn call lists (every fourth with about 300 partials), by solver_ref.same_bits against the twins
  * eval: hip_accuracy on logits drawn from eight values (ties the rule) with a share of invalid labels, hip_eval_accum around 256 and 512 images under top_k 1, 2, C, C + 3,
    hip_bn_fold on eval_ref.fold_inputs at C 1-600, by bits;  data: hip_data_transform on drawn crops, layouts, mean forms and plans, by bytes from NaN-filled outputs
No tolerance is new: every comparison is bits against a twin or one of the written bounds of bn_ref / loss_ref.

Counts: two lists of 12 bn cases (which bnf runs as well), 12 bnc cases, two lists of 12 loss cases, 12 update and 12 norm cases, 3 x 12 eval cases, 12 data cases."""
import os
import sys

import numpy as np
import pytest

_TOOLS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools")
if _TOOLS not in sys.path:
    sys.path.insert(0, _TOOLS)
import fuzz_step as F

import bn_ref as R
import bnc_ref as RC
import freeze_ref as RF
import accum_ref as A
import data_ref as D
import eval_ref as E
import loss_ref as L
import sgd_ref as S
import solver_ref as V
from boda_amd import rtc as rtc_mod
from boda_amd.bck_graph import LossSpec
from boda_amd.cnn_op import (accuracy_func_op, bn_fold_func_op, data_transform_func_op, eval_accum_func_op, bn_bck_in_func_op, bn_bck_sums_func_op, bn_fwd_func_op, bn_stats_func_op, bnf_bck_func_op, fan_out_func_op, loss_norm_func_op,
                             softmax_loss_bck_func_op, softmax_loss_fwd_func_op)
from boda_amd.conv_pipe import fold_affine
from boda_amd.op import Dims
from boda_amd.rtc import make_rtc

# ---- the one table of seeds and lists (tests/test_gpu_step_fuzz.py imports it).  A seed is replaced only where its list misses a category of its wants
N = 12
BN_LISTS = {"bn_q": ("quad", 2101), "bn_e": ("elem", 2102)}
BNC_SEED = 2201
LOSS_LISTS = {"loss_pel": ("pel", 2301), "loss_wave": ("wave", 2302)}
SOLVER_SEED, NORM_SEED = 2401, 2402
ACC_SEED, ACCUM_SEED, FOLD_SEED, DATA_SEED = 2501, 2502, 2503, 2601
INPLACE = {"bn_q": (0, 5), "bn_e": (0, 4)}   # the two cases of each bn list that also run the in-place forms (bn_e: an HW = 1 plane and a slab edge inside a plane)

WORST = {}   # bound name -> largest observed fraction of it
USED = {}    # "kernel what" -> launches


def bn_list(key):
    return F.bn_cases(N, BN_LISTS[key][1], BN_LISTS[key][0])


def bnc_list():
    return F.bnc_cases(N, BNC_SEED)


def loss_list(key):
    return F.loss_cases(N, LOSS_LISTS[key][1], LOSS_LISTS[key][0])


def solver_list():
    return F.solver_cases(N, SOLVER_SEED)


def norm_list():
    return F.norm_cases(N, NORM_SEED)


def acc_list():
    return F.acc_cases(N, ACC_SEED)


def accum_list():
    return F.accum_cases(N, ACCUM_SEED)


def fold_list():
    return F.fold_cases(N, FOLD_SEED)


def data_list():
    return F.data_cases(N, DATA_SEED)


def data_seed(key, i):
    return 100 * (1 + (list(BN_LISTS) + ["bnc"] + list(LOSS_LISTS) + ["solver", "norm"]).index(key)) + i


def note(key):
    USED[key] = USED.get(key, 0) + 1


def under(name, frac):
    WORST[name] = max(WORST.get(name, 0.0), frac)
    assert frac <= 1.0, (name, frac)


BN_KEYS = ("mean", "inv_std", "run_mean2", "run_var2", "out", "sg", "bg", "dx")


def bn_sum_launch(ln, case, kernels):
    """The launch record of a reducing bn function: bodahip_bn_sum on C * nslabs workgroups of the restated plan -- the slabs counted on the host are what ran."""
    (B, C, H, W), forced, _ = case
    ns = F.bn_slab_plan(C, B * H * W, forced)[1]
    assert ln["kernel"] == "bodahip_bn_sum" and ln["kernels"] == kernels and ln["grid"] == C * ns and ln["block"] == 256, (case, ln)
    note(f"bn_sum {'quad' if (H * W) % 4 == 0 else 'elem'} {'slabs>1' if ns > 1 else 'one slab'}")


def check_bn_case(rtc, other, case, seed, inplace=False):
    """The five functions and hip_fan_out on `rtc` against the twin (and `other`, a second backend) by bits."""
    shape, forced, kind = case
    B, C, H, W = shape
    d = R.dims_of(shape)
    ins = F.bn_inputs(case, seed)
    relu = seed % 2
    g = R.run_all_five(rtc, shape, forced, relu=relu, repeat=2, inputs=ins)   # (every reducing function launched twice on the same workspace)
    R.check_against_numpy(g, shape, forced, relu=relu)
    common = {"in": g["x"], "mean": g["mean"], "inv_std": g["inv_std"]}
    keep = []
    out2 = R.run_func(rtc, bn_fwd_func_op(d, 1 - relu), dict(common, scale=g["scale"], bias=g["bias"]), keep=keep)[0]["out"]
    assert R.same_bits(out2, R.fwd_np(g["x"], g["mean"], g["inv_std"], g["scale"], g["bias"], 1 - relu)), ("out under the other relu", case)
    if rtc.be == "hip":
        bn_sum_launch(g["launch_stats"], case, 3)
        assert keep[0]["kernel"] == "bodahip_bn_fwd", keep
        note("bn_fwd")
    if other is not None:
        c = R.run_all_five(other, shape, forced, relu=relu, inputs=ins)
        for k in BN_KEYS:
            assert R.same_bits(g[k], c[k]), (k, "against the other backend", case)
    n = 2 + seed % 7
    keep = []
    outs = R.run_func(rtc, fan_out_func_op(d, n), {"in": g["x"]}, keep=keep)[0]
    assert len(outs) == n and all(R.same_bits(a, g["x"]) for a in outs.values()), ("fan_out", n, case)
    if rtc.be == "hip":
        assert keep[0]["kernel"] == "bodahip_fan_out", keep
        note("fan_out")
    if kind == "normal" and B * H * W >= 8:
        for k, v in R.f64_bounds_fractions(g, shape, relu=relu).items():
            under("bn " + k, v)
    if inplace:
        out = R.run_func(rtc, bn_fwd_func_op(d, relu), dict(common, scale=g["scale"], bias=g["bias"]), bind={"out": "in"})[0]["out"]
        assert R.same_bits(out, g["out"]), ("out on in", case)
        dx = R.run_func(rtc, bn_bck_in_func_op(d), dict(common, scale=g["scale"], scale_grad_loss=g["sg"], bias_grad_loss=g["bg"], out_grad_loss=g["dy"]),
                        bind={"in_grad_loss": "out_grad_loss"})[0]["in_grad_loss"]
        assert R.same_bits(dx, g["dx"]), ("in_grad_loss on out_grad_loss", case)


def check_bnf_case(rtc, other, case, seed):
    """hip_bnf_prep, hip_bnf_bck (twice on one workspace, and in place: the DX=1 store of bodahip_bn_sum) and hip_bnf_bck_in (and in place) against the twin by bits."""
    shape, forced, kind = case
    ins = F.bn_inputs(case, seed)
    r = RF.run_all_three(rtc, shape, forced, repeat=2, inputs=ins)
    RF.check_against_numpy(r, shape, forced)
    if rtc.be == "hip":
        bn_sum_launch(r["launch"], case, 2)
    if other is not None:
        c = RF.run_all_three(other, shape, forced, repeat=1, inputs=ins)
        for k in RF.RESULT_KEYS:
            assert R.same_bits(r[k], c[k]), (k, "against the other backend", case)


def check_bnc_case(rtc, other, case, seed):
    shape, chunks, forced, kind = case
    ins = F.bn_inputs((shape, forced, kind), seed)
    relu = seed % 2
    r = RC.run_all_four(rtc, shape, chunks, forced, relu=relu, repeat=2, inputs=ins)
    RC.check_against_numpy(r, shape, chunks, forced, relu=relu)
    if rtc.be == "hip":
        assert rtc.last_launch()["kernel"] == "bodahip_bn_bck_in", rtc.last_launch()
        note("bnc chain")
    if other is not None:
        c = RC.run_all_four(other, shape, chunks, forced, relu=relu, inputs=ins)
        for k in BN_KEYS:
            assert R.same_bits(r[k], c[k]), (k, "against the other backend", case)


def frac(got, want, bound):
    err = np.abs(np.asarray(got, np.float64) - want)
    return float(np.max(np.where(err == 0, 0.0, err / np.maximum(bound, 1e-300))))


def check_loss_case(rtc, other, case, seed=0):
    """The three functions chained on `rtc`: prob and loss_per_pel under loss_ref's bounds against float64, everything behind them by bits against the twins on the
    backend's OWN prob and loss_per_pel (and against `other` on those same inputs)."""
    shape, lseed, lset, nz, w, kind = case
    B, C, H, W = shape
    d = L.dims_of(shape)
    hip = rtc.be == "hip"
    name, lab, ig, meant = L.label_sets(shape, lseed)[lset]
    assert name == F.LOSS_SETS[lset]
    spec = LossSpec(w, ig, nz)
    x = L.logits(shape, kind, lseed)
    ffop = softmax_loss_fwd_func_op(d, spec)
    got = L.run_func(rtc, ffop, {"in": x, "label": lab}, kernel=L.KERNELS["hip_softmax_loss_fwd"] if hip else None)
    if hip:
        ln = rtc.last_launch()
        assert ln["grid"] == F.loss_plan(shape)["fwd"][0] and ln["block"] == 256, (case, ln)
        note(f"softmax_loss_fwd {F.loss_form(shape)} CREG={F.loss_plan(shape)['fwd'][1]}")
    prob, lpp = got["prob"], got["loss_per_pel"]
    assert np.all(np.isfinite(prob)) and np.all(np.isfinite(lpp)), case
    want = L.softmax_f64(x)
    under(f"loss prob/{F.loss_form(shape)}", frac(prob, want, L.prob_bound(want, C)))
    own = L.lpp_f64(prob, lab, spec)
    under("loss loss_per_pel", frac(lpp, own, L.lpp_bound(own)))
    ignored, valid, _ = L.classes(lab, C, spec)
    assert int(ignored.sum()) == meant, (case, meant)
    assert np.all(L.bits(lpp)[ignored] == 0) and np.all(L.bits(lpp)[~ignored & ~valid] == L.bits(L.INVALID_LOSS)), case
    ins = {"label": lab, "loss_per_pel": lpp}
    nfop = loss_norm_func_op(d, spec)
    gn = L.run_func(rtc, nfop, ins, kernel=L.KERNELS["hip_loss_norm"] if hip else None)
    loss, state = L.norm_f32(lab, lpp, spec)
    assert L.bits_eq(gn["loss"], loss) and L.bits_eq(gn["loss_state"], state), ("loss / loss_state against the twin", case, gn, loss, state)
    again = L.run_func(rtc, nfop, ins, runs=2)   # the reducing call twice on the same workspace
    assert L.bits_eq(again["loss"], gn["loss"]) and L.bits_eq(again["loss_state"], gn["loss_state"]), ("hip_loss_norm: a second run", case)
    ins_b = {"prob": prob, "label": lab, "loss_state": state}
    bfop = softmax_loss_bck_func_op(d, spec)
    gb = L.run_func(rtc, bfop, ins_b, kernel=L.KERNELS["hip_softmax_loss_bck"] if hip else None)["in_grad_loss"]
    if hip:
        assert rtc.last_launch()["grid"] == F.loss_plan(shape)["bck"][0], (case, rtc.last_launch())
        note("loss_norm"); note("softmax_loss_bck")
    assert L.bits_eq(gb, L.bck_f32(prob, lab, state, spec)), ("in_grad_loss against the twin", case)
    assert np.all(L.bits(gb)[np.broadcast_to(ignored[:, None], gb.shape)] == 0), case
    if meant == lab.size:
        assert L.bits(gn["loss"]).item() == 0 and not np.any(L.bits(gb)) and not np.any(np.isnan(gn["loss_state"])), case
    if other is not None:
        o = L.run_func(other, nfop, ins)
        assert L.bits_eq(gn["loss"], o["loss"]) and L.bits_eq(gn["loss_state"], o["loss_state"]), ("hip_loss_norm against the other backend", case)
        assert L.bits_eq(gb, L.run_func(other, bfop, ins_b)["in_grad_loss"]), ("hip_softmax_loss_bck against the other backend", case)


def check_solver_case(rtc, other, case, seed):
    """hip_solver_update under every form of solver_ref.FORMS and hip_sgd_update against their twins (and `other`) by solver_ref.same_bits, g read back unchanged, a guard
    var behind every tensor; hip_grad_accum's three calls (first / add / add and apply) through accum_ref's check on the case's sizes; hip_solver_update_acc with the case's
    mults, hyper words and coef under one form and a drawn scale, apply 0 and 1, against its twin and `other`."""
    sizes, lm, dm, (lr, mom, wd, mom2, delta, t), coef = case
    sizes, lm, dm = list(sizes), list(lm), list(dm)
    hypers = [V.hyper8(lr, mom, wd, mom2, delta, V.corr_f64(mom, mom2, t))]
    state = np.array([coef, 9.0, 81.0, 0.0], np.float32)
    ins = V.make_inputs(sizes, seed)
    guard = np.full(4, V.GUARD_BITS, np.uint32)
    hip = rtc.be == "hip"
    for form in V.FORMS:
        keep = []
        got, guards = V.run_update(rtc, sizes, form, lm, dm, hypers, ins, state, guards=True, keep=keep)
        if hip:
            assert keep[0]["kernel"] == "bodahip_solver_update_" + form[0] and keep[0]["grid"] == F.solver_grid(sizes), (sizes, keep)
            note("solver_update_" + form[0])
        want = V.want_update(form, lm, dm, hypers, ins, state)
        on_other = V.run_update(other, sizes, form, lm, dm, hypers, ins, state)[0] if other is not None else None
        for i in range(len(sizes)):
            what = (V.form_id(form), i, sizes[i])
            assert V.same_bits(got[i][1], ins[i][1]) and np.array_equal(np.isnan(got[i][1]), np.isnan(ins[i][1])), (what, "g was written")
            for k, nm in ((2, "history"), (3, "second history"), (0, "param")):
                assert V.same_bits(got[i][k], want[i][k]), (what, nm, "against the twin")
                assert on_other is None or (V.same_bits(got[i][k], on_other[i][k]) and V.same_bits(on_other[i][k], got[i][k])), (what, nm, "against the other backend")
        assert len(guards) == (4 if form[0] == "adam" else 3) * len(sizes) + 2
        assert all(np.array_equal(a.view(np.uint32), guard) for a in guards.values()), (sizes, V.form_id(form), "an element outside the tensors changed")
    keep = []
    old, guards = S.run_sgd(rtc, sizes, lm, dm, [(lr, mom, wd)], [x[:3] for x in ins], guards=True, keep=keep)
    want = S.want_sgd(sizes, lm, dm, [(lr, mom, wd)], [x[:3] for x in ins])
    for i in range(len(sizes)):
        assert V.same_bits(old[i][1], ins[i][1]) and all(V.same_bits(old[i][k], want[i][k]) for k in (0, 2)), ("hip_sgd_update", i, sizes[i])
    assert all(np.array_equal(a.view(np.uint32), guard) for a in guards.values()), (sizes, "hip_sgd_update: an element outside the tensors changed")
    if hip:
        assert keep[0]["kernel"] == "bodahip_sgd_update" and keep[0]["grid"] == F.solver_grid(sizes), keep
        note("sgd_update")
    if other is not None:
        o_sgd, _ = S.run_sgd(other, sizes, lm, dm, [(lr, mom, wd)], [x[:3] for x in ins])
        assert all(V.same_bits(old[i][k], o_sgd[i][k]) for i in range(len(sizes)) for k in (0, 2)), ("hip_sgd_update against the other backend", sizes)
    # hip_grad_accum: first / add / add with a drawn scale word (it does not read it) on accum_ref's three gradients; hip_solver_update_acc: the case's own mults, hyper
    # words, coef and a drawn scale -- apply 0 keeps every bit, apply 1 leaves the twin's
    keeps = A.check_accum_three_calls(rtc, sizes)
    form = V.FORMS[seed % len(V.FORMS)]
    scale = float([0.25, A.THIRD, 0.5, 1.0, 3.0][seed % 5])
    fop = A.update_acc_fop(sizes, form, lm, dm)
    vals = {"state": state, "hyper": hypers[0]}
    for i, (w, g, h, h2) in enumerate(ins):
        vals.update({f"w_{i}": w, f"g_{i}": g, f"h_{i}": h})
        if form[0] == "adam":
            vals[f"h2_{i}"] = h2
    for acc in (A.words(0, 0, scale, 1), A.words(0, 1, scale, 2), A.words(1, 1, 1, 0)):
        (seen,), gv = A.run_steps(rtc, "slva", fop, vals, [{"accum": acc}], keep=keeps)
        oseen = A.run_steps(other, "slva", fop, vals, [{"accum": acc}])[0][0] if other is not None else None
        for i, (w, g, h, h2) in enumerate(ins):
            what = ("hip_solver_update_acc", V.form_id(form), list(acc), i, sizes[i])
            w2, hn, vn = A.update_acc_np(form[0], w, g, h, h2, hypers[0], acc, lm[i], dm[i], form[1], state[0], form[2])
            assert V.same_bits(seen[f"g_{i}"], g) and np.array_equal(np.isnan(seen[f"g_{i}"]), np.isnan(g.reshape(-1))), (what, "g was written")
            if acc[1] == 0:
                assert A.bits_equal(seen[f"w_{i}"], w.reshape(-1)) and A.bits_equal(seen[f"h_{i}"], h.reshape(-1)), (what, "apply = 0 wrote")
                assert form[0] != "adam" or A.bits_equal(seen[f"h2_{i}"], h2.reshape(-1)), (what, "apply = 0 wrote")
                continue
            for an, tw in ((f"w_{i}", w2), (f"h_{i}", hn)) + (((f"h2_{i}", vn),) if form[0] == "adam" else ()):
                assert V.same_bits(seen[an], tw), (what, an, "against the twin")
                assert oseen is None or (V.same_bits(seen[an], oseen[an]) and V.same_bits(oseen[an], seen[an])), (what, an, "against the other backend")
        for an, a in (("hyper", hypers[0]), ("state", state), ("accum", acc)):
            assert A.bits_equal(seen[an], np.asarray(a, np.float32)), (an, "was written")
        A.guards_intact(gv, (4 if form[0] == "adam" else 3) * len(sizes) + 3)
    if hip:
        assert all(k["kernel"] in ("bodahip_grad_accum", "bodahip_solver_update_" + form[0]) and k["grid"] == F.solver_grid(sizes) for k in keeps), keeps
        note("grad_accum"); note("solver_update_acc")


def check_norm_case(rtc, other, case, seed):
    """The hip_grad_sumsq calls of a case into one partials var, then hip_grad_norm, against the twin's chain (and `other`) by bits; the clip below, above or equal to the
    norm the twin gives; the whole sequence twice."""
    calls_sz, total, clipk = case
    rng = np.random.default_rng([seed, 93])
    calls = [(p0, [rng.uniform(-1, 1, n).astype(np.float32) for n in sz]) for p0, sz in calls_sz]
    prefill = np.full(total, 0.5, np.float32)
    norm = float(V.want_norm(calls, prefill, 0.0)[1][1])
    assert np.isfinite(norm) and norm > 0
    clip = {"below": float(np.float32(norm * 0.5)), "above": float(np.float32(norm * 2)), "equal": norm, "off": 0.0}[clipk]
    keep = []
    seen, state = V.run_norm(rtc, calls, total, prefill, clip, keep)
    wseen, wstate = V.want_norm(calls, prefill, clip)
    assert all(V.same_bits(a, b) for a, b in zip(seen, wseen)), ("partials against the twin", total, clipk)
    assert V.same_bits(state, wstate), ("state against the twin", total, clipk, state, wstate)
    assert (state[0] == 0.5) if clipk == "below" else (state[0] == 1.0) if clipk in ("above", "equal") else True, (clipk, state)
    if rtc.be == "hip":
        assert [k["kernel"] for k in keep] == ["bodahip_grad_sumsq"] * len(calls) and [k["grid"] for k in keep] == [F.solver_grid(sz) for _, sz in calls_sz], keep
        assert rtc.last_launch()["kernel"] == "bodahip_grad_norm", rtc.last_launch()
        note("grad_sumsq"); note("grad_norm" + (" >256 partials" if total > 256 else ""))
    seen2, state2 = V.run_norm(rtc, calls, total, prefill, clip)
    assert V.same_bits(seen2[-1], seen[-1]) and V.same_bits(state2, state), ("a second run", total, clipk)
    if other is not None:
        oseen, ostate = V.run_norm(other, calls, total, prefill, clip)
        assert V.same_bits(seen[-1], oseen[-1]) and V.same_bits(state, ostate), ("against the other backend", total, clipk)


# ---- the evaluation functions and the input transform
def check_acc_case(rtc, other, case, seed=0):
    B, C, share, _ = case
    x, lab = F.acc_data(case)
    want = E.accuracy_np(x, lab)
    fop = accuracy_func_op(Dims.make("float", img=B, chan=C, y=1, x=1))
    keep = []
    vals = {"in": x, "label": lab, "rank": np.full(B, E.POISON, np.uint32)}
    (seen,), gv = E.run_steps(rtc, "acc", fop, vals, [{}], keep=keep)
    assert seen["rank"].dtype == np.uint32 and np.array_equal(seen["rank"], want), ("rank against the twin", case, seen["rank"], want)
    assert seen["in"].tobytes() == x.tobytes() and seen["label"].tobytes() == lab.tobytes(), ("an input was written", case)
    E.guards_intact(gv, 3)
    if rtc.be == "hip":
        assert keep[0]["kernel"] == "bodahip_accuracy" and keep[0]["grid"] == F.eval_grids("accuracy", B=B) and keep[0]["block"] == 256, keep
        note("accuracy")
    if other is not None:
        assert np.array_equal(E.run_steps(other, "acc", fop, vals, [{}])[0][0]["rank"], seen["rank"]), ("against the other backend", case)


def check_accum_case(rtc, other, case, seed=0):
    """first, add, add with rank, loss and ctl rewritten in between (eval_ref.check_eval_accum's scheme on drawn ranks); counts start as POISON, loss_sum as a payload NaN."""
    B, C, top_k, dseed = case
    rng = np.random.default_rng([dseed, 67])
    ranks = []
    for k in range(3):
        r = rng.integers(0, C, B).astype(np.uint32)
        r[rng.random(B) < 0.15] = E.INVALID
        ranks.append(r)
    losses = [np.array([v], np.float32) for v in rng.uniform(0, 3, 3)]
    ctls = [np.array([1, 0, 0, 0], np.uint32), np.array([0, 0, 0, 0], np.uint32), np.array([0, 7, 7, 7], np.uint32)]
    fop = eval_accum_func_op(B, top_k)
    vals = {"counts": np.full(4, E.POISON, np.uint32), "loss_sum": np.full(1, E.GUARD_BITS, np.uint32).view(np.float32)}
    steps = [{"rank": ranks[k], "loss": losses[k], "ctl": ctls[k]} for k in range(3)]
    keep = []
    seen, gv = E.run_steps(rtc, "eacc", fop, vals, steps, keep=keep)
    oseen = E.run_steps(other, "eacc", fop, vals, steps)[0] if other is not None else None
    counts, ls = vals["counts"], vals["loss_sum"]
    for k in range(3):
        counts, ls = E.eval_accum_np(ranks[k], losses[k], ctls[k], counts, ls, top_k)
        assert np.array_equal(seen[k]["counts"], counts) and seen[k]["loss_sum"].tobytes() == ls.tobytes(), ("counts / loss_sum against the twin", case, k, seen[k]["counts"], counts)
        assert np.array_equal(seen[k]["rank"], ranks[k]) and seen[k]["loss"].tobytes() == losses[k].tobytes() and np.array_equal(seen[k]["ctl"], ctls[k]), ("an input was written", case)
        assert oseen is None or (np.array_equal(oseen[k]["counts"], counts) and oseen[k]["loss_sum"].tobytes() == ls.tobytes()), ("against the other backend", case, k)
    assert counts[0] == 3 * B and counts[3] == 3 and counts[1] <= counts[2] <= 3 * B - sum(int(np.count_nonzero(r == E.INVALID)) for r in ranks)
    E.guards_intact(gv, 5)
    if rtc.be == "hip":
        assert all(k["kernel"] == "bodahip_eval_accum" and k["grid"] == 1 and k["block"] == 256 for k in keep), keep
        note("eval_accum")


def check_fold_case(rtc, other, case, seed=0):
    C, fseed = case
    mean, var, scale, bias = E.fold_inputs(C, fseed)
    fop = bn_fold_func_op(C, E.FOLD_EPS)
    nanf = lambda: np.full(C, E.GUARD_BITS, np.uint32).view(np.float32)
    vals = {"run_mean": mean, "run_var": var, "scale": scale, "bias": bias, "a": nanf(), "b": nanf()}
    keep = []
    (seen,), gv = E.run_steps(rtc, "fold", fop, vals, [{}], keep=keep)
    with np.errstate(all="ignore"):
        wa, wb = fold_affine([("BatchNorm", mean, var, E.FOLD_EPS), ("Scale", scale, bias)])
    assert E.same_bits(seen["a"], wa) and E.same_bits(seen["b"], wb), ("a, b against fold_affine", case)
    assert np.array_equal(np.isnan(seen["a"]), np.isnan(wa)) and np.array_equal(np.isnan(seen["b"]), np.isnan(wb)), case
    for an, v in (("run_mean", mean), ("run_var", var), ("scale", scale), ("bias", bias)):
        assert seen[an].tobytes() == v.tobytes(), (an, "was written", case)
    E.guards_intact(gv, 6)
    if rtc.be == "hip":
        assert keep[0]["kernel"] == "bodahip_bn_fold" and keep[0]["grid"] == F.eval_grids("fold", C=C), keep
        note("bn_fold")
    if other is not None:
        o = E.run_steps(other, "fold", fop, vals, [{}])[0][0]
        nn = ~np.isnan(wa) & ~np.isnan(wb)
        assert seen["a"][nn].tobytes() == o["a"][nn].tobytes() and seen["b"][nn].tobytes() == o["b"][nn].tobytes(), ("against the other backend", case)


def check_data_case(rtc, other, c, seed=0):
    """hip_data_transform on data_ref.case_data's source and mean under fuzz_step.data_plans' plans, `out` pre-filled with the payload NaN before every call: bytes against
    the twin (a NaN for a NaN) and `other`."""
    sd, md, src, mean, _ = D.case_data(c)
    plans = F.data_plans(c)
    crop = (c["ch"], c["cw"])
    fop = data_transform_func_op(sd, crop, md, c["scale"])
    od = fop.get_dims("out")
    steps = [{"plan": p, "out": D.nan_out(od.sizes)} for p in plans]
    keep = []
    seen, gv = D.run_steps(rtc, "dxf", fop, {"src": src, "mean": mean}, steps, keep=keep)
    oseen = D.run_steps(other, "dxf", fop, {"src": src, "mean": mean}, steps)[0] if other is not None else None
    for k, (p, s) in enumerate(zip(plans, seen)):
        want = D.data_transform_np(src, p, mean, c["scale"], crop, c["layout"])
        assert s["out"].dtype == np.float32 and s["out"].shape == want.shape
        assert D.same_bits(s["out"], want) and np.array_equal(np.isnan(s["out"]), np.isnan(want)), ("out against the twin", D.case_id(c), p.tolist())
        assert s["src"].tobytes() == src.tobytes() and s["plan"].tobytes() == p.tobytes() and s["mean"].tobytes() == mean.tobytes(), ("an input was written", D.case_id(c))
        if oseen is not None:
            nn = ~np.isnan(want)
            assert s["out"][nn].tobytes() == oseen[k]["out"][nn].tobytes() and np.array_equal(np.isnan(oseen[k]["out"]), np.isnan(want)), ("against the other backend", D.case_id(c))
    E.guards_intact(gv, 4)
    if rtc.be == "hip":
        assert all(k["kernel"] == "bodahip_data_transform" and k["grid"] == F.data_grid(c) and k["block"] == 256 for k in keep), keep
        note("data_transform")


@pytest.fixture(scope="module")
def cpu():
    r = make_rtc("(be=cpu)")
    r.init()
    yield r
    r.close()


# ---- the generators
def test_generators_are_pure_functions_of_n_and_seed():
    gens = [lambda n, s, p=p: F.bn_cases(n, s, p) for p in F.BN_WANTS] + [F.bnc_cases] + [lambda n, s, f=f: F.loss_cases(n, s, f) for f in F.LOSS_WANTS]
    for gen in gens:
        assert gen(24, 5) == gen(24, 5) and gen(24, 5) != gen(24, 6) and len(gen(24, 5)) == 24
        assert gen(24, 5)[:8] == gen(8, 5)   # a longer list extends a shorter one
    for gen in (F.acc_cases, F.accum_cases, F.fold_cases, F.data_cases):
        assert gen(12, 5) == gen(12, 5) != gen(12, 6) and gen(12, 5)[:8] == gen(8, 5)
    assert F.solver_cases(12, 5) == F.solver_cases(12, 5) != F.solver_cases(12, 6) and F.norm_cases(12, 5) == F.norm_cases(12, 5) != F.norm_cases(12, 6)


def test_cases_stay_inside_their_ranges():
    for path in F.BN_WANTS:
        cases = F.bn_cases(120, 3, path)
        for (B, C, H, W), forced, kind in cases:
            assert B >= 1 and 1 <= H <= 64 and 1 <= W <= 40 and B * C * H * W <= F.ELEM_CAP and forced % 4 == 0 and kind in F.BN_KINDS
            assert (C in F.BN_CHANS or C in (255, 256, 257)) and F.bn_slab_plan(C, B * H * W, forced)[1] <= F.BN_MAX_SLABS and (path != "quad" or (H * W) % 4 == 0)
        for cat in F.BN_WANTS[path]:
            assert sum(1 for c in cases if cat in F.bn_categories(c)) >= 0.05 * len(cases), (path, cat)
        assert all(sum(1 for c in cases if c[2] == k) >= 0.1 * len(cases) for k in F.BN_KINDS)
    for (B, C, H, W), ch, forced, kind in F.bnc_cases(120, 3):
        assert ch in (2, 3, 5, B, B + 1) and B * C * H * W <= F.ELEM_CAP
    for form in F.LOSS_WANTS:
        cases = F.loss_cases(120, 3, form)
        for (B, C, H, W), lseed, lset, nz, w, kind in cases:
            assert B * C * H * W <= F.ELEM_CAP and F.loss_form((B, C, H, W)) == form and 0 <= lset < len(F.LOSS_SETS) and nz in L.NORMS and 0.0 <= w < 4.0 and kind in L.DATA
        for cat in F.LOSS_WANTS[form]:
            assert sum(1 for c in cases if cat in F.loss_categories(c)) >= 0.05 * len(cases), (form, cat)
    assert (F.LOSS_NORMS, F.LOSS_WEIGHTS, F.LOSS_DATA, F.LOSS_CREG) == (L.NORMS, L.WEIGHTS, L.DATA, 32)


def test_lists_reach_every_category():
    """Every category the issue names, on the lists as used."""
    for key, (path, _) in BN_LISTS.items():
        cases = bn_list(key)
        assert len(cases) == N
        count = {cat: sum(1 for c in cases if cat in F.bn_categories(c)) for cat in F.BN_WANTS[path] + ["slabs2", "empty_chains", "ragged_last"] + list(F.BN_KINDS)}
        print(key, count)
        assert all(v >= 1 for v in count.values()), (key, count)
        assert all(path == "elem" or "quad" in F.bn_categories(c) for c in cases)
        for i in INPLACE[key]:
            assert (path == "quad") == ("quad" in F.bn_categories(cases[i])), (key, i)   # the in-place forms run on both load paths
    cats = [F.bn_categories(c) for c in bn_list("bn_q")]
    assert any({"quad", "q_gt4096", "slabs2"} <= c for c in cats)   # the outer round on a launch of more than one slab
    cats = [F.bn_categories(c) for c in bn_list("bn_e")]
    assert any({"elem", "e_gt1024"} <= c for c in cats) and any({"elem", "slabs2"} <= c for c in cats)
    cl = bnc_list()
    count = {cat: sum(1 for c in cl if cat in F.bnc_categories(c)) for cat in F.BNC_WANTS + ["chunk_quad", "chunk_elem"]}
    print("bnc", count)
    assert len(cl) == N and all(v >= 2 for v in count.values()), count
    for key, (form, _) in LOSS_LISTS.items():
        cases = loss_list(key)
        count = {cat: sum(1 for c in cases if cat in F.loss_categories(c)) for cat in F.LOSS_WANTS[form]}
        print(key, count)
        assert len(cases) == N and all(v >= 1 for v in count.values()), (key, count)
    both = [F.loss_categories(c) for k in LOSS_LISTS for c in loss_list(k)]
    for cat in ("hw63", "hw64", "hw65", "pel_c1", "pel_c31", "pel_c32", "pel_c33", "pel_c_gt64", "wave_c_lt64", "wave_c64", "wave_c_65_127", "wave_c_ge192_ragged", "n_lt256",
                "n_eq256", "n_gt256_ragged", "e_not_quad", "tiny_plane", "all_ignored", "ignore_in_range") + L.NORMS + L.DATA:
        assert any(cat in c for c in both), cat


def test_restated_plans_are_the_planners():
    """bn_slab_plan and plan_loss_op restated in fuzz_step give the planner's own grids on every case of the lists."""
    for key in BN_LISTS:
        for (shape, forced, kind) in bn_list(key):
            B, C, H, W = shape
            slab, ns = F.bn_slab_plan(C, B * H * W, forced)
            assert (slab, ns) == R.slab_plan(C, B * H * W, forced)
            plan = rtc_mod.explain_plan(bn_bck_sums_func_op(R.dims_of(shape), forced))
            assert plan.startswith(f"bodahip_bn_sum grid={C * ns} block=256 -DMODE=2 ") and plan.endswith(f"slab={slab} slabs={ns}"), (shape, forced, plan)
            assert rtc_mod.explain_plan(bnf_bck_func_op(R.dims_of(shape), forced)).startswith(f"bodahip_bn_sum grid={C * ns} block=256 -DMODE=2 -DDX=1 ")
            assert rtc_mod.explain_plan(bn_stats_func_op(R.dims_of(shape), R.EPS, R.MAF, forced)).startswith(f"bodahip_bn_sum grid={C * ns} block=256 -DMODE=0 ")
    for key in LOSS_LISTS:
        for case in loss_list(key):
            shape = case[0]
            d, spec, pl = L.dims_of(shape), LossSpec(1.0, None, "valid"), F.loss_plan(shape)
            plan = rtc_mod.explain_plan(softmax_loss_fwd_func_op(d, spec))
            assert plan.startswith(f"bodahip_softmax_loss_fwd grid={pl['fwd'][0]} block=256 form={F.loss_form(shape)} -DCREG={pl['fwd'][1]} "), (shape, plan)
            assert rtc_mod.explain_plan(loss_norm_func_op(d, spec)).startswith("bodahip_loss_norm grid=1 block=256 ")
            assert rtc_mod.explain_plan(softmax_loss_bck_func_op(d, spec)).startswith(f"bodahip_softmax_loss_bck grid={pl['bck'][0]} block=256 "), shape


# ---- every check on be=cpu, on the GPU's cases
@pytest.mark.parametrize("key", list(BN_LISTS))
def test_cpu_bn(cpu, key):
    for i, case in enumerate(bn_list(key)):
        check_bn_case(cpu, None, case, data_seed(key, i), inplace=i in INPLACE[key])


@pytest.mark.parametrize("key", list(BN_LISTS))
def test_cpu_bnf(cpu, key):
    for i, case in enumerate(bn_list(key)):
        check_bnf_case(cpu, None, case, data_seed(key, i))


def test_cpu_bnc(cpu):
    for i, case in enumerate(bnc_list()):
        check_bnc_case(cpu, None, case, data_seed("bnc", i))


@pytest.mark.parametrize("key", list(LOSS_LISTS))
def test_cpu_loss(cpu, key):
    for i, case in enumerate(loss_list(key)):
        check_loss_case(cpu, None, case)


def test_cpu_solver(cpu):
    cases = solver_list()
    count = {cat: sum(1 for c in cases if cat in F.solver_categories(c)) for cat in F.SOLVER_WANTS + ["drawn_size"]}
    print("solver", count)
    assert len(cases) == N and all(v >= 1 for v in count.values()), count
    for i, case in enumerate(cases):
        assert all(m in F.SOLVER_MULTS for m in case[1] + case[2]) and 1 <= len(case[0]) <= 32
        check_solver_case(cpu, None, case, data_seed("solver", i))


def test_cpu_norm(cpu):
    cases = norm_list()
    count = {cat: sum(1 for c in cases if cat in F.norm_categories(c)) for cat in ["parts_gt256", "calls2", "tensor_chunks2"] + ["clip_" + k for k in F.NORM_CLIPS]}
    print("norm", count)
    assert len(cases) == N and all(v >= 1 for v in count.values()), count
    assert all(len(sz) <= 32 for c in cases for _, sz in c[0])
    assert any({"parts_gt256", "clip_" + k} <= F.norm_categories(c) for c in cases for k in ("above", "equal"))
    for i, case in enumerate(cases):
        check_norm_case(cpu, None, case, data_seed("norm", i))


def test_cpu_eval(cpu):
    al, ul, fl = acc_list(), accum_list(), fold_list()
    count = {cat: sum(1 for c in al if cat in F.acc_categories(c)) for cat in F.ACC_WANTS + ["invalid"]}
    count.update({cat: sum(1 for c in ul if cat in F.accum_categories(c)) for cat in F.ACCUM_WANTS})
    print("eval", count)
    assert len(al) == len(ul) == len(fl) == N and all(v >= 1 for v in count.values()), count
    assert all(1 <= B <= 40 and 1 <= C <= 1100 for B, C, _, _ in al) and all(1 <= C <= 600 for C, _ in fl) and {1, 255, 256, 257} <= {C for C, _ in fl}
    ties = 0
    for case in al:
        x, lab = F.acc_data(case)
        assert set(np.unique(x.view(np.uint32))) <= set(np.array(F.ACC_VALUES, np.float32).view(np.uint32))
        ties += int(np.count_nonzero(E.accuracy_np(x, lab)[(lab.reshape(-1) >= 0) & (lab.reshape(-1) < case[1])] > 0))
        check_acc_case(cpu, None, case)
    assert ties > 20   # ties are the rule: a true class that is not alone at the top
    for case in ul:
        check_accum_case(cpu, None, case)
    for case in fl:
        check_fold_case(cpu, None, case)


def test_cpu_data(cpu):
    cases = data_list()
    count = {cat: sum(1 for c in cases if cat in F.data_categories(c)) for cat in F.DATA_WANTS + ["mirror_clamped", "chan_mean", "wgs2"]}
    print("data", count)
    assert len(cases) == N and all(v >= 1 for v in count.values()) and count["mirror_clamped"] == N, count
    words = {int(r[2]) for c in cases for p in F.data_plans(c) for r in p}
    assert words == set(F.DATA_MIRRORS) and F.DATA_SCALES == D.SCALES
    for c in cases:
        H, W = c["ch"] + c["dh"], c["cw"] + c["dw"]
        assert 1 <= H <= 40 and 1 <= W <= 40 and c["chan"] in (1, 3, 4) and 1 <= c["B"] <= 5 and c["scale"] in D.SCALES
        offs = {int(r[1]) for p in F.data_plans(c) for r in p}
        assert any(o > c["dw"] for o in offs)   # an x offset beyond the clamp
        check_data_case(cpu, None, c)


def test_zz_report_worst_fractions_of_the_bounds():
    """Not a check of its own: prints what the sweeps above measured on be=cpu (run with -s)."""
    for name in sorted(WORST):
        print(f"largest observed fraction of the bound on be=cpu, {name}: {WORST[name]:.3f}")
    assert all(v <= 1.0 for v in WORST.values())
